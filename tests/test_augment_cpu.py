"""CPU-only checks of the training augmentation (random resized crop, flip, normalize, erase): data.TrainAugment's
draws against torchvision's / timm's rules, the host path against Pillow's crop().resize(), host_transform unchanged
without mean / std, the wrapper's table validation (it precedes every upload, so it is tested here without a GPU),
train.py's flags on the host path, and tests/host_abi_aug_check.c (the argument checks of vit_augment_to_tensor, ABI
still 18)."""
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from VisionTransformer import _lib, _ops, data
from VisionTransformer.data import AugTable, TrainAugment

PIL = pytest.importorskip("PIL.Image")
Image = PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20_000
SOURCES = [(32, 32), (375, 500), (1000, 30), (2, 300), (5, 5), (1, 1)]        # (H, W)
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _img(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)
    return a[:, :, 0] if c == 1 else a


# ---- sampler --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crop_draws():
    """20,000 crop draws per source: {(H, W): int array [N, 5] = (x0, y0, cw, ch, fallback)}."""
    out = {}
    for k, (H, W) in enumerate(SOURCES):
        aug = TrainAugment(seed=k, rank=0)
        out[(H, W)] = np.array([aug.crop_box(H, W) for _ in range(N)], dtype=np.int64)
    return out


@pytest.mark.parametrize("hw", SOURCES)
def test_crop_boxes_lie_inside_their_image(crop_draws, hw):
    H, W = hw
    x0, y0, cw, ch, _ = crop_draws[hw].T
    assert (cw >= 1).all() and (ch >= 1).all()
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x0 + cw <= W).all() and (y0 + ch <= H).all()


def test_crop_fallback_and_area(crop_draws):
    x0, y0, cw, ch, fb = crop_draws[(32, 32)].T
    assert not fb.any()                                   # a square source always accepts within 10 attempts
    frac = cw * ch / (32 * 32)
    assert frac.min() >= 0.078 and frac.max() <= 1.0      # scale (0.08, 1) up to the rounding of w and h
    assert len(np.unique(x0)) > 10 and len(np.unique(y0)) > 10
    # no box of aspect within (3/4, 4/3) fits these: every draw is the central fallback, the aspect clamped into ratio
    for hw, box in (((1000, 30), (0, 480, 30, 40)), ((2, 300), (148, 0, 3, 2))):
        d = crop_draws[hw]
        assert d[:, 4].all()
        assert (d[:, :4] == np.array(box)).all(), (hw, d[0])
    assert crop_draws[(375, 500)][:, 4].mean() < 1e-3     # 5e-5 by the rule's own arithmetic
    assert not crop_draws[(5, 5)][:, 4].any()


def test_draw_is_reproducible_per_seed_and_rank():
    meta = np.array([[0, 375, 500, 3], [1, 32, 32, 3], [2, 97, 131, 4]] * 8, dtype=np.int64)
    kw = dict(erase_prob=0.5, seed=7)
    a = TrainAugment(rank=0, **kw).draw(meta, 224, 224)
    b = TrainAugment(rank=0, **kw).draw(meta, 224, 224)
    c = TrainAugment(rank=1, **kw).draw(meta, 224, 224)
    d = TrainAugment(rank=0, erase_prob=0.5, seed=8).draw(meta, 224, 224)
    assert isinstance(a, AugTable) and all(col.dtype == np.int32 and col.shape == (24,) for col in a)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert any(not np.array_equal(p, q) for p, q in zip(a, c))
    assert any(not np.array_equal(p, q) for p, q in zip(a, d))
    # a torch meta (what the loader yields) gives the same table
    e = TrainAugment(rank=0, **kw).draw(torch.from_numpy(meta), 224, 224)
    assert all(np.array_equal(p, q) for p, q in zip(a, e))


def test_flip_and_erase_rates_and_erase_boxes():
    meta = np.array([[0, 64, 64, 3]] * N, dtype=np.int64)
    for hflip, ep in ((0.5, 0.25), (0.2, 0.7)):
        t = TrainAugment(hflip=hflip, erase_prob=ep, seed=11, rank=0).draw(meta, 224, 224)
        assert set(np.unique(t.flip)) <= {0, 1}
        boxed = (t.ey1 > t.ey0) & (t.ex1 > t.ex0)
        for rate, p in ((t.flip.mean(), hflip), (boxed.mean(), ep)):
            assert abs(rate - p) <= 4 * math.sqrt(p * (1 - p) / N), (rate, p)
        # strictly inside the output: never a whole axis (timm accepts h < H and w < W only)
        assert (t.ey0 >= 0).all() and (t.ey1 <= 224).all() and (t.ex0 >= 0).all() and (t.ex1 <= 224).all()
        assert ((t.ey1 - t.ey0) < 224).all() and ((t.ex1 - t.ex0) < 224).all()
        area = ((t.ey1 - t.ey0) * (t.ex1 - t.ex0))[boxed] / 224 ** 2
        assert 0.015 < area.min() and area.max() < 0.35           # erase_scale (0.02, 1/3) up to rounding
        assert ((~boxed) == ((t.ey0 == 0) & (t.ey1 == 0) & (t.ex0 == 0) & (t.ex1 == 0))).all()
    t = TrainAugment(hflip=0.0, erase_prob=0.0, seed=1, rank=0).draw(meta[:100], 224, 224)
    assert not t.flip.any() and not t.ey1.any() and not t.ex1.any()
    assert TrainAugment(hflip=1.0, seed=1, rank=0).draw(meta[:100], 8, 8).flip.all()


def test_scale_none_gives_full_boxes_and_bad_arguments_raise():
    meta = np.array([[0, h, w, 3] for h, w in SOURCES], dtype=np.int64)
    t = TrainAugment(scale=None, hflip=0.0, seed=2, rank=0).draw(meta, 64, 48)
    ident = data.identity_table(meta)
    assert all(np.array_equal(p, q) for p, q in zip(t, ident))
    assert ident.cw.tolist() == [w for _, w in SOURCES] and ident.ch.tolist() == [h for h, _ in SOURCES]
    for kw in (dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.2)), dict(scale=(0.5, 1.5)), dict(ratio=(0.0, 1.0)),
               dict(hflip=1.5), dict(erase_prob=-0.1), dict(erase_value=float("nan")), dict(erase_scale=(0.5, 2.0))):
        with pytest.raises(ValueError, match="TrainAugment"):
            TrainAugment(rank=0, **kw)


# ---- host path ------------------------------------------------------------------------------------------------------
def _pil_aug_ref(a, size, row, mean=None, std=None, erase_value=0.0):
    """crop().resize() + transpose(FLIP_LEFT_RIGHT) + ToTensor + torch normalize + fill, written out."""
    sh, sw = size
    x0, y0, cw, ch, flip, ey0, ey1, ex0, ex1 = row
    c = 1 if a.ndim == 2 else a.shape[2]
    im = Image.fromarray(a, mode=MODES[c]).convert("RGB").crop((x0, y0, x0 + cw, y0 + ch))
    im = im.resize((sw, sh), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.asarray(im, dtype=np.uint8).astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)
    if mean is not None:
        x = (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    x = x.clone()
    x[:, ey0:ey1, ex0:ex1] = erase_value
    return x


HOST_ROWS = [  # (H, W, C), table row
    ((97, 131, 4), (10, 20, 60, 70, 0, 0, 0, 0, 0)),
    ((97, 131, 4), (71, 27, 60, 70, 1, 3, 20, 5, 40)),            # touches the right and bottom edges, flipped, erased
    ((17, 45, 1), (44, 16, 1, 1, 1, 0, 1, 0, 1)),
    ((300, 200, 3), (0, 150, 200, 1, 0, 63, 64, 47, 48)),
    ((5, 5, 3), (0, 0, 5, 5, 1, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("norm", [None, IMAGENET])
def test_host_train_transform_equals_pillow_crop_resize(monkeypatch, norm):
    mean, std = norm if norm else (None, None)
    aug = TrainAugment(erase_value=-1.5, seed=0, rank=0)
    tf = data.host_train_transform((64, 48), aug, mean, std)
    for k, (shape, row) in enumerate(HOST_ROWS):
        a = _img(*shape, seed=k)
        monkeypatch.setattr(aug, "draw", lambda meta, oh, ow, row=row: AugTable(*(np.array([v], np.int32) for v in row)))
        got = tf(a)
        want = _pil_aug_ref(a, (64, 48), row, mean, std, erase_value=-1.5)
        assert got.dtype == torch.float32 and got.shape == (3, 64, 48)
        assert torch.equal(got, want), (shape, row)
        if row[5:] != (0, 0, 0, 0):
            assert (got[:, row[5]:row[6], row[7]:row[8]] == -1.5).all()
    # crop-then-resize is not resize(box=): the taps are clamped to the crop (the case the kernel test relies on)
    a = _img(97, 131, 4, seed=0)
    im = Image.fromarray(a, mode="RGBA").convert("RGB")
    boxed = np.asarray(im.resize((64, 64), Image.BILINEAR, box=(10, 20, 70, 90)))
    cropped = np.asarray(im.crop((10, 20, 70, 90)).resize((64, 64), Image.BILINEAR))
    assert (boxed != cropped).sum() > 100
    # a table outside the image is refused on the host path too
    monkeypatch.setattr(aug, "draw", lambda *_: AugTable(*(np.array([v], np.int32) for v in (0, 0, 132, 5, 0, 0, 0, 0, 0))))
    with pytest.raises(ValueError, match="augment table"):
        tf(a)


def test_host_train_transform_draws_differ_and_repeat_per_seed():
    a = _img(40, 50, 3, seed=3)
    runs = []
    for _ in range(2):
        tf = data.host_train_transform(32, TrainAugment(erase_prob=0.5, seed=5, rank=0))
        runs.append(torch.stack([tf(a) for _ in range(6)]))
    assert torch.equal(runs[0], runs[1])
    assert not torch.equal(runs[0][0], runs[0][1])
    other = data.host_train_transform(32, TrainAugment(erase_prob=0.5, seed=5, rank=1))
    assert not torch.equal(runs[0][0], other(a))


def test_host_train_transform_reseeds_per_worker(monkeypatch):
    """In a DataLoader worker the stream restarts from [seed, rank, worker id, the worker's seed]."""
    import collections
    Info = collections.namedtuple("Info", "id seed")
    a = _img(40, 50, 3, seed=3)
    outs = {}
    for wid in (0, 1):
        monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda wid=wid: Info(wid, 1234567890123 + wid))
        aug = TrainAugment(seed=5, rank=0)
        tf = data.host_train_transform(32, aug)
        outs[wid] = torch.stack([tf(a) for _ in range(3)])
        want = TrainAugment(seed=5, rank=0)
        want.reseed(wid, 1234567890123 + wid)
        monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: None)
        ref = data.host_train_transform(32, want)
        assert torch.equal(outs[wid], torch.stack([ref(a) for _ in range(3)]))
    assert not torch.equal(outs[0], outs[1])


CASES = [  # tests/test_image_pipeline.py's
    (32, 32, 3, 224, 224), (32, 32, 3, 256, 256), (300, 200, 3, 64, 64), (17, 45, 1, 224, 224),
    (97, 131, 4, 50, 333), (512, 512, 3, 224, 224), (64, 64, 3, 64, 64), (1000, 30, 2, 7, 99), (5, 5, 3, 256, 256),
    (224, 100, 3, 224, 224),
]


@pytest.mark.parametrize("case", CASES)
def test_host_transform_without_mean_is_unchanged(case):
    h, w, c, oh, ow = case
    a = _img(h, w, c, seed=h * 7 + w)
    im = Image.fromarray(a, mode=MODES[c]).convert("RGB")
    ref = (np.asarray(im.resize((ow, oh), Image.BILINEAR), dtype=np.uint8).astype(np.float32) / np.float32(255.0))
    ref = torch.from_numpy(ref.transpose(2, 0, 1).copy())
    got = data.host_transform((oh, ow))(Image.fromarray(a, mode=MODES[c]))
    assert torch.equal(got, ref) and got.is_contiguous()
    mean, std = IMAGENET
    gotn = data.host_transform((oh, ow), mean=mean, std=std)(a)
    assert torch.equal(gotn, (ref - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))
    with pytest.raises(TypeError):
        data.host_transform((oh, ow), mean, std)              # keyword-only
    with pytest.raises(ValueError, match="normalize"):
        data.host_transform((oh, ow), mean=mean)


# ---- wrapper --------------------------------------------------------------------------------------------------------
class _FixedAugment:
    erase_value = 0.0

    def __init__(self, table):
        self.table = table

    def draw(self, meta, oh, ow):
        return self.table


def test_wrapper_validates_the_table_before_any_upload(monkeypatch):
    items = [(_img(20, 30, 3, 1), 0), (_img(8, 9, 1, 2), 1)]
    packed, meta, _ = data.collate_raw(items)
    good = [list(c) for c in data.identity_table(meta)]
    uploads = []

    class UploadReached(Exception):
        pass

    def no_upload(*a, **k):
        uploads.append(a)
        raise UploadReached
    monkeypatch.setattr(_ops, "aug_table_host", no_upload)
    monkeypatch.setattr(torch.cuda, "current_stream", no_upload)

    def bad(col, row, value):
        t = [list(c) for c in good]
        t[col][row] = value
        return AugTable(*t)
    cases = [bad(2, 0, 0), bad(3, 1, 0), bad(2, 0, 31), bad(0, 0, 1), bad(1, 1, 1), bad(0, 1, -1), bad(1, 0, -3),
             bad(3, 0, 21), bad(4, 0, 2), bad(6, 0, 65), bad(5, 1, -1), bad(8, 1, 49), bad(7, 0, 5),
             AugTable(*[c[:1] for c in good])]
    for t in cases:
        with pytest.raises(ValueError, match="augment table"):
            data.GpuTrainTransform((64, 48), _FixedAugment(t))(packed, meta, device="cpu")
    assert uploads == []
    # a good table gets past the validation, to the first device work; and the meta checks come first
    with pytest.raises(UploadReached):
        data.GpuTrainTransform((64, 48), _FixedAugment(AugTable(*good)))(packed, meta, device="cpu")
    assert len(uploads) == 1
    with pytest.raises(ValueError, match="outside the packed buffer"):
        data.GpuTrainTransform(64, _FixedAugment(AugTable(*good)))(packed[:-1], meta, device="cpu")
    for kw in (dict(mean=(0.5,) * 3), dict(mean=(0.5,) * 3, std=(0.5, 0.0, 0.5)),
               dict(mean=(float("inf"),) * 3, std=(0.5,) * 3), dict(mean=(0.5,) * 2, std=(0.5,) * 2)):
        with pytest.raises(ValueError, match="normalize"):
            data.GpuTrainTransform(64, TrainAugment(rank=0), **kw)
        with pytest.raises(ValueError, match="normalize"):
            data.GpuImageTransform(64, **kw)
    with pytest.raises(TypeError):
        data.GpuImageTransform(64, torch.float32, (0.5,) * 3, (0.5,) * 3)     # keyword-only


def test_table_layout_and_ksize():
    t = AugTable(*(np.array([v, v + 10], np.int32) for v in range(1, 10)))
    host = _ops.aug_table_host(t)
    assert host.dtype == torch.uint8 and host.numel() == 2 * 36 == 2 * _ops.AUG_ITEM_BYTES
    raw = np.frombuffer(host.numpy().tobytes(), dtype=np.int32).reshape(2, 9)
    assert raw.tolist() == [list(range(1, 10)), list(range(11, 20))]
    assert _ops.AUG_COLUMNS == AugTable._fields == tuple(n for n, _ in _lib.AugItem._fields_)
    lib = _lib.load()
    assert _ops.aug_ksize([32, 500], [32, 375], 224, 224) == lib.vit_resize_ksize(500, 224) == 7
    assert _ops.aug_ksize([32], [32], 224, 224) == 3


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_stays_18_with_the_augment_exports():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.vit_abi_version() == 18
    assert {"vit_augment_workspace_bytes", "vit_augment_to_tensor"} <= set(_lib.EXPORTED_SYMBOLS)
    assert hasattr(lib, "vit_augment_to_tensor") and hasattr(lib, "vit_augment_workspace_bytes")
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "#define VIT_ABI_VERSION 18" in hdr and "} vit_aug_item; /* 36 bytes */" in hdr
    for name, v in (("ROWS", _lib.AUG_TILE_ROWS), ("COLS", _lib.AUG_TILE_COLS), ("MAX_SPAN", _lib.AUG_TILE_MAX_SPAN)):
        assert f"#define VIT_AUG_TILE_{name} {v}\n" in hdr
    assert _lib.get_option("augment_path") == 0
    with _lib.option("augment_path", 2):
        assert _lib.get_option("augment_path") == 2
    assert _lib.get_option("augment_path") == 0


def test_host_abi_aug_checker_c(tmp_path):
    """tests/host_abi_aug_check.c (gcc, no GPU): sizeof(vit_aug_item), every refusal of vit_augment_to_tensor with a
    vit_last_error() message naming it, vit_augment_workspace_bytes monotone, and ABI 18."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_aug_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_aug_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


# ---- train.py on the host path --------------------------------------------------------------------------------------
def _run_train(monkeypatch, tmp_path, extra):
    import train as T
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    threads = torch.get_num_threads()
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "2",
                                      "--steps", "2", "--epochs", "0", "--train-size", "4", "--test-size", "2",
                                      "--workers", "0", "--threads", "2", "--log-dir", logs, "--checkpoint-dir", ck,
                                      *extra])
    try:
        T.main()
    finally:
        torch.set_num_threads(threads)
    return logs


def test_train_main_augmentation_flags_on_cpu(tmp_path, monkeypatch):
    seen = {}
    real = data.host_train_transform

    def spy(size, augment, mean=None, std=None):
        seen.update(size=size, augment=augment, mean=mean, std=std)
        return real(size, augment, mean, std)
    monkeypatch.setattr(data, "host_train_transform", spy)
    logs = _run_train(monkeypatch, tmp_path, ["--data", "synthetic-u8", "--random-resized-crop", "--crop-scale", "0.3",
                                              "1.0", "--hflip", "0.5", "--random-erase", "0.25", "--mean", "0.5", "0.5",
                                              "0.5", "--std", "0.25", "0.25", "0.25", "--mixup", "0.8"])
    losses = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    losses = [r["value"] for r in losses if r["tag"] == "Loss/train_batch"]
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    aug = seen["augment"]
    assert seen["size"] == 32 and seen["mean"] == [0.5] * 3 and seen["std"] == [0.25] * 3
    assert aug.scale == (0.3, 1.0) and aug.hflip == 0.5 and aug.erase_prob == 0.25 and aug.erase_value == 0.0


def test_train_main_flip_only_keeps_the_full_image(tmp_path, monkeypatch):
    seen = {}
    real = data.host_train_transform
    monkeypatch.setattr(data, "host_train_transform",
                        lambda size, augment, mean=None, std=None: seen.update(a=augment) or real(size, augment, mean, std))
    _run_train(monkeypatch, tmp_path, ["--data", "synthetic-u8", "--hflip", "1.0"])
    assert seen["a"].scale is None and seen["a"].hflip == 1.0


@pytest.mark.parametrize("flags", [["--random-resized-crop"], ["--hflip", "0.5"], ["--random-erase", "0.1"],
                                   ["--mean", "0.5", "0.5", "0.5", "--std", "0.5", "0.5", "0.5"]])
def test_train_main_refuses_augmentation_of_synthetic_floats(tmp_path, monkeypatch, capsys, flags):
    with pytest.raises(SystemExit):
        _run_train(monkeypatch, tmp_path, ["--data", "synthetic", *flags])
    assert "--data synthetic feeds float tensors" in capsys.readouterr().err
