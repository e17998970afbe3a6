"""CPU-only checks of RandAugment (data.RandAugment, the host path, the table checks): the config strings, the level
functions against the values the policy states, the draws (deterministic per seed and rank, a stream apart from
TrainAugment's), host_train_transform(..., rand_augment=...) against Pillow's own calls composed here from the drawn
tables, the unchanged output without it, _ops.check_ra_table and the device table's layout, train.py's flag on the host
path, and tests/host_abi_randaug_check.c (struct layout and refusals of the entry points, ABI still 18)."""
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
from VisionTransformer.data import RA_OPS, RandAugment, RaTable, TrainAugment

PIL = pytest.importorskip("PIL.Image")
Image = PIL
from PIL import ImageEnhance, ImageOps      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FILL = (128, 128, 128)


def _img(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)
    return a[:, :, 0] if c == 1 else a


# ---- config strings -------------------------------------------------------------------------------------------------
def test_from_config_parses_every_key():
    ra = RandAugment.from_config("rand-m9-mstd0.5-inc1", rank=0)
    assert (ra.magnitude, ra.magnitude_std, ra.increasing, ra.num_layers, ra.prob) == (9.0, 0.5, True, 2, 0.5)
    ra = RandAugment.from_config("rand-m7.5-n3-mstd1-inc0-p0.25", seed=4, rank=1, fill=(1, 2, 3))
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.increasing, ra.prob) == (7.5, 3, 1.0, False, 0.25)
    assert (ra.seed, ra.rank, ra.fill) == (4, 1, (1, 2, 3))
    assert RandAugment.from_config("rand-mstd100", rank=0).magnitude_std == float("inf")
    assert RandAugment.from_config("rand-mstd101.5", rank=0).magnitude_std == float("inf")
    assert RandAugment.from_config("rand-mstd99", rank=0).magnitude_std == 99.0
    # a key the string leaves out has timm's default for the string form
    ra = RandAugment.from_config("rand", rank=0)
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.increasing, ra.prob) == (10.0, 2, 0.0, False, 0.5)
    assert RandAugment.from_config("rand-n4", rank=0).num_layers == _lib.RA_MAX_LAYERS == 4
    assert ra.ops == RA_OPS[1:] and len(ra.ops) == 15 and ra.translate_pct == 0.45 and ra.fill == FILL


@pytest.mark.parametrize("bad", ["", "augmix-m9", "rand-w0", "rand-m9-w1", "rand-x3", "rand-m", "rand-mnine", "rand-n5",
                                 "rand-n0", "rand-n1.5", "rand-m11", "rand-p1.5", "rand-inc2", "rand--m9", "rand-m9-"])
def test_from_config_refuses_bad_strings(bad):
    with pytest.raises(ValueError, match="RandAugment"):
        RandAugment.from_config(bad, rank=0)


def test_constructor_refusals():
    for kw in (dict(num_layers=0), dict(num_layers=5), dict(magnitude=-1), dict(magnitude=10.5), dict(magnitude_std=-0.1),
               dict(prob=1.1), dict(translate_pct=2.0), dict(fill=(1, 2)), dict(fill=(0, 0, 256)), dict(ops=()),
               dict(ops=("Rotate", "Blur"))):
        with pytest.raises(ValueError, match="RandAugment"):
            RandAugment(rank=0, **kw)
    assert RandAugment(ops=("Rotate", "Invert"), rank=0).ops == ("Rotate", "Invert")


# ---- level functions ------------------------------------------------------------------------------------------------
def test_level_functions_at_magnitudes_0_9_10():
    inc, flat = RandAugment(increasing=True, rank=0), RandAugment(increasing=False, rank=0)
    close = lambda a, b: abs(a - b) <= 1e-12      # noqa: E731
    for ra in (inc, flat):
        for neg, s in ((False, 1.0), (True, -1.0)):
            for mag, L in ((0.0, 0.0), (9.0, 0.9), (10.0, 1.0)):
                assert close(ra.level_arg("Rotate", mag, neg), s * 30 * L)
                assert close(ra.level_arg("ShearX", mag, neg), s * 0.3 * L)
                assert close(ra.level_arg("ShearY", mag, neg), s * 0.3 * L)
                assert close(ra.level_arg("TranslateXRel", mag, neg), s * 0.45 * L)
                assert close(ra.level_arg("TranslateYRel", mag, neg), s * 0.45 * L)
                for name in ("AutoContrast", "Equalize", "Invert"):
                    assert ra.level_arg(name, mag, neg) == 0.0
                assert ra.level_arg("SolarizeAdd", mag, neg) == {0.0: 0, 9.0: 99, 10.0: 110}[mag]
    # the values the policy's description lists at mag = 9
    assert close(inc.level_arg("Rotate", 9.0), 27.0) and close(inc.level_arg("Rotate", 9.0, True), -27.0)
    assert close(inc.level_arg("ShearX", 9.0, True), -0.27) and close(inc.level_arg("TranslateYRel", 9.0), 0.405)
    for name in ("Color", "Contrast", "Brightness", "Sharpness"):
        assert close(inc.level_arg(name, 9.0), 1.81) and close(inc.level_arg(name, 9.0, True), 0.19)
        assert close(inc.level_arg(name, 0.0), 1.0) and close(inc.level_arg(name, 0.0, True), 1.0)
        assert close(inc.level_arg(name, 10.0), 1.9) and close(inc.level_arg(name, 10.0, True), 0.1)
        for neg in (False, True):       # not increasing: no sign
            assert close(flat.level_arg(name, 0.0, neg), 0.1) and close(flat.level_arg(name, 9.0, neg), 1.72)
            assert close(flat.level_arg(name, 10.0, neg), 1.9)
        assert inc.negates(name) and not flat.negates(name)
    assert [inc.level_arg("Posterize", m) for m in (0.0, 9.0, 10.0)] == [4, 1, 0]
    assert [flat.level_arg("Posterize", m) for m in (0.0, 9.0, 10.0)] == [0, 3, 4]
    assert [inc.level_arg("Solarize", m) for m in (0.0, 9.0, 10.0)] == [256, 26, 0]
    assert [flat.level_arg("Solarize", m) for m in (0.0, 9.0, 10.0)] == [0, 230, 256]
    assert inc.negates("Rotate") and flat.negates("TranslateXRel") and not inc.negates("Solarize")
    with pytest.raises(ValueError, match="RandAugment"):
        inc.level_arg("Blur", 5.0)


def test_rotate_coefficients_are_pillows(monkeypatch):
    """RandAugment.coefficients("Rotate", ...) is the matrix Image.rotate hands to Image.transform."""
    seen = []
    real = Image.Image.transform
    monkeypatch.setattr(Image.Image, "transform", lambda self, size, method, data=None, *a, **k:
                        seen.append((size, method, tuple(data))) or real(self, size, method, data, *a, **k))
    for (h, w) in ((32, 32), (17, 23), (1, 1), (224, 224)):
        im = Image.fromarray(_img(h, w, 3, 1))
        for deg in (27.0, -27.0, 17.3, -30.0, 1e-3):
            seen.clear()
            im.rotate(deg, resample=Image.BILINEAR, fillcolor=FILL)
            assert seen == [((w, h), Image.AFFINE, RandAugment.coefficients("Rotate", deg, h, w))]
    assert RandAugment.coefficients("Rotate", 0.0, 5, 7) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    assert RandAugment.coefficients("ShearX", 0.25, 5, 7) == (1.0, 0.25, 0.0, 0.0, 1.0, 0.0)
    assert RandAugment.coefficients("ShearY", -0.25, 5, 7) == (1.0, 0.0, 0.0, -0.25, 1.0, 0.0)
    assert RandAugment.coefficients("TranslateXRel", 3.5, 5, 7) == (1.0, 0.0, 3.5, 0.0, 1.0, 0.0)
    assert RandAugment.coefficients("TranslateYRel", -2.0, 5, 7) == (1.0, 0.0, 0.0, 0.0, 1.0, -2.0)
    with pytest.raises(ValueError, match="RandAugment"):
        RandAugment.coefficients("Rotate", 180.0, 5, 7)


# ---- draws ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def test_draws_are_deterministic_per_seed_and_rank():
    kw = dict(num_layers=3, seed=7)
    a = RandAugment(rank=0, **kw).draw(64, 224, 200)
    assert isinstance(a, RaTable) and a.op.dtype == np.int32 and a.op.shape == (64, 3)
    assert a.arg.shape == (64, 3) and a.coef.shape == (64, 3, 6) and a.arg.dtype == a.coef.dtype == np.float64
    assert _same(a, RandAugment(rank=0, **kw).draw(64, 224, 200))
    assert not _same(a, RandAugment(rank=1, **kw).draw(64, 224, 200))
    assert not _same(a, RandAugment(rank=0, num_layers=3, seed=8).draw(64, 224, 200))
    # a batch draw is the sequence of single draws (the host path draws per image), and reseed() restarts it
    ra = RandAugment(rank=0, **kw)
    singles = [ra.draw(1, 224, 200) for _ in range(64)]
    assert _same(a, RaTable(*(np.concatenate(c) for c in zip(*singles))))
    ra.reseed()
    assert _same(a, ra.draw(64, 224, 200))
    ra.reseed(3, 99)
    assert not _same(a, ra.draw(64, 224, 200))
    _ops.check_ra_table(a, 64)


def test_draw_statistics_and_arguments():
    N = 6000
    ra = RandAugment(num_layers=2, magnitude=9.0, magnitude_std=0.5, increasing=True, prob=0.5, seed=1, rank=0)
    t = ra.draw(N, 224, 160)
    none = t.op == 0
    assert abs(none.mean() - 0.5) <= 4 * math.sqrt(0.25 / (2 * N))
    counts = np.bincount(t.op[~none], minlength=16)[1:]
    assert (counts > 0).all() and counts.max() / counts.min() < 1.5          # uniform over the 15 ops
    ident = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    for k, name in enumerate(RA_OPS):
        sel = t.op == k
        arg, coef = t.arg[sel], t.coef[sel]
        if name == "Rotate":
            assert (np.abs(arg) <= 30.0).all() and (arg > 0).any() and (arg < 0).any()
            assert not (coef == ident).all(axis=1).any()
        elif name in ("ShearX", "ShearY"):
            assert (np.abs(arg) <= 0.3).all() and (arg > 0).any() and (arg < 0).any()
            assert (coef[:, 1 if name == "ShearX" else 3] == arg).all()
        elif name in ("TranslateXRel", "TranslateYRel"):
            size = 160 if name == "TranslateXRel" else 224
            assert (np.abs(arg) <= 0.45 * size).all() and np.abs(arg).max() > 0.3 * size
            assert (coef[:, 2 if name == "TranslateXRel" else 5] == arg).all()
        elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
            assert (arg >= 0.1).all() and (arg <= 1.9).all() and (arg > 1).any() and (arg < 1).any()
            assert (coef == ident).all()
        elif name == "Posterize":
            assert set(arg) <= {0.0, 1.0, 2.0, 3.0, 4.0}
        elif name == "Solarize":
            assert (arg == np.floor(arg)).all() and (arg >= 0).all() and (arg <= 256).all()
        elif name == "SolarizeAdd":
            assert (arg == np.floor(arg)).all() and (arg >= 0).all() and (arg <= 110).all()
        else:
            assert (arg == 0).all() and (coef == ident).all()
    # the magnitude: constant without a std, uniform(0, m) with an infinite one
    flat = RandAugment(magnitude=9.0, magnitude_std=0.0, prob=1.0, ops=("Rotate",), seed=2, rank=0).draw(200, 32, 32)
    assert set(np.round(np.abs(flat.arg.ravel()), 9)) == {27.0}
    uni = RandAugment(magnitude=10.0, magnitude_std=float("inf"), prob=1.0, ops=("SolarizeAdd",), seed=2, rank=0)
    u = uni.draw(2000, 32, 32).arg.ravel()
    assert u.min() < 10 and u.max() > 100 and abs(u.mean() - 55) < 4
    assert (RandAugment(prob=0.0, seed=3, rank=0).draw(50, 32, 32).op == 0).all()


def test_train_augment_stream_is_independent_of_rand_augment():
    """TrainAugment.draw returns the tables it always did whether or not a RandAugment of the same seed and rank exists
    and draws beside it."""
    meta = np.array([[0, 375, 500, 3], [1, 32, 32, 3], [2, 97, 131, 4]] * 8, dtype=np.int64)
    alone = TrainAugment(erase_prob=0.5, seed=7, rank=0)
    want = [alone.draw(meta, 224, 224) for _ in range(3)]
    aug, ra = TrainAugment(erase_prob=0.5, seed=7, rank=0), RandAugment(seed=7, rank=0)
    got = []
    for _ in range(3):
        ra.draw(24, 224, 224)
        got.append(aug.draw(meta, 224, 224))
        ra.draw(5, 224, 224)
    assert all(_same(a, b) for a, b in zip(want, got))
    # and the two streams are not the same stream
    a = np.random.default_rng([7, 0]).random(4)
    b = np.random.default_rng([7, 0, RandAugment.TAG]).random(4)
    assert not np.array_equal(a, b)


# ---- host path against Pillow ---------------------------------------------------------------------------------------
def _pillow_chain(im, ops, args, fill):
    """The chain in Pillow calls, written out from the table (nothing of the implementation under test is called)."""
    W, H = im.size
    for k, a in zip(ops, args):
        name = RA_OPS[int(k)]
        if name == "AutoContrast":
            im = ImageOps.autocontrast(im)
        elif name == "Equalize":
            im = ImageOps.equalize(im)
        elif name == "Invert":
            im = ImageOps.invert(im)
        elif name == "Rotate":
            im = im.rotate(a, resample=Image.BILINEAR, fillcolor=fill)
        elif name == "Posterize":
            im = ImageOps.posterize(im, int(a)) if int(a) < 8 else im
        elif name == "Solarize":
            im = ImageOps.solarize(im, int(a))
        elif name == "SolarizeAdd":
            im = im.point([min(255, i + int(a)) if i < 128 else i for i in range(256)] * 3)
        elif name == "Color":
            im = ImageEnhance.Color(im).enhance(a)
        elif name == "Contrast":
            im = ImageEnhance.Contrast(im).enhance(a)
        elif name == "Brightness":
            im = ImageEnhance.Brightness(im).enhance(a)
        elif name == "Sharpness":
            im = ImageEnhance.Sharpness(im).enhance(a)
        elif name == "ShearX":
            im = im.transform((W, H), Image.AFFINE, (1, a, 0, 0, 1, 0), resample=Image.BILINEAR, fillcolor=fill)
        elif name == "ShearY":
            im = im.transform((W, H), Image.AFFINE, (1, 0, 0, a, 1, 0), resample=Image.BILINEAR, fillcolor=fill)
        elif name == "TranslateXRel":
            im = im.transform((W, H), Image.AFFINE, (1, 0, a, 0, 1, 0), resample=Image.BILINEAR, fillcolor=fill)
        elif name == "TranslateYRel":
            im = im.transform((W, H), Image.AFFINE, (1, 0, 0, 0, 1, a), resample=Image.BILINEAR, fillcolor=fill)
        else:
            assert name == "None"
    return im


def _host_reference(a, size, row, ra_row, fill, mean, std, erase_value):
    sh, sw = size
    x0, y0, cw, ch, flip, ey0, ey1, ex0, ex1 = (int(v) for v in row)
    c = 1 if a.ndim == 2 else a.shape[2]
    im = Image.fromarray(a, mode=MODES[c]).convert("RGB").crop((x0, y0, x0 + cw, y0 + ch))
    im = im.resize((sw, sh), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = _pillow_chain(im, [int(k) for k in ra_row[0]], [float(v) for v in ra_row[1]], fill)
    x = torch.from_numpy(np.asarray(im, dtype=np.uint8).astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)
    if mean is not None:
        x = (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    x = x.clone()
    x[:, ey0:ey1, ex0:ex1] = erase_value
    return x


HOST_SOURCES = [(97, 131, 4), (17, 45, 1), (40, 33, 3), (300, 200, 3), (5, 5, 3), (64, 20, 2), (1, 1, 3)]   # ragged


@pytest.mark.parametrize("norm", [None, IMAGENET], ids=["plain", "imagenet"])
def test_host_path_equals_pillow_composed_from_the_tables(norm):
    """Ragged RGB, L, LA and RGBA sources through host_train_transform with a RandAugment: every image equals, with ==,
    the Pillow calls composed here from the tables that fresh objects of the same seeds draw."""
    mean, std = norm if norm else (None, None)
    size = (24, 19)
    mk = lambda: (TrainAugment(erase_prob=0.5, erase_value=-1.5, seed=3, rank=0),      # noqa: E731
                  RandAugment(num_layers=3, prob=0.8, fill=(10, 200, 30), seed=3, rank=0))
    aug, ra = mk()
    tf = data.host_train_transform(size, aug, mean, std, rand_augment=ra)
    aug2, ra2 = mk()
    seen = set()
    for rep in range(8):
        for k, shape in enumerate(HOST_SOURCES):
            a = _img(*shape, seed=10 * rep + k)
            src = Image.fromarray(a, mode=MODES[shape[2]]) if (rep + k) % 2 else a      # PIL images and arrays alike
            got = tf(src)
            t = aug2.draw(np.array([[0, shape[0], shape[1], 3]], dtype=np.int64), *size)
            r = ra2.draw(1, *size)
            want = _host_reference(a, size, [c[0] for c in t], (r.op[0], r.arg[0]), (10, 200, 30), mean, std, -1.5)
            assert got.dtype == torch.float32 and got.shape == (3, *size)
            assert torch.equal(got, want), (shape, r.op[0], r.arg[0])
            seen |= set(int(v) for v in r.op[0])
    assert seen == set(range(16))                       # every op, and None, took part


def test_apply_pil_every_op_at_its_extremes():
    """RandAugment.apply_pil, one op at a time at the ends and the middle of its range, against the Pillow call."""
    ra = RandAugment(rank=0)
    cases = {"AutoContrast": [0.0], "Equalize": [0.0], "Invert": [0.0], "None": [0.0],
             "Rotate": [30.0, -30.0, 0.0, 17.3], "Posterize": list(range(9)), "Solarize": [0, 128, 256],
             "SolarizeAdd": [0, 99, 128], "ShearX": [0.3, -0.3, 0.0], "ShearY": [0.3, -0.3, 0.0]}
    for name in ("Color", "Contrast", "Brightness", "Sharpness"):
        cases[name] = [0.1, 1.0, 1.9]
    for (h, w) in ((32, 32), (17, 23), (3, 5), (2, 2), (1, 1)):
        cases["TranslateXRel"] = [0.45 * w, -0.45 * w, 0.0]
        cases["TranslateYRel"] = [0.45 * h, -0.45 * h, 0.0]
        one = _img(h, w, 3, 2)
        one[:, :, 1] = 9
        for a in (_img(h, w, 3, 1), np.full((h, w, 3), 77, np.uint8), one, np.zeros((h, w, 3), np.uint8),
                  np.full((h, w, 3), 255, np.uint8)):
            im = Image.fromarray(a)
            for name, args in cases.items():
                for v in args:
                    got = ra.apply_pil(im, ([RA_OPS.index(name)], [v]))
                    want = _pillow_chain(im, [RA_OPS.index(name)], [v], FILL)
                    assert np.array_equal(np.asarray(got), np.asarray(want)), (h, w, name, v)
                    assert got.size == im.size and got.mode == "RGB"
    # posterize to 0 bits is black, to 8 bits and above the image itself
    im = Image.fromarray(_img(9, 9, 3, 5))
    assert not np.asarray(ra.apply_pil(im, ([5], [0]))).any()
    assert np.array_equal(np.asarray(ra.apply_pil(im, ([5, 5], [8, 11]))), np.asarray(im))


def test_host_path_without_rand_augment_is_unchanged():
    """rand_augment=None: bitwise the output of the transform as it was, with or without the keyword."""
    for k, shape in enumerate(HOST_SOURCES):
        a = _img(*shape, seed=k)
        outs = []
        for kw in ({}, {"rand_augment": None}):
            tf = data.host_train_transform((24, 19), TrainAugment(erase_prob=0.5, seed=5, rank=0), *IMAGENET, **kw)
            outs.append(torch.stack([tf(a) for _ in range(3)]))
        aug = TrainAugment(erase_prob=0.5, seed=5, rank=0)
        want = []
        for _ in range(3):
            t = aug.draw(np.array([[0, shape[0], shape[1], 3]], dtype=np.int64), 24, 19)
            want.append(_host_reference(a, (24, 19), [c[0] for c in t], ([], []), FILL, *IMAGENET, 0.0))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], torch.stack(want))


def test_host_path_reseeds_both_streams_per_worker(monkeypatch):
    import collections
    Info = collections.namedtuple("Info", "id seed")
    a = _img(40, 50, 3, seed=3)
    outs = {}
    for wid in (0, 1):
        monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda wid=wid: Info(wid, 1234567890123 + wid))
        tf = data.host_train_transform(32, TrainAugment(seed=5, rank=0), rand_augment=RandAugment(prob=1.0, seed=5, rank=0))
        outs[wid] = torch.stack([tf(a) for _ in range(3)])
        aug, ra = TrainAugment(seed=5, rank=0), RandAugment(prob=1.0, seed=5, rank=0)
        aug.reseed(wid, 1234567890123 + wid)
        ra.reseed(wid, 1234567890123 + wid)
        monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: None)
        ref = data.host_train_transform(32, aug, rand_augment=ra)
        assert torch.equal(outs[wid], torch.stack([ref(a) for _ in range(3)]))
    assert not torch.equal(outs[0], outs[1])


# ---- table checks and layout ----------------------------------------------------------------------------------------
def _table(B, L, op=0):
    coef = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (B, L, 1))
    return RaTable(np.full((B, L), op, np.int32), np.zeros((B, L)), coef)


def test_check_ra_table_refusals():
    good = _table(3, 4)
    out = _ops.check_ra_table(good, 3)
    assert isinstance(out, RaTable) and out.op.dtype == np.int32 and out.coef.dtype == np.float64
    with pytest.raises(ValueError, match="randaug table.*layers"):
        _ops.check_ra_table(_table(3, 5), 3)
    with pytest.raises(ValueError, match="randaug table.*layers"):
        _ops.check_ra_table(_table(3, 0), 3)
    for bad in (float("nan"), float("inf"), -float("inf")):
        t = _table(3, 2)
        t.coef[1, 1, 4] = bad
        with pytest.raises(ValueError, match="randaug table.*non-finite"):
            _ops.check_ra_table(t, 3)
        t = _table(3, 2)
        t.arg[2, 0] = bad
        with pytest.raises(ValueError, match="randaug table.*non-finite"):
            _ops.check_ra_table(t, 3)
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table(good, 4)                                          # another batch size
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table(RaTable(good.op, good.arg[:, :3], good.coef), 3)
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table(RaTable(good.op, good.arg, good.coef[:, :, :5]), 3)
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table(RaTable(good.op[0], good.arg[0], good.coef[0]), 3)
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table(RaTable(good.op.astype(np.float64), good.arg, good.coef), 3)
    with pytest.raises(ValueError, match="randaug table"):
        _ops.check_ra_table((good.op, good.arg), 3)
    for v in (-1, 16):
        with pytest.raises(ValueError, match="randaug table.*op"):
            _ops.check_ra_table(_table(3, 2, op=v), 3)


def test_wrapper_validates_both_tables_before_any_upload(monkeypatch):
    items = [(_img(20, 30, 3, 1), 0), (_img(8, 9, 1, 2), 1)]
    packed, meta, _ = data.collate_raw(items)
    uploads = []

    class UploadReached(Exception):
        pass

    def no_upload(*a, **k):
        uploads.append(a)
        raise UploadReached
    monkeypatch.setattr(_ops, "aug_table_host", no_upload)
    monkeypatch.setattr(_ops, "randaug_table_host", no_upload)
    monkeypatch.setattr(torch.cuda, "current_stream", no_upload)

    class Fixed:
        fill = FILL

        def __init__(self, t):
            self.t = t

        def draw(self, B, oh, ow):
            return self.t
    nan = _table(2, 2)
    nan.coef[0, 0, 2] = float("nan")
    for t in (nan, _table(2, 5), _table(3, 2)):
        with pytest.raises(ValueError, match="randaug table"):
            data.GpuTrainTransform((16, 12), TrainAugment(rank=0), rand_augment=Fixed(t))(packed, meta, device="cpu")
    assert uploads == []
    with pytest.raises(UploadReached):
        data.GpuTrainTransform((16, 12), TrainAugment(rank=0), rand_augment=Fixed(_table(2, 2)))(packed, meta,
                                                                                                  device="cpu")
    assert len(uploads) == 1


def test_device_table_layout_and_stats_mask():
    ra = RandAugment(rank=0)
    names = ["Posterize", "Solarize", "SolarizeAdd", "Color", "Rotate", "ShearX", "None", "Contrast"]
    args = [3, 26, 99, 1.81, 17.3, -0.27, 0.0, 0.19]
    op = np.array([[RA_OPS.index(n) for n in names[:4]], [RA_OPS.index(n) for n in names[4:]]], np.int32)
    arg = np.array([args[:4], args[4:]], np.float64)
    coef = np.array([[ra.coefficients(n, a, 20, 30) for n, a in zip(names[:4], args[:4])],
                     [ra.coefficients(n, a, 20, 30) for n, a in zip(names[4:], args[4:])]])
    t = _ops.check_ra_table((op, arg, coef), 2)
    host = _ops.randaug_table_host(t, fill=(1, 2, 3))
    assert host.dtype == torch.uint8 and host.numel() == 2 * 288 == 2 * _ops.RA_ITEM_BYTES
    raw = (_lib.RaItem * 2).from_buffer_copy(host.numpy().tobytes())
    kinds = [[raw[b].layer[l].kind for l in range(4)] for b in range(2)]
    assert kinds == [[_lib.RA_POSTERIZE, _lib.RA_SOLARIZE, _lib.RA_SOLARIZE_ADD, _lib.RA_COLOR],
                     [_lib.RA_AFFINE, _lib.RA_AFFINE, _lib.RA_NONE, _lib.RA_CONTRAST]]
    assert [raw[0].layer[l].iarg0 for l in range(3)] == [3, 26, 99] and raw[0].layer[2].iarg1 == 128
    assert raw[0].layer[3].farg == np.float32(1.81) and raw[1].layer[3].farg == np.float32(0.19)
    assert tuple(raw[1].layer[0].coef) == ra.coefficients("Rotate", 17.3, 20, 30)
    assert tuple(raw[1].layer[1].coef) == (1.0, -0.27, 0.0, 0.0, 1.0, 0.0)
    assert all(tuple(raw[b].layer[l].fill)[:3] == (1, 2, 3) for b in range(2) for l in range(4))
    assert _ops.ra_stats_layers(t) == 0b1000
    assert _ops.ra_stats_layers(_table(3, 2, op=RA_OPS.index("Equalize"))) == 0b11
    assert _ops.ra_stats_layers(_table(3, 4, op=RA_OPS.index("Rotate"))) == 0
    # a table of fewer layers leaves the rest NONE
    short = (_lib.RaItem * 1).from_buffer_copy(_ops.randaug_table_host(_table(1, 1, op=3)).numpy().tobytes())
    assert [short[0].layer[l].kind for l in range(4)] == [_lib.RA_INVERT, 0, 0, 0]
    assert set(_ops.RA_KIND) == set(RA_OPS) and max(_ops.RA_KIND.values()) == _lib.RA_KINDS - 1


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_stays_18_with_the_randaug_exports():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.vit_abi_version() == 18
    names = {"vit_augment_to_u8", "vit_randaug_workspace_bytes", "vit_randaug_to_tensor"}
    assert names <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in names)
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "#define VIT_ABI_VERSION 18" in hdr and "#define VIT_RA_MAX_LAYERS 4\n" in hdr
    assert "} vit_ra_layer; /* 72 bytes */" in hdr and "} vit_ra_item; /* 288 bytes */" in hdr
    for name in ("NONE", "AUTOCONTRAST", "EQUALIZE", "INVERT", "POSTERIZE", "SOLARIZE", "SOLARIZE_ADD", "COLOR",
                 "CONTRAST", "BRIGHTNESS", "SHARPNESS", "AFFINE", "KINDS"):
        assert f"  VIT_RA_{name} = {getattr(_lib, 'RA_' + name)}" in hdr
    # two pictures of the batch and one layer's tables; monotone
    need = lib.vit_randaug_workspace_bytes(8, 17, 23)
    assert need >= 2 * 8 * 17 * 23 * 3 + 8 * 768
    assert lib.vit_randaug_workspace_bytes(9, 17, 23) > need and lib.vit_randaug_workspace_bytes(0, 17, 23) < 0


def test_host_abi_randaug_checker_c(tmp_path):
    """tests/host_abi_randaug_check.c (gcc, no GPU): the layout of vit_ra_layer / vit_ra_item, every refusal of
    vit_augment_to_u8 and vit_randaug_to_tensor with a vit_last_error() message naming it, and ABI 18."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_randaug_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_randaug_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
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
                                      "--data", "synthetic-u8", *extra])
    try:
        T.main()
    finally:
        torch.set_num_threads(threads)
    return logs


def test_train_main_rand_augment_on_cpu(tmp_path, monkeypatch):
    seen = {}
    real = data.host_train_transform
    monkeypatch.setattr(data, "host_train_transform", lambda size, augment, mean=None, std=None, **kw:
                        seen.update(kw) or real(size, augment, mean, std, **kw))
    plain = []
    real_plain = data.host_transform
    monkeypatch.setattr(data, "host_transform", lambda *a, **k: plain.append((a, k)) or real_plain(*a, **k))
    logs = _run_train(monkeypatch, tmp_path, ["--hflip", "0.5", "--rand-augment", "rand-m9-mstd0.5-inc1"])
    losses = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    losses = [r["value"] for r in losses if r["tag"] == "Loss/train_batch"]
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    ra = seen["rand_augment"]
    assert isinstance(ra, RandAugment)
    assert (ra.magnitude, ra.magnitude_std, ra.increasing, ra.num_layers, ra.prob) == (9.0, 0.5, True, 2, 0.5)
    assert len(plain) == 1 and "rand_augment" not in plain[0][1]      # validation stays un-augmented


def test_train_main_without_rand_augment_calls_the_transform_as_before(tmp_path, monkeypatch):
    seen = []
    real = data.host_train_transform
    monkeypatch.setattr(data, "host_train_transform", lambda size, augment, mean=None, std=None, **kw:
                        seen.append(kw) or real(size, augment, mean, std, **kw))
    _run_train(monkeypatch, tmp_path, ["--hflip", "0.5"])
    assert seen == [{}]


@pytest.mark.parametrize("extra,msg", [(["--rand-augment", "rand-m9"], "--random-resized-crop, --hflip or --random-erase"),
                                       (["--hflip", "0.5", "--rand-augment", "rand-m9-w0"], "unknown key 'w'"),
                                       (["--hflip", "0.5", "--rand-augment", "augmix-m3"], "does not start with 'rand'")])
def test_train_main_refuses_bad_rand_augment_flags(tmp_path, monkeypatch, capsys, extra, msg):
    with pytest.raises(SystemExit):
        _run_train(monkeypatch, tmp_path, extra)
    assert msg in capsys.readouterr().err
