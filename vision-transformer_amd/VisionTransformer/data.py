"""Data path of the training loop — reference src/train.py:151-162 and src/BrainTumorDataset.py:10-39.

The reference decodes PIL images in 4 DataLoader workers and runs `Compose([convert('RGB'), Resize((S, S)),
ToTensor()])` on the host per image; its published run was loader-bound (~375 img/s).  Here the workers
only decode to raw uint8 HWC arrays and pack a batch into one byte buffer; the RGB conversion, the PIL-bilinear
resize and the /255 scaling run on the GPU in one kernel launch per batch (`vit_resize_to_tensor`, bit-exact with
Pillow), on a side stream one batch ahead of the training step.

  * `BrainTumorDataset(data_dir, train, test_size, transform, random_state)` — the reference's folder-per-class
    dataset with the same stratified split (BrainTumorDataset.py:10-32); `transform=None` returns the PIL image as
    the reference does, `transform=decode` returns the raw array for the GPU pipeline;
  * `CIFAR10Bin(root, train)` — CIFAR-10 from its binary distribution (cifar-10-batches-bin; no pickle, no network:
    the reference's `CIFAR10(download=True)` at train.py:157-159 cannot run offline);
  * `SyntheticRawImages` — deterministic uint8 images (optionally ragged sizes) for tests and benchmarks;
  * `collate_raw` / `raw_loader` — the packing collate and its DataLoader;
  * `GpuImageTransform(size)` — packed batch -> [B, 3, S, S] device tensor;
  * `DeviceBatches(loader, transform, device, mix=None)` — iterates (images on device, labels on device), prefetching
    the next batch's copy + transform (+ mix) on a side stream;
  * `BatchMix(mixup_alpha, cutmix_alpha, ...)` — mixup / CutMix of a batch in one kernel launch (`vit_mix_batch`),
    labels as `optim.MixedLabels` (not in the reference);
  * `host_transform(size)` — the same transform on the host with Pillow (the CPU path, train.py --device cpu);
  * `TrainAugment(...)` / `GpuTrainTransform(size, augment, ...)` — random resized crop, horizontal flip, normalize
    and constant erase inside the resize launch (`vit_augment_to_tensor`; not in the reference), and
    `host_train_transform(size, augment, ...)`, the same on the host;
  * `RandAugment(...)` / `RandAugment.from_config("rand-m9-mstd0.5-inc1")` — timm's policy augmentation between the
    flip and ToTensor: `GpuTrainTransform(..., rand_augment=ra)` runs its chains on the GPU (`vit_augment_to_u8`,
    `vit_randaug_to_tensor`), `host_train_transform(..., rand_augment=ra)` in Pillow's own calls, bit for bit the same.
"""
import collections
import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib

RAW_MODES = ("L", "LA", "RGB", "RGBA")


def decode(img):
    """PIL image -> uint8 [H, W] or [H, W, C] array the GPU pipeline converts to RGB itself (L / LA / RGB / RGBA);
    other modes (P, I;16, CMYK, ...) are converted to RGB here with Pillow, exactly as convert('RGB') would."""
    if img.mode not in RAW_MODES:
        img = img.convert("RGB")
    return np.asarray(img, dtype=np.uint8)


class BrainTumorDataset(torch.utils.data.Dataset):
    """Folder-per-class images with a stratified train/test split (reference BrainTumorDataset.py:10-39: classes are
    `os.listdir(data_dir)` in listing order, split by sklearn train_test_split(stratify=class, random_state))."""

    def __init__(self, data_dir, train=True, test_size=0.2, transform=None, random_state=42):
        import pandas as pd
        from sklearn.model_selection import train_test_split
        labels = os.listdir(data_dir)
        self.transform = transform
        self.data_dir = data_dir
        self.class_encoding = dict(enumerate(labels))
        rows = []
        for i, lab in enumerate(labels):
            rows += [(os.path.join(data_dir, lab, f), i) for f in os.listdir(os.path.join(data_dir, lab))]
        df = pd.DataFrame(rows, columns=["image", "class"])
        tr_x, ts_x, tr_y, ts_y = train_test_split(df[["image"]], df[["class"]], test_size=test_size,
                                                  stratify=df[["class"]], random_state=random_state)
        self.train = pd.concat([tr_x, tr_y], axis=1)
        self.test = pd.concat([ts_x, ts_y], axis=1)
        self.indexer = self.train if train else self.test

    def __len__(self):
        return self.indexer.shape[0]

    def __getitem__(self, idx):
        from PIL import Image
        path, label = self.indexer.iloc[idx]
        image = Image.open(path)
        if self.transform is not None:
            image = self.transform(image)
        return image, int(label)


class CIFAR10Bin(torch.utils.data.Dataset):
    """CIFAR-10 binary version: records of 1 label byte + 3072 bytes (R, G, B planes of 32x32).  Items are uint8
    [32, 32, 3] arrays (what PIL's Image.fromarray gives torchvision's CIFAR10) and int labels."""

    RECORD = 1 + 3 * 32 * 32

    def __init__(self, root, train=True):
        d = os.path.join(root, "cifar-10-batches-bin") if os.path.isdir(os.path.join(root, "cifar-10-batches-bin")) \
            else root
        files = sorted(glob.glob(os.path.join(d, "data_batch_*.bin"))) if train else [os.path.join(d, "test_batch.bin")]
        if not files or not all(os.path.exists(f) for f in files):
            raise FileNotFoundError(f"CIFAR-10 binary batches not found under {root} (no download: offline)")
        self.maps = [np.memmap(f, dtype=np.uint8, mode="r").reshape(-1, self.RECORD) for f in files]
        self.offsets = np.cumsum([0] + [m.shape[0] for m in self.maps])

    def __len__(self):
        return int(self.offsets[-1])

    def __getitem__(self, i):
        f = int(np.searchsorted(self.offsets, i, side="right")) - 1
        rec = self.maps[f][i - self.offsets[f]]
        return np.ascontiguousarray(rec[1:].reshape(3, 32, 32).transpose(1, 2, 0)), int(rec[0])


class SyntheticRawImages(torch.utils.data.Dataset):
    """Deterministic uint8 images: fixed `size` (H, W, C) or, with `ragged`, H and W drawn per item in
    [size/2, 2*size] (exercises the ragged-batch path)."""

    def __init__(self, n, size=(32, 32, 3), classes=10, seed=0, ragged=False):
        self.n, self.size, self.classes, self.seed, self.ragged = n, size, classes, seed, ragged

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed * 1000003 + i)
        h, w, c = self.size
        if self.ragged:
            h, w = int(rng.integers(h // 2, 2 * h + 1)), int(rng.integers(w // 2, 2 * w + 1))
        img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        return img, int(rng.integers(0, self.classes))


def collate_raw(batch):
    """[(uint8 array [H, W] / [H, W, C], label)] -> (packed uint8 [total bytes], meta int64 [B, 4] = (offset, H, W,
    C), labels int64 [B]).  Runs in the DataLoader workers; the buffers are then pinned by the loader."""
    arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a, _ in batch]
    meta = np.zeros((len(arrays), 4), dtype=np.int64)
    off = 0
    for i, a in enumerate(arrays):
        h, w = a.shape[:2]
        c = a.shape[2] if a.ndim == 3 else 1
        if c not in (1, 2, 3, 4):
            raise ValueError(f"image {i}: {c} channels (expected L, LA, RGB or RGBA)")
        meta[i] = (off, h, w, c)
        off += a.size
    packed = np.empty(off, dtype=np.uint8)
    for (o, _, _, _), a in zip(meta, arrays):
        packed[o:o + a.size] = a.reshape(-1)
    labels = torch.tensor([int(l) for _, l in batch], dtype=torch.int64)
    return torch.from_numpy(packed), torch.from_numpy(meta), labels


def raw_loader(dataset, batch_size, shuffle=True, num_workers=4, drop_last=True, pin_memory=True, sampler=None):
    """DataLoader yielding packed raw batches (train.py:161-162 uses 4 workers)."""
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle and sampler is None,
                                       sampler=sampler, num_workers=num_workers, drop_last=drop_last,
                                       pin_memory=pin_memory, collate_fn=collate_raw,
                                       persistent_workers=num_workers > 0)


def _checked_meta(packed, meta):
    """The batch's meta on the host, after the checks that keep the kernels inside `packed`."""
    meta_h = meta.cpu() if meta.is_cuda else meta
    if meta_h.shape[0] == 0:
        raise ValueError("empty batch")
    off, h, w, c = (meta_h[:, i] for i in range(4))
    if (h <= 0).any() or (w <= 0).any() or not ((c >= 1) & (c <= 4)).all():
        raise ValueError("invalid image metadata")
    if int((off + h * w * c).max()) > packed.numel() or (off < 0).any():
        raise ValueError("image metadata points outside the packed buffer")
    return meta_h


AugTable = collections.namedtuple("AugTable", "x0 y0 cw ch flip ey0 ey1 ex0 ex1")


def identity_table(meta):
    """The AugTable that augments nothing: the full image, no flip, no erase box."""
    m = np.asarray(meta, dtype=np.int64).reshape(-1, 4)
    z = np.zeros(m.shape[0], dtype=np.int32)
    return AugTable(z, z, m[:, 2].astype(np.int32), m[:, 1].astype(np.int32), z, z, z, z, z)


def _augment_launch(tf, packed, meta_h, table, device, stream, erase_value=0.0):
    """One vit_augment_to_tensor launch of transform `tf` (its size, dtype, mean, std and workspace) over a packed
    batch with the host AugTable `table`, validated here BEFORE anything is uploaded.  The table goes up from a fresh
    pinned tensor by a non-blocking copy on the launch's stream: no host sync."""
    from . import _ops
    sh, sw = tf.size
    m = meta_h.numpy()
    cols = _ops.check_aug_table(table, m[:, 1], m[:, 2], sh, sw)
    ks = _ops.aug_ksize(cols[2], cols[3], sh, sw)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    B = meta_h.shape[0]
    with torch.cuda.stream(s):
        src = packed.to(dev, non_blocking=True)
        meta_d = meta_h.to(dev, non_blocking=True)
        items = _ops.aug_table_host(cols, pin=True).to(dev, non_blocking=True)
        need = _lib.load().vit_augment_workspace_bytes(B, sh, sw, ks)
        if tf._ws is None or tf._ws.numel() < need or tf._ws.device != dev:
            tf._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, sh, sw, dtype=tf.dtype, device=dev)
    _ops.augment_to_tensor(src, meta_d, items, sh, sw, ks, out, tf._ws, mean=tf.mean, std=tf.std,
                           erase_value=erase_value, stream=s)
    if stream is not None:
        for t in (src, meta_d, items, tf._ws):
            t.record_stream(stream)
    return out


class GpuImageTransform:
    """convert('RGB') -> Resize((S, S)) (PIL bilinear) -> ToTensor on the GPU: packed batch -> [B, 3, S, S].  With the
    keyword-only `mean` / `std` (evaluation beside a normalised training run) also Normalize(mean, std)."""

    def __init__(self, size, dtype=torch.float32, *, mean=None, std=None):
        from . import _ops
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.dtype = dtype
        self.mean, self.std = _ops.check_mean_std(mean, std)
        self._ws = None

    def __call__(self, packed, meta, device=None, stream=None):
        meta_h = _checked_meta(packed, meta)
        B = meta_h.shape[0]
        sh, sw = self.size
        off, h, w, c = (meta_h[:, i] for i in range(4))
        if self.mean is not None:      # evaluation with Normalize: the augmenting launch with an identity table
            return _augment_launch(self, packed, meta_h, identity_table(meta_h), device, stream)
        lib = _lib.load()
        ks = max(max(lib.vit_resize_ksize(int(a), sh) for a in h.unique()),
                 max(lib.vit_resize_ksize(int(a), sw) for a in w.unique()))
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        src = packed.to(dev, non_blocking=True)
        meta_d = meta_h.to(dev, non_blocking=True)
        need = lib.vit_resize_workspace_bytes(B, sh, sw, ks)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, sh, sw, dtype=self.dtype, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        code = _lib.F32 if self.dtype == torch.float32 else _lib.BF16
        _lib.check(lib.vit_resize_to_tensor(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(meta_d.data_ptr()), B,
                                            sh, sw, ks, ctypes.c_void_p(out.data_ptr()), code,
                                            ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                            ctypes.c_void_p(s.cuda_stream)), "vit_resize_to_tensor")
        if stream is not None:
            for t in (src, meta_d, self._ws):
                t.record_stream(stream)
        return out


class TrainAugment:
    """The geometric training augmentation's draws (not in the reference, whose only transform is the resize,
    train.py:151-155): torchvision's RandomResizedCrop.get_params and RandomHorizontalFlip, timm's RandomErasing
    (mode='const') box.  `draw(meta, out_h, out_w)` returns the host AugTable of one batch, one entry per image.

    Crop: up to 10 attempts of area * U(scale), aspect exp(U(log r0, log r1)), w = int(round(sqrt(a r))),
    h = int(round(sqrt(a / r))), accepted if 0 < w <= W and 0 < h <= H and placed uniformly; else the central box with
    the aspect clamped into `ratio` and the long side whole.  `scale=None`: the full image.  Flip: with probability
    `hflip`.  Erase: with probability `erase_prob`, up to 10 attempts of (out area) * U(erase_scale), log-uniform
    aspect, h = int(round(sqrt(a r))), w = int(round(sqrt(a / r))), accepted if h < out_h and w < out_w and placed
    uniformly; else no box.  The box is in output pixels, after the flip, and is filled with `erase_value` after the
    normalize (timm erases the normalised tensor, before mixup).

    The RNG is numpy.random.default_rng([seed, rank]) as in BatchMix; `rank` defaults to the process group's."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), hflip=0.5, erase_prob=0.0, erase_scale=(0.02, 1 / 3),
                 erase_ratio=(0.3, 3.3), erase_value=0.0, seed=0, rank=None):
        def pair(v, name, top=None):
            lo, hi = (float(a) for a in v)
            if not (0.0 < lo <= hi) or (top is not None and hi > top):
                raise ValueError(f"TrainAugment: {name} must be 0 < lo <= hi" + (f" <= {top}" if top else ""))
            return lo, hi
        self.scale = None if scale is None else pair(scale, "scale", 1.0)
        self.ratio = pair(ratio, "ratio")
        self.erase_scale, self.erase_ratio = pair(erase_scale, "erase_scale", 1.0), pair(erase_ratio, "erase_ratio")
        if not (0.0 <= hflip <= 1.0 and 0.0 <= erase_prob <= 1.0):
            raise ValueError("TrainAugment: hflip and erase_prob must lie in [0, 1]")
        if not np.isfinite(erase_value):
            raise ValueError("TrainAugment: erase_value must be finite")
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.hflip, self.erase_prob, self.erase_value = float(hflip), float(erase_prob), float(erase_value)
        self.seed, self.rank = int(seed), int(rank)
        self.reseed()

    def reseed(self, *more):
        """Restart the stream from [seed, rank, *more] (host_train_transform: one stream per DataLoader worker)."""
        self._rng = np.random.default_rng([self.seed, self.rank, *(int(v) for v in more)])

    def crop_box(self, H, W):
        """(x0, y0, cw, ch, fallback) of one RandomResizedCrop draw on an H x W image."""
        if self.scale is None:
            return 0, 0, W, H, False
        rng = self._rng
        area = H * W
        l0, l1 = np.log(self.ratio[0]), np.log(self.ratio[1])
        for _ in range(10):
            a = area * rng.uniform(self.scale[0], self.scale[1])
            r = float(np.exp(rng.uniform(l0, l1)))
            w, h = int(round(float(np.sqrt(a * r)))), int(round(float(np.sqrt(a / r))))
            if 0 < w <= W and 0 < h <= H:
                y0 = int(rng.integers(0, H - h + 1))
                x0 = int(rng.integers(0, W - w + 1))
                return x0, y0, w, h, False
        in_ratio = W / H
        if in_ratio < self.ratio[0]:
            w, h = W, int(round(W / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            w, h = int(round(H * self.ratio[1])), H
        else:
            w, h = W, H
        w, h = min(max(w, 1), W), min(max(h, 1), H)
        return (W - w) // 2, (H - h) // 2, w, h, True

    def erase_box(self, out_h, out_w):
        """(ey0, ey1, ex0, ex1) of one RandomErasing draw; an empty box (zeros) when nothing is erased."""
        rng = self._rng
        if self.erase_prob <= 0.0 or rng.random() >= self.erase_prob:
            return 0, 0, 0, 0
        area = out_h * out_w
        l0, l1 = np.log(self.erase_ratio[0]), np.log(self.erase_ratio[1])
        for _ in range(10):
            a = area * rng.uniform(self.erase_scale[0], self.erase_scale[1])
            r = float(np.exp(rng.uniform(l0, l1)))
            h, w = int(round(float(np.sqrt(a * r)))), int(round(float(np.sqrt(a / r))))
            if h < out_h and w < out_w:
                y0 = int(rng.integers(0, out_h - h + 1))
                x0 = int(rng.integers(0, out_w - w + 1))
                return y0, y0 + h, x0, x0 + w
        return 0, 0, 0, 0

    def draw(self, meta, out_h, out_w):
        """The host AugTable of the next batch from its meta [B, 4] = (offset, H, W, C): int32 numpy arrays.  Per
        image the draws are taken in the order crop, flip, erase."""
        rows = []
        for _, H, W, _ in np.asarray(meta, dtype=np.int64).reshape(-1, 4).tolist():
            x0, y0, cw, ch, _ = self.crop_box(H, W)
            flip = int(self.hflip > 0.0 and self._rng.random() < self.hflip)
            rows.append((x0, y0, cw, ch, flip, *self.erase_box(out_h, out_w)))
        return AugTable(*(np.asarray(c, dtype=np.int32) for c in zip(*rows)))


RA_OPS = ("None", "AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color",
          "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RA_MAX_LAYERS = 4       # VIT_RA_MAX_LAYERS (vit_hip.h)
_RA_ENHANCE = ("Color", "Contrast", "Brightness", "Sharpness")
_RA_GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")

RaTable = collections.namedtuple("RaTable", "op arg coef")


class RandAugment:
    """RandAugment's policy and draws (not in the reference; the rules are timm's `rand_augment_transform`, restated):
    per image `num_layers` times one of `ops`, chosen uniformly with replacement, applied with probability `prob` at
    a magnitude drawn around `magnitude` (of 10).  It sits between the flip and ToTensor: every op maps the uint8 RGB
    picture of the output size to another one.

    `draw(B, out_h, out_w)` returns the host RaTable of one batch: `op` int32 [B, num_layers] (index into RA_OPS, 0 =
    None), `arg` float64 [B, num_layers] (the op's argument as its Pillow call takes it: degrees, shear factor,
    translation in pixels, enhance factor, bits, threshold, addend) and `coef` float64 [B, num_layers, 6] (the AFFINE
    coefficients Pillow receives for the geometric ops, the identity's otherwise).  Per image and layer the draws are
    taken in this order: the op (integers(len(ops))); random() — the entry is None unless it is <= prob; the
    magnitude (uniform(0, m) if magnitude_std is infinite, normal(m, std) if it is > 0, m otherwise; clipped to
    [0, 10]); for an op whose level is negated at random, random() > 0.5.

    Levels, with L = mag / 10: Rotate +-30 L degrees, ShearX / ShearY +-0.3 L, TranslateXRel / TranslateYRel
    +-translate_pct L of the width / height; Color, Contrast, Brightness, Sharpness 1.8 L + 0.1, or with `increasing`
    max(0.1, 1 +- 0.9 L); Posterize int(4 L) bits, increasing 4 - int(4 L); Solarize threshold min(256, int(256 L)),
    increasing 256 - that; SolarizeAdd min(128, int(110 L)) below the threshold 128.

    The RNG is numpy.random.default_rng([seed, rank, RandAugment.TAG]): a stream of its own, so a TrainAugment or
    BatchMix of the same seed draws what it drew without this object beside it."""

    TAG = 0x52416E64        # "RAnd": keeps this stream apart from TrainAugment's [seed, rank]

    def __init__(self, num_layers=2, magnitude=9.0, magnitude_std=0.5, increasing=True, prob=0.5, translate_pct=0.45,
                 fill=(128, 128, 128), ops=None, seed=0, rank=None):
        if not (1 <= int(num_layers) <= RA_MAX_LAYERS) or int(num_layers) != num_layers:
            raise ValueError(f"RandAugment: num_layers must be 1..{RA_MAX_LAYERS}")
        if not (0.0 <= magnitude <= 10.0) or not (magnitude_std >= 0.0) or not (0.0 <= prob <= 1.0):
            raise ValueError("RandAugment: magnitude must lie in [0, 10], magnitude_std be >= 0 and prob lie in [0, 1]")
        if not (0.0 <= translate_pct <= 1.0):
            raise ValueError("RandAugment: translate_pct must lie in [0, 1]")
        fill = tuple(int(v) for v in fill)
        if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
            raise ValueError("RandAugment: fill must be three values in [0, 255]")
        ops = RA_OPS[1:] if ops is None else tuple(ops)
        if not ops or any(o not in RA_OPS[1:] for o in ops):
            raise ValueError(f"RandAugment: ops must be a non-empty choice of {RA_OPS[1:]}")
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.num_layers, self.magnitude, self.magnitude_std = int(num_layers), float(magnitude), float(magnitude_std)
        self.increasing, self.prob, self.translate_pct = bool(increasing), float(prob), float(translate_pct)
        self.fill, self.ops = fill, ops
        self.seed, self.rank = int(seed), int(rank)
        self.reseed()

    @classmethod
    def from_config(cls, config, **kw):
        """timm's `--aa` string: 'rand' and then '-'-separated keys m (magnitude), n (layers), mstd (magnitude std;
        >= 100 means infinite: a uniform magnitude), inc (increasing, 0 / 1) and p (probability).  A key the string
        leaves out has timm's default for the string form — m10, n2, mstd0, inc0, p0.5 —, not the constructor's.  Further
        keyword arguments go to the constructor and win over the string."""
        import re
        parts = str(config).split("-")
        if parts[0] != "rand":
            raise ValueError(f"RandAugment: config {config!r} does not start with 'rand'")
        args = dict(num_layers=2, magnitude=10.0, magnitude_std=0.0, increasing=False, prob=0.5)
        for part in parts[1:]:
            m = re.fullmatch(r"([a-z]+)(\d+(?:\.\d*)?|\.\d+)", part)
            if not m:
                raise ValueError(f"RandAugment: cannot parse {part!r} in config {config!r}")
            key, val = m.group(1), m.group(2)
            if key == "m":
                args["magnitude"] = float(val)
            elif key == "n":
                if not val.isdigit():
                    raise ValueError(f"RandAugment: n needs an integer, not {val!r}")
                args["num_layers"] = int(val)
            elif key == "mstd":
                args["magnitude_std"] = float("inf") if float(val) >= 100 else float(val)
            elif key == "inc":
                if val not in ("0", "1"):
                    raise ValueError(f"RandAugment: inc is 0 or 1, not {val!r}")
                args["increasing"] = val == "1"
            elif key == "p":
                args["prob"] = float(val)
            else:
                raise ValueError(f"RandAugment: unknown key {key!r} in config {config!r} (m, n, mstd, inc, p)")
        return cls(**{**args, **kw})

    def reseed(self, *more):
        """Restart the stream from [seed, rank, TAG, *more] (host_train_transform: one stream per DataLoader worker)."""
        self._rng = np.random.default_rng([self.seed, self.rank, self.TAG, *(int(v) for v in more)])

    def negates(self, name):
        """Is the level of op `name` negated at random?"""
        return name in _RA_GEOMETRIC or (self.increasing and name in _RA_ENHANCE)

    def level_arg(self, name, mag, negate=False):
        """The argument of op `name` at magnitude `mag` (of 10); the translations' as a fraction of the size."""
        lv = mag / 10.0
        sign = -1.0 if negate and self.negates(name) else 1.0
        if name == "Rotate":
            return sign * (lv * 30.0)
        if name in ("ShearX", "ShearY"):
            return sign * (lv * 0.3)
        if name in ("TranslateXRel", "TranslateYRel"):
            return sign * (lv * self.translate_pct)
        if name in _RA_ENHANCE:
            return max(0.1, 1.0 + sign * (lv * 0.9)) if self.increasing else lv * 1.8 + 0.1
        if name == "Posterize":
            return 4 - int(lv * 4) if self.increasing else int(lv * 4)
        if name == "Solarize":
            t = min(256, int(lv * 256))
            return 256 - t if self.increasing else t
        if name == "SolarizeAdd":
            return min(128, int(lv * 110))
        if name in ("AutoContrast", "Equalize", "Invert", "None"):
            return 0.0
        raise ValueError(f"RandAugment: unknown op {name!r}")

    @staticmethod
    def coefficients(name, arg, out_h, out_w):
        """The six AFFINE coefficients Pillow's transform receives for op `name` with argument `arg` on an out_w x
        out_h picture (Image.rotate's own matrix for Rotate); the identity's for every other op."""
        import math
        if name == "ShearX":
            return (1.0, float(arg), 0.0, 0.0, 1.0, 0.0)
        if name == "ShearY":
            return (1.0, 0.0, 0.0, float(arg), 1.0, 0.0)
        if name == "TranslateXRel":
            return (1.0, 0.0, float(arg), 0.0, 1.0, 0.0)
        if name == "TranslateYRel":
            return (1.0, 0.0, 0.0, 0.0, 1.0, float(arg))
        if name != "Rotate" or arg % 360.0 == 0:
            return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        angle = arg % 360.0
        if angle in (90.0, 180.0, 270.0):
            raise ValueError("RandAugment: Image.rotate turns by 90, 180 or 270 degrees with a transpose, not AFFINE")
        cx, cy = out_w / 2, out_h / 2
        angle = -math.radians(angle)
        m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
             round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
        m[2] = m[0] * -cx + m[1] * -cy + m[2]
        m[5] = m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
        return tuple(m)

    def draw(self, B, out_h, out_w):
        """The host RaTable of the next batch of B images of out_h x out_w (see the class)."""
        L = self.num_layers
        op = np.zeros((B, L), dtype=np.int32)
        arg = np.zeros((B, L), dtype=np.float64)
        coef = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (B, L, 1))
        rng = self._rng
        for b in range(B):
            for l in range(L):
                name = self.ops[int(rng.integers(len(self.ops)))]
                if not rng.random() <= self.prob:
                    continue
                mag = self.magnitude
                if np.isinf(self.magnitude_std):
                    mag = float(rng.uniform(0.0, mag))
                elif self.magnitude_std > 0:
                    mag = float(rng.normal(mag, self.magnitude_std))
                mag = min(10.0, max(0.0, mag))
                negate = self.negates(name) and rng.random() > 0.5
                a = self.level_arg(name, mag, negate)
                if name == "TranslateXRel":
                    a = a * out_w
                elif name == "TranslateYRel":
                    a = a * out_h
                op[b, l], arg[b, l] = RA_OPS.index(name), a
                coef[b, l] = self.coefficients(name, a, out_h, out_w)
        return RaTable(op, arg, coef)

    def apply_pil(self, img, row):
        """The chain `row` = (ops, args) of one image (one row of a RaTable's `op` and `arg`) on the RGB PIL image
        `img`, in the literal Pillow calls: the host path, and what the kernels are bit-exact with."""
        from PIL import Image, ImageEnhance, ImageOps
        for k, a in zip(*row):
            name = RA_OPS[int(k)]
            if name == "AutoContrast":
                img = ImageOps.autocontrast(img)
            elif name == "Equalize":
                img = ImageOps.equalize(img)
            elif name == "Invert":
                img = ImageOps.invert(img)
            elif name == "Posterize":
                img = img if int(a) >= 8 else ImageOps.posterize(img, int(a))
            elif name == "Solarize":
                img = ImageOps.solarize(img, int(a))
            elif name == "SolarizeAdd":
                lut = [min(255, i + int(a)) if i < 128 else i for i in range(256)]
                img = img.point(lut + lut + lut)
            elif name in _RA_ENHANCE:
                img = getattr(ImageEnhance, name)(img).enhance(float(a))
            elif name == "Rotate":
                img = img.rotate(float(a), resample=Image.BILINEAR, fillcolor=self.fill)
            elif name in _RA_GEOMETRIC:
                img = img.transform(img.size, Image.AFFINE, self.coefficients(name, float(a), img.size[1], img.size[0]),
                                    resample=Image.BILINEAR, fillcolor=self.fill)
        return img


def _randaug_launch(tf, packed, meta_h, table, ra, device, stream, erase_value=0.0):
    """GpuTrainTransform with a RandAugment: vit_augment_to_u8 (crop, resize, flip), then vit_randaug_to_tensor (the
    chains, normalize, erase) on the same stream.  Both host tables are validated BEFORE anything is uploaded, and go
    up from fresh pinned tensors by non-blocking copies on that stream: no host sync."""
    from . import _ops
    sh, sw = tf.size
    m = meta_h.numpy()
    B = meta_h.shape[0]
    cols = _ops.check_aug_table(table, m[:, 1], m[:, 2], sh, sw)
    ra = _ops.check_ra_table(ra, B)
    ks = _ops.aug_ksize(cols[2], cols[3], sh, sw)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    lib = _lib.load()
    with torch.cuda.stream(s):
        src = packed.to(dev, non_blocking=True)
        meta_d = meta_h.to(dev, non_blocking=True)
        items = _ops.aug_table_host(cols, pin=True).to(dev, non_blocking=True)
        ra_items = _ops.randaug_table_host(ra, tf.rand_augment.fill, pin=True).to(dev, non_blocking=True)
        need = lib.vit_augment_workspace_bytes(B, sh, sw, ks)
        if tf._ws is None or tf._ws.numel() < need or tf._ws.device != dev:
            tf._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=dev)
        need = lib.vit_randaug_workspace_bytes(B, sh, sw)
        if tf._ws_ra is None or tf._ws_ra.numel() < need or tf._ws_ra.device != dev:
            tf._ws_ra = torch.empty(need, dtype=torch.uint8, device=dev)
        u8 = torch.empty(B, sh, sw, 3, dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, sh, sw, dtype=tf.dtype, device=dev)
    _ops.augment_to_u8(src, meta_d, items, sh, sw, ks, u8, tf._ws, stream=s)
    _ops.randaug_to_tensor(u8, ra_items, ra.op.shape[1], _ops.ra_stats_layers(ra), items, out, tf._ws_ra, mean=tf.mean,
                           std=tf.std, erase_value=erase_value, stream=s)
    if stream is not None:
        for t in (src, meta_d, items, ra_items, u8, tf._ws, tf._ws_ra):
            t.record_stream(stream)
    return out


class GpuTrainTransform:
    """The training transform on the GPU: RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize ->
    RandomErasing of a packed batch in ONE vit_augment_to_tensor launch (bit-exact with Pillow's crop().resize()),
    called like GpuImageTransform, so DeviceBatches takes it unchanged.  The table is drawn on the host from `meta`
    (`augment`, a TrainAugment), validated, and uploaded by a non-blocking copy on the launch's stream.

    With `rand_augment` (a RandAugment) its chains run between the flip and ToTensor, bit-exact with Pillow's calls
    (RandAugment.apply_pil): the crop, resize and flip store the uint8 picture (vit_augment_to_u8) and
    vit_randaug_to_tensor takes it from there, on the same stream, still without a host sync."""

    def __init__(self, size, augment, dtype=torch.float32, mean=None, std=None, rand_augment=None):
        from . import _ops
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.augment, self.dtype, self.rand_augment = augment, dtype, rand_augment
        self.mean, self.std = _ops.check_mean_std(mean, std)
        self._ws = self._ws_ra = None

    def __call__(self, packed, meta, device=None, stream=None):
        meta_h = _checked_meta(packed, meta)
        table = self.augment.draw(meta_h.numpy(), *self.size)
        if self.rand_augment is None:
            return _augment_launch(self, packed, meta_h, table, device, stream, erase_value=self.augment.erase_value)
        ra = self.rand_augment.draw(meta_h.shape[0], *self.size)
        return _randaug_launch(self, packed, meta_h, table, ra, device, stream, erase_value=self.augment.erase_value)


MixTable = collections.namedtuple("MixTable", "src w y0 y1 x0 x1 lam")


class BatchMix:
    """mixup and CutMix of a batch and its labels (not in the reference, whose only transform is the resize,
    train.py:151-155; the recipe is timm's Mixup): `mix(x, y) -> (x_mixed, optim.MixedLabels)`.

    Image i is paired with image B - 1 - i (timm's flip; the loader already shuffles).  With probability 1 - `prob`
    nothing is mixed; otherwise CutMix is chosen with probability `switch_prob` when both alphas are > 0, else
    whichever alpha is > 0.  mixup: lambda ~ Beta(alpha, alpha), x = lambda * x[i] + (1 - lambda) * x[B-1-i].  CutMix
    (timm's rand_bbox with the corrected lambda): r = sqrt(1 - lambda), a box of int(H r) x int(W r) around a centre
    uniform in the image, clipped to it, is taken from the partner, and lambda = 1 - box area / (H W).
    `per_image=False` makes one draw for the whole batch, `True` one per image.

    The RNG is numpy.random.default_rng([seed, rank]); `rank` defaults to the process group's rank (0 without one), so
    replicas mix differently and no stream coincides with the weight-init seed.

    Device tensors (float32 / bfloat16): one vit_mix_batch launch, out of place; the table and lambda are uploaded
    from fresh pinned tensors by non-blocking copies; the partner labels are y.flip(0); no host sync.  Host tensors:
    the same formula in torch ops.  `x` is never modified."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_image=False, seed=0,
                 rank=None):
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError("BatchMix needs mixup_alpha > 0 or cutmix_alpha > 0 (and neither negative)")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("BatchMix: prob and switch_prob must lie in [0, 1]")
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.per_image = float(prob), float(switch_prob), bool(per_image)
        self.seed, self.rank = int(seed), int(rank)
        self._rng = np.random.default_rng([self.seed, self.rank])

    def _draw_one(self, H, W):
        """(w, y0, y1, x0, x1, lam) of one draw."""
        rng = self._rng
        if rng.random() >= self.prob:
            return 1.0, 0, 0, 0, 0, 1.0
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            lam = float(np.float32(rng.beta(self.mixup_alpha, self.mixup_alpha)))
            return lam, 0, 0, 0, 0, lam
        lam = rng.beta(self.cutmix_alpha, self.cutmix_alpha)
        r = np.sqrt(1.0 - lam)
        ch, cw = int(H * r), int(W * r)
        cy, cx = int(rng.integers(H)), int(rng.integers(W))
        y0, y1 = int(np.clip(cy - ch // 2, 0, H)), int(np.clip(cy + ch // 2, 0, H))
        x0, x1 = int(np.clip(cx - cw // 2, 0, W)), int(np.clip(cx + cw // 2, 0, W))
        return 1.0, y0, y1, x0, x1, 1.0 - (y1 - y0) * (x1 - x0) / (H * W)

    def draw(self, B, H, W):
        """The host table of the next batch: MixTable(src, w, y0, y1, x0, x1, lam), numpy arrays of B entries (int32
        but w and lam, float32).  lam is the weight of image i's own label."""
        rows = [self._draw_one(H, W) for _ in range(B if self.per_image else 1)]
        if not self.per_image:
            rows = rows * B
        w, y0, y1, x0, x1, lam = zip(*rows)
        i32 = lambda v: np.asarray(v, dtype=np.int32)     # noqa: E731
        return MixTable(np.arange(B - 1, -1, -1, dtype=np.int32), np.asarray(w, dtype=np.float32), i32(y0), i32(y1),
                        i32(x0), i32(x1), np.asarray(lam, dtype=np.float32))

    @staticmethod
    def mix_host(x, tab):
        """The formula of vit_mix_batch in torch ops, on any device: inside the box x[src]; outside it x itself where
        w == 1, else w * x + (1 - w) * x[src] in fp32 rounded once."""
        B, _, H, W = x.shape
        dev = x.device
        col = lambda v, dt: torch.as_tensor(np.asarray(v), dtype=dt, device=dev).view(B, 1, 1, 1)     # noqa: E731
        xs = x[torch.as_tensor(np.asarray(tab.src), dtype=torch.long, device=dev)]
        ys = torch.arange(H, device=dev).view(1, 1, H, 1)
        cs = torch.arange(W, device=dev).view(1, 1, 1, W)
        y0, y1, x0, x1 = (col(v, torch.long) for v in (tab.y0, tab.y1, tab.x0, tab.x1))
        box = (ys >= y0) & (ys < y1) & (cs >= x0) & (cs < x1)
        w = col(tab.w, torch.float32)
        blend = (w * x.float() + (1.0 - w) * xs.float()).to(x.dtype)
        return torch.where(box, xs, torch.where(w == 1.0, x, blend))

    def __call__(self, x, y, stream=None):
        from . import _ops
        from .optim import MixedLabels
        if x.dim() != 4 or y.shape[0] != x.shape[0]:
            raise ValueError("BatchMix: x must be [B, C, H, W] and y must have B entries")
        B, _, H, W = x.shape
        tab = self.draw(B, H, W)
        if not x.is_cuda:
            return self.mix_host(x, tab), MixedLabels(y.long(), y.long().flip(0), torch.from_numpy(tab.lam.copy()))
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        out = _ops.mix_batch(x.contiguous(), tab[:6], stream=s)
        with torch.cuda.stream(s):
            a = y.to(x.device, non_blocking=True).long()
            lam = torch.from_numpy(tab.lam).pin_memory().to(x.device, non_blocking=True)
            labels = MixedLabels(a, a.flip(0), lam)       # src_i = B - 1 - i: the gather is a flip
        return out, labels


class DeviceBatches:
    """Iterate a raw loader as (images [B, 3, S, S] on device, labels on device): the next batch's host->device copy
    and GPU transform are issued on a side stream while the caller's step runs on the current one.  With `mix` (a
    BatchMix) the mix is staged on the side stream directly after the resize, one batch ahead like it, and the
    iterator yields (mixed images, optim.MixedLabels)."""

    def __init__(self, loader, transform, device, mix=None):
        self.loader, self.transform, self.device, self.mix = loader, transform, torch.device(device), mix

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch, stream):
        packed, meta, labels = batch
        with torch.cuda.stream(stream):
            x = self.transform(packed, meta, self.device, stream=stream)
            y = labels.to(self.device, non_blocking=True)
            if self.mix is not None:
                x, y = self.mix(x, y, stream=stream)
            ev = torch.cuda.Event()
            ev.record(stream)
        return x, y, ev

    def __iter__(self):
        side = torch.cuda.Stream(device=self.device)
        it = iter(self.loader)
        nxt = None
        try:
            nxt = self._stage(next(it), side)
        except StopIteration:
            return
        while nxt is not None:
            x, y, ev = nxt
            torch.cuda.current_stream(self.device).wait_event(ev)
            for t in (x, *(y if isinstance(y, tuple) else (y,))):      # every tensor the side stream made
                t.record_stream(torch.cuda.current_stream(self.device))
            try:
                nxt = self._stage(next(it), side)
            except StopIteration:
                nxt = None
            yield x, y


class Transformed(torch.utils.data.Dataset):
    """(item, label) dataset with a per-item transform (the host path's Compose)."""

    def __init__(self, ds, tf):
        self.ds, self.tf = ds, tf

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        x, y = self.ds[i]
        return self.tf(x), y


def _mean_std_columns(mean, std):
    from . import _ops
    mean, std = _ops.check_mean_std(mean, std)
    if mean is None:
        return None, None
    return (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (mean, std))


def host_transform(size, *, mean=None, std=None):
    """The reference transform on the host (Pillow): convert('RGB') -> resize((S, S), BILINEAR) -> /255 CHW; with the
    keyword-only `mean` / `std` then (x - mean) / std per channel."""
    sh, sw = (size, size) if isinstance(size, int) else size
    mean_c, std_c = _mean_std_columns(mean, std)

    def tf(img):
        from PIL import Image
        if not isinstance(img, Image.Image):
            img = Image.fromarray(np.asarray(img, dtype=np.uint8))
        if img.mode != "RGB":
            img = img.convert("RGB")
        a = np.asarray(img.resize((sw, sh), Image.BILINEAR), dtype=np.uint8)
        x = torch.from_numpy(a.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).contiguous()
        return x if mean_c is None else (x - mean_c) / std_c
    return tf


def host_train_transform(size, augment, mean=None, std=None, rand_augment=None):
    """GpuTrainTransform on the host, per item, with Pillow and torch ops (train.py --device cpu): crop().resize(),
    transpose(FLIP_LEFT_RIGHT), /255, (x - mean) / std, erase fill — the table drawn per image by `augment` (a
    TrainAugment); with `rand_augment` (a RandAugment) its chain, drawn per image, runs in Pillow's own calls between
    the flip and /255.  In a DataLoader worker the streams of both are restarted once from [seed, rank, ..., worker id,
    the worker's seed], so the workers' copies do not repeat each other."""
    sh, sw = (size, size) if isinstance(size, int) else size
    mean_c, std_c = _mean_std_columns(mean, std)
    seeded = set()

    def tf(img):
        from PIL import Image
        info = torch.utils.data.get_worker_info()
        if info is not None and info.id not in seeded:
            seeded.add(info.id)
            augment.reseed(info.id, info.seed)
            if rand_augment is not None:
                rand_augment.reseed(info.id, info.seed)
        if not isinstance(img, Image.Image):
            img = Image.fromarray(np.asarray(img, dtype=np.uint8))
        if img.mode != "RGB":
            img = img.convert("RGB")
        W, H = img.size
        t = augment.draw(np.array([[0, H, W, 3]], dtype=np.int64), sh, sw)
        x0, y0, cw, ch, flip, ey0, ey1, ex0, ex1 = (int(c[0]) for c in t)
        if not (0 <= x0 and 1 <= cw and x0 + cw <= W and 0 <= y0 and 1 <= ch and y0 + ch <= H):
            raise ValueError(f"augment table: crop ({x0}, {y0}, {cw}, {ch}) is empty or outside its {H} x {W} image")
        img = img.crop((x0, y0, x0 + cw, y0 + ch)).resize((sw, sh), Image.BILINEAR)
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        if rand_augment is not None:
            from . import _ops
            ra = _ops.check_ra_table(rand_augment.draw(1, sh, sw), 1)
            img = rand_augment.apply_pil(img, (ra.op[0], ra.arg[0]))
        a = np.asarray(img, dtype=np.uint8)
        x = torch.from_numpy(a.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).contiguous()
        if mean_c is not None:
            x = (x - mean_c) / std_c
        x[:, max(ey0, 0):ey1, max(ex0, 0):ex1] = augment.erase_value
        return x
    return tf
