"""Time the RandAugment launches at the ViT-B input shape: B = 256 pictures of 224 x 224 from 256 x 256 x 3 uint8
sources.  usage: python tools/randaug_bench.py [--calls 200] [--batch 256] [--dtype bf16]

Arms, each timed with device events around `--calls` calls after as many untimed ones:
  u8 stage      vit_augment_to_u8 with TrainAugment(seed=0) boxes and flips (coefficient launch + apply launch);
  one layer     vit_randaug_to_tensor with one layer in which every image has the same kind — None (the copy), a lookup
                table that needs no statistics (Posterize), one that does (Equalize: + the statistics launch), the blend
                with the pixel's gray (Color), the blend with the 3x3 smooth (Sharpness), the affine gather (Rotate 27) —
                followed by the finish launch every call ends in;
  rand-m9 mix   vit_randaug_to_tensor with the table RandAugment.from_config("rand-m9-mstd0.5-inc1", seed=0) draws: two
                layers, the kinds mixed across the batch.
Beside each time: the launches of the call, the bytes it moves by its shapes (a layer reads and writes the uint8
batch; the statistics launch reads the pictures that need it; the finish reads it and writes the tensor) and the GB/s
they imply.  The None arm is the floor of the others: a copy and the finish."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _time(fn, calls):
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    import numpy as np
    from VisionTransformer import _lib, _ops, data
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, S, SRC = args.batch, 224, 256
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)
    packed = torch.randint(0, 256, (B * SRC * SRC * 3,), dtype=torch.uint8, generator=g).to(dev)
    meta = torch.tensor([[i * SRC * SRC * 3, SRC, SRC, 3] for i in range(B)], dtype=torch.int64)
    table = data.TrainAugment(hflip=0.5, erase_prob=0.25, seed=0, rank=0).draw(meta, S, S)
    cols = _ops.check_aug_table(table, meta[:, 1].numpy(), meta[:, 2].numpy(), S, S)
    ks = _ops.aug_ksize(cols[2], cols[3], S, S)
    items = _ops.aug_table_host(cols).to(dev)
    meta_d = meta.to(dev)
    ws1 = torch.empty(lib.vit_augment_workspace_bytes(B, S, S, ks), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(lib.vit_randaug_workspace_bytes(B, S, S), dtype=torch.uint8, device=dev)
    u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, S, S, dtype=dtype, device=dev)
    pic = B * S * S * 3
    fin = pic + out.numel() * out.element_size()
    print(f"RandAugment launches, B = {B}, {SRC} x {SRC} x 3 sources -> {S} x {S}, out {args.dtype}; {args.calls} calls "
          f"timed after {args.calls} untimed; one uint8 batch is {pic / 1e6:.1f} MB")
    print("  %-28s %10s %9s %10s %9s" % ("arm", "us / call", "launches", "MB moved", "GB/s"))

    def report(name, us, launches, nbytes):
        print("  %-28s %10.1f %9d %10.1f %9.0f" % (name, us, launches, nbytes / 1e6, nbytes / us / 1e3), flush=True)

    src_bytes = int((cols[2] * cols[3] * 3).sum())
    report(f"u8 stage (ksize {ks})", _time(lambda: _ops.augment_to_u8(packed, meta_d, items, S, S, ks, u8, ws1), args.calls),
           2, src_bytes + pic)
    _ops.augment_to_u8(packed, meta_d, items, S, S, ks, u8, ws1)

    def arm(name, ra):
        ra = _ops.check_ra_table(ra, B)
        host, L, stats = _ops.randaug_table_host(ra).to(dev), ra.op.shape[1], _ops.ra_stats_layers(ra)
        kinds = _ops._ra_kinds(ra.op)
        need = np.isin(kinds, _ops._RA_STATS_KINDS)
        nbytes = L * 2 * pic + int(need.sum()) * S * S * 3 + fin
        us = _time(lambda: _ops.randaug_to_tensor(u8, host, L, stats, items, out, ws2, mean=IMAGENET[0],
                                                  std=IMAGENET[1]), args.calls)
        report(name, us, L + bin(stats).count("1") + 1, nbytes)

    def uniform(name, a):
        op = np.full((B, 1), data.RA_OPS.index(name), np.int32)
        coef = np.tile(np.array(data.RandAugment.coefficients(name, a, S, S)), (B, 1, 1))
        return data.RaTable(op, np.full((B, 1), float(a)), coef)
    for title, name, a in (("None (copy)", "None", 0.0), ("table (Posterize 1)", "Posterize", 1),
                           ("table + stats (Equalize)", "Equalize", 0.0), ("blend (Color 1.81)", "Color", 1.81),
                           ("smooth (Sharpness 1.81)", "Sharpness", 1.81), ("affine (Rotate 27)", "Rotate", 27.0)):
        arm("1 layer: " + title, uniform(name, a))
    ra = data.RandAugment.from_config("rand-m9-mstd0.5-inc1", seed=0, rank=0)
    t = ra.draw(B, S, S)
    used = sorted({data.RA_OPS[k] for k in t.op.ravel()})
    arm("rand-m9-mstd0.5-inc1 mix", t)
    print(f"  the mix: {int((t.op != 0).sum())} of {t.op.size} entries applied, {len(used) - 1} ops drawn")


if __name__ == "__main__":
    main()
