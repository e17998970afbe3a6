"""Time vit_augment_to_tensor against vit_resize_to_tensor at the loader's shapes, event to event, warmed, arms
interleaved rep by rep in one process.  usage: python tools/augment_bench.py [--reps 20] [--batch 256]

Shapes, at B = 256, output 224 x 224, fp32 and bf16:
  (i)   32 x 32 x 3 sources, full box (CIFAR, ksize 3);
  (ii)  375 x 500 x 3 sources, full box (ksize 7);
  (iii) 375 x 500 x 3 sources with TrainAugment(seed=0) boxes, flip 0.5, erase 0.25, ImageNet mean / std.
Arms: vit_resize_to_tensor (i, ii: the launch the identity table must not be slower than), and vit_augment_to_tensor
under augment_path 0 (automatic), 1 (direct) and 2 (tiled); every arm includes its coefficient kernel.  For (iii) also
the torch formulation a user would write — per-image slicing, F.interpolate(antialias=True), flip, normalize, fill —
for scale only: its pixels differ from Pillow's.  Algorithmic bytes from the shapes: the source bytes of the boxes
read once plus 3 * 224^2 * esize written per image.  Each line gives median [min .. max]; the acceptance lines compare
a difference of medians with the larger of the two arms' own min-max spreads.  vit_adamw on the ViT-B/16 parameter
set, the project's streaming yardstick, is timed in the same process."""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mix_bench import _interleaved, _stats, adamw_yardstick  # noqa: E402

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _batch(B, H, W, dev):
    g = torch.Generator().manual_seed(0)
    packed = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, generator=g)
    meta = torch.tensor([[i * H * W * 3, H, W, 3] for i in range(B)], dtype=torch.int64)
    return packed.to(dev), meta


def _torch_formulation(src, meta, table, S, mean, std, dtype):
    """What a user would write in torch ops over the ragged crops (not Pillow's pixels: for scale only)."""
    m = torch.tensor(mean, device=src.device).view(3, 1, 1)
    s = torch.tensor(std, device=src.device).view(3, 1, 1)
    rows = list(zip(*(c.tolist() for c in table)))
    metas = meta.tolist()

    def run():
        out = []
        for (off, H, W, C), (x0, y0, cw, ch, flip, ey0, ey1, ex0, ex1) in zip(metas, rows):
            img = src[off:off + H * W * C].view(H, W, C)[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1).float()
            r = F.interpolate(img[None], size=(S, S), mode="bilinear", antialias=True, align_corners=False)[0]
            if flip:
                r = r.flip(-1)
            r = (r.round().clamp(0, 255) / 255.0 - m) / s
            r[:, ey0:ey1, ex0:ex1] = 0.0
            out.append(r)
        return torch.stack(out).to(dtype)
    return run


def _report(name, ts, nbytes=None):
    m_, lo, hi = _stats(ts)
    bw = f"  {nbytes / m_ / 1e6:5.2f} TB/s ({nbytes / 1e6:.0f} MB algorithmic)" if nbytes else ""
    print("    %-34s %9.1f [%9.1f .. %9.1f]%s" % (name, m_, lo, hi, bw))
    return m_, hi - lo


def augment_bench(reps, B, dev, skip_torch):
    from VisionTransformer import _lib, _ops, data
    lib = _lib.load()
    S = 224
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    shapes = {"(i) 32x32x3, full box": (32, 32, False), "(ii) 375x500x3, full box": (375, 500, False),
              "(iii) 375x500x3, TrainAugment(seed=0) boxes, flip 0.5, erase 0.25, ImageNet mean/std": (375, 500, True)}
    print(f"vit_augment_to_tensor, B = {B}, output {S} x {S} ({reps} reps after 3 warm-up, us: median [min .. max])")
    for title, (H, W, aug) in shapes.items():
        src, meta = _batch(B, H, W, dev)
        meta_d = meta.to(dev)
        if aug:
            table = data.TrainAugment(hflip=0.5, erase_prob=0.25, seed=0, rank=0).draw(meta, S, S)
            mean, std = IMAGENET
        else:
            table, mean, std = data.identity_table(meta), None, None
        cols = _ops.check_aug_table(table, meta[:, 1].numpy(), meta[:, 2].numpy(), S, S)
        ks = _ops.aug_ksize(cols[2], cols[3], S, S)
        ks_full = _ops.aug_ksize([W], [H], S, S)
        items = _ops.aug_table_host(cols).to(dev)
        ws = torch.empty(lib.vit_augment_workspace_bytes(B, S, S, max(ks, ks_full)), dtype=torch.uint8, device=dev)
        src_bytes = int((cols[2] * cols[3] * 3).sum())
        print(f"  {title}: ksize {ks}, {src_bytes / 1e6:.1f} MB of source inside the boxes")
        for dtype in (torch.float32, torch.bfloat16):
            es = torch.empty((), dtype=dtype).element_size()
            out = torch.empty(B, 3, S, S, dtype=dtype, device=dev)
            nbytes = src_bytes + B * 3 * S * S * es
            code = _ops.dtype_code(out)
            arms = {}
            if not aug:
                arms["vit_resize_to_tensor"] = lambda: _lib.call(
                    "vit_resize_to_tensor", _ops._ptr(src), _ops._ptr(meta_d), B, S, S, ks_full, _ops._ptr(out), code,
                    _ops._ptr(ws), ws.numel(), stream())

            def launch(path):
                _lib.set_option("augment_path", path)
                _ops.augment_to_tensor(src, meta_d, items, S, S, ks, out, ws, mean=mean, std=std)
            for path, name in ((0, "augment, automatic"), (1, "augment, direct"), (2, "augment, tiled")):
                arms[name] = lambda path=path: launch(path)
            times = _interleaved(arms, reps)
            _lib.set_option("augment_path", 0)
            if aug and not skip_torch:
                # in a loop of its own: its ~1,300 small launches leave the arm after it a cold cache
                times.update(_interleaved({"torch slicing + interpolate": _torch_formulation(
                    src, meta, table, S, mean, std, dtype)}, reps))
            print(f"   {str(dtype)[6:]}")
            res = {name: _report(name, ts, None if name.startswith("torch") else nbytes) for name, ts in times.items()}
            d, t = res["augment, direct"], res["augment, tiled"]
            spread = max(d[1], t[1])
            print(f"    tiled vs direct: {d[0] - t[0]:+.1f} us in favour of tiled, spread {spread:.1f} us -> "
                  f"{'tiled faster' if d[0] - t[0] > spread else 'direct faster' if t[0] - d[0] > spread else 'tie'}")
            if not aug:
                p, a = res["vit_resize_to_tensor"], res["augment, automatic"]
                spread = max(p[1], a[1])
                print(f"    identity table (automatic) vs vit_resize_to_tensor: {a[0] - p[0]:+.1f} us, spread "
                      f"{spread:.1f} us -> {'ok' if a[0] - p[0] <= spread else 'SLOWER'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the torch formulation of shape (iii)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    augment_bench(args.reps, args.batch, dev, args.skip_torch)
    adamw_yardstick(args.reps, dev)


if __name__ == "__main__":
    main()
