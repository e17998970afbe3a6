"""Time vit_mix_batch and vit_softmax_xent_mixed at the benchmark shapes, event to event, warmed, arms interleaved rep
by rep in one process.  usage: python tools/mix_bench.py [--reps 20]

  * vit_mix_batch on [256, 3, 224, 224], fp32 and bf16: all-mixup (w = 0.3, empty boxes) and all-CutMix (w = 1, one
    lambda = 0.5 box per image: 158 x 158 pixels at a fixed off-centre position), the device table already resident
    (BatchMix uploads 6 KB per batch beside it).  Algorithmic bytes from the shapes: mixup reads two images and writes
    one (3 N esize), CutMix reads one or the other and writes one (2 N esize).
  * timm's in-place torch formulation of the same results: x.flip(0).mul_(1 - lam); x.mul_(lam).add_(flipped) and
    x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh].
  * vit_softmax_xent_mixed (eps = 0.1, two labels) at 256 x 1000 against F.cross_entropy on a dense smoothed target,
    forward and backward, with and without building that target.
  * vit_adamw on the ViT-B/16 parameter set, the project's measured streaming yardstick (30 B per element), from the
    same process."""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def _stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _interleaved(arms, reps, warmup=3):
    times = {k: [] for k in arms}
    for i in range(reps + warmup):
        for name, fn in arms.items():
            t = _timed(fn)
            if i >= warmup:
                times[name].append(t)
    return times


def mix_bench(reps, dev):
    from VisionTransformer import _lib, _ops
    B, C, H, W = 256, 3, 224, 224
    n = B * C * H * W
    side = int(round((0.5 * H * W) ** 0.5))                        # lambda = 0.5: a 158 x 158 box
    y0, x0 = 31, 45                                                # odd x0: both box edges cut a 16-byte unit
    src = list(range(B - 1, -1, -1))
    tables = {"mixup": (src, [0.3] * B, [0] * B, [0] * B, [0] * B, [0] * B),
              "cutmix": (src, [1.0] * B, [y0] * B, [y0 + side] * B, [x0] * B, [x0 + side] * B)}
    print(f"vit_mix_batch on [{B}, {C}, {H}, {W}] ({reps} reps after 3 warm-up, us: median [min .. max]); CutMix box "
          f"{side} x {side} at ({y0}, {x0})")
    for dtype in (torch.float32, torch.bfloat16):
        es = torch.empty((), dtype=dtype).element_size()
        x = torch.randn(B, C, H, W, device=dev).to(dtype)
        out = torch.empty_like(x)
        xt = x.clone()                                             # timm's formulation works in place
        arms, nbytes = {}, {}
        for kind, tab in tables.items():
            cols = _ops.check_mix_table(*tab, B, H, W)
            items = _ops.mix_table_host(*cols).to(dev)
            arms[f"vit_mix_batch {kind}"] = (lambda items=items: _lib.call(
                "vit_mix_batch", _ops._ptr(x), _ops._ptr(out), _ops.dtype_code(x), B, C, H, W, _ops._ptr(items),
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            # CutMix reads every element from exactly one of the two images and writes it once: 2 N esize
            nbytes[f"vit_mix_batch {kind}"] = (3 if kind == "mixup" else 2) * n * es
        lam = 0.3

        def timm_mixup():
            flipped = xt.flip(0).mul_(1.0 - lam)
            xt.mul_(lam).add_(flipped)

        def timm_cutmix():
            xt[:, :, y0:y0 + side, x0:x0 + side] = xt.flip(0)[:, :, y0:y0 + side, x0:x0 + side]

        arms["timm in-place mixup"], arms["timm in-place cutmix"] = timm_mixup, timm_cutmix
        times = _interleaved(arms, reps)
        med = {}
        for name, ts in times.items():
            m_, lo, hi = _stats(ts)
            med[name] = m_
            bw = f"  {nbytes[name] / m_ / 1e6:5.2f} TB/s ({nbytes[name] / 1e6:.0f} MB algorithmic)" if name in nbytes else ""
            print("  %-5s %-24s %8.1f [%8.1f .. %8.1f]%s" % (str(dtype)[6:], name, m_, lo, hi, bw))
        for kind in tables:
            print(f"  {str(dtype)[6:]:5s} timm / vit_mix_batch, {kind}: "
                  f"{med['timm in-place ' + kind] / med['vit_mix_batch ' + kind]:.2f}x")


def xent_bench(reps, dev):
    from VisionTransformer import _ops
    rows, classes, eps = 256, 1000, 0.1
    lg = torch.randn(rows, classes, device=dev) * 4
    a, b = (torch.randint(0, classes, (rows,), device=dev) for _ in range(2))
    lam = torch.rand(rows, device=dev)
    lg_t = lg.clone().requires_grad_(True)

    def dense():
        t = torch.zeros(rows, classes, device=dev)
        t.scatter_add_(1, a[:, None], lam[:, None])
        t.scatter_add_(1, b[:, None], (1 - lam)[:, None])
        return t * (1 - eps) + eps / classes

    target = dense()

    def torch_loss(t):
        lg_t.grad = None
        F.cross_entropy(lg_t, t).backward()

    arms = {"vit_softmax_xent_mixed": lambda: _ops.softmax_xent_mixed(lg, a, b, lam, eps),
            "vit_softmax_xent (hard labels)": lambda: _ops.softmax_xent(lg, a),
            "F.cross_entropy fwd+bwd, dense target given": lambda: torch_loss(target),
            "dense target + F.cross_entropy fwd+bwd": lambda: torch_loss(dense())}
    times = _interleaved(arms, reps)
    print(f"loss at {rows} x {classes}, eps {eps}, two labels per row (loss and gradient; the kernel arms include the "
          "wrapper's three small allocations), us: median [min .. max]")
    med = {}
    for name, ts in times.items():
        med[name] = _stats(ts)[0]
        print("  %-46s %8.1f [%8.1f .. %8.1f]" % ((name,) + _stats(ts)))
    k = med["vit_softmax_xent_mixed"]
    print(f"  torch (target given) / kernel: {med['F.cross_entropy fwd+bwd, dense target given'] / k:.2f}x;  "
          f"torch (with target) / kernel: {med['dense target + F.cross_entropy fwd+bwd'] / k:.2f}x;  "
          f"mixed / hard-label kernel: {k / med['vit_softmax_xent (hard labels)']:.2f}x")


def adamw_yardstick(reps, dev):
    from VisionTransformer import _ops, config, vit
    cfg = config.ViTConfig.preset("base", img_size=224, batch_size=256, num_classes=1000, device="cpu")
    ps = [p.detach() for p in vit.VisionTransformer(cfg).to(dev).parameters()]
    gs = [torch.randn_like(p) for p in ps]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    sh = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) for p in ps]
    n = sum(p.numel() for p in ps)
    tab, nc = _ops.build_chunk_table(list(zip(ps, gs, ms, vs, sh)), dev)
    ts = _interleaved({"adamw": lambda: _ops.adamw(tab, nc, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 0.1, 0.001, 1.0,
                                                   torch.bfloat16)}, reps)["adamw"]
    m_, lo, hi = _stats(ts)
    print(f"yardstick: vit_adamw on the C2 parameter set ({n / 1e6:.1f}M elements, {nc} workgroups) "
          f"{m_:.1f} [{lo:.1f} .. {hi:.1f}] us = {n * 30 / m_ / 1e6:.2f} TB/s (30 B / element)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mix_bench(args.reps, dev)
    xent_bench(args.reps, dev)
    adamw_yardstick(args.reps, dev)


if __name__ == "__main__":
    main()
