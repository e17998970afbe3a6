"""Time the knowledge-distillation step and its loss kernel, as interleaved arms inside one process (one JSON line at
the end), in the manner of tools/lamb_step_bench.py.

Steps: one ViT-S/16 student (224 x 224, batch 256, bf16: the C2 shape at the `small` preset), one resident synthetic
batch and one FusedAdamW; an arm is the teacher: "none" (the plain step: cross_entropy, the launches of a run without
a teacher), or a frozen eval-mode teacher of a --teachers preset, run under no_grad on the batch before
optim.distillation_loss (soft, alpha 0.5, tau 1).  Each round runs --steps train()-style steps (teacher forward,
student forward, loss, zero_grad, backward, step) of every arm in turn — the order reversed every other round — after
--warmup untimed steps of that arm; a round's time is wall clock between two device synchronisations.  Each teacher's
eval forward is also timed alone, in the same rounds.  Reported per arm: the mean ms/step over the rounds, the spread
(max - min) of the rounds, the difference to the "none" arm, and the teacher's eval forward beside it.

Kernel: vit_softmax_xent_distill (soft and hard) against vit_softmax_xent_mixed on the same logits, labels and
smoothing at (256, 1000) and (256, 10), --kernel-calls calls between two device events after as many untimed ones, the
arms interleaved over the same rounds; microseconds per call (each call is the row launch and the reduce launch).
usage: python tools/distill_step_bench.py [--teachers small,base] [--rounds 4] [--steps 20] [--warmup 5] [--batch 256]
       [--student small] [--kernel-calls 200] [--skip-steps] [--skip-kernel]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def bench_steps(args, dev):
    from VisionTransformer import config, vit
    from VisionTransformer.optim import cross_entropy, distillation_loss, make_optimizer
    B, S = args.batch, 224

    def preset(name):
        return config.ViTConfig.preset(name, img_size=S, batch_size=B, num_classes=1000, device="cpu",
                                       precision=torch.bfloat16)

    torch.manual_seed(0)
    model = vit.VisionTransformer(preset(args.student)).to(dev).train()
    opt = make_optimizer(model.parameters(), lr=1e-4, weight_decay=1e-4, device=dev)
    teachers = {"none": None}
    for name in [t for t in args.teachers.split(",") if t]:
        torch.manual_seed(1)
        t = vit.VisionTransformer(preset(name)).to(dev).eval().requires_grad_(False)     # vit.load_teacher's state
        t.store_attention_probs = False
        teachers[name] = t
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).to(dev).bfloat16()
    y = torch.randint(0, 1000, (B,), generator=g).to(dev)

    def steps(teacher, n):
        loss = None
        for _ in range(n):
            if teacher is None:
                loss = cross_entropy(model(x), y)
            else:
                with torch.no_grad():
                    tz = teacher(x)
                loss = distillation_loss(model(x), y, tz, kind="soft", alpha=0.5, tau=1.0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return loss

    def forwards(teacher, n):
        with torch.no_grad():
            for _ in range(n):
                teacher(x)

    def timed(fn, *a):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn(*a, args.steps)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / max(args.steps, 1), out

    names = list(teachers)
    ms = {k: [] for k in names}
    fwd = {k: [] for k in names if teachers[k] is not None}
    last = {}
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            steps(teachers[name], args.warmup)
            t, loss = timed(steps, teachers[name])
            ms[name].append(t)
            last[name] = float(loss.item())
            print(f"{r + 1} [{name}] {t:.3f} ms/step", file=sys.stderr, flush=True)
            if teachers[name] is not None:
                forwards(teachers[name], args.warmup)
                t, _ = timed(forwards, teachers[name])
                fwd[name].append(t)
                print(f"{r + 1} [{name} eval forward alone] {t:.3f} ms", file=sys.stderr, flush=True)

    def summary(d):
        mean = {k: sum(v) / len(v) for k, v in d.items()}
        return mean, {"ms": {k: round(mean[k], 3) for k in d},
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in d.items()},
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in d.items()}}

    mean, step_out = summary(ms)
    fmean, fwd_out = summary(fwd)
    return {"student": args.student, "batch": B, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
            "step": step_out, "teacher_eval_forward_alone": fwd_out,
            "step_minus_none_ms": {k: round(mean[k] - mean["none"], 3) for k in fwd},
            "step_minus_none_over_forward": {k: round((mean[k] - mean["none"]) / fmean[k], 3) for k in fwd},
            "final_loss": {k: round(v, 5) for k, v in last.items()}}


def bench_kernel(args, dev):
    from VisionTransformer import _ops
    out = {}
    n = args.kernel_calls
    for rows, classes in ((256, 1000), (256, 10)):
        g = torch.Generator().manual_seed(classes)
        lg = (torch.randn(rows, classes, generator=g) * 4).to(dev)
        tz = (torch.randn(rows, classes, generator=g) * 4).to(dev)
        a = torch.randint(0, classes, (rows,), generator=g).to(dev)
        b = torch.randint(0, classes, (rows,), generator=g).to(dev)
        lam = torch.rand(rows, generator=g).to(dev)
        arms = {"mixed": lambda: _ops.softmax_xent_mixed(lg, a, b, lam, 0.1),
                "distill_soft": lambda: _ops.softmax_xent_distill(lg, tz, a, b, lam, 0.1, "soft", 0.5, 2.0),
                "distill_hard": lambda: _ops.softmax_xent_distill(lg, tz, a, b, lam, 0.1, "hard", 0.5, 2.0)}
        us = {k: [] for k in arms}
        names = list(arms)
        for r in range(args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                fn = arms[name]
                for _ in range(n):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / n)
                print(f"{r + 1} [{rows}x{classes} {name}] {us[name][-1]:.2f} us/call", file=sys.stderr, flush=True)
        mean = {k: sum(v) / len(v) for k, v in us.items()}
        out[f"{rows}x{classes}"] = {"us_per_call": {k: round(mean[k], 2) for k in us},
                                    "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
                                    "rounds_us": {k: [round(t, 2) for t in v] for k, v in us.items()},
                                    "calls": n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teachers", default="small,base")
    ap.add_argument("--student", default="small")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {}
    if not args.skip_kernel:
        out["kernel"] = bench_kernel(args, dev)
    if not args.skip_steps:
        out["steps"] = bench_steps(args, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
