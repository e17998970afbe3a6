"""Time whole training steps with FusedAdamW and with FusedLamb, as an interleaved A/B inside one process (one JSON
line at the end), in the manner of tools/drop_path_step_bench.py.

One ViT-B/16 model (224 x 224, batch 256, bf16: the C2 configuration), one resident synthetic batch and two optimizers
over the same parameters, each with its own moments; an arm is the optimizer that steps.  Each round runs --steps
train()-style steps (forward, loss, zero_grad, backward, step) of one arm, then of the other, after --warmup untimed
steps of each, so both arms see the same machine, clocks and allocator state; a round's time is wall clock between two
device synchronisations.  Reported per arm: the mean ms/step over the rounds and the spread (max - min) of the rounds,
and the difference lamb - adamw.  --no-decay-1d steps timm's two weight-decay groups in both arms.
usage: python tools/lamb_step_bench.py [--rounds 4] [--steps 20] [--warmup 5] [--batch 256] [--no-decay-1d]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", default="base")
    ap.add_argument("--no-decay-1d", action="store_true")
    args = ap.parse_args()
    from VisionTransformer import config, vit
    from VisionTransformer.optim import cross_entropy, make_optimizer, param_groups_weight_decay
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    cfg = config.ViTConfig.preset(args.model, img_size=S, batch_size=B, num_classes=1000, device="cpu",
                                  precision=torch.bfloat16)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(dev).train()

    def params():
        return param_groups_weight_decay(model, 0.05) if args.no_decay_1d else model.parameters()

    arms = {name: make_optimizer(params(), lr=1e-4, weight_decay=0.05, device=dev, opt=name)
            for name in ("adamw", "lamb")}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).to(dev).bfloat16()
    y = torch.randint(0, 1000, (B,), generator=g).to(dev)

    def steps(opt, n):
        loss = None
        for _ in range(n):
            loss = cross_entropy(model(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return loss

    ms = {k: [] for k in arms}
    last = {}
    for r in range(args.rounds):
        for name in (("adamw", "lamb") if r % 2 == 0 else ("lamb", "adamw")):
            steps(arms[name], args.warmup)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loss = steps(arms[name], args.steps)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3 / max(args.steps, 1))
            last[name] = float(loss.item())
            print(f"{r + 1} [{name}] {ms[name][-1]:.3f} ms/step", file=sys.stderr, flush=True)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    print(json.dumps({"model": args.model, "batch": B, "no_decay_1d": args.no_decay_1d, "rounds": args.rounds,
                      "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": {k: round(mean[k], 3) for k in ms},
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
                      "lamb_minus_adamw_ms": round(mean["lamb"] - mean["adamw"], 3),
                      "lamb_minus_adamw_pct": round(100.0 * (mean["lamb"] - mean["adamw"]) / mean["adamw"], 2),
                      "final_loss": {k: round(v, 5) for k, v in last.items()}}), flush=True)


if __name__ == "__main__":
    main()
