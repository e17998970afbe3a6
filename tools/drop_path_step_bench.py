"""Time whole training steps with and without stochastic depth, as an interleaved A/B inside one process (one JSON
line at the end).

One ViT-B/16 model (224 x 224, batch 256, bf16: the C2 configuration) and one resident synthetic batch; an arm is the
value of `model.drop_path_rates`: `off` = all 0 (the launches of a model built without the keyword), `on` = timm's
linspace rule up to --rate.  Each round runs --steps train()-style steps (forward, loss, zero_grad, backward,
FusedAdamW step) of one arm, then of the other, after --warmup untimed steps of each, so both arms see the same
machine, clocks and allocator state; a round's time is wall clock between two device synchronisations.  Reported per
arm: the mean ms/step over the rounds and the spread (max - min) of the rounds, and the difference on - off.
usage: python tools/drop_path_step_bench.py [--rate 0.1] [--rounds 4] [--steps 20] [--warmup 5] [--batch 256]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", default="base")
    args = ap.parse_args()
    from VisionTransformer import config, vit
    from VisionTransformer.optim import cross_entropy, make_optimizer
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    cfg = config.ViTConfig.preset(args.model, img_size=S, batch_size=B, num_classes=1000, device="cpu",
                                  precision=torch.bfloat16)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(dev).train()
    opt = make_optimizer(model.parameters(), lr=1e-4, weight_decay=1e-4, device=dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).to(dev).bfloat16()
    y = torch.randint(0, 1000, (B,), generator=g).to(dev)
    arms = {"off": [0.0] * cfg.num_blocks, "on": config.drop_path_rates(args.rate, cfg.num_blocks)}

    def steps(n):
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
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            model.drop_path_rates = arms[name]
            steps(args.warmup)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loss = steps(args.steps)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3 / max(args.steps, 1))
            last[name] = float(loss.item())
            print(f"{r + 1} [{name}] {ms[name][-1]:.3f} ms/step", file=sys.stderr, flush=True)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    print(json.dumps({"model": args.model, "batch": B, "rate": args.rate, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup,
                      "ms_per_step": {k: round(mean[k], 3) for k in ms},
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
                      "on_minus_off_ms": round(mean["on"] - mean["off"], 3),
                      "on_minus_off_pct": round(100.0 * (mean["on"] - mean["off"]) / mean["off"], 2),
                      "final_loss": {k: round(v, 5) for k, v in last.items()}}), flush=True)


if __name__ == "__main__":
    main()
