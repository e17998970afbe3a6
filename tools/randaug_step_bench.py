"""Time whole training steps fed through data.DeviceBatches with and without RandAugment, both arms in ONE process,
interleaved round by round (the model, the optimizer and the batches are shared; each arm has its own transform).

As tools/augment_step_bench.py: forward, loss, zero_grad, backward, optimizer step on the C2 configuration (ViT-B/16,
224 x 224, batch 256, bf16), every batch staged by DeviceBatches on its side stream one step ahead from four
pre-collated pinned batches of uint8 images, cycled, so that the host loader is not what is timed.
Arm `augment`: GpuTrainTransform(224, TrainAugment(erase_prob=0.25), ImageNet mean / std) — the single launch.
Arm `randaug`: the same with rand_augment=RandAugment.from_config("rand-m9-mstd0.5-inc1") — the uint8 stage, two layers
and the finish, and the chains' draws on the host.
Per round and arm: ms per step over `--steps` steps after `--warmup`; then each arm's median and spread (max - min) and
whether the difference of the medians exceeds the larger spread.
usage: python tools/randaug_step_bench.py [--rounds 4] [--steps 20] [--warmup 5] [--src 256]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from augment_step_bench import IMAGENET, Cycle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--src", type=int, default=256, help="side of the square uint8 source images")
    ap.add_argument("--config", default="rand-m9-mstd0.5-inc1")
    args = ap.parse_args()
    from VisionTransformer import config, data, vit
    from VisionTransformer.optim import cross_entropy, make_optimizer
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    cfg = config.ViTConfig.preset("base", img_size=S, batch_size=B, num_classes=1000, device="cpu",
                                  precision=torch.bfloat16)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(dev).train()
    opt = make_optimizer(model.parameters(), lr=1e-4, weight_decay=1e-4, device=dev)
    ds = data.SyntheticRawImages(4 * B, (args.src, args.src, 3), 1000, seed=1)
    batches = []
    for k in range(4):
        packed, meta, labels = data.collate_raw([ds[k * B + j] for j in range(B)])
        batches.append((packed.pin_memory(), meta, labels.pin_memory()))

    def transform(arm):
        ra = data.RandAugment.from_config(args.config, seed=0, rank=0) if arm == "randaug" else None
        return data.GpuTrainTransform(S, data.TrainAugment(erase_prob=0.25, seed=0, rank=0), mean=IMAGENET[0],
                                      std=IMAGENET[1], rand_augment=ra)
    tfs = {arm: transform(arm) for arm in ("augment", "randaug")}

    def run(arm):
        loss = None
        t0 = time.perf_counter()
        for i, (x, y) in enumerate(data.DeviceBatches(Cycle(batches, args.warmup + args.steps), tfs[arm], dev)):
            if i == args.warmup:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            loss = cross_entropy(model(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        last = float(loss.item())
        return (time.perf_counter() - t0) / max(args.steps, 1) * 1e3, last
    ms = {arm: [] for arm in tfs}
    for r in range(args.rounds):
        for arm in tfs:
            t, last = run(arm)
            ms[arm].append(t)
            print(json.dumps({"round": r, "arm": arm, "batch": B, "src": args.src, "warmup": args.warmup,
                              "steps": args.steps, "ms_per_step": round(t, 3), "final_loss": round(last, 5)}), flush=True)
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: max(v) - min(v) for arm, v in ms.items()}
    for arm in ms:
        print(f"{arm:8s} median {med[arm]:8.3f} ms/step, spread {spread[arm]:.3f} ms over {args.rounds} rounds")
    diff, lim = med["randaug"] - med["augment"], max(spread.values())
    print(f"randaug - augment: {diff:+.3f} ms/step; the larger spread is {lim:.3f} ms -> "
          f"{'inside the spread' if abs(diff) <= lim else 'OUTSIDE the spread'}")


if __name__ == "__main__":
    main()
