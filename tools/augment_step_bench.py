"""Time whole training steps fed through data.DeviceBatches, with or without the training augmentation, for an
interleaved A/B (a fresh process per arm and round; one JSON line per run).

`train.py --bench` times one resident float batch and never enters the loader, so this tool times a fixed number of
train()-style steps instead: forward, loss, zero_grad, backward, optimizer step on the C2 configuration (ViT-B/16,
224 x 224, batch 256, bf16), every batch staged by DeviceBatches on its side stream one step ahead from synthetic-u8
input (32 x 32 x 3 uint8 images, four pre-collated pinned batches cycled, so that the host loader is not what is
timed).  Arm `plain`: GpuImageTransform(224).  Arm `augment`: GpuTrainTransform(224, TrainAugment(erase_prob=0.25),
ImageNet mean / std) — crop, flip 0.5, erase and normalize in the one launch.
usage: python tools/augment_step_bench.py {plain|augment} [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


class Cycle:
    """A loader of n batches that repeats a few pre-collated, pinned ones."""

    def __init__(self, batches, n):
        self.batches, self.n = batches, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.batches[i % len(self.batches)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("arm", choices=["plain", "augment"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
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
    ds = data.SyntheticRawImages(4 * B, (32, 32, 3), 1000, seed=1)
    batches = []
    for k in range(4):
        packed, meta, labels = data.collate_raw([ds[k * B + j] for j in range(B)])
        batches.append((packed.pin_memory(), meta, labels.pin_memory()))
    if args.arm == "plain":
        tf = data.GpuImageTransform(S)
    else:
        tf = data.GpuTrainTransform(S, data.TrainAugment(erase_prob=0.25, seed=0, rank=0), mean=IMAGENET[0],
                                    std=IMAGENET[1])
    loss = None
    t0 = time.perf_counter()
    for i, (x, y) in enumerate(data.DeviceBatches(Cycle(batches, args.warmup + args.steps), tf, dev)):
        if i == args.warmup:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        loss = cross_entropy(model(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    last = float(loss.item())
    sec = (time.perf_counter() - t0) / max(args.steps, 1)
    print(json.dumps({"arm": args.arm, "batch": B, "warmup": args.warmup, "steps": args.steps,
                      "ms_per_step": round(sec * 1e3, 3), "images_per_s": round(B / sec, 1),
                      "final_loss": round(last, 5)}), flush=True)


if __name__ == "__main__":
    main()
