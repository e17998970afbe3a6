"""Time a validation pass with evaluate() and with validate(), as an interleaved A/B inside one process, and the metrics
kernels alone (one JSON line at the end), in the manner of tools/lamb_step_bench.py.

One ViT-B/16 model (224 x 224, batch 256, bf16: the C2 configuration) in eval mode and --batches device-resident
batches of synthetic images with pinned host labels (a pin_memory loader's), served by a list; an arm is the function
that scores them: train.evaluate(model, loader, accuracy_score), one argmax transfer and one scikit-learn call per
batch, or train.validate(model, loader), whose state stays on the device until its one read.  Each round runs one
whole pass of one arm, then of the other, after one untimed pass of each, so both arms see the same machine, clocks and
allocator state; a pass's time is wall clock between two device synchronisations.  Reported per arm: the mean
images/s over the rounds and the spread (max - min) of the rounds, and the two top-1 figures, which must agree.

Then vit_eval_update alone at (256, 1000) and (256, 10), maxk 5 with a confusion matrix: --launches calls between two
device events after --launches untimed ones, microseconds per call (two kernels).  --kernels-only runs just that
part, for a kernel trace.
usage: python tools/eval_bench.py [--rounds 4] [--batches 40] [--batch 256] [--model base] [--launches 200]
                                  [--kernels-only]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def kernel_us(rows, classes, launches, dev):
    from VisionTransformer import _ops
    g = torch.Generator().manual_seed(classes)
    lg = torch.randn(rows, classes, generator=g).to(dev)
    lb = torch.randint(0, classes, (rows,), generator=g).to(dev)
    maxk = min(5, classes)
    counts = torch.zeros(2 + maxk, dtype=torch.int64, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    cm = torch.zeros(classes, classes, dtype=torch.int64, device=dev)
    for _ in range(launches):
        _ops.eval_update(lg, lb, counts, loss, cm, maxk=maxk)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(launches):
        _ops.eval_update(lg, lb, counts, loss, cm, maxk=maxk)
    end.record()
    torch.cuda.synchronize(dev)
    assert int(counts[0]) == 2 * launches * rows
    return start.elapsed_time(end) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", default="base")
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true", help="only the kernel timing (what a kernel trace wants)")
    args = ap.parse_args()
    if args.kernels_only:
        dev = torch.device("cuda", 0)
        print(json.dumps({"eval_update_us_per_call": {f"{r}x{c}": round(kernel_us(r, c, args.launches, dev), 3)
                                                      for r, c in ((256, 1000), (256, 10))},
                          "launches": args.launches}), flush=True)
        return
    import train as T
    from sklearn.metrics import accuracy_score
    from VisionTransformer import config, vit
    dev = torch.device("cuda", 0)
    T.device = "cuda"
    B, S = args.batch, args.img
    cfg = config.ViTConfig.preset(args.model, img_size=S, batch_size=B, num_classes=args.classes, device="cpu",
                                  precision=torch.bfloat16)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    loader = [(torch.randn(B, 3, S, S, generator=g).to(dev).bfloat16(),
               torch.randint(0, args.classes, (B,), generator=g).pin_memory()) for _ in range(args.batches)]
    arms = {"evaluate": lambda: float(T.evaluate(model, loader, accuracy_score)),
            "validate": lambda: T.validate(model, loader, topk=(1, 5), confusion=True)["top1"]}
    images = B * args.batches
    ips = {k: [] for k in arms}
    top1 = {}
    for name, arm in arms.items():                                 # warm-up: every shape, both code paths
        arm()
    for r in range(args.rounds):
        for name in (("evaluate", "validate") if r % 2 == 0 else ("validate", "evaluate")):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            top1[name] = arms[name]()
            torch.cuda.synchronize(dev)
            ips[name].append(images / (time.perf_counter() - t0))
            print(f"{r + 1} [{name}] {ips[name][-1]:.1f} images/s", file=sys.stderr, flush=True)
    mean = {k: sum(v) / len(v) for k, v in ips.items()}
    kern = {f"{rows}x{classes}": round(kernel_us(rows, classes, args.launches, dev), 3)
            for rows, classes in ((256, 1000), (256, 10))}
    print(json.dumps({"model": args.model, "img": S, "batch": B, "batches": args.batches, "rounds": args.rounds,
                      "images_per_s": {k: round(mean[k], 1) for k in ips},
                      "spread_images_per_s": {k: round(max(v) - min(v), 1) for k, v in ips.items()},
                      "rounds_images_per_s": {k: [round(t, 1) for t in v] for k, v in ips.items()},
                      "validate_over_evaluate": round(mean["validate"] / mean["evaluate"], 4),
                      "top1": top1, "eval_update_us_per_call": kern, "launches": args.launches}), flush=True)


if __name__ == "__main__":
    main()
