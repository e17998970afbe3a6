"""What an attention-rollout map costs on top of a forward, and against the only way there was before: arms
interleaved inside one process, one JSON line at the end, in the manner of tools/eval_bench.py.

One ViT-B/16 model (224 x 224, bf16) in eval mode under no_grad and one device-resident batch per batch size.  Arms:
  at --small-batch (12: the largest batch whose probabilities the automatic budget stores)
    probs+host    a store_attention_probs=True forward, then rollout.rollout_from_probs on the stored tensors (device)
    rollout       model.attention_rollout(x): logits bitwise the probs forward's (its attention kernel, images in
                  chunks, probabilities dropped)
    rollout-fast  model.attention_rollout(x, fast_attention=True): the MFMA attention forward
  at --batch (256)
    forward       the plain eval forward, model(x) with store_attention_probs=False
    rollout, rollout-fast
    probs+host    as above, the probabilities forced on (12 x [B, H, T, T] fp32: 5.7 GB at B 256); --no-big-probs
                  leaves this arm out
Each round runs --iters calls of one arm, then of the next, after one untimed round, so all arms see the same machine,
clocks and allocator state; a call's time is wall clock between two device synchronisations over the iters.  Reported
per arm: the mean ms per call over the rounds and the spread (max - min) of the rounds.

Then vit_attn_rollout_step alone at the C2 shape (B 256, T 197, H 12, hd 64, bf16, mean) and at C5's (B 64, T 577),
each in both forms: --launches calls between two device events after as many untimed ones, microseconds per
call (two kernels).  --kernels-only runs just that part, for a kernel trace.
usage: python tools/rollout_bench.py [--rounds 4] [--iters 5] [--batch 256] [--small-batch 12] [--launches 50]
                                     [--no-big-probs] [--kernels-only]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def step_us(B, T, H, hd, form, launches, dev):
    from VisionTransformer import _ops
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).bfloat16().to(dev)
    pair = [torch.full((B, T), 1.0 / T, device=dev), torch.empty(B, T, device=dev)]
    ws = torch.empty(_ops.attn_rollout_workspace_bytes(B, T, H, hd, torch.bfloat16, 0) // 4, device=dev)

    def run():
        for i in range(launches):
            _ops.attn_rollout_step(qkv, pair[i & 1], B, T, H, hd, hd ** 0.5, 0, r_out=pair[1 - (i & 1)], workspace=ws,
                                   form=form)

    run()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    run()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) * 1e3 / launches


def kernels(launches, dev):
    from VisionTransformer import _lib
    return {"c2_b256_t197_mfma": round(step_us(256, 197, 12, 64, _lib.ROLLOUT_FORM_MFMA, launches, dev), 1),
            "c2_b256_t197_valu": round(step_us(256, 197, 12, 64, _lib.ROLLOUT_FORM_VALU, launches, dev), 1),
            "c5_b64_t577_mfma": round(step_us(64, 577, 12, 64, _lib.ROLLOUT_FORM_MFMA, launches, dev), 1),
            "c5_b64_t577_valu": round(step_us(64, 577, 12, 64, _lib.ROLLOUT_FORM_VALU, launches, dev), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--small-batch", type=int, default=12)
    ap.add_argument("--model", default="base")
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--no-big-probs", action="store_true", help="leave out the probs+host arm at --batch")
    ap.add_argument("--kernels-only", action="store_true", help="only the kernel timing (what a kernel trace wants)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.kernels_only:
        print(json.dumps({"rollout_step_us_per_call": kernels(args.launches, dev), "launches": args.launches}),
              flush=True)
        return
    from VisionTransformer import config, rollout, vit
    out = {"model": args.model, "img": args.img, "rounds": args.rounds, "iters": args.iters}
    for B in (args.small_batch, args.batch):
        cfg = config.ViTConfig.preset(args.model, img_size=args.img, batch_size=B, num_classes=1000, device="cpu",
                                      precision=torch.bfloat16)
        torch.manual_seed(0)
        model = vit.VisionTransformer(cfg).to(dev).eval()
        x = torch.randn(B, 3, args.img, args.img, generator=torch.Generator().manual_seed(1)).to(dev).bfloat16()
        blocks = model.transformer_encoder.blocks

        def probs_host():
            model.store_attention_probs = True
            logits = model(x)
            maps = rollout.rollout_from_probs([b.multi_head.attention_probs for b in blocks])
            for b in blocks:
                b.multi_head.attention_probs = None              # (the next call allocates them again)
            return logits, maps

        def forward():
            model.store_attention_probs = False
            return model(x), None

        arms = {"rollout": lambda: model.attention_rollout(x),
                "rollout-fast": lambda: model.attention_rollout(x, fast_attention=True)}
        if B == args.small_batch or not args.no_big_probs:
            arms["probs+host"] = probs_host
        if B == args.batch:
            arms["forward"] = forward
        times = {k: [] for k in arms}
        res = {}
        with torch.no_grad():
            for r in range(args.rounds + 1):
                for name, fn in arms.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        res[name] = fn()
                    torch.cuda.synchronize(dev)
                    if r:                                        # round 0 is untimed
                        times[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
        row = {k: {"ms": round(sum(v) / len(v), 3), "spread_ms": round(max(v) - min(v), 3)} for k, v in times.items()}
        if "probs+host" in res:                                   # the two routes agree (bf16 qkv, fp32 arithmetic)
            row["max_abs_diff_maps"] = float((res["probs+host"][1] - res["rollout"][1]).abs().max())
            row["logits_bitwise_equal"] = bool(torch.equal(res["probs+host"][0], res["rollout"][0]))
            row["max_abs_diff_maps_fast"] = float((res["rollout-fast"][1] - res["rollout"][1]).abs().max())
            row["max_abs_diff_logits_fast"] = float((res["rollout-fast"][0].float()
                                                     - res["rollout"][0].float()).abs().max())
        row["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
        out[f"B{B}"] = row
        print(f"B {B}: {row}", file=sys.stderr, flush=True)
        del model, x, res
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
    out["rollout_step_us_per_call"] = kernels(args.launches, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
