"""Time the optimizer step over layer-wise learning-rate decay groups, one launch per group against one grouped launch,
as an interleaved A/B inside one process (one JSON line at the end), in the manner of tools/lamb_step_bench.py.

--mode opt (default): the optimizer alone.  One ViT-B/16 model (the C2 parameter set; 28 groups from
optim.param_groups_layer_decay), its engine built and its gradients made by one forward / backward, then nothing but
optimizer.step() calls.  Arms, each an optimizer of its own (own moments) over the same parameters and gradients:
  adamw/per_group   FusedAdamW over the 28 groups, fuse_groups off: 28 launches
  adamw/grouped     the same with fuse_groups: 1 launch (vit_adamw_groups)
  adamw/single      FusedAdamW over ONE group holding every parameter: the single-group kernel (vit_adamw)
  lamb/per_group, lamb/grouped: FusedLamb alike (84 launches against 3)
and every one of them again with max_grad_norm=1.0 (".../clip").  A round times --steps steps of each arm in turn
(order reversed every other round) after --warmup untimed ones; a round's time is wall clock between two device
synchronisations.  Reported per arm: the mean us/step over the rounds and the spread (max - min) of the rounds, the
ratios grouped / per_group and grouped / single, and "host": the part of a round's wall clock that passed before the
last step() returned, i.e. before the final synchronisation (close to the whole where the host, not the device, sets the
pace).  Last, "kernel": the launches alone, 28 groups through vit_adamw_groups against the single-group vit_adamw over
the same parameters, called back to back on the optimizers' own cached tables with no optimizer code in between.

--mode step: whole training steps (forward, loss, zero_grad, backward, step, schedule) at the C2 configuration (224 x
224, batch 256, bf16) under layer decay, fuse_groups on against off: ms/step and spread.
usage: python tools/opt_groups_bench.py [--mode opt|step] [--rounds 5] [--steps 50] [--warmup 5] [--batch N]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-transformer_amd"))


def kernels_alone(arms, rounds, n, dev):
    """us per launch of vit_adamw over the single-group table and of vit_adamw_groups over the merged one."""
    from VisionTransformer import _ops
    single, grouped = arms["adamw/single"][0], arms["adamw/grouped"][0]
    st, gt = single._tables[(0, "all")], grouped._tables[("groups", "all")]
    (span,) = gt.spans
    specs = [grouped._group_spec(group, 10) for group in grouped.param_groups]
    lr, b1, b2, eps, wd, bc1, bc2, _ = single._group_spec(single.param_groups[0], 10)
    run = {"adamw_single": lambda: _ops.adamw(st.dev_tab, st.nchunks, lr, b1, b2, eps, wd, bc1, bc2, 1.0,
                                              st.shadow_dtype),
           "adamw_grouped": lambda: _ops.adamw_groups(span.rows, span.group_of_chunk, span.c1 - span.c0, specs, 1.0,
                                                      gt.shadow_dtype)}
    us = {k: [] for k in run}
    for r in range(rounds):
        for name in (list(run) if r % 2 == 0 else list(run)[::-1]):
            for _ in range(5):
                run[name]()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                run[name]()
            torch.cuda.synchronize(dev)
            us[name].append((time.perf_counter() - t0) * 1e6 / n)
    mean = {k: sum(v) / len(v) for k, v in us.items()}
    return {"chunks": {"adamw_single": st.nchunks, "adamw_grouped": gt.nchunks},
            "per_launch": {k: round(v, 3) for k, v in mean.items()},
            "spread": {k: round(max(v) - min(v), 3) for k, v in us.items()},
            "grouped : single": round(mean["adamw_grouped"] / mean["adamw_single"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="opt", choices=["opt", "step"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=None, help="timed steps per arm and round (opt: 50, step: 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="opt: 32 (only the cls parameter depends on it); step: 256")
    ap.add_argument("--model", default="base")
    ap.add_argument("--layer-decay", type=float, default=0.75)
    args = ap.parse_args()
    from VisionTransformer import config, vit
    from VisionTransformer.optim import (FusedAdamW, FusedLamb, LRSchedule, cross_entropy, param_groups_layer_decay)
    dev = torch.device("cuda", 0)
    opt_mode = args.mode == "opt"
    B, S = args.batch or (32 if opt_mode else 256), 224
    nsteps = args.steps or (50 if opt_mode else 20)
    cfg = config.ViTConfig.preset(args.model, img_size=S, batch_size=B, num_classes=1000, device="cpu",
                                  precision=torch.bfloat16)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, S, S, generator=g).to(dev).bfloat16()
    y = torch.randint(0, 1000, (B,), generator=g).to(dev)

    def groups():
        return param_groups_layer_decay(model, 0.05, args.layer_decay)

    def make(cls, params, **kw):
        opt = cls(params, lr=1e-5, weight_decay=0.05, **kw)
        return opt, LRSchedule(opt, "constant", 0)            # applies every group's lr_scale

    arms = {}
    if opt_mode:
        for clip in (None, 1.0):
            tag = "/clip" if clip else ""
            arms["adamw/per_group" + tag] = make(FusedAdamW, groups(), max_grad_norm=clip)
            arms["adamw/grouped" + tag] = make(FusedAdamW, groups(), max_grad_norm=clip, fuse_groups=True)
            arms["adamw/single" + tag] = make(FusedAdamW, model.parameters(), max_grad_norm=clip)
            arms["lamb/per_group" + tag] = make(FusedLamb, groups(), max_grad_norm=clip)
            arms["lamb/grouped" + tag] = make(FusedLamb, groups(), max_grad_norm=clip, fuse_groups=True)
        cross_entropy(model(x), y).backward()                 # the engine, its shadows, and gradients to step on
    else:
        arms["per_group"] = make(FusedAdamW, groups())
        arms["grouped"] = make(FusedAdamW, groups(), fuse_groups=True)
    ngroups = len(groups())

    def steps(arm, n):
        opt, sched = arm
        loss = None
        for _ in range(n):
            if not opt_mode:
                loss = cross_entropy(model(x), y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
            opt.step()
            sched.step()
        return loss

    unit = 1e6 if opt_mode else 1e3
    t = {k: [] for k in arms}
    host = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            steps(arms[name], args.warmup)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            steps(arms[name], nsteps)
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            t[name].append((time.perf_counter() - t0) * unit / max(nsteps, 1))
            host[name].append((t1 - t0) * unit / max(nsteps, 1))
            print(f"{r + 1} [{name}] {t[name][-1]:.3f} {'us' if opt_mode else 'ms'}/step", file=sys.stderr, flush=True)
    mean = {k: sum(v) / len(v) for k, v in t.items()}
    out = {"mode": args.mode, "model": args.model, "batch": B, "groups": ngroups, "layer_decay": args.layer_decay,
           "rounds": args.rounds, "steps": nsteps, "warmup": args.warmup, "unit": "us" if opt_mode else "ms",
           "per_step": {k: round(mean[k], 3) for k in t},
           "spread": {k: round(max(v) - min(v), 3) for k, v in t.items()},
           "host": {k: round(sum(v) / len(v), 3) for k, v in host.items()},
           "rounds_per_step": {k: [round(a, 3) for a in v] for k, v in t.items()}}
    if opt_mode:
        out["kernel"] = kernels_alone(arms, args.rounds, nsteps, dev)
    ratio = {}
    for k in t:
        if "grouped" in k.split("/"):
            for other in ("per_group", "single"):
                o = k.replace("grouped", other)
                if o in mean:
                    ratio[f"{k} : {o}"] = round(mean[k] / mean[o], 4)
    out["ratio"] = ratio
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
