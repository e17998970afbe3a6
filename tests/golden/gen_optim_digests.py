"""SHA-256 digests of what three fused optimizer steps leave behind, through the public surface only (make_optimizer,
param_groups_layer_decay, ema_weights(), grad_norm(), skipped_steps(), trust_ratios()), so that this file runs
unchanged at any commit that has them.  tests/golden/optim_step_sha256.json is its output at the commit before the
optimizer's step paths were merged into one; tests/test_gpu_optim_bits.py recomputes the digests and compares, which
catches what a comparison of the code with itself (grouped against per-group) or with fp64 under a tolerance cannot: a
factor that the host now rounds differently.

A case is "<dtype>/<opt>/<variant>[/<extra>]":
  dtype    fp32 | bf16: the model's precision, hence the dtype of the engine's shadow weights
  opt      adamw | lamb
  variant  plain | clip_ema (max_grad_norm=1.0, ema_decay=0.9)
  extra    late   one parameter's first gradient arrives at step 2: per-count tables, and a grouped step falls back
           inf    (clip_ema) one infinite gradient element at step 2: a skipped step
           swap   (clip_ema) the weights and shadows inside ema_weights(), and again after it
           flags  (lamb) trust_clip=True, always_adapt=True
The model is the micro ViT (2 blocks, embedding 128), its engine built by one forward / backward; the groups are
param_groups_layer_decay(model, 0.05, 0.75) with a learning rate that differs per group and per step; the chunk is 64
elements, so tensors have several chunks and ragged tails; the gradients come from a seeded CPU generator.  After
the three steps the digest takes in, in named_parameters() order, the bytes of the parameter, exp_avg, exp_avg_sq, the
EMA, the shadow and LAMB's trust ratio, each where it exists, then for clip_ema grad_norm() and skipped_steps().
`fuse_groups` is not part of a case: off and on must give the same digest.

usage: python tests/golden/gen_optim_digests.py > tests/golden/optim_step_sha256.json      (needs the GPU)"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "vision-transformer_amd")) if p not in sys.path]

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STEPS, CHUNK, LATE = 3, 64, 5      # LATE: the index of the parameter whose first gradient comes at step 2
CASES = [f"{d}/{o}/{v}" for d in DTYPES for o in ("adamw", "lamb") for v in (
    "plain", "clip_ema", "plain/late", "clip_ema/late", "clip_ema/inf", "clip_ema/swap")]
CASES += [f"{d}/lamb/{v}/flags" for d in DTYPES for v in ("plain", "clip_ema")]


def _feed(h, t):
    h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())


def digest(case, fuse_groups, device="cuda"):
    """The hex digest of `case` with `fuse_groups` off or on."""
    from VisionTransformer import _ops, config, vit
    from VisionTransformer._engine import shadow_of
    from VisionTransformer.optim import cross_entropy, make_optimizer, param_groups_layer_decay

    dname, opt_name, variant, *extra = case.split("/")
    extra = extra[0] if extra else None
    clipped = variant == "clip_ema"
    chunk, _ops.CHUNK = _ops.CHUNK, CHUNK
    try:
        cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 2, precision=DTYPES[dname])
        torch.manual_seed(0)
        model = vit.VisionTransformer(cfg).to(device).eval()
        model.store_attention_probs = False        # whatever the automatic rule would choose for this batch
        g = torch.Generator().manual_seed(1)
        x, y = torch.randn(2, 3, 64, 64, generator=g).to(device), torch.randint(0, 10, (2,), generator=g).to(device)
        cross_entropy(model(x), y).backward()      # builds the engine: the shadows exist, the gradients are its views
        kw = dict(max_grad_norm=1.0, ema_decay=0.9) if clipped else {}
        if extra == "flags":
            kw.update(trust_clip=True, always_adapt=True)
        opt = make_optimizer(param_groups_layer_decay(model, 0.05, 0.75), lr=1e-2, weight_decay=0.05, device=device,
                             opt=opt_name, fuse_groups=fuse_groups, **kw)
        named = list(model.named_parameters())
        if extra == "late":
            named[LATE][1].grad = None
        h = hashlib.sha256()
        for step in range(1, STEPS + 1):
            for group in opt.param_groups:         # what a schedule does: another rate per group at every step
                group["lr"] = 1e-2 * group["lr_scale"] / step
            g = torch.Generator().manual_seed(100 + step)
            for i, (_, p) in enumerate(named):
                v = torch.randn(p.shape, generator=g)
                if extra == "inf" and step == 2 and i == 3:
                    v.view(-1)[v.numel() // 2] = float("inf")
                if extra == "late" and i == LATE and step < 2:
                    continue
                if p.grad is None:
                    p.grad = v.to(device)
                else:
                    p.grad.copy_(v)
            opt.step()
        ratios = opt.trust_ratios() if opt_name == "lamb" else {}
        for _, p in named:
            st = opt.state.get(p, {})
            for t in (p, st.get("exp_avg"), st.get("exp_avg_sq"), st.get("ema"), shadow_of(p), ratios.get(p)):
                if t is not None:
                    _feed(h, t)
        if clipped:
            _feed(h, opt.grad_norm())
            _feed(h, opt.skipped_steps())
        if extra == "swap":
            with opt.ema_weights():
                for _, p in named:
                    _feed(h, p)
                    if shadow_of(p) is not None:
                        _feed(h, shadow_of(p))
            for _, p in named:
                _feed(h, p)
                if shadow_of(p) is not None:
                    _feed(h, shadow_of(p))
        torch.cuda.synchronize()
        return h.hexdigest()
    finally:
        _ops.CHUNK = chunk


def toolchain():
    return {"torch": torch.__version__, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0)}


def main():
    out = {}
    for case in CASES:
        out[case] = digest(case, False)
        if digest(case, True) != out[case]:
            raise SystemExit(f"{case}: fuse_groups on and off disagree")
    print(json.dumps({"toolchain": toolchain(), "digests": out}, indent=1))


if __name__ == "__main__":
    main()
