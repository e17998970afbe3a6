"""Generate tests/golden/rollout_micro.npz by importing the REFERENCE model (build container only, as gen_golden.py):
attention-rollout maps of the micro config (D 64, H 4, L 2, 32^2, B 4) under torch.manual_seed(0) on the synthetic
batch, from the reference module's own `.attention_probs`.  Run:  python tests/golden/gen_rollout_golden.py

Keys, for fuse in {mean, max, min} and token in {0, T - 1 = 4}:
  "{fuse}_{token}"        [B, T] fp64: row `token` of A_L ... A_1, A_l = (fuse_h P_l + I) with rows re-normalised,
                          from the reference module run in fp64
  "err32_{fuse}_{token}"  max |the same from the reference module run in fp32 (product in fp32) - the fp64 map|: the
                          measured term of the tests' gate
Nothing from the reference's source is stored: only outputs (data).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gen_golden import batch, ref_model   # noqa: E402  (imports the reference package)


def rollout(probs, token, fuse):
    R = None
    for p in probs:                        # first block to last: R <- A_l R
        f = {"mean": p.mean(1), "max": p.amax(1), "min": p.amin(1)}[fuse]
        a = f + torch.eye(f.shape[-1], dtype=f.dtype)
        a = a / a.sum(-1, keepdim=True)
        R = a if R is None else a @ R
    return R[:, token, :]


def main():
    D, H, L, img, B, nc = 64, 4, 2, 32, 4, 10
    x, _ = batch(B, 3, img, nc)
    probs = {}
    for dt in (torch.float64, torch.float32):
        m, _ = ref_model(D, H, L, img, B, nc)
        m = m.to(dt).eval()
        with torch.no_grad():
            m(x.to(dt))
        probs[dt] = [blk.multi_head.attention_probs.detach() for blk in m.transformer_encoder.blocks]
    T = probs[torch.float64][0].shape[-1]
    out = {}
    for fuse in ("mean", "max", "min"):
        for token in (0, T - 1):
            r64 = rollout(probs[torch.float64], token, fuse)
            r32 = rollout(probs[torch.float32], token, fuse)
            out[f"{fuse}_{token}"] = r64.numpy()
            out[f"err32_{fuse}_{token}"] = np.array(float((r32.double() - r64).abs().max()))
    np.savez_compressed(os.path.join(HERE, "rollout_micro.npz"), **out)
    print("rollout_micro.npz:", {k: (v.shape if v.ndim else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
