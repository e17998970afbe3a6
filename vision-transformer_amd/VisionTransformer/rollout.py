"""Attention rollout (Abnar & Zuidema 2020) from stored attention probabilities, in plain torch.

For block l = 1..L with probabilities P_l [B, H, T, T] (`multi_head.attention_probs`, transformer.py:48):
    F_l = fuse over heads of P_l                       (mean, max or min)
    A_l = (F_l + I) with every row divided by its sum  (the residual connection, rows re-normalised)
    R   = A_L A_{L-1} ... A_1 ;  map = R[token, :]
The map of one token needs no T x T product: it is the vector-matrix chain r_L = e_token,
    w = r / (1 + rowsum(F_l)),  r <- w F_l + w,   for l = L down to 1,
which `rollout_from_probs` evaluates in the dtype of its input.  It is the host path of
`VisionTransformer.attention_rollout` (a model on the CPU), the tool for anyone who already holds `attention_probs`,
and in fp64 the tests' twin of the device chain (`Engine.rollout`, vit_attn_rollout_step), which forms the same
vectors from each block's qkv without storing any P.

The classifier reads token 0 (the first patch: the reference appends the CLS token LAST, vit.py:41,80), so `token`
defaults to 0; the CLS token is index T - 1.
"""
import torch

HEAD_FUSIONS = ("mean", "max", "min")


def check_rollout_args(token, head_fusion, T):
    """`token` as an int in [0, T) and `head_fusion` one of HEAD_FUSIONS, or ValueError."""
    if isinstance(token, bool) or not isinstance(token, int) or not 0 <= token < T:
        raise ValueError(f"token must be an int in [0, {T}), got {token!r}")
    if head_fusion not in HEAD_FUSIONS:
        raise ValueError(f"head_fusion must be one of {HEAD_FUSIONS}, got {head_fusion!r}")
    return token


def fuse_heads(p, head_fusion):
    """[B, H, T, T] -> [B, T, T]."""
    if head_fusion == "mean":
        return p.mean(dim=1)
    return p.amax(dim=1) if head_fusion == "max" else p.amin(dim=1)


def rollout_step(p, r, head_fusion="mean"):
    """One step of the chain: r [B, T] through one block's probabilities p [B, H, T, T], in their dtype."""
    f = fuse_heads(p, head_fusion)
    w = r / (1 + f.sum(dim=-1))
    return torch.matmul(w.unsqueeze(1), f).squeeze(1) + w


def rollout_from_probs(probs, token=0, head_fusion="mean", return_layers=False):
    """The rollout map [B, T] of `token` from `probs`, a list of [B, H, T, T] tensors, first block to last.  With
    `return_layers` also [L, B, T]: entry l is the vector after block l's step (entry 0 is the map)."""
    probs = list(probs)
    if not probs:
        raise ValueError("rollout_from_probs: no attention probabilities (an empty list)")
    shape = probs[0].shape
    for p in probs:
        if not isinstance(p, torch.Tensor) or p.dim() != 4 or p.shape[2] != p.shape[3] or p.shape != shape:
            raise ValueError("rollout_from_probs: every entry must be a [B, H, T, T] tensor of one shape (a block "
                             "whose attention_probs is None was not stored: set model.store_attention_probs = True)")
    B, _, T, _ = shape
    token = check_rollout_args(token, head_fusion, T)
    r = torch.zeros(B, T, dtype=probs[0].dtype, device=probs[0].device)
    r[:, token] = 1
    layers = [None] * len(probs)
    for l in range(len(probs) - 1, -1, -1):
        r = rollout_step(probs[l], r, head_fusion)
        layers[l] = r
    return (r, torch.stack(layers)) if return_layers else r
