"""Host (CPU) path of the drop-in modules: what a model or module whose parameters live on the CPU runs.

The reference selects `device = 'cuda' if available else 'cpu'` (src/train.py:26) and trains wherever the model is
(train.py:80,89-96); BASELINE config 1 (ViT-Tiny/16 64^2 B8 fp32) is exactly that CPU run.  This module is the
package's own CPU implementation of the same arithmetic — NOT the oracle (oracle/ is test infrastructure and is never
imported here) and never a fallback for device tensors: it is reached only when both the input and the parameters
are CPU tensors (`vit.VisionTransformer.forward`, `_functional`).

It is written for the host's cores rather than mirrored from the reference's module structure:
  * the per-head key/query/value Linears of a block (transformer.py:12-18, one GEMM each per head) run as ONE GEMM
    against the concatenation of all heads' weights (rows: queries, keys, values), and the H per-head attention
    loops (transformer.py:44) as one batched scaled-dot-product attention with the reference's MULTIPLIED scale
    sqrt(hd) (transformer.py:24) — torch's fused CPU attention kernel;
  * `attention_probs` (transformer.py:48) is materialised as on the device path: per
    `model.wants_attention_probs(B)` (store_attention_probs, auto by size; [B, H, T, T] fp32 per block).
Standard autograd throughout, so requires_grad, hooks and torch DDP (gloo) behave as for any nn.Module.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import config as _config
from ._engine import site_seed

DROPOUT_P = 0.2          # transformer.py:35,53 (config.dropout is stored but unused by the reference)
LN_EPS = 1e-5


def _fused_qkv_weight(mh):
    """[3D, D]: query rows of every head, then keys, then values (the device engine's fused layout)."""
    heads = mh.heads
    return torch.cat([h.query.weight for h in heads] + [h.key.weight for h in heads] +
                     [h.value.weight for h in heads], dim=0)


def attention(a, w_qkv, H, want_probs=False):
    """softmax(q k^T * sqrt(hd)) v for all heads of a [B, T, D] input and fused weights [3*H*hd, D]; returns
    (o [B, T, H*hd], probs [B, H, T, T] or None)."""
    B, T, _ = a.shape
    hd = w_qkv.shape[0] // (3 * H)
    qkv = F.linear(a, w_qkv).view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)      # [3, B, H, T, hd]
    q, k, v = qkv[0], qkv[1], qkv[2]
    scale = float(hd) ** 0.5                                                  # multiplied (transformer.py:24)
    probs = None
    if want_probs:
        probs = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
        o = probs @ v
    else:
        o = F.scaled_dot_product_attention(q, k, v, scale=scale)
    return o.transpose(1, 2).reshape(B, T, H * hd), probs


def patch_embed(x, w, b, cls, pos, P):
    """Conv2d(k=s=P) -> flatten -> permute -> cat(CLS LAST) -> + pos (vit.py:21-29,39-42)."""
    e = F.conv2d(x.to(w.dtype), w, b, stride=P).flatten(2).transpose(1, 2)
    return torch.cat([e, cls.to(e.dtype)], dim=1) + pos


def drop_path(y, p, training):
    """Stochastic depth of a [B, T, D] branch output (timm's drop_path, scale_by_keep=True): image b's slab is kept
    and scaled by 1 / (1 - p) with probability 1 - p, else zeroed — one torch.rand(B, 1, 1) draw per call.  With
    p == 0 or outside training it returns y and draws nothing, so the CPU RNG stream (hence the dropout masks) of a
    rate-0 model is the one it always was."""
    if p == 0.0 or not training:
        return y
    keep = torch.rand(y.shape[0], 1, 1, device=y.device) >= p
    return (y / (1.0 - p)) * keep.to(y.dtype)


def patch_keep_table(seed, L, B, N, K):
    """Host twin of vit_patch_keep (vit_hip.h "Patch dropout"): (idx int32 [B, K], inv int32 [B, N]) for the forward
    seed `seed` (after dropout_seed) of a model with L blocks.  Key of patch n of image b: vit_hash_u32(site_seed(seed,
    2L, 0), b * N + n); patch 0 is kept, and patch n >= 1 iff fewer than K - 1 patches of 1 .. N-1 have a smaller
    (key, n) pair.  idx is ascending; inv[b, n] is the row of patch n or -1."""
    if not 1 <= K <= N:
        raise ValueError(f"patch_keep_table: need 1 <= K <= N, got K={K} N={N}")
    ps = np.uint64(site_seed(seed, 2 * L, 0))
    m32 = np.uint64(0xFFFFFFFF)
    ctr = (np.arange(B * N, dtype=np.uint64) & m32).reshape(B, N)
    x = (ctr * np.uint64(0x9E3779B1) + ps) & m32                    # the package's host hash (_engine._hash_u32),
    x ^= x >> np.uint64(16)                                         # over a whole table at once
    x = (x * np.uint64(0x85EBCA6B)) & m32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m32
    x ^= x >> np.uint64(16)
    pair = (x << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]      # (key, n), compared as one number
    keep = np.zeros((B, N), dtype=bool)
    keep[:, 0] = True
    if K > 1:
        order = np.argsort(pair[:, 1:], axis=1, kind="stable")[:, :K - 1] + 1
        np.put_along_axis(keep, order, True, axis=1)
    idx = np.nonzero(keep)[1].reshape(B, K).astype(np.int32)
    inv = np.where(keep, np.cumsum(keep, axis=1) - 1, -1).astype(np.int32)
    return torch.from_numpy(idx), torch.from_numpy(inv)


def check_keep_indices(keep, B, N):
    """A caller's keep table: int32 / int64 [B, K] with 1 <= K <= N (shape and dtype only: the entries — ascending,
    column 0 equal to 0 — are the caller's responsibility, so that a device table is never synchronised on).
    Returns K."""
    if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.int32, torch.int64):
        raise TypeError("keep_indices must be an int32 or int64 tensor")
    if keep.dim() != 2 or keep.shape[0] != B or not 1 <= keep.shape[1] <= N:
        raise ValueError(f"keep_indices must be [B, K] = [{B}, 1..{N}], got {tuple(keep.shape)}")
    return keep.shape[1]


def gather_tokens(e, idx):
    """The kept tokens of e [B, N + 1, D]: patches idx [B, K] in their order, then the CLS token (row N) — [B, K+1, D]."""
    B, T, D = e.shape
    rows = torch.cat([idx.to(torch.int64), torch.full((B, 1), T - 1, dtype=torch.int64, device=idx.device)], dim=1)
    return e.gather(1, rows[:, :, None].expand(-1, -1, D))


def block(blk, x, training, want_probs=False, drop_path_rate=0.0):
    """Pre-LN block (transformer.py:76-79): x + drop(proj(MHA(ln1 x))), then x + drop(FFN(ln2 x)); each branch
    under drop_path(., drop_path_rate)."""
    mh = blk.multi_head
    a = F.layer_norm(x, (x.shape[-1],), blk.ln1.weight, blk.ln1.bias, LN_EPS)
    o, probs = attention(a, _fused_qkv_weight(mh), len(mh.heads), want_probs)
    mh.attention_probs = probs.detach() if probs is not None else None
    x = x + drop_path(F.dropout(F.linear(o, mh.proj.weight, mh.proj.bias), DROPOUT_P, training), drop_path_rate,
                      training)
    fc1, _, fc2, _ = blk.ffwd.mlp
    a = F.layer_norm(x, (x.shape[-1],), blk.ln2.weight, blk.ln2.bias, LN_EPS)
    h = torch.relu(F.linear(a, fc1.weight, fc1.bias))
    return x + drop_path(F.dropout(F.linear(h, fc2.weight, fc2.bias), DROPOUT_P, training), drop_path_rate, training)


def vit_forward(model, x, training=None, want_probs=None, keep_indices=None):
    """VisionTransformer.forward (vit.py:77-80) on the host: embeddings -> L blocks -> classifier on token 0.
    `training` / `want_probs` other than None override model.training / model.wants_attention_probs for this call
    (VisionTransformer.attention_rollout: an eval forward that stores the probabilities, whatever the flags say).
    Patch dropout (training, model.patch_drop_rate > 0 or `keep_indices`): after + pos the blocks get the kept tokens
    alone; the table is patch_keep_table's under one seed drawn from the CPU RNG, as the device forward draws it —
    at rate 0 nothing is drawn, so the RNG stream is the one it always was."""
    training = model.training if training is None else training
    want_probs = model.wants_attention_probs(x.shape[0]) if want_probs is None else want_probs
    emb = model.emdeddings
    conv = emb.sequence[0]
    if x.shape[0] != emb.cls_tkn_embd.shape[0]:
        raise RuntimeError(f"batch size {x.shape[0]} != config.batch_size {emb.cls_tkn_embd.shape[0]} "
                           "(the CLS token parameter is batch-shaped)")
    e = patch_embed(x, conv.weight, conv.bias, emb.cls_tkn_embd, emb.pos_embd, conv.kernel_size[0])
    B, N = e.shape[0], e.shape[1] - 1
    rate = model.patch_drop_rate if training else 0.0
    if keep_indices is not None:
        if not training:
            raise ValueError("keep_indices: patch dropout is training-only (the model is in eval mode)")
        check_keep_indices(keep_indices, B, N)
        idx = keep_indices.to(torch.int32)
    elif rate > 0.0:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        idx = patch_keep_table(seed, len(model.transformer_encoder.blocks), B, N, _config.patch_keep_count(N, rate))[0]
    else:
        idx = None
    if idx is not None:
        e = gather_tokens(e, idx)
        model.last_patch_keep = idx
    rates = model.drop_path_rates
    for l, blk in enumerate(model.transformer_encoder.blocks):
        e = block(blk, e, training, want_probs, rates[l])
    fc0, _, ln, fc3 = model.mlp
    z = F.gelu(F.linear(e[:, 0, :], fc0.weight, fc0.bias))                  # token 0 = first PATCH (vit.py:80)
    z = F.layer_norm(z, (z.shape[-1],), ln.weight, ln.bias, LN_EPS)
    return F.linear(z, fc3.weight, fc3.bias)
