"""Tensor-level wrappers over the C-ABI (no autograd here).  Every function launches on the current HIP stream
(or `stream`) and returns immediately.  Shapes/dtypes are validated on the host; the kernels re-validate."""
import ctypes
import os
import struct

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, BF16, F32, FLAG_SHARED_CUS, MASK4  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dtype_code(t):
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype if isinstance(t, torch.Tensor) else t}; use float32 or bfloat16")


def _stream(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("VisionTransformer HIP path: tensors must live on a ROCm device (got CPU tensor); "
                               "the CPU restatement under oracle/ is test infrastructure, not a fallback")


def mask4_bytes(m, n):
    """Bytes of a VIT_MASK4 bit mask of an [m][n] tensor (include/vit_hip.h)."""
    return 4 * ((m + 3) // 4) * ((n + 3) // 4)


def mask4_empty(m, n, device):
    return torch.empty(mask4_bytes(m, n), dtype=torch.uint8, device=device)


# None, or a list: every gemm() then appends what the library says it launches for the call (vit_gemm_kernel_choice:
# the kernel generation and the 256x256 kernel's epilogue kind, _lib.EPI_*), so a test can tell which kernel a case —
# the engine's own launches included — really reached.  Off (None) it costs one comparison.
GEMM_CHOICE_LOG = None


def gemm(a, b, c, m, n, k, lda, ldb, ldc, a_kcontig=True, b_kcontig=True, alpha=1.0, beta=0.0, bias=None,
         act=ACT_NONE, aux=None, ldaux=0, res=None, ldres=0, res_rowmod=0, dropout_p=0.0, seed=0, split_k=1,
         out_group=(0, 0), workspace=None, colsum_part=None, mask_out=None, drop_row_stride=1, shared_cus=False,
         drop_row0=0, row_scale=None, stream=None):
    """C[i][j] = epi(alpha * sum_r A(i,r) B(j,r)); see include/vit_hip.h.  `shared_cus`: VIT_FLAG_SHARED_CUS (other
    kernels — RCCL collectives — may hold CUs meanwhile: no persistent grid).  `colsum_part` (f32, colsum_part_rows(m) x n)
    receives per-256-row-block column sums of C as stored — finish with colsum_finish.  `aux` may be a uint8 mask4
    tensor (the ReLU mask saved by the forward); `mask_out` (uint8, mask4_bytes(m, n)) receives C's mask4 (dropout
    keep bits when dropout_p > 0, else C > 0).  `drop_row_stride` S: output row i draws the dropout bits of row i*S of
    the full tensor (C = token-0 rows of it); `drop_row0` R0: row i draws those of row i + R0 (C = a row range of a
    larger tensor).  `row_scale` (f32, vit_gemm_rowscale): a per-row factor applied after the dropout, read at that same
    row index (i + R0) * S — 0 drops the row's branch and clears its mask_out bits (drop path).  Returns c."""
    _need_cuda(a, b, c, bias, aux, res, colsum_part, mask_out, row_scale)
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or not row_scale.is_contiguous():
            raise TypeError("gemm: row_scale must be contiguous float32")
        if row_scale.numel() <= (m - 1 + drop_row0) * max(drop_row_stride, 1):
            raise ValueError("gemm: row_scale does not reach the last row's index")
    if a.dtype != b.dtype:
        raise TypeError("gemm: A and B dtypes differ")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("gemm: bias must be float32")
    d = _lib.GemmDesc()
    d.a, d.b, d.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.m, d.n, d.k = m, n, k
    d.a_kcontig, d.b_kcontig = int(a_kcontig), int(b_kcontig)
    d.in_dtype, d.out_dtype = dtype_code(a), dtype_code(c)
    d.alpha, d.beta = alpha, beta
    d.bias = None if bias is None else bias.data_ptr()
    d.act = act
    if aux is not None:
        if aux.dtype == torch.uint8:
            if aux.numel() < mask4_bytes(m, n):
                raise ValueError("gemm: mask4 aux too small")
            d.aux, d.ldaux, d.aux_dtype = aux.data_ptr(), 0, MASK4
        else:
            d.aux, d.ldaux, d.aux_dtype = aux.data_ptr(), ldaux, dtype_code(aux)
    if mask_out is not None:
        if mask_out.dtype != torch.uint8 or mask_out.numel() < mask4_bytes(m, n):
            raise ValueError("gemm: mask_out must be uint8 with >= mask4_bytes(m, n) elements")
        d.mask_out = mask_out.data_ptr()
    d.dropout_row_stride = drop_row_stride
    d.flags = FLAG_SHARED_CUS if shared_cus else 0
    d.dropout_row0 = drop_row0
    if res is not None:
        d.res, d.ldres, d.res_rowmod, d.res_dtype = res.data_ptr(), ldres, res_rowmod, dtype_code(res)
    d.dropout_p, d.dropout_seed = dropout_p, seed & 0xFFFFFFFF
    d.split_k = split_k
    d.out_group_rows, d.out_group_stride = out_group
    if colsum_part is not None:
        if colsum_part.dtype != torch.float32 or colsum_part.numel() < colsum_part_rows(m) * n:
            raise ValueError("gemm: colsum_part must be float32 with >= ceil(m/256)*n elements")
        d.colsum_part = colsum_part.data_ptr()
    # split-K slabs (split_k > 1), or the slabs of the split-K tail of the last partial round of tiles
    need = _lib.load().vit_gemm_workspace_bytes(ctypes.byref(d))
    if need > 0:
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(need // 4 + 1, dtype=torch.float32, device=c.device)
            if stream is not None:
                workspace.record_stream(stream)      # freed on return: not reusable before `stream` is done with it
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if GEMM_CHOICE_LOG is not None:
        impl, kind = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().vit_gemm_kernel_choice(ctypes.byref(d), _ptr(row_scale), ctypes.byref(impl),
                                                      ctypes.byref(kind)), "vit_gemm_kernel_choice")
        GEMM_CHOICE_LOG.append({"m": m, "n": n, "k": k, "row_scale": row_scale is not None, "impl": impl.value,
                                "kind": kind.value})
    if row_scale is not None:
        _lib.check(_lib.load().vit_gemm_rowscale(ctypes.byref(d), _ptr(row_scale), _stream(stream)),
                   "vit_gemm_rowscale")
        return c
    _lib.check(_lib.load().vit_gemm(ctypes.byref(d), _stream(stream)), "vit_gemm")
    return c


def drop_path_rows(seed, rates, B, T, device, out=None, stream=None):
    """The drop-path factor table of one forward (vit_drop_path_rows): float32 [L, 2, B*T], entry (l, site, b*T + t) =
    1 / (1 - rates[l]) where image b keeps its (l, site) branch, else 0.  `rates`: L host floats, passed in the kernel
    arguments (no upload, no sync)."""
    L = len(rates)
    if L > _lib.DROP_PATH_MAX_LAYERS:
        raise ValueError(f"drop_path_rows: {L} layers exceed the library's {_lib.DROP_PATH_MAX_LAYERS}")
    out = torch.empty(L, 2, B * T, dtype=torch.float32, device=device) if out is None else out
    _need_cuda(out)
    arr = (ctypes.c_float * L)(*rates)
    _lib.call("vit_drop_path_rows", _ptr(out), seed & 0xFFFFFFFF, L, B, T, arr, _stream(stream))
    return out


def colsum_part_rows(m):
    """Rows of a GEMM's colsum_part: one per 256-row block of C."""
    return (m + 255) // 256


def linear(x2d, w, bias=None, out_dtype=None, act=ACT_NONE, **kw):
    """y = act(x @ w^T + bias) for row-major x [M,K], w [N,K]."""
    M, K = x2d.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=out_dtype or x2d.dtype, device=x2d.device)
    return gemm(x2d, w, y, M, N, K, x2d.stride(0), w.stride(0), N, bias=bias, act=act, **kw)


def im2col(x, P, dtype, stream=None, cols=None):
    _need_cuda(x)
    B, C, H, W = x.shape
    n = (H // P) * (W // P)
    cols = torch.empty(B * n, C * P * P, dtype=dtype, device=x.device) if cols is None else cols
    _lib.call("vit_im2col", _ptr(x), dtype_code(x), _ptr(cols), dtype_code(dtype), B, C, H, W, P, _stream(stream))
    return cols


def col2im(cols, x, P, stream=None):
    """Inverse of im2col for k = s = P (a permutation): x[B, C, H, W] <- cols[B*N, C*P*P] (input-image gradient)."""
    _need_cuda(cols, x)
    B, C, H, W = x.shape
    _lib.call("vit_col2im", _ptr(cols), dtype_code(cols), _ptr(x), dtype_code(x), B, C, H, W, P, _stream(stream))
    return x


def embed_cls(cls, pos, x0, B, T, D, stream=None):
    _lib.call("vit_embed_cls", _ptr(cls), _ptr(pos), _ptr(x0), dtype_code(x0), B, T, D, _stream(stream))


# ---- patch dropout (vit_hip.h "Patch dropout"): the keep table and the gathering / scattering embedding kernels
def _check_table(t, B, n, what):
    if t.dtype != torch.int32 or tuple(t.shape) != (B, n) or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous int32 [{B}, {n}] tensor, got {t.dtype} {tuple(t.shape)}")


def patch_keep(seed, L, B, N, K, device, idx=None, inv=None, stream=None):
    """(idx int32 [B, K], inv int32 [B, N]) of vit_patch_keep: the K kept patches of every image in ascending order
    (column 0 is patch 0) and, per patch, its row or -1.  No host sync."""
    idx = torch.empty(B, K, dtype=torch.int32, device=device) if idx is None else idx
    inv = torch.empty(B, N, dtype=torch.int32, device=device) if inv is None else inv
    _need_cuda(idx, inv)
    _check_table(idx, B, K, "patch_keep: idx")
    _check_table(inv, B, N, "patch_keep: inv")
    _lib.call("vit_patch_keep", seed & 0xFFFFFFFF, L, B, N, K, _ptr(idx), _ptr(inv), _stream(stream))
    return idx, inv


def im2col_gather(x, P, dtype, idx, cols=None, stream=None):
    """im2col of the patches idx [B, K] names: cols [B*K, C*P*P], row b*K + j from patch idx[b, j]."""
    _need_cuda(x, idx)
    B, C, H, W = x.shape
    K = idx.shape[1]
    _check_table(idx, B, K, "im2col_gather: idx")
    cols = torch.empty(B * K, C * P * P, dtype=dtype, device=x.device) if cols is None else cols
    if cols.numel() != B * K * C * P * P or not cols.is_contiguous() or not x.is_contiguous():
        raise ValueError("im2col_gather: x must be contiguous and cols a contiguous [B*K, C*P*P]")
    _lib.call("vit_im2col_gather", _ptr(x), dtype_code(x), _ptr(cols), dtype_code(cols), _ptr(idx), B, C, H, W, P, K,
              _stream(stream))
    return cols


def gather_pos(pos, idx, N, out=None, stream=None):
    """float32 [B*K, D]: row b*K + j = pos[idx[b, j]] (pos: float32 [>= N, D], contiguous)."""
    _need_cuda(pos, idx)
    B, K = idx.shape
    D = pos.shape[-1]
    _check_table(idx, B, K, "gather_pos: idx")
    if pos.dtype != torch.float32 or not pos.is_contiguous() or pos.numel() < N * D:
        raise TypeError("gather_pos: pos must be contiguous float32 with at least N rows")
    out = torch.empty(B * K, D, dtype=torch.float32, device=pos.device) if out is None else out
    if out.dtype != torch.float32 or out.numel() != B * K * D or not out.is_contiguous():
        raise TypeError("gather_pos: out must be contiguous float32 [B*K, D]")
    _lib.call("vit_gather_pos", _ptr(pos), _ptr(idx), _ptr(out), B, N, K, D, _stream(stream))
    return out


def pos_grad_gather(dx, inv, K, gpos, beta=0.0, stream=None):
    """gpos [N+1, D] (float32) = beta * gpos + per position the sum of its rows of dx [B*(K+1), D] over the images that
    kept it (inv [B, N]); position N sums the CLS rows.  Deterministic."""
    _need_cuda(dx, inv, gpos)
    B, N = inv.shape
    D = dx.shape[-1]
    _check_table(inv, B, N, "pos_grad_gather: inv")
    if not dx.is_contiguous() or dx.numel() != B * (K + 1) * D:
        raise ValueError("pos_grad_gather: dx must be a contiguous [B*(K+1), D]")
    if gpos.dtype != torch.float32 or not gpos.is_contiguous() or gpos.numel() != (N + 1) * D:
        raise TypeError("pos_grad_gather: gpos must be contiguous float32 with (N+1)*D elements")
    _lib.call("vit_pos_grad_gather", _ptr(dx), dtype_code(dx), _ptr(inv), _ptr(gpos), B, N, K, D, float(beta),
              _stream(stream))
    return gpos


def col2im_scatter(cols, inv, K, x, P, stream=None):
    """col2im of gathered cols [B*K, C*P*P]: patch n of image b from row b*K + inv[b, n], zeros where inv < 0."""
    _need_cuda(cols, inv, x)
    B, C, H, W = x.shape
    _check_table(inv, B, (H // P) * (W // P), "col2im_scatter: inv")
    if not cols.is_contiguous() or cols.numel() != B * K * C * P * P or not x.is_contiguous():
        raise ValueError("col2im_scatter: cols must be a contiguous [B*K, C*P*P] and x contiguous")
    _lib.call("vit_col2im_scatter", _ptr(cols), dtype_code(cols), _ptr(inv), _ptr(x), dtype_code(x), B, C, H, W, P, K,
              _stream(stream))
    return x


def layernorm_fwd(x2d, gamma, beta, y=None, eps=1e-5, stream=None, mean=None, rstd=None):
    _need_cuda(x2d, gamma, beta)
    rows, cols = x2d.shape
    y = torch.empty_like(x2d) if y is None else y
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device) if mean is None else mean
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device) if rstd is None else rstd
    _lib.call("vit_layernorm_fwd", _ptr(x2d), x2d.stride(0), _ptr(gamma), _ptr(beta), _ptr(y), y.stride(0),
              _ptr(mean), _ptr(rstd), rows, cols, eps, dtype_code(x2d), _stream(stream))
    return y, mean, rstd


def layernorm_bwd_parts(rows, cols):
    return _lib.load().vit_layernorm_bwd_parts(rows, cols)


def layernorm_bwd(dy, x, gamma, mean, rstd, dx_out, dres=None, drop_out=None, drop_p=0.0, drop_seed=0,
                  partial=None, osum=False, drop_mask=None, stream=None):
    """dx_out = LN_bwd(dy) (+ dres); drop_out = dx_out * keep (UNSCALED: consumers multiply by 1/(1-p)); returns
    partial [2, parts, cols] f32 (dgamma / dbeta per workgroup) — [3, parts, cols] with `osum`: + the column sums of
    the gradient the next Linear sees (drop_out / (1-p) when given, else dx_out), i.e. its bias gradient.  Reduce
    with colsum_finish.  `drop_mask` (uint8 mask4): the keep bits saved by the forward, instead of the hash."""
    rows, cols = x.shape
    if drop_mask is not None and (drop_mask.dtype != torch.uint8 or drop_mask.numel() < mask4_bytes(rows, cols)):
        raise ValueError("layernorm_bwd: drop_mask must be uint8 with >= mask4_bytes(rows, cols) elements")
    parts = layernorm_bwd_parts(rows, cols)
    if partial is None:
        partial = torch.empty(3 if osum else 2, parts, cols, dtype=torch.float32, device=x.device)
    _lib.call("vit_layernorm_bwd", _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(gamma), _ptr(mean), _ptr(rstd),
              _ptr(dres), _ptr(dx_out), _ptr(drop_out), drop_p, drop_seed & 0xFFFFFFFF, _ptr(drop_mask), _ptr(partial),
              int(bool(osum)),
              rows, cols, dtype_code(x), _stream(stream))
    return partial


def attn_fwd(qkv, B, T, H, hd, scale, o=None, lse=None, probs=None, o32=None, max_wgs=0, stream=None):
    """o = softmax(scale Q K^T) V per head; `o32` (bf16 only): also store O unrounded (fp32) for attn_bwd's delta
    where attn_bwd_uses_o32() says the backward takes it.  `max_wgs` > 0: at most that many workgroups for the
    persistent ring forward, for this call only (0: automatic / the library option)."""
    _need_cuda(qkv)
    D = H * hd
    o = torch.empty(B * T, D, dtype=qkv.dtype, device=qkv.device) if o is None else o
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device) if lse is None else lse
    _lib.call("vit_attn_fwd", _ptr(qkv), _ptr(o), _ptr(o32), _ptr(lse), _ptr(probs), B, T, H, hd, scale,
              dtype_code(qkv), int(max_wgs), _stream(stream))
    return o, lse


def attn_bwd_uses_o32(B, T, H, hd, dtype):
    """True when attn_bwd at this shape forms delta from the forward's fp32 O (the tiled T > 256 path); the fused
    T <= 256 backward forms it from P and dP itself and reads neither O nor o32."""
    return bool(_lib.load().vit_attn_bwd_uses_o32(B, T, H, hd, dtype_code(dtype)))


def attn_bwd_workspace_bytes(B, T, H, hd, dtype):
    return _lib.load().vit_attn_bwd_workspace_bytes(B, T, H, hd, dtype_code(dtype))


def attn_bwd(qkv, o, d_o, lse, B, T, H, hd, scale, dqkv=None, workspace=None, o32=None, shared_cus=False,
             stream=None):
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    need = attn_bwd_workspace_bytes(B, T, H, hd, qkv.dtype)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=qkv.device)
    _lib.call("vit_attn_bwd", _ptr(qkv), _ptr(o), _ptr(o32), _ptr(d_o), _ptr(lse), _ptr(dqkv), B, T, H, hd, scale,
              dtype_code(qkv), _ptr(workspace), FLAG_SHARED_CUS if shared_cus else 0, _stream(stream))
    return dqkv


def attn_fwd_row0(qkv, B, T, H, hd, scale, o=None, lse=None, stream=None):
    """Attention output row 0 of every image (vit_attn_fwd_row0): o rows b*T and lse[b][h][0] are written, the other
    rows / entries are left as they are (o and lse may be fresh, uninitialised tensors)."""
    _need_cuda(qkv)
    D = H * hd
    o = torch.empty(B * T, D, dtype=qkv.dtype, device=qkv.device) if o is None else o
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device) if lse is None else lse
    _lib.call("vit_attn_fwd_row0", _ptr(qkv), _ptr(o), _ptr(lse), B, T, H, hd, scale, dtype_code(qkv), _stream(stream))
    return o, lse


def attn_bwd_row0(qkv, d_o0, ldo, dqkv, B, T, H, hd, scale, stream=None):
    """Backward of attn_fwd_row0 from the row-0 output gradients d_o0 (image b at row b, stride ldo): dQ row 0 and all
    of dK, dV into dqkv (dQ rows 1..T-1 untouched)."""
    _need_cuda(qkv, d_o0, dqkv)
    _lib.call("vit_attn_bwd_row0", _ptr(qkv), _ptr(d_o0), ldo, _ptr(dqkv), B, T, H, hd, scale,
              dtype_code(qkv), _stream(stream))
    return dqkv


ROLLOUT_FUSE = {"mean": _lib.ROLLOUT_MEAN, "max": _lib.ROLLOUT_MAX, "min": _lib.ROLLOUT_MIN}


def attn_rollout_workspace_bytes(B, T, H, hd, dtype, fuse):
    return _lib.load().vit_attn_rollout_workspace_bytes(B, T, H, hd, dtype_code(dtype), fuse)


def attn_rollout_step(qkv, r_in, B, T, H, hd, scale, fuse, r_out=None, workspace=None, form=_lib.ROLLOUT_FORM_AUTO,
                      stream=None):
    """One step of the attention-rollout chain (vit_attn_rollout_step): r_out[B][T] (fp32) from r_in[B][T] (fp32) and
    one block's qkv[B*T][3*H*hd]; `fuse` is a ROLLOUT_FUSE value.  r_out must not be r_in.  `form` other than automatic
    goes through vit_attn_rollout_step_form (A/B runs and tests)."""
    _need_cuda(qkv, r_in, r_out, workspace)
    if r_in.dtype != torch.float32 or not r_in.is_contiguous() or r_in.numel() != B * T:
        raise ValueError("attn_rollout_step: r_in must be a contiguous float32 [B, T] tensor")
    r_out = torch.empty(B, T, dtype=torch.float32, device=qkv.device) if r_out is None else r_out
    if r_out.dtype != torch.float32 or not r_out.is_contiguous() or r_out.numel() != B * T:
        raise ValueError("attn_rollout_step: r_out must be a contiguous float32 [B, T] tensor")
    if not qkv.is_contiguous() or qkv.numel() != B * T * 3 * H * hd:
        raise ValueError("attn_rollout_step: qkv must be a contiguous [B*T, 3*H*hd] tensor")
    need = attn_rollout_workspace_bytes(B, T, H, hd, qkv.dtype, fuse)
    if workspace is None:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=qkv.device)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"attn_rollout_step: workspace holds {workspace.numel() * workspace.element_size()} bytes, "
                         f"the step needs {need}")
    if form == _lib.ROLLOUT_FORM_AUTO:
        _lib.call("vit_attn_rollout_step", _ptr(qkv), _ptr(r_in), _ptr(r_out), B, T, H, hd, scale, dtype_code(qkv),
                  fuse, _ptr(workspace), _stream(stream))
    else:
        _lib.call("vit_attn_rollout_step_form", _ptr(qkv), _ptr(r_in), _ptr(r_out), B, T, H, hd, scale,
                  dtype_code(qkv), fuse, form, _ptr(workspace), _stream(stream))
    return r_out


def colsum(x, rows, cols, ldx, out, beta=0.0, workspace=None, alpha=1.0, stream=None):
    need = _lib.load().vit_colsum_workspace_bytes(rows, cols)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=x.device)
    _lib.call("vit_colsum", _ptr(x), ldx, dtype_code(x), rows, cols, _ptr(out), alpha, beta, _ptr(workspace),
              _stream(stream))
    return out


def colsum_finish(part, outs, beta=0.0, stream=None):
    """outs[s] = beta * outs[s] + sum_p part[s][p] (fixed order) for s < len(outs) <= 3 — the second stage of the
    column sums vit_gemm (colsum_part) and vit_layernorm_bwd produce.  part: [sets, nparts, cols] or [nparts, cols]."""
    p3 = part if part.dim() == 3 else part.unsqueeze(0)
    n = len(outs)
    if not 1 <= n <= min(3, p3.shape[0]):
        raise ValueError(f"colsum_finish: {n} outputs for {p3.shape[0]} partial sets")
    for t in outs:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p3.shape[2]:
            raise ValueError("colsum_finish: outputs must be contiguous float32 of length cols")
    ptrs = [_ptr(t) for t in outs] + [None] * (3 - n)
    _lib.call("vit_colsum_finish", _ptr(p3), p3.shape[1], p3.shape[2], n, *ptrs, beta, _stream(stream))
    return outs


def colsum_finish_batch(jobs, stream=None):
    """Several colsum_finish jobs [(part, outs, beta), ...] (<= 8) in one launch; each job's outputs are bitwise what
    colsum_finish(part, outs, beta) gives."""
    if not 1 <= len(jobs) <= 8:
        raise ValueError("colsum_finish_batch: 1..8 jobs")
    arr = (_lib.ColsumJob * len(jobs))()
    for i, (part, outs, beta) in enumerate(jobs):
        p3 = part if part.dim() == 3 else part.unsqueeze(0)
        n = len(outs)
        if not 1 <= n <= min(3, p3.shape[0]) or not p3.is_contiguous() or p3.dtype != torch.float32:
            raise ValueError(f"colsum_finish_batch: job {i}: {n} outputs for {p3.shape[0]} partial sets")
        for t in outs:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p3.shape[2]:
                raise ValueError("colsum_finish_batch: outputs must be contiguous float32 of length cols")
        arr[i].part, arr[i].nparts, arr[i].cols, arr[i].nsets = _ptr(p3), p3.shape[1], p3.shape[2], n
        for s_, t in enumerate(outs):
            arr[i].out[s_] = _ptr(t)
        arr[i].beta = beta
    _lib.call("vit_colsum_finish_batch", arr, len(jobs), _stream(stream))


def copy2d(src, lds, dst, ldd, rows, cols, group=(0, 0), beta=0.0, stream=None):
    _lib.call("vit_copy2d", _ptr(src), lds, dtype_code(src), _ptr(dst), ldd, dtype_code(dst), rows, cols, group[0],
              group[1], beta, _stream(stream))
    return dst


def dropout_bwd(x, y, p, seed, scale=None, stream=None):
    """y = x * keep * scale (scale defaults to 1/(1-p))."""
    scale = 1.0 / (1.0 - p) if scale is None else scale
    _lib.call("vit_dropout_bwd", _ptr(x), _ptr(y), dtype_code(x), x.numel(), p, seed & 0xFFFFFFFF, scale,
              _stream(stream))
    return y


def mask4_apply(x, y, mask, scale=1.0, stream=None):
    """y = x * mask4 bit * scale for 2-D x, y (any float dtypes, row strides allowed)."""
    _need_cuda(x, y, mask)
    rows, cols = x.shape
    if mask.dtype != torch.uint8 or mask.numel() < mask4_bytes(rows, cols) or tuple(y.shape) != (rows, cols):
        raise ValueError("mask4_apply: bad mask or output shape")
    _lib.call("vit_mask4_apply", _ptr(x), x.stride(0), dtype_code(x), _ptr(y), y.stride(0), dtype_code(y), _ptr(mask),
              rows, cols, scale, _stream(stream))
    return y


def relu_bwd(dy, y, dx=None, stream=None):
    dx = torch.empty_like(dy) if dx is None else dx
    _lib.call("vit_relu_bwd", _ptr(dy), _ptr(y), _ptr(dx), dtype_code(dy), dy.numel(), _stream(stream))
    return dx


def gelu_fwd(x, y=None, stream=None):
    y = torch.empty_like(x) if y is None else y
    _lib.call("vit_gelu_fwd", _ptr(x), _ptr(y), x.numel(), _stream(stream))
    return y


def gelu_bwd(x, dy, dx=None, stream=None):
    dx = torch.empty_like(x) if dx is None else dx
    _lib.call("vit_gelu_bwd", _ptr(x), _ptr(dy), _ptr(dx), x.numel(), _stream(stream))
    return dx


def softmax_xent(logits, labels, stream=None):
    """Returns (loss [1] f32, dlogits [rows, classes] f32 = d(mean loss)/dlogits)."""
    _need_cuda(logits, labels)
    rows, classes = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.call("vit_softmax_xent", _ptr(logits), _ptr(labels), rows, classes, _ptr(loss), _ptr(dlogits), _ptr(ws),
              _stream(stream))
    return loss, dlogits


def softmax_xent_mixed(logits, labels_a, labels_b=None, lam=None, smoothing=0.0, stream=None):
    """vit_softmax_xent_mixed: softmax_xent against the target (1 - smoothing) * (lam * onehot(a) + (1 - lam) *
    onehot(b)) + smoothing / classes, which is never built.  `labels_b` int64 [rows] and `lam` float32 [rows] (the
    weight of `labels_a`) on the logits' device, or both None.  Returns (loss [1] f32, dlogits [rows, classes] f32)."""
    _need_cuda(logits, labels_a, labels_b, lam)
    rows, classes = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be contiguous float32")
    for name, t, dt in (("labels_a", labels_a, torch.int64), ("labels_b", labels_b, torch.int64),
                        ("lam", lam, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != rows or not t.is_contiguous()
                              or t.device != logits.device):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of {rows} elements on the logits' device")
    if lam is not None and labels_b is None:
        raise ValueError("lam given without labels_b")
    if not 0.0 <= smoothing < 1.0:
        raise ValueError(f"label smoothing must lie in [0, 1) (got {smoothing!r})")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.call("vit_softmax_xent_mixed", _ptr(logits), _ptr(labels_a), _ptr(labels_b), _ptr(lam), float(smoothing),
              rows, classes, _ptr(loss), _ptr(dlogits), _ptr(ws), _stream(stream))
    return loss, dlogits


DISTILL_KINDS = {"soft": _lib.DISTILL_SOFT, "hard": _lib.DISTILL_HARD}


def check_distill_args(kind, alpha, tau):
    """ValueError unless `kind` is "soft" / "hard", 0 <= alpha <= 1 and tau is finite and positive (the conditions of
    vit_softmax_xent_distill, checked before any launch)."""
    if kind not in DISTILL_KINDS:
        raise ValueError(f"distillation kind must be 'soft' or 'hard' (got {kind!r})")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distillation alpha must lie in [0, 1] (got {alpha!r})")
    if not (0.0 < tau < float("inf")):
        raise ValueError(f"distillation tau must be finite and positive (got {tau!r})")


def softmax_xent_distill(logits, teacher_logits, labels_a, labels_b=None, lam=None, smoothing=0.0, kind="soft",
                         alpha=0.5, tau=1.0, stream=None):
    """vit_softmax_xent_distill: (1 - alpha) * softmax_xent_mixed's loss + alpha * the distillation term against
    `teacher_logits` (float32, the logits' shape and device): kind "soft" tau^2 * KL(softmax(z / tau) || softmax(x /
    tau)) with batchmean reduction, kind "hard" the cross entropy against the teacher's lowest arg max.  Labels as
    softmax_xent_mixed takes them.  Returns (loss [1] f32, dlogits [rows, classes] f32); no gradient for the teacher."""
    _need_cuda(logits, teacher_logits, labels_a, labels_b, lam)
    check_distill_args(kind, alpha, tau)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous float32 [rows, classes] tensor")
    rows, classes = logits.shape
    if (teacher_logits.shape != logits.shape or teacher_logits.dtype != torch.float32
            or not teacher_logits.is_contiguous() or teacher_logits.device != logits.device):
        raise ValueError(f"teacher_logits must be a contiguous float32 tensor of shape {tuple(logits.shape)} on the "
                         f"logits' device (got {tuple(teacher_logits.shape)}, {teacher_logits.dtype})")
    for name, t, dt in (("labels_a", labels_a, torch.int64), ("labels_b", labels_b, torch.int64),
                        ("lam", lam, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != rows or not t.is_contiguous()
                              or t.device != logits.device):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of {rows} elements on the logits' device")
    if lam is not None and labels_b is None:
        raise ValueError("lam given without labels_b")
    if not 0.0 <= smoothing < 1.0:
        raise ValueError(f"label smoothing must lie in [0, 1) (got {smoothing!r})")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.call("vit_softmax_xent_distill", _ptr(logits), _ptr(teacher_logits), _ptr(labels_a), _ptr(labels_b),
              _ptr(lam), float(smoothing), DISTILL_KINDS[kind], float(alpha), float(tau), rows, classes, _ptr(loss),
              _ptr(dlogits), _ptr(ws), _stream(stream))
    return loss, dlogits


def eval_update(logits, labels, counts, loss_sum, confusion=None, rows=None, maxk=None, stream=None):
    """vit_eval_update: score the first `rows` rows of `logits` (float32 [R, classes], unit column stride, any row
    stride) against `labels` (int64, at least `rows` of them) and ACCUMULATE into `counts` (int64 [2 + maxk]),
    `loss_sum` (float64 [1]) and `confusion` (int64 [classes, classes] or None).  Returns the call's (pred int64
    [rows], rank int32 [rows], row_loss float32 [rows]); nothing reaches the host."""
    _need_cuda(logits, labels, counts, loss_sum, confusion)
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise ValueError("logits must be a float32 [rows, classes] tensor with unit column stride")
    classes = logits.shape[1]
    rows = logits.shape[0] if rows is None else int(rows)
    ld = logits.stride(0) if logits.shape[0] > 1 else classes
    maxk = counts.numel() - 2 if maxk is None else int(maxk)
    if not 0 < rows <= logits.shape[0] or labels.dim() != 1 or labels.numel() < rows:
        raise ValueError(f"rows = {rows} needs that many rows of logits and labels (got {logits.shape[0]}, "
                         f"{labels.numel()})")
    for name, t, dt, n in (("labels", labels, torch.int64, rows), ("counts", counts, torch.int64, 2 + maxk),
                           ("loss_sum", loss_sum, torch.float64, 1),
                           ("confusion", confusion, torch.int64, classes * classes)):
        if t is not None and (t.dtype != dt or t.numel() < n or not t.is_contiguous() or t.device != logits.device):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of {n} elements on the logits' device")
    pred = torch.empty(rows, dtype=torch.int64, device=logits.device)
    rank = torch.empty(rows, dtype=torch.int32, device=logits.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.call("vit_eval_update", _ptr(logits), ld, _ptr(labels), rows, classes, maxk, _ptr(pred), _ptr(rank),
              _ptr(row_loss), _ptr(counts), _ptr(loss_sum), _ptr(confusion), _stream(stream))
    return pred, rank, row_loss


MIX_ITEM_BYTES = ctypes.sizeof(_lib.MixItem)      # vit_mix_item: int32 src, float w, int32 y0, y1, x0, x1
_MIX_DTYPE = np.dtype([("src", "<i4"), ("w", "<f4"), ("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"), ("x1", "<i4")])
assert _MIX_DTYPE.itemsize == MIX_ITEM_BYTES == 24


def check_mix_table(src, w, y0, y1, x0, x1, B, H, W):
    """The caller's contract of vit_mix_batch, which the kernel cannot check: six host sequences of B entries with
    0 <= src < B, 0 <= w <= 1, 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W."""
    cols = [np.asarray(c, dtype=np.float64 if k == 1 else np.int64) for k, c in enumerate((src, w, y0, y1, x0, x1))]
    if any(c.shape != (B,) for c in cols):
        raise ValueError(f"mix table: every column needs {B} entries")
    s, wi, a0, a1, b0, b1 = cols
    ok_src = (0 <= s) & (s < B)
    ok_w = (0.0 <= wi) & (wi <= 1.0)                  # also refuses NaN
    ok_box = (0 <= a0) & (a0 <= a1) & (a1 <= H) & (0 <= b0) & (b0 <= b1) & (b1 <= W)
    bad = np.flatnonzero(~(ok_src & ok_w & ok_box))
    if bad.size:
        i = int(bad[0])
        if not ok_src[i]:
            raise ValueError(f"mix table row {i}: src {s[i]} outside [0, {B})")
        if not ok_w[i]:
            raise ValueError(f"mix table row {i}: w {wi[i]} outside [0, 1]")
        raise ValueError(f"mix table row {i}: box rows [{a0[i]}, {a1[i]}) x columns [{b0[i]}, {b1[i]}) outside a "
                         f"{H} x {W} image")
    return cols


def mix_table_host(src, w, y0, y1, x0, x1, pin=False):
    """The vit_mix_item array of the six columns as a uint8 host tensor (pinned with `pin`)."""
    B = len(src)
    tab = np.zeros(B, dtype=_MIX_DTYPE)
    for name, col in zip(("src", "w", "y0", "y1", "x0", "x1"), (src, w, y0, y1, x0, x1)):
        tab[name] = col
    host = torch.empty(B * MIX_ITEM_BYTES, dtype=torch.uint8, pin_memory=pin)
    host.copy_(torch.from_numpy(tab.view(np.uint8)))
    return host


def mix_batch(x, table, out=None, stream=None):
    """vit_mix_batch over a contiguous [B, C, H, W] float32 / bfloat16 device batch: out = x[src] inside each image's
    box, w * x + (1 - w) * x[src] outside it (x itself, bitwise, where w == 1).  `table` = (src, w, y0, y1, x0, x1),
    host sequences of B entries; it is validated here, BEFORE any device work (so a bad table raises without a GPU),
    then uploaded from a fresh pinned tensor with a non-blocking copy: no host sync.  `x` is not modified."""
    if x.dim() != 4:
        raise ValueError("mix_batch: x must be [B, C, H, W]")
    B, C, H, W = x.shape
    cols = check_mix_table(*table, B, H, W)
    _need_cuda(x, out)
    if not x.is_contiguous():
        raise ValueError("mix_batch: x must be contiguous")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("mix_batch: out must be a contiguous tensor of x's shape, dtype and device")
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    with torch.cuda.stream(s):                    # what is made here belongs to the stream that uses it
        if out is None:
            out = torch.empty_like(x)
        items = mix_table_host(*cols, pin=True).to(x.device, non_blocking=True)
    _lib.call("vit_mix_batch", _ptr(x), _ptr(out), dtype_code(x), B, C, H, W, _ptr(items), _stream(s))
    return out


AUG_ITEM_BYTES = ctypes.sizeof(_lib.AugItem)      # vit_aug_item: nine int32
AUG_COLUMNS = ("x0", "y0", "cw", "ch", "flip", "ey0", "ey1", "ex0", "ex1")
_AUG_DTYPE = np.dtype([(n, "<i4") for n in AUG_COLUMNS])
assert _AUG_DTYPE.itemsize == AUG_ITEM_BYTES == 36


def check_aug_table(table, heights, widths, out_h, out_w):
    """The table of vit_augment_to_tensor, which the entry point cannot read: nine host sequences (AUG_COLUMNS) of B
    entries with the crop box inside its image (0 <= x0, 1 <= cw, x0 + cw <= W; rows likewise), flip 0 or 1 and the
    erase box inside the output (0 <= ey0 <= ey1 <= out_h, 0 <= ex0 <= ex1 <= out_w).  Returns the int64 columns."""
    H, W = np.asarray(heights, dtype=np.int64), np.asarray(widths, dtype=np.int64)
    B = H.shape[0]
    if len(table) != len(AUG_COLUMNS):
        raise ValueError(f"augment table: {len(AUG_COLUMNS)} columns expected ({', '.join(AUG_COLUMNS)})")
    cols = [np.asarray(c, dtype=np.int64) for c in table]
    if any(c.shape != (B,) for c in cols) or W.shape != (B,):
        raise ValueError(f"augment table: every column needs {B} entries")
    x0, y0, cw, ch, flip, ey0, ey1, ex0, ex1 = cols
    ok_box = (0 <= x0) & (1 <= cw) & (x0 + cw <= W) & (0 <= y0) & (1 <= ch) & (y0 + ch <= H)
    ok_flip = (flip == 0) | (flip == 1)
    ok_erase = (0 <= ey0) & (ey0 <= ey1) & (ey1 <= out_h) & (0 <= ex0) & (ex0 <= ex1) & (ex1 <= out_w)
    bad = np.flatnonzero(~(ok_box & ok_flip & ok_erase))
    if bad.size:
        i = int(bad[0])
        if not ok_box[i]:
            raise ValueError(f"augment table row {i}: crop columns [{x0[i]}, {x0[i] + cw[i]}) x rows [{y0[i]}, "
                             f"{y0[i] + ch[i]}) is empty or outside its {H[i]} x {W[i]} image")
        if not ok_flip[i]:
            raise ValueError(f"augment table row {i}: flip {flip[i]} is neither 0 nor 1")
        raise ValueError(f"augment table row {i}: erase rows [{ey0[i]}, {ey1[i]}) x columns [{ex0[i]}, {ex1[i]}) "
                         f"outside a {out_h} x {out_w} output")
    return cols


def aug_table_host(table, pin=False):
    """The vit_aug_item array of the nine columns as a uint8 host tensor (pinned with `pin`)."""
    B = len(table[0])
    tab = np.zeros(B, dtype=_AUG_DTYPE)
    for name, col in zip(AUG_COLUMNS, table):
        tab[name] = col
    host = torch.empty(B * AUG_ITEM_BYTES, dtype=torch.uint8, pin_memory=pin)
    host.copy_(torch.from_numpy(tab.view(np.uint8)))
    return host


def aug_ksize(cw, ch, out_h, out_w):
    """ksize of vit_augment_to_tensor for crops of the given widths and heights: the most taps of any axis."""
    lib = _lib.load()
    return max(max(lib.vit_resize_ksize(int(a), out_w) for a in np.unique(cw)),
               max(lib.vit_resize_ksize(int(a), out_h) for a in np.unique(ch)))


def check_mean_std(mean, std):
    """(mean, std) as two float triples, or (None, None): both or neither, mean finite, std finite and non-zero."""
    if mean is None and std is None:
        return None, None
    if mean is None or std is None:
        raise ValueError("normalize: mean and std go together")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("normalize: mean and std need 3 entries each")
    if not all(np.isfinite(mean)) or not all(np.isfinite(std)) or any(s == 0.0 for s in std):
        raise ValueError("normalize: mean must be finite, std finite and non-zero")
    return mean, std


def augment_to_tensor(src, meta, items, out_h, out_w, ksize, out, workspace=None, mean=None, std=None,
                      erase_value=0.0, stream=None):
    """vit_augment_to_tensor: `src` the packed uint8 batch, `meta` int64 [B, 4] and `items` the vit_aug_item array
    (uint8, aug_table_host's layout), all on the device; `out` [B, 3, out_h, out_w] float32 / bfloat16.  The table is
    NOT validated here (it is device memory; the kernel clamps it): data.GpuTrainTransform validates on the host
    before it uploads.  One launch on `stream`, no host sync."""
    mean, std = check_mean_std(mean, std)
    _need_cuda(src, meta, items, out, workspace)
    B = meta.shape[0]
    if items.numel() * items.element_size() != B * AUG_ITEM_BYTES:
        raise ValueError(f"augment_to_tensor: the table needs {B} items of {AUG_ITEM_BYTES} bytes")
    if tuple(out.shape) != (B, 3, out_h, out_w) or not out.is_contiguous():
        raise ValueError(f"augment_to_tensor: out must be a contiguous [{B}, 3, {out_h}, {out_w}] tensor")
    need = _lib.load().vit_augment_workspace_bytes(B, out_h, out_w, ksize)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=out.device)
    f3 = ctypes.c_float * 3
    _lib.call("vit_augment_to_tensor", _ptr(src), _ptr(meta), _ptr(items), B, out_h, out_w, ksize,
              f3(*mean) if mean else None, f3(*std) if std else None, float(erase_value), _ptr(out),
              dtype_code(out), _ptr(workspace), workspace.numel(), _stream(stream))
    return out


RA_ITEM_BYTES = ctypes.sizeof(_lib.RaItem)        # vit_ra_item: VIT_RA_MAX_LAYERS layers of 72 bytes
_RA_LAYER_DTYPE = np.dtype([("coef", "<f8", (6,)), ("kind", "<i4"), ("iarg0", "<i4"), ("iarg1", "<i4"), ("farg", "<f4"),
                            ("fill", "u1", (4,)), ("pad_", "<i4")])
_RA_DTYPE = np.dtype([("layer", _RA_LAYER_DTYPE, (_lib.RA_MAX_LAYERS,))])
assert _RA_LAYER_DTYPE.itemsize == ctypes.sizeof(_lib.RaLayer) == 72 and _RA_DTYPE.itemsize == RA_ITEM_BYTES == 288
# data.RA_OPS name -> VIT_RA_* kind; the geometric ops are all the one AFFINE kind, told apart by their coefficients
RA_KIND = {"None": _lib.RA_NONE, "AutoContrast": _lib.RA_AUTOCONTRAST, "Equalize": _lib.RA_EQUALIZE,
           "Invert": _lib.RA_INVERT, "Posterize": _lib.RA_POSTERIZE, "Solarize": _lib.RA_SOLARIZE,
           "SolarizeAdd": _lib.RA_SOLARIZE_ADD, "Color": _lib.RA_COLOR, "Contrast": _lib.RA_CONTRAST,
           "Brightness": _lib.RA_BRIGHTNESS, "Sharpness": _lib.RA_SHARPNESS, "Rotate": _lib.RA_AFFINE,
           "ShearX": _lib.RA_AFFINE, "ShearY": _lib.RA_AFFINE, "TranslateXRel": _lib.RA_AFFINE,
           "TranslateYRel": _lib.RA_AFFINE}
_RA_STATS_KINDS = (_lib.RA_AUTOCONTRAST, _lib.RA_EQUALIZE, _lib.RA_CONTRAST)


def check_ra_table(table, B):
    """The host table of vit_randaug_to_tensor, which the entry point cannot read: (op, arg, coef) = int [B, L] indices
    into data.RA_OPS, float64 [B, L] arguments and float64 [B, L, 6] AFFINE coefficients, 1 <= L <= VIT_RA_MAX_LAYERS,
    every argument and coefficient finite.  Returns it as a data.RaTable of int32 / float64 / float64 arrays."""
    from .data import RA_OPS, RaTable
    if len(table) != 3:
        raise ValueError("randaug table: three arrays expected (op, arg, coef)")
    op, arg, coef = np.asarray(table[0]), np.asarray(table[1], dtype=np.float64), np.asarray(table[2], dtype=np.float64)
    if op.ndim != 2 or op.shape[0] != B or not np.issubdtype(op.dtype, np.integer):
        raise ValueError(f"randaug table: op must be an integer [{B}, layers] array")
    L = op.shape[1]
    if not 1 <= L <= _lib.RA_MAX_LAYERS:
        raise ValueError(f"randaug table: {L} layers (1 to {_lib.RA_MAX_LAYERS} allowed)")
    if arg.shape != (B, L) or coef.shape != (B, L, 6):
        raise ValueError(f"randaug table: arg must be [{B}, {L}] and coef [{B}, {L}, 6]")
    if ((op < 0) | (op >= len(RA_OPS))).any():
        raise ValueError(f"randaug table: an op outside [0, {len(RA_OPS)})")
    if not np.isfinite(arg).all() or not np.isfinite(coef).all():
        raise ValueError("randaug table: a non-finite argument or coefficient")
    return RaTable(op.astype(np.int32), arg, coef)


def _ra_kinds(op):
    from .data import RA_OPS
    return np.array([RA_KIND[n] for n in RA_OPS], dtype=np.int32)[op]


def ra_stats_layers(table):
    """The stats_layers mask of vit_randaug_to_tensor: bit l is set when some image's layer l needs the histograms."""
    kinds = _ra_kinds(np.asarray(table[0]))
    return sum(1 << l for l in range(kinds.shape[1]) if np.isin(kinds[:, l], _RA_STATS_KINDS).any())


def randaug_table_host(table, fill=(128, 128, 128), pin=False):
    """The vit_ra_item array of a checked RaTable as a uint8 host tensor (pinned with `pin`): the kind of every op, its
    integer or fp32 argument, the AFFINE coefficients in fp64 and the fill colour."""
    from .data import RA_OPS
    op, arg, coef = table
    B, L = op.shape
    tab = np.zeros(B, dtype=_RA_DTYPE)
    lay = tab["layer"][:, :L]
    kinds = _ra_kinds(op)
    lay["kind"] = kinds
    lay["coef"] = coef
    ints = np.isin(kinds, (_lib.RA_POSTERIZE, _lib.RA_SOLARIZE, _lib.RA_SOLARIZE_ADD))
    lay["iarg0"] = np.where(ints, arg, 0.0).astype(np.int32)
    lay["iarg1"] = np.where(op == RA_OPS.index("SolarizeAdd"), 128, 0)
    lay["farg"] = arg.astype(np.float32)
    lay["fill"][..., :3] = np.asarray(fill, dtype=np.uint8)
    tab["layer"][:, :L] = lay
    host = torch.empty(B * RA_ITEM_BYTES, dtype=torch.uint8, pin_memory=pin)
    host.copy_(torch.from_numpy(tab.view(np.uint8)))
    return host


def augment_to_u8(src, meta, items, out_h, out_w, ksize, out, workspace=None, stream=None):
    """vit_augment_to_u8: vit_augment_to_tensor's crop, resize and flip with a uint8 store; `out` is a contiguous uint8
    [B, out_h, out_w, 3] device tensor (HWC, RGB).  Arguments as for augment_to_tensor; no normalize, no erase."""
    _need_cuda(src, meta, items, out, workspace)
    B = meta.shape[0]
    if items.numel() * items.element_size() != B * AUG_ITEM_BYTES:
        raise ValueError(f"augment_to_u8: the table needs {B} items of {AUG_ITEM_BYTES} bytes")
    if tuple(out.shape) != (B, out_h, out_w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"augment_to_u8: out must be a contiguous uint8 [{B}, {out_h}, {out_w}, 3] tensor")
    if workspace is None:
        workspace = torch.empty(_lib.load().vit_augment_workspace_bytes(B, out_h, out_w, ksize), dtype=torch.uint8,
                                device=out.device)
    _lib.call("vit_augment_to_u8", _ptr(src), _ptr(meta), _ptr(items), B, out_h, out_w, ksize, _ptr(out),
              _ptr(workspace), workspace.numel(), _stream(stream))
    return out


def randaug_to_tensor(u8, ra_items, nlayers, stats_layers, erase_items, out, workspace=None, mean=None, std=None,
                      erase_value=0.0, stream=None):
    """vit_randaug_to_tensor: `u8` the uint8 [B, S_h, S_w, 3] picture of augment_to_u8, `ra_items` the vit_ra_item array
    (uint8, randaug_table_host's layout), `erase_items` the vit_aug_item array whose erase boxes apply, all on the
    device; `out` [B, 3, S_h, S_w] float32 / bfloat16.  The tables are NOT validated here (device memory; the kernels
    clamp): data.GpuTrainTransform validates on the host before it uploads.  No allocation inside, no host sync."""
    mean, std = check_mean_std(mean, std)
    _need_cuda(u8, ra_items, erase_items, out, workspace)
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8 or not u8.is_contiguous():
        raise ValueError("randaug_to_tensor: u8 must be a contiguous uint8 [B, S_h, S_w, 3] tensor")
    B, sh, sw, _ = u8.shape
    if ra_items.numel() * ra_items.element_size() != B * RA_ITEM_BYTES:
        raise ValueError(f"randaug_to_tensor: the table needs {B} items of {RA_ITEM_BYTES} bytes")
    if erase_items.numel() * erase_items.element_size() != B * AUG_ITEM_BYTES:
        raise ValueError(f"randaug_to_tensor: the erase table needs {B} items of {AUG_ITEM_BYTES} bytes")
    if tuple(out.shape) != (B, 3, sh, sw) or not out.is_contiguous():
        raise ValueError(f"randaug_to_tensor: out must be a contiguous [{B}, 3, {sh}, {sw}] tensor")
    if workspace is None:
        workspace = torch.empty(_lib.load().vit_randaug_workspace_bytes(B, sh, sw), dtype=torch.uint8,
                                device=out.device)
    f3 = ctypes.c_float * 3
    _lib.call("vit_randaug_to_tensor", _ptr(u8), _ptr(ra_items), B, sh, sw, int(nlayers), int(stats_layers),
              f3(*mean) if mean else None, f3(*std) if std else None, _ptr(erase_items), float(erase_value), _ptr(out),
              dtype_code(out), _ptr(workspace), workspace.numel(), _stream(stream))
    return out


def adamw(table_dev, nchunks, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale,
          shadow_dtype, stream=None, clip=None):
    """vit_adamw; with `clip` (the [4] f32 device block grad_clip_finish wrote) vit_adamw_clipped: the gradient
    scale is multiplied by clip[1] on the device and nothing is updated when clip[2] is set."""
    if clip is None:
        _lib.call("vit_adamw", _ptr(table_dev), nchunks, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2,
                  grad_scale, dtype_code(shadow_dtype), _stream(stream))
        return
    _lib.call("vit_adamw_clipped", _ptr(table_dev), nchunks, lr, beta1, beta2, eps, weight_decay, bias_corr1,
              bias_corr2, grad_scale, dtype_code(shadow_dtype), _clip_ptr(clip), _stream(stream))


def _check_clip(clip):
    _need_cuda(clip)
    if clip.dtype != torch.float32 or clip.numel() < 4 or not clip.is_contiguous():
        raise ValueError("clip state must be a contiguous float32 tensor of at least 4 elements")


def _clip_ptr(clip):
    """The pointer of a step's clip block, checked; None (NULL) for the unclipped step.  No deeper in calls than the
    checks it replaces, nor is _ema_args: they run for every launch of a per-group step, whose pace the host sets."""
    if clip is None:
        return None
    _check_clip(clip)
    return ctypes.c_void_p(clip.data_ptr())


def grad_sumsq(table_dev, nchunks, grad_scale, partial, stream=None):
    """partial[i] = sum over chunk i of (grad_scale * g)^2, fp64 (vit_grad_sumsq).  `partial`: float64 device tensor
    (or a slice of one) of at least nchunks elements."""
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() < nchunks or not partial.is_contiguous():
        raise ValueError(f"partial must be a contiguous float64 tensor of at least {nchunks} elements")
    _lib.call("vit_grad_sumsq", _ptr(table_dev), nchunks, grad_scale, _ptr(partial), _stream(stream))


def grad_clip_finish(partial, nparts, max_norm, clip, skip_nonfinite=True, stream=None):
    """clip[0..4) = (norm, coef, skip, skipped total += skip) from partial[0..nparts) (vit_grad_clip_finish).
    `skip_nonfinite=False` passes -max_norm: the bound is the same and a non-finite norm is not skipped."""
    _need_cuda(partial)
    _check_clip(clip)
    if max_norm is None or not max_norm > 0:
        raise ValueError(f"max_norm must be a positive number (got {max_norm!r})")
    if partial.dtype != torch.float64 or partial.numel() < nparts:
        raise ValueError(f"partial must be a float64 tensor of at least {nparts} elements")
    _lib.call("vit_grad_clip_finish", _ptr(partial), nparts, max_norm if skip_nonfinite else -max_norm, _ptr(clip),
              _stream(stream))


def pack(table_dev, nchunks, shadow_dtype, stream=None):
    _lib.call("vit_pack", _ptr(table_dev), nchunks, dtype_code(shadow_dtype), _stream(stream))


# elements per multi-tensor chunk (one 256-thread workgroup each).  Measured on the C2 parameter set
# (tools/adamw_bench.py, profiles/r60_adamw_chunk.log): 64 Ki 527 us, 16 Ki 476, 8 Ki 471, 4 Ki 473 — more, smaller
# workgroups keep more loads in flight per CU.  VIT_ADAMW_CHUNK overrides it.
CHUNK = int(os.environ.get("VIT_ADAMW_CHUNK", 8192))


def _chunks(numel):
    """The (offset, n) pieces a tensor of `numel` elements is cut into: the one place that knows the boundaries, so
    the chunk table and the EMA pointer array that goes with it cannot disagree.  Reads CHUNK at call time."""
    return [(off, min(CHUNK, numel - off)) for off in range(0, numel, CHUNK)]


def build_chunk_table(entries, device):
    """entries: list of (p, g, m, v, shadow) tensors (fp32 contiguous, shadow may be None).  Returns (uint8 device
    tensor holding the vit_tensor_chunk array, nchunks)."""
    chunks = []
    for p, g, m, v, sh in entries:
        es = sh.element_size() if sh is not None else 0
        for off, n in _chunks(p.numel()):
            c = _lib.TensorChunk()
            c.p = p.data_ptr() + 4 * off
            c.g = (g.data_ptr() + 4 * off) if g is not None else 0
            c.m = (m.data_ptr() + 4 * off) if m is not None else 0
            c.v = (v.data_ptr() + 4 * off) if v is not None else 0
            c.shadow = (sh.data_ptr() + es * off) if sh is not None else None
            c.n = n
            chunks.append(c)
    arr = (_lib.TensorChunk * len(chunks))(*chunks)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(chunks)


def build_ema_pointers(entries, device):
    """The EMA pointer array that goes with build_chunk_table(entries): `entries` is a list of (p, ema) in the same
    order, ema an fp32 contiguous tensor of p's size (4-B alignment suffices) or None.  One pointer per chunk, cut by
    the same _chunks(); 0 (NULL) for every chunk of a tensor without an EMA.  Returns (int64 device tensor, nchunks)."""
    ptrs = []
    for p, e in entries:
        n = p.numel()
        if e is not None and (e.dtype != torch.float32 or e.numel() != n or not e.is_contiguous()
                              or e.device != p.device):
            raise ValueError("an EMA tensor must be contiguous float32 of its parameter's size, on its device")
        ptrs.extend(e.data_ptr() + 4 * off if e is not None else 0 for off, _ in _chunks(n))
    return torch.tensor(ptrs, dtype=torch.int64).to(device), len(ptrs)


def _check_ema(ema_dev, nchunks):
    _need_cuda(ema_dev)
    if ema_dev.dtype != torch.int64 or ema_dev.numel() != nchunks or not ema_dev.is_contiguous():
        raise ValueError(f"the EMA pointer array must be a contiguous int64 tensor of {nchunks} elements")


def _ema_args(ema_dev, ema_decay, nchunks, optional=True):
    """(pointer, weight) of a step's EMA; (NULL, 0) for an `optional` one that is not kept.  The weight 1 - ema_decay
    is formed in double here and rounded to fp32 once, as the `float` argument it becomes."""
    if ema_dev is None and optional:
        return None, 0.0
    _check_ema(ema_dev, nchunks)
    return ctypes.c_void_p(ema_dev.data_ptr()), 1.0 - float(ema_decay)


def adamw_ema(table_dev, ema_dev, nchunks, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale,
              shadow_dtype, ema_decay, stream=None, clip=None):
    """vit_adamw_ema: the (clipped, with `clip`) AdamW update, then e += (1 - ema_decay) * (p_new - e) for every chunk
    whose EMA pointer is set."""
    ema_p, ema_w = _ema_args(ema_dev, ema_decay, nchunks, optional=False)
    _lib.call("vit_adamw_ema", _ptr(table_dev), ema_p, nchunks, lr, beta1, beta2, eps, weight_decay, bias_corr1,
              bias_corr2, grad_scale, dtype_code(shadow_dtype), ema_w, _clip_ptr(clip), _stream(stream))


def ema_swap(table_dev, ema_dev, nchunks, shadow_dtype, stream=None):
    """vit_ema_swap: p <-> e for every chunk whose EMA pointer is set, and shadow = (dtype) p there."""
    _check_ema(ema_dev, nchunks)
    _lib.call("vit_ema_swap", _ptr(table_dev), _ptr(ema_dev), nchunks, dtype_code(shadow_dtype), _stream(stream))


# ---- LAMB (vit_hip.h "LAMB") ----------------------------------------------------------------------------------------
def build_tensor_index(entries, device):
    """The per-tensor maps that go with build_chunk_table(entries), cut by the same _chunks(): `tensor_first`
    (int32 [ntensors + 1], the index of each tensor's first chunk, nchunks last) and `tensor_of_chunk` (int32
    [nchunks]).  `entries` is any list whose items start with the parameter.  Returns (tensor_first, tensor_of_chunk,
    ntensors, nchunks), the first two on `device`."""
    first, owner = [0], []
    for i, ent in enumerate(entries):
        n = len(_chunks(ent[0].numel()))
        if n == 0:
            raise ValueError("a tensor without elements has no chunk, so it cannot have a trust ratio")
        owner.extend([i] * n)
        first.append(first[-1] + n)
    return (torch.tensor(first, dtype=torch.int32).to(device), torch.tensor(owner, dtype=torch.int32).to(device),
            len(entries), len(owner))


def _check_lamb_buffer(t, dtype, numel, what, exactly=None):
    """A contiguous device tensor of `dtype` with at least `numel` elements; with `exactly` (how the message names
    that count: "nchunks = ", or "" for the number alone) no more than that either, as an index array has."""
    _need_cuda(t)
    if t is None or t.dtype != dtype or t.numel() < numel or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} device tensor of at least {numel} elements")
    if exactly is not None and t.numel() != numel:
        raise ValueError(f"{what} must have {exactly}{numel} elements")


def _check_partial_sums(partial):
    """The partials the trust pass reads, indexed by the tensor index: any length."""
    if partial is None or partial.dtype != torch.float64 or not partial.is_contiguous():
        raise ValueError("partial must be a contiguous float64 device tensor")
    if not partial.is_cuda:
        _need_cuda(partial)      # raises, with its message


def lamb_moments(table_dev, nchunks, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale, partial,
                 stream=None, clip=None):
    """vit_lamb_moments: m and v of every chunk, and partial[2i], partial[2i + 1] = the chunk's fp64 sums of p^2 and
    u^2.  `partial`: float64 device tensor of at least 2 * nchunks elements.  `clip` as in adamw()."""
    _need_cuda(table_dev)
    _check_lamb_buffer(partial, torch.float64, 2 * nchunks, "partial")
    _lib.call("vit_lamb_moments", _ptr(table_dev), nchunks, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2,
              grad_scale, _clip_ptr(clip), _ptr(partial), _stream(stream))


def lamb_trust(partial, tensor_first, ntensors, trust, adapt=True, trust_clip=False, stream=None, clip=None):
    """vit_lamb_trust: trust[i] = |p| / |u| of tensor i from lamb_moments' partials where `adapt` is set and both norms
    are positive, else 1; at most 1 with `trust_clip`.  `tensor_first` from build_tensor_index."""
    _check_lamb_buffer(tensor_first, torch.int32, ntensors + 1, "tensor_first", "ntensors + 1 = ")
    _check_lamb_buffer(trust, torch.float32, ntensors, "trust")
    _check_partial_sums(partial)
    _lib.call("vit_lamb_trust", _ptr(partial), _ptr(tensor_first), ntensors, int(bool(adapt)), int(bool(trust_clip)),
              _ptr(trust), _clip_ptr(clip), _stream(stream))


def lamb_update(table_dev, tensor_of_chunk, trust, nchunks, lr, eps, weight_decay, bias_corr1, bias_corr2,
                shadow_dtype, ema_dev=None, ema_decay=None, stream=None, clip=None):
    """vit_lamb_update: p -= lr * trust[tensor of the chunk] * u, the shadows, and with `ema_dev` / `ema_decay` the
    EMA of adamw_ema() for every chunk whose pointer is set.  eps, weight_decay and the bias corrections are those
    lamb_moments was given."""
    _need_cuda(table_dev)
    _check_lamb_buffer(tensor_of_chunk, torch.int32, nchunks, "tensor_of_chunk", "nchunks = ")
    _check_lamb_buffer(trust, torch.float32, 1, "trust")
    ema_p, ema_w = _ema_args(ema_dev, ema_decay, nchunks)
    _lib.call("vit_lamb_update", _ptr(table_dev), ema_p, _ptr(tensor_of_chunk), _ptr(trust), nchunks, lr, eps,
              weight_decay, bias_corr1, bias_corr2, dtype_code(shadow_dtype), ema_w, _clip_ptr(clip), _stream(stream))


# ---- grouped steps (vit_hip.h "Grouped optimizer steps") -----------------------------------------------------------
def build_group_index(entries, sizes, device):
    """The group maps that go with build_chunk_table(entries) and build_tensor_index(entries), cut by the same
    _chunks(): `entries` holds the tensors of group 0, then those of group 1, ... and `sizes[k]` is how many belong to
    group k.  Returns (group_of_chunk int32 [nchunks], group_of_tensor int32 [ntensors]) on `device`, and `bounds`, a
    host list of (first tensor, first chunk) per group with (ntensors, nchunks) last.  The indices are taken modulo
    OPT_MAX_GROUPS, so that a launch over groups [64 k, 64 k + 64) can hand the kernel those 64 alone."""
    if sum(sizes) != len(entries):
        raise ValueError("sizes must add up to the number of entries")
    of_chunk, of_tensor, bounds, it = [], [], [], iter(entries)
    for k, size in enumerate(sizes):
        bounds.append((len(of_tensor), len(of_chunk)))
        for _ in range(size):
            of_tensor.append(k % _lib.OPT_MAX_GROUPS)
            of_chunk.extend([k % _lib.OPT_MAX_GROUPS] * len(_chunks(next(it)[0].numel())))
    bounds.append((len(of_tensor), len(of_chunk)))
    return (torch.tensor(of_chunk, dtype=torch.int32).to(device), torch.tensor(of_tensor, dtype=torch.int32).to(device),
            bounds)


def opt_groups(specs):
    """The host vit_opt_group array of `specs`: (lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, flags)
    per group, the floats rounded to fp32 as a `float` argument of the single-group entry points is."""
    if not 1 <= len(specs) <= _lib.OPT_MAX_GROUPS:
        raise ValueError(f"a grouped launch takes 1..{_lib.OPT_MAX_GROUPS} groups (got {len(specs)})")
    packed = struct.pack("7fi" * len(specs), *[x for s in specs for x in s])      # one call, not one object per field
    return (_lib.OptGroup * len(specs)).from_buffer_copy(packed)


def adamw_groups(table_dev, group_of_chunk, nchunks, specs, grad_scale, shadow_dtype, ema_dev=None, ema_decay=None,
                 stream=None, clip=None):
    """vit_adamw_groups: adamw() / adamw_ema() over the chunks of several groups in one launch; chunk i takes the
    scalars of specs[group_of_chunk[i]] (opt_groups).  `ema_dev` / `ema_decay` and `clip` as in adamw_ema()."""
    _need_cuda(table_dev)
    _check_lamb_buffer(group_of_chunk, torch.int32, nchunks, "group_of_chunk", "")
    ema_p, ema_w = _ema_args(ema_dev, ema_decay, nchunks)
    clip_p, groups = _clip_ptr(clip), opt_groups(specs)
    _lib.call("vit_adamw_groups", _ptr(table_dev), ema_p, _ptr(group_of_chunk), nchunks, groups, len(groups),
              grad_scale, dtype_code(shadow_dtype), ema_w, clip_p, _stream(stream))


def lamb_moments_groups(table_dev, group_of_chunk, nchunks, specs, grad_scale, partial, stream=None, clip=None):
    """vit_lamb_moments_groups: lamb_moments() with each chunk's scalars from specs[group_of_chunk[i]]."""
    _need_cuda(table_dev)
    _check_lamb_buffer(group_of_chunk, torch.int32, nchunks, "group_of_chunk", "")
    _check_lamb_buffer(partial, torch.float64, 2 * nchunks, "partial")
    clip_p, groups = _clip_ptr(clip), opt_groups(specs)
    _lib.call("vit_lamb_moments_groups", _ptr(table_dev), _ptr(group_of_chunk), nchunks, groups, len(groups),
              grad_scale, clip_p, _ptr(partial), _stream(stream))


def lamb_trust_groups(partial, tensor_first, group_of_tensor, ntensors, specs, trust, stream=None, clip=None):
    """vit_lamb_trust_groups: lamb_trust() with each tensor's flags from specs[group_of_tensor[i]]."""
    _check_lamb_buffer(tensor_first, torch.int32, ntensors + 1, "tensor_first", "ntensors + 1 = ")
    _check_lamb_buffer(group_of_tensor, torch.int32, ntensors, "group_of_tensor", "")
    _check_lamb_buffer(trust, torch.float32, ntensors, "trust")
    _check_partial_sums(partial)
    clip_p, groups = _clip_ptr(clip), opt_groups(specs)
    _lib.call("vit_lamb_trust_groups", _ptr(partial), _ptr(tensor_first), _ptr(group_of_tensor), ntensors, groups,
              len(groups), _ptr(trust), clip_p, _stream(stream))


def lamb_update_groups(table_dev, tensor_of_chunk, trust, group_of_chunk, nchunks, specs, shadow_dtype, ema_dev=None,
                       ema_decay=None, stream=None, clip=None):
    """vit_lamb_update_groups: lamb_update() with each chunk's scalars from specs[group_of_chunk[i]], the specs
    lamb_moments_groups was given."""
    _need_cuda(table_dev)
    _check_lamb_buffer(tensor_of_chunk, torch.int32, nchunks, "tensor_of_chunk", "")
    _check_lamb_buffer(group_of_chunk, torch.int32, nchunks, "group_of_chunk", "")
    _check_lamb_buffer(trust, torch.float32, 1, "trust")
    ema_p, ema_w = _ema_args(ema_dev, ema_decay, nchunks)
    clip_p, groups = _clip_ptr(clip), opt_groups(specs)
    _lib.call("vit_lamb_update_groups", _ptr(table_dev), ema_p, _ptr(tensor_of_chunk), _ptr(trust),
              _ptr(group_of_chunk), nchunks, groups, len(groups), dtype_code(shadow_dtype), ema_w, clip_p,
              _stream(stream))
