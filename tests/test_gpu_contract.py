"""Every kernel instantiation and every GEMM epilogue field against a plain fp64 reference, at the shapes the
benchmark-sized tests of test_gpu_kernels.py never launch.  Each reference is torch in fp64 (or an oracle.vit_oracle
helper) evaluated from the same stored inputs the kernel reads.

Host-dispatch branch -> the test that reaches it:

| branch                                                   | test                                                    |
|----------------------------------------------------------|---------------------------------------------------------|
| attention RING(1..16), one item per workgroup            | test_attention_ring_every_nt (max_wgs 0)                |
| attention RING(1..16), several items per workgroup       | test_attention_ring_every_nt (max_wgs 2, grid 4)        |
| attention RING(1..16) with the fp32 O store              | test_attention_ring_every_nt (o32)                      |
| attention BWD(1..8), one item per workgroup              | test_attention_bwd_fused_every_nq (shared_cus)          |
| attention BWD(1..8), several items per workgroup         | test_attention_bwd_fused_every_nq (attn_bwd_grid 2)     |
| tiled forward / backward at 128-row block edges          | test_attention_tiled_block_edges                        |
| generic probability-storing forward -> BWD(NQ)           | test_attention_probs_forward_feeds_mfma_backward        |
| NV 1, 2, 4, 6, 8 x ln16 forward x LDS accumulators       | test_layernorm_every_width[200/512/1000/1536/2048-bf16] |
| NV 2, 6, 16 x fallback forward (cols % 8 == 4)           | test_layernorm_every_width[260/1284/3076-bf16]          |
| NV 3, 6, 12 x fallback forward (ln16 0; row stride)      | test_layernorm_ln16_option, ..._strided_rows[bf16-772]  |
| NV 16 x ln16 forward, register form (both dtypes)        | test_layernorm_every_width[4096-*], [3076-*]            |
| NV 1, 2, 4 fp32 register form; NV 6, 8 fp32 LDS form     | test_layernorm_every_width[*-fp32]                      |
| NV 3, 6, 12 bf16 / NV 6, 12 fp32 register form (ln_al 0) | test_layernorm_accumulator_forms                        |
| few-row spread, partial 4-row mask group, odd row count  | test_layernorm_few_rows_saved_mask, ..._every_width     |
| gemm_impl 1 (forced, and K % 64 != 0) x vector epilogue  | test_gemm_contract[v1-*], [v1_k72-*]                    |
| gemm_impl 2 x vector epilogue                            | test_gemm_contract[v2-*]                                |
| gemm_impl 4 x vector epilogue (every specialised kind)   | test_gemm_contract[v4-*]                                |
| f32 kernel x vector epilogue                             | test_gemm_contract[f32-*]                               |
| gemm_impl 1, 2, 4, f32 x scalar epilogue (N = 10)        | test_gemm_contract_scalar_epilogue                      |
| gemm_impl 1, 2, 4, f32 x scalar epilogue (ldc = N + 1)   | test_gemm_contract_odd_ldc, ..._scalar_aux              |
| gemm_impl 1, 2, 4, f32 x split-K reduce, vector          | test_gemm_contract[*-l], [*-m], ..._three_full_slices   |
| gemm_impl 1, 2, 4, f32 x split-K reduce, scalar          | test_gemm_contract_scalar_epilogue[l-*]                 |
| one-row last tile row of a partial round; gemm_group_m   | test_gemm_one_row_partial_round; test_gemm_group_m      |
| v4 bias + GELU (LDS-image epilogue) + mask_out + colsum  | test_gemm_v4_bias_gelu_side_outputs                     |
| vit_col2im, vit_embed_cls, vit_relu_bwd                  | test_col2im, test_embed_cls, test_relu_bwd              |
| vit_mask4_apply, vit_pack                                | test_mask4_apply, test_pack                             |
| vit_adamw (grad_scale, f32 / NULL shadow)                | test_adamw_grad_scale_and_shadows                       |
| vit_copy2d casts, vit_colsum bf16                        | test_copy2d_casts, test_colsum_bf16_strided             |
| vit_softmax_xent                                         | test_softmax_xent                                       |
"""
import math
import zlib

import pytest
import torch

import test_gpu_kernels as K
from oracle import vit_oracle as O
from test_gpu_kernels import _attn_flash_grads, _check_attn_bwd_bf16, _ints, _mask4_pack, _ref_op

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 7.0


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------------------------------------------------------
# 1. vit_gemm against the documented formula (include/vit_hip.h, "GEMM with fused epilogue")
# ---------------------------------------------------------------------------------------------------------------
def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gemm_contract_ref(A, B, m, n, akc, bkc, out_dtype, alpha=1.0, beta=0.0, c_old=None, bias=None, act=0,
                       aux_bits=None, dropout_p=0.0, seed=0, drop_row_stride=1, drop_row0=0, res=None, res_rowmod=0):
    """epi(alpha * sum_r A(i,r) B(j,r)) in fp64 from the stored operands: + beta*C_old, + bias, act, aux mask, dropout
    at index ((i + R0)*S)*n + j with scale 1/(1-p), + res(i % res_rowmod).  Returns (C before the output rounding,
    C as stored, the mask4 bytes of mask_out, colsum_part = per-256-row-block column sums of C as stored).  The
    out_group row remap only moves rows: the caller places row i of C."""
    v = alpha * _ref_op(A, B, akc, bkc)
    assert v.shape == (m, n)
    if beta != 0.0:
        v = v + beta * c_old.double()
    if bias is not None:
        v = v + bias.double()
    if act == _ops.ACT_RELU:
        v = v.clamp_min(0.0)
    elif act == _ops.ACT_GELU:
        v = _gelu64(v)
    if aux_bits is not None:
        v = v * aux_bits.double()
    keep = None
    if dropout_p > 0.0:
        S = max(int(drop_row_stride), 1)
        big = O.dropout_keep(seed, ((m + drop_row0) * S, n), dropout_p).to(DEV)
        keep = big[drop_row0 * S::S][:m]                    # rows (i + R0) * S of the larger tensor
        assert keep.shape == (m, n)
        v = v * keep.double() * (1.0 / (1.0 - dropout_p))
    if res is not None:
        rows = torch.arange(m, device=DEV)
        v = v + res.double()[rows % res_rowmod if res_rowmod else rows]
    stored = v.float().to(out_dtype)
    bits = keep.bool() if keep is not None else stored > 0
    csum = torch.stack([stored[r:r + 256].double().sum(0) for r in range(0, m, 256)]).float()
    return v, stored, _mask4_pack(bits), csum


def _mask4_valid(nbytes, m, n):
    """bytes of rows >= m (the padding of the last 4-row group) are unspecified"""
    b = torch.arange(nbytes, device=DEV)
    return (b // 4 // (-(-n // 4))) * 4 + b % 4 < m


# kernel path -> (option gemm_impl, input dtype, (M, N, K))
GEMM_PATHS = {"v1": (1, BF, (200, 136, 128)), "v1_k72": (0, BF, (200, 136, 72)), "v2": (2, BF, (200, 136, 128)),
              "v4": (4, BF, (264, 272, 128)), "f32": (0, F32, (100, 72, 40))}
TT, TF, FF, FT = (True, True), (True, False), (False, False), (False, True)


def _run_gemm_recipe(libopt, path, layout, recipe, n=None, k=None, ldc_extra=0):
    """One vit_gemm call of `recipe` on kernel `path`, compared with _gemm_contract_ref: exact (integer-valued
    operands, alpha in {1, 0.5}, dropout p = 0.5) except GELU; every byte of the output buffer outside the m x n
    window must keep its sentinel."""
    impl, in_dt, (M, N, Kd) = GEMM_PATHS[path]
    akc, bkc = layout
    N = n or N
    Kd = k or Kd
    if recipe == "d" and path in ("v1", "v2", "v4"):
        Kd = 64
    libopt("gemm_impl", impl)
    g = torch.Generator().manual_seed(_seed(path, layout, recipe, N, Kd))
    lo, hi = (-1, 2) if recipe == "d" else (-4, 5)
    pad = 8 if recipe == "k" else 0

    def ints(shape, dtype=in_dt, lo_=lo, hi_=hi):
        return _ints(shape, lo_, hi_, gen=g, dtype=dtype)

    if recipe == "i":                       # rows 0, 5, 10, ... of a 5x taller tensor: lda = 5 K
        assert akc
        A = ints((5 * M, Kd)).view(M, 5 * Kd)[:, :Kd]
    else:
        A = ints((M, Kd + pad))[:, :Kd] if akc else ints((Kd, M + pad))[:, :M]
    B = ints((N, Kd + pad))[:, :Kd] if bkc else ints((Kd, N + pad))[:, :N]
    bias = ints((N,), F32)
    kw, ref_kw = {}, {}
    out_dt = in_dt
    aux_bits = None
    if recipe in ("a", "d", "f"):
        kw["alpha"] = 0.5
    if recipe in ("b", "m"):
        kw["beta"], out_dt = 1.0, F32
    if recipe in ("c", "l"):
        kw.update(bias=bias, act=_ops.ACT_RELU)
    if recipe == "d":
        kw.update(bias=bias, act=_ops.ACT_GELU)
    if recipe == "e":
        aux = ints((M, N + 8), BF)[:, :N]
        kw.update(aux=aux, ldaux=N + 8)
        aux_bits = aux > 0
    if recipe == "f":
        aux_bits = torch.randint(0, 2, (M, N), generator=g).bool().to(DEV)
        kw["aux"] = _mask4_pack(aux_bits)
    if recipe in ("g", "h", "i"):
        res = ints((M, N + 16), BF)[:, :N] if recipe != "h" else ints((M, N), F32)
        kw.update(bias=bias, dropout_p=0.5, seed=1234 + M, res=res, ldres=res.stride(0))
    if recipe == "h":
        out_dt = BF
    if recipe == "i":
        kw.update(drop_row_stride=5, drop_row0=3)
    if recipe == "j":
        res = ints((7, N), F32)
        kw.update(bias=bias, res=res, ldres=N, res_rowmod=7, out_group=(7, 9))
    if recipe in ("l", "m"):
        kw["split_k"] = 3
    if recipe == "l":
        out_dt = BF
    want_mask = recipe in ("c", "g", "h", "i", "l")
    want_csum = recipe in ("e", "f")
    # the output buffer, sentinel-filled (C_old for beta), and C as a view of it
    if recipe == "k":                       # a column slice: ldc = N + 24, 8 columns in, 3 more rows below
        cbuf = torch.full((M + 3, N + 24), SENTINEL, dtype=out_dt, device=DEV)
        C = cbuf[:M, 8:8 + N]
    elif recipe == "j":
        cbuf = torch.full((-(-M // 7) * 9, N), SENTINEL, dtype=out_dt, device=DEV)
        C = cbuf
    else:
        cbuf = torch.full((M, N + ldc_extra), SENTINEL, dtype=out_dt, device=DEV)
        C = cbuf[:, :N]
        if "beta" in kw:
            C.copy_(ints((M, N), F32))
    before = cbuf.clone()
    c_old = C.clone() if "beta" in kw else None
    mask = torch.full((_ops.mask4_bytes(M, N),), 0xAA, dtype=torch.uint8, device=DEV) if want_mask else None
    part = torch.full((_ops.colsum_part_rows(M), N), SENTINEL, device=DEV) if want_csum else None
    _ops.gemm(A, B, C, M, N, Kd, A.stride(0), B.stride(0), C.stride(0), a_kcontig=akc, b_kcontig=bkc,
              mask_out=mask, colsum_part=part, **kw)
    torch.cuda.synchronize()
    for name in ("alpha", "beta", "bias", "act", "dropout_p", "seed", "drop_row_stride", "drop_row0", "res",
                 "res_rowmod"):
        if name in kw:
            ref_kw[name] = kw[name]
    pre, stored, ref_mask, ref_csum = _gemm_contract_ref(A, B, M, N, akc, bkc, out_dt, c_old=c_old, aux_bits=aux_bits,
                                                         **ref_kw)
    expect = before.clone()
    if recipe == "j":
        rows = torch.arange(M, device=DEV)
        orow = (rows // 7) * 9 + rows % 7
        expect[orow] = stored
        got = cbuf[orow]
    else:
        (expect[:M, 8:8 + N] if recipe == "k" else expect[:, :N]).copy_(stored)
        got = C
    if recipe == "d":
        # GELU, the one inexact recipe: |pre-activation| <= alpha * K + 1 < 40, where erf saturates long before the
        # fp32 rounding of the result (ulp(32) = 3.8e-6) reaches the gate
        err = (got.double() - pre).abs()
        if out_dt == F32:
            assert float(err.max()) <= 1e-5, float(err.max())
        else:
            assert bool((err <= 2.0 ** -8 * pre.abs() + 2e-5).all()), float((err - 2.0 ** -8 * pre.abs()).max())
        outside = torch.ones_like(cbuf, dtype=torch.bool)
        outside[:, :N] = False
        assert torch.equal(cbuf[outside], before[outside])
    else:
        assert torch.equal(cbuf, expect), (float((got.double() - stored.double()).abs().max()),
                                           int((cbuf != expect).sum()))
    if want_mask:
        valid = _mask4_valid(mask.numel(), M, N)
        assert torch.equal(mask[valid], ref_mask[valid])
    if want_csum:
        assert torch.equal(part, ref_csum), float((part - ref_csum).abs().max())


def _gemm_cases():
    cases = []
    for path, (_, dt, _) in GEMM_PATHS.items():
        for r in ("plain", "a", "b", "c", "d", "g", "h", "i", "j", "k", "l", "m"):
            cases.append((path, TT, r))
        cases += [(path, TF, r) for r in ("plain", "e", "f")]
        cases += [(path, FF, r) for r in ("plain", "c")]
        if dt == F32:
            cases += [(path, FT, r) for r in ("plain", "c")]
    return cases


def _lid(layout):
    return {TT: "kk", TF: "kr", FF: "rr", FT: "rk"}[layout]


@pytest.mark.parametrize("path,layout,recipe", _gemm_cases(), ids=lambda v: _lid(v) if isinstance(v, tuple) else v)
def test_gemm_contract(libopt, path, layout, recipe):
    """Epilogue recipes (a)-(m) on every kernel path and the layouts it supports, the 4-wide epilogue branch:
    a alpha | b beta, f32 C | c bias + ReLU + mask_out | d bias + GELU | e bf16 aux (ldaux = N + 8) + colsum_part |
    f mask4 aux + colsum_part + alpha | g bias + dropout + mask_out + bf16 res (ldres = N + 16) | h the same with an
    f32 res into a bf16 C | i g with drop_row_stride 5, drop_row0 3 and lda = 5 K | j res_rowmod 7 + out_group (7, 9) |
    k C a column slice (ldc = N + 24), lda = ldb = K + 8 | l split_k 3 + bias + ReLU + mask_out into bf16 (K = 128 /
    72 / 40: the last K-slice is empty) | m split_k 3 + beta, f32 C."""
    _run_gemm_recipe(libopt, path, layout, recipe)


@pytest.mark.parametrize("path", ["v1", "v2", "v4"])
def test_gemm_contract_split_k_three_full_slices(libopt, path):
    """Recipe (l) with K = 192: three k-tiles, one per slice (test_gemm_contract's K = 128 leaves the last empty)."""
    _run_gemm_recipe(libopt, path, TT, "l", k=192)


@pytest.mark.parametrize("recipe", ["a", "c", "g", "l"])
@pytest.mark.parametrize("path", list(GEMM_PATHS))
def test_gemm_contract_scalar_epilogue(libopt, path, recipe):
    """N = 10 (a 10-class head): N % 4 != 0 sets e.vec false, so every element takes epilogue4's scalar branch — and
    split-K (l) the reduce kernel's scalar slab loads."""
    _run_gemm_recipe(libopt, path, TT, recipe, n=10)


@pytest.mark.parametrize("path", list(GEMM_PATHS))
def test_gemm_contract_odd_ldc(libopt, path):
    """ldc = N + 1 for an f32 C (beta = 1, recipe b): N % 4 == 0 but the unaligned rows set e.vec false."""
    _run_gemm_recipe(libopt, path, TT, "b", ldc_extra=1)


@pytest.mark.parametrize("recipe", ["e", "f"])
@pytest.mark.parametrize("path", list(GEMM_PATHS))
def test_gemm_contract_scalar_aux(libopt, path, recipe):
    """The aux mask (bf16 with ldaux = N + 8, and mask4: the `jj & 3` bit of the group's byte) and the separate
    column-sum pass over a C with ldc = N + 1: the scalar branch again."""
    _run_gemm_recipe(libopt, path, TF, recipe, ldc_extra=1)


def test_gemm_contract_scalar_aux_ten_columns(libopt):
    """mask4 aux at N = 10 (the last byte of a row's mask holds 2 columns); the f32 kernel takes a row-strided B of
    any N."""
    _run_gemm_recipe(libopt, "f32", TF, "f", n=10)


def _partial_round_smallest_m(n):
    """The smallest M at which the 256x256 tiles of an [M][n] output start a last partial round of the 256 CUs: with
    tn = ceil(n / 256) tile columns, rounds = tm * tn // 256 >= 1 whole rounds and a last round tail =
    (tm - rounds * 256 // tn) * tn with 0 < 2 * tail <= 256 (tail_split, vit_gemm.hip); one row past the previous tile
    row."""
    tn = -(-n // 256)
    tm = 1
    while True:
        rounds = tm * tn // 256
        tail = (tm - rounds * 256 // tn) * tn
        if rounds >= 1 and 0 < 2 * tail <= 256:
            return (tm - 1) * 256 + 1
        tm += 1


@pytest.mark.parametrize("recipe", ["plain", "g"])
def test_gemm_one_row_partial_round(recipe):
    """N = 768 (3 tile columns) starts a last partial round at 86 tile rows (258 tiles = one round of 256 + a last
    round of 3), i.e. M = 85 * 256 + 1 = 21761, K = 64: a one-row last tile row, unsplit (the split-K tail is off by
    default and K is below its minimum), whose dropout indices, residual and mask4 rows continue at row 21760.  Exact
    on integers."""
    M, N, Kd = _partial_round_smallest_m(768), 768, 64
    assert M == 85 * 256 + 1
    g = torch.Generator().manual_seed(21)
    A, B = _ints((M, Kd), gen=g), _ints((N, Kd), gen=g)
    C = torch.full((M, N), SENTINEL, dtype=BF, device=DEV)
    if recipe == "plain":
        _ops.gemm(A, B, C, M, N, Kd, Kd, Kd, N)
        assert torch.equal(C, _ref_op(A, B, True, True).float().bfloat16())
        return
    bias = _ints((N,), gen=g, dtype=F32)
    res = _ints((M, N + 16), gen=g)[:, :N]
    mask = torch.full((_ops.mask4_bytes(M, N),), 0xAA, dtype=torch.uint8, device=DEV)
    kw = dict(bias=bias, dropout_p=0.5, seed=77, res=res)
    _ops.gemm(A, B, C, M, N, Kd, Kd, Kd, N, ldres=N + 16, mask_out=mask, **kw)
    _, stored, ref_mask, _ = _gemm_contract_ref(A, B, M, N, True, True, BF, **kw)
    assert torch.equal(C, stored), float((C.double() - stored.double()).abs().max())
    valid = _mask4_valid(mask.numel(), M, N)
    assert torch.equal(mask[valid], ref_mask[valid])


def test_gemm_v4_bias_gelu_side_outputs(libopt):
    """bias + GELU, the one fast v4 kind that keeps the LDS-image epilogue, with both side outputs: (264, 272, 64),
    layout kk, inputs as in recipe (d) — two tile rows, so colsum_part has a full and an 8-row block.  C is bitwise
    the general epilogue's (option gemm_epi_general); mask_out is C > 0; each colsum_part row is the fp64 column sum
    of C as stored over its 256-row block, to the fused column sums' gate (test_gpu_kernels.test_gemm_colsum_part)."""
    M, N, Kd = 264, 272, 64
    libopt("gemm_impl", 4)
    g = torch.Generator().manual_seed(_seed("bias_gelu_side", M, N, Kd))
    A, B = _ints((M, Kd), -1, 2, gen=g), _ints((N, Kd), -1, 2, gen=g)
    bias = _ints((N,), -1, 2, gen=g, dtype=F32)
    outs = []
    for general in (0, 1):
        libopt("gemm_epi_general", general)
        C = torch.full((M, N), SENTINEL, dtype=BF, device=DEV)
        mask = torch.full((_ops.mask4_bytes(M, N),), 0xAA, dtype=torch.uint8, device=DEV)
        part = torch.full((_ops.colsum_part_rows(M), N), SENTINEL, device=DEV)
        _ops.gemm(A, B, C, M, N, Kd, Kd, Kd, N, alpha=0.5, bias=bias, act=_ops.ACT_GELU, mask_out=mask,
                  colsum_part=part)
        outs.append((C, mask, part))
    torch.cuda.synchronize()
    C, mask, part = outs[0]
    assert torch.equal(C, outs[1][0])
    valid = _mask4_valid(mask.numel(), M, N)
    assert torch.equal(mask[valid], _mask4_pack(C > 0)[valid])
    assert part.shape[0] == 2
    for blk in range(part.shape[0]):
        cb = C[256 * blk:256 * (blk + 1)].double()
        err = (part[blk].double() - cb.sum(0)).abs()
        assert bool((err <= 1e-5 * cb.abs().sum(0) + 1e-5).all()), (blk, float(err.max()))


@pytest.mark.parametrize("group_m", [1, 3])
def test_gemm_group_m(libopt, group_m):
    """Option gemm_group_m: the 5 x 5 tiles of (1100, 1100, 64) visited row-major (1) and in groups of 3 tile rows
    (a last group of 2); every tile must still land on its own rows and columns."""
    libopt("gemm_group_m", group_m)
    M, N, Kd = 1100, 1100, 64
    g = torch.Generator().manual_seed(group_m)
    A, B = _ints((M, Kd), gen=g), _ints((N, Kd), gen=g)
    ref = _ref_op(A, B, True, True)
    C = torch.full((M, N), SENTINEL, dtype=F32, device=DEV)
    _ops.gemm(A, B, C, M, N, Kd, Kd, Kd, N)
    assert torch.equal(C.double(), ref)
    Cb = torch.full((M, N), SENTINEL, dtype=BF, device=DEV)
    _ops.gemm(A, B, Cb, M, N, Kd, Kd, Kd, N)
    assert torch.equal(Cb, ref.float().bfloat16())


# ---------------------------------------------------------------------------------------------------------------
# 2. attention: every instantiation, one and several items per workgroup
# ---------------------------------------------------------------------------------------------------------------
AB, AH, HD, ASCALE = 3, 3, 64, 8.0
AD = AH * HD


def _attn_inputs(T, seed):
    torch.manual_seed(seed)
    return (torch.randn(AB * T, 3 * AD, device=DEV) * 0.5).bfloat16()


def _attn_ref64(qkv, T):
    q, k, v = qkv.double().view(AB, T, 3, AH, HD).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * ASCALE
    p = torch.softmax(s, -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(AB * T, AD), torch.logsumexp(s, -1), p


def _gate_o_lse(o, lse, o_ref, lse_ref):
    assert float((o.double() - o_ref).abs().max()) <= 2e-2 * max(1.0, float(o_ref.abs().max()))
    assert float((lse.double() - lse_ref).abs().max()) <= 1e-3 * max(1.0, float(lse_ref.abs().max()))


RING_T = sorted({t for nt in range(1, 17) for t in (16 * nt - 15, 16 * nt)})


@pytest.mark.parametrize("T", RING_T)
def test_attention_ring_every_nt(libopt, T):
    """attn_fwd_ring<NT> for NT = 1..16 at T = 16 NT - 15 (the last wave holds one valid query) and 16 NT, 9 items:
    one item per workgroup (max_wgs 0), 5 and 4 items per workgroup (max_wgs 2: both slot parities, the clamped
    prefetch past the last item) and 3 / 2 items (option attn_fwd_grid 4).  Bitwise equal, within the o / lse gates
    against fp64 on the same bf16 inputs; with o32 the bf16 o is unchanged and is o32 rounded."""
    qkv = _attn_inputs(T, T)
    o_ref, lse_ref, _ = _attn_ref64(qkv, T)
    outs = []
    for wgs, opt in ((0, 0), (2, 0), (0, 4)):
        libopt("attn_fwd_grid", opt)
        o = torch.full((AB * T, AD), 3.0, device=DEV, dtype=BF)
        lse = torch.full((AB, AH, T), 3.0, device=DEV)
        _ops.attn_fwd(qkv, AB, T, AH, HD, ASCALE, o=o, lse=lse, max_wgs=wgs)
        torch.cuda.synchronize()
        _gate_o_lse(o, lse, o_ref, lse_ref)
        outs.append((o, lse))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])
    libopt("attn_fwd_grid", 0)
    o32 = torch.full((AB * T, AD), 3.0, device=DEV)
    o2, lse2 = _ops.attn_fwd(qkv, AB, T, AH, HD, ASCALE, o32=o32)
    assert torch.equal(o2, outs[0][0]) and torch.equal(lse2, outs[0][1])
    assert torch.equal(o32.bfloat16(), o2)
    assert float((o32.double() - o_ref).abs().max()) <= 2e-2 * max(1.0, float(o_ref.abs().max()))


BWD_T = sorted({t for nq in range(1, 9) for t in (32 * nq - 31, 32 * nq)})


@pytest.mark.parametrize("T", BWD_T)
def test_attention_bwd_fused_every_nq(libopt, T):
    """attn_bwd_fused<NQ> for NQ = 1..8 at T = 32 NQ - 31 and 32 NQ, 9 items: the default grid and one workgroup per
    item (shared_cus), and 5 / 4 items per workgroup (attn_bwd_grid 2: the next item staged during the current one).
    Bitwise equal, within the gradient gate of the same-rounding fp64 reference."""
    qkv = _attn_inputs(T, 1000 + T)
    o, lse = _ops.attn_fwd(qkv, AB, T, AH, HD, ASCALE)
    d_o = torch.randn(AB * T, AD, device=DEV).bfloat16()
    base = _ops.attn_bwd(qkv, o, d_o, lse, AB, T, AH, HD, ASCALE)
    shared = _ops.attn_bwd(qkv, o, d_o, lse, AB, T, AH, HD, ASCALE, shared_cus=True)
    libopt("attn_bwd_grid", 2)
    two = _ops.attn_bwd(qkv, o, d_o, lse, AB, T, AH, HD, ASCALE)
    torch.cuda.synchronize()
    assert torch.equal(shared, base)
    assert torch.equal(two, base)
    _check_attn_bwd_bf16(base, _attn_flash_grads(qkv, d_o, AB, T, AH, HD, ASCALE), AD)


@pytest.mark.parametrize("T", [257, 384, 385])
def test_attention_tiled_block_edges(libopt, T):
    """The tiled kernels one row past two 128-row blocks, at exactly three blocks and one row past them (the body of
    test_attention_tiled_kernels_any_grid)."""
    K.test_attention_tiled_kernels_any_grid(libopt, AB, AH, T)


@pytest.mark.parametrize("T", [17, 65, 197])
def test_attention_probs_forward_feeds_mfma_backward(T):
    """attn_fwd(probs=...) on bf16 hd = 64 runs the generic VALU kernel (the default training forward of small
    batches); its o and lse then feed the fused MFMA backward.  probs against the fp64 softmax to 1e-5 with rows
    summing to 1, o / lse within their gates, the backward within the gradient gate, and the lse of the MFMA forward
    (no probs) within the lse gate of it."""
    qkv = _attn_inputs(T, 2000 + T)
    o_ref, lse_ref, p_ref = _attn_ref64(qkv, T)
    probs = torch.full((AB, AH, T, T), 3.0, device=DEV)
    o, lse = _ops.attn_fwd(qkv, AB, T, AH, HD, ASCALE, probs=probs)
    assert float((probs.double() - p_ref).abs().max()) <= 1e-5
    assert float((probs.double().sum(-1) - 1.0).abs().max()) <= 1e-5
    _gate_o_lse(o, lse, o_ref, lse_ref)
    d_o = torch.randn(AB * T, AD, device=DEV).bfloat16()
    dqkv = _ops.attn_bwd(qkv, o, d_o, lse, AB, T, AH, HD, ASCALE)
    _check_attn_bwd_bf16(dqkv, _attn_flash_grads(qkv, d_o, AB, T, AH, HD, ASCALE), AD)
    o_m, lse_m = _ops.attn_fwd(qkv, AB, T, AH, HD, ASCALE)
    assert float((lse_m - lse).abs().max()) <= 1e-3 * max(1.0, float(lse_ref.abs().max()))
    _gate_o_lse(o_m, lse_m, o_ref, lse_ref)


# ---------------------------------------------------------------------------------------------------------------
# 3. LayerNorm: every NV, both forward kernels, both accumulator forms
# ---------------------------------------------------------------------------------------------------------------
LN_P, LN_SEED = 0.2, 99


def _ln_tol(dtype):
    return 2e-5 if dtype == F32 else 2e-2


def _ln_inputs(dtype, rows, cols, ld=None, seed=3):
    """x, dy (column slices of [rows, ld] buffers when ld is given), dres, gamma, beta"""
    torch.manual_seed(seed + cols)
    ld = ld or cols
    x = (torch.randn(rows, ld, device=DEV) * 2 + 0.5).to(dtype)[:, :cols]
    dy = torch.randn(rows, ld, device=DEV).to(dtype)[:, :cols]
    dres = torch.randn(rows, cols, device=DEV).to(dtype)
    return x, dy, dres, torch.rand(cols, device=DEV) + 0.5, torch.randn(cols, device=DEV)


def _ln_run(x, dy, dres, g, b, ld=None, drop_mask=None):
    """forward + backward with the fused dropout and the third partial set; y is a column slice of a sentinel-filled
    [rows, ld] buffer"""
    rows, cols = x.shape
    ybuf = torch.full((rows, ld or cols), SENTINEL, dtype=x.dtype, device=DEV)
    y = ybuf[:, :cols]
    _, mean, rstd = _ops.layernorm_fwd(x, g, b, y=y)
    dx, drop = torch.empty(rows, cols, dtype=x.dtype, device=DEV), torch.empty(rows, cols, dtype=x.dtype, device=DEV)
    part = _ops.layernorm_bwd(dy, x, g, mean, rstd, dx, dres=dres, drop_out=drop, drop_p=LN_P, drop_seed=LN_SEED,
                              osum=True, drop_mask=drop_mask)
    sums = [torch.zeros(cols, device=DEV) for _ in range(3)]
    _ops.colsum_finish(part, sums)
    torch.cuda.synchronize()
    return dict(ybuf=ybuf, y=y, mean=mean, rstd=rstd, dx=dx, drop=drop, part=part, dg=sums[0], db=sums[1], ds=sums[2])


def _ln_gate(r, x, dy, dres, g, b):
    """the assertions of test_layernorm_fwd_bwd, against fp64 torch on the stored inputs"""
    rows, cols = x.shape
    tol = _ln_tol(x.dtype)
    xr = x.double().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (cols,), gr, br, 1e-5)
    yr.backward(dy.double())
    assert float((r["y"].double() - yr.detach()).abs().max()) <= tol * 4
    assert bool((r["ybuf"][:, cols:] == SENTINEL).all())
    ref_dx = xr.grad + dres.double()
    assert float((r["dx"].double() - ref_dx).abs().max()) <= tol * 4 * float(ref_dx.abs().max())
    assert float((r["dg"] - gr.grad).abs().max()) <= tol * 4 * float(gr.grad.abs().max())
    assert float((r["db"] - br.grad).abs().max()) <= tol * 4 * float(br.grad.abs().max())
    keep = O.dropout_keep(LN_SEED, (rows, cols), LN_P).to(DEV)
    assert torch.equal(r["drop"].float(), r["dx"].float() * keep)
    ref_ds = r["drop"].double().sum(0) / (1.0 - LN_P)
    assert bool(((r["ds"].double() - ref_ds).abs() <= 1e-5 * r["drop"].double().abs().sum(0) + 1e-6).all())
    # without drop_out the third set sums dx_out
    dx2 = torch.empty_like(r["dx"])
    part2 = _ops.layernorm_bwd(dy, x, g, r["mean"], r["rstd"], dx2, dres=dres, osum=True)
    assert torch.equal(dx2, r["dx"])
    s3 = [torch.zeros(cols, device=DEV) for _ in range(3)]
    _ops.colsum_finish(part2, s3)
    dxs = r["dx"].double()
    assert bool(((s3[2].double() - dxs.sum(0)).abs() <= 1e-5 * dxs.abs().sum(0) + 1e-6).all())
    assert torch.allclose(s3[0], r["dg"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols", [200, 260, 512, 1000, 1284, 1536, 2048, 3076, 4096])
def test_layernorm_every_width(dtype, cols):
    """NV 1 (200), 2 (260, 512), 4 (1000), 6 (1284, 1536), 8 (2048), 16 (3076, 4096), with a partly empty last
    256-column piece (200, 260, 1000, 1284, 3076); cols % 8 == 4 is the 8-byte bf16 forward.  37 rows: odd (the 16-B
    forward's half-wave without a second row), a last group of one row, the few-rows spread of the backward."""
    x, dy, dres, g, b = _ln_inputs(dtype, 37, cols)
    _ln_gate(_ln_run(x, dy, dres, g, b), x, dy, dres, g, b)


@pytest.mark.parametrize("rows", [1, 2, 3, 5])
def test_layernorm_few_rows_saved_mask(rows):
    """A drop_mask group of fewer than 4 rows: the saved-mask form equals the hash form bit for bit."""
    x, dy, dres, g, b = _ln_inputs(BF, rows, 768)
    keep = O.dropout_keep(LN_SEED, (rows, 768), LN_P).to(DEV)
    h = _ln_run(x, dy, dres, g, b)
    m = _ln_run(x, dy, dres, g, b, drop_mask=_mask4_pack(keep.bool()))
    for k in ("y", "dx", "drop", "part"):
        assert torch.equal(h[k], m[k]), k
    _ln_gate(m, x, dy, dres, g, b)


@pytest.mark.parametrize("dtype,ld", [(F32, 776), (F32, 772), (BF, 776), (BF, 772)],
                         ids=["fp32-776", "fp32-772", "bf16-776", "bf16-772"])
def test_layernorm_strided_rows(dtype, ld):
    """x, y and dy as column slices with row stride 776 (a multiple of 8: bf16 keeps the 16-B forward) and 772
    (% 8 == 4: the 8-byte fallback); the gap columns of y keep their sentinel."""
    x, dy, dres, g, b = _ln_inputs(dtype, 37, 768, ld=ld)
    assert x.stride(0) == ld and dy.stride(0) == ld
    r = _ln_run(x, dy, dres, g, b, ld=ld)
    _ln_gate(r, x, dy, dres, g, b)
    if ld % 8 == 0 or dtype == F32:            # the kernels of contiguous rows, seeing only another stride: same bits
        c = _ln_run(x.contiguous(), dy.contiguous(), dres, g, b)
        for k in ("y", "mean", "rstd", "dx", "drop", "part"):
            assert torch.equal(r[k], c[k]), k


@pytest.mark.parametrize("cols", [768, 1536, 3072])
def test_layernorm_ln16_option(libopt, cols):
    """bf16 forward: the 16-B kernel (ln16 1) against the 8-byte one (ln16 0).  They sum in different orders: mean and
    rstd to 1e-6 relative, y within the gate of each other and of fp64."""
    x, dy, dres, g, b = _ln_inputs(BF, 37, cols)
    outs = []
    for v in (1, 0):
        libopt("ln16", v)
        outs.append(_ln_run(x, dy, dres, g, b))
        _ln_gate(outs[-1], x, dy, dres, g, b)
    a, c = outs
    for k in ("mean", "rstd"):
        assert float((a[k] - c[k]).abs().max()) <= 1e-6 * float(a[k].abs().max()), k
    assert float((a["y"].float() - c["y"].float()).abs().max()) <= _ln_tol(BF) * 4


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols", [768, 1536, 3072])
def test_layernorm_accumulator_forms(libopt, dtype, cols):
    """Backward accumulators in LDS (ln_al 1) against registers (ln_al 0): the per-row arithmetic is shared, so dx and
    drop_out are bitwise equal; the finished column sums to rtol = atol = 1e-5."""
    x, dy, dres, g, b = _ln_inputs(dtype, 37, cols)
    outs = []
    for v in (1, 0):
        libopt("ln_al", v)
        outs.append(_ln_run(x, dy, dres, g, b))
        _ln_gate(outs[-1], x, dy, dres, g, b)
    a, c = outs
    assert torch.equal(a["dx"], c["dx"]) and torch.equal(a["drop"], c["drop"])
    for k in ("dg", "db", "ds"):
        assert torch.allclose(a[k], c[k], rtol=1e-5, atol=1e-5), k


# ---------------------------------------------------------------------------------------------------------------
# 4. entry points without a direct test
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,P", [((2, 3, 64, 48), 16), ((2, 3, 32, 32), 4)], ids=["P16", "P4"])
def test_col2im(shape, P):
    """col2im is the inverse of im2col (asymmetric image: a swapped h % P / w % P cannot pass) and equals the torch
    permutation for f32 -> f32, bf16 -> bf16 and bf16 cols -> f32 image."""
    torch.manual_seed(8)
    B, C, H, W = shape
    x = torch.randn(shape, device=DEV)
    n = (H // P) * (W // P)

    def perm(img):        # [B, C, H, W] -> [B*N, C*P*P], column order (c, kh, kw)
        return img.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * n, C * P * P)

    cols = _ops.im2col(x, P, F32)
    assert torch.equal(cols, perm(x))
    back = _ops.col2im(cols, torch.full_like(x, SENTINEL), P)
    assert torch.equal(back, x)
    xb = x.bfloat16()
    colsb = perm(xb).contiguous()
    assert torch.equal(_ops.col2im(colsb, torch.full_like(xb, SENTINEL), P), xb)
    assert torch.equal(_ops.col2im(colsb, torch.full_like(x, SENTINEL), P), xb.float())
    cols2 = torch.randn(B * n, C * P * P, device=DEV)                  # and from columns that are no image's
    ref = cols2.view(B, H // P, W // P, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(shape)
    assert torch.equal(_ops.col2im(cols2, torch.full_like(x, SENTINEL), P), ref)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_embed_cls(dtype):
    torch.manual_seed(9)
    B, T, D = 3, 5, 200
    cls, pos = torch.randn(B, D, device=DEV), torch.randn(T, D, device=DEV)
    x0 = torch.full((B * T, D), SENTINEL, dtype=dtype, device=DEV)
    _ops.embed_cls(cls, pos, x0, B, T, D)
    want = torch.full((B, T, D), SENTINEL, dtype=dtype, device=DEV)
    want[:, T - 1] = (cls + pos[T - 1]).to(dtype)                        # one rounding of the fp32 sum
    assert torch.equal(x0.view(B, T, D), want)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_relu_bwd(dtype):
    torch.manual_seed(10)
    n = 5000
    y = torch.randn(n, device=DEV).to(dtype)
    y[::7] = 0.0
    y[3::7] = -0.0
    dy = torch.randn(n, device=DEV).to(dtype)
    dx = _ops.relu_bwd(dy, y, torch.full_like(dy, SENTINEL))
    assert torch.equal(dx, dy * (y > 0))


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, BF), (BF, F32), (BF, BF)],
                         ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
def test_mask4_apply(xdt, ydt, scale):
    torch.manual_seed(11)
    rows, cols = 37, 200
    bits = torch.rand(rows, cols, device=DEV) < 0.5
    x = torch.randn(rows, cols + 8, device=DEV).to(xdt)[:, :cols]
    ybuf = torch.full((rows, cols + 12), SENTINEL, dtype=ydt, device=DEV)
    _ops.mask4_apply(x, ybuf[:, :cols], _mask4_pack(bits), scale=scale)
    want = (x.float() * bits * scale).to(ydt)                            # x * scale is exact in fp32: one rounding
    assert torch.equal(ybuf[:, :cols], want)
    assert bool((ybuf[:, cols:] == SENTINEL).all())


def _table(ps, shadows):
    z = [torch.zeros_like(p) for p in ps]
    return _ops.build_chunk_table([(p, p, a, a, s) for p, a, s in zip(ps, z, shadows)], DEV)


def test_pack():
    """vit_pack after external writes to the fp32 params: shadow = (dtype) p for bf16 and f32 shadows, a NULL-shadow
    entry is skipped (its neighbours still land in their own shadows)."""
    torch.manual_seed(12)
    shapes = [(300,), (70000,), (1,)]
    for dt in (BF, F32):
        ps = [torch.randn(s, device=DEV) for s in shapes] + [torch.randn(300, device=DEV)]
        sh = [torch.full(s, SENTINEL, dtype=dt, device=DEV) for s in shapes] + [None]
        table, n = _table(ps, sh)
        for p in ps:
            p.copy_(torch.randn_like(p))
        before = [p.clone() for p in ps]
        _ops.pack(table, n, dt)
        torch.cuda.synchronize()
        for p, p0, s in zip(ps, before, sh):
            assert torch.equal(p, p0)
            if s is not None:
                assert torch.equal(s, p.to(dt))


@pytest.mark.parametrize("shadow", ["f32", "null"])
def test_adamw_grad_scale_and_shadows(shadow):
    """grad_scale = 0.125 against torch AdamW fed g * 0.125, with an f32 shadow and with none; 8193 elements are one
    past a chunk."""
    torch.manual_seed(13)
    shapes = [(300,), (8193,), (128, 64)]
    ps = [torch.randn(s, device=DEV) for s in shapes]
    gs = [torch.randn(s, device=DEV) for s in shapes]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    sh = [torch.full(s, SENTINEL, device=DEV) if shadow == "f32" else None for s in shapes]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-4)
    table, n = _ops.build_chunk_table(list(zip(ps, gs, ms, vs, sh)), DEV)
    assert n == sum(-(-p.numel() // _ops.CHUNK) for p in ps) and _ops.CHUNK < 8193 <= 2 * _ops.CHUNK
    for step in range(1, 4):
        for r, g in zip(ref, gs):
            r.grad = g * 0.125
        opt.step()
        _ops.adamw(table, n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1 - 0.9 ** step, 1 - 0.999 ** step, 0.125, F32)
    for p, r, s in zip(ps, ref, sh):
        assert float((p - r.detach()).abs().max()) < 1e-6
        if s is not None:
            assert torch.equal(s, p)


def test_copy2d_casts():
    """f32 -> bf16 and bf16 -> f32 with grouped source rows, and the cast accumulated onto the destination (beta 1)."""
    torch.manual_seed(14)
    for sdt, ddt in ((F32, BF), (BF, F32)):
        src = torch.randn(4 * 5, 24, device=DEV).to(sdt)
        want_rows = src.view(4, 5, 24)[:, :3, :20].reshape(12, 20)
        dst = torch.full((12, 28), SENTINEL, dtype=ddt, device=DEV)
        _ops.copy2d(src, 24, dst, 28, 12, 20, group=(3, 5))
        assert torch.equal(dst[:, :20], want_rows.to(ddt)) and bool((dst[:, 20:] == SENTINEL).all())
        acc = torch.randn(12, 28, device=DEV).to(ddt)
        acc0 = acc.clone()
        _ops.copy2d(src, 24, acc, 28, 12, 20, group=(3, 5), beta=1.0)
        assert torch.equal(acc[:, :20], (want_rows.float() + acc0[:, :20].float()).to(ddt))
        assert torch.equal(acc[:, 20:], acc0[:, 20:])


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("rows", [1, 33, 1000])
def test_colsum_bf16_strided(rows, beta):
    torch.manual_seed(15 + rows)
    cols, ld = 301, 304
    x = torch.randn(rows, ld, device=DEV).bfloat16()
    out0 = torch.randn(cols + 3, device=DEV)
    out = out0.clone()
    _ops.colsum(x, rows, cols, ld, out, beta=beta, alpha=0.25)
    xs = x[:, :cols].double()
    ref = beta * out0[:cols].double() + 0.25 * xs.sum(0)
    assert bool(((out[:cols].double() - ref).abs() <= 1e-5 * xs.abs().sum(0) + 1e-6).all())
    assert torch.equal(out[cols:], out0[cols:])


@pytest.mark.parametrize("rows,classes,extreme", [(1, 4, False), (8, 10, False), (37, 257, True), (300, 1000, False)])
def test_softmax_xent(rows, classes, extreme):
    """The loader's class counts (4, 10), one past a block of 256 threads, and the benchmark's 1000.  `extreme`: every
    row's maximum is 80 and another entry is -80 — finite, and shift-invariant.  Labels include class 0 and
    classes - 1."""
    torch.manual_seed(16 + classes)
    lg = (torch.randn(rows, classes, device=DEV) * 4 * 1024).round() / 1024    # a 2^-10 grid: shifts are exact
    if extreme:
        lg = lg.clamp(-60, 60)
        idx = torch.arange(rows, device=DEV)
        lg[idx, idx % classes] = 80.0
        lg[idx, (idx + 5) % classes] = -80.0
    lb = torch.randint(0, classes, (rows,), device=DEV)
    lb[0] = 0
    lb[-1] = classes - 1 if rows > 1 else 0
    if rows > 2:
        lb[1] = classes - 1

    def check(logits):
        loss, dl = _ops.softmax_xent(logits.contiguous(), lb)
        lr_ = logits.double().requires_grad_(True)
        lref = torch.nn.functional.cross_entropy(lr_, lb)
        lref.backward()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
        assert abs(loss.item() - lref.item()) <= 1e-5 * max(1.0, abs(lref.item()))
        assert float((dl.double() - lr_.grad).abs().max()) <= 1e-6
        assert float(dl.double().sum(-1).abs().max()) <= 1e-6
        return loss, dl

    loss, dl = check(lg)
    loss_s, dl_s = check(lg - 16.0)                                     # exact in fp32 (|x| <= 96, 2^-10 grid)
    assert abs(loss.item() - loss_s.item()) <= 1e-5 * max(1.0, abs(loss.item()))
    assert float((dl - dl_s).abs().max()) <= 1e-6
