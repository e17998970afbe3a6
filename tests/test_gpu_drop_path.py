"""Stochastic depth (drop path) on the MI355X: the factor-table kernel against its Python twin, vit_gemm_rowscale on
every kernel and epilogue that applies the dropout (the 256x256 kernel's new fast kind against the general epilogue,
the 128x128 kernel, the fp32 kernel, the split-K reduce) against vit_gemm and fp64, and the whole model in train mode
against the oracle, which is called unchanged with float masks (element keep & image keep) / (1 - p_l)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _engine, _lib, _ops, config, vit
    from VisionTransformer.optim import cross_entropy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BASE_SEED = 195950210         # what torch.manual_seed(42) makes the engine's forward draw


# ---- the table kernel -----------------------------------------------------------------------------------------------
def _twin_table(seed, rates, B, T):
    L = len(rates)
    t = torch.empty(L, 2, B, T)
    for l, p in enumerate(rates):
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        for site in (0, 1):
            t[l, site] = (_engine.path_keep(seed, L, l, site, B, p).float() * scale)[:, None]
    return t.reshape(L, 2, B * T)


def test_drop_path_rows_is_the_twins_table():
    rates, B, T = [0.0, 0.25, 0.5], 5, 3
    got = _ops.drop_path_rows(BASE_SEED, rates, B, T, DEV)
    want = _twin_table(BASE_SEED, rates, B, T)
    assert got.shape == (3, 2, B * T) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    assert bool((got[0] == 1.0).all())                                   # rate 0: every row 1.0f
    vals = set(got[1:].unique().tolist())
    assert vals == {0.0, float(np.float32(1) / np.float32(0.75)), 2.0}   # both outcomes occur at both rates
    # another data-parallel rank draws another table
    seed1 = _engine.dropout_seed(BASE_SEED, 1)
    got1 = _ops.drop_path_rows(seed1, rates, B, T, DEV)
    assert torch.equal(got1.cpu(), _twin_table(seed1, rates, B, T)) and not torch.equal(got1, got)
    with pytest.raises(RuntimeError, match="vit_drop_path_rows"):
        _ops.drop_path_rows(BASE_SEED, [0.0, 1.0], B, T, DEV)
    with pytest.raises(ValueError, match="layers"):
        _ops.drop_path_rows(BASE_SEED, [0.1] * 65, B, T, DEV)


# ---- vit_gemm_rowscale ----------------------------------------------------------------------------------------------
def _mask4_bits(mask, m, n):
    """A VIT_MASK4 buffer of an [m][n] tensor as a bool [m, n] (vit_hip.h: byte ((i/4) ceil(n/4) + j/4) 4 + i%4, bit
    j%4)."""
    m4, n4 = (m + 3) // 4, (n + 3) // 4
    b = mask[:4 * m4 * n4].view(m4, n4, 4, 1).to(torch.int32)
    bits = (b >> torch.arange(4, device=mask.device, dtype=torch.int32)) & 1          # [m4, n4, row, col]
    return bits.permute(0, 2, 1, 3).reshape(4 * m4, 4 * n4)[:m, :n].bool()


class _choices:
    """The kernel choices (vit_gemm_kernel_choice) of every _ops.gemm call made inside the block."""

    def __enter__(self):
        self.prev, _ops.GEMM_CHOICE_LOG = _ops.GEMM_CHOICE_LOG, []
        return _ops.GEMM_CHOICE_LOG

    def __exit__(self, *exc):
        _ops.GEMM_CHOICE_LOG = self.prev
        return False


def _rowscale_case(dtype, m, n, k, p, rs, row0, split_k=1, *, expect):
    """`expect`: the (kernel generation, 256x256 epilogue kind) the library must choose for the call with the table."""
    g = torch.Generator().manual_seed(m * 7 + n * 3 + rs + row0)
    A = torch.randn(m, k, generator=g).to(DEV).to(dtype)
    W = (torch.randn(n, k, generator=g) * 0.1).to(DEV).to(dtype)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(m, n, generator=g).to(DEV).to(dtype)
    seed = 4242
    rows = (torch.arange(m) + row0) * rs                   # the dropout's (and the table's) row index of output row i
    # factors from {0, 1, 2}, at least one of each; every entry that must NOT be read is NaN, which would reach C
    f = torch.randint(0, 3, (m,), generator=g).float()
    f[:3] = torch.tensor([0.0, 1.0, 2.0])
    f = f[torch.randperm(m, generator=g)]
    table = torch.full(((m + row0) * rs,), float("nan"))
    table[rows] = f
    table = table.to(DEV)
    kw = dict(bias=bias, res=res, ldres=n, dropout_p=p, seed=seed, drop_row_stride=rs, drop_row0=row0,
              split_k=split_k)

    def run(row_scale, a=A):
        out = torch.empty(m, n, dtype=dtype, device=DEV)
        mask = torch.zeros(_ops.mask4_bytes(m, n), dtype=torch.uint8, device=DEV)
        _ops.gemm(a, W, out, m, n, k, k, k, n, mask_out=mask, row_scale=row_scale, **kw)
        return out, mask

    with _choices() as log:
        out, mask = run(table)
    assert [(c["impl"], c["kind"], c["row_scale"]) for c in log] == [(*expect, True)], log
    # a table of 1.0 is vit_gemm, bit for bit (values and mask)
    ones = torch.ones_like(table)
    o1, m1 = run(ones)
    o0, m0 = run(None)
    assert torch.equal(o1, o0) and torch.equal(m1, m0)
    # the kernel's own epilogue kind is the general epilogue, bit for bit
    prev = _lib.set_option("gemm_epi_general", 1)
    try:
        with _choices() as log:
            og, mg = run(table)
    finally:
        _lib.set_option("gemm_epi_general", prev)
    assert [c["kind"] for c in log] == [_lib.EPI_GENERAL], log
    assert torch.equal(out, og) and torch.equal(mask, mg)
    # fp64 over the same inputs and the same hash mask
    keep = torch.ones(m, n, dtype=torch.bool)
    if p > 0:
        keep = O.dropout_keep(seed, ((m + row0) * rs, n), p)[rows]
    keep = keep.to(DEV)
    fd = f.to(DEV).double()[:, None]
    y = A.double() @ W.double().t() + bias.double()
    ref = res.double() + torch.where(fd != 0, y * keep / (1.0 - p) * fd, torch.zeros_like(y))
    tol = 1e-4 if dtype == torch.float32 else 3e-2          # test_gemm_epilogue_bias_relu_dropout_residual's
    zero, two = (f == 0).to(DEV), (f == 2).to(DEV)
    bits = _mask4_bits(mask, m, n)
    assert bool((out[zero] == res[zero]).all())            # a dropped row is its residual row ...
    assert not bool(bits[zero].any())                      # ... with every mask bit clear
    for sel in (two, ~zero):
        err = (out[sel].double() - ref[sel]).abs().max().item()
        assert err <= tol * max(1.0, ref[sel].abs().max().item()), (err, tol)
    want_bits = (keep if p > 0 else out > 0) & ~zero[:, None]
    assert torch.equal(bits, want_bits)
    # a NaN in the branch of a dropped row does not reach C (the zero is a select, not a product)
    An = A.clone()
    victim = int(torch.nonzero(zero)[0])
    An[victim, 0] = float("nan")
    on, mn = run(table, An)
    assert not bool(torch.isnan(on.float()).any())
    assert torch.equal(on, out) and torch.equal(mn, mask)


@pytest.mark.parametrize("rs,row0", [(1, 0), (3, 0), (1, 136)])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("n", [256, 328])
@pytest.mark.parametrize("m", [256, 392])
def test_gemm_rowscale_bf16_256_tile(m, n, p, rs, row0):
    """gemm_impl automatic: m, n >= 256 runs the 256x256 kernel, whose dropout + residual epilogue with a row factor
    is a fast kind of its own (k = 128; a full tile, and ragged ones in both directions) — and the library says that
    this kind is what it launches."""
    _rowscale_case(torch.bfloat16, m, n, 128, p, rs, row0, expect=(4, _lib.EPI_BDRS))


@pytest.mark.parametrize("dtype,m,n,k,split_k,impl", [
    (torch.float32, 40, 72, 128, 1, 0),        # the fp32 kernel
    (torch.bfloat16, 136, 256, 128, 1, 2),     # the 128x128 kernel
    (torch.bfloat16, 16, 256, 128, 2, 2)])     # its split-K slabs and the reduce (the pruned block's path)
def test_gemm_rowscale_other_kernels(dtype, m, n, k, split_k, impl):
    for p, rs, row0 in ((0.2, 1, 0), (0.0, 3, 0), (0.2, 1, 136)):
        _rowscale_case(dtype, m, n, k, p, rs, row0, split_k, expect=(impl, _lib.EPI_GENERAL))


def test_gemm_rowscale_table_must_reach_the_last_row():
    A = torch.zeros(8, 64, device=DEV)
    out = torch.empty(8, 8, device=DEV)
    with pytest.raises(ValueError, match="row_scale"):
        _ops.gemm(A, A, out, 8, 8, 64, 64, 64, 8, row_scale=torch.ones(8, device=DEV), drop_row0=1)
    with pytest.raises(TypeError, match="row_scale"):
        _ops.gemm(A, A, out, 8, 8, 64, 64, 64, 8, row_scale=torch.ones(8, device=DEV, dtype=torch.float64))


# ---- the model ------------------------------------------------------------------------------------------------------
RATES = [0.3, 0.5]


def _ocfg(D, H, B):
    ocfg = O.make_config("micro", img=64, batch=B, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = D, H
    return ocfg


def _model(ocfg, st, dtype=torch.float32, **kw):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype, **kw)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st)
    return m.to(DEV)


def _oracle_masks(ocfg, rates, seed=BASE_SEED):
    """{(l, site): float [B, T, D]} = (element keep & image keep) / (1 - p_l) — every site must have both a kept and a
    dropped image, or the test would not see a wrong draw."""
    L, B, T, D = ocfg.num_blocks, ocfg.batch_size, ocfg.num_patches + 1, ocfg.embedding_size
    masks = {}
    for l, p in enumerate(rates):
        for site in (0, 1):
            pk = _engine.path_keep(seed, L, l, site, B, p)
            assert 0 < int(pk.sum()) < B, (l, site, pk)
            dk = O.dropout_keep(O.site_seed(seed, l, site), (B, T, D))
            masks[(l, site)] = (dk & pk[:, None, None]).float() / (1.0 - p)
    return masks


def _oracle_grads(st, x, y, ocfg, masks, **kw):
    """O.loss_and_grads with explicit masks (O.forward unchanged)."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in st.items()}
    logits = O.forward(params, x, ocfg, train=True, masks=masks, **kw)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in params.items()}


def _step(m, x, y, between=None):
    torch.manual_seed(42)
    drawn = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    assert drawn == BASE_SEED, f"torch.manual_seed(42) makes the forward draw {drawn}, the masks are BASE_SEED's"
    torch.manual_seed(42)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    if between is not None:
        between()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return logits.detach(), loss.detach(), grads


_FP32 = {}


def _fp32_reference():
    """The fp32 oracle run shared by the fp32 model tests (computed once, never modified)."""
    if not _FP32:
        ocfg = _ocfg(128, 2, 8)
        st = O.init_state(ocfg, seed=1)
        x, y = O.synthetic_batch(ocfg)
        torch.manual_seed(42)
        assert int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) == BASE_SEED
        _FP32.update(ocfg=ocfg, st=st, x=x, y=y, ref=_oracle_grads(st, x, y, ocfg, _oracle_masks(ocfg, RATES)))
    return _FP32


@pytest.mark.parametrize("prune", [True, False])
def test_model_fp32_vs_oracle(prune):
    """test_hd64_fp32_vs_oracle's shape at B = 8 (two half-batch chains) and its gates, rates [0.3, 0.5]; one chain
    (fwd_streams = 1) gives the same bits."""
    r = _fp32_reference()
    ocfg, x, y = r["ocfg"], r["x"], r["y"]
    lg_ref, loss_ref, g_ref = r["ref"]
    m = _model(ocfg, r["st"]).train()
    m.drop_path_rates = RATES
    m.hip_engine.prune_last = prune
    assert m.hip_engine.fwd_streams == 2
    logits, loss, grads = _step(m, x, y)
    err = (logits.cpu() - lg_ref).abs().max().item()
    print(f"fp32 prune={prune}: logits max err {err:.3e}, loss err {abs(loss.item() - loss_ref.item()):.3e}")
    assert err < 1e-4
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    for k, g in grads.items():
        e = (g.cpu() - g_ref[k]).abs().max().item()
        assert math.isfinite(e) and e <= 2e-4 * max(1.0, g_ref[k].abs().max().item()), (k, e)
    # the drop path did something: the plain-dropout oracle is far away
    lg_plain = O.forward(r["st"], x, ocfg, train=True, seed=BASE_SEED)
    assert (lg_plain - lg_ref).abs().max().item() > 0.1
    m.hip_engine.fwd_streams = 1
    logits1, loss1, grads1 = _step(m, x, y)
    assert torch.equal(logits1, logits) and torch.equal(loss1, loss)
    assert all(torch.equal(grads1[k], grads[k]) for k in grads)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(b.double().norm(), 1e-30))


_BF16 = {}


def _bf16_reference(B):
    """The two oracle runs (bf16 storage rounding, fp32) of the bf16 model tests at batch B (computed once each)."""
    if B not in _BF16:
        ocfg = _ocfg(256, 4, B)
        st = O.init_state(ocfg, seed=2)
        x, y = O.synthetic_batch(ocfg)
        masks = _oracle_masks(ocfg, RATES)
        _BF16[B] = dict(ocfg=ocfg, st=st, x=x, y=y, bf=_oracle_grads(st, x, y, ocfg, masks, bf16=True),
                        f32=_oracle_grads(st, x, y, ocfg, masks))
    return _BF16[B]


@pytest.mark.parametrize("B,streams,prune,launches,wide", [
    (16, 1, True, 4, 2),   # one chain of M = 272 rows, a full 256-row tile and a ragged one; last block: 16 rows, split-K
    (16, 1, False, 4, 4),  # ... and the last block's 272 rows too
    (32, 2, False, 8, 8),  # two half-batch chains of 272 rows each (dropout_row0 = 272 on the second)
    (16, 2, True, 6, 0)])  # two chains of 136 rows: the 128x128 kernel, and the split-K reduce
def test_model_bf16_vs_oracle_same_rounding(B, streams, prune, launches, wide):
    """D = 256 in bf16 at test_bf16_vs_oracle_same_rounding's gates: the engine's table, keep bits and backward
    scalars through the 256x256 kernel's new epilogue kind — `launches` row-factor GEMMs in the forward, of which `wide` are the ones the library
    says run that kind (vit_gemm_kernel_choice), the path of every proj / fc2 GEMM of a real training step — and, in the last
    case, through the general epilogue of the smaller kernels."""
    r = _bf16_reference(B)
    ocfg, x, y = r["ocfg"], r["x"], r["y"]
    lg_bf, _, g_bf = r["bf"]
    _, _, g_32 = r["f32"]
    m = _model(ocfg, r["st"], dtype=torch.bfloat16).train()
    m.drop_path_rates = RATES
    m.hip_engine.prune_last = prune
    m.hip_engine.fwd_streams = streams
    with _choices() as log:
        logits, loss, grads = _step(m, x, y)
    scaled = [c for c in log if c["row_scale"]]
    assert len(scaled) == launches, scaled               # proj and fc2 of both blocks, per chain where chains run
    bdrs = [c for c in scaled if (c["impl"], c["kind"]) == (4, _lib.EPI_BDRS)]
    assert len(bdrs) == wide and all(c["m"] >= 256 and c["n"] >= 256 for c in bdrs), scaled
    assert math.isfinite(loss.item())
    e = _rel(logits.float().cpu(), lg_bf)
    print(f"bf16 prune={prune}: logits rel err {e:.3e}")
    assert e < 1e-2
    worst = []
    for k, g in grads.items():
        ours, ora = _rel(g.cpu(), g_32[k]), _rel(g_bf[k], g_32[k])
        worst.append((ours / max(ora, 1e-9), k, ours, ora))
        assert ours <= max(1e-2, 2 * ora), (k, ours, ora)
    print("bf16 worst grad error ratios:", sorted(worst)[-3:])


def test_no_change_when_off():
    r = _fp32_reference()
    ocfg, x, y, st = r["ocfg"], r["x"], r["y"], r["st"]
    plain = _model(ocfg, st)
    zero = _model(ocfg, st, drop_path_rate=0.0)
    on = _model(ocfg, st, drop_path_rate=0.5)
    assert on.drop_path_rates == [0.0, 0.5] and zero.drop_path_rates == [0.0, 0.0]
    # eval: a model with rates > 0 is the rate-0 model
    a, b = _step(on.eval(), x, y), _step(zero.eval(), x, y)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    with torch.no_grad():
        assert torch.equal(on(x.to(DEV)), zero(x.to(DEV)))
    # train, rate 0: the model built without the keyword, under the same seed
    a, b = _step(zero.train(), x, y), _step(plain.train(), x, y)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    # ... while a rate > 0 changes the training forward, also without a tape
    c = _step(on.train(), x, y)
    assert not torch.equal(c[0], a[0])
    with torch.no_grad():
        torch.manual_seed(42)
        assert torch.equal(on(x.to(DEV)), c[0])


def test_backward_uses_the_forwards_rates():
    r = _fp32_reference()
    ocfg, x, y = r["ocfg"], r["x"], r["y"]
    m = _model(ocfg, r["st"]).train()
    m.drop_path_rates = RATES
    want = _step(m, x, y)

    def change():
        m.drop_path_rates = [0.0, 0.1]

    got = _step(m, x, y, between=change)
    assert m.drop_path_rates == [0.0, 0.1]
    assert torch.equal(got[0], want[0]) and all(torch.equal(got[2][k], want[2][k]) for k in want[2])


def test_train_main_drop_path_bf16(tmp_path, monkeypatch):
    """train.py --drop-path 0.1 --dtype bf16 --steps 3 on the device (FusedAdamW) ends with a finite loss."""
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    from VisionTransformer.optim import FusedAdamW
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    made = []
    real = T.make_optimizer
    monkeypatch.setattr(T, "make_optimizer", lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1])
    launches = []
    real_rows = _ops.drop_path_rows
    monkeypatch.setattr(_ops, "drop_path_rows", lambda *a, **k: (launches.append(a[1]), real_rows(*a, **k))[1])
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cuda", "--model", "tiny", "--img", "32", "--batch", "4",
                                      "--steps", "3", "--epochs", "0", "--train-size", "12", "--test-size", "4",
                                      "--workers", "0", "--dtype", "bf16", "--drop-path", "0.1", "--log-dir", logs,
                                      "--checkpoint-dir", ck])
    T.main()
    losses = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    losses = [r["value"] for r in losses if r["tag"] == "Loss/train_batch"]
    assert len(losses) == 3 and all(math.isfinite(v) and v > 0 for v in losses)
    assert made and all(isinstance(o, FusedAdamW) for o in made)
    L = config.PRESETS["tiny"][2]
    assert len(launches) == 3 and all(r == config.drop_path_rates(0.1, L) for r in launches)
