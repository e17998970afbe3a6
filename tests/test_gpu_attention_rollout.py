"""Attention rollout on the device (vit_attn_rollout_step, Engine.rollout, VisionTransformer.attention_rollout): the
step kernel in both forms against an fp64 evaluation of rollout.py's recurrence on probabilities formed in fp64 from
the kernel's own inputs, its tolerance-free properties and refusals, the model in fp32 (micro, tiny) against the
test's own matrix-product form over the oracle's fp64 probabilities, the model in bf16 (tiny) against the chain
recomputed from the qkv tensors the steps were given, patch_map, and train.py --eval-only --rollout-out.

Gates.  Kernel: max(4 * e32, T * 2^-24), e32 the error of the same formula evaluated by torch in fp32 from the same
inputs against fp64 (the factor covers the kernel's other summation order and its hardware exp2, both of torch's
fp32 error class; T * 2^-24 is the worst case of summing T terms of at most 1 in fp32).  fp32 model:
max(2 * the fp32 oracle's error against fp64, T * 2^-24).  bf16 model: max(4 * e32 of the fp32 torch chain from the
recorded inputs, L * T * 2^-24).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O
from VisionTransformer import _lib, _ops, config, rollout, vit

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FUSIONS = ("mean", "max", "min")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------
# the step kernel
# ---------------------------------------------------------------------------------------------------------------
def probs_of(qkv, B, T, H, hd, scale, dtype):
    """[B, H, T, T] softmax(scale q k^T) in `dtype` from qkv [B*T, 3*H*hd] (upcast exactly)."""
    z = qkv.to(dtype).view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    return torch.softmax((z[0] @ z[1].transpose(-2, -1)) * scale, dim=-1)


def make_inputs(B, T, H, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).to(dtype)
    rs = {"token0": torch.zeros(B, T), "cls": torch.zeros(B, T)}
    rs["token0"][:, 0] = 1
    rs["cls"][:, T - 1] = 1
    r = torch.rand(B, T, generator=g)
    r[torch.rand(B, T, generator=g) < 0.3] = 0          # some exact zeros
    r[:, 0] += 1e-3                                     # (never an all-zero row)
    rs["random"] = r / r.sum(-1, keepdim=True)
    return qkv, rs


SHAPES = [(1, 1, 1, 64), (3, 5, 4, 16), (2, 31, 2, 64), (2, 32, 2, 64), (2, 33, 2, 64), (2, 63, 3, 64),
          (2, 64, 3, 64), (2, 65, 3, 64), (2, 17, 3, 64), (2, 197, 12, 64), (1, 257, 2, 64), (1, 577, 2, 64),
          (2, 33, 2, 4), (2, 33, 2, 128)]
WORST = {}


def forms_of(hd, dtype):
    if dtype == torch.bfloat16 and hd == 64:      # both forms of the shape that has two
        return (_lib.ROLLOUT_FORM_AUTO, _lib.ROLLOUT_FORM_MFMA, _lib.ROLLOUT_FORM_VALU)
    return (_lib.ROLLOUT_FORM_AUTO,)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_T%d_H%d_hd%d" % s)
def test_step_against_fp64(shape, dtype):
    B, T, H, hd = shape
    qkv, rs = make_inputs(B, T, H, hd, dtype, seed=T * 131 + hd)
    qkv_d = qkv.to(DEV)
    floor = T * 2.0 ** -24
    worst = 0.0
    for scale in (hd ** -0.5, hd ** 0.5):               # soft rows; the reference's scale: saturated rows
        p64 = probs_of(qkv, B, T, H, hd, scale, torch.float64)
        p32 = probs_of(qkv, B, T, H, hd, scale, torch.float32)
        for fuse in FUSIONS:
            for name, r in rs.items():
                want = rollout.rollout_step(p64, r.double(), fuse)
                if name != "random":                    # a one-hot step is rollout_from_probs of one block
                    tok = 0 if name == "token0" else T - 1
                    assert torch.equal(want, rollout.rollout_from_probs([p64], tok, fuse))
                e32 = float((rollout.rollout_step(p32, r, fuse).double() - want).abs().max())
                gate = max(4 * e32, floor)
                for form in forms_of(hd, dtype):
                    got = _ops.attn_rollout_step(qkv_d, r.to(DEV), B, T, H, hd, scale, _ops.ROLLOUT_FUSE[fuse],
                                                 form=form).cpu().double()
                    err = float((got - want).abs().max())
                    worst = max(worst, err / gate)
                    assert err <= gate, (shape, dtype, scale, fuse, name, form, err, e32, gate)
                    # the chain keeps the mass: sum_j r_out = sum_i r_in
                    assert float((got.sum(-1) - r.double().sum(-1)).abs().max()) <= gate, (shape, fuse, name, form)
    WORST[(shape, dtype)] = worst
    print(f"rollout step {shape} {dtype}: worst error / gate = {worst:.3f}")


def test_worst_ratio_report():
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f"rollout step: worst error / gate over {len(WORST)} cases = {WORST[k]:.3f} at {k}")
        assert WORST[k] <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_one_token_is_the_identity(dtype):
    """T == 1: P = 1, F = 1, w = r / 2, r_out = w + w = r, bit for bit, in every form and fusing."""
    for H, hd in ((1, 64), (3, 64), (2, 16)):
        qkv = torch.randn(4, 3 * H * hd).to(dtype).to(DEV)
        r = torch.tensor([[1.0], [0.3], [0.0], [1e-30]], device=DEV)
        for fuse in FUSIONS:
            for form in forms_of(hd, dtype):
                got = _ops.attn_rollout_step(qkv, r, 4, 1, H, hd, hd ** 0.5, _ops.ROLLOUT_FUSE[fuse], form=form)
                assert torch.equal(got, r), (H, hd, fuse, form)


def guarded(t, pad, align=1):
    """A copy of t between two NaN-filled guards of `pad` elements (rounded up to `align`): (whole buffer, view)."""
    pad = (pad + align - 1) // align * align
    whole = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV).to(t.dtype)
    whole[pad:pad + t.numel()] = t.reshape(-1).to(DEV)
    return whole, whole[pad:pad + t.numel()].view(t.shape)


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, (3, 70, 3, 64)), (torch.float32, (3, 70, 3, 16)),
                                         (torch.bfloat16, (2, 300, 2, 64))], ids=["mfma", "valu", "mfma_T300"])
def test_repeatable_guards_and_isolation(dtype, shape):
    """Two runs give equal bits; nothing outside r_out and the workspace's bytes is written and the inputs are left
    as they were; a NaN in image 0's qkv leaves the other images' outputs bitwise as they were."""
    B, T, H, hd = shape
    qkv, rs = make_inputs(B, T, H, hd, dtype, seed=5)
    r = rs["random"]
    scale = hd ** -0.5
    pad = 4096
    for fuse in FUSIONS:
        code = _ops.ROLLOUT_FUSE[fuse]
        qkv_w, qkv_v = guarded(qkv, pad, 8)                       # (16-B aligned views)
        rin_w, rin_v = guarded(r, pad, 4)
        out_w, out_v = guarded(torch.full((B, T), float("nan")), pad, 4)
        need = _ops.attn_rollout_workspace_bytes(B, T, H, hd, dtype, code)
        assert need > 0 and need % 4 == 0
        ws_w, ws_v = guarded(torch.full((need // 4,), float("nan")), pad, 4)
        before = [t.clone() for t in (qkv_w, rin_w)]
        got = _ops.attn_rollout_step(qkv_v, rin_v, B, T, H, hd, scale, code, r_out=out_v, workspace=ws_v)
        assert got.data_ptr() == out_v.data_ptr() and not torch.isnan(out_v).any()
        n = B * T
        p = out_w.numel() - n
        assert torch.isnan(out_w[:p // 2]).all() and torch.isnan(out_w[p // 2 + n:]).all()
        p = ws_w.numel() - need // 4
        assert torch.isnan(ws_w[:p // 2]).all() and torch.isnan(ws_w[p // 2 + need // 4:]).all()
        for a, b in zip(before, (qkv_w, rin_w)):                  # inputs and their guards: bitwise unchanged
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        again = _ops.attn_rollout_step(qkv_v, rin_v, B, T, H, hd, scale, code)
        assert torch.equal(again, out_v)
        bad = qkv.clone()
        bad.view(B, T, -1)[0, T // 2, 5] = float("nan")
        bad.view(B, T, -1)[0, 0, 3 * H * hd - 1] = float("nan")  # (V is not read; K and Q are)
        bad.view(B, T, -1)[0, 1, H * hd] = float("inf")
        poisoned = _ops.attn_rollout_step(bad.to(DEV), rin_v, B, T, H, hd, scale, code)
        assert torch.equal(poisoned[1:], out_v[1:])


def test_refusals():
    """VIT_ERR_INVALID through VIT_REQUIRE before any launch, with a message naming the entry point; r_out is not
    written."""
    lib = _lib.load()
    B, T, H, hd = 2, 9, 2, 64
    qkv = torch.randn(B * T, 3 * H * hd, device=DEV).bfloat16()
    r_in = torch.full((B, T), 1.0 / T, device=DEV)
    r_out = torch.full((B, T), float("nan"), device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.float32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    s = _ops._stream()

    def call(qkv_p=P(qkv), rin_p=P(r_in), rout_p=P(r_out), B=B, T=T, H=H, hd=hd, dtype=_lib.BF16, fuse=0, ws_p=P(ws)):
        rc = lib.vit_attn_rollout_step(qkv_p, rin_p, rout_p, B, T, H, hd, 1.0, dtype, fuse, ws_p, s)
        msg = lib.vit_last_error().decode()
        return rc == 1 and "vit_attn_rollout_step" in msg

    assert call(hd=0) and call(hd=132) and call(hd=66) and call(hd=256)        # hd out of range
    assert call(hd=132, dtype=_lib.F32) and call(hd=6, dtype=_lib.F32)
    assert call(T=1025) and call(T=0) and call(T=1 << 20)                      # T beyond the limit
    assert call(fuse=3) and call(fuse=-1)                                      # fuse out of range
    assert call(dtype=2) and call(dtype=-1)
    assert call(B=0) and call(H=0)
    assert call(rout_p=P(r_in))                                                # r_in == r_out
    assert call(rout_p=ctypes.c_void_p(r_in.data_ptr() + 4 * T))               # ... or overlapping
    assert call(qkv_p=None) and call(rin_p=None) and call(rout_p=None) and call(ws_p=None)
    form = lambda f, **kw: lib.vit_attn_rollout_step_form(                     # noqa: E731
        P(qkv), P(r_in), P(r_out), B, T, H, kw.get("hd", hd), 1.0, kw.get("dtype", _lib.BF16), 0, f, P(ws), s) == 1
    assert form(3) and form(-1) and form(2, hd=32) and form(2, dtype=_lib.F32)
    assert lib.vit_attn_rollout_workspace_bytes(B, 1025, H, hd, _lib.BF16, 0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(r_out).all()
    with pytest.raises(ValueError):
        _ops.attn_rollout_step(qkv, r_in, B, T, H, hd, 1.0, 0, workspace=ws[:4])
    assert lib.vit_attn_rollout_step(P(qkv), P(r_in), P(r_out), B, T, H, hd, 1.0, _lib.BF16, 0, P(ws), s) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(r_out).any()


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def matrix_rollout(probs, token, fuse):
    """The definition as a matrix product, written independently of rollout.py: A_l = rows-normalised (F_l + I),
    R = A_L ... A_1, row `token`.  In the dtype of `probs`."""
    R = None
    for p in probs:                                              # first block to last: R <- A_l R
        F = {"mean": lambda t: t.sum(1) / t.shape[1], "max": lambda t: t.max(1).values,
             "min": lambda t: t.min(1).values}[fuse](p)
        A = F + torch.eye(F.shape[-1], dtype=F.dtype)
        A = A / A.sum(-1, keepdim=True)
        R = A if R is None else A @ R
    return R[:, token, :]


def build(ocfg, dtype):
    c = config.ViTConfig(3, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size, ocfg.patch_size, ocfg.num_heads,
                         ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)
    return vit.VisionTransformer(c)


@pytest.fixture(scope="module")
def oracle_cases():
    """micro (D 64, H 4, L 2, 32^2, B 4: hd 16, the VALU form) and tiny (64^2, B 8, L 12, T 17, hd 64): state, batch,
    the oracle's probabilities in fp64 and fp32.  Computed once, never modified."""
    out = {}
    for name, ocfg in (("micro", O.make_config("micro", img=32, batch=4)),
                       ("tiny", O.make_config("tiny", img=64, batch=8))):
        torch.manual_seed(0)
        st = O.init_state(ocfg, seed=0)
        x, _ = O.synthetic_batch(ocfg)
        _, p64 = O.forward(st, x, ocfg, keep_probs=True, dtype=torch.float64)
        _, p32 = O.forward(st, x, ocfg, keep_probs=True, dtype=torch.float32)
        out[name] = (ocfg, st, x, p64, p32)
    return out


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_model_fp32_against_the_oracle(name, oracle_cases):
    ocfg, st, x, p64, p32 = oracle_cases[name]
    T = ocfg.T
    m = build(ocfg, torch.float32)
    m.load_state_dict(st)
    m = m.to(DEV).train()                                        # (training mode: the call runs eval-mode anyway)
    gold = np.load(os.path.join(GOLDEN, "rollout_micro.npz")) if name == "micro" else None
    worst = 0.0
    for fuse in FUSIONS:
        for token in (0, T - 1):
            want = matrix_rollout(p64, token, fuse)
            e32 = float((matrix_rollout(p32, token, fuse).double() - want).abs().max())
            gate = max(2 * e32, T * 2.0 ** -24)
            logits, maps = m.attention_rollout(x.to(DEV), token=token, head_fusion=fuse)
            assert maps.dtype == torch.float32 and maps.shape == (ocfg.batch_size, T)
            err = float((maps.cpu().double() - want).abs().max())
            worst = max(worst, err / gate)
            assert err <= gate, (name, fuse, token, err, e32, gate)
            if gold is not None:
                g = torch.from_numpy(gold[f"{fuse}_{token}"])
                ggate = max(2 * float(gold[f"err32_{fuse}_{token}"]), T * 2.0 ** -24)
                assert float((maps.cpu().double() - g).abs().max()) <= ggate, (fuse, token)
    assert m.training and m.store_attention_probs is None
    print(f"rollout fp32 model {name}: worst error / gate = {worst:.3f}")


def test_model_bf16_tiny(oracle_cases, monkeypatch):
    ocfg, st, x, _, _ = oracle_cases["tiny"]
    T, L, H, hd = ocfg.T, ocfg.num_blocks, ocfg.num_heads, ocfg.hd
    B = ocfg.batch_size
    m = build(ocfg, torch.bfloat16)
    m.load_state_dict(st)
    m = m.to(DEV).train()
    calls, kept = [], []
    step, fwd = _ops.attn_rollout_step, m.hip_engine.forward

    def rec_step(qkv, r_in, *a, **kw):
        calls.append(qkv)
        return step(qkv, r_in, *a, **kw)

    def rec_fwd(*a, **kw):
        out = fwd(*a, **kw)
        kept.append(out[2])
        return out

    monkeypatch.setattr(_ops, "attn_rollout_step", rec_step)
    monkeypatch.setattr(m.hip_engine, "forward", rec_fwd)
    xd = x.to(DEV)
    worst = 0.0
    for fuse in FUSIONS:
        for token in (0, T - 1):
            del calls[:], kept[:]
            logits, maps, layers = m.attention_rollout(xd, token=token, head_fusion=fuse, return_layers=True)
            assert len(calls) == L and len(kept) == 1 and len(kept[0]) == L
            for i, q in enumerate(calls):                         # last block first
                assert q.data_ptr() == kept[0][L - 1 - i].data_ptr() and q.dtype == torch.bfloat16
            assert layers.shape == (L, B, T) and torch.equal(layers[0], maps)
            qk = [q.cpu() for q in kept[0]]
            p64 = [probs_of(q, B, T, H, hd, hd ** 0.5, torch.float64) for q in qk]
            p32 = [probs_of(q, B, T, H, hd, hd ** 0.5, torch.float32) for q in qk]
            want, wl = rollout.rollout_from_probs(p64, token, fuse, return_layers=True)
            e32 = float((rollout.rollout_from_probs(p32, token, fuse).double() - want).abs().max())
            gate = max(4 * e32, L * T * 2.0 ** -24)
            err = float((maps.cpu().double() - want).abs().max())
            worst = max(worst, err / gate)
            assert err <= gate, (fuse, token, err, e32, gate)
            assert float((layers.cpu().double() - wl).abs().max()) <= gate
    assert m.training and m.store_attention_probs is None
    monkeypatch.undo()
    m.store_attention_probs = True
    m.eval()
    with torch.no_grad():
        stored = m(xd)
    assert torch.equal(stored, logits)                           # bitwise the probability-storing forward's logits
    assert m.transformer_encoder.blocks[0].multi_head.attention_probs is not None
    # fast_attention: the plain forward's attention kernel (other bits in bf16); every step still keeps the mass
    m.store_attention_probs = None
    l_fast, maps_fast, layers_fast = m.attention_rollout(xd, token=T - 1, head_fusion="min", return_layers=True,
                                                         fast_attention=True)
    assert torch.isfinite(l_fast).all() and not torch.equal(l_fast, logits)
    assert float((maps_fast.sum(-1) - 1).abs().max()) <= L * T * 2.0 ** -24
    assert all(b.multi_head.attention_probs is None for b in m.transformer_encoder.blocks)
    print(f"rollout bf16 tiny: worst error / gate = {worst:.3f}")


def test_bad_arguments_on_the_device(oracle_cases):
    ocfg, st, x, _, _ = oracle_cases["micro"]
    m = build(ocfg, torch.float32).to(DEV)
    for kw in ({"token": ocfg.T}, {"token": -1}, {"token": 0.5}, {"head_fusion": "median"}):
        with pytest.raises(ValueError):
            m.attention_rollout(x.to(DEV), **kw)


def test_patch_map_on_a_non_square_input():
    """32 x 64 at patch 16: 2 x 4 patches, row-major; the CLS entry (index N = 8) is dropped."""
    c = config.ViTConfig(3, 10, 8, 64, 16, 4, 1, "cpu", 2)
    m = vit.VisionTransformer(c)
    maps = torch.arange(18, dtype=torch.float32).view(2, 9)
    pm = m.patch_map(maps, (32, 64))
    assert pm.shape == (2, 2, 4)
    assert torch.equal(pm[0], torch.tensor([[0., 1, 2, 3], [4, 5, 6, 7]])) and pm[1, 1, 3] == 16
    with pytest.raises(ValueError):
        m.patch_map(maps, (64, 64))
    md = m.to(DEV)
    x = torch.randn(2, 3, 32, 64, device=DEV)
    logits, mp = md.attention_rollout(x)
    assert md.patch_map(mp, x.shape[2:]).shape == (2, 2, 4)


def test_train_eval_only_rollout_out(tmp_path, monkeypatch, capsys):
    """train.py --eval-only --rollout-out on the tiny 32^2 preset: the three arrays with their shapes, K cut from whole
    batches, and maps equal to model.attention_rollout on the same batch."""
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    cfg = config.ViTConfig(3, 10, 4, 192, 16, 3, 12, "cpu", 4)
    torch.manual_seed(3)
    model = vit.VisionTransformer(cfg)
    ck = tmp_path / "ck"
    ck.mkdir()
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, ck / "0.pt")
    out = str(tmp_path / "maps.npz")
    monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cuda", "--model", "tiny", "--img", "32", "--batch", "4",
                                      "--test-size", "7", "--workers", "0", "--eval-only", "--checkpoint-dir", str(ck),
                                      "--rollout-out", out, "--rollout-images", "6", "--rollout-fusion", "max",
                                      "--rollout-token", "4"])
    T.main()
    assert '"top1"' in capsys.readouterr().out
    z = np.load(out)
    assert z["maps"].shape == (6, 2, 2) and z["maps"].dtype == np.float32
    assert z["pred"].shape == (6,) and z["label"].shape == (6,)
    ts = T.SyntheticImages(7, 3, 32, 10, seed=10_000)
    x, y = next(iter(torch.utils.data.DataLoader(ts, batch_size=4)))
    model = model.to(DEV)
    logits, maps = model.attention_rollout(x.to(DEV), token=4, head_fusion="max")
    assert np.array_equal(z["maps"][:4], model.patch_map(maps, (32, 32)).cpu().numpy())
    assert np.array_equal(z["pred"][:4], logits.argmax(-1).cpu().numpy())
    assert np.array_equal(z["label"][:4], y.numpy())
