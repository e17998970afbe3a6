"""Model-level parity on the MI355X: the drop-in VisionTransformer (fused HIP engine, through the C-ABI) against the
oracle (CPU restatement pinned to the reference) and the reference's own goldens.

Tolerances: fp32 1e-4 per op/block and end-to-end at depth <= 2; bf16 1e-2 against
an oracle that rounds to bf16 at the same storage points; at full depth fp32 is gated at the reference's own
fp32-vs-fp64 error scale because the x sqrt(hd) logit scaling saturates the softmax."""
import os

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _lib, _ops, config, transformer, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy

DEV = "cuda"


def _model(ocfg, seed=0, dtype=torch.float32):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)
    torch.manual_seed(seed)
    m = vit.VisionTransformer(c)
    return m.to(DEV)


def _grads(m):
    return {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(b.double().norm(), 1e-30))


def test_micro_fp32_vs_reference_goldens(golden_dir):
    """G1: eval-mode logits / loss / every gradient of the reference micro model (hd=16: generic attention)."""
    g = np.load(os.path.join(golden_dir, "micro.npz"))
    ocfg = O.make_config("micro", img=32, batch=4)
    m = _model(ocfg).eval()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits"], atol=1e-4, rtol=0)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    for k, p in m.named_parameters():
        ref = torch.from_numpy(g["grad/" + k])
        err = (p.grad.cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)


@pytest.mark.parametrize("train", [False, True])
def test_hd64_fp32_vs_oracle(train):
    """D=128, H=2 (hd=64), L=2, 64x64 images: fp32 path incl. counter-hash dropout in train mode."""
    ocfg = O.make_config("micro", img=64, batch=3, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    st = O.init_state(ocfg, seed=1)
    m = _model(ocfg)
    m.load_state_dict(st)
    m.train(train)
    x, y = O.synthetic_batch(ocfg)
    torch.manual_seed(42)
    base_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(42)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    loss.backward()
    lg_ref, loss_ref, g_ref = O.loss_and_grads(st, x, y, ocfg, train=train, seed=base_seed)
    assert (logits.detach().cpu() - lg_ref).abs().max().item() < 1e-4
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    for k, p in m.named_parameters():
        err = (p.grad.cpu() - g_ref[k]).abs().max().item()
        assert err <= 2e-4 * max(1.0, g_ref[k].abs().max().item()), (k, err)


@pytest.mark.parametrize("hd_heads", [(64, 2), (16, 4)])
def test_bf16_vs_oracle_same_rounding(hd_heads):
    """bf16 compute (MFMA GEMM + MFMA attention when hd=64).  Gate: logits within 1e-2 (norm-wise) of the oracle
    that rounds to bf16 at the same storage points; every gradient's error against the fp32 oracle no worse than
    max(1e-2, 2x) the bf16-emulating oracle's own error (K-projection gradients under the saturated x sqrt(hd)
    softmax are small differences of near-equal terms, so bf16 alone costs them ~10-20%)."""
    hd, H = hd_heads
    ocfg = O.make_config("micro", img=64, batch=4, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = hd * H, H
    st = O.init_state(ocfg, seed=2)
    m = _model(ocfg, dtype=torch.bfloat16)
    m.load_state_dict(st)
    m.eval()
    x, y = O.synthetic_batch(ocfg)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    loss.backward()
    lg_bf, _, g_bf = O.loss_and_grads(st, x, y, ocfg, bf16=True)
    lg_32, _, g_32 = O.loss_and_grads(st, x, y, ocfg)
    assert _rel(logits.detach().cpu(), lg_bf) < 1e-2
    worst = []
    for k, p in m.named_parameters():
        ours, ora = _rel(p.grad.cpu(), g_32[k]), _rel(g_bf[k], g_32[k])
        worst.append((ours / max(ora, 1e-9), k, ours, ora))
        assert ours <= max(1e-2, 2 * ora), (k, ours, ora)
    print("bf16 worst grad error ratios:", sorted(worst)[-3:])


def _tiny_c1_logits_and_grads(golden_dir, store_probs):
    """Logits and every gradient of the C1 model against the reference's goldens; `store_probs` sets
    model.store_attention_probs (None: left as it is)."""
    g = np.load(os.path.join(golden_dir, "tiny.npz"))
    ocfg = O.make_config("tiny", img=64, batch=8)
    m = _model(ocfg).eval()
    if store_probs is not None:
        m.store_attention_probs = store_probs
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)
    logits = m(x)
    ref64 = torch.from_numpy(g["logits64"])
    ref32 = torch.from_numpy(g["logits"])
    ref_err = (ref32.double() - ref64).abs().max().item()
    our_err = (logits.detach().cpu().double() - ref64).abs().max().item()
    assert our_err <= max(1e-4, 2 * ref_err), (our_err, ref_err)
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    # Tolerance scale per tensor: the larger of two valid fp32 evaluations' error vs fp64 — the reference's own
    # (MKL blocked sums) and the oracle with sequential-chain GEMM accumulation (this path's summation order).  At
    # depth 12 the saturated softmax amplifies summation-order rounding in lower-block gradients to ~1e-2.
    g_seq = _tiny_seq_chain_grads(ocfg, x, y)
    # Each scale is a single sample of chaotic rounding amplification, so the per-tensor gate is 8x (measured worst
    # 4.67x, blocks.5.ln2.weight, round 6), and the whole gradient vector (all tensors' slices concatenated) must be
    # within 2x of the sequential-order sample.
    params = dict(m.named_parameters())
    cat = {"ours": [], "seq": [], "r64": []}
    ratios = []
    for k in params:
        ours = params[k].grad.cpu().reshape(-1)[::97].double().numpy()
        r32, r64 = g["gslice/" + k].astype(np.float64), g["gslice64/" + k]
        rsq = g_seq[k].reshape(-1)[::97].double().numpy()
        n64 = max(np.linalg.norm(r64), 1e-30)
        e_ours = np.linalg.norm(ours - r64) / n64
        e_ref = max(np.linalg.norm(r32 - r64), np.linalg.norm(rsq - r64)) / n64
        ratios.append((e_ours / max(e_ref, 1e-12), k))
        assert e_ours <= max(2e-4, 8 * e_ref), (k, e_ours, e_ref)
        for n_, v_ in (("ours", ours), ("seq", rsq), ("r64", r64)):
            cat[n_].append(v_)
    print("ViT-Tiny fp32 worst gradient error ratios (ours / valid-order error):", sorted(ratios)[-4:])
    o, sq, r = (np.concatenate(cat[n_]) for n_ in ("ours", "seq", "r64"))
    assert np.linalg.norm(o - r) <= max(1e-5 * np.linalg.norm(r), 2 * np.linalg.norm(sq - r))
    if store_probs:
        assert all(b.multi_head.attention_probs is not None for b in m.transformer_encoder.blocks)
    return x, y, ocfg, g


_TINY_SEQ = {}


def _tiny_seq_chain_grads(ocfg, x, y):
    """The oracle's gradients with sequential-chain GEMM accumulation (CPU, computed once for the C1 tests)."""
    if "g" not in _TINY_SEQ:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _TINY_SEQ["g"] = O.loss_and_grads(O.init_state(ocfg, 0), x.cpu(), y.cpu(), ocfg, seq_chain=True)[2]
    return _TINY_SEQ["g"]


def test_tiny_c1_fp32_vs_reference(golden_dir):
    """G4: BASELINE config 1 dims (ViT-Tiny/16, 64^2, B8) on the GPU.  Full depth (12 blocks) under the saturating
    x sqrt(hd) softmax, so the gates are the reference's own fp32-vs-fp64 error scale: logits and
    every gradient (strided slices) vs the reference's fp64 run within max(floor, 4x the reference fp32 error)."""
    x, y, ocfg, g = _tiny_c1_logits_and_grads(golden_dir, None)
    # 3-step AdamW trace: step 1 is the same loss; later steps are AdamW-chaotic (first updates ~ lr*sign(g)),
    # the reference's own fp32 and fp64 traces already differ by 2.8e-3 at step 3.
    m2 = _model(ocfg).eval()
    opt = FusedAdamW(m2.parameters(), lr=1e-4, weight_decay=1e-4)
    trace = []
    for _ in range(3):
        lg = m2(x)
        ls = cross_entropy(lg, y)
        opt.zero_grad(set_to_none=True)
        ls.backward()
        opt.step()
        trace.append(ls.item())
    assert abs(trace[0] - g["trace64"][0]) < 2e-5
    np.testing.assert_allclose(trace, g["trace64"], rtol=2e-2)
    assert trace[2] < trace[1] < trace[0]


def test_tiny_c1_fp32_storing_attention_probs_vs_reference(golden_dir):
    """The same C1 golden comparison with store_attention_probs=True — the forward a small training batch runs by
    default (store_attention_probs=None under the shipped budget): every block's attention goes through the
    probability-storing generic kernel, and the backward starts from its o and lse."""
    _tiny_c1_logits_and_grads(golden_dir, True)


def _tiny_c1_bf16_probs_run(blocks):
    """C1 dims in bf16 (D = 192, 3 heads of hd = 64, 64^2 images, batch 8) with store_attention_probs=True, eval mode:
    (config, state, batch, logits, gradients)."""
    ocfg = O.make_config("tiny", img=64, batch=8, blocks=blocks)
    st = O.init_state(ocfg, seed=2)
    m = _model(ocfg, dtype=torch.bfloat16)
    m.load_state_dict(st)
    m.eval()
    m.store_attention_probs = True
    x, y = O.synthetic_batch(ocfg)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    loss.backward()
    assert all(b.multi_head.attention_probs is not None for b in m.transformer_encoder.blocks)
    return ocfg, st, x, y, logits.detach().cpu(), _grads(m)


def test_tiny_c1_bf16_storing_attention_probs_vs_oracle():
    """C1 dims in bf16 with store_attention_probs=True, the default forward of a small training batch: the generic
    VALU attention forward hands its o and lse to the fused MFMA backward.  Two blocks, the depth of
    test_bf16_vs_oracle_same_rounding, and its gates: logits within 1e-2 (norm-wise) of the bf16-rounding oracle,
    every gradient's error against the fp32 oracle at most max(1e-2, 2x) that oracle's own.  (At 12 blocks a single
    bf16 oracle is no reference: see the full-depth test below.)"""
    ocfg, st, x, y, logits, ours = _tiny_c1_bf16_probs_run(2)
    lg_bf, _, g_bf = O.loss_and_grads(st, x, y, ocfg, bf16=True)
    _, _, g_32 = O.loss_and_grads(st, x, y, ocfg)
    assert _rel(logits, lg_bf) < 1e-2
    worst = []
    for k, g in ours.items():
        e, ora = _rel(g, g_32[k]), _rel(g_bf[k], g_32[k])
        worst.append((e / max(ora, 1e-9), k, e, ora))
        assert e <= max(1e-2, 2 * ora), (k, e, ora)
    print("bf16 C1 width, 2 blocks, probs stored: worst grad error ratios:", sorted(worst)[-3:])


def test_tiny_c1_bf16_full_depth_storing_attention_probs_vs_valid_oracles():
    """The same at C1's own depth (12 blocks).  Under the saturating x sqrt(hd) softmax, 12 blocks of bf16 rounding
    are chaotic: the oracle's own valid bf16 evaluations (fp32 arithmetic between the storage points, fp64 arithmetic,
    the flash kernels' roundings) lie 5.0e-2 and 1.1e-1 (norm-wise, logits) from each other, and 78-85% from the fp32
    oracle in the lower blocks' query / key gradients, so no evaluation is within 1e-2 of a single one of them
    (measured: this path 6.8e-2, the MFMA forward without probabilities 1.06e-1).  The reference is therefore the set
    of valid evaluations, as in test_gpu_dropin.py::test_base_width_bf16_engine_vs_oracle, with that test's gradient
    gates (per tensor, query / key projections per block, and the whole vector: error vs the fp32 oracle <=
    max(1e-2, 2 x the largest valid error)); logits within max(1e-2, 2 x the largest distance between two valid
    evaluations) of the bf16 oracle."""
    ocfg, st, x, y, logits, ours = _tiny_c1_bf16_probs_run(12)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lg_bf, _, g_bf = O.loss_and_grads(st, x, y, ocfg, bf16=True)
    _, _, g_32 = O.loss_and_grads(st, x, y, ocfg)
    lg_64, _, g_64 = O.loss_and_grads(st, x, y, ocfg, bf16=True, dtype=torch.float64)
    lg_fl, _, g_fl = O.loss_and_grads(st, x, y, ocfg, bf16=True, flash=True)
    valid = [g_bf, g_64, g_fl]
    spread = max(_rel(lg_64, lg_bf), _rel(lg_fl, lg_bf), _rel(lg_fl, lg_64))
    e_lg = _rel(logits, lg_bf)
    print(f"bf16 C1 full depth, probs stored: logits {e_lg:.2e} from the bf16 oracle, valid spread {spread:.2e}")
    assert e_lg <= max(1e-2, 2 * spread), (e_lg, spread)

    def err(g, keys):
        a = torch.cat([g[k].reshape(-1).double() for k in keys])
        r = torch.cat([g_32[k].reshape(-1).double() for k in keys])
        return float((a - r).norm() / r.norm())

    groups = {}
    for k in g_32:
        if ".query." in k or ".key." in k:
            groups.setdefault(k.split(".multi_head")[0] + " q/k (all heads)", []).append(k)
        else:
            groups[k] = [k]
    groups["ALL"] = list(g_32)
    bad, worst = [], []
    for name, keys in groups.items():
        e_ours = err(ours, keys)
        e_ora = max(err(v, keys) for v in valid)
        worst.append((e_ours / max(e_ora, 1e-9), name, e_ours, e_ora))
        if e_ours > max(1e-2, 2 * e_ora):
            bad.append((name, e_ours, e_ora))
    print("bf16 C1 full depth, probs stored: worst error ratios:", sorted(worst)[-4:])
    assert not bad, bad


def test_fused_adamw_matches_torch_adamw_on_model():
    """Same gradients fed to FusedAdamW (model params) and torch.optim.AdamW (a synced copy) for 4 steps."""
    ocfg = O.make_config("micro", img=32, batch=4)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)
    m = _model(ocfg, seed=5).eval()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    shadow = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    ref = torch.optim.AdamW(shadow, lr=1e-3, weight_decay=1e-4)
    for _ in range(4):
        ls = cross_entropy(m(x), y)
        opt.zero_grad(set_to_none=True)
        ls.backward()
        for s_, p in zip(shadow, m.parameters()):
            s_.grad = p.grad.clone()
            with torch.no_grad():
                s_.copy_(p)
        opt.step()
        ref.step()
        for s_, p in zip(shadow, m.parameters()):
            assert (s_.detach() - p.detach()).abs().max().item() < 1e-6
    sd = opt.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    # checkpoint interchange: torch AdamW loads the fused optimizer's state
    ref2 = torch.optim.AdamW(shadow, lr=1e-3, weight_decay=1e-4)
    ref2.load_state_dict(sd)


def test_module_level_api_block_and_head(golden_dir):
    """Standalone module forwards (Head / Block / FeedForward) run HIP kernels and match the reference KATs."""
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    head = transformer.Head(16, 64, 5).to(DEV)
    with torch.no_grad():
        head.query.weight.copy_(t("head/wq"))
        head.key.weight.copy_(t("head/wk"))
        head.value.weight.copy_(t("head/wv"))
    xh = t("head/x").requires_grad_(True)
    out, wei = head(xh)
    assert (out.detach() - t("head/out")).abs().max().item() < 1e-5
    assert (wei - t("head/wei")).abs().max().item() < 1e-6
    out.backward(t("head/gout"))
    assert (xh.grad - t("head/dx")).abs().max().item() < 1e-4
    ff = transformer.FeedForward(32).to(DEV).eval()
    with torch.no_grad():
        ff.mlp[0].weight.copy_(t("ffn/w1"))
        ff.mlp[0].bias.copy_(t("ffn/b1"))
        ff.mlp[2].weight.copy_(t("ffn/w2"))
        ff.mlp[2].bias.copy_(t("ffn/b2"))
    assert (ff(t("ffn/x")).detach() - t("ffn/y")).abs().max().item() < 1e-5


def test_block_base_width_module_path(golden_dir):
    """G2: one ViT-B-width Block (D768 H12 T197 B2) through the module-level HIP path vs the reference."""
    g = np.load(os.path.join(golden_dir, "block_base.npz"))
    torch.manual_seed(11)
    blk = transformer.Block(768, 12, 197).eval()
    blk = blk.to(DEV)
    xb = torch.randn(2, 197, 768, generator=torch.Generator().manual_seed(12), dtype=torch.float64).float()
    xb = xb.to(DEV).requires_grad_(True)
    yb = blk(xb)
    gy = torch.randn(2, 197, 768, generator=torch.Generator().manual_seed(13), dtype=torch.float64).float().to(DEV)
    yb.backward(gy)
    ys = yb.detach().double().cpu().reshape(-1)[::101].numpy()
    dxs = xb.grad.double().cpu().reshape(-1)[::101].numpy()
    np.testing.assert_allclose(ys, g["f64/y_slice"], atol=1e-4 * max(1.0, np.abs(g["f64/y_slice"]).max()))
    scale = np.abs(g["f64/dx_slice"]).max()
    np.testing.assert_allclose(dxs, g["f64/dx_slice"], atol=1e-4 * max(1.0, scale))


def test_vit_base_224_bf16_full_size_properties():
    """BASELINE config 2 at full size (ViT-B/16, 224^2, B=256, bf16): finite loss, deterministic (bitwise) gradients
    across two identical steps, loss decreases over 3 FusedAdamW steps on a fixed batch."""
    c = config.ViTConfig.preset("base", batch_size=256, precision=torch.bfloat16, device="cpu")
    torch.manual_seed(0)
    m = vit.VisionTransformer(c).to(DEV).eval()
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(256, 3, 224, 224, generator=gen).to(DEV)
    y = torch.randint(0, 1000, (256,), generator=torch.Generator().manual_seed(1235)).to(DEV)
    gs = []
    for _ in range(2):
        loss = cross_entropy(m(x), y)
        for p in m.parameters():
            p.grad = None
        loss.backward()
        gs.append(m.hip_engine.G.clone())
        assert torch.isfinite(loss).item()
    assert torch.equal(gs[0], gs[1])
    assert torch.isfinite(gs[0]).all().item()
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    losses = []
    for _ in range(3):
        loss = cross_entropy(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[2] < losses[0], losses


@pytest.mark.parametrize("dtype,train", [(torch.float32, True), (torch.float32, False), (torch.bfloat16, True)])
def test_pruned_last_block_matches_all_rows(dtype, train):
    """The last block's proj / LN2 / MLP on the B token-0 rows only (engine.prune_last, default), with its attention
    on query 0 alone (engine.row0_attention, default) or through the full attention kernels, == all B*T rows
    (prune_last = False): the classifier reads token 0 only (vit.py:80).  Same dropout bits (drawn at the full
    tensor's indices).  ViT-B width, 2 blocks; fp32 to summation-order rounding, bf16 to a few storage roundings."""
    ocfg = O.make_config("micro", img=64, batch=8, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 768, 12
    st = O.init_state(ocfg, seed=5)
    x, y = O.synthetic_batch(ocfg)
    out = []
    for prune, row0 in ((True, True), (True, False), (False, True)):       # row0: query-0 attention kernels
        m = _model(ocfg, dtype=dtype)
        m.hip_engine.prune_last = prune
        m.hip_engine.row0_attention = row0
        m.load_state_dict(st)
        m.train(train)
        torch.manual_seed(11)
        logits = m(x.to(DEV))
        loss = cross_entropy(logits, y.to(DEV))
        loss.backward()
        out.append((logits.detach().cpu(), loss.item(), _grads(m)))
    tol = 1e-4 if dtype == torch.float32 else 2e-2       # Q/K weight gradients amplify summation-order rounding
    for i, a in enumerate(out[:2]):
        errs = sorted((_rel(a[2][k], out[2][2][k]), k) for k in out[2][2])
        print(f"variant {i}: logits {_rel(a[0], out[2][0]):.2e}, worst gradients {errs[-3:]}")
        assert _rel(a[0], out[2][0]) < tol
        assert abs(a[1] - out[2][1]) < tol * max(1.0, abs(out[2][1]))
        assert errs[-1][0] < tol, errs[-1]


@pytest.mark.parametrize("first", [True, False], ids=["row0_fwd", "full_fwd"])
def test_row0_mode_recorded_on_tape(first):
    """The backward of the pruned block runs the attention backward matching the forward it saved (Tape.row0), even
    when engine.row0_attention is flipped between the two (the full backward would read o / lse rows the
    query-0 forward never wrote): bitwise equal to the unflipped run."""
    ocfg = O.make_config("micro", img=64, batch=8, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 256, 4
    st = O.init_state(ocfg, seed=5)
    x, y = O.synthetic_batch(ocfg)
    gs = []
    for flip in (False, True):
        m = _model(ocfg, dtype=torch.bfloat16)
        m.load_state_dict(st)
        m.train()
        m.hip_engine.row0_attention = first
        torch.manual_seed(3)
        loss = cross_entropy(m(x.to(DEV)), y.to(DEV))
        if flip:
            m.hip_engine.row0_attention = not first
        loss.backward()
        torch.cuda.synchronize()
        gs.append(m.hip_engine.G.clone())
    assert torch.isfinite(gs[0]).all()
    assert torch.equal(gs[0], gs[1])


def test_side_stream_weight_gradients_bitwise_equal():
    """Weight gradients on the side stream (engine.concurrent_wgrad) equal the in-order schedule bit for bit."""
    ocfg = O.make_config("micro", img=64, batch=4, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    st = O.init_state(ocfg, seed=4)
    x, y = O.synthetic_batch(ocfg)
    gs = []
    for conc in (True, False):
        m = _model(ocfg, dtype=torch.bfloat16)
        m.load_state_dict(st)
        m.train()
        m.hip_engine.concurrent_wgrad = conc
        torch.manual_seed(7)
        loss = cross_entropy(m(x.to(DEV)), y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        gs.append(m.hip_engine.G.clone())
    assert torch.equal(gs[0], gs[1])


def _two_stream_vs_one(dtype, img, train, prune_last=True, row0_attention=True):
    ocfg = O.make_config("micro", img=img, batch=8, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 768, 12
    st = O.init_state(ocfg, seed=8)
    x, y = O.synthetic_batch(ocfg)
    out = []
    for streams in (2, 1):
        m = _model(ocfg, dtype=dtype)
        m.load_state_dict(st)
        m.train(train)
        m.hip_engine.fwd_streams = streams
        m.hip_engine.prune_last, m.hip_engine.row0_attention = prune_last, row0_attention
        torch.manual_seed(5)
        logits = m(x.to(DEV))
        loss = cross_entropy(logits, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        out.append((logits.detach().clone(), loss.detach().clone(), m.hip_engine.G.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2])


@pytest.mark.parametrize("dtype,img,train", [(torch.bfloat16, 224, True), (torch.bfloat16, 224, False),
                                             (torch.float32, 64, True), (torch.bfloat16, 64, True)])
def test_two_stream_forward_bitwise_equal(dtype, img, train):
    """The forward's encoder blocks as two half-batch chains on two streams (engine.fwd_streams = 2, the default for
    batches divisible by 8) equal one chain bit for bit: logits, loss, every gradient (the backward reads the same
    saved tensors), dropout bits included — the half-batch GEMMs draw the whole batch's dropout indices (vit_gemm_desc
    dropout_row0).  ViT-B width, 2 blocks (the second pruned, with the query-0 attention), B = 8."""
    _two_stream_vs_one(dtype, img, train)


@pytest.mark.parametrize("prune_last,row0_attention", [(True, False), (False, True)])
def test_two_stream_forward_bitwise_equal_last_block_modes(prune_last, row0_attention):
    """... and so with the other forms of the last block: pruned with the full attention (after the chains join, with
    no per-chain ln1 / K-V pass), and not pruned at all (every block split, none after the join).  The smallest case
    above: bf16, 64^2, training, B = 8 (the smallest batch the split takes), 2 blocks (one split, one last)."""
    _two_stream_vs_one(torch.bfloat16, 64, True, prune_last, row0_attention)


def test_two_stream_forward_no_grad_bitwise_equal():
    """The inference forward (torch.no_grad: nothing saved, no masks kept) through the two-chain forward equals one
    chain bit for bit, in eval and in train mode (dropout drawn, keep bits not stored).  Five blocks: the four split
    ones reuse the two ping-ponged buffer sets twice each."""
    ocfg = O.make_config("micro", img=224, batch=8, blocks=5)
    ocfg.embedding_size, ocfg.num_heads = 768, 12
    st = O.init_state(ocfg, seed=10)
    x, _ = O.synthetic_batch(ocfg)
    for train in (False, True):
        out = []
        for streams in (2, 1):
            m = _model(ocfg, dtype=torch.bfloat16)
            m.load_state_dict(st)
            m.train(train)
            m.hip_engine.fwd_streams = streams
            torch.manual_seed(3)
            with torch.no_grad():
                out.append(m(x.to(DEV)).clone())
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]), train


def test_two_threads_forward_bitwise_and_no_option_mutation():
    """Two models forwarding concurrently from two host threads: each thread's logits equal its solo
    run bit for bit, and the two-chain forward never touches the process-wide option table (its 3/4-CU ring-attention
    grid travels per call, vit_attn_fwd max_wgs, ABI 14) — polled while both threads run."""
    import threading
    ocfg = O.make_config("micro", img=224, batch=8, blocks=3)
    ocfg.embedding_size, ocfg.num_heads = 768, 12
    x, _ = O.synthetic_batch(ocfg)
    xd = x.to(DEV)
    models, solo = [], []
    for i, streams in enumerate((2, 1)):
        m = _model(ocfg, dtype=torch.bfloat16)
        m.load_state_dict(O.init_state(ocfg, seed=20 + i))
        m.eval()
        m.hip_engine.fwd_streams = streams
        with torch.no_grad():
            solo.append(m(xd).clone())
        models.append(m)
    torch.cuda.synchronize()
    assert _lib.get_option("attn_fwd_grid") == 0
    results = [[], []]
    errors = []

    def run(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st), torch.no_grad():
                for _ in range(6):
                    results[i].append(models[i](xd).clone())
            st.synchronize()
        except Exception as e:          # surfaced below
            errors.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    seen = set()
    while any(t.is_alive() for t in threads):
        seen.add(_lib.get_option("attn_fwd_grid"))
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert seen <= {0}
    for i in range(2):
        assert len(results[i]) == 6
        for r in results[i]:
            assert torch.equal(r, solo[i]), i


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_long_sequence_384_vs_oracle(dtype):
    """BASELINE config 5's sequence length (384^2 / patch 16 -> 576 patches + cls = 577 tokens) at reduced width
    (D=128, H=2, hd=64, L=1, B=2): T > 256 takes the tiled attention kernels (attn_fwd_mfma, attn_bwd_dq_mfma,
    attn_bwd_dkdv_mfma; delta in the dQ kernel), not the single-workgroup fused ones.  fp32: logits 1e-4, grads 2e-4 (scaled);
    bf16: the same gate as test_bf16_vs_oracle_same_rounding."""
    ocfg = O.make_config("micro", img=384, batch=2, blocks=1)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    st = O.init_state(ocfg, seed=3)
    bf = dtype == "bf16"
    m = _model(ocfg, dtype=torch.bfloat16 if bf else torch.float32)
    m.load_state_dict(st)
    m.eval()
    x, y = O.synthetic_batch(ocfg)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    loss.backward()
    lg_32, loss_32, g_32 = O.loss_and_grads(st, x, y, ocfg)
    if not bf:
        assert (logits.detach().cpu() - lg_32).abs().max().item() < 1e-4
        assert abs(loss.item() - loss_32.item()) < 1e-5
        for k, p in m.named_parameters():
            err = (p.grad.cpu() - g_32[k]).abs().max().item()
            assert err <= 2e-4 * max(1.0, g_32[k].abs().max().item()), (k, err)
        return
    lg_bf, _, g_bf = O.loss_and_grads(st, x, y, ocfg, bf16=True)
    assert _rel(logits.detach().cpu(), lg_bf) < 1e-2
    # The query / key projection gradients are dS-driven (dQ = dS K, dK = dS^T Q over 577 tokens, each softmax row
    # of dS summing to zero), so bf16 rounding of P / dS is amplified by cancellation (the bf16-emulating oracle
    # itself is 4-12% off fp32 there).  Gate: the spread of VALID bf16 evaluations between the same
    # storage points — fp32 and fp64 arithmetic, and the flash kernels' own roundings (oracle flash=True: P rounded
    # for dV, dS rounded for dQ / dK, delta from the unrounded O, which is what the tiled kernels take from o32) —
    # at 2x, floor 1e-2; query / key gradients per block with both heads together, as in the headline-width tests.
    valid = [g_bf, O.loss_and_grads(st, x, y, ocfg, bf16=True, dtype=torch.float64)[2],
             O.loss_and_grads(st, x, y, ocfg, bf16=True, flash=True)[2]]
    groups = {}
    for k in g_32:
        if ".query." in k or ".key." in k:
            groups.setdefault(k.split(".multi_head")[0] + " q/k (all heads)", []).append(k)
        else:
            groups[k] = [k]
    ours = {k: p.grad.cpu() for k, p in m.named_parameters()}

    def cat(gd, keys):
        return torch.cat([gd[k].reshape(-1).double() for k in keys])

    bad = []
    for name, keys in groups.items():
        e = _rel(cat(ours, keys), cat(g_32, keys))
        spread = max(_rel(cat(v, keys), cat(g_32, keys)) for v in valid)
        print(f"{name}: ours {e:.4f} valid spread {spread:.4f} ratio {e / max(spread, 1e-9):.2f}")
        if e > max(1e-2, 2 * spread):
            bad.append((name, e, spread))
    assert not bad, bad


@pytest.mark.parametrize("preset,img,batch", [("large", 224, 128), ("base", 384, 64)])
def test_full_size_configs_properties(preset, img, batch):
    """BASELINE configs 4 (ViT-L/16 224^2, B=128/GPU) and 5 (ViT-B/16 384^2, B=64) at full size in bf16: finite loss,
    bitwise-deterministic gradients over two identical steps, loss decreases over 3 FusedAdamW steps."""
    c = config.ViTConfig.preset(preset, img_size=img, batch_size=batch, precision=torch.bfloat16, device="cpu")
    torch.manual_seed(0)
    m = vit.VisionTransformer(c).to(DEV).eval()
    x = torch.randn(batch, 3, img, img, generator=torch.Generator().manual_seed(7)).to(DEV)
    y = torch.randint(0, 1000, (batch,), generator=torch.Generator().manual_seed(8)).to(DEV)
    gs = []
    for _ in range(2):
        loss = cross_entropy(m(x), y)
        for p in m.parameters():
            p.grad = None
        loss.backward()
        gs.append(m.hip_engine.G.clone())
        assert torch.isfinite(loss).item()
    assert torch.equal(gs[0], gs[1])
    assert torch.isfinite(gs[0]).all().item()
    del gs
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    losses = []
    for _ in range(3):
        loss = cross_entropy(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[2] < losses[0], losses


def _engine_relu_masks(m, x, L, B, T, D, own):
    """The engine's ReLU branch decisions per block (the forward's saved mask4 bits, decoded by vit_mask4_apply) as
    bool [B, T, 4D]; the pruned last block has them for its token-0 rows only, its other rows keep `own` (the oracle's
    decisions: those rows carry no gradient and are never read)."""
    _, tape = m.hip_engine.forward(x, False, True)
    out = {}
    for l in range(L):
        hm = tape.blocks[l].hm
        R = B if (tape.pruned and l == L - 1) else B * T
        ones = torch.ones(R, 4 * D, device=DEV)
        bits = _ops.mask4_apply(ones, torch.empty_like(ones), hm, 1.0) > 0
        if R == B * T:
            out[l] = bits.view(B, T, 4 * D)
        else:
            full = own[l].clone()
            full[:, 0] = bits
            out[l] = full
    return out


def test_vit_base_full_depth_fp32_vs_fp64():
    """ViT-B/16 at FULL depth (12 blocks, transformer.py:82-90), 224^2, B=8, fp32, eval mode, through the engine vs the
    oracle evaluated on the GPU in fp64.  Gates:
      * logits: max-abs error vs fp64 <= max(1e-4, 2x the fp32 oracle's error vs fp64 (torch GEMMs: what the
        reference runs));
      * ReLU branches: the FFN ReLU decides on the sign of a pre-activation, and one whose value sits at 0 to within
        rounding can go either way in any valid evaluation; with few gradient rows (the pruned last block: B token-0
        rows, 24.6k hidden values) one such flip moves that block's fc1 / ln2 gradients by ~1% (measured: 0.9%; the
        teacher-forced fp32 blocks show the same 1e-3 jumps at blocks where a flip occurs).  So every engine decision
        that differs from fp64's must be a near-tie (|pre-activation| <= 1e-3 of its row's max: at depth the block
        inputs themselves carry the amplified rounding of the blocks below), and such flips must be rare (<= 1e-4 of
        the decisions; measured 1.2e-5; a wrong mask bit layout flips ~half of them); then
      * gradients vs fp64 evaluated with the engine's ReLU branches (the way the dropout masks are shared): every
        tensor within max(2e-4, 4x the larger error of two valid fp32 summation orders — torch's and the oracle with
        sequential-chain accumulation, this path's order — on the same branches), and the whole gradient vector
        within 2x the sequential-order sample (the rule of test_tiny_c1_fp32_vs_reference)."""
    ocfg = O.make_config("base", img=224, batch=8, num_classes=1000)
    L, B, T, D = ocfg.num_blocks, ocfg.batch_size, ocfg.T, ocfg.embedding_size
    st = O.init_state(ocfg, seed=31)
    m = _model(ocfg)
    m.load_state_dict(st)
    m.eval()
    x, y = O.synthetic_batch(ocfg)
    xd, yd = x.to(DEV), y.to(DEV)
    logits = m(xd)
    cross_entropy(logits, yd).backward()
    ours = {k: p.grad.detach().double() for k, p in m.named_parameters()}
    logits = logits.detach().double()
    sd = {k: v.to(DEV) for k, v in st.items()}
    pre64 = {}
    lg64, _, g64_own = O.loss_and_grads(sd, xd, yd, ocfg, dtype=torch.float64, record=pre64)
    own = {l: pre64[l] > 0 for l in range(L)}
    with torch.no_grad():
        masks = _engine_relu_masks(m, xd, L, B, T, D, own)
    del m
    torch.cuda.empty_cache()
    pre32 = {}
    lg32, _, _ = O.loss_and_grads(sd, xd, yd, ocfg, record=pre32)
    ref_err = float((lg32.double() - lg64).abs().max())
    our_err = float((logits - lg64).abs().max())
    print(f"logits max-abs vs fp64: ours {our_err:.3e}, oracle fp32 {ref_err:.3e}")
    assert our_err <= max(1e-4, 2 * ref_err), (our_err, ref_err)
    flips, flips32, worst_tie, total = 0, 0, 0.0, 0
    for l in range(L):
        rows = slice(None) if l < L - 1 else slice(0, 1)                 # the pruned block decides token 0 only
        z, mk = pre64[l][:, rows], masks[l][:, rows]
        diff = mk != (z > 0)
        total += diff.numel()
        flips32 += int(((pre32[l][:, rows] > 0) != (z > 0)).sum())
        if bool(diff.any()):
            scale = z.abs().amax(-1, keepdim=True).expand_as(z)
            flips += int(diff.sum())
            worst_tie = max(worst_tie, float((z.abs() / scale)[diff].max()))
    print(f"ReLU branches differing from fp64: ours {flips} of {total} (the fp32 oracle's: {flips32}), largest "
          f"|pre-activation| / row max {worst_tie:.2e}")
    assert worst_tie <= 1e-3 and flips <= max(2, 1e-4 * total), (flips, worst_tie)
    _, _, g64 = O.loss_and_grads(sd, xd, yd, ocfg, dtype=torch.float64, relu_masks=masks)
    _, _, g32 = O.loss_and_grads(sd, xd, yd, ocfg, relu_masks=masks)
    _, _, gsq = O.loss_and_grads(sd, xd, yd, ocfg, seq_chain=True, relu_masks=masks)
    worst, bad = [], []
    cat = {"ours": [], "seq": [], "r64": []}
    for k in g64:
        r64 = g64[k].reshape(-1)
        n64 = max(float(r64.norm()), 1e-30)
        e_ours = float((ours[k].reshape(-1) - r64).norm()) / n64
        e_ref = max(float((g32[k].double().reshape(-1) - r64).norm()),
                    float((gsq[k].double().reshape(-1) - r64).norm())) / n64
        e_own = float((ours[k].reshape(-1) - g64_own[k].reshape(-1)).norm()) / n64
        worst.append((e_ours / max(e_ref, 1e-12), k, e_ours, e_ref, e_own))
        if e_ours > max(2e-4, 4 * e_ref):          # the ViT-Tiny rule (round 6: was 8x; measured worst 2.16x)
            bad.append((k, e_ours, e_ref))
        cat["ours"].append(ours[k].reshape(-1))
        cat["seq"].append(gsq[k].double().reshape(-1))
        cat["r64"].append(r64)
    print("worst gradient error ratios (ours / valid-order error, ours vs fp64 on the same ReLU branches, ours vs "
          "fp64 on its own branches):", sorted(worst)[-4:])
    assert not bad, bad
    o, sq, r = (torch.cat(cat[n_]) for n_ in ("ours", "seq", "r64"))
    e_all, e_sq = float((o - r).norm()), float((sq - r).norm())
    print(f"whole gradient vector: ours {e_all / float(r.norm()):.3e}, seq-chain {e_sq / float(r.norm()):.3e}")
    assert e_all <= max(1e-5 * float(r.norm()), 2 * e_sq)
