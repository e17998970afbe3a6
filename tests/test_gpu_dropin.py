"""Drop-in behaviour and headline-shape parity on the MI355X (round 2):

  * bf16 engine parity at ViT-Base width (D=768, H=12, T=197, L=2, B=2), eval AND train (dropout), against the oracle
    that rounds to bf16 at the same storage points — this runs the C2 kernel variants: v4 GEMM epilogues at N=768,
    attn_*_fused<7> with H=12, split-K weight gradients at D=768;
  * the inference path: `store_attention_probs=True` and the no-grad eval forward vs the oracle's
    `keep_probs` forward (transformer.py:48);
  * the reference's only hand KAT (tests/multihead-attention-test.ipynb:231-240,266-289: divide-by-sqrt(d), hd=2,
    two heads) through vit_gemm + vit_attn_fwd;
  * the RCCL branch of the engine's bucketed all-reduce on a world-size-1 `nccl` group (default and side-stream
    weight gradients): gradients bitwise equal to the non-parallel run;
  * module semantics: requires_grad (frozen parameters), input gradient, parameter hooks, deepcopy, DDP refusal,
    FusedAdamW state reload.
"""
import copy
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _engine, _lib, _ops, config, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy

DEV = "cuda"


def _model(ocfg, st, dtype=torch.float32):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st)
    return m.to(DEV)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(b.double().norm(), 1e-30))


def _hd64_cfg(img=64, batch=3, blocks=2):
    ocfg = O.make_config("micro", img=img, batch=batch, blocks=blocks)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    return ocfg


@pytest.mark.parametrize("preset,img", [("base", 224), ("large", 224), ("base", 384)],
                         ids=["C2_base224", "C4_large224", "C5_base384"])
@pytest.mark.parametrize("train", [False, True])
def test_base_width_bf16_engine_vs_oracle(train, preset, img):
    """BASELINE shapes through the engine in bf16 at L=2, B=2, nc=1000: C2 (D=768, H=12, hd 64, T=197), C4's ViT-L
    width (D=1024, H=16, T=197: v4 GEMMs at N=1024/3072/4096, split-K wgrad at D=1024) and C5's sequence (T=577 at
    D=768: the tiled T > 256 attention kernels and v4 GEMMs at M=1154).

    Tolerance scale: the spread of VALID bf16 evaluations, each rounding to bf16 at this path's storage points —
    the oracle with fp32 arithmetic between them, the same with fp64, and the same with the MFMA flash-attention
    kernels' internal roundings (oracle `flash=True`: P and dS in bf16).  Gates:
      * logits within 1e-2 (norm-wise) of the bf16 oracle;
      * every gradient except the attention query / key projections: error vs the fp32 oracle <= max(1e-2, 2 x the
        largest error of a valid evaluation) — north_star's 1e-2 bf16 tolerance as the floor;
      * query / key projection gradients, per block with all heads concatenated: the same gate.  Per head they are
        chaotic under the saturating x sqrt(hd) softmax — block 1's attention gets gradient on query 0 only (the
        classifier reads token 0), and two valid evaluations differ by 10-200% on single heads (measured);
      * the whole gradient vector: <= max(1e-2, 2 x the largest valid error).
    Train mode uses the same counter-hash dropout masks in all evaluations (element-exact mask parity)."""
    ocfg = O.make_config(preset, img=img, batch=2, blocks=2, num_classes=1000)
    st = O.init_state(ocfg, seed=21)
    m = _model(ocfg, st, torch.bfloat16).train(train)
    x, y = O.synthetic_batch(ocfg)
    torch.manual_seed(5)
    base_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(5)
    logits = m(x.to(DEV))
    loss = cross_entropy(logits, y.to(DEV))
    loss.backward()
    ours = {k: p.grad.cpu().double() for k, p in m.named_parameters()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    kw = dict(train=train, seed=base_seed)
    lg_bf, _, g_bf = O.loss_and_grads(st, x, y, ocfg, bf16=True, **kw)
    _, _, g_32 = O.loss_and_grads(st, x, y, ocfg, **kw)
    valid = [g_bf, O.loss_and_grads(st, x, y, ocfg, bf16=True, dtype=torch.float64, **kw)[2],
             O.loss_and_grads(st, x, y, ocfg, bf16=True, flash=True, **kw)[2]]
    assert _rel(logits.detach().cpu(), lg_bf) < 1e-2

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
    print("worst error ratios:", sorted(worst)[-4:])
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_forward_and_attention_probs_vs_oracle(dtype):
    """evaluate() path: no-grad eval forward with store_attention_probs=True vs oracle.forward(keep_probs=True)."""
    ocfg = _hd64_cfg()
    st = O.init_state(ocfg, seed=6)
    bf = dtype == "bf16"
    m = _model(ocfg, st, torch.bfloat16 if bf else torch.float32).eval()
    m.store_attention_probs = True
    x, _ = O.synthetic_batch(ocfg)
    with torch.no_grad():
        logits = m(x.to(DEV))
    ref, probs = O.forward(st, x, ocfg, keep_probs=True, bf16=bf)
    if bf:
        assert _rel(logits.cpu(), ref) < 1e-2
    else:
        assert (logits.cpu() - ref).abs().max().item() < 1e-4
    for l, blk in enumerate(m.transformer_encoder.blocks):
        p = blk.multi_head.attention_probs
        assert p is not None and tuple(p.shape) == (ocfg.batch_size, ocfg.num_heads, ocfg.T, ocfg.T)
        err = (p.cpu() - probs[l]).abs().max().item()
        assert err < (2e-2 if bf else 5e-5), (l, err)
    # without the flag the fused path keeps no probabilities (477 MB per layer at ViT-B/16 B256)
    m.store_attention_probs = False
    with torch.no_grad():
        again = m(x.to(DEV))
    assert all(b.multi_head.attention_probs is None for b in m.transformer_encoder.blocks)
    if bf:      # probabilities come from the VALU attention kernel; the MFMA one runs without them
        assert _rel(again.cpu(), ref) < 1e-2
    else:       # the pruned last block runs query 0 alone without probabilities: summation order only
        assert (again - logits).abs().max().item() < 1e-5


def test_attention_probs_auto_default(probs_auto_budget, monkeypatch):
    """store_attention_probs=None (the default, vit.py): a small batch fills every block's attention_probs on the
    fused path — no-grad eval forward and autograd training forward alike, as the reference does on every forward
    (transformer.py:48) — equal to the oracle's; above vit.ATTENTION_PROBS_AUTO_BYTES they are skipped (None)."""
    ocfg = _hd64_cfg()
    st = O.init_state(ocfg, seed=6)
    m = _model(ocfg, st).eval()
    assert m.store_attention_probs is None and m.wants_attention_probs(ocfg.batch_size)
    x, y = O.synthetic_batch(ocfg)
    with torch.no_grad():
        logits = m(x.to(DEV))
    ref, probs = O.forward(st, x, ocfg, keep_probs=True)
    assert (logits.cpu() - ref).abs().max().item() < 1e-4
    for l, blk in enumerate(m.transformer_encoder.blocks):
        p = blk.multi_head.attention_probs
        assert p is not None and (p.cpu() - probs[l]).abs().max().item() < 5e-5, l
        blk.multi_head.attention_probs = None
    m.train()
    loss = cross_entropy(m(x.to(DEV)), y.to(DEV))
    loss.backward()
    assert all(b.multi_head.attention_probs is not None for b in m.transformer_encoder.blocks)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setattr(vit, "ATTENTION_PROBS_AUTO_BYTES", 0)
    m.eval()
    with torch.no_grad():
        again = m(x.to(DEV))
    assert all(b.multi_head.attention_probs is None and b.multi_head._probs_skipped
               for b in m.transformer_encoder.blocks)
    assert (again - logits).abs().max().item() < 1e-5


@pytest.mark.parametrize("T", [197, 577])
def test_attention_backward_exact_delta_under_saturation(libopt, T):
    """The x sqrt(hd) scale saturates most softmax rows (max P > 0.99); there dS = P (dP - delta) is a tiny difference.
    The shipped backward forms delta exactly to fp32 — T <= 256: the fused kernel from its own fp32 P and dP (no O
    read at all); T > 256: the tiled kernels from the forward's fp32 O (o32) — and dQ / dK track an fp64 evaluation on
    the same bf16 Q, K, V as closely as rounding dS to bf16 allows (emulated: ~2e-3); delta from the bf16 O (the tiled
    kernels without o32) does not.  Gradient only on query 0 of each image (the last block of the model: the
    classifier reads token 0)."""
    B, H, hd = 4, 12, 64
    D = H * hd
    g = torch.Generator().manual_seed(31)
    a = torch.randn(B * T, D, generator=g, dtype=torch.float64)
    W = (torch.rand(3 * D, D, generator=g, dtype=torch.float64) * 2 - 1) / D ** 0.5
    qkv = (a @ W.t()).to(torch.bfloat16)
    d_o = torch.zeros(B, T, D, dtype=torch.float64)
    d_o[:, 0] = torch.randn(B, D, generator=g, dtype=torch.float64) * 1e-2
    d_o = d_o.view(B * T, D).to(torch.bfloat16)
    scale = hd ** 0.5
    qd, dd = qkv.to(DEV), d_o.to(DEV)
    uses_o32 = _ops.attn_bwd_uses_o32(B, T, H, hd, torch.bfloat16)
    assert uses_o32 == (T > 256)
    o32 = torch.empty(B * T, D, dtype=torch.float32, device=DEV) if uses_o32 else None
    o, lse = _ops.attn_fwd(qd, B, T, H, hd, scale, o32=o32)
    o_ref, lse_ref = _ops.attn_fwd(qd, B, T, H, hd, scale)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    exact = _ops.attn_bwd(qd, o, dd, lse, B, T, H, hd, scale, o32=o32).double().cpu()
    libopt("attn_bwd_split", 1)                        # the tiled kernels with delta from the bf16 O
    approx = _ops.attn_bwd(qd, o, dd, lse, B, T, H, hd, scale).double().cpu()
    # fp64 reference on the same bf16 inputs
    q, k, v = (qkv.double().view(B, T, 3, H, hd)[:, :, i].transpose(1, 2) for i in range(3))
    q.requires_grad_(True)
    k.requires_grad_(True)
    v.requires_grad_(True)
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    (P @ v).backward(d_o.double().view(B, T, H, hd).transpose(1, 2))
    assert float((P[:, :, 0].max(-1).values > 0.99).double().mean()) > 0.25       # saturated rows present
    ref = torch.cat([t.transpose(1, 2).reshape(B * T, D) for t in (q.grad, k.grad, v.grad)], 1)   # [B*T, 3D]
    for name, sl in (("dQ", slice(0, D)), ("dK", slice(D, 2 * D)), ("dV", slice(2 * D, 3 * D))):
        e_exact = _rel(exact[:, sl], ref[:, sl])
        e_approx = _rel(approx[:, sl], ref[:, sl])
        print(f"T={T} {name}: exact-delta {e_exact:.2e}, bf16-O delta {e_approx:.2e}")
        assert e_exact < 1e-2, (name, e_exact)
    assert _rel(exact[:, :D], ref[:, :D]) < _rel(approx[:, :D], ref[:, :D])


def test_notebook_sdpa_kat_through_c_abi(golden_dir):
    """G5 (tests/multihead-attention-test.ipynb): for each (block, head) of the notebook's weights, Q/K/V = emb W and
    softmax(Q K^T / sqrt(2)) V, computed by vit_gemm + vit_attn_fwd (scale = 1/sqrt(2), H = 2, hd = 2, T = 5).
    Expected outputs are printed at 4 dp in the notebook."""
    k = json.load(open(os.path.join(golden_dir, "sdpa_notebook.json")))
    emb = torch.tensor(k["embeddings"], dtype=torch.float32, device=DEV)              # [T=5, D=4]
    w = torch.tensor(k["qkv_weights"], dtype=torch.float32).view(2, 2, 4, 6)          # [block, head, D, 6]
    expected = torch.tensor(k["expected_out"]).view(2, 2, 5, 2)
    for blk in range(2):
        # fused projection matrix [3*H*hd, D]: rows = Q of head 0, 1, then K, then V (the engine's layout)
        rows = [w[blk, h, :, c0:c0 + 2].t() for c0 in (0, 2, 4) for h in range(2)]
        wf = torch.cat(rows, 0).contiguous().to(DEV)
        qkv = torch.empty(5, 12, dtype=torch.float32, device=DEV)
        _ops.gemm(emb, wf, qkv, 5, 12, 4, 4, 4, 12)
        o, lse = _ops.attn_fwd(qkv, 1, 5, 2, 2, 1.0 / 2 ** 0.5)
        torch.cuda.synchronize()
        for h in range(2):
            np.testing.assert_allclose(o[:, 2 * h:2 * h + 2].cpu().numpy(), expected[blk, h].numpy(), atol=6e-4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("side_stream,comm", [(False, "fp32"), (True, "fp32"), (False, "bf16"), (True, "bf16")])
def test_rccl_bucket_allreduce_world1_bitwise(side_stream, comm):
    """The engine's RCCL branch (ReduceOp.AVG on the `nccl` backend = RCCL, launched per block bucket inside the
    backward, optionally from the weight-gradient side stream) on a one-rank group: gradients equal the
    non-parallel run bit for bit; with bf16 buckets (enable_data_parallel(grad_dtype=torch.bfloat16)) they equal the
    non-parallel gradients rounded to bf16 (the average of one rank), and comm_exposed_ms() reports a time."""
    import torch.distributed as dist
    ocfg = _hd64_cfg(batch=4)
    st = O.init_state(ocfg, seed=8)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)

    def grads(ddp):
        m = _model(ocfg, st, torch.bfloat16).train()
        m.hip_engine.concurrent_wgrad = side_stream
        if ddp:
            m.enable_data_parallel(force=True, grad_dtype=torch.bfloat16 if comm == "bf16" else torch.float32)
            assert m.hip_engine.ddp_enabled and dist.get_backend() == "nccl"
            m.hip_engine.time_comm = True
        torch.manual_seed(3)
        cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        if ddp:
            t = m.hip_engine.comm_exposed_ms()
            assert t is not None and t >= 0.0
        return m.hip_engine.G.clone()

    g_plain = grads(False)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=torch.device(DEV, torch.cuda.current_device()))
    try:
        g_ddp = grads(True)
    finally:
        dist.destroy_process_group()
    assert torch.equal(g_plain.bfloat16().float() if comm == "bf16" else g_plain, g_ddp)


def test_frozen_parameters_and_input_gradient():
    """requires_grad=False: no .grad, no weight-gradient GEMM; the rest still matches the oracle.  x.requires_grad:
    the input-image gradient (conv dgrad + col2im) matches the oracle's autograd input gradient."""
    ocfg = _hd64_cfg()
    st = O.init_state(ocfg, seed=9)
    m = _model(ocfg, st).eval()
    frozen = {k for k in st if k.startswith("transformer_encoder.blocks.1.") or k.endswith("mlp.0.weight")}
    for k, p in m.named_parameters():
        p.requires_grad_(k not in frozen)
    x, y = O.synthetic_batch(ocfg)
    xd = x.to(DEV).requires_grad_(True)
    cross_entropy(m(xd), y.to(DEV)).backward()
    params = {k: v.detach().clone().requires_grad_(k not in frozen) for k, v in st.items()}
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(O.forward(params, xr, ocfg), y).backward()
    for k, p in m.named_parameters():
        if k in frozen:
            assert p.grad is None, k
        else:
            ref = params[k].grad
            assert (p.grad.cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item()), k
    assert (xd.grad.cpu() - xr.grad).abs().max().item() <= 1e-4 * max(1.0, xr.grad.abs().max().item())
    # freezing everything below the head stops the backward at the head (no encoder work, same head grads)
    m2 = _model(ocfg, st).eval()
    for k, p in m2.named_parameters():
        p.requires_grad_(k.startswith("mlp."))
    cross_entropy(m2(x.to(DEV)), y.to(DEV)).backward()
    assert all(p.grad is None for k, p in m2.named_parameters() if not k.startswith("mlp."))
    ref = dict(m.named_parameters())["mlp.3.weight"].grad
    assert torch.allclose(dict(m2.named_parameters())["mlp.3.weight"].grad, ref, atol=1e-6)


def test_parameter_hooks_run_once_per_backward():
    ocfg = _hd64_cfg()
    m = _model(ocfg, O.init_state(ocfg, seed=10)).eval()
    seen = []
    w = m.transformer_encoder.blocks[0].multi_head.heads[1].value.weight
    m.mlp[3].bias.register_post_accumulate_grad_hook(lambda p: seen.append(("post", p.grad.clone())))
    w.register_hook(lambda g: g * 0.5)
    x, y = O.synthetic_batch(ocfg)
    cross_entropy(m(x.to(DEV)), y.to(DEV)).backward()
    g_half = w.grad.clone()
    assert len(seen) == 1 and torch.equal(seen[0][1], m.mlp[3].bias.grad)
    m2 = _model(ocfg, O.init_state(ocfg, seed=10)).eval()
    cross_entropy(m2(x.to(DEV)), y.to(DEV)).backward()
    w2 = m2.transformer_encoder.blocks[0].multi_head.heads[1].value.weight
    assert torch.allclose(g_half, 0.5 * w2.grad)


def test_parameter_hooks_with_gradient_accumulation():
    """Two backwards without zero_grad: a `register_hook` hook transforms each backward's gradient only,
    as autograd's does — 0.5 g1 + 0.5 g2, not 0.5 (0.5 g1 + g2) — and hook-free parameters accumulate exactly as
    without hooks."""
    ocfg = _hd64_cfg()
    st = O.init_state(ocfg, seed=12)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)

    def run(hook):
        m = _model(ocfg, st).eval()
        if hook:
            m.transformer_encoder.blocks[0].multi_head.heads[1].value.weight.register_hook(lambda g: g * 0.5)
        for _ in range(2):
            cross_entropy(m(x), y).backward()
        return dict(m.named_parameters())

    hooked, plain = run(True), run(False)
    key = "transformer_encoder.blocks.0.multi_head.heads.1.value.weight"
    # same input twice in eval mode: g1 == g2, so autograd gives g1 = 0.5 * (g1 + g2) exactly
    assert torch.equal(hooked[key].grad, 0.5 * plain[key].grad)
    for k, p in hooked.items():
        if k != key:
            assert torch.allclose(p.grad, plain[k].grad, rtol=1e-6, atol=1e-7), k


@pytest.mark.parametrize("hook", [True, False])
def test_freeze_between_accumulating_backwards(hook):
    """a parameter frozen between two accumulating backwards keeps the .grad it had (autograd never touches
    a frozen parameter's gradient), also when it shares the fused QKV gradient region with heads that still train
    and when another parameter's `register_hook` sends the backward through the hook-accumulation path."""
    ocfg = _hd64_cfg()
    st = O.init_state(ocfg, seed=15)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)
    m = _model(ocfg, st).eval()
    if hook:
        m.mlp[3].weight.register_hook(lambda g: g * 0.5)
    frozen_keys = ["transformer_encoder.blocks.0.multi_head.heads.0.query.weight",   # shares block 0's QKV region
                   "transformer_encoder.blocks.1.ffwd.mlp.0.weight"]                    # a region of its own
    named = dict(m.named_parameters())
    cross_entropy(m(x), y).backward()
    first = {k: p.grad.clone() for k, p in named.items()}
    for k in frozen_keys:
        named[k].requires_grad_(False)
    cross_entropy(m(x), y).backward()
    for k in frozen_keys:
        assert torch.equal(named[k].grad, first[k]), k
    # the parameters that still train accumulated g1 + g2 = 2 g1 (same input, eval mode)
    for k in ("transformer_encoder.blocks.0.multi_head.heads.0.key.weight", "mlp.3.weight",
              "transformer_encoder.blocks.1.ffwd.mlp.2.weight"):
        assert torch.allclose(named[k].grad, 2 * first[k], rtol=1e-6, atol=1e-7), k


def test_deepcopy_snapshot_is_independent():
    """A deep copy (EMA / best-model snapshot) builds its own engine: same outputs, and training the original does
    not touch the copy."""
    ocfg = _hd64_cfg(batch=4)
    m = _model(ocfg, O.init_state(ocfg, seed=11), torch.bfloat16).eval()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)
    cross_entropy(m(x), y).backward()
    opt.step()
    snap = copy.deepcopy(m)
    with torch.no_grad():
        a, b = m(x), snap(x)
    assert torch.equal(a, b)
    assert snap.hip_engine is not m.hip_engine and snap.hip_engine.model_ref() is snap
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        cross_entropy(m(x), y).backward()
        opt.step()
    with torch.no_grad():
        assert torch.equal(snap(x), b)
        assert not torch.equal(m(x), b)
    assert all(p.grad is None for p in snap.parameters())


def test_ddp_wrapper_is_refused():
    import torch.distributed as dist
    ocfg = _hd64_cfg()
    m = _model(ocfg, O.init_state(ocfg, seed=12))
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    x, _ = O.synthetic_batch(ocfg)
    try:
        try:
            ddp = torch.nn.parallel.DistributedDataParallel(m)
        except RuntimeError:          # gloo without device broadcast: exercise the same forward context directly
            ddp = None
        if ddp is not None:
            with pytest.raises(RuntimeError, match="enable_data_parallel"):
                ddp(x.to(DEV))
        else:
            DDP = torch.nn.parallel.DistributedDataParallel
            fake = torch.nn.Module()
            fake.module = m
            DDP._active_ddp_module = fake
            try:
                with pytest.raises(RuntimeError, match="enable_data_parallel"):
                    m(x.to(DEV))
            finally:
                DDP._active_ddp_module = None
    finally:
        dist.destroy_process_group()


def test_fused_adamw_reload_state_matches_torch():
    """step -> state_dict -> load_state_dict into the SAME optimizer -> step, against torch.optim.AdamW doing the same
    (the cached chunk tables must follow the new moment tensors); step counters stay per-parameter."""
    ocfg = O.make_config("micro", img=32, batch=4)
    st = O.init_state(ocfg, seed=13)
    m = _model(ocfg, st).eval()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    shadow = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    ref = torch.optim.AdamW(shadow, lr=1e-3, weight_decay=1e-4)
    x, y = O.synthetic_batch(ocfg)
    x, y = x.to(DEV), y.to(DEV)
    saved = None
    for i in range(5):
        opt.zero_grad(set_to_none=True)
        cross_entropy(m(x), y).backward()
        for s_, p in zip(shadow, m.parameters()):
            s_.grad = p.grad.clone()
        if i == 2:
            saved = (copy.deepcopy(opt.state_dict()), copy.deepcopy(ref.state_dict()),
                     [p.detach().clone() for p in m.parameters()])
        opt.step()
        ref.step()
        if i == 3:          # roll both back to the snapshot taken before step 2, then continue
            opt.load_state_dict(saved[0])
            ref.load_state_dict(saved[1])
            with torch.no_grad():
                for p, s_, v in zip(m.parameters(), shadow, saved[2]):
                    p.copy_(v)
                    s_.copy_(v)
    for s_, p in zip(shadow, m.parameters()):
        assert (s_.detach() - p.detach()).abs().max().item() < 1e-6
    steps = sorted({float(opt.state[p]["step"]) for p in m.parameters()})
    assert steps == [float(ref.state[shadow[0]]["step"])] == [3.0]
    torch.optim.AdamW(shadow, lr=1e-3).load_state_dict(opt.state_dict())


def test_fused_adamw_follows_repointed_storage():
    """`p.data = new` on a parameter no engine owns, and a replaced moment tensor, after the chunk table was
    cached: the next steps update the new storage (as torch.optim.AdamW does), not the old one."""
    torch.manual_seed(0)
    ps = [torch.randn(37, 5, device=DEV).requires_grad_(True), torch.randn(300, device=DEV).requires_grad_(True)]
    ref = [p.detach().clone().requires_grad_(True) for p in ps]
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=1e-2)
    ropt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    for i in range(4):
        grads = [torch.randn_like(p) for p in ps]
        for p, r, g in zip(ps, ref, grads):
            p.grad, r.grad = g.clone(), g.clone()
        if i == 2:
            with torch.no_grad():
                ps[0].data = ps[0].data.clone() + 1.0       # new storage
                ref[0].data = ref[0].data.clone() + 1.0
                opt.state[ps[1]]["exp_avg"] = opt.state[ps[1]]["exp_avg"].clone()
        opt.step()
        ropt.step()
    for p, r in zip(ps, ref):
        assert (p.detach() - r.detach()).abs().max().item() < 1e-6


def test_fused_adamw_follows_repointed_grad_storage():
    """a .grad tensor object that stays the same while its storage is re-pointed (`p.grad.data = t`,
    `p.grad.set_(t)`) after the chunk table was cached: the next steps read the new gradient storage."""
    torch.manual_seed(1)
    ps = [torch.randn(37, 5, device=DEV).requires_grad_(True), torch.randn(300, device=DEV).requires_grad_(True)]
    ref = [p.detach().clone().requires_grad_(True) for p in ps]
    for p, r in zip(ps, ref):                   # persistent gradient objects, written in place (the engine's way)
        p.grad, r.grad = torch.zeros_like(p), torch.zeros_like(r)
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=1e-2)
    ropt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    for i in range(5):
        grads = [torch.randn_like(p) for p in ps]
        for j, (p, g) in enumerate(zip(ps, grads)):
            if (i, j) == (2, 0):
                p.grad.data = g.clone()                 # same object, new storage
            elif (i, j) == (3, 1):
                p.grad.set_(g.clone())
            else:
                p.grad.copy_(g)
        for r, g in zip(ref, grads):
            r.grad.copy_(g)
        opt.step()
        ropt.step()
    for p, r in zip(ps, ref):
        assert (p.detach() - r.detach()).abs().max().item() < 1e-6


def test_missing_library_fails_loudly(monkeypatch):
    """No silent fallback: a device model with libvit_hip.so absent raises (the host path is never used for device
    tensors)."""
    ocfg = _hd64_cfg()
    m = _model(ocfg, O.init_state(ocfg, seed=14))
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libvit_hip.so")
    x, _ = O.synthetic_batch(ocfg)
    with pytest.raises(_lib.HipLibraryError):
        m(x.to(DEV))


def _engine_vs_oracle_on_gpu(ocfg, seed, full_depth=False):
    """bf16 TRAIN-mode engine run vs the oracle evaluated on the GPU with torch ops.  Depth 2 (full_depth False):
    logits within 1e-2 of the bf16 oracle; each gradient (q/k per block, all heads together) <= max(1e-2, 2 x the
    spread of valid bf16 evaluations: fp32 / fp64 / flash rounding between the same storage points); the whole vector
    likewise.  full_depth: at depth 12 the valid bf16 evaluations themselves disagree by ~46% in the logits (the
    saturating x sqrt(hd) softmax turns rounding differences into different attention argmaxes), so no elementwise
    gate is meaningful there; the run is a property check — finite, and the mean loss within 2e-2 (relative) of the
    fp32 oracle's — and per-block parity at that depth is test_vit_base_depth12_teacher_forced_blocks_bf16."""
    st = O.init_state(ocfg, seed=seed)
    m = _model(ocfg, st, torch.bfloat16).train()
    x, y = O.synthetic_batch(ocfg)
    xd, yd = x.to(DEV), y.to(DEV)
    torch.manual_seed(5)
    base_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(5)
    logits = m(xd)
    loss = cross_entropy(logits, yd)
    loss.backward()
    ours = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    logits, loss = logits.detach(), float(loss)
    del m
    torch.cuda.empty_cache()
    sd = {k: v.to(DEV) for k, v in st.items()}
    kw = dict(train=True, seed=base_seed)
    lg_bf, loss_bf, g_bf = O.loss_and_grads(sd, xd, yd, ocfg, bf16=True, **kw)
    lg_32, loss_32, g_32 = O.loss_and_grads(sd, xd, yd, ocfg, **kw)
    lg_64, _, g_64 = O.loss_and_grads(sd, xd, yd, ocfg, bf16=True, dtype=torch.float64, **kw)
    lg_fl, _, g_fl = O.loss_and_grads(sd, xd, yd, ocfg, bf16=True, flash=True, **kw)
    valid = [g_bf, g_64, g_fl]
    lspread = max(_rel(v, lg_32) for v in (lg_bf, lg_64, lg_fl))
    print(f"logits: vs bf16 oracle {_rel(logits, lg_bf):.3e}, vs fp32 {_rel(logits, lg_32):.3e}, "
          f"valid-bf16 spread {lspread:.3e}; loss ours {loss:.5f} bf16 oracle {float(loss_bf):.5f} "
          f"fp32 {float(loss_32):.5f}")
    if full_depth:
        assert np.isfinite(loss) and all(bool(torch.isfinite(g).all()) for g in ours.values())
        assert abs(loss - float(loss_32)) <= 2e-2 * abs(float(loss_32)), (loss, float(loss_32))
        return
    assert _rel(logits, lg_bf) < 1e-2, _rel(logits, lg_bf)

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
    print("worst error ratios:", sorted(worst)[-4:])
    assert not bad, bad


def test_c2_full_shape_bf16_train_vs_oracle():
    """BASELINE config 2 at its real shape: ViT-B/16 224^2, B=256 (M = 50,432 token rows), bf16, TRAIN mode (dropout),
    two blocks (block 0 runs every GEMM at full M with dense gradients; block 1 is the pruned last block), through the
    engine, against the oracle evaluated on the GPU with torch ops.  This brings the full-size kernels under parity
    test: the K = 50,432 split-K weight-gradient GEMMs, the persistent many-round forward / dgrad GEMMs (591-2,364
    tiles; their split-K tails are off by default since round 5 and gated at these shapes in test_gpu_kernels), the
    3,072-item persistent attention backward.  Gates of _engine_vs_oracle_on_gpu
    (logits 1e-2 vs the bf16 oracle, hard)."""
    _engine_vs_oracle_on_gpu(O.make_config("base", img=224, batch=256, blocks=2, num_classes=1000), seed=23)


def test_vit_large_width_two_chain_ragged_ring_vs_oracle():
    """C4's ViT-L width (D = 1024, H = 16, T = 197) bf16 train through the default two-chain forward (fwd_streams 2)
    at B = 32: each chain's ring attention forward runs its 16 x 16 = 256 items on the 3/4-CU grid
    (192 workgroups: 64 of them take a second item, the rest one), the ragged multi-item case C4 itself hits at
    B = 128 (1,024 items per chain).  Gates of _engine_vs_oracle_on_gpu (logits 1e-2 vs the bf16 oracle)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    items = (32 // 2) * 16
    assert items > cus * 3 // 4 and items % (cus * 3 // 4) != 0
    _engine_vs_oracle_on_gpu(O.make_config("large", img=224, batch=32, blocks=2, num_classes=1000), seed=31)


def test_vit_base_full_depth_bf16_train_properties():
    """ViT-B/16 at FULL depth (12 blocks, transformer.py:82-90), 224^2, B=8, bf16, train mode, through the engine:
    a property check only (finite; loss within 2e-2 of the fp32 oracle's).  Elementwise parity at depth 12 is gated
    per block by the teacher-forced test below and end to end in fp32 by test_vit_base_full_depth_fp32_vs_fp64."""
    _engine_vs_oracle_on_gpu(O.make_config("base", img=224, batch=8, blocks=12, num_classes=1000), seed=29,
                             full_depth=True)


def test_vit_base_depth12_teacher_forced_blocks_bf16():
    """Per-block bf16 parity at C2 widths through depth 12, teacher-forced: the oracle runs the whole
    ViT-B/16 (224^2, B=8, train mode, counter-hash dropout) in fp32 and records every block's input and the loss
    gradient at every block's output; each engine block (Engine.block_forward / block_backward: the fused kernels of
    the whole-model path) is then fed THAT block's input and output gradient, rounded to bf16, so errors cannot
    compound across depth.  Per block, against the oracle block that rounds to bf16 at the same storage points:
      * block output and input gradient within 1e-2 (norm-wise) of the bf16 oracle;
      * every weight gradient (per-head q / k / v of a block concatenated) within max(1e-2, 2x the spread of the
        valid bf16 evaluations — fp32 / fp64 arithmetic, flash rounding — around the fp64 one) of the fp64 one."""
    ocfg = O.make_config("base", img=224, batch=8, num_classes=1000)
    L, B, T, D, H = ocfg.num_blocks, ocfg.batch_size, ocfg.T, ocfg.embedding_size, ocfg.num_heads
    M = B * T
    st = O.init_state(ocfg, seed=29)
    m = _model(ocfg, st, torch.bfloat16).train()
    x, y = O.synthetic_batch(ocfg)
    xd, yd = x.to(DEV), y.to(DEV)
    seed = 987654321
    sd = {k: v.to(DEV) for k, v in st.items()}
    # the teacher: fp32 oracle forward / backward, every block's output kept with its gradient
    e = O.embed_forward(sd, xd, ocfg).detach().requires_grad_(True)
    ins, outs = [], []
    for l in range(L):
        ins.append(e)
        e, _ = O.block_forward(sd, l, e, ocfg, train=True, seed=seed)
        e.retain_grad()
        outs.append(e)
    torch.nn.functional.cross_entropy(O.head_forward(sd, e), yd).backward()
    eng = m.hip_engine
    eng.ensure_ready(xd.device)
    req = {k: True for k in eng.owners}
    rnd = O._RoundBF16.apply
    names = _engine.BLOCK_REGIONS
    bad, report = [], []
    for l in range(L):
        x_in = ins[l].detach().bfloat16()
        dy = outs[l].grad.detach().bfloat16()
        # ---- engine block
        x_out, saved = eng.block_forward(l, x_in.view(M, D).contiguous(), B, True, seed, True)
        eng.G.zero_()
        dxo = dy.view(M, D).contiguous()
        g1 = _ops.mask4_apply(dxo, torch.empty_like(dxo), saved.fm, 1.0)
        dx_in, _ = eng.block_backward(l, saved, dxo, g1, False, 0.0, req, None, True, B)
        torch.cuda.synchronize()
        ours = {n: eng.gw[f"{l}.{n}"].double().clone() for n in names}

        # ---- oracle block between the same bf16 storage points: fp32 / fp64 arithmetic, flash rounding
        def oracle_block(dtype, flash=False):
            pre = f"transformer_encoder.blocks.{l}."
            p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
            xi = x_in.to(dtype).requires_grad_(True)
            yo, _ = O.block_forward(p, l, xi, ocfg, rnd, train=True, seed=seed, flash=flash)
            yo.backward(dy.to(dtype))
            q = [p[pre + f"multi_head.heads.{h}.query.weight"].grad for h in range(H)]
            k = [p[pre + f"multi_head.heads.{h}.key.weight"].grad for h in range(H)]
            v = [p[pre + f"multi_head.heads.{h}.value.weight"].grad for h in range(H)]
            g = {"qkv_w": torch.cat(q + k + v, 0), "proj_w": p[pre + "multi_head.proj.weight"].grad,
                 "proj_b": p[pre + "multi_head.proj.bias"].grad, "fc1_w": p[pre + "ffwd.mlp.0.weight"].grad,
                 "fc1_b": p[pre + "ffwd.mlp.0.bias"].grad, "fc2_w": p[pre + "ffwd.mlp.2.weight"].grad,
                 "fc2_b": p[pre + "ffwd.mlp.2.bias"].grad, "ln1_w": p[pre + "ln1.weight"].grad,
                 "ln1_b": p[pre + "ln1.bias"].grad, "ln2_w": p[pre + "ln2.weight"].grad,
                 "ln2_b": p[pre + "ln2.bias"].grad}
            return yo.detach(), xi.grad.detach(), {n: t.double() for n, t in g.items()}

        y_bf, dx_bf, g_bf = oracle_block(torch.float32)
        _, _, g_64 = oracle_block(torch.float64)
        _, _, g_fl = oracle_block(torch.float32, flash=True)
        e_out = _rel(x_out.view(B, T, D), y_bf)
        e_dx = _rel(dx_in.view(B, T, D), dx_bf)
        report.append((l, "out", e_out))
        report.append((l, "dx", e_dx))
        if e_out >= 1e-2 or e_dx >= 1e-2:
            bad.append((l, "out/dx", e_out, e_dx))
        for n in names:
            e_ours = _rel(ours[n], g_64[n])
            spread = max(_rel(g_bf[n], g_64[n]), _rel(g_fl[n], g_64[n]))
            report.append((l, n, e_ours, spread))
            if e_ours > max(1e-2, 2 * spread):
                bad.append((l, n, e_ours, spread))
        del saved, x_out, dx_in
    print("teacher-forced per-block errors:")
    for r in report:
        print("  ", r)
    assert not bad, bad
