"""Patch dropout on the MI355X: vit_patch_keep against its host twin, the gathering / scattering embedding kernels
against the dense ones, vit_pos_grad_gather against fp64, the engine's gathered embedding against the dense one bit
for bit, the whole model in training mode on T' = K + 1 tokens against the oracle composed on the kept tokens
(tests/patch_drop_reference.py), what must not change (rate 0, eval mode), two data-parallel ranks, the attention
kernels at the token counts the feature introduces, and train()."""
import os
import socket
import sys

import pytest
import torch

from oracle import vit_oracle as O
from patch_drop_reference import BASE_SEED, CASES, check_bf16, check_fp32, check_table, oracle_run

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _cpu, _engine, _functional, _ops, config, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = 0x5A5A5A5A


# ---- vit_patch_keep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", CASES)
def test_patch_keep_is_the_twins_table(B, N, K):
    L = 3
    want_idx, want_inv = _cpu.patch_keep_table(BASE_SEED, L, B, N, K)
    pad = 64                                               # sentinel words after both outputs
    bi = torch.full((B * K + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    bv = torch.full((B * N + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    idx, inv = bi[:B * K].view(B, K), bv[:B * N].view(B, N)
    _ops.patch_keep(BASE_SEED, L, B, N, K, DEV, idx=idx, inv=inv)
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(inv.cpu(), want_inv)
    check_table(idx.cpu(), inv.cpu(), B, N, K)
    assert bool((bi[B * K:] == SENTINEL).all()) and bool((bv[B * N:] == SENTINEL).all())
    first = (bi.clone(), bv.clone())
    bi[:B * K] = -7                                        # a repeated launch gives the same bytes
    bv[:B * N] = -7
    _ops.patch_keep(BASE_SEED, L, B, N, K, DEV, idx=idx, inv=inv)
    assert torch.equal(bi, first[0]) and torch.equal(bv, first[1])
    # another data-parallel rank draws another table, the twin's again
    seed1 = _engine.dropout_seed(BASE_SEED, 1)
    i1, v1 = _ops.patch_keep(seed1, L, B, N, K, DEV)
    t1 = _cpu.patch_keep_table(seed1, L, B, N, K)
    assert torch.equal(i1.cpu(), t1[0]) and torch.equal(v1.cpu(), t1[1])
    if 1 < K < N and B * N >= 64:
        assert not torch.equal(i1, idx)


def test_patch_keep_refusals():
    for B, N, K in ((2, 4, 5), (2, 4, 0), (2, 4097, 8)):
        with pytest.raises(RuntimeError, match="vit_patch_keep"):
            _ops.patch_keep(1, 2, B, N, K, DEV)
    with pytest.raises(TypeError, match="idx"):
        _ops.patch_keep(1, 2, 2, 4, 2, DEV, idx=torch.empty(2, 2, dtype=torch.int64, device=DEV))


# ---- the embedding kernels ------------------------------------------------------------------------------------------
DTYPE_PAIRS = [(torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)]


def _image(B, C, S, dtype, seed=0):
    return torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)


@pytest.mark.parametrize("P,K", [(16, 8), (4, 255), (4, 1)])
@pytest.mark.parametrize("xdt,cdt", DTYPE_PAIRS)
def test_im2col_gather_is_the_dense_rows(xdt, cdt, P, K):
    B, C, S = 3, 3, 64
    N = (S // P) ** 2
    x = _image(B, C, S, xdt)
    dense = _ops.im2col(x, P, cdt)
    idx = _cpu.patch_keep_table(5, 2, B, N, K)[0].to(DEV)
    CPP = C * P * P
    buf = torch.full((B * K * CPP + 64,), -3.0, dtype=cdt, device=DEV)
    cols = _ops.im2col_gather(x, P, cdt, idx, cols=buf[:B * K * CPP].view(B * K, CPP))
    rows = (torch.arange(B, device=DEV)[:, None] * N + idx.long()).reshape(-1)
    assert torch.equal(cols, dense[rows])
    assert bool((buf[B * K * CPP:] == -3.0).all())


@pytest.mark.parametrize("P,K", [(16, 8), (4, 255), (4, 1)])
@pytest.mark.parametrize("xdt,cdt", DTYPE_PAIRS)
def test_col2im_scatter_is_col2im_of_zero_filled_cols(xdt, cdt, P, K):
    """(dtype pairs named as im2col's: the image's, the cols')"""
    B, C, S = 3, 3, 64
    N, CPP = (S // P) ** 2, C * P * P
    idx, inv = (t.to(DEV) for t in _cpu.patch_keep_table(9, 2, B, N, K))
    dcols = torch.randn(B * K, CPP, generator=torch.Generator().manual_seed(1)).to(DEV).to(cdt)
    dense = torch.zeros(B * N, CPP, dtype=cdt, device=DEV)
    rows = (torch.arange(B, device=DEV)[:, None] * N + idx.long()).reshape(-1)
    dense[rows] = dcols
    want = _ops.col2im(dense, torch.empty(B, C, S, S, dtype=xdt, device=DEV), P)
    buf = torch.full((B * C * S * S + 64,), -3.0, dtype=xdt, device=DEV)
    got = _ops.col2im_scatter(dcols, inv, K, buf[:B * C * S * S].view(B, C, S, S), P)
    assert torch.equal(got, want)
    assert bool((buf[B * C * S * S:] == -3.0).all())
    if K < N:
        assert bool((got == 0).any())


def test_gather_pos_rows():
    B, N, K, D = 5, 36, 27, 192
    pos = torch.randn(N + 1, D, device=DEV)
    idx = _cpu.patch_keep_table(3, 2, B, N, K)[0].to(DEV)
    buf = torch.full((B * K * D + 64,), -3.0, device=DEV)
    got = _ops.gather_pos(pos, idx, N, out=buf[:B * K * D].view(B * K, D))
    assert torch.equal(got, pos[idx.long().reshape(-1)])
    assert bool((buf[B * K * D:] == -3.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D", [(1, 192), (65, 768), (65, 192)])
def test_pos_grad_gather_vs_fp64(dtype, B, D):
    """gpos against fp64 from the same inputs at test_gpu_kernels.py's column-sum gate (1e-5 of the column's sum of
    magnitudes + 1e-5), beta 0 and 1, with a position no image kept, bitwise repeats and sentinels."""
    N, K = 16, 8
    idx, inv = _cpu.patch_keep_table(21 + B, 2, B, N, K)
    counts = torch.bincount(idx.long().reshape(-1), minlength=N)
    if B == 1:
        assert int((counts == 0).sum()) == N - K           # positions no image kept
    else:                                                   # make one: drop patch 5 everywhere it was kept
        for b in range(B):
            if inv[b, 5] >= 0:
                free = int((inv[b] < 0).nonzero()[0])
                row = sorted(set(idx[b].tolist()) - {5} | {free})
                idx[b] = torch.tensor(row, dtype=torch.int32)
        inv = torch.full((B, N), -1, dtype=torch.int32)
        inv.scatter_(1, idx.long(), torch.arange(K, dtype=torch.int32).expand(B, K))
    check_table(idx, inv, B, N, K)
    dx = torch.randn(B * (K + 1), D, generator=torch.Generator().manual_seed(B + D)).to(DEV).to(dtype)
    old = torch.randn(N + 1, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    d64 = dx.double().view(B, K + 1, D).cpu()
    ref = torch.zeros(N + 1, D, dtype=torch.float64)
    mag = torch.zeros(N + 1, D, dtype=torch.float64)
    for b in range(B):
        rows = torch.cat([idx[b].long(), torch.tensor([N])])
        ref[rows] += d64[b]
        mag[rows] += d64[b].abs()
    invd = inv.to(DEV)
    for beta in (0.0, 1.0):
        buf = torch.full(((N + 1) * D + 64,), float("nan") if beta == 0.0 else 0.0, device=DEV)
        gpos = buf[:(N + 1) * D].view(N + 1, D)
        if beta:
            gpos.copy_(old)
        buf[(N + 1) * D:] = -3.0
        _ops.pos_grad_gather(dx, invd, K, gpos, beta=beta)
        want = ref + beta * old.double().cpu()
        err = (gpos.double().cpu() - want).abs()
        bound = 1e-5 * (mag + beta * old.double().cpu().abs()) + 1e-5
        print(f"pos_grad_gather {dtype} B={B} D={D} beta={beta}: max err {err.max().item():.3e}")
        assert bool((err <= bound).all())
        assert bool((buf[(N + 1) * D:] == -3.0).all())
        empty = 5 if B > 1 else int((counts == 0).nonzero()[0])
        assert torch.equal(gpos[empty], old[empty] if beta else torch.zeros(D, device=DEV))   # beta * old, exactly
        first = gpos.clone()
        if beta:
            gpos.copy_(old)
        _ops.pos_grad_gather(dx, invd, K, gpos, beta=beta)
        assert torch.equal(gpos, first)                     # bitwise repeatable


# ---- the engine's embedding -----------------------------------------------------------------------------------------
def _ocfg(D, H, B, img):
    ocfg = O.make_config("micro", img=img, batch=B, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = D, H
    return ocfg


def _model(ocfg, st, dtype=torch.float32, **kw):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype, **kw)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st)
    return m.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_gathered_embed_is_the_dense_rows(dtype):
    ocfg = _ocfg(192, 3, 4, 96)
    B, N, D = ocfg.batch_size, ocfg.num_patches, ocfg.embedding_size
    m = _model(ocfg, O.init_state(ocfg, seed=3), dtype)
    eng = m.hip_engine
    eng.ensure_ready(torch.device(DEV, torch.cuda.current_device()))
    x = O.synthetic_batch(ocfg)[0].to(DEV)

    def embed(idx):
        K = N if idx is None else idx.shape[1]
        cols = torch.empty(B * K, eng.CPP, dtype=dtype, device=DEV)
        x0 = torch.empty(B * (K + 1), D, dtype=dtype, device=DEV)
        posg = None if idx is None else _ops.gather_pos(eng.params["pos"], idx, N)
        eng._embed(x, cols, x0, 0, B, idx, posg)
        return x0.view(B, K + 1, D), cols

    dense, dcols = embed(None)
    every = torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    same, scols = embed(every)
    assert torch.equal(same, dense) and torch.equal(scols, dcols)
    idx = _cpu.patch_keep_table(BASE_SEED, 2, B, N, 27)[0].to(DEV)
    sub, _ = embed(idx)
    rows = torch.cat([idx.long(), torch.full((B, 1), N, device=DEV)], dim=1)
    assert torch.equal(sub, dense.gather(1, rows[:, :, None].expand(-1, -1, D)))
    # per chain of the two-stream forward: images 2 .. 3 alone, into their rows
    K = 27
    cols = torch.zeros(B * K, eng.CPP, dtype=dtype, device=DEV)
    x0 = torch.zeros(B * (K + 1), D, dtype=dtype, device=DEV)
    eng._embed(x, cols, x0, 2, 2, idx, _ops.gather_pos(eng.params["pos"], idx, N))
    assert torch.equal(x0.view(B, K + 1, D)[2:], sub[2:]) and not bool(x0.view(B, K + 1, D)[:2].any())


def test_module_patch_embed_keep_names_the_engine():
    w, b = torch.randn(8, 3, 4, 4, device=DEV), torch.randn(8, device=DEV)
    cls, pos = torch.randn(2, 1, 8, device=DEV), torch.randn(1, 5, 8, device=DEV)
    x = torch.randn(2, 3, 8, 8, device=DEV)
    with pytest.raises(NotImplementedError, match="engine"):
        _functional.patch_embed(x, w, b, cls, pos, 4, torch.float32, keep=torch.zeros(2, 1, dtype=torch.int64, device=DEV))
    assert _functional.patch_embed(x, w, b, cls, pos, 4, torch.float32).shape == (2, 5, 8)


# ---- the model against the oracle -----------------------------------------------------------------------------------
# (name, image size, batch, rate): ViT-Tiny width (D 192, 3 heads of 64), 2 blocks
SHAPES = {"t9": (64, 4, 0.5),          # N 16, K 8, T' 9: one chain
          "t28": (96, 8, 0.25)}        # N 36, K 27, T' 28, B 8: the two-chain forward (4 * 28 rows per chain)
PATH_RATES = [0.0, 0.1]
_REF = {}


def _setup(shape):
    img, B, rate = SHAPES[shape]
    key = ("setup", shape)
    if key not in _REF:
        ocfg = _ocfg(192, 3, B, img)
        x, y = O.synthetic_batch(ocfg)
        _REF[key] = dict(ocfg=ocfg, st=O.init_state(ocfg, seed=4), x=x, y=y, rate=rate,
                         K=config.patch_keep_count(ocfg.num_patches, rate))
    return _REF[key]


def _table(shape, variant):
    """The keep table of a variant: the one the forward draws under torch.manual_seed(42), or the caller's own."""
    s = _setup(shape)
    o = s["ocfg"]
    seed = 1234 if variant == "explicit" else BASE_SEED
    return _cpu.patch_keep_table(seed, o.num_blocks, o.batch_size, o.num_patches, s["K"])[0]


def _reference(shape, variant, bf16):
    """The oracle runs of (shape, variant), computed once and never modified: fp32, and with bf16 storage rounding."""
    key = (shape, variant, bf16)
    if key not in _REF:
        s = _setup(shape)
        o = s["ocfg"]
        idx = _table(shape, variant)
        masks = None
        if variant == "explicit":                          # ... which also runs with drop path 0.1 on
            B, T, D = o.batch_size, s["K"] + 1, o.embedding_size
            masks = {}
            for l, p in enumerate(PATH_RATES):
                for site in (0, 1):
                    pk = _engine.path_keep(BASE_SEED, o.num_blocks, l, site, B, p)
                    dk = O.dropout_keep(O.site_seed(BASE_SEED, l, site), (B, T, D))
                    masks[(l, site)] = (dk & pk[:, None, None]).float() / (1.0 - p)
        _REF[key] = oracle_run(s["st"], s["x"], s["y"], o, idx, masks=masks, bf16=bf16)
    return _REF[key]


def _step(m, x, y, between=None, zero=True, **fwd):
    torch.manual_seed(42)
    drawn = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    assert drawn == BASE_SEED, f"torch.manual_seed(42) makes the forward draw {drawn}, the references are BASE_SEED's"
    torch.manual_seed(42)
    xin = x.to(DEV).requires_grad_(True)
    logits = m(xin, **fwd)
    loss = cross_entropy(logits, y.to(DEV))
    if between is not None:
        between()
    loss.backward()
    grads = {k: p.grad.detach().clone().cpu() for k, p in m.named_parameters()}
    if zero:
        m.zero_grad(set_to_none=True)
    return logits.detach().cpu(), loss.detach().cpu(), grads, xin.grad.cpu()


@pytest.mark.parametrize("variant", ["drawn", "drawn_noprune", "explicit"])
@pytest.mark.parametrize("shape", ["t9", "t28"])
@pytest.mark.parametrize("bf16", [False, True])
def test_model_vs_oracle(bf16, shape, variant):
    """Logits, loss and every gradient (pos, cls, conv_w, conv_b and the input image's included) of a training step on
    the kept tokens, at the model gates of tests/test_gpu_drop_path.py.  `drawn`: the table vit_patch_keep draws, read
    back from model.last_patch_keep; `drawn_noprune`: with the last block on every row; `explicit`: a table passed
    as keep_indices (int64), with drop path 0.1 on."""
    s = _setup(shape)
    o, x, y = s["ocfg"], s["x"], s["y"]
    dtype = torch.bfloat16 if bf16 else torch.float32
    idx = _table(shape, variant)
    fwd = {}
    if variant == "explicit":
        m = _model(o, s["st"], dtype).train()              # rate 0: the table alone turns the subset on
        m.drop_path_rates = PATH_RATES
        fwd = dict(keep_indices=idx.long().to(DEV))
    else:
        m = _model(o, s["st"], dtype, patch_drop_rate=s["rate"]).train()
    eng = m.hip_engine
    eng.prune_last = variant != "drawn_noprune"
    split0 = eng.stats["split_forwards"]
    got = _step(m, x, y, **fwd)
    # the two-chain forward ran exactly where its condition holds at T' (B 8: two chains of 4 images x 28 rows)
    assert eng.stats["split_forwards"] - split0 == (1 if shape == "t28" else 0)
    keep = m.last_patch_keep
    assert keep.is_cuda and keep.dtype == torch.int32 and torch.equal(keep.cpu(), idx)
    what = f"{shape} {variant}"
    if bf16:
        check_bf16(got, _reference(shape, variant, True), _reference(shape, variant, False), what)
    else:
        check_fp32(got, _reference(shape, variant, False), what)
    # dropped patches get no image gradient
    P, B, N = o.patch_size, o.batch_size, o.num_patches
    g = got[3].float().reshape(B, 3, o.img_size // P, P, o.img_size // P, P).abs().amax(dim=(1, 3, 5)).reshape(B, N)
    kept = torch.zeros(B, N, dtype=torch.bool).scatter_(1, idx.long(), True)
    assert bool((g[~kept] == 0).all()) and bool((g[kept] > 0).all())
    if variant == "drawn" and not bf16:
        # one chain gives the two chains' bits
        eng.fwd_streams = 1
        again = _step(m, x, y)
        assert torch.equal(again[0], got[0]) and all(torch.equal(again[2][k], got[2][k]) for k in got[2])
        assert torch.equal(again[3], got[3])


def test_probs_are_of_the_kept_tokens():
    s = _setup("t9")
    m = _model(s["ocfg"], s["st"], patch_drop_rate=0.5).train()
    m.store_attention_probs = True
    with torch.no_grad():
        m(s["x"].to(DEV))
    T = s["K"] + 1
    p = m.transformer_encoder.blocks[0].multi_head.attention_probs
    assert tuple(p.shape) == (4, 3, T, T)
    assert float((p.sum(-1) - 1).abs().max()) < 1e-5


# ---- behaviour ------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
            and torch.equal(a[3], b[3]))


def test_backward_uses_the_tapes_table():
    s = _setup("t9")
    m = _model(s["ocfg"], s["st"], patch_drop_rate=0.5).train()
    want = _step(m, s["x"], s["y"])

    def change():
        m.patch_drop_rate = 0.75

    got = _step(m, s["x"], s["y"], between=change)
    assert m.patch_drop_rate == 0.75 and _same(got, want)
    # ... and the next forward runs at the new rate
    _step(m, s["x"], s["y"])
    assert m.last_patch_keep.shape == (4, 4)


def test_gradient_accumulation_over_two_tables():
    """Two backwards with different tables (K 8, then K 4) into the same .grad equal the sum of the two.  Each
    accumulating kernel forms old + increment in one rounding where the separate run rounds the increment first, so an
    element may differ by an ulp of its size: 2^-22 of |g1| + |g2| bounds it."""
    s = _setup("t9")
    o = s["ocfg"]
    m = _model(o, s["st"]).train()
    t1 = _cpu.patch_keep_table(1, 2, 4, 16, 8)[0].to(DEV)
    t2 = _cpu.patch_keep_table(2, 2, 4, 16, 4)[0].to(DEV)
    g1 = _step(m, s["x"], s["y"], keep_indices=t1)[2]
    g2 = _step(m, s["x"], s["y"], keep_indices=t2)[2]
    _step(m, s["x"], s["y"], zero=False, keep_indices=t1)
    acc = _step(m, s["x"], s["y"], zero=False, keep_indices=t2)[2]
    worst = 0.0
    for k in g1:
        err = (acc[k].double() - (g1[k].double() + g2[k].double())).abs()
        bound = 2.0 ** -22 * (g1[k].abs() + g2[k].abs()).double() + 1e-30
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
    print(f"accumulation: worst error {worst:.3f} of the bound")
    pos = acc["emdeddings.pos_embd"][0]
    assert bool((pos[0] != 0).any()) and bool((pos[16] != 0).any())     # patch 0 and CLS: kept by every image


def test_rate_zero_and_eval_are_the_model_without_the_keyword():
    s = _setup("t28")
    o, x, y, st = s["ocfg"], s["x"], s["y"], s["st"]
    plain, zero, on = _model(o, st), _model(o, st, patch_drop_rate=0.0), _model(o, st, patch_drop_rate=0.5)
    # eval: a model with a rate > 0 is the plain model
    assert _same(_step(on.eval(), x, y), _step(plain.eval(), x, y))
    with torch.no_grad():
        assert torch.equal(on(x.to(DEV)), plain(x.to(DEV)))
    # train, rate 0: the model built without the keyword under the same seed, launch for launch
    launches = {}
    for name, m in (("plain", plain), ("zero", zero)):
        _step(m.train(), x, y)                              # (the first step of a model also packs its shadows)
        log, real = [], _ops._lib.call
        _ops._lib.call = lambda n, *a, log=log, real=real: (log.append(n), real(n, *a))[1]
        try:
            launches[name] = (_step(m.train(), x, y), log)
        finally:
            _ops._lib.call = real
    assert _same(launches["zero"][0], launches["plain"][0])
    assert launches["zero"][1] == launches["plain"][1] and len(launches["plain"][1]) > 10
    assert not any("gather" in n or "scatter" in n or n == "vit_patch_keep" for n in launches["zero"][1])
    assert zero.last_patch_keep is None
    # ... while a rate > 0 changes the training forward, also without a tape
    c = _step(on.train(), x, y)
    assert c[0].shape == launches["plain"][0][0].shape and not torch.equal(c[0], launches["plain"][0][0])
    with torch.no_grad():
        torch.manual_seed(42)
        assert torch.equal(on(x.to(DEV)).cpu(), c[0])
    # refusals: a table in eval mode, a wrong shape, a wrong dtype, a host table
    on.eval()
    with pytest.raises(ValueError, match="training-only"):
        on(x.to(DEV), keep_indices=torch.zeros(8, 1, dtype=torch.int64, device=DEV))
    on.train()
    for bad, exc in ((torch.zeros(8, 1, device=DEV), TypeError), (torch.zeros(7, 1, dtype=torch.int64, device=DEV), ValueError),
                     (torch.zeros(8, 37, dtype=torch.int64, device=DEV), ValueError),
                     (torch.zeros(8, 1, dtype=torch.int64), ValueError)):
        with pytest.raises(exc, match="keep"):
            on(x.to(DEV), keep_indices=bad)


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-transformer_amd")]
    import torch.distributed as dist
    from VisionTransformer import config, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, patch_drop_rate=0.5)
    m = vit.VisionTransformer(cfg).cuda().train().enable_data_parallel()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(100 + rank)
    x, y = torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)
    loss = cross_entropy(m(x.cuda()), y.cuda())
    table = m.last_patch_keep.cpu().numpy()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    q.put((rank, table, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_different_tables_and_agree_on_the_weights():
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1].shape == res[1][1].shape == (4, 8)
    assert not np.array_equal(res[0][1], res[1][1])                      # each rank its own table
    assert all(np.array_equal(res[0][2][k], res[1][2][k]) for k in res[0][2])     # bitwise-equal weights after the step


# ---- the attention kernels at the token counts the feature introduces -----------------------------------------------
@pytest.mark.parametrize("T", [50, 99, 148, 289])
def test_attention_at_patch_drop_token_counts(T):
    """attn_fwd / attn_bwd in bf16 at hd 64 against fp64 at tests/test_gpu_kernels.py's attention gates: T' of
    ViT-B/16 224 at rates 0.75 / 0.5 / 0.25 and of 384 at 0.5.  These pass without the feature; they pin the shapes
    it now depends on."""
    import test_gpu_kernels as TK
    torch.manual_seed(T + 64)
    B, H, hd = 2, 2, 64
    D = H * hd
    scale = hd ** 0.5
    qkv = (torch.randn(B * T, 3 * D, device=DEV) * 0.15).to(torch.bfloat16)
    o32 = torch.empty(B * T, D, device=DEV) if _ops.attn_bwd_uses_o32(B, T, H, hd, torch.bfloat16) else None
    o, lse = _ops.attn_fwd(qkv, B, T, H, hd, scale, o32=o32)
    q, k, v = qkv.double().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    s64 = (q @ k.transpose(-1, -2)) * scale
    o_ref = (torch.softmax(s64, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, D)
    lse_ref = torch.logsumexp(s64, -1)
    assert (o.double() - o_ref).abs().max().item() <= 2e-2 * max(1.0, o_ref.abs().max().item())
    assert (lse.double() - lse_ref).abs().max().item() <= 1e-3 * max(1.0, lse_ref.abs().max().item())
    d_o = torch.randn(B * T, D, device=DEV).to(torch.bfloat16)
    dqkv = _ops.attn_bwd(qkv, o, d_o, lse, B, T, H, hd, scale, o32=o32)
    TK._check_attn_bwd_bf16(dqkv, TK._attn_flash_grads(qkv, d_o, B, T, H, hd, scale), D)


# ---- train() --------------------------------------------------------------------------------------------------------
def test_train_patch_drop_checkpoint_and_resume(tmp_path):
    """Three steps of train() on ViT-Tiny width with patch dropout 0.5, a checkpoint, and a resumed run."""
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    cfg = config.ViTConfig(3, 10, 16, 192, 16, 3, 2, "cpu", 4, precision=torch.bfloat16, patch_drop_rate=0.5)
    ds = T.SyntheticImages(12, 3, 64, 10, seed=3)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True)
    ck, logs = str(tmp_path / "ck"), str(tmp_path / "logs")
    tables = []
    real = _ops.patch_keep
    _ops.patch_keep = lambda *a, **k: (tables.append(a[1:5]), real(*a, **k))[1]
    try:
        l0 = T.train(cfg, loader, loader, epochs=0, eval_iter=1, log_dir=logs, checkpoint_dir=ck, lr=1e-3)
        assert len(tables) == 3 and all(t == (2, 4, 16, 8) for t in tables)      # training forwards only
        assert torch.isfinite(torch.tensor(l0)) and T.search_checkpoint(ck) == 0
        ckpt = torch.load(os.path.join(ck, "0.pt"), weights_only=True)
        assert ckpt["step"] == 3
        assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
        l1 = T.train(cfg, loader, loader, epochs=0, eval_iter=1, log_dir=logs, checkpoint_dir=ck, lr=1e-3)
        assert torch.load(os.path.join(ck, "0.pt"), weights_only=True)["step"] == 6 and len(tables) == 6
        assert torch.isfinite(torch.tensor(l1))
    finally:
        _ops.patch_keep = real
