"""GPU tests of the weight EMA kept inside the fused AdamW step (include/vit_hip.h "Weight EMA"): vit_adamw_ema leaves
p / m / v / shadows bitwise those of vit_adamw and vit_adamw_clipped, its EMA against fp64, the skipped step, the swap
kernel, FusedAdamW(ema_decay=...) over param groups and state dicts, the fused engine evaluating the swapped-in EMA
with no repack, and train()'s checkpoint key."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops, config, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -777.0
PAD = 5                                    # sentinel elements behind every buffer
SHAPES = [(1,), (300,), (8193,), (128, 64), (7,)]      # tests/test_gpu_grad_clip.py's _Set, plus its 7-element tensor
NO_SHADOW, NO_EMA, VIEW = 1, 3, 4         # the (300,) entry has a NULL shadow, (128, 64) a NULL EMA pointer; the
BF = torch.bfloat16                        # 7-element entry's EMA is a view 4 bytes into a larger buffer
LR, WD = 1e-3, 1e-4
# One EMA update e + w * (p - e) in fp32 with w = fl32(1 - decay) <= 0.5: the rounding of w (w * 2^-24 relative, on a
# product of at most w * 2M), the subtraction (2^-24 * 2M), the product (2^-24 * 2wM) and the sum (2^-24 * M) stay
# below (1 + 6w) * 2^-24 * M <= 2^-22 * M with M = max(|e_prev|, |p_new|).
GATE = 2.0 ** -22


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    """Bitwise equality of two tensor lists."""
    return len(a) == len(b) and all(torch.equal(_bits(x.detach()), _bits(y.detach())) for x, y in zip(a, b))


class _Set:
    """p / g / m / v / shadow / EMA tensors of SHAPES, each the head of its own buffer with PAD sentinels behind it,
    their chunk table and EMA pointer array, and the norm pass's partial / clip buffers."""

    def __init__(self, seed, sdt=BF):
        gen = torch.Generator().manual_seed(seed)
        self.tails = []

        def guarded(shape, values, dtype=torch.float32):
            n = values.numel()
            buf = torch.full((n + PAD,), SENTINEL, dtype=dtype, device=DEV)
            buf[:n] = values.reshape(-1).to(DEV, dtype)
            self.tails.append(buf[n:])
            return buf[:n].view(shape)

        rnd = lambda s, scale=1.0: torch.randn(s, generator=gen) * scale
        self.sdt = sdt
        self.ps = [guarded(s, rnd(s)) for s in SHAPES]
        self.gs = [guarded(s, rnd(s)) for s in SHAPES]
        self.ms = [guarded(s, rnd(s, 0.1)) for s in SHAPES]
        self.vs = [guarded(s, rnd(s).square() * 0.01) for s in SHAPES]
        # shadows as a pack leaves them; the NULL-EMA entry's holds sentinels, so a swap that wrote it would show
        self.sh = [None if i == NO_SHADOW else
                   guarded(s, torch.full(s, SENTINEL) if i == NO_EMA else p.cpu().to(sdt).float(), sdt)
                   for i, (s, p) in enumerate(zip(SHAPES, self.ps))]
        self.emas = [guarded(s, rnd(s)) for s in SHAPES[:VIEW]]
        self.ebuf = torch.full((64,), SENTINEL, device=DEV)
        self.ebuf[1:8] = rnd((7,)).to(DEV)
        self.emas.append(self.ebuf[1:8])
        assert self.emas[VIEW].data_ptr() % 16 == 4
        self.tails += [self.ebuf[:1], self.ebuf[8:]]
        self.unused = self.emas[NO_EMA]                 # a buffer the table never points at: all sentinels
        self.unused.fill_(SENTINEL)
        self.emas[NO_EMA] = None
        self.table, self.n = _ops.build_chunk_table(list(zip(self.ps, self.gs, self.ms, self.vs, self.sh)), DEV)
        self.ema_dev, n = _ops.build_ema_pointers(list(zip(self.ps, self.emas)), DEV)
        assert n == self.n == sum(-(-p.numel() // _ops.CHUNK) for p in self.ps)
        assert _ops.CHUNK < 8193 <= 2 * _ops.CHUNK
        assert int((self.ema_dev == 0).sum()) == 1 and self.ema_dev.dtype == torch.int64
        self.partial = torch.empty(self.n, dtype=torch.float64, device=DEV)
        self.clip = torch.zeros(4, device=DEV)

    def norm_pass(self, max_norm):
        _ops.grad_sumsq(self.table, self.n, 1.0, self.partial)
        _ops.grad_clip_finish(self.partial, self.n, max_norm, self.clip)

    def ref_norm(self):
        return float(torch.sqrt(sum(g.double().pow(2).sum() for g in self.gs)))

    def step(self, t, decay=None, clip=False):
        adam = (LR, 0.9, 0.999, 1e-8, WD, 1 - 0.9 ** t, 1 - 0.999 ** t, 1.0, self.sdt)
        if decay is None:
            _ops.adamw(self.table, self.n, *adam, clip=self.clip if clip else None)
        else:
            _ops.adamw_ema(self.table, self.ema_dev, self.n, *adam, decay, clip=self.clip if clip else None)

    def adam_state(self):
        return [t.clone() for ts in (self.ps, self.ms, self.vs, [s for s in self.sh if s is not None]) for t in ts]

    def ema_state(self):
        return [e.clone() for e in self.emas if e is not None]

    def intact(self):
        """Every sentinel behind (and, for the view, before) a buffer, and the buffer no pointer names."""
        return all(bool((t == SENTINEL).all()) for t in self.tails + [self.unused])


@pytest.mark.parametrize("clipped", [False, True], ids=["vit_adamw", "vit_adamw_clipped"])
def test_update_leaves_adamw_alone(clipped):
    a, b = _Set(31), _Set(31)
    assert _same(a.adam_state(), b.adam_state())
    max_norm = 0.5 * a.ref_norm()                      # every step clips
    for t in range(1, 4):
        if clipped:
            a.norm_pass(max_norm)
            b.norm_pass(max_norm)
            assert 0.49 < float(a.clip[1]) < 0.51 and float(a.clip[2]) == 0
        a.step(t, decay=0.9, clip=clipped)
        b.step(t, clip=clipped)                        # the kernel it extends, on a twin set
    assert _same(a.adam_state(), b.adam_state())
    for p, sh in zip(a.ps, a.sh):
        assert sh is None or torch.equal(sh, p.to(BF))
    assert not _same(a.ema_state(), b.ema_state()) and _same(b.ema_state(), _Set(31).ema_state())
    assert a.intact() and b.intact()


@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_ema_values_against_fp64(decay):
    s, again = _Set(32), _Set(32)
    w64 = 1.0 - decay
    worst = 0.0
    for t in range(1, 4):
        e_prev = s.ema_state()
        s.step(t, decay=decay)
        again.step(t, decay=decay)
        p_new = [p for p, e in zip(s.ps, s.emas) if e is not None]      # the kernel's own p_new
        for e, ep, p in zip(s.ema_state(), e_prev, p_new):
            ref = ep.double() + w64 * (p.double() - ep.double())
            big = torch.maximum(ep.abs(), p.abs()).double()
            assert bool((big > 0).all())
            ratio = float(((e.double() - ref).abs() / big).max())
            worst = max(worst, ratio)
            print(f"decay {decay} step {t} shape {tuple(e.shape)}: |e - ref| / max(|e_prev|, |p_new|) <= {ratio:.3e}")
    print(f"decay {decay}: worst |e - ref| / max(|e_prev|, |p_new|) over 3 steps = {worst:.3e} (gate {GATE:.3e})")
    assert worst <= GATE
    assert s.intact()
    # a repeat from the same inputs: bitwise the same
    assert _same(s.ema_state(), again.ema_state()) and _same(s.adam_state(), again.adam_state())


def test_skipped_step_touches_nothing():
    s = _Set(33)
    s.norm_pass(1.0)
    s.step(1, decay=0.9, clip=True)                    # a real step first
    before = s.adam_state() + s.ema_state()
    s.gs[VIEW][5] = float("inf")
    s.norm_pass(1.0)
    s.step(2, decay=0.9, clip=True)
    assert float(s.clip[2]) == 1 and float(s.clip[1]) == 0 and float(s.clip[3]) == 1
    assert _same(s.adam_state() + s.ema_state(), before) and s.intact()
    s.gs[VIEW][5] = 0.25                               # a finite step afterwards moves both, and the counter stays
    s.norm_pass(1.0)
    s.step(2, decay=0.9, clip=True)
    assert float(s.clip[2]) == 0 and float(s.clip[3]) == 1
    moved = [t.clone() for t in s.ps] + s.ema_state()                 # (a bf16 shadow may round to where it was)
    assert all(not torch.equal(x, y) for x, y in zip(moved, before[:len(s.ps)] + before[-len(s.ema_state()):]))
    assert all(bool(torch.isfinite(p).all()) for p in s.ps)


@pytest.mark.parametrize("sdt", [BF, torch.float32], ids=["bf16_shadows", "fp32_shadows"])
def test_swap(sdt):
    s = _Set(34, sdt)
    p0, e0, sh0 = [p.clone() for p in s.ps], s.ema_state(), [None if x is None else x.clone() for x in s.sh]
    _ops.ema_swap(s.table, s.ema_dev, s.n, sdt)
    has = [i for i, e in enumerate(s.emas) if e is not None]
    assert _same([s.ps[i] for i in has], e0)                           # p holds the old EMA bits
    assert _same([s.emas[i] for i in has], [p0[i] for i in has])       # and e the old p bits
    for i in has:
        if s.sh[i] is not None:
            assert torch.equal(s.sh[i], s.ps[i].to(sdt)), i
    assert s.sh[NO_SHADOW] is None
    # the NULL-EMA entry: p and shadow untouched
    assert _same([s.ps[NO_EMA], s.sh[NO_EMA]], [p0[NO_EMA], sh0[NO_EMA]])
    assert bool((s.sh[NO_EMA] == SENTINEL).all()) and s.intact()
    _ops.ema_swap(s.table, s.ema_dev, s.n, sdt)
    assert _same(s.ps, p0) and _same(s.ema_state(), e0) and s.intact()
    assert _same([x for x in s.sh if x is not None], [x for x in sh0 if x is not None])


# ---- FusedAdamW(ema_decay=...) --------------------------------------------------------------------------------------
def _groups(t, extra):
    return [{"params": t[:2] + extra, "lr": 1e-3}, {"params": t[2:], "lr": 3e-3}]


def _params(seed, shapes=SHAPES[:4]):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)


def test_optimizer_two_groups_and_a_gradless_parameter():
    ps = _params(35)
    idle = torch.nn.Parameter(torch.randn(50, device=DEV))             # never gets a gradient
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = FusedAdamW(_groups(ps, [idle]), weight_decay=WD, ema_decay=0.9)
    ref = FusedAdamW(_groups(twin, []), weight_decay=WD)
    assert "ema_decay" not in opt.state_dict()["param_groups"][0]
    idle0 = idle.detach().clone()
    # the fp64 recurrence from the initial weights over the kernel's own p_t.  Bound: a step adds at most GATE * M_t
    # of its own rounding (M_t = max(|e_{t-1}|, |p_t|), |e_{t-1}| <= |ref_{t-1}| + bound_{t-1}) and carries the error
    # it inherited forward times (1 - w) < 1:  bound_t = (1 - w) * bound_{t-1} + GATE * (M_t + bound_{t-1}).
    w64 = 1.0 - 0.9
    refs = [p.detach().double() for p in ps]
    bound = [torch.zeros_like(r) for r in refs]
    for t in range(3):
        _set_grads(ps, 100 + t)
        _set_grads(twin, 100 + t)
        opt.step()
        ref.step()
        for i, p in enumerate(ps):
            big = torch.maximum(refs[i].abs(), p.detach().double().abs())
            bound[i] = (1 - w64) * bound[i] + GATE * (big + bound[i])
            refs[i] = refs[i] + w64 * (p.detach().double() - refs[i])
    assert _same(ps, twin)                                               # the EMA leaves the update alone
    worst = 0.0
    for p, r, b in zip(ps, refs, bound):
        e = opt.state[p]["ema"]
        assert e.dtype == torch.float32 and e.is_contiguous() and e.shape == p.shape
        err = (e.double() - r).abs()
        worst = max(worst, float((err / b).max()))
        assert bool((err <= b).all())
        assert not torch.equal(e, p.detach())
    print(f"EMA after 3 steps vs the fp64 recurrence: worst error / compounded bound = {worst:.3f}")
    assert torch.equal(idle, idle0) and not opt.state.get(idle)          # untouched: no moments, no EMA
    assert all("ema" not in ref.state[q] for q in twin)


def test_optimizer_state_dict_interchanges_with_torch_adamw():
    ps = _params(36)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = FusedAdamW(_groups(ps, []), weight_decay=WD, ema_decay=0.9)
    ref = FusedAdamW(_groups(twin, []), weight_decay=WD)
    for t in range(2):
        _set_grads(ps, 200 + t)
        _set_grads(twin, 200 + t)
        opt.step()
        ref.step()
    emas = [opt.state[p]["ema"].clone() for p in ps]
    t_opt = torch.optim.AdamW(_groups(ps, []), weight_decay=WD)
    t_opt.load_state_dict(opt.state_dict())                              # torch carries the unknown key along
    assert _same([t_opt.state[p]["ema"] for p in ps], emas)
    back = FusedAdamW(_groups(ps, []), weight_decay=WD, ema_decay=0.9)
    back.load_state_dict(t_opt.state_dict())
    assert _same([back.state[p]["ema"] for p in ps], emas)
    _set_grads(ps, 202)
    _set_grads(twin, 202)
    back.step()
    ref.step()
    assert _same(ps, twin)                                               # moments and step counts came along too
    for p, e_prev in zip(ps, emas):
        r = e_prev.double() + 0.1 * (p.detach().double() - e_prev.double())
        big = torch.maximum(e_prev.abs(), p.detach().abs()).double()
        assert bool(((back.state[p]["ema"].double() - r).abs() <= GATE * big).all())


def test_optimizer_loading_a_state_without_ema_clones_the_weights():
    ps = _params(37)
    plain = torch.optim.AdamW(_groups(ps, []), weight_decay=WD)
    _set_grads(ps, 300)
    plain.step()
    late = FusedAdamW(_groups(ps, []), weight_decay=WD, ema_decay=0.9)
    late.load_state_dict(plain.state_dict())
    assert all("ema" not in late.state[p] for p in ps)
    before = [p.detach().clone() for p in ps]
    _set_grads(ps, 301)
    late.step()
    for p, b in zip(ps, before):
        r = b.double() + 0.1 * (p.detach().double() - b.double())
        big = torch.maximum(b.abs(), p.detach().abs()).double()
        assert bool(((late.state[p]["ema"].double() - r).abs() <= GATE * big).all())
        assert not torch.equal(p.detach(), b)


def test_optimizer_swap_context():
    ps = _params(38)
    idle = torch.nn.Parameter(torch.randn(50, device=DEV))
    opt = FusedAdamW(_groups(ps, [idle]), weight_decay=WD, ema_decay=0.9)
    for t in range(2):
        _set_grads(ps, 400 + t)
        opt.step()
    opt.zero_grad(set_to_none=True)                                      # the swap needs no gradient
    p0, e0, idle0 = [p.detach().clone() for p in ps], [opt.state[p]["ema"].clone() for p in ps], idle.detach().clone()
    with opt.ema_weights():
        assert _same(ps, e0) and _same([opt.state[p]["ema"] for p in ps], p0) and torch.equal(idle, idle0)
        _set_grads(ps, 402)
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
        with pytest.raises(RuntimeError, match="already swapped in"):
            with opt.ema_weights():
                pass
        inside = opt.ema_state_dict(torch.nn.ParameterList(ps))
    assert _same(ps, p0) and _same([opt.state[p]["ema"] for p in ps], e0)
    with pytest.raises(KeyError, match="boom"):
        with opt.ema_weights():
            raise KeyError("boom")
    assert _same(ps, p0) and _same([opt.state[p]["ema"] for p in ps], e0)   # an exception still swaps back
    esd = opt.ema_state_dict(torch.nn.ParameterList(ps))
    assert _same(list(esd.values()), e0) and _same(list(inside.values()), e0)
    assert not opt.state.get(idle)                                       # looking for EMAs made no state for it
    opt.step()                                                           # and the optimizer steps again


def test_plain_step_never_reaches_the_ema_entry_points(monkeypatch):
    """ema_decay=None: the step launches through _ops.adamw exactly as before, and builds no EMA pointer array."""
    def refuse(*a, **k):
        raise AssertionError("an EMA entry point was reached without ema_decay")
    monkeypatch.setattr(_ops, "adamw_ema", refuse)
    monkeypatch.setattr(_ops, "build_ema_pointers", refuse)
    ps = _params(39)
    for kw in ({}, {"max_grad_norm": 1.0}):
        opt = FusedAdamW(ps, lr=LR, **kw)
        for t in range(2):
            _set_grads(ps, 500 + t)
            opt.step()
        assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} for p in ps)


# ---- through the fused engine ---------------------------------------------------------------------------------------
def _train_step(m, opt, x, y, seed):
    m.train()
    torch.manual_seed(seed)                                              # the same dropout draw on both twins
    opt.zero_grad(set_to_none=True)
    cross_entropy(m(x), y).backward()
    opt.step()


def _eval_logits(m, x):
    m.eval()
    with torch.no_grad():
        return m(x).clone()


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_engine_evaluates_the_swapped_in_ema_without_a_repack(dtype):
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 8, precision=dtype)      # D128 H2 (hd 64) L2, T = 17
    torch.manual_seed(0)
    m = vit.VisionTransformer(cfg).to(DEV)
    torch.manual_seed(0)
    twin = vit.VisionTransformer(cfg).to(DEV)
    g = torch.Generator().manual_seed(40)
    x, y = torch.randn(8, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV)
    opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-2, ema_decay=0.9)
    ref = FusedAdamW(twin.parameters(), lr=1e-2, weight_decay=1e-2)
    for i in range(3):
        _train_step(m, opt, x, y, 10 + i)
        _train_step(twin, ref, x, y, 10 + i)
    assert _same(list(m.parameters()), list(twin.parameters()))
    # the yardstick of tests/test_gpu_weight_coherence.py: a fresh model, a new engine, a new pack
    F = vit.VisionTransformer(m.vit_config)
    F.load_state_dict(opt.ema_state_dict(m))
    want = _eval_logits(F.to(DEV), x)
    eng = m.hip_engine
    before = _eval_logits(m, x)
    packs, G, W = eng.stats["packs"], eng.G, eng.W
    with opt.ema_weights():
        inside = _eval_logits(m, x)
        assert eng.stats["packs"] == packs
    assert torch.equal(inside, want) and not torch.equal(inside, before)
    after = _eval_logits(m, x)
    assert torch.equal(after, before)
    assert eng.stats["packs"] == packs and eng.G is G and eng.W is W and m.hip_engine is eng
    _train_step(m, opt, x, y, 13)                                        # a further step equals the twin's
    _train_step(twin, ref, x, y, 13)
    assert _same(list(m.parameters()), list(twin.parameters()))
    assert eng.stats["packs"] == packs


def test_train_saves_the_ema(tmp_path, monkeypatch):
    """train(..., ema_decay=...) on the device: "ema_state_dict" in the checkpoint, different from the trained weights
    and equal to what the restored optimizer state gives; without the keyword the key set is unchanged."""
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, precision=BF)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(12, 3, 64, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(4, 3, 64, 10, seed=4), batch_size=4)

    def run(name, **kw):
        T.train(cfg, loader, test_loader, epochs=0, eval_iter=1, log_dir=str(tmp_path / name),
                checkpoint_dir=str(tmp_path / (name + "_ck")), lr=1e-3, **kw)
        return torch.load(tmp_path / (name + "_ck") / "0.pt", map_location="cpu", weights_only=True)

    plain = run("plain")
    assert set(plain) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
    ck = run("ema", ema_decay=0.9)
    assert set(ck) == set(plain) | {"ema_state_dict"}
    msd, esd = ck["model_state_dict"], ck["ema_state_dict"]
    assert list(esd) == list(msd)
    assert all(not torch.equal(esd[k], msd[k]) for k in msd if msd[k].numel() > 1)
    model = vit.VisionTransformer(cfg)
    model.load_state_dict(msd)
    model = model.to(DEV)
    opt = make_optimizer(model.parameters(), lr=1e-3, weight_decay=1e-4, device=DEV, ema_decay=0.9)
    opt.load_state_dict(ck["optimizer_state_dict"])                      # resume: the EMA rides in the optimizer state
    again = opt.ema_state_dict(model)
    assert all(torch.equal(again[k].cpu(), esd[k]) for k in esd)
