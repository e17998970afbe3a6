"""GPU tests of LAMB in the fused optimizer step (include/vit_hip.h "LAMB"): vit_lamb_moments / vit_lamb_trust /
vit_lamb_update against the formulas in fp64 from the kernels' own fp32 inputs, bitwise repeatability, shadows,
sentinels, the flags, clip and skip, the EMA, FusedLamb over param groups, step counts and state dicts, the fused
engine, two data-parallel ranks, and train(opt="lamb")."""
import math
import os
import socket
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops, config, vit
    from VisionTransformer._engine import shadow_of
    from VisionTransformer.optim import (FusedAdamW, FusedLamb, Lamb, cross_entropy, make_optimizer,
                                         param_groups_weight_decay)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -777.0
PAD = 5                                    # sentinel elements behind every buffer
BF = torch.bfloat16
# tests/test_gpu_ema.py's SHAPES (the 7-element entry's gradient and EMA are views 4 bytes into larger buffers), an
# all-zero weight tensor, and 19,200 elements: 300 chunks of 64, more than the 256 threads of the per-tensor finish
SHAPES = [(1,), (300,), (8193,), (128, 64), (7,), (33,), (19200,)]
NO_SHADOW, NO_EMA, VIEW, ZERO, LONG = 1, 3, 4, 5, 6
BIG, SMALL = 1, 2                          # weights scaled by 10 and by 0.1: ratios above and below 1
LR, WD, B1, B2, EPS = 1e-2, 0.05, 0.9, 0.999, 1e-6
U = 2.0 ** -24
# the norm tests' bound (tests/test_gpu_grad_clip.py NORM_RTOL): the sums are fp64, so what is left is fp32 roundings
RATIO_RTOL = 2.0 ** -22
# p_new = fma(-(lr * r), u, p) with u = fma(wd, p, m / fma(sqrt(v), c1, c2)), c1 = fl(bc1 / sqrt(bc2)), c2 = fl(bc1 * eps).
# Roundings, each at most U = 2^-24 relative:
#   u:  c1, c2, sqrt, the inner fma, the quotient, the outer fma                          6, relative to |u|
#   r:  the 6 of u carry into |u| (the fp64 sums add ~1e-13), the cast of the quotient     7
#   lr * r                                                                                  1
#   the last fma rounds a result of at most |p_old| + |lr r u| <= 2 M                       2, relative to M
# so |p_new - ref| <= (6 + 7 + 1) U |lr r u| + 2 U M <= 16 U M = 2^-20 M with M = max(|p_old|, |lr r u|).
GATE_P = 2.0 ** -20
GATE_EMA = 2.0 ** -22                      # tests/test_gpu_ema.py GATE, same recurrence
MV_ATOL = 1e-6                             # m and v as the AdamW tests gate their results (tests/test_gpu_kernels.py)


def f32(x):
    """The fp32 value a Python float becomes on its way into an entry point."""
    return float(torch.tensor(x, dtype=torch.float32))


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same(a, b):
    """Bitwise equality of two tensor lists."""
    return len(a) == len(b) and all(torch.equal(_bits(x.detach()), _bits(y.detach())) for x, y in zip(a, b))


def lamb_ref(p_old, m_new, v_new, t, lr, wd, adapt, trust_clip, b1=B1, b2=B2, eps=EPS):
    """The specification in fp64 from fp32 tensors and the fp32 scalars the kernels were handed: (u, r, p_new)."""
    m, v, p = m_new.double(), v_new.double(), p_old.double()
    bc1, bc2 = f32(1 - b1 ** t), f32(1 - b2 ** t)
    u = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + f32(eps)) + f32(wd) * p
    r = 1.0
    if adapt:
        wn, un = float(p.norm()), float(u.norm())
        if wn > 0 and un > 0:
            r = wn / un
    if trust_clip:
        r = min(r, 1.0)
    return u, r, p - f32(lr) * r * u


class _Set:
    """p / g / m / v / shadow / EMA tensors of SHAPES, each the head of its own buffer with PAD sentinels behind it,
    the chunk table, EMA pointers and tensor index, and the partial / trust / clip buffers with sentinels of their own."""

    def __init__(self, seed, sdt=BF):
        gen = torch.Generator().manual_seed(seed)
        self.tails = []

        def guarded(shape, values, dtype=torch.float32, lead=0):
            n = values.numel()
            buf = torch.full((lead + n + PAD,), SENTINEL, dtype=dtype, device=DEV)
            buf[lead:lead + n] = values.reshape(-1).to(DEV, dtype)
            self.tails += [buf[:lead], buf[lead + n:]]
            return buf[lead:lead + n].view(shape)

        def rnd(s, scale=1.0):
            return torch.randn(s, generator=gen) * scale

        self.sdt = sdt
        scale = {BIG: 10.0, SMALL: 0.1, ZERO: 0.0}
        self.ps = [guarded(s, rnd(s, scale.get(i, 1.0))) for i, s in enumerate(SHAPES)]
        self.gs = [guarded(s, rnd(s), lead=int(i == VIEW)) for i, s in enumerate(SHAPES)]
        self.ms = [guarded(s, rnd(s, 0.1)) for s in SHAPES]
        self.vs = [guarded(s, rnd(s).square() * 0.01) for s in SHAPES]
        self.sh = [None if i == NO_SHADOW else guarded(s, p.cpu().to(sdt).float(), sdt)
                   for i, (s, p) in enumerate(zip(SHAPES, self.ps))]
        self.emas = [guarded(s, rnd(s), lead=int(i == VIEW)) for i, s in enumerate(SHAPES)]
        assert self.gs[VIEW].data_ptr() % 16 == 4 and self.emas[VIEW].data_ptr() % 16 == 4
        assert not bool(self.ps[ZERO].any())
        self.unused = self.emas[NO_EMA]                 # a buffer the table never points at: all sentinels
        self.unused.fill_(SENTINEL)
        self.emas[NO_EMA] = None
        entries = list(zip(self.ps, self.gs, self.ms, self.vs, self.sh))
        self.table, self.n = _ops.build_chunk_table(entries, DEV)
        self.ema_dev, n = _ops.build_ema_pointers(list(zip(self.ps, self.emas)), DEV)
        self.first, self.owner, self.nt, n2 = _ops.build_tensor_index(entries, DEV)
        assert n == n2 == self.n == sum(-(-p.numel() // _ops.CHUNK) for p in self.ps) and self.nt == len(SHAPES)
        assert int(self.first[-1]) == self.n and self.owner.numel() == self.n
        self.partial = torch.full((2 * self.n + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
        self.trust = torch.full((self.nt + PAD,), SENTINEL, device=DEV)
        self.clip = torch.full((4 + PAD,), SENTINEL, device=DEV)
        self.clip[:4] = 0
        self.norm_partial = torch.empty(self.n, dtype=torch.float64, device=DEV)
        self.tails += [self.partial[2 * self.n:], self.trust[self.nt:], self.clip[4:]]

    def norm_pass(self, max_norm):
        _ops.grad_sumsq(self.table, self.n, 1.0, self.norm_partial)
        _ops.grad_clip_finish(self.norm_partial, self.n, max_norm, self.clip)

    def ref_norm(self):
        return float(torch.sqrt(sum(g.double().pow(2).sum() for g in self.gs)))

    def step(self, t, wd=WD, adapt=True, trust_clip=False, clip=False, decay=None):
        c = self.clip if clip else None
        bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
        _ops.lamb_moments(self.table, self.n, B1, B2, EPS, wd, bc1, bc2, 1.0, self.partial, clip=c)
        _ops.lamb_trust(self.partial, self.first, self.nt, self.trust, adapt=adapt, trust_clip=trust_clip, clip=c)
        _ops.lamb_update(self.table, self.owner, self.trust, self.n, LR, EPS, wd, bc1, bc2, self.sdt,
                         ema_dev=self.ema_dev if decay is not None else None, ema_decay=decay, clip=c)

    def state(self):
        return [t.clone() for ts in (self.ps, self.ms, self.vs, [s for s in self.sh if s is not None]) for t in ts]

    def ema_state(self):
        return [e.clone() for e in self.emas if e is not None]

    def ratios(self):
        return self.trust[:self.nt].clone()

    def intact(self):
        """Every sentinel behind (and, for the views, before) a buffer, and the buffer no pointer names."""
        return all(bool((t == SENTINEL).all()) for t in self.tails + [self.unused])


def _check_step(s, t, old, wd=WD, adapt=True, trust_clip=False, g_eff=None):
    """One finished step of `s` against fp64: m and v against the recurrence, every ratio and every element of p
    against lamb_ref on the kernel's own m, v and the p it read.  Returns the worst (ratio, p) errors over their gates."""
    p0, m0, v0 = old
    worst_r = worst_p = 0.0
    got_r = s.ratios().tolist()
    for i in range(len(SHAPES)):
        g = (s.gs[i] if g_eff is None else g_eff[i]).double()
        m64 = f32(B1) * m0[i].double() + (1 - f32(B1)) * g
        v64 = f32(B2) * v0[i].double() + (1 - f32(B2)) * g * g
        assert float((s.ms[i].double() - m64).abs().max()) < MV_ATOL, (t, i)
        assert float((s.vs[i].double() - v64).abs().max()) < MV_ATOL, (t, i)
        u, r, p_ref = lamb_ref(p0[i], s.ms[i], s.vs[i], t, LR, wd, adapt, trust_clip)
        worst_r = max(worst_r, abs(got_r[i] - r) / (RATIO_RTOL * r))
        big = torch.maximum(p0[i].double().abs(), (f32(LR) * r * u).abs())
        assert bool((big > 0).all())
        worst_p = max(worst_p, float(((s.ps[i].double() - p_ref).abs() / (GATE_P * big)).max()))
        if s.sh[i] is not None:
            assert torch.equal(s.sh[i], s.ps[i].to(s.sdt)), (t, i)
    return worst_r, worst_p


def _old(s):
    return [p.clone() for p in s.ps], [m.clone() for m in s.ms], [v.clone() for v in s.vs]


@pytest.mark.parametrize("sdt", [BF, torch.float32], ids=["bf16_shadows", "fp32_shadows"])
@pytest.mark.parametrize("chunk", [None, 64], ids=["chunk_default", "chunk_64"])
def test_kernels_against_fp64(monkeypatch, chunk, sdt):
    if chunk is not None:
        monkeypatch.setattr(_ops, "CHUNK", chunk)
    s, again = _Set(51, sdt), _Set(51, sdt)
    per_tensor = (s.first[1:] - s.first[:-1]).tolist()
    if chunk is None:
        assert _ops.CHUNK < 8193 <= 2 * _ops.CHUNK and per_tensor[2] == 2      # two chunks, a one-element tail
    else:
        assert per_tensor[LONG] == 300 and per_tensor[2] == 129
    worst_r = worst_p = 0.0
    for t in range(1, 4):
        old = _old(s)
        s.step(t)
        again.step(t)
        r, p = _check_step(s, t, old)
        worst_r, worst_p = max(worst_r, r), max(worst_p, p)
        ratios = s.ratios()
        assert (float(ratios[ZERO]) == 1.0) == (t == 1)                        # |w| = 0 at step 1 only: then w moves
        assert float(ratios[BIG]) > 1.0 > float(ratios[SMALL]) > 0.0
        # per chunk: partial[2i], partial[2i + 1] are fp64 sums of at most CHUNK squares (two summation orders
        # differ by at most CHUNK * 2^-53 relative)
        p0 = torch.cat([x.reshape(-1)[o:o + _ops.CHUNK].double().pow(2).sum().reshape(1) for x in old[0]
                        for o in range(0, x.numel(), _ops.CHUNK)])
        assert torch.allclose(s.partial[:2 * s.n:2], p0, rtol=1e-12, atol=0)
    print(f"chunk {_ops.CHUNK} {sdt}: worst ratio error / (2^-22 r) = {worst_r:.3f}, worst p error / (2^-20 M) = "
          f"{worst_p:.3f} over 3 steps")
    assert worst_r <= 1.0 and worst_p <= 1.0
    assert s.intact() and again.intact()
    # the same inputs twice: bitwise the same p, m, v, shadows, ratios and partials
    assert _same(s.state(), again.state()) and _same([s.trust, s.partial], [again.trust, again.partial])


def test_chunking_does_not_change_what_a_tensor_is(monkeypatch):
    """The ratio is per tensor, not per chunk: cut at 64 and at the default the ratios agree to fp64 summation order,
    and every chunk of a tensor moves by the same ratio."""
    a = _Set(52)
    a.step(1)
    monkeypatch.setattr(_ops, "CHUNK", 64)
    b = _Set(52)
    b.step(1)
    assert _same(a.ms + a.vs, b.ms + b.vs)
    assert torch.allclose(a.ratios().double(), b.ratios().double(), rtol=2.0 ** -23, atol=0)
    for x, y in zip(a.ps, b.ps):                     # a one-ulp ratio difference moves p by at most an ulp of the step
        assert float((x - y).abs().max()) <= 2.0 ** -22 * max(float(x.abs().max()), LR)


@pytest.mark.parametrize("trust_clip", [False, True], ids=["", "trust_clip"])
@pytest.mark.parametrize("wd,adapt", [(WD, True), (0.0, False), (0.0, True)],
                         ids=["decay", "no_decay", "no_decay_always_adapt"])
def test_flags_follow_the_rule_per_tensor(wd, adapt, trust_clip):
    s = _Set(53)
    old = _old(s)
    s.step(1, wd=wd, adapt=adapt, trust_clip=trust_clip)
    worst_r, worst_p = _check_step(s, 1, old, wd=wd, adapt=adapt, trust_clip=trust_clip)
    assert worst_r <= 1.0 and worst_p <= 1.0
    ratios = s.ratios().tolist()
    if not adapt:
        assert ratios == [1.0] * len(SHAPES)
    else:
        assert ratios[ZERO] == 1.0 and ratios[SMALL] < 0.5
        assert ratios[BIG] == 1.0 if trust_clip else ratios[BIG] > 2.0
        assert all(r <= 1.0 for r in ratios) or not trust_clip
    assert s.intact()


def test_zero_gradient_without_decay_leaves_the_weights_bitwise():
    s = _Set(54)
    for g, m in zip(s.gs, s.ms):
        g.zero_()
        m.zero_()
    before = [p.clone() for p in s.ps]
    s.step(1, wd=0.0, adapt=True)                    # u = 0 everywhere: |u| = 0, r = 1, p - lr * 0
    assert s.ratios().tolist() == [1.0] * len(SHAPES)
    assert _same(s.ps, before) and s.intact()


def test_clip_coefficient_reaches_the_gradient_and_skip_touches_nothing():
    s = _Set(55)
    max_norm = 0.5 * s.ref_norm()
    s.norm_pass(max_norm)
    assert 0.49 < float(s.clip[1]) < 0.51 and float(s.clip[2]) == 0
    old = _old(s)
    s.step(1, clip=True)
    g_eff = [g * (torch.tensor(1.0, device=DEV) * s.clip[1]) for g in s.gs]      # the fp32 products the kernel forms
    worst_r, worst_p = _check_step(s, 1, old, g_eff=g_eff)
    assert worst_r <= 1.0 and worst_p <= 1.0
    raw = f32(B1) * old[1][2].double() + (1 - f32(B1)) * s.gs[2].double()          # not the unclipped gradient's m
    assert float((s.ms[2].double() - raw).abs().max()) > 1e-3
    # a non-finite norm: p, m, v, shadows, the EMA, the trust buffer and the partials stay bitwise what they were
    before = s.state() + s.ema_state() + [s.trust.clone(), s.partial.clone()]
    s.gs[VIEW][5] = float("inf")
    s.norm_pass(max_norm)
    s.step(2, clip=True, decay=0.9)
    assert float(s.clip[2]) == 1 and float(s.clip[1]) == 0 and float(s.clip[3]) == 1
    assert _same(s.state() + s.ema_state() + [s.trust, s.partial], before) and s.intact()
    s.gs[VIEW][5] = 0.25                               # a finite step afterwards moves them again
    s.norm_pass(max_norm)
    s.step(2, clip=True, decay=0.9)
    assert float(s.clip[2]) == 0 and float(s.clip[3]) == 1
    assert all(not torch.equal(x, y) for x, y in zip(s.ps, before[:len(s.ps)]))
    assert all(bool(torch.isfinite(p).all()) for p in s.ps) and s.intact()


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
def test_ema_inside_the_update(clipped):
    a, b = _Set(56), _Set(56)
    max_norm = 0.5 * a.ref_norm()
    worst = 0.0
    for t in range(1, 4):
        if clipped:
            a.norm_pass(max_norm)
            b.norm_pass(max_norm)
        e_prev = a.ema_state()
        a.step(t, clip=clipped, decay=0.9)
        b.step(t, clip=clipped)                        # the EMA-less step on a twin set
        p_new = [p for p, e in zip(a.ps, a.emas) if e is not None]
        for e, ep, p in zip(a.ema_state(), e_prev, p_new):
            ref = ep.double() + (1.0 - 0.9) * (p.double() - ep.double())
            big = torch.maximum(ep.abs(), p.abs()).double()
            worst = max(worst, float(((e.double() - ref).abs() / (GATE_EMA * big)).max()))
    print(f"EMA inside vit_lamb_update: worst error / (2^-22 max(|e_prev|, |p_new|)) = {worst:.3f}")
    assert worst <= 1.0
    assert _same(a.state(), b.state()) and _same([a.trust], [b.trust])          # p, m, v, shadows, ratios: bitwise
    assert _same(b.ema_state(), _Set(56).ema_state()) and not _same(a.ema_state(), b.ema_state())
    assert a.intact() and b.intact()                   # the NULL-EMA chunk's buffer among them


def test_ops_validate_their_buffers():
    s = _Set(57)
    with pytest.raises(ValueError, match="partial"):
        _ops.lamb_moments(s.table, s.n, B1, B2, EPS, WD, 0.1, 0.001, 1.0, s.partial[:2 * s.n - 1])
    with pytest.raises(ValueError, match="partial"):
        _ops.lamb_moments(s.table, s.n, B1, B2, EPS, WD, 0.1, 0.001, 1.0, s.partial.float())
    with pytest.raises(ValueError, match="tensor_first"):
        _ops.lamb_trust(s.partial, s.first[:-1], s.nt, s.trust)
    with pytest.raises(ValueError, match="trust"):
        _ops.lamb_trust(s.partial, s.first, s.nt, s.trust[:s.nt - 1])
    with pytest.raises(ValueError, match="tensor_of_chunk"):
        _ops.lamb_update(s.table, s.owner.long(), s.trust, s.n, LR, EPS, WD, 0.1, 0.001, BF)
    with pytest.raises(RuntimeError, match="ROCm device"):
        _ops.lamb_trust(s.partial, s.first, s.nt, s.trust.cpu())
    with pytest.raises(RuntimeError, match="bias corrections"):
        _ops.lamb_moments(s.table, s.n, B1, B2, EPS, WD, 0.0, 0.001, 1.0, s.partial)
    assert s.intact()


# ---- FusedLamb ------------------------------------------------------------------------------------------------------
P_SHAPES = [(1,), (300,), (8193,), (128, 64)]
# FusedLamb in fp32 against the host Lamb on fp64 twins fed the same gradients: after k steps the twins' p, m and v
# differ from the device's by the roundings of k updates (at most GATE_P * M each on p), which the ratio inherits
# through both norms; 2^-17 leaves room for three steps of that.  Parameters: 1e-6 absolute, as the AdamW tests gate.
TWIN_RATIO_RTOL, TWIN_ATOL = 2.0 ** -17, 1e-6


def _params(seed, shapes=P_SHAPES):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]


def _twins(ps):
    return [torch.nn.Parameter(p.detach().double()) for p in ps]


def _set_grads(ps, twins, seed, only=None):
    g = torch.Generator().manual_seed(seed)
    for i, (p, q) in enumerate(zip(ps, twins)):
        v = torch.randn(p.shape, generator=g).to(DEV)
        if only is None or i in only:
            p.grad, q.grad = v, v.double()


def _close(opt, ref, ps, twins):
    got, want = opt.trust_ratios(), ref.trust_ratios()
    for p, q in zip(ps, twins):
        assert float((p.detach().double() - q.detach()).abs().max()) < TWIN_ATOL
        if p in got:
            assert q in want and got[p].shape == () and got[p].is_cuda
            assert abs(float(got[p]) - float(want[q])) <= TWIN_RATIO_RTOL * float(want[q])
        else:
            assert q not in want


def test_optimizer_groups_step_counts_and_set_to_none():
    ps = _params(61)
    idle = torch.nn.Parameter(torch.randn(50, device=DEV))             # never gets a gradient
    twins = _twins(ps)
    groups = lambda t, extra: [{"params": t[:2] + extra, "lr": 1e-3, "weight_decay": 0.0},
                               {"params": t[2:], "lr": 3e-3, "weight_decay": 0.05, "trust_clip": True}]
    opt = FusedLamb(groups(ps, [idle]), max_grad_norm=None)
    ref = Lamb(groups(twins, []))
    assert [g["trust_clip"] for g in opt.param_groups] == [False, True]
    idle0 = idle.detach().clone()
    # step 1 reaches only two parameters, so from step 2 on each group holds two step counts: two tables per group
    for k, only in enumerate(([0, 3], None, None)):
        opt.zero_grad(set_to_none=True)
        ref.zero_grad(set_to_none=True)
        _set_grads(ps, twins, 600 + k, only)
        opt.step()
        ref.step()
        _close(opt, ref, ps, twins)
        assert len(opt.trust_ratios()) == (2 if only else 4)
    assert {k[:2] for k in opt._tables} == {(0, "t"), (1, "t")}
    assert len(opt._stepped) == 4 and all(tab.lamb.ntensors == 1 for tab in opt._stepped)
    assert [int(opt.state[p]["step"]) for p in ps] == [3, 2, 2, 3]
    r = opt.trust_ratios()
    assert float(r[ps[0]]) == 1.0 and float(r[ps[1]]) == 1.0           # weight_decay = 0, always_adapt off
    assert float(r[ps[2]]) <= 1.0 and float(r[ps[3]]) <= 1.0           # trust_clip
    assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} for p in ps)
    assert torch.equal(idle, idle0) and not opt.state.get(idle)
    sd = opt.state_dict()["param_groups"]
    assert [g["always_adapt"] for g in sd] == [False, False] and [g["trust_clip"] for g in sd] == [False, True]


def test_optimizer_clip_ema_and_skip():
    ps = _params(62)
    twins = _twins(ps)
    opt = FusedLamb(ps, lr=LR, weight_decay=WD, max_grad_norm=1.0, ema_decay=0.9)
    ref = Lamb(twins, lr=LR, weight_decay=WD, max_grad_norm=1.0, ema_decay=0.9)
    for k in range(2):
        _set_grads(ps, twins, 700 + k)
        opt.step()
        ref.step()
        _close(opt, ref, ps, twins)
        assert abs(float(opt.grad_norm()) - float(ref.grad_norm())) <= 2.0 ** -22 * float(ref.grad_norm())
    for p, q in zip(ps, twins):
        assert float((opt.state[p]["ema"].double() - ref.state[q]["ema"]).abs().max()) < TWIN_ATOL
    before = [t.clone() for p in ps for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"],
                                              opt.state[p]["ema"])]
    ratios = opt.trust_ratios()
    _set_grads(ps, twins, 702)
    ps[1].grad[7] = float("nan")
    opt.step()
    assert float(opt.skipped_steps()) == 1 and not math.isfinite(float(opt.grad_norm()))
    after = [t for p in ps for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"],
                                     opt.state[p]["ema"])]
    assert _same(after, before) and _same(list(opt.trust_ratios().values()), list(ratios.values()))
    assert [int(opt.state[p]["step"]) for p in ps] == [3] * 4           # the documented deviation: the counters advance
    with opt.ema_weights():                            # the inherited swap surface
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()


def test_optimizer_loads_a_torch_adamw_state():
    ps = _params(63)
    torch_opt = torch.optim.AdamW(ps, lr=LR, weight_decay=WD)
    _set_grads(ps, _twins(ps), 800)
    torch_opt.step()
    twins = _twins(ps)
    opt = FusedLamb(ps, lr=LR, weight_decay=WD, trust_clip=True)
    ref = Lamb(twins, lr=LR, weight_decay=WD, trust_clip=True)
    opt.load_state_dict(torch_opt.state_dict())
    ref.load_state_dict(torch_opt.state_dict())
    assert opt.param_groups[0]["trust_clip"] is True and ref.state[twins[0]]["exp_avg"].dtype == torch.float64
    for k in range(2):
        _set_grads(ps, twins, 801 + k)
        opt.step()
        ref.step()
        _close(opt, ref, ps, twins)
    assert [int(opt.state[p]["step"]) for p in ps] == [3] * 4
    back = FusedAdamW(ps, lr=LR, weight_decay=WD)       # and FusedAdamW takes FusedLamb's state
    back.load_state_dict(opt.state_dict())
    _set_grads(ps, twins, 803)
    back.step()
    assert [int(back.state[p]["step"]) for p in ps] == [4] * 4


def test_plain_fused_adamw_never_reaches_a_lamb_entry_point(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a LAMB entry point was reached by FusedAdamW")
    for name in ("lamb_moments", "lamb_trust", "lamb_update", "build_tensor_index"):
        monkeypatch.setattr(_ops, name, refuse)
    ps = _params(64)
    for kw in ({}, {"max_grad_norm": 1.0}, {"ema_decay": 0.9}):
        opt = FusedAdamW(ps, lr=LR, **kw)
        for t in range(2):
            _set_grads(ps, _twins(ps), 900 + t)
            opt.step()
        assert all(tab.lamb is None for tab in opt._tables.values())
    lamb = FusedLamb(ps, lr=LR)
    with pytest.raises(AssertionError, match="LAMB entry point"):
        lamb.step()


# ---- through the fused engine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_engine_two_lamb_steps_against_the_host_lamb_in_fp64(dtype):
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 2, precision=dtype)      # D128 H2 L2, B2
    torch.manual_seed(0)
    m = vit.VisionTransformer(cfg).to(DEV).eval()          # eval: no dropout draw
    twin = [torch.nn.Parameter(p.detach().double()) for p in m.parameters()]
    names = [k for k, _ in m.named_parameters()]
    groups = param_groups_weight_decay(m, WD)
    index = {id(p): i for i, p in enumerate(m.parameters())}
    tgroups = [{"params": [twin[index[id(p)]] for p in g["params"]], "weight_decay": g["weight_decay"]} for g in groups]
    opt = FusedLamb(groups, lr=1e-3, max_grad_norm=1.0)
    ref = Lamb(tgroups, lr=1e-3, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(65)
    x, y = torch.randn(2, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 10, (2,), generator=g).to(DEV)
    packs = None
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        cross_entropy(m(x), y).backward()
        if packs is None:
            packs = m.hip_engine.stats["packs"]
        for p, q in zip(m.parameters(), twin):             # the same gradients
            q.grad = p.grad.detach().double()
        opt.step()
        ref.step()
    assert m.hip_engine.stats["packs"] == packs            # the update refreshed the shadows itself: no repack
    cross_entropy(m(x), y).backward()
    assert m.hip_engine.stats["packs"] == packs
    got, want = opt.trust_ratios(), ref.trust_ratios()
    shadowed = adapted = 0
    for k, p, q in zip(names, m.parameters(), twin):
        assert float((p.detach().double() - q.detach()).abs().max()) < 1e-6, k
        assert abs(float(got[p]) - float(want[q])) <= TWIN_RATIO_RTOL * float(want[q]), k
        adapted += float(got[p]) != 1.0
        if shadow_of(p) is not None and shadow_of(p).dtype == BF:
            shadowed += 1
            assert torch.equal(shadow_of(p).reshape(-1), p.detach().bfloat16().reshape(-1)), k
    assert dtype != BF or shadowed > 10
    assert adapted == len(groups[1]["params"]) and all(float(got[p]) == 1.0 for p in groups[0]["params"])


# ---- data parallel, 2 ranks (gloo; the parent makes no GPU call here, each child runs under its own timeout) -------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-transformer_amd")]
    import numpy as np
    import torch.distributed as dist
    from VisionTransformer import config, vit
    from VisionTransformer.optim import FusedLamb, cross_entropy, param_groups_weight_decay
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    m = vit.VisionTransformer(config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4)).cuda().train().enable_data_parallel()
    opt = FusedLamb(param_groups_weight_decay(m, 0.05), lr=1e-3, max_grad_norm=0.05)
    g = torch.Generator().manual_seed(100 + rank)
    x, y = torch.randn(4, 3, 64, 64, generator=g).cuda(), torch.randint(0, 10, (4,), generator=g).cuda()
    ratios = []
    for _ in range(2):
        loss = cross_entropy(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        r = opt.trust_ratios()
        ratios.append(torch.stack([r[p] for p in m.parameters()]))
    state = np.concatenate([v.detach().float().cpu().numpy().ravel() for v in m.state_dict().values()])
    q.put((rank, torch.stack(ratios).cpu().numpy(), state))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_ranks_adapt_alike():
    """After the AVG all-reduce both ranks hold the same gradients, so they compute bitwise the same norms and ratios
    and their parameters stay bitwise equal through two train-mode LAMB steps."""
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    (_, r0, st0), (_, r1, st1) = res
    assert r0.shape[0] == 2 and np.isfinite(r0).all() and (r0 != 1.0).any() and (r0 == 1.0).any()
    assert np.array_equal(r0.view(np.int32), r1.view(np.int32))
    assert np.array_equal(st0.view(np.int32), st1.view(np.int32))


def test_train_with_lamb_and_its_checkpoint_loads_into_fused_adamw(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, precision=BF)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, 64, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(4, 3, 64, 10, seed=4), batch_size=4)
    T.train(cfg, loader, test_loader, epochs=0, eval_iter=1, log_dir=str(tmp_path / "log"),
            checkpoint_dir=str(tmp_path / "ck"), lr=1e-3, opt="lamb", weight_decay=0.05, no_decay_1d=True,
            max_grad_norm=1.0, ema_decay=0.9)
    ck = torch.load(tmp_path / "ck" / "0.pt", map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step", "ema_state_dict"}
    assert ck["step"] == 2 and math.isfinite(float(ck["loss"]))
    assert [g["weight_decay"] for g in ck["optimizer_state_dict"]["param_groups"]] == [0.0, 0.05]
    model = vit.VisionTransformer(cfg)
    model.load_state_dict(ck["model_state_dict"])
    model = model.to(DEV)
    adam = FusedAdamW(param_groups_weight_decay(model, 0.05), lr=1e-3)
    adam.load_state_dict(ck["optimizer_state_dict"])
    assert all(int(adam.state[p]["step"]) == 2 and "ema" in adam.state[p] for p in model.parameters())
    x, y = next(iter(loader))
    cross_entropy(model(x.to(DEV)), y.to(DEV)).backward()
    adam.step()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    lamb = make_optimizer(param_groups_weight_decay(model, 0.05), lr=1e-3, weight_decay=0.05, opt="lamb")
    assert type(lamb) is FusedLamb
