"""GPU tests of the grouped optimizer steps (include/vit_hip.h "Grouped optimizer steps"): vit_adamw_groups and the three
vit_lamb_*_groups launches bit for bit against per-group launches of the single-group entry points (which have fp64
tests of their own, so no tolerance appears here), FusedAdamW / FusedLamb with fuse_groups against twins without, the
fused engine under layer-wise learning-rate decay, and train() with a schedule."""
import copy
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops, config, vit
    from VisionTransformer.optim import (FusedAdamW, FusedLamb, LRSchedule, cross_entropy, param_groups_layer_decay)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -777.0
PAD = 5                                    # sentinel elements behind every buffer
LEAD = 4                                   # and in front of it (16 bytes of fp32: the alignment stays what it was)
BF = torch.bfloat16
SIZES = [1, 63, 64, 257, 8192, 8193, 3 * 8192 + 5]
ZERO = 3                                   # this tensor's weights are all zero: LAMB's zero-norm rule
ADAPT, TRUST_CLIP = 1, 2


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x.detach()), _bits(y.detach())) for x, y in zip(a, b))


def _group_of(i, ntensors, G, layout):
    return i * G // ntensors if layout == "consecutive" else i % G


def _hyper(k):
    """Group k's own lr, beta1, beta2, eps, weight_decay and step count (group 0 has no weight decay)."""
    return dict(lr=1e-3 * (1 + k), b1=0.9 - 0.002 * k, b2=0.999 - 0.0002 * k, eps=1e-8 * (1 + 3 * k), wd=0.01 * k,
                t=1 + k % 5)


class _Bank:
    """p / g / m / v / shadow / EMA buffers for `ntensors` tensors of SIZES (cycled), each with LEAD sentinels in
    front of it and PAD behind; every third tensor has no EMA and every fourth no shadow.  Two banks of one seed hold
    the same bits.  `bufs` lists the whole buffers, sentinels included."""

    def __init__(self, seed, ntensors, sdt):
        gen = torch.Generator().manual_seed(seed)
        self.bufs, self.sdt, self.n = [], sdt, ntensors
        sizes = [SIZES[i % len(SIZES)] for i in range(ntensors)]

        def guarded(values, dtype=torch.float32):
            n = values.numel()
            buf = torch.full((LEAD + n + PAD,), SENTINEL, dtype=dtype, device=DEV)
            buf[LEAD:LEAD + n] = values.to(DEV, dtype)
            self.bufs.append(buf)
            return buf[LEAD:LEAD + n]

        def rnd(n, scale=1.0):
            return torch.randn(n, generator=gen) * scale

        self.ps = [guarded(rnd(n, 0.0 if i == ZERO else 1.0)) for i, n in enumerate(sizes)]
        self.gs = [guarded(rnd(n)) for n in sizes]
        self.ms = [guarded(rnd(n, 0.1)) for n in sizes]
        self.vs = [guarded(rnd(n).square() * 0.01) for n in sizes]
        self.sh = [None if i % 4 == 1 else guarded(p.cpu().to(sdt).float(), sdt) for i, p in enumerate(self.ps)]
        self.emas = [None if i % 3 == 2 else guarded(rnd(n)) for i, n in enumerate(sizes)]
        self.clip = guarded(torch.tensor([3.0, 0.37, 0.0, 0.0]))
        self.entries = list(zip(self.ps, self.gs, self.ms, self.vs, self.sh))

    def tables(self, idx):
        """Chunk table, EMA pointers and tensor index over the tensors `idx`, in that order."""
        ent = [self.entries[i] for i in idx]
        table, n = _ops.build_chunk_table(ent, DEV)
        ema_dev, _ = _ops.build_ema_pointers([(self.ps[i], self.emas[i]) for i in idx], DEV)
        first, owner, nt, _ = _ops.build_tensor_index(ent, DEV)
        return table, n, ema_dev, first, owner, nt

    def chunks_of(self, idx):
        return [len(_ops._chunks(self.ps[i].numel())) for i in idx]


def _spec(k, flags=0, f32_betas=False):
    h = _hyper(k)
    b1, b2 = h["b1"], h["b2"]
    if f32_betas:
        b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in (b1, b2))
    return (h["lr"], b1, b2, h["eps"], h["wd"], 1.0 - b1 ** h["t"], 1.0 - b2 ** h["t"], flags)


def _adamw_per_group(bank, members, mode):
    """The reference: one launch of the single-group entry point per group, on that group's own table."""
    clip = bank.clip if "clip" in mode else None
    for k, idx in enumerate(members):
        if not idx:
            continue
        table, n, ema_dev, _, _, _ = bank.tables(idx)
        lr, b1, b2, eps, wd, bc1, bc2, _ = _spec(k)
        if "ema" in mode:
            _ops.adamw_ema(table, ema_dev, n, lr, b1, b2, eps, wd, bc1, bc2, 0.5, bank.sdt, 0.9, clip=clip)
        else:
            _ops.adamw(table, n, lr, b1, b2, eps, wd, bc1, bc2, 0.5, bank.sdt, clip=clip)


def _adamw_grouped(bank, group_of, G, mode, of_chunk=None):
    table, n, ema_dev, _, _, _ = bank.tables(range(bank.n))
    if of_chunk is None:
        of_chunk = [g for g, c in zip(group_of, bank.chunks_of(range(bank.n))) for _ in range(c)]
    ema = "ema" in mode
    _ops.adamw_groups(table, torch.tensor(of_chunk, dtype=torch.int32, device=DEV), n, [_spec(k) for k in range(G)],
                      0.5, bank.sdt, ema_dev=ema_dev if ema else None, ema_decay=0.9 if ema else None,
                      clip=bank.clip if "clip" in mode else None)


CASES = [pytest.param(c, G, lay, id=f"chunk_{c or 'default'}-G{G}-{lay}")
         for c in (None, 64) for G in (1, 2, 3, 64) for lay in ("consecutive", "interleaved")]


@pytest.mark.parametrize("sdt", [BF, torch.float32], ids=["bf16_shadows", "fp32_shadows"])
@pytest.mark.parametrize("chunk,G,layout", CASES)
def test_adamw_groups_bitwise_against_per_group_launches(monkeypatch, chunk, G, layout, sdt):
    if chunk is not None:
        monkeypatch.setattr(_ops, "CHUNK", chunk)
    nt = 7 if G <= 3 else 70
    group_of = [_group_of(i, nt, G, layout) for i in range(nt)]
    members = [[i for i in range(nt) if group_of[i] == k] for k in range(G)]
    assert all(members)
    for mode in ("plain", "clip", "ema", "ema+clip"):
        ref, got = _Bank(11, nt, sdt), _Bank(11, nt, sdt)
        before = [b.clone() for b in got.bufs]
        _adamw_per_group(ref, members, mode)
        _adamw_grouped(got, group_of, G, mode)
        assert _same(got.bufs, ref.bufs), mode                          # p, m, v, shadows, EMA and every sentinel
        moved = list(range(nt)) + list(range(2 * nt, 4 * nt))           # every p, m and v buffer changed
        assert not any(_same([got.bufs[i]], [before[i]]) for i in moved), mode
    # a skipped step (clip[2] != 0) touches nothing
    for mode in ("clip", "ema+clip"):
        got = _Bank(12, nt, sdt)
        got.clip[2] = 1.0
        before = [b.clone() for b in got.bufs]
        _adamw_grouped(got, group_of, G, mode)
        assert _same(got.bufs, before), mode
    # a chunk whose group index equals ngroups is left alone; the others are not disturbed by it
    ref, got = _Bank(13, nt, sdt), _Bank(13, nt, sdt)
    skip = members[-1][-1]
    before = [t.clone() for t in (got.ps[skip], got.ms[skip], got.vs[skip])]
    of_chunk = [(G if i == skip else g) for i, (g, c) in enumerate(zip(group_of, got.chunks_of(range(nt))))
                for _ in range(c)]
    _adamw_grouped(got, group_of, G, "ema", of_chunk=of_chunk)
    assert _same([got.ps[skip], got.ms[skip], got.vs[skip]], before)
    _adamw_per_group(ref, [[i for i in idx if i != skip] for idx in members], "ema")
    assert _same(got.bufs, ref.bufs)


def _lamb_per_group(bank, members, flags, mode):
    clip = bank.clip if "clip" in mode else None
    trust = {}
    for k, idx in enumerate(members):
        table, n, ema_dev, first, owner, nt = bank.tables(idx)
        lr, b1, b2, eps, wd, bc1, bc2, _ = _spec(k, f32_betas=True)
        partial = torch.zeros(2 * n, dtype=torch.float64, device=DEV)
        tr = torch.full((nt,), SENTINEL, device=DEV)
        _ops.lamb_moments(table, n, b1, b2, eps, wd, bc1, bc2, 0.5, partial, clip=clip)
        _ops.lamb_trust(partial, first, nt, tr, adapt=bool(flags[k] & ADAPT), trust_clip=bool(flags[k] & TRUST_CLIP),
                        clip=clip)
        _ops.lamb_update(table, owner, tr, n, lr, eps, wd, bc1, bc2, bank.sdt,
                         ema_dev=ema_dev if "ema" in mode else None, ema_decay=0.9 if "ema" in mode else None,
                         clip=clip)
        trust.update(zip(idx, tr.clone()))
    return torch.stack([trust[i] for i in range(bank.n)])


def _lamb_grouped(bank, group_of, G, flags, mode):
    clip = bank.clip if "clip" in mode else None
    table, n, ema_dev, first, owner, nt = bank.tables(range(bank.n))
    of_chunk = torch.tensor([g for g, c in zip(group_of, bank.chunks_of(range(bank.n))) for _ in range(c)],
                            dtype=torch.int32, device=DEV)
    of_tensor = torch.tensor(group_of, dtype=torch.int32, device=DEV)
    specs = [_spec(k, flags[k], f32_betas=True) for k in range(G)]
    partial = torch.zeros(2 * n, dtype=torch.float64, device=DEV)
    tr = torch.full((nt + PAD,), SENTINEL, device=DEV)
    ema = "ema" in mode
    _ops.lamb_moments_groups(table, of_chunk, n, specs, 0.5, partial, clip=clip)
    _ops.lamb_trust_groups(partial, first, of_tensor, nt, specs, tr, clip=clip)
    _ops.lamb_update_groups(table, owner, tr, of_chunk, n, specs, bank.sdt, ema_dev=ema_dev if ema else None,
                            ema_decay=0.9 if ema else None, clip=clip)
    assert bool((tr[nt:] == SENTINEL).all())
    return tr[:nt].clone()


@pytest.mark.parametrize("sdt", [BF, torch.float32], ids=["bf16_shadows", "fp32_shadows"])
@pytest.mark.parametrize("chunk,G,layout", CASES)
def test_lamb_groups_bitwise_against_per_group_launches(monkeypatch, chunk, G, layout, sdt):
    if chunk is not None:
        monkeypatch.setattr(_ops, "CHUNK", chunk)
    nt = 7 if G <= 3 else 70
    group_of = [_group_of(i, nt, G, layout) for i in range(nt)]
    members = [[i for i in range(nt) if group_of[i] == k] for k in range(G)]
    # groups differ in ADAPT / TRUST_CLIP; the zero-norm tensor's group adapts, so that its rule (r = 1) decides
    flags = [(k + 1) % 4 for k in range(G)]
    flags[group_of[ZERO]] |= ADAPT
    for mode in ("plain", "ema+clip"):
        ref, got = _Bank(21, nt, sdt), _Bank(21, nt, sdt)
        want = _lamb_per_group(ref, members, flags, mode)
        trust = _lamb_grouped(got, group_of, G, flags, mode)
        assert _same(got.bufs, ref.bufs), mode
        assert torch.equal(_bits(trust), _bits(want)), mode
        assert float(trust[ZERO]) == 1.0
        adapting = [i for i in range(nt) if flags[group_of[i]] == ADAPT and i % len(SIZES) != ZERO]
        assert all(float(trust[i]) != 1.0 for i in adapting[:5]) and adapting
        assert all(float(trust[i]) == 1.0 for i in range(nt) if not flags[group_of[i]] & ADAPT)
        assert all(float(trust[i]) <= 1.0 for i in range(nt) if flags[group_of[i]] & TRUST_CLIP)
    # a skipped step touches nothing, trust[] included
    got = _Bank(22, nt, sdt)
    got.clip[2] = 1.0
    before = [b.clone() for b in got.bufs]
    trust = _lamb_grouped(got, group_of, G, flags, "ema+clip")
    assert _same(got.bufs, before) and bool((trust == SENTINEL).all())
    # a tensor whose group index equals ngroups keeps its ratio and its weights
    got = _Bank(23, nt, sdt)
    table, n, ema_dev, first, owner, _ = got.tables(range(nt))
    skip = nt - 1
    per = got.chunks_of(range(nt))
    of_chunk = torch.tensor([(G if i == skip else g) for i, (g, c) in enumerate(zip(group_of, per)) for _ in range(c)],
                            dtype=torch.int32, device=DEV)
    of_tensor = torch.tensor([(G if i == skip else g) for i, g in enumerate(group_of)], dtype=torch.int32, device=DEV)
    specs = [_spec(k, flags[k], f32_betas=True) for k in range(G)]
    partial = torch.zeros(2 * n, dtype=torch.float64, device=DEV)
    tr = torch.full((nt,), SENTINEL, device=DEV)
    before = [t.clone() for t in (got.ps[skip], got.ms[skip], got.vs[skip])]
    _ops.lamb_moments_groups(table, of_chunk, n, specs, 0.5, partial)
    _ops.lamb_trust_groups(partial, first, of_tensor, nt, specs, tr)
    _ops.lamb_update_groups(table, owner, tr, of_chunk, n, specs, sdt)
    assert _same([got.ps[skip], got.ms[skip], got.vs[skip]], before) and float(tr[skip]) == SENTINEL
    assert bool((partial[2 * (n - per[skip]):] == 0).all()) and bool((tr[:skip] != SENTINEL).all())


def test_grouped_launches_repeat_bitwise(monkeypatch):
    monkeypatch.setattr(_ops, "CHUNK", 64)
    group_of = [i % 3 for i in range(7)]
    a, b = _Bank(31, 7, BF), _Bank(31, 7, BF)
    for bank in (a, b):
        _adamw_grouped(bank, group_of, 3, "ema+clip")
    assert _same(a.bufs, b.bufs)
    a, b = _Bank(32, 7, BF), _Bank(32, 7, BF)
    ta, tb = (_lamb_grouped(bank, group_of, 3, [1, 3, 0], "ema+clip") for bank in (a, b))
    assert _same(a.bufs, b.bufs) and torch.equal(_bits(ta), _bits(tb))


def test_ops_validate_the_group_arrays():
    bank = _Bank(33, 7, BF)
    table, n, ema_dev, first, owner, nt = bank.tables(range(7))
    of_chunk = torch.zeros(n, dtype=torch.int32, device=DEV)
    specs = [_spec(0)]
    with pytest.raises(ValueError, match="group_of_chunk"):
        _ops.adamw_groups(table, of_chunk[:-1], n, specs, 1.0, BF)
    with pytest.raises(ValueError, match="group_of_chunk"):
        _ops.adamw_groups(table, of_chunk.long(), n, specs, 1.0, BF)
    with pytest.raises(ValueError, match="1..64"):
        _ops.adamw_groups(table, of_chunk, n, [_spec(0)] * 65, 1.0, BF)
    with pytest.raises(RuntimeError, match="flags"):
        _ops.adamw_groups(table, of_chunk, n, [_spec(0, ADAPT)], 1.0, BF)
    with pytest.raises(RuntimeError, match="bias corrections"):
        _ops.lamb_moments_groups(table, of_chunk, n, [(1e-3, 0.9, 0.999, 1e-6, 0.0, 0.0, 0.5, 0)], 1.0,
                                 torch.zeros(2 * n, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="group_of_tensor"):
        _ops.lamb_trust_groups(torch.zeros(2 * n, dtype=torch.float64, device=DEV), first,
                               torch.zeros(nt + 1, dtype=torch.int32, device=DEV), nt, specs,
                               torch.ones(nt, device=DEV))


# ---- FusedAdamW / FusedLamb with fuse_groups against twins without --------------------------------------------------
def _micro(dtype=torch.float32, blocks=2):
    return config.ViTConfig(3, 10, 16, 64, 16, 2, blocks, "cpu", 4, precision=dtype)


def _model(cfg, seed=0):
    torch.manual_seed(seed)
    return vit.VisionTransformer(cfg).to(DEV).eval()


def _fill_grads(models, seed, skip=()):
    """The same fresh values into every model's gradients, in place once they exist (a cached table stays valid)."""
    g = torch.Generator().manual_seed(seed)
    for i, ps in enumerate(zip(*[list(m.parameters()) for m in models])):
        v = torch.randn(ps[0].shape, generator=g).to(DEV)
        for p in ps:
            if i in skip:
                continue
            if p.grad is None:
                p.grad = v.clone()
            else:
                p.grad.copy_(v)


def _opt_state(opt, model):
    out = []
    for p in model.parameters():
        st = opt.state.get(p, {})
        out += [p.detach()] + [st[k] for k in ("exp_avg", "exp_avg_sq", "ema") if k in st]
        out += [torch.tensor(float(st["step"]))] if "step" in st else []
    return out


def _count(monkeypatch, names):
    calls = {n: 0 for n in names}
    for n in names:
        def wrap(*a, _n=n, _f=getattr(_ops, n), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(_ops, n, wrap)
    return calls


GROUPED = ("adamw_groups", "lamb_moments_groups", "lamb_trust_groups", "lamb_update_groups")
SINGLE = ("adamw", "adamw_ema", "lamb_moments", "lamb_trust", "lamb_update")


@pytest.mark.parametrize("extras", [{}, {"max_grad_norm": 1.0, "ema_decay": 0.9}], ids=["plain", "clip_ema"])
@pytest.mark.parametrize("cls_name", ["FusedAdamW", "FusedLamb"])
def test_optimizer_fuse_groups_equals_the_per_group_twin(monkeypatch, cls_name, extras):
    cls = {"FusedAdamW": FusedAdamW, "FusedLamb": FusedLamb}[cls_name]
    cfg = _micro()
    ma, mb = _model(cfg), _model(cfg)
    opts = []
    for m, fuse in ((ma, True), (mb, False)):
        groups = param_groups_layer_decay(m, 0.05, 0.75)
        assert len(groups) == 2 * (cfg.num_blocks + 2)
        kw = dict(extras, **({"trust_clip": True} if cls is FusedLamb else {}))
        opts.append(cls(groups, lr=1e-2, fuse_groups=fuse, **kw))
    a, b = opts
    scheds = [LRSchedule(o, "cosine", 5, warmup_steps=2, warmup_lr=1e-4, min_lr=1e-3) for o in opts]
    calls = _count(monkeypatch, GROUPED + SINGLE + ("build_chunk_table", "grad_sumsq"))
    late = 5                                     # this parameter's first gradient arrives at step 3
    for step in range(1, 6):
        _fill_grads([ma, mb], 100 + step, skip=(late,) if step < 3 else ())
        for n in calls:
            calls[n] = 0
        a.step()
        grouped, single, built = (sum(calls[n] for n in GROUPED), sum(calls[n] for n in SINGLE),
                                  calls["build_chunk_table"])
        sumsq_a = calls["grad_sumsq"]
        lrs = [g["lr"] for g in a.param_groups]
        b.step()
        per_launch = 3 if cls is FusedLamb else 1
        if step < 3:                                       # every group at one step count: ONE grouped launch (set)
            assert grouped == per_launch and single == 0, (step, calls)
            assert sumsq_a == (1 if extras else 0)
            assert ("groups", "all") in a._tables and len(a._tables) == 1
            assert built == (1 if step == 1 else 0), (step, built)       # a new group["lr"] builds no table
        else:                                              # the late parameter's group holds two step counts
            assert grouped == 0 and single > 0, (step, calls)
        assert lrs == [g["lr"] for g in b.param_groups] and len(set(lrs)) > 3
        assert _same(_opt_state(a, ma), _opt_state(b, mb)), step
        if extras:
            assert torch.equal(_bits(a.grad_norm()), _bits(b.grad_norm())) and float(a.grad_norm()) > 0
        if cls is FusedLamb:
            ra, rb = a.trust_ratios(), b.trust_ratios()
            assert _same([ra[p] for p in ma.parameters() if p in ra], [rb[p] for p in mb.parameters() if p in rb])
            assert len(ra) == len(rb) > 0
        for s in scheds:
            s.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and "fuse_groups" not in sa["param_groups"][0]
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        assert _same(list(sa["state"][k].values()), list(sb["state"][k].values()))
    assert {k[1] for k in b._tables} <= {"all", "t"} and ("groups", "all") not in b._tables


def test_seventy_groups_run_as_two_launches_and_equal_the_twin(monkeypatch):
    monkeypatch.setattr(_ops, "CHUNK", 64)
    torch.manual_seed(3)
    shapes = [(1 + 37 * (i % 5),) for i in range(70)]
    pa = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    mk = lambda ps: [{"params": [p], "lr": 1e-3 * (1 + i), "weight_decay": 0.01 * (i % 3)} for i, p in enumerate(ps)]
    for cls, per in ((FusedAdamW, 1), (FusedLamb, 3)):
        a, b = cls(mk(pa), fuse_groups=True, max_grad_norm=1.0), cls(mk(pb), max_grad_norm=1.0)
        calls = _count(monkeypatch, GROUPED)
        for step in range(2):
            g = torch.Generator().manual_seed(40 + step)
            for p, q in zip(pa, pb):
                p.grad = torch.randn(p.shape, generator=g).to(DEV)
                q.grad = p.grad.clone()
            for n in calls:
                calls[n] = 0
            a.step()
            assert sum(calls.values()) == 2 * per, calls
            b.step()
            assert _same([p.detach() for p in pa], [p.detach() for p in pb])
            assert _same([a.state[p][k] for p in pa for k in ("exp_avg", "exp_avg_sq")],
                         [b.state[p][k] for p in pb for k in ("exp_avg", "exp_avg_sq")])
        assert len(a._tables[("groups", "all")].spans) == 2
        monkeypatch.undo()
        monkeypatch.setattr(_ops, "CHUNK", 64)


def test_fused_groups_checkpoint_loads_into_torch_adamw_and_back():
    cfg = _micro()
    m = _model(cfg)
    mk = lambda: param_groups_layer_decay(m, 0.05, 0.75)
    opt = FusedAdamW(mk(), lr=1e-3, fuse_groups=True)
    sched = LRSchedule(opt, "cosine", 10, warmup_steps=2)
    for step in range(2):
        _fill_grads([m], 50 + step)
        opt.step()
        sched.step()
    sd = opt.state_dict()
    t = torch.optim.AdamW(mk(), lr=1e-3)
    t.load_state_dict(copy.deepcopy(sd))
    assert all(int(t.state[p]["step"]) == 2 for p in m.parameters())
    assert [g["lr"] for g in t.param_groups] == [g["lr"] for g in opt.param_groups]
    assert all(g["initial_lr"] == 1e-3 for g in t.param_groups)
    _fill_grads([m], 52)
    t.step()
    back = FusedAdamW(mk(), lr=1e-3, fuse_groups=True)
    back.load_state_dict(t.state_dict())
    s2 = LRSchedule(back, "cosine", 10, warmup_steps=2)
    s2.load_state_dict(sched.state_dict())
    assert [g["lr"] for g in back.param_groups] == [g["lr"] for g in opt.param_groups]
    _fill_grads([m], 53)
    back.step()
    assert all(int(back.state[p]["step"]) == 4 for p in m.parameters())
    assert ("groups", "all") in back._tables and all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- through the fused engine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["FusedAdamW", "FusedLamb"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_engine_three_steps_under_layer_decay(dtype, cls_name):
    cls = {"FusedAdamW": FusedAdamW, "FusedLamb": FusedLamb}[cls_name]
    cfg = _micro(dtype)
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(4, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 10, (4,), generator=g).to(DEV)
    runs = []
    for fuse in (True, False):
        m = _model(cfg)
        opt = cls(param_groups_layer_decay(m, 0.05, 0.75), lr=1e-3, fuse_groups=fuse, max_grad_norm=1.0,
                  ema_decay=0.9)
        sched = LRSchedule(opt, "cosine", 3, warmup_steps=1, warmup_lr=1e-5)
        out, packs = [], None
        for step in range(3):
            opt.zero_grad(set_to_none=True)
            logits = m(x)
            if packs is None:
                packs = m.hip_engine.stats["packs"]
            loss = cross_entropy(logits, y)
            loss.backward()
            opt.step()
            sched.step()
            out += [logits.detach().clone(), loss.detach().clone()]
        assert m.hip_engine.stats["packs"] == packs            # the grouped update refreshed the shadows itself
        with opt.ema_weights(), torch.no_grad():
            out.append(m(x).detach().clone())
        out.append(m(x).detach().clone())
        assert m.hip_engine.stats["packs"] == packs            # nor does evaluating the EMA repack
        assert (("groups", "all") in opt._tables) == fuse
        runs.append(out)
    assert _same(runs[0], runs[1])
    assert not torch.equal(runs[0][0], runs[0][2]) and not torch.equal(runs[0][-1], runs[0][-2])


def test_train_with_a_cosine_schedule_and_layer_decay(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = _micro(BF)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, 64, 10, seed=3), batch_size=4, drop_last=True)
    kw = dict(eval_iter=1, log_dir=str(tmp_path / "log"), checkpoint_dir=str(tmp_path / "ck"), lr=1e-3,
              sched="cosine", warmup_steps=1, warmup_lr=1e-5, layer_decay=0.75, weight_decay=0.05, max_grad_norm=1.0)
    T.train(cfg, loader, None, epochs=0, **kw)
    ck = torch.load(tmp_path / "ck" / "0.pt", map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step", "lr_schedule"}
    assert ck["lr_schedule"] == {"t": 2} and ck["step"] == 2 and math.isfinite(float(ck["loss"]))
    groups = ck["optimizer_state_dict"]["param_groups"]
    assert len(groups) == 2 * (cfg.num_blocks + 2) and groups[0]["lr_scale"] == 0.75 ** 3
    assert all(g["initial_lr"] == 1e-3 for g in groups)
    T.train(cfg, loader, None, epochs=1, **kw)                 # resumes from 0.pt at t = 2
    ck1 = torch.load(tmp_path / "ck" / "1.pt", map_location="cpu", weights_only=True)
    assert ck1["lr_schedule"] == {"t": 6} and ck1["step"] == 6 and math.isfinite(float(ck1["loss"]))
    assert all(int(s["step"]) == 6 for s in ck1["optimizer_state_dict"]["state"].values())
