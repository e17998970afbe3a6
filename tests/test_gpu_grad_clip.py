"""GPU tests of global-norm gradient clipping inside the fused AdamW step (include/vit_hip.h "Gradient clipping"):
the norm and finish kernels against fp64, the clipped update against clip_grad_norm_ + torch.optim.AdamW, identity
when nothing is clipped, the non-finite skip, FusedAdamW(max_grad_norm=...) over param groups and through the
engine, and two data-parallel ranks staying bitwise in step."""
import os
import socket
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops, config, vit
    from VisionTransformer._engine import shadow_of
    from VisionTransformer.optim import FusedAdamW, cross_entropy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -777.0
SHAPES = [(1,), (300,), (8193,), (128, 64)]
BF = torch.bfloat16
LR, WD = 1e-3, 1e-4
# fp64 accumulation leaves the fp32 product's conversion and the final sqrt-and-cast as the only fp32 roundings
NORM_RTOL = 2.0 ** -22


class _Set:
    """p / g / m / v / shadow tensors of SHAPES plus a 7-element tensor whose gradient starts 4 bytes (not 16) into
    a larger buffer, their chunk table, and the partial / clip buffers with sentinels behind them."""

    def __init__(self, seed):
        torch.manual_seed(seed)
        self.ps = [torch.randn(s, device=DEV) for s in SHAPES] + [torch.randn(7, device=DEV)]
        self.gs = [torch.randn(s, device=DEV) for s in SHAPES]
        self.gbuf = torch.randn(64, device=DEV)
        self.gs.append(self.gbuf[1:8])
        assert self.gs[-1].data_ptr() % 16 == 4
        self.ms = [torch.zeros_like(p) for p in self.ps]
        self.vs = [torch.zeros_like(p) for p in self.ps]
        # bf16 shadows, one entry (300 elements) without: a NULL-shadow chunk
        self.sh = [None if i == 1 else torch.full(p.shape, SENTINEL, dtype=BF, device=DEV)
                   for i, p in enumerate(self.ps)]
        self.table, self.n = _ops.build_chunk_table(list(zip(self.ps, self.gs, self.ms, self.vs, self.sh)), DEV)
        assert self.n == sum(-(-p.numel() // _ops.CHUNK) for p in self.ps) and _ops.CHUNK < 8193 <= 2 * _ops.CHUNK
        self.partial = torch.full((self.n + 3,), SENTINEL, dtype=torch.float64, device=DEV)
        self.clip = torch.full((7,), SENTINEL, device=DEV)
        self.clip[:4] = 0

    def norm_pass(self, max_norm, gs=1.0, skip_nonfinite=True):
        _ops.grad_sumsq(self.table, self.n, gs, self.partial)
        _ops.grad_clip_finish(self.partial, self.n, max_norm, self.clip, skip_nonfinite)

    def adamw(self, step, gs=1.0, clip=True):
        _ops.adamw(self.table, self.n, LR, 0.9, 0.999, 1e-8, WD, 1 - 0.9 ** step, 1 - 0.999 ** step, gs, BF,
                   clip=self.clip if clip else None)

    def ref_norm(self, gs=1.0):
        return float(torch.sqrt(sum((gs * g).double().pow(2).sum() for g in self.gs)))

    def state(self):
        return [t.clone() for ts in (self.ps, self.ms, self.vs, [s for s in self.sh if s is not None]) for t in ts]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    """Bitwise equality of two tensor lists (NaNs and signed zeros included)."""
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_norm_kernels_against_fp64(gs):
    s = _Set(21)
    s.norm_pass(1.0, gs)
    want = s.ref_norm(gs)
    got = float(s.clip[0])
    print(f"grad_scale {gs}: norm {got!r} vs fp64 {want!r}, rel err {abs(got - want) / want:.3e}")
    assert abs(got - want) <= NORM_RTOL * want
    # per chunk too: partial[i] is that chunk's fp64 sum of squares; two fp64 summation orders of at most 8192
    # non-negative terms differ by at most 8192 * 2^-53 < 1e-12 relative
    chunks = [(gs * g).reshape(-1)[o:o + _ops.CHUNK].double().pow(2).sum() for g in s.gs
              for o in range(0, g.numel(), _ops.CHUNK)]
    assert torch.allclose(s.partial[:s.n], torch.stack(chunks), rtol=1e-12, atol=0)
    coef = float(s.clip[1])
    assert coef == min(1.0, float(torch.tensor(1.0) / (s.clip[0].cpu() + 1e-6)))
    assert float(s.clip[2]) == 0 and float(s.clip[3]) == 0
    # sentinels behind partial[n) and clip[4) are untouched
    assert bool((s.partial[s.n:] == SENTINEL).all()) and bool((s.clip[4:] == SENTINEL).all())
    # a second run: bitwise the same
    first = (s.partial.clone(), s.clip.clone())
    s.partial[:s.n] = 0
    s.norm_pass(1.0, gs)
    assert torch.equal(s.partial.view(torch.int64), first[0].view(torch.int64))
    assert torch.equal(s.clip.view(torch.int32), first[1].view(torch.int32))


def test_clipped_update_against_torch():
    s = _Set(22)
    max_norm = 0.5 * s.ref_norm()                      # every step clips: the gradients stay the same
    ref = [p.clone().requires_grad_(True) for p in s.ps]
    opt = torch.optim.AdamW(ref, lr=LR, weight_decay=WD)
    for step in range(1, 4):
        for r, g in zip(ref, s.gs):
            r.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
        s.norm_pass(max_norm)
        s.adamw(step)
        assert 0.49 < float(s.clip[1]) < 0.51 and float(s.clip[2]) == 0
    for p, r, sh in zip(s.ps, ref, s.sh):
        assert float((p - r.detach()).abs().max()) < 1e-6
        if sh is not None:
            assert torch.equal(sh, p.bfloat16())
    assert s.sh[1] is None                             # the NULL-shadow entry was updated like the others


def test_identity_when_nothing_is_clipped():
    a, b = _Set(23), _Set(23)
    a.norm_pass(2.0 * a.ref_norm())
    assert float(a.clip[1]) == 1.0 and float(a.clip[2]) == 0
    for step in range(1, 3):
        a.adamw(step)
        b.adamw(step, clip=False)                      # vit_adamw on the same inputs
    assert _same(a.state(), b.state())


def test_nonfinite_norm_skips_the_update():
    s = _Set(24)
    s.norm_pass(1.0)
    s.adamw(1)                                         # moments and shadows hold real values before the bad steps
    before = s.state()
    for count, bad in ((1, float("inf")), (2, float("nan"))):
        s.gs[-1][5] = bad                              # in the last tensor
        s.norm_pass(1.0)
        s.adamw(2)
        assert float(s.clip[2]) == 1 and float(s.clip[1]) == 0 and float(s.clip[3]) == count
        assert not bool(torch.isfinite(s.clip[0]))
        assert _same(s.state(), before)
    # a finite step afterwards updates, and the counter stays
    s.gs[-1][5] = 0.25
    s.norm_pass(1.0)
    s.adamw(2)
    assert float(s.clip[2]) == 0 and float(s.clip[3]) == 2 and not _same(s.state(), before)
    assert all(bool(torch.isfinite(p).all()) for p in s.ps)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_norm_without_skip_follows_torch(bad):
    s = _Set(25)
    s.gs[-1][5] = bad
    ref = [p.clone().requires_grad_(True) for p in s.ps]
    for r, g in zip(ref, s.gs):
        r.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ref, 1.0)
    torch.optim.AdamW(ref, lr=LR, weight_decay=WD).step()
    s.norm_pass(1.0, skip_nonfinite=False)
    s.adamw(1)
    assert float(s.clip[2]) == 0 and float(s.clip[3]) == 0
    for p, r in zip(s.ps, ref):                        # non-finite exactly where torch's parameters are
        assert torch.equal(torch.isfinite(p), torch.isfinite(r.detach()))
    assert not bool(torch.isfinite(s.ps[-1]).all())


def test_optimizer_two_groups_and_a_gradless_parameter():
    torch.manual_seed(26)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in SHAPES]
    idle = torch.nn.Parameter(torch.randn(50, device=DEV))           # never gets a gradient
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    groups = lambda t, extra: [{"params": t[:2] + extra, "lr": 1e-3}, {"params": t[2:], "lr": 3e-3}]
    grads = [[torch.randn(s, device=DEV) * (1 + k) for s in SHAPES] for k in range(3)]
    norm0 = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads[0])))
    max_norm = 0.5 * norm0                                           # later steps have larger gradients: all clip
    opt = FusedAdamW(groups(ps, [idle]), weight_decay=WD, max_grad_norm=max_norm)
    ref = torch.optim.AdamW(groups(twin, []), weight_decay=WD)
    idle0 = idle.detach().clone()
    seen, want = [], []
    for gset in grads:
        for p, t, g in zip(ps, twin, gset):
            p.grad, t.grad = g.clone(), g.clone()
        want.append(float(torch.sqrt(sum(g.double().pow(2).sum() for g in gset))))
        torch.nn.utils.clip_grad_norm_(twin, max_norm)
        ref.step()
        opt.step()
        seen.append(opt.grad_norm())                                 # read only after the loop
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]
    for got, w in zip(torch.stack(seen).tolist(), want):
        assert abs(got - w) <= NORM_RTOL * w
    assert len({float(v) for v in seen}) == 3 and float(opt.skipped_steps()) == 0
    for p, t in zip(ps, twin):
        assert float((p - t).detach().abs().max()) < 1e-6
    assert torch.equal(idle, idle0) and not opt.state.get(idle)          # untouched, and no moments were made for it


def test_optimizer_unclipped_path_is_unchanged():
    """max_grad_norm=None: bitwise the step of a FusedAdamW built without the keyword, and no clip state appears."""
    torch.manual_seed(27)
    a = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in SHAPES]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = FusedAdamW(a, lr=LR, max_grad_norm=None), FusedAdamW(b, lr=LR)
    for _ in range(2):
        for p, q in zip(a, b):
            p.grad = torch.randn_like(p)
            q.grad = p.grad.clone()
        oa.step()
        ob.step()
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and oa._clip is None and oa._partial is None


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["micro_fp32", "d128h2_bf16"])
def test_engine_clipped_step_equals_clip_grad_norm_then_step(dtype):
    if dtype == torch.float32:
        cfg, img = config.ViTConfig(3, 10, 4, 64, 16, 4, 2, "cpu", 4), 32
    else:
        cfg, img = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, precision=BF), 64
    torch.manual_seed(0)
    m = vit.VisionTransformer(cfg).to(DEV).eval()          # eval: no dropout draw, the twin sees the same gradients
    torch.manual_seed(0)
    twin = vit.VisionTransformer(cfg).to(DEV).eval()
    g = torch.Generator().manual_seed(28)
    x, y = torch.randn(4, 3, img, img, generator=g).to(DEV), torch.randint(0, 10, (4,), generator=g).to(DEV)
    cross_entropy(twin(x), y).backward()
    max_norm = 0.5 * float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in twin.parameters())))
    opt = FusedAdamW(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=max_norm)
    ref = FusedAdamW(twin.parameters(), lr=LR, weight_decay=WD)
    for step in range(2):
        for mod, o in ((m, opt), (twin, ref)):
            o.zero_grad(set_to_none=True)
            cross_entropy(mod(x), y).backward()
        want = torch.nn.utils.clip_grad_norm_(list(twin.parameters()), max_norm)
        ref.step()
        opt.step()
        assert abs(float(opt.grad_norm()) - float(want)) <= 1e-5 * float(want), step
    assert float(opt.skipped_steps()) == 0
    shadowed = 0
    for (k, p), q in zip(m.named_parameters(), twin.parameters()):
        assert float((p - q).detach().abs().max()) < 1e-6, k
        if shadow_of(p) is not None and shadow_of(p).dtype == BF:
            shadowed += 1
            assert torch.equal(shadow_of(p), shadow_of(q)), k
            assert torch.equal(shadow_of(p).reshape(-1), p.detach().bfloat16().reshape(-1)), k
    assert dtype != BF or shadowed > 10                  # the GEMM weights of the bf16 engine have bf16 shadows


@pytest.mark.parametrize("reference_loop", [False, True])
def test_train_logs_grad_norm_when_clipping(tmp_path, monkeypatch, capsys, reference_loop):
    """train(..., max_grad_norm=...) on the device: GradNorm/train_batch beside every Loss/train_batch record, the
    first norm above the bound (so the step clipped), the skipped-step line; without the keyword, no such record."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, precision=BF)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(12, 3, 64, 10, seed=3), batch_size=4, drop_last=True)

    def run(name, **kw):
        T.train(cfg, loader, None, epochs=0, eval_iter=1, log_dir=str(tmp_path / name),
                checkpoint_dir=str(tmp_path / (name + "_ck")), lr=1e-3, reference_loop=reference_loop, **kw)
        recs = [json.loads(l) for l in open(tmp_path / name / "scalars.jsonl")]
        return {tag: [(r["step"], r["value"]) for r in recs if r["tag"] == tag]
                for tag in ("Loss/train_batch", "GradNorm/train_batch")}

    got = run("clip", max_grad_norm=0.05)
    assert [s_ for s_, _ in got["GradNorm/train_batch"]] == [0, 1, 2] == [s_ for s_, _ in got["Loss/train_batch"]]
    norms = [v for _, v in got["GradNorm/train_batch"]]
    assert all(v > 0.05 and v == v and v != float("inf") for v in norms) and len(set(norms)) == 3
    assert "steps skipped for a non-finite gradient norm: 0" in capsys.readouterr().out
    plain = run("plain")
    assert plain["GradNorm/train_batch"] == [] and len(plain["Loss/train_batch"]) == 3
    assert "skipped" not in capsys.readouterr().out


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
    from VisionTransformer import vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    from VisionTransformer import config
    m = vit.VisionTransformer(config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4)).cuda().train().enable_data_parallel()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=0.05)
    g = torch.Generator().manual_seed(100 + rank)
    x, y = torch.randn(4, 3, 64, 64, generator=g).cuda(), torch.randint(0, 10, (4,), generator=g).cuda()
    norms = []
    for _ in range(2):
        loss = cross_entropy(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        norms.append(opt.grad_norm())
    state = np.concatenate([v.detach().float().cpu().numpy().ravel() for v in m.state_dict().values()])
    q.put((rank, torch.stack(norms).cpu().numpy(), float(opt.skipped_steps()), state))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_ranks_clip_alike():
    """After the AVG all-reduce both ranks hold the same gradients, so they compute bitwise the same norm and
    coefficient and their parameters stay bitwise equal through two clipped train-mode steps."""
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
    (_, n0, s0, st0), (_, n1, s1, st1) = res
    assert n0.shape == (2,) and np.isfinite(n0).all() and (n0 > 0.05).all()      # both steps clipped
    assert np.array_equal(n0.view(np.int32), n1.view(np.int32))
    assert s0 == s1 == 0
    assert np.array_equal(st0.view(np.int32), st1.view(np.int32))
