"""CPU-only checks of LAMB: the host optimizer optim.Lamb against an fp64 restatement of the formulas (FusedLamb's
docstring), its trust ratios, the degenerate tensors, the non-finite skip, the state-dict round trips through
torch.optim.AdamW and FusedAdamW, optim.param_groups_weight_decay, make_optimizer's unchanged defaults,
_ops.build_tensor_index, train() on the host path, and tests/host_abi_lamb_check.c (ABI still 18, and the argument
checks of the three new entry points, no GPU)."""
import copy
import math
import os
import shutil
import subprocess

import pytest
import torch

from VisionTransformer import _lib, _ops, config, vit
from VisionTransformer.optim import (ClippedAdamW, EmaAdamW, FusedAdamW, FusedLamb, Lamb, cross_entropy,
                                     make_optimizer, param_groups_weight_decay)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-2, 0.05
B1, B2, EPS = 0.9, 0.999, 1e-6
U = 2.0 ** -24                 # one fp32 rounding, relative
# The host path forms everything in fp32 torch ops.  Counting roundings of the expressions as optim.Lamb writes them:
#   m = m * b1 (1) + fl(1 - b1) (1) * g (1), summed (1): 4, on max(|m_old|, |g|)
#   v = v * b2 (1) + fl(1 - b2) (1) * g * g (2), summed (1): 5, on max(v_old, g^2)
#   u = (m / bc1) (1) / (sqrt(v) (1) / sqrt(bc2) (1) + eps (1)) (1) + wd * p (2): 7, relative to max(|m_hat/denom|, |wd p|)
#   a norm: torch sums squares in fp32 blocks (vectorised partial sums, then a tree); for the fewer than 2^16 elements
#           of this model's tensors the square (1) and 16 levels of adds bound it by 17, halved by the sqrt, and one
#           more for the sqrt itself: 9.5 per norm, 19 for both
#   r = wn / un (1): 7 (u inside its norm) + 19 + 1 = 27 -> GATE_R = 2^-19 (32 roundings)
#   p = p + (-lr) * (u * r (1)) (1), summed (1 on the result): (7 + 27 + 2) * |lr r u| + 1 * M = 37 -> GATE_P = 2^-18 * M
# with M = max(|p_old|, |lr r u|).  Measured ratios are printed; they sit far below, errors being random in sign.
GATE_M, GATE_V, GATE_R, GATE_P = 2.0 ** -22, 2.0 ** -21, 2.0 ** -19, 2.0 ** -18


def _micro():
    return config.ViTConfig(3, 10, 4, 64, 16, 4, 2, "cpu", 4)


def _batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)


def _backward(m, x, y):
    for p in m.parameters():
        p.grad = None
    cross_entropy(m(x), y).backward()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _model(seed=0):
    torch.manual_seed(seed)
    return vit.VisionTransformer(_micro()).eval()        # eval: no dropout draw, a twin sees the same gradients


def lamb_ref(p_old, m_new, v_new, t, lr, wd, adapt, trust_clip, b1=B1, b2=B2, eps=EPS):
    """The specification in fp64 from fp32 tensors: (u, r, p_new)."""
    m, v, p = m_new.double(), v_new.double(), p_old.double()
    u = (m / (1 - b1 ** t)) / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps) + wd * p
    r = 1.0
    if adapt:
        wn, un = float(p.norm()), float(u.norm())
        if wn > 0 and un > 0:
            r = wn / un
    if trust_clip:
        r = min(r, 1.0)
    return u, r, p - lr * r * u


@pytest.mark.parametrize("max_grad_norm", [None, 0.05], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("trust_clip", [False, True], ids=["", "trust_clip"])
@pytest.mark.parametrize("always_adapt", [False, True], ids=["", "always_adapt"])
def test_host_lamb_against_fp64(always_adapt, trust_clip, max_grad_norm):
    m = _model()
    x, y = _batch()
    groups = param_groups_weight_decay(m, WD)
    assert [g["weight_decay"] for g in groups] == [0.0, WD] and all(g["params"] for g in groups)
    opt = make_optimizer(groups, lr=LR, weight_decay=WD, device="cpu", opt="lamb", always_adapt=always_adapt,
                         trust_clip=trust_clip, max_grad_norm=max_grad_norm)
    assert type(opt) is Lamb and opt.defaults["eps"] == EPS and opt.defaults["betas"] == (B1, B2)
    assert all(g["always_adapt"] is always_adapt and g["trust_clip"] is trust_clip for g in opt.param_groups)
    worst = dict(m=0.0, v=0.0, r=0.0, p=0.0)
    names = {p: k for k, p in m.named_parameters()}
    for t in range(1, 4):
        _backward(m, x, y)
        raw = {p: p.grad.clone() for p in names}
        old = {p: (p.detach().clone(), opt.state[p]["exp_avg"].clone() if t > 1 else torch.zeros_like(p),
                   opt.state[p]["exp_avg_sq"].clone() if t > 1 else torch.zeros_like(p)) for p in names}
        opt.step()
        ratios = opt.trust_ratios()
        assert set(ratios) == set(names)
        if max_grad_norm:
            norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in raw.values()))
            assert norm > max_grad_norm and abs(float(opt.grad_norm()) - norm) <= 1e-5 * norm
            coef = max_grad_norm / (norm + 1e-6)
        small = 0
        for group in opt.param_groups:
            wd, adapt = group["weight_decay"], group["weight_decay"] != 0 or always_adapt
            for p in group["params"]:
                p0, m0, v0 = old[p]
                g = p.grad                                   # after clip_grad_norm_: what the update read
                if max_grad_norm:                            # coef reached g
                    assert torch.allclose(g.double(), raw[p].double() * coef, rtol=1e-5, atol=0)
                else:
                    assert torch.equal(g, raw[p])
                st = opt.state[p]
                assert int(st["step"]) == t and set(st) == {"step", "exp_avg", "exp_avg_sq"}
                m64 = B1 * m0.double() + (1 - B1) * g.double()
                v64 = B2 * v0.double() + (1 - B2) * g.double() ** 2
                big_m = torch.maximum(m0.abs(), g.abs()).double()
                big_v = torch.maximum(v0, g * g).double()
                worst["m"] = max(worst["m"], float(((st["exp_avg"].double() - m64).abs() / (GATE_M * big_m + 1e-300)).max()))
                worst["v"] = max(worst["v"], float(((st["exp_avg_sq"].double() - v64).abs() / (GATE_V * big_v + 1e-300)).max()))
                u, r, p_ref = lamb_ref(p0, st["exp_avg"], st["exp_avg_sq"], t, LR, wd, adapt, trust_clip)
                got = float(ratios[p])
                if not adapt:
                    assert got == 1.0, names[p]              # exactly 1 for every weight_decay = 0 tensor
                if trust_clip:
                    assert got <= 1.0
                worst["r"] = max(worst["r"], abs(got - r) / (GATE_R * r))
                big = torch.maximum(p0.double().abs(), (LR * r * u).abs())
                worst["p"] = max(worst["p"], float(((p.detach().double() - p_ref).abs() / (GATE_P * big + 1e-300)).max()))
                if wd != 0 and got < 0.5:
                    small += 1
        if t == 1:
            # at step 1 u ~ sign(g) + wd * w: a weight matrix's |u| is about sqrt(numel), its |w| far less, so LAMB
            # is far from AdamW there
            assert small >= 1
    print("worst error / gate over 3 steps: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def _one(values, grad, **kw):
    p = torch.nn.Parameter(torch.tensor(values, dtype=torch.float32))
    p.grad = torch.tensor(grad, dtype=torch.float32)
    return p, Lamb([p], lr=LR, **kw)


def test_degenerate_tensors():
    # an all-zero weight tensor: |w| = 0, so r = 1 and the step is Adam's
    p, opt = _one([0.0, 0.0, 0.0], [1.0, -2.0, 0.5], weight_decay=WD)
    opt.step()
    assert float(opt.trust_ratios()[p]) == 1.0
    _, r, ref = lamb_ref(torch.zeros(3), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], 1, LR, WD, True, False)
    assert r == 1.0 and torch.allclose(p.detach().double(), ref, rtol=1e-6, atol=0) and bool((p != 0).all())
    # zero gradient, no decay: u = 0, r = 1 (always_adapt too: |u| = 0), w unchanged bitwise
    for always in (False, True):
        p, opt = _one([0.3, -1.5, 2.0 ** -130], [0.0, 0.0, 0.0], weight_decay=0.0, always_adapt=always)
        before = p.detach().clone()
        opt.step()
        assert float(opt.trust_ratios()[p]) == 1.0 and torch.equal(_bits(p), _bits(before))
        assert int(opt.state[p]["step"]) == 1
    # a ratio above 1 is bounded by trust_clip and only by it
    for clip, want in ((False, 100.0), (True, 1.0)):
        p, opt = _one([100.0], [1.0], weight_decay=0.0, always_adapt=True, trust_clip=clip)
        opt.step()
        assert abs(float(opt.trust_ratios()[p]) - want) <= 1e-4 * want


def test_nonfinite_norm_with_skip_leaves_everything_alone():
    m = _model(1)
    x, y = _batch()
    opt = make_optimizer(param_groups_weight_decay(m, WD), lr=LR, weight_decay=WD, device="cpu", opt="lamb",
                         max_grad_norm=1.0, ema_decay=0.9)
    _backward(m, x, y)
    opt.step()
    ps = list(m.parameters())
    before = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in ps]
    ratios = opt.trust_ratios()
    _backward(m, x, y)
    ps[-1].grad.view(-1)[0] = float("inf")
    opt.step()
    assert float(opt.skipped_steps()) == 1 and not bool(torch.isfinite(opt.grad_norm()))
    for p, (b, st) in zip(ps, before):
        assert torch.equal(_bits(p), _bits(b)) and set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
        assert all(torch.equal(opt.state[p][k], v) for k, v in st.items())
        assert torch.equal(opt.trust_ratios()[p], ratios[p])
    _backward(m, x, y)
    opt.step()
    assert float(opt.skipped_steps()) == 1
    assert all(not torch.equal(p.detach(), b) for p, (b, _) in zip(ps, before) if p.numel() > 1)


def test_ema_follows_the_lamb_weights():
    m, twin = _model(2), _model(2)
    x, y = _batch()
    opt = Lamb(param_groups_weight_decay(m, WD), lr=LR, ema_decay=0.9)
    ref = Lamb(param_groups_weight_decay(twin, WD), lr=LR)
    for _ in range(2):
        _backward(m, x, y)
        _backward(twin, x, y)
        prev = [opt.state[p]["ema"].clone() if "ema" in opt.state[p] else p.detach().clone() for p in m.parameters()]
        opt.step()
        ref.step()
        for p, q, e in zip(m.parameters(), twin.parameters(), prev):
            assert torch.equal(_bits(p), _bits(q))               # the EMA leaves the update alone
            want = e.double() + 0.1 * (p.detach().double() - e.double())
            big = torch.maximum(e.abs(), p.detach().abs()).double()
            assert bool(((opt.state[p]["ema"].double() - want).abs() <= 2.0 ** -22 * big).all())
    p0 = [p.detach().clone() for p in m.parameters()]
    with opt.ema_weights():
        assert all(torch.equal(p, opt.state[p]["ema"]) is False or p.numel() == 1 for p in m.parameters())
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(m.parameters(), p0))


def test_state_dict_round_trips_through_adamw_formats():
    m = _model(3)
    x, y = _batch()
    ps = list(m.parameters())
    opt = Lamb(param_groups_weight_decay(m, WD), lr=LR, always_adapt=True, trust_clip=True)
    for _ in range(2):
        _backward(m, x, y)
        opt.step()
    sd = opt.state_dict()
    assert all(g["always_adapt"] is True and g["trust_clip"] is True for g in sd["param_groups"])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    moments = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    # torch.optim.AdamW takes it, steps from it, and hands it back
    t = torch.optim.AdamW(param_groups_weight_decay(m, WD), lr=LR)
    t.load_state_dict(copy.deepcopy(sd))
    assert all(torch.equal(t.state[p]["exp_avg"], a) and int(t.state[p]["step"]) == 2 for p, (a, _) in zip(ps, moments))
    _backward(m, x, y)
    t.step()
    back = Lamb(param_groups_weight_decay(m, WD), lr=LR, trust_clip=True)
    tsd = t.state_dict()
    for g in tsd["param_groups"]:                                # a torch AdamW checkpoint knows neither key
        g.pop("always_adapt", None)
        g.pop("trust_clip", None)
    back.load_state_dict(tsd)
    assert all(g["always_adapt"] is False and g["trust_clip"] is True for g in back.param_groups)
    _backward(m, x, y)
    back.step()
    assert all(int(back.state[p]["step"]) == 4 for p in ps)
    # FusedAdamW's and FusedLamb's format (constructing and loading them needs no GPU)
    for cls in (FusedAdamW, FusedLamb):
        f = cls(param_groups_weight_decay(m, WD), lr=LR)
        f.load_state_dict(copy.deepcopy(sd))
        assert all(torch.equal(f.state[p]["exp_avg"], a) and torch.equal(f.state[p]["exp_avg_sq"], b)
                   and int(f.state[p]["step"]) == 2 for p, (a, b) in zip(ps, moments))
        again = Lamb(param_groups_weight_decay(m, WD), lr=LR)
        again.load_state_dict(f.state_dict())
        assert all(torch.equal(again.state[p]["exp_avg"], a) for p, (a, _) in zip(ps, moments))
    plain = FusedAdamW(param_groups_weight_decay(m, WD), lr=LR).state_dict()
    fl = FusedLamb(param_groups_weight_decay(m, WD), lr=LR, always_adapt=True)
    assert set(fl.state_dict()["param_groups"][0]) == set(plain["param_groups"][0]) | {"always_adapt", "trust_clip"}
    fl.load_state_dict(plain)
    assert all(g["always_adapt"] is True and g["trust_clip"] is False for g in fl.param_groups)


def test_param_groups_weight_decay_on_the_real_model():
    m = vit.VisionTransformer(config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4))
    frozen = m.mlp[3].weight
    frozen.requires_grad_(False)
    plain, decay = param_groups_weight_decay(m, 0.05)
    assert plain["weight_decay"] == 0.0 and decay["weight_decay"] == 0.05
    names = {id(p): k for k, p in m.named_parameters()}
    in_plain, in_decay = {names[id(p)] for p in plain["params"]}, {names[id(p)] for p in decay["params"]}
    assert not in_plain & in_decay and names[id(frozen)] not in in_plain | in_decay
    assert in_plain | in_decay == {k for k, p in m.named_parameters() if p.requires_grad}
    for k, p in m.named_parameters():
        if p.requires_grad:
            want_plain = p.ndim <= 1 or k.endswith(".bias") or k.rsplit(".", 1)[-1] in ("cls_tkn_embd", "pos_embd")
            assert (k in in_plain) == want_plain, k
    assert {"emdeddings.cls_tkn_embd", "emdeddings.pos_embd"} <= in_plain       # 3-d, listed by name
    assert any(k.endswith(".weight") and m.get_parameter(k).ndim == 1 for k in in_plain)      # norm weights
    assert all(m.get_parameter(k).ndim >= 2 for k in in_decay) and in_decay
    # an empty list leaves only the shape and the ".bias" rule; a full name works as a last component does
    p2, d2 = param_groups_weight_decay(m, 0.05, no_decay=())
    assert {names[id(p)] for p in d2["params"]} == in_decay | {"emdeddings.cls_tkn_embd", "emdeddings.pos_embd"}
    p3, _ = param_groups_weight_decay(m, 0.05, no_decay=("emdeddings.pos_embd",))
    assert "emdeddings.pos_embd" in {names[id(p)] for p in p3["params"]}
    assert "emdeddings.cls_tkn_embd" not in {names[id(p)] for p in p3["params"]}


def test_make_optimizer_defaults_are_unchanged():
    p = torch.nn.Parameter(torch.ones(4))
    assert type(make_optimizer([p], device="cpu")) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", opt="adamw")) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", max_grad_norm=1.0)) is ClippedAdamW
    assert type(make_optimizer([p], device="cpu", ema_decay=0.9)) is EmaAdamW
    assert type(make_optimizer([p], device="cuda")) is FusedAdamW          # constructing it needs no GPU
    assert type(make_optimizer([p], device="cuda", opt="lamb")) is FusedLamb
    assert type(make_optimizer([p], device="cpu", opt="lamb")) is Lamb
    d = make_optimizer([p], device="cuda").defaults
    assert d == dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    for cls in (FusedLamb, Lamb):
        o = cls([p])
        assert {k: o.defaults[k] for k in ("lr", "betas", "eps", "weight_decay", "always_adapt", "trust_clip")} == dict(
            lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False, trust_clip=False)
        assert o.max_grad_norm is None and o.ema_decay is None and o.skip_nonfinite is True
        with pytest.raises(ValueError, match="always_adapt"):
            cls([p], always_adapt=1)
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls([p], max_grad_norm=0.0)
        with pytest.raises(ValueError, match="ema_decay"):
            cls([p], ema_decay=1.0)
    assert FusedLamb.refreshes_shadows is True and issubclass(FusedLamb, FusedAdamW)
    with pytest.raises(ValueError, match="opt must be"):
        make_optimizer([p], device="cpu", opt="lars")
    with pytest.raises(ValueError, match="belong to opt='lamb'"):
        make_optimizer([p], device="cpu", trust_clip=True)


def test_tensor_index_is_cut_like_the_chunk_table(monkeypatch):
    monkeypatch.setattr(_ops, "CHUNK", 64)
    ts = [torch.zeros(n) for n in (1, 64, 65, 19200, 7)]
    first, owner, ntensors, nchunks = _ops.build_tensor_index([(t,) for t in ts], "cpu")
    counts = [len(_ops._chunks(t.numel())) for t in ts]
    assert counts == [1, 1, 2, 300, 1] and ntensors == 5 and nchunks == sum(counts)
    assert first.dtype == torch.int32 and owner.dtype == torch.int32
    assert first.tolist() == [0, 1, 2, 4, 304, 305]
    assert owner.tolist() == [i for i, c in enumerate(counts) for _ in range(c)]
    with pytest.raises(ValueError, match="without elements"):
        _ops.build_tensor_index([(torch.zeros(0),)], "cpu")


def test_abi_is_still_18_and_the_entry_points_are_exported():
    assert _lib.ABI_VERSION == 18 and _lib.load().vit_abi_version() == 18
    assert {"vit_lamb_moments", "vit_lamb_trust", "vit_lamb_update"} <= set(_lib.EXPORTED_SYMBOLS)


def test_host_abi_lamb_checker_c(tmp_path):
    """tests/host_abi_lamb_check.c (gcc, no GPU): the ABI is still 18, and every new entry point refuses a NULL table,
    partial, index or trust pointer, a count <= 0 and a bias correction outside (0, 1], each with a message."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_lamb_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_lamb_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


def test_train_with_lamb_on_the_host_path(tmp_path, monkeypatch):
    """train(opt="lamb", no_decay_1d=True, ...) on the host path: two steps, the usual checkpoint keys, two groups in
    the optimizer state, and a state torch.optim.AdamW loads."""
    import train as T
    monkeypatch.setattr(T, "device", "cpu")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = _micro()
    loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, 32, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(4, 3, 32, 10, seed=4), batch_size=4)

    def run(name, **kw):
        T.train(cfg, loader, test_loader, epochs=0, eval_iter=1, log_dir=str(tmp_path / name),
                checkpoint_dir=str(tmp_path / (name + "_ck")), lr=1e-3, **kw)
        return torch.load(tmp_path / (name + "_ck") / "0.pt", map_location="cpu", weights_only=True)

    plain = run("plain")
    ck = run("lamb", opt="lamb", weight_decay=0.05, no_decay_1d=True, max_grad_norm=1.0, trust_clip=True)
    assert set(ck) == set(plain) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
    groups = ck["optimizer_state_dict"]["param_groups"]
    assert [g["weight_decay"] for g in groups] == [0.0, 0.05] and all(g["trust_clip"] is True for g in groups)
    assert all(not torch.equal(ck["model_state_dict"][k], plain["model_state_dict"][k])
               for k in ck["model_state_dict"] if ck["model_state_dict"][k].numel() > 1)
    model = vit.VisionTransformer(cfg)
    model.load_state_dict(ck["model_state_dict"])
    t = torch.optim.AdamW(param_groups_weight_decay(model, 0.05), lr=1e-3)
    t.load_state_dict(ck["optimizer_state_dict"])
    assert all(int(t.state[p]["step"]) == 2 for p in model.parameters())
    sec, last = T.time_steps(cfg, 1, 0, dev="cpu", opt="lamb", no_decay_1d=True)      # --bench can time a LAMB step
    assert sec > 0 and math.isfinite(last)
