"""CPU-only checks of the weight EMA kept inside the optimizer step: the host optimizer make_optimizer(device="cpu",
ema_decay=...) — its recurrence against fp64, swap / context semantics, the non-finite skip, ema_state_dict, the
state-dict round trip through torch.optim.AdamW —, the ema_decay validation of both optimizer classes, train()'s
checkpoint key on the host path, and tests/host_abi_ema_check.c (ABI 18 and the argument checks of the two new entry
points, no GPU)."""
import copy
import os
import shutil
import subprocess

import pytest
import torch

from VisionTransformer import _lib, config, vit
from VisionTransformer.optim import ClippedAdamW, EmaAdamW, FusedAdamW, cross_entropy, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-3, 1e-4
# One EMA update e + w * (p - e) in fp32 with w = fl32(1 - decay) <= 0.5: the rounding of w (w * 2^-24 relative, on a
# product of at most w * 2M), the subtraction (2^-24 * 2M), the product (2^-24 * 2wM) and the sum (2^-24 * M) stay
# below (1 + 6w) * 2^-24 * M <= 2^-22 * M with M = max(|e_prev|, |p_new|).
GATE = 2.0 ** -22


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


def _gate_ratio(e, e_prev, p_new, decay):
    """max over elements of |e - ref| / max(|e_prev|, |p_new|), ref = e_prev + (1 - decay) * (p_new - e_prev) in
    fp64 (0 where both are 0 and e is too)."""
    ref = e_prev.double() + (1.0 - decay) * (p_new.double() - e_prev.double())
    big = torch.maximum(e_prev.abs(), p_new.abs()).double()
    err = (e.double() - ref).abs()
    assert bool((err[big == 0] == 0).all())
    return float((err[big > 0] / big[big > 0]).max()) if bool((big > 0).any()) else 0.0


@pytest.mark.parametrize("max_grad_norm", [None, 0.05], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_host_recurrence_against_fp64(decay, max_grad_norm):
    m = _model()
    twin = copy.deepcopy(m)
    x, y = _batch()
    opt = make_optimizer(m.parameters(), lr=LR, weight_decay=WD, device="cpu", ema_decay=decay,
                         max_grad_norm=max_grad_norm)
    ref = make_optimizer(twin.parameters(), lr=LR, weight_decay=WD, device="cpu", max_grad_norm=max_grad_norm)
    assert isinstance(opt, EmaAdamW) and opt.ema_decay == decay and "ema_decay" not in opt.param_groups[0]
    assert isinstance(ref, ClippedAdamW if max_grad_norm else torch.optim.AdamW)
    worst = 0.0
    for step in range(3):
        _backward(m, x, y)
        _backward(twin, x, y)
        # ema_0 is the weights before the first update
        prev = [opt.state[p]["ema"].clone() if "ema" in opt.state[p] else p.detach().clone() for p in m.parameters()]
        opt.step()
        ref.step()
        for (k, p), q, e_prev in zip(m.named_parameters(), twin.parameters(), prev):
            assert torch.equal(_bits(p), _bits(q)), (step, k)        # the EMA leaves AdamW alone
            e = opt.state[p]["ema"]
            assert e.dtype == torch.float32 and e.is_contiguous() and e.shape == p.shape
            worst = max(worst, _gate_ratio(e, e_prev, p.detach(), decay))
    print(f"decay {decay}: worst |e - ref| / max(|e_prev|, |p_new|) = {worst:.3e} (gate {GATE:.3e})")
    assert worst <= GATE
    if max_grad_norm:
        assert float(opt.grad_norm()) > max_grad_norm and float(opt.skipped_steps()) == 0
    assert all(not torch.equal(opt.state[p]["ema"], p) for p in m.parameters() if p.numel() > 1)


def _stepped(decay=0.9, steps=2, **kw):
    m = _model(1)
    x, y = _batch()
    opt = make_optimizer(m.parameters(), lr=LR, weight_decay=WD, device="cpu", ema_decay=decay, **kw)
    for _ in range(steps):
        _backward(m, x, y)
        opt.step()
    return m, opt, x, y


def test_swap_and_context_semantics():
    m, opt, x, y = _stepped()
    ps = list(m.parameters())
    p0 = [p.detach().clone() for p in ps]
    e0 = [opt.state[p]["ema"].clone() for p in ps]
    opt.swap_ema()
    assert all(torch.equal(_bits(p), _bits(e)) for p, e in zip(ps, e0))
    assert all(torch.equal(_bits(opt.state[p]["ema"]), _bits(q)) for p, q in zip(ps, p0))
    _backward(m, x, y)
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.step()
    with pytest.raises(RuntimeError, match="already swapped in"):
        with opt.ema_weights():
            pass
    opt.swap_ema()
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(ps, p0))
    assert all(torch.equal(_bits(opt.state[p]["ema"]), _bits(e)) for p, e in zip(ps, e0))
    # the context manager: EMA inside, step() and nesting refused, restored afterwards — also after an exception
    with opt.ema_weights():
        assert all(torch.equal(_bits(p), _bits(e)) for p, e in zip(ps, e0))
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
        with pytest.raises(RuntimeError, match="already swapped in"):
            with opt.ema_weights():
                pass
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(ps, p0))
    with pytest.raises(KeyError, match="boom"):
        with opt.ema_weights():
            raise KeyError("boom")
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(ps, p0))
    assert all(torch.equal(_bits(opt.state[p]["ema"]), _bits(e)) for p, e in zip(ps, e0))
    opt.step()                                           # and the optimizer steps again


def test_skipped_step_leaves_the_ema_alone():
    m, opt, x, y = _stepped(max_grad_norm=1.0)
    ps = list(m.parameters())
    before = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in ps]
    _backward(m, x, y)
    ps[-1].grad.view(-1)[0] = float("inf")
    opt.step()
    assert float(opt.skipped_steps()) == 1 and not bool(torch.isfinite(opt.grad_norm()))
    for p, (b, st) in zip(ps, before):
        assert torch.equal(_bits(p), _bits(b))
        assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
        for k, v in st.items():
            assert torch.equal(opt.state[p][k], v), k
    _backward(m, x, y)
    opt.step()                                           # a finite step afterwards moves both again
    assert float(opt.skipped_steps()) == 1
    assert all(not torch.equal(opt.state[p]["ema"], st["ema"]) for p, (_, st) in zip(ps, before) if p.numel() > 1)


def test_ema_state_dict():
    m, opt, _, _ = _stepped()
    frozen = list(m.parameters())[0]
    del opt.state[frozen]["ema"]                        # a parameter without an EMA keeps its own value
    sd, esd = m.state_dict(), opt.ema_state_dict(m)
    assert list(esd) == list(sd)
    names = dict(m.named_parameters())
    for k, v in esd.items():
        if k in names and names[k] is not frozen:
            e = opt.state[names[k]]["ema"]
            assert torch.equal(_bits(v), _bits(e)) and v.data_ptr() != e.data_ptr() and not torch.equal(v, sd[k])
        else:
            assert torch.equal(v, sd[k])
    fresh = vit.VisionTransformer(_micro())
    fresh.load_state_dict(esd)                           # a loadable state_dict
    with opt.ema_weights():                              # swapped in, the parameters hold those values: same answer
        inside = opt.ema_state_dict(m)
    assert all(torch.equal(_bits(inside[k]), _bits(esd[k])) for k in esd)


def test_state_dict_round_trip_through_torch_adamw():
    m, opt, x, y = _stepped()
    ps = list(m.parameters())
    emas = [opt.state[p]["ema"].clone() for p in ps]
    assert set(opt.state_dict()["param_groups"][0]) == set(
        torch.optim.AdamW(ps, lr=LR, weight_decay=WD).state_dict()["param_groups"][0])
    t = torch.optim.AdamW(ps, lr=LR, weight_decay=WD)
    t.load_state_dict(opt.state_dict())
    _backward(m, x, y)
    t.step()                                             # torch carries the key along and ignores it
    assert all(torch.equal(t.state[p]["ema"], e) for p, e in zip(ps, emas))
    back = make_optimizer(ps, lr=LR, weight_decay=WD, device="cpu", ema_decay=0.9)
    back.load_state_dict(t.state_dict())
    assert all(torch.equal(back.state[p]["ema"], e) for p, e in zip(ps, emas))
    before = [p.detach().clone() for p in ps]
    _backward(m, x, y)
    back.step()
    assert max(_gate_ratio(back.state[p]["ema"], e, p.detach(), 0.9) for p, e in zip(ps, emas)) <= GATE
    # a torch AdamW state without "ema": cloned from the weights as they stand at the next step
    plain = torch.optim.AdamW(ps, lr=LR, weight_decay=WD)
    _backward(m, x, y)
    plain.step()
    late = make_optimizer(ps, lr=LR, weight_decay=WD, device="cpu", ema_decay=0.9)
    late.load_state_dict(plain.state_dict())
    assert all("ema" not in late.state[p] for p in ps)
    before = [p.detach().clone() for p in ps]
    _backward(m, x, y)
    late.step()
    assert max(_gate_ratio(late.state[p]["ema"], b, p.detach(), 0.9) for p, b in zip(ps, before)) <= GATE
    assert all(int(late.state[p]["step"]) == 2 for p in ps)


@pytest.mark.parametrize("bad", [0, 1, 0.0, 1.0, -0.1, 1.5, float("nan")])
def test_ema_decay_is_validated(bad):
    p = torch.nn.Parameter(torch.ones(4))
    with pytest.raises(ValueError, match="ema_decay"):
        make_optimizer([p], device="cpu", ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        EmaAdamW([p], bad)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW([p], ema_decay=bad)                   # constructing it needs no GPU
    opt = make_optimizer([p], device="cpu", ema_decay=0.5)
    opt.ema_decay = bad                                  # the attribute may be changed between steps: checked there
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()


def test_ema_decay_is_an_attribute_and_off_by_default():
    p = torch.nn.Parameter(torch.ones(4))
    assert type(make_optimizer([p], device="cpu")) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", ema_decay=None)) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", max_grad_norm=1.0, ema_decay=None)) is ClippedAdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        make_optimizer([p], device="cpu", ema_decay=0.9, max_grad_norm=0.0)
    opt = FusedAdamW([p], ema_decay=0.999)
    assert opt.ema_decay == 0.999 and FusedAdamW([p]).ema_decay is None
    assert set(opt.param_groups[0]) == set(FusedAdamW([p]).param_groups[0])
    assert set(opt.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
    assert opt.state_dict()["state"] == {}


def test_abi_18_and_exports():
    assert _lib.ABI_VERSION == 18 and _lib.load().vit_abi_version() == 18
    assert {"vit_adamw_ema", "vit_ema_swap"} <= set(_lib.EXPORTED_SYMBOLS)


def test_host_abi_ema_checker_c(tmp_path):
    """tests/host_abi_ema_check.c (gcc, no GPU): ABI 18, and both new entry points refuse a NULL table, a NULL EMA
    array, nchunks = 0 and (vit_adamw_ema) a weight of 0 or 1, each with a vit_last_error() message."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_ema_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_ema_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


def test_train_saves_the_ema_on_the_host_path(tmp_path, monkeypatch):
    """train(..., ema_decay=...) on the host path: the checkpoint gains "ema_state_dict", equal to what the restored
    optimizer state gives and different from the trained weights; without the keyword the key set is unchanged."""
    import train as T
    monkeypatch.setattr(T, "device", "cpu")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = _micro()
    loader = torch.utils.data.DataLoader(T.SyntheticImages(12, 3, 32, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(4, 3, 32, 10, seed=4), batch_size=4)

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
    # the weights were swapped back after validation: the same data without an EMA trains to the same weights
    assert all(torch.equal(msd[k], plain["model_state_dict"][k]) for k in msd)
    model = vit.VisionTransformer(cfg)
    model.load_state_dict(msd)
    opt = make_optimizer(model.parameters(), lr=1e-3, weight_decay=1e-4, device="cpu", ema_decay=0.9)
    opt.load_state_dict(ck["optimizer_state_dict"])      # resume: the EMA rides in the optimizer state
    again = opt.ema_state_dict(model)
    assert all(torch.equal(again[k], esd[k]) for k in esd)
