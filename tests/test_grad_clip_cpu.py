"""CPU-only checks of global-norm gradient clipping: the host optimizer make_optimizer(device="cpu",
max_grad_norm=...) against clip_grad_norm_ + torch.optim.AdamW, its non-finite skip, the argument checks of the three
C-ABI entry points (dlopen only, no launch), and train.py's --clip-grad-norm on the host path."""
import copy
import ctypes
import json
import os
import sys

import pytest
import torch

from VisionTransformer import _lib, config, vit
from VisionTransformer.optim import ClippedAdamW, cross_entropy, make_optimizer


def _micro():
    return config.ViTConfig(3, 10, 4, 64, 16, 4, 2, "cpu", 4)


def _batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)


def _backward(m, x, y):
    for p in m.parameters():
        p.grad = None
    cross_entropy(m(x), y).backward()


def test_host_optimizer_equals_clip_grad_norm_then_adamw():
    torch.manual_seed(0)
    m = vit.VisionTransformer(_micro()).eval()          # eval: no dropout draw, so the twin sees the same gradients
    twin = copy.deepcopy(m)
    x, y = _batch()
    _backward(m, x, y)
    norm0 = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m.parameters())))
    max_norm = 0.5 * norm0                               # the first step clips for certain
    opt = make_optimizer(m.parameters(), lr=1e-3, weight_decay=1e-4, device="cpu", max_grad_norm=max_norm)
    assert isinstance(opt, ClippedAdamW) and "max_grad_norm" not in opt.param_groups[0]
    ref = torch.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=1e-4)
    norms = []
    for step in range(3):
        _backward(m, x, y)
        _backward(twin, x, y)
        want = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
        ref.step()
        opt.step()
        assert torch.equal(opt.grad_norm(), want), step
        norms.append(opt.grad_norm())
        for (k, a), b in zip(m.named_parameters(), twin.parameters()):
            assert torch.equal(a, b), (step, k)
    assert float(norms[0]) > max_norm and abs(float(norms[0]) - norm0) < 1e-5 * norm0
    assert float(opt.skipped_steps()) == 0
    # torch AdamW's state_dict, loadable by it
    torch.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=1e-4).load_state_dict(opt.state_dict())


def test_host_optimizer_skips_a_nonfinite_step_and_resumes():
    torch.manual_seed(1)
    m = vit.VisionTransformer(_micro()).eval()
    x, y = _batch()
    opt = make_optimizer(m.parameters(), lr=1e-3, weight_decay=1e-4, device="cpu", max_grad_norm=1.0)
    _backward(m, x, y)
    opt.step()                                           # a finite step first, so the moments exist
    before = [p.detach().clone() for p in m.parameters()]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for p in m.parameters()]
    _backward(m, x, y)
    last = list(m.parameters())[-1]
    last.grad.view(-1)[0] = float("inf")
    opt.step()
    assert float(opt.skipped_steps()) == 1 and not bool(torch.isfinite(opt.grad_norm()))
    for p, b, s in zip(m.parameters(), before, state):
        assert torch.equal(p, b)
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], s[k]), k
    _backward(m, x, y)
    opt.step()
    assert float(opt.skipped_steps()) == 1 and bool(torch.isfinite(opt.grad_norm()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert all(not torch.equal(p, b) for p, b in zip(m.parameters(), before))


def test_host_optimizer_without_skip_follows_torch():
    """skip_nonfinite=False: the step runs with clip_grad_norm_'s coefficient, as plain torch code would."""
    p = torch.nn.Parameter(torch.ones(4))
    opt = make_optimizer([p], device="cpu", max_grad_norm=1.0, skip_nonfinite=False)
    p.grad = torch.tensor([1.0, float("nan"), 0.0, 2.0])
    opt.step()
    assert float(opt.skipped_steps()) == 0 and not bool(torch.isfinite(p).all())


def test_no_max_grad_norm_is_plain_adamw():
    p = torch.nn.Parameter(torch.ones(4))
    assert type(make_optimizer([p], device="cpu")) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", max_grad_norm=None)) is torch.optim.AdamW
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            make_optimizer([p], device="cpu", max_grad_norm=bad)


def test_fused_optimizer_keeps_max_grad_norm_out_of_param_groups():
    """Constructing FusedAdamW needs no GPU: the keyword is an attribute, and state_dict() has torch AdamW's keys."""
    from VisionTransformer.optim import FusedAdamW
    p = torch.nn.Parameter(torch.ones(4))
    opt = FusedAdamW([p], max_grad_norm=1.0, skip_nonfinite=False)
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is False
    assert set(opt.param_groups[0]) == set(FusedAdamW([p]).param_groups[0])
    assert FusedAdamW([p]).max_grad_norm is None
    assert set(opt.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW([p], max_grad_norm=0.0)


def test_entry_points_refuse_bad_arguments():
    """Every new entry point returns VIT_ERR_INVALID, with a message that names it, before any launch."""
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))         # a non-null pointer; refused calls never dereference it
    adam = (1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.1, 0.001, 1.0, _lib.F32)
    cases = [
        ("vit_grad_sumsq", (None, 1, 1.0, ptr, None)),
        ("vit_grad_sumsq", (ptr, 1, 1.0, None, None)),
        ("vit_grad_sumsq", (ptr, 0, 1.0, ptr, None)),
        ("vit_grad_sumsq", (ptr, -3, 1.0, ptr, None)),
        ("vit_grad_clip_finish", (None, 1, 1.0, ptr, None)),
        ("vit_grad_clip_finish", (ptr, 1, 1.0, None, None)),
        ("vit_grad_clip_finish", (ptr, 0, 1.0, ptr, None)),
        ("vit_grad_clip_finish", (ptr, 1, 0.0, ptr, None)),
        ("vit_grad_clip_finish", (ptr, 1, float("nan"), ptr, None)),
        ("vit_adamw_clipped", (None, 1) + adam + (ptr, None)),
        ("vit_adamw_clipped", (ptr, 1) + adam + (None, None)),
        ("vit_adamw_clipped", (ptr, 0) + adam + (ptr, None)),
    ]
    for name, args in cases:
        assert getattr(lib, name)(*args) == 1, (name, args)          # VIT_ERR_INVALID
        assert name in lib.vit_last_error().decode(), (name, lib.vit_last_error())


def test_train_main_clip_grad_norm_on_cpu(tmp_path, monkeypatch, capsys):
    import train as T
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)    # the package's own JSONL writer, readable without tensorboard
    threads = torch.get_num_threads()
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "2",
                                      "--steps", "2", "--epochs", "0", "--train-size", "4", "--test-size", "2",
                                      "--workers", "0", "--threads", "2", "--clip-grad-norm", "0.5", "--log-dir", logs,
                                      "--checkpoint-dir", ck])
    try:
        T.main()
    finally:
        torch.set_num_threads(threads)
    recs = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    norms = [r for r in recs if r["tag"] == "GradNorm/train_batch"]
    losses = [r for r in recs if r["tag"] == "Loss/train_batch"]
    assert [r["step"] for r in norms] == [0, 1] == [r["step"] for r in losses]
    assert all(r["value"] > 0 and r["value"] == r["value"] for r in norms)
    assert "steps skipped for a non-finite gradient norm: 0" in capsys.readouterr().out
    assert os.path.exists(os.path.join(ck, "0.pt"))
