"""CPU-only checks of the learning-rate schedule and the layer-wise decay groups: optim.LRSchedule against its closed
forms in fp64, its state and refusals, optim.param_groups_layer_decay on the real model, make_optimizer's and
train()'s unchanged defaults, train() with a cosine schedule on the host path (logged rates, resume), the group maps
_ops.build_group_index cuts, and tests/host_abi_groups_check.c (ABI still 18, sizeof(vit_opt_group), and the argument
checks of the four grouped entry points, no GPU)."""
import json
import math
import os
import shutil
import subprocess

import pytest
import torch

from VisionTransformer import _lib, _ops, config, vit
from VisionTransformer.optim import (FusedAdamW, FusedLamb, LRSchedule, make_optimizer, param_groups_layer_decay,
                                     param_groups_weight_decay)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def closed_form(kind, base, t, N, W, warmup_lr, min_lr):
    """Section 4 of the issue, restated: the rate of update t (0-based) in Python doubles."""
    if t < W:
        return warmup_lr + (base - warmup_lr) * t / W
    if kind == "constant":
        return base
    if t >= N:
        return min_lr
    return min_lr + 0.5 * (base - min_lr) * (1 + math.cos(math.pi * (t - W) / (N - W)))


def _opt(scales=(1.0, 0.5, 0.125), lr=0.02):
    ps = [torch.nn.Parameter(torch.ones(3)) for _ in scales]
    groups = [{"params": [p], "lr_scale": s} if s is not None else {"params": [p]} for p, s in zip(ps, scales)]
    return torch.optim.AdamW(groups, lr=lr)


@pytest.mark.parametrize("kind", ["constant", "cosine"])
@pytest.mark.parametrize("N,W", [(20, 5), (20, 0), (7, 7), (1, 0), (12, 1)])
def test_schedule_values_equal_the_closed_forms(kind, N, W):
    base, warmup_lr, min_lr = 0.02, 1e-5, 3e-4
    scales = (None, 0.5, 0.75 ** 3)
    opt = _opt(scales, base)
    s = LRSchedule(opt, kind, N, warmup_steps=W, warmup_lr=warmup_lr, min_lr=min_lr)
    assert s.t == 0 and all(g["initial_lr"] == base for g in opt.param_groups)
    points = sorted({t for t in (0, W - 1, W, W + 1, N - 1, N, N + 5) if t >= 0})
    for t in points:
        s.set_step(t)
        want = closed_form(kind, base, t, N, W, warmup_lr, min_lr)
        for g, sc in zip(opt.param_groups, scales):
            assert g["lr"] == want * (1.0 if sc is None else sc), (t, sc)      # the same doubles, the same operations
        assert s.last_lr() == want and s.t == t
    # step() walks the same values one update at a time
    s.set_step(0)
    for t in range(N + 3):
        assert opt.param_groups[0]["lr"] == closed_form(kind, base, t, N, W, warmup_lr, min_lr), t
        s.step()
    assert s.t == N + 3
    # the shape: the warmup starts at warmup_lr and rises, the cosine falls to min_lr, constant holds the base
    if W > 0:
        assert closed_form(kind, base, 0, N, W, warmup_lr, min_lr) == warmup_lr
    assert closed_form(kind, base, W, N, W, warmup_lr, min_lr) == pytest.approx(
        base if (kind == "constant" or W < N) else min_lr, rel=1e-15)
    assert closed_form(kind, base, N + 5, N, W, warmup_lr, min_lr) == (base if kind == "constant" else min_lr)


def test_schedule_state_round_trip_and_initial_lr_survives_load_state_dict():
    opt = _opt()
    s = LRSchedule(opt, "cosine", 30, warmup_steps=4, warmup_lr=1e-6, min_lr=1e-5)
    for _ in range(9):
        s.step()
    assert s.state_dict() == {"t": 9}
    lrs = [g["lr"] for g in opt.param_groups]
    sd = opt.state_dict()
    assert all(g["initial_lr"] == 0.02 and "lr_scale" in g for g in sd["param_groups"])
    # a fresh optimizer at another rate: load_state_dict brings lr, initial_lr and lr_scale back with the groups
    opt2 = _opt(lr=0.5)
    opt2.load_state_dict(sd)
    s2 = LRSchedule(opt2, "cosine", 30, warmup_steps=4, warmup_lr=1e-6, min_lr=1e-5)
    assert all(g["initial_lr"] == 0.02 for g in opt2.param_groups) and s2.t == 0
    s2.load_state_dict(s.state_dict())
    assert s2.t == 9 and [g["lr"] for g in opt2.param_groups] == lrs
    s.step()
    s2.step()
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups]
    # the fused optimizers carry the keys alike (constructing them needs no GPU); fuse_groups is no group key
    for cls in (FusedAdamW, FusedLamb):
        f = cls([{"params": [torch.nn.Parameter(torch.ones(2))], "lr_scale": 0.5}], lr=0.1, fuse_groups=True)
        LRSchedule(f, "constant", 10)
        g = f.state_dict()["param_groups"][0]
        assert g["lr"] == 0.05 and g["initial_lr"] == 0.1 and g["lr_scale"] == 0.5 and "fuse_groups" not in g
        assert f.fuse_groups is True and cls([torch.nn.Parameter(torch.ones(2))]).fuse_groups is False


def test_schedule_refusals():
    opt = _opt()
    with pytest.raises(ValueError, match="kind"):
        LRSchedule(opt, "linear", 10)
    with pytest.raises(ValueError, match="exceeds"):
        LRSchedule(opt, "cosine", 10, warmup_steps=11)
    for kw in (dict(total_steps=-1), dict(total_steps=5, warmup_steps=-1), dict(total_steps=5, warmup_lr=-1e-3),
               dict(total_steps=5, min_lr=-1e-3)):
        with pytest.raises(ValueError, match="negative"):
            LRSchedule(opt, "cosine", **kw)
    assert all("initial_lr" not in g for g in opt.param_groups)      # a refused constructor touched nothing


def _tiny(blocks):
    D, H, _ = config.PRESETS["tiny"]
    return vit.VisionTransformer(config.ViTConfig(3, 10, 4, D, 16, H, blocks, "cpu", 2))


@pytest.mark.parametrize("L", [2, 12])
def test_param_groups_layer_decay_on_the_real_model(L):
    m = _tiny(L)
    frozen = m.mlp[3].bias
    frozen.requires_grad_(False)
    names = {id(p): k for k, p in m.named_parameters()}
    decay = 0.75
    groups = param_groups_layer_decay(m, 0.05, decay)

    def layer_of(name):
        if name.startswith("emdeddings."):
            return 0
        if name.startswith("transformer_encoder.blocks."):
            return int(name.split(".")[2]) + 1
        return L + 1

    seen, order = [], []
    for g in groups:
        assert g["params"] and set(g) == {"params", "weight_decay", "lr_scale"}
        layers = {layer_of(names[id(p)]) for p in g["params"]}
        assert len(layers) == 1
        (i,) = layers
        assert g["lr_scale"] == decay ** (L + 1 - i)
        assert g["weight_decay"] in (0.0, 0.05)
        order.append((i, g["weight_decay"] != 0.0))
        seen += [names[id(p)] for p in g["params"]]
    assert order == sorted(order) and len(set(order)) == len(order)          # ascending layers, no-decay first
    assert len(groups) == 2 * (L + 2)                                         # every layer has both kinds
    assert groups[-1]["lr_scale"] == 1.0 and groups[0]["lr_scale"] == decay ** (L + 1)
    assert len(seen) == len(set(seen)) and names[id(frozen)] not in seen
    assert set(seen) == {k for k, p in m.named_parameters() if p.requires_grad}
    assert {"emdeddings.cls_tkn_embd", "emdeddings.pos_embd", "emdeddings.sequence.0.weight"} <= set(
        names[id(p)] for g in groups[:2] for p in g["params"])
    assert all(names[id(p)].startswith("mlp.") for g in groups[-2:] for p in g["params"])
    # for every weight-decay value the union of the groups is param_groups_weight_decay's set
    plain, dec = param_groups_weight_decay(m, 0.05)
    for ref in (plain, dec):
        mine = [id(p) for g in groups if g["weight_decay"] == ref["weight_decay"] for p in g["params"]]
        assert sorted(mine) == sorted(id(p) for p in ref["params"])
    # no_decay is passed through; layer_decay = 1 scales nothing; the bounds
    g2 = param_groups_layer_decay(m, 0.05, 1.0, no_decay=())
    assert all(g["lr_scale"] == 1.0 for g in g2)
    assert "emdeddings.pos_embd" in {names[id(p)] for g in g2 if g["weight_decay"] for p in g["params"]}
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="layer_decay"):
            param_groups_layer_decay(m, 0.05, bad)
    # a layer with nothing trainable leaves no empty group behind
    for p in m.emdeddings.parameters():
        p.requires_grad_(False)
    g3 = param_groups_layer_decay(m, 0.05, decay)
    assert len(g3) == 2 * (L + 1) and all(g["params"] for g in g3)


def test_make_optimizer_defaults_are_unchanged():
    p = torch.nn.Parameter(torch.ones(4))
    assert type(make_optimizer([p], device="cpu")) is torch.optim.AdamW
    assert type(make_optimizer([p], device="cpu", fuse_groups=True)) is torch.optim.AdamW      # ignored on the host
    assert make_optimizer([p], device="cpu", opt="lamb", fuse_groups=True).param_groups[0]["lr"] == 1e-4
    for opt, cls in (("adamw", FusedAdamW), ("lamb", FusedLamb)):
        o = make_optimizer([p], device="cuda", opt=opt)
        assert type(o) is cls and o.fuse_groups is False
        assert make_optimizer([p], device="cuda", opt=opt, fuse_groups=True).fuse_groups is True
        keys = {"params", "lr", "betas", "eps", "weight_decay"} | ({"always_adapt", "trust_clip"} if opt == "lamb"
                                                                  else set())
        assert {k for k in o.param_groups[0] if k in keys or "lr" in k or "fuse" in k} == keys
        assert not {"initial_lr", "lr_scale", "fuse_groups"} & set(o.state_dict()["param_groups"][0])
    assert make_optimizer([p], device="cuda").defaults == dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                                                               weight_decay=1e-4)


def test_group_index_is_cut_like_the_chunk_table(monkeypatch):
    monkeypatch.setattr(_ops, "CHUNK", 64)
    ts = [torch.zeros(n) for n in (1, 64, 65, 200, 7)]
    of_chunk, of_tensor, bounds = _ops.build_group_index([(t,) for t in ts], [2, 0, 1, 2], "cpu")
    assert of_chunk.dtype == torch.int32 and of_tensor.dtype == torch.int32
    assert of_tensor.tolist() == [0, 0, 2, 3, 3]
    assert of_chunk.tolist() == [0, 0, 2, 2, 3, 3, 3, 3, 3]
    assert bounds == [(0, 0), (2, 2), (2, 2), (3, 4), (5, 9)]
    # past OPT_MAX_GROUPS the indices wrap: a launch takes the 64 groups of its span alone
    many = [(torch.zeros(1),) for _ in range(70)]
    of_chunk, _, bounds = _ops.build_group_index(many, [1] * 70, "cpu")
    assert of_chunk.tolist() == [k % 64 for k in range(70)] and bounds[64] == (64, 64) and bounds[-1] == (70, 70)
    with pytest.raises(ValueError, match="add up"):
        _ops.build_group_index(many, [1] * 69, "cpu")
    with pytest.raises(ValueError, match="1..64"):
        _ops.opt_groups([])
    with pytest.raises(ValueError, match="1..64"):
        _ops.opt_groups([(1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 0)] * 65)
    arr = _ops.opt_groups([(1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 3)])
    assert len(arr) == 1 and arr[0].flags == 3 and arr[0].lr == torch.tensor(1e-3).item()


def test_abi_is_still_18_and_the_entry_points_are_exported():
    import ctypes
    assert _lib.ABI_VERSION == 18 and _lib.load().vit_abi_version() == 18
    assert {"vit_adamw_groups", "vit_lamb_moments_groups", "vit_lamb_trust_groups",
            "vit_lamb_update_groups"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.OptGroup) == 32 and _lib.OPT_MAX_GROUPS == 64


def test_host_abi_groups_checker_c(tmp_path):
    """tests/host_abi_groups_check.c (gcc, no GPU): the ABI is still 18, sizeof(vit_opt_group) is 32, and every new
    entry point refuses NULLs, ngroups 0 and 65, a bad bias correction, and flags in the AdamW form."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_groups_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_groups_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


def _scalars(log_dir, tag):
    with open(os.path.join(log_dir, "scalars.jsonl")) as f:
        rows = [json.loads(line) for line in f]
    return [(r["step"], r["value"]) for r in rows if r["tag"] == tag]


def test_train_on_the_host_path_defaults_schedule_and_resume(tmp_path, monkeypatch):
    """train() with none of the new keywords keeps today's optimizer groups and checkpoint keys; with sched="cosine"
    the logged LR/train_batch values are the formula's, the checkpoint holds "lr_schedule", and a resumed run goes on
    at the right t; layer_decay alone takes a constant schedule and param_groups_layer_decay's groups."""
    import train as T
    monkeypatch.setattr(T, "device", "cpu")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = config.ViTConfig(3, 10, 4, 64, 16, 4, 2, "cpu", 4)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(12, 3, 32, 10, seed=3), batch_size=4, drop_last=True)

    def run(name, epochs=0, **kw):
        T.train(cfg, loader, None, epochs=epochs, eval_iter=1, log_dir=str(tmp_path / name),
                checkpoint_dir=str(tmp_path / (name + "_ck")), lr=1e-3, **kw)
        return torch.load(tmp_path / (name + "_ck") / f"{epochs}.pt", map_location="cpu", weights_only=True)

    plain = run("plain")
    assert set(plain) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
    (g,) = plain["optimizer_state_dict"]["param_groups"]
    assert not {"initial_lr", "lr_scale"} & set(g) and g["lr"] == 1e-3
    assert _scalars(str(tmp_path / "plain"), "LR/train_batch") == []

    # 2 epochs x 3 steps = 6 optimizer steps; 2 of warmup
    N, W, kw = 6, 2, dict(sched="cosine", warmup_steps=2, warmup_lr=1e-5, min_lr=1e-4)
    first = run("cos", epochs=0, **kw)            # one epoch of a run planned for one: N = 3
    want3 = [closed_form("cosine", 1e-3, t, 3, W, 1e-5, 1e-4) for t in range(3)]
    assert _scalars(str(tmp_path / "cos"), "LR/train_batch") == [(t, v) for t, v in enumerate(want3)]
    assert set(first) == set(plain) | {"lr_schedule"} and first["lr_schedule"] == {"t": 3} and first["step"] == 3
    (g,) = first["optimizer_state_dict"]["param_groups"]
    assert g["initial_lr"] == 1e-3 and g["lr"] == closed_form("cosine", 1e-3, 3, 3, W, 1e-5, 1e-4) == 1e-4
    # resumed with epochs=1 (N = 6): epoch 0 runs again, as the reference's loop does, at t = 3, 4, 5, then epoch 1
    os.rename(tmp_path / "cos_ck", tmp_path / "cos2_ck")
    second = run("cos2", epochs=1, **kw)
    got = _scalars(str(tmp_path / "cos2"), "LR/train_batch")
    assert got == [(t, closed_form("cosine", 1e-3, t, N, W, 1e-5, 1e-4)) for t in range(3, 9)]
    assert second["lr_schedule"] == {"t": 9} and second["step"] == 9

    ld = run("ld", layer_decay=0.5, weight_decay=0.05)
    groups = ld["optimizer_state_dict"]["param_groups"]
    assert len(groups) == 2 * (cfg.num_blocks + 2) and ld["lr_schedule"] == {"t": 3}
    assert [g["lr"] for g in groups] == [1e-3 * g["lr_scale"] for g in groups]
    assert groups[0]["lr_scale"] == 0.5 ** 3 and groups[-1]["lr_scale"] == 1.0
    assert _scalars(str(tmp_path / "ld"), "LR/train_batch") == [(t, 1e-3) for t in range(3)]
    with pytest.raises(ValueError, match="belong to a schedule"):
        run("bad", warmup_steps=2)
    sec, last = T.time_steps(cfg, 1, 0, dev="cpu", layer_decay=0.75, fuse_groups=True)      # --bench takes them too
    assert sec > 0 and math.isfinite(last)
