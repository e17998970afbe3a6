"""CPU-only checks of stochastic depth (drop path): the Python twin of the device draw against the oracle's hash
primitives and its statistics, the per-block linspace rule and its validation, the host path's _cpu.drop_path and the
rule that a rate of 0 changes nothing (values, RNG stream), train.py's --drop-path on the host path, and
tests/host_abi_drop_path_check.c (the argument checks of vit_drop_path_rows and vit_gemm_rowscale, ABI still 18)."""
import json
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from oracle import vit_oracle as O
from VisionTransformer import _cpu, _engine, _lib, config, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 195950210          # the base seed torch.manual_seed(42) gives the engine's forward


def _cfg(**kw):
    return config.ViTConfig(3, 10, 4, 64, 16, 4, 3, "cpu", 4, **kw)


# ---- the draw -------------------------------------------------------------------------------------------------------
def test_path_keep_is_the_oracles_hash_on_layers_L_to_2L():
    L, B, rates = 3, 8, [0.0, 0.25, 0.5]
    for l, p in enumerate(rates):
        for site in (0, 1):
            ours = _engine.path_keep(SEED, L, l, site, B, p)
            ref = O.dropout_keep(O.site_seed(SEED, L + l, site), (B,), p)
            assert ours.dtype == torch.bool and torch.equal(ours, ref), (l, site)
    assert bool(_engine.path_keep(SEED, L, 0, 0, B, 0.0).all())          # rate 0 keeps every image
    # the element dropout's streams are layers 0 .. L-1: a different seed for every (layer, site) of both families
    seeds = {_engine.site_seed(SEED, layer, site) for layer in range(2 * L) for site in (0, 1)}
    assert len(seeds) == 4 * L


def test_path_keep_statistics():
    n = 4096
    for p in (0.1, 0.5):
        dropped = 1.0 - _engine.path_keep(SEED, 3, 0, 0, n, p).float().mean().item()
        print(f"p = {p}: dropped share {dropped:.4f}")
        assert abs(dropped - p) <= 4 * math.sqrt(p * (1 - p) / n), (p, dropped)


def test_keep_scale_folds_the_two_rates():
    assert _engine._keep_scale(0.0) == (_engine.DROPOUT_P, 1.0 / (1.0 - _engine.DROPOUT_P))      # today's scalars
    dp, gs = _engine._keep_scale(0.25)
    assert dp == pytest.approx(1 - 0.8 * 0.75, rel=1e-15) and gs == pytest.approx(1 / (0.8 * 0.75), rel=1e-15)


# ---- rates ----------------------------------------------------------------------------------------------------------
def test_linspace_rule_and_validation():
    for rate, L in ((0.1, 12), (0.3, 3), (0.5, 1), (0.0, 4)):
        want = [x.item() for x in torch.linspace(0, rate, L)]
        assert config.drop_path_rates(rate, L) == want
    m = vit.VisionTransformer(_cfg(drop_path_rate=0.3))
    assert m.drop_path_rates == [x.item() for x in torch.linspace(0, 0.3, 3)] and m.vit_config.drop_path_rate == 0.3
    assert vit.VisionTransformer(_cfg()).drop_path_rates == [0.0, 0.0, 0.0] and _cfg().drop_path_rate == 0.0
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="drop_path_rate"):
            _cfg(drop_path_rate=bad)
    with pytest.raises(TypeError):
        _cfg(drop_path_rate="0.1")
    with pytest.raises(TypeError):                       # keyword-only
        config.ViTConfig(3, 10, 4, 64, 16, 4, 3, "cpu", 4, 0.2, torch.float32, None, 0.1)
    m.drop_path_rates = [0.0, 0.5, 0.25]                 # settable
    assert m.drop_path_rates == [0.0, 0.5, 0.25]
    for bad in ([0.1, 0.2], [0.1, 0.2, 1.0], [0.1, -0.2, 0.3], [0.1, float("nan"), 0.3]):
        with pytest.raises(ValueError, match="drop_path_rates"):
            m.drop_path_rates = bad
    assert m.drop_path_rates == [0.0, 0.5, 0.25]         # a refused assignment changes nothing
    m.drop_path_rates[1] = 7.0                           # the getter hands out a copy: no way round the validation
    assert m.drop_path_rates == [0.0, 0.5, 0.25]
    # no parameter, no buffer: the state_dict is the reference's
    assert list(m.state_dict()) == list(vit.VisionTransformer(_cfg()).state_dict())


# ---- the host path --------------------------------------------------------------------------------------------------
def test_cpu_drop_path_slabs_identity_and_rng():
    torch.manual_seed(3)
    y = torch.randn(64, 5, 7)
    p = 0.3
    out = _cpu.drop_path(y, p, True)
    kept = 0
    for b in range(y.shape[0]):
        zero, scaled = bool((out[b] == 0).all()), torch.equal(out[b], y[b] / (1 - p))
        assert zero or scaled, b
        kept += scaled
    assert 0 < kept < y.shape[0]
    assert _cpu.drop_path(y, p, False) is y and _cpu.drop_path(y, 0.0, True) is y
    state = torch.get_rng_state()
    _cpu.drop_path(y, 0.0, True)
    _cpu.drop_path(y, p, False)
    assert torch.equal(torch.get_rng_state(), state)
    _cpu.drop_path(y, p, True)
    assert not torch.equal(torch.get_rng_state(), state)


def test_host_model_rate_zero_is_the_model_without_the_keyword():
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    outs = []
    for kw in ({}, {"drop_path_rate": 0.0}, {"drop_path_rate": 0.4}):
        torch.manual_seed(0)
        m = vit.VisionTransformer(_cfg(**kw)).train()
        torch.manual_seed(7)
        y = m(x)
        y.square().sum().backward()
        outs.append((y.detach(), m.mlp[0].weight.grad.clone(), m))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])       # ... and a rate > 0 does something in train mode,
    m = outs[2][2].eval()
    with torch.no_grad():                                # nothing in eval mode
        assert torch.equal(m(x), outs[0][2].eval()(x))


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_stays_18_with_the_added_exports():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.vit_abi_version() == 18
    assert {"vit_drop_path_rows", "vit_gemm_rowscale"} <= set(_lib.EXPORTED_SYMBOLS)
    assert hasattr(lib, "vit_drop_path_rows") and hasattr(lib, "vit_gemm_rowscale")
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "#define VIT_ABI_VERSION 18" in hdr
    assert f"#define VIT_DROP_PATH_MAX_LAYERS {_lib.DROP_PATH_MAX_LAYERS}\n" in hdr


def test_host_abi_drop_path_checker_c(tmp_path):
    """tests/host_abi_drop_path_check.c (gcc, no GPU): both symbols link, ABI 18, and every refusal — NULL pointers,
    L / B / T <= 0, L above the cap, B * T >= 2^31, a rate outside [0, 1) or NaN, a misaligned row_scale, a descriptor
    vit_gemm refuses — returns VIT_ERR_INVALID with a vit_last_error() message naming the entry point."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_drop_path_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_drop_path_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


# ---- train.py on the host path --------------------------------------------------------------------------------------
def test_train_main_drop_path_on_cpu(tmp_path, monkeypatch):
    import train as T
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    threads = torch.get_num_threads()
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "2",
                                      "--steps", "2", "--epochs", "0", "--train-size", "4", "--test-size", "2",
                                      "--workers", "0", "--threads", "2", "--drop-path", "0.1", "--log-dir", logs,
                                      "--checkpoint-dir", ck])
    seen = []
    real = _cpu.drop_path
    monkeypatch.setattr(_cpu, "drop_path", lambda y, p, training: (seen.append((p, training)), real(y, p, training))[1])
    try:
        T.main()
    finally:
        torch.set_num_threads(threads)
    losses = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    losses = [r["value"] for r in losses if r["tag"] == "Loss/train_batch"]
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    # the flag reached the blocks: the last block trains at the full rate, the first at 0
    L = T.config.PRESETS["tiny"][2]
    train_rates = {p for p, training in seen if training}
    assert train_rates == set(config.drop_path_rates(0.1, L)) and max(train_rates) == pytest.approx(0.1, rel=1e-6)
    with pytest.raises(SystemExit):                      # argparse refuses what is no number ...
        monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cpu", "--drop-path", "oops"])
        T.main()
    for bad in ("1.5", "1.0", "-0.1"):                   # ... and the config a rate outside [0, 1)
        monkeypatch.setattr(sys, "argv", ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch",
                                          "2", "--workers", "0", "--threads", "2", "--drop-path", bad,
                                          "--log-dir", logs, "--checkpoint-dir", ck])
        try:
            with pytest.raises(ValueError, match="drop_path_rate"):
                T.main()
        finally:
            torch.set_num_threads(threads)
