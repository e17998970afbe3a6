"""CPU-only checks of patch dropout: the config keyword and the keep count, the host twin of vit_patch_keep (its
defining properties on every table shape the device test uses, and the uniformity of the draw as a condition), the
host model in training mode against the oracle composed on the kept tokens, the rule that rate 0 and eval mode change
nothing, the module-level patch_embed's `keep`, tests/host_abi_patch_drop_check.c (the argument checks of the five new
entry points, ABI still 18), and train.py --patch-drop on the host path."""
import json
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from oracle import vit_oracle as O
from patch_drop_reference import BASE_SEED, CASES, check_fp32, check_table, oracle_run
from VisionTransformer import _cpu, _engine, _functional, _lib, config, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    return config.ViTConfig(3, 10, 4, 64, 16, 4, 3, "cpu", 4, **kw)


# ---- the keyword and the count --------------------------------------------------------------------------------------
def test_config_keyword():
    assert _cfg().patch_drop_rate == 0.0 and _cfg(patch_drop_rate=0.5).patch_drop_rate == 0.5
    assert _cfg(patch_drop_rate=0).patch_drop_rate == 0.0
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="patch_drop_rate"):
            _cfg(patch_drop_rate=bad)
    for bad in ("0.1", None, True, [0.1]):
        with pytest.raises(TypeError, match="patch_drop_rate"):
            _cfg(patch_drop_rate=bad)
    with pytest.raises(TypeError):                       # keyword-only
        config.ViTConfig(3, 10, 4, 64, 16, 4, 3, "cpu", 4, 0.2, torch.float32, None, 0.0, 0.5)
    assert repr(_cfg(patch_drop_rate=0.5)) == repr(_cfg())
    m = vit.VisionTransformer(_cfg(patch_drop_rate=0.25))
    assert m.patch_drop_rate == 0.25 and m.last_patch_keep is None
    m.patch_drop_rate = 0.5                              # a mutable attribute, validated
    assert m.patch_drop_rate == 0.5
    with pytest.raises(ValueError, match="patch_drop_rate"):
        m.patch_drop_rate = 1.0
    with pytest.raises(TypeError, match="patch_drop_rate"):
        m.patch_drop_rate = "0.5"
    assert m.patch_drop_rate == 0.5                      # a refused assignment changes nothing
    assert vit.VisionTransformer(_cfg()).patch_drop_rate == 0.0
    # no parameter, no buffer: the state_dict is the reference's
    assert list(m.state_dict()) == list(vit.VisionTransformer(_cfg()).state_dict())


def test_patch_keep_count():
    for N in (1, 2, 3, 4, 16, 36, 196, 576, 1024, 4096):
        assert config.patch_keep_count(N, 0.0) == N and config.patch_keep_count(N, 0) == N
        for r in (0.0, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.99, 0.999999):
            assert config.patch_keep_count(N, r) == max(1, int(N * (1 - r))), (N, r)
    assert config.patch_keep_count(196, 0.5) == 98 and config.patch_keep_count(196, 0.25) == 147
    assert config.patch_keep_count(576, 0.5) == 288 and config.patch_keep_count(16, 0.99) == 1
    with pytest.raises(ValueError, match="patch_drop_rate"):
        config.patch_keep_count(16, 1.0)


# ---- the host twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", CASES)
def test_host_twin_properties(B, N, K):
    L = 3
    idx, inv = _cpu.patch_keep_table(BASE_SEED, L, B, N, K)
    check_table(idx, inv, B, N, K)
    again = _cpu.patch_keep_table(BASE_SEED, L, B, N, K)
    assert torch.equal(again[0], idx) and torch.equal(again[1], inv)     # the same seed: the same table
    if 1 < K < N:
        other = _cpu.patch_keep_table(BASE_SEED + 1, L, B, N, K)[0]
        assert not torch.equal(other, idx)                                 # another seed: another
        assert not torch.equal(_cpu.patch_keep_table(BASE_SEED, L + 1, B, N, K)[0], idx)   # (its stream is layer 2L's)
        if B > 1 and N >= 16:
            assert all(not torch.equal(idx[0], idx[b]) for b in range(1, min(B, 8)))        # images differ
        # the rule, literally: n >= 1 is kept iff fewer than K - 1 patches of 1 .. N-1 have a smaller (key, n)
        if N <= 36:
            ps = _engine.site_seed(BASE_SEED, 2 * L, 0)
            for b in range(B):
                keys = [(_engine._hash_u32(ps, b * N + n), n) for n in range(N)]
                kept = [0] + [n for n in range(1, N) if sum(keys[m] < keys[n] for m in range(1, N)) < K - 1]
                assert idx[b].tolist() == kept, b
    with pytest.raises(ValueError, match="patch_keep_table"):
        _cpu.patch_keep_table(BASE_SEED, L, B, N, N + 1)
    with pytest.raises(ValueError, match="patch_keep_table"):
        _cpu.patch_keep_table(BASE_SEED, L, B, N, 0)


def test_host_twin_rank_hashes_into_the_table():
    """Data-parallel ranks differ through dropout_seed, as the dropout masks do."""
    a = _cpu.patch_keep_table(_engine.dropout_seed(BASE_SEED, 0), 2, 4, 16, 8)[0]
    b = _cpu.patch_keep_table(_engine.dropout_seed(BASE_SEED, 1), 2, 4, 16, 8)[0]
    assert torch.equal(a, _cpu.patch_keep_table(BASE_SEED, 2, 4, 16, 8)[0]) and not torch.equal(a, b)


UNIFORMITY_SEED = BASE_SEED   # chosen on the CPU: the host twin meets the band below under this seed (hash fixed)


def test_uniformity_is_a_condition():
    """N 16, K 8, B 4096: every patch 1 .. 15 is kept 4096 * 7 / 15 = 1911 times in the mean with sd 31.9 (a
    hypergeometric draw per image: p = 7/15, variance 4096 p (1 - p)); the band is +- 6 sd = 192."""
    idx, _ = _cpu.patch_keep_table(UNIFORMITY_SEED, 12, 4096, 16, 8)
    counts = torch.bincount(idx.long().reshape(-1), minlength=16)
    print("kept counts of patches 0 .. 15:", counts.tolist())
    assert int(counts[0]) == 4096
    assert all(1911 - 192 <= int(c) <= 1911 + 192 for c in counts[1:]), counts.tolist()


# ---- the host model -------------------------------------------------------------------------------------------------
def _ocfg(B=4, img=64):
    ocfg = O.make_config("micro", img=img, batch=B, blocks=2)
    return ocfg


def _host_model(ocfg, st, **kw):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, **kw)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st)
    return m


def _host_step(m, x, y, monkeypatch, **fwd):
    """One training step of the host model with the dropout masks recorded: (logits, loss, grads, image grad), masks."""
    masks = []

    def dropout(t, p, training):
        if not training:
            return t
        keep = torch.rand(t.shape) >= p
        masks.append(keep)
        return t * keep.to(t.dtype) * (1.0 / (1.0 - p))

    xin = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "dropout", dropout)
        torch.manual_seed(42)
        logits = m(xin, **fwd)
        loss = torch.nn.functional.cross_entropy(logits, y)
        m.zero_grad(set_to_none=True)
        loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    L = len(m.transformer_encoder.blocks)
    assert len(masks) == 2 * L
    return (logits.detach(), loss.detach(), grads, xin.grad), {(l, s): masks[2 * l + s] for l in range(L) for s in (0, 1)}


@pytest.mark.parametrize("explicit", [False, True])
def test_host_model_vs_oracle(monkeypatch, explicit):
    """The host model at rate 0.5 in training mode against the oracle composed on the kept tokens (embed_forward ->
    gather with the twin's indices -> block_forward x L with the recorded dropout masks -> head_forward): logits, loss
    and every gradient, the input image's included, at the fp32 model gates of the drop-path tests."""
    ocfg = _ocfg()
    st = O.init_state(ocfg, seed=1)
    x, y = O.synthetic_batch(ocfg)
    N, L, B = ocfg.num_patches, ocfg.num_blocks, ocfg.batch_size
    m = _host_model(ocfg, st, patch_drop_rate=0.5).train()
    if explicit:
        idx = _cpu.patch_keep_table(77, L, B, N, 5)[0].long()            # a table of the caller's, K = 5, int64
        got, masks = _host_step(m, x, y, monkeypatch, keep_indices=idx)
    else:
        idx = _cpu.patch_keep_table(BASE_SEED, L, B, N, config.patch_keep_count(N, 0.5))[0]
        got, masks = _host_step(m, x, y, monkeypatch)
    assert torch.equal(m.last_patch_keep, idx.to(torch.int32))
    K = idx.shape[1]
    assert all(v.shape == (B, K + 1, ocfg.embedding_size) for v in masks.values())
    ref = oracle_run(st, x, y, ocfg, idx, masks=masks)
    check_fp32(got, ref, f"host model explicit={explicit}")
    # the subset matters: the oracle on every token, same seedless masks aside, is far away
    dense = O.forward(st, x, ocfg)
    assert (dense - ref[0]).abs().max().item() > 1e-2
    # a dropped patch gets no image gradient, a kept one does
    P = ocfg.patch_size
    gimg = got[3].reshape(B, 3, ocfg.img_size // P, P, ocfg.img_size // P, P).abs().amax(dim=(1, 3, 5)).reshape(B, N)
    kept = torch.zeros(B, N, dtype=torch.bool).scatter_(1, idx.long(), True)
    assert bool((gimg[~kept] == 0).all()) and bool((gimg[kept] > 0).all())


def test_host_model_rate_zero_and_eval_are_the_model_without_the_keyword():
    ocfg = _ocfg()
    st = O.init_state(ocfg, seed=1)
    x, y = O.synthetic_batch(ocfg)
    outs = []
    for kw in ({}, {"patch_drop_rate": 0.0}, {"patch_drop_rate": 0.5}):
        m = _host_model(ocfg, st, **kw).train()
        torch.manual_seed(7)
        logits = m(x)
        torch.nn.functional.cross_entropy(logits, y).backward()
        outs.append((logits.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, m, torch.get_rng_state()))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])
    assert torch.equal(outs[0][3], outs[1][3])           # rate 0 draws nothing: the RNG stream is the old one
    assert outs[1][2].last_patch_keep is None
    assert not torch.equal(outs[0][0], outs[2][0])       # ... and a rate > 0 does something in train mode,
    on, plain = outs[2][2].eval(), outs[0][2].eval()
    with torch.no_grad():                                # nothing in eval mode
        assert torch.equal(on(x), plain(x))
    with pytest.raises(ValueError, match="training-only"):
        on(x, keep_indices=torch.zeros(4, 1, dtype=torch.int64))
    on.train()
    with pytest.raises(TypeError, match="keep_indices"):
        on(x, keep_indices=torch.zeros(4, 1))
    with pytest.raises(ValueError, match="keep_indices"):
        on(x, keep_indices=torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="keep_indices"):
        on(x, keep_indices=torch.zeros(4, 17, dtype=torch.int64))


def test_module_patch_embed_keep():
    """The module-level patch_embed: on the host `keep` gathers the embedding's tokens; on a device it names the
    engine (tests/test_gpu_patch_drop.py)."""
    torch.manual_seed(0)
    w, b = torch.randn(8, 3, 4, 4), torch.randn(8)
    cls, pos = torch.randn(2, 1, 8), torch.randn(1, 5, 8)
    x = torch.randn(2, 3, 8, 8)
    full = _functional.patch_embed(x, w, b, cls, pos, 4, torch.float32)
    keep = torch.tensor([[0, 2], [0, 3]])
    sub = _functional.patch_embed(x, w, b, cls, pos, 4, torch.float32, keep=keep)
    assert sub.shape == (2, 3, 8)
    assert torch.equal(sub[0], full[0, [0, 2, 4]]) and torch.equal(sub[1], full[1, [0, 3, 4]])
    with pytest.raises(ValueError, match="keep_indices"):
        _functional.patch_embed(x, w, b, cls, pos, 4, torch.float32, keep=torch.zeros(2, 5, dtype=torch.int64))


# ---- C ABI ----------------------------------------------------------------------------------------------------------
NEW = ("vit_patch_keep", "vit_im2col_gather", "vit_gather_pos", "vit_pos_grad_gather", "vit_col2im_scatter")


def test_abi_stays_18_with_the_added_exports():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.vit_abi_version() == 18
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in NEW)
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "#define VIT_ABI_VERSION 18" in hdr
    assert f"#define VIT_PATCH_KEEP_MAX_N {_lib.PATCH_KEEP_MAX_N}\n" in hdr


def test_host_abi_patch_drop_checker_c(tmp_path):
    """tests/host_abi_patch_drop_check.c (gcc, no GPU): the five symbols link, ABI 18, and every refusal — NULL
    pointers, K > N, K < 1, N > 4096, B <= 0 and the shape conditions shared with vit_im2col / vit_col2im — returns
    VIT_ERR_INVALID with a vit_last_error() message naming the entry point."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_patch_drop_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_patch_drop_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


# ---- train.py on the host path --------------------------------------------------------------------------------------
def test_train_main_patch_drop_on_cpu_and_resume(tmp_path, monkeypatch):
    import train as T
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    threads = torch.get_num_threads()
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    argv = ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "2", "--steps", "2",
            "--epochs", "0", "--train-size", "4", "--test-size", "2", "--workers", "0", "--threads", "2",
            "--patch-drop", "0.5", "--log-dir", logs, "--checkpoint-dir", ck]
    monkeypatch.setattr(sys, "argv", argv)
    tables = []
    real = _cpu.patch_keep_table
    monkeypatch.setattr(_cpu, "patch_keep_table", lambda *a: (tables.append(a), real(*a))[1])

    def losses():
        rows = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
        return [r["value"] for r in rows if r["tag"] == "Loss/train_batch"]

    try:
        T.main()
        first = losses()
        assert len(first) == 2 and all(math.isfinite(v) and v > 0 for v in first)
        # every training forward drew a table of K = int(4 * 0.5) = 2 of the N = 4 patches; evaluation drew none
        L = T.config.PRESETS["tiny"][2]
        assert len(tables) == 2 and all(a[1:] == (L, 2, 4, 2) for a in tables)
        assert T.search_checkpoint(ck) is not None
        T.main()                                         # finds the checkpoint and goes on from it
        assert len(tables) > 2 and all(math.isfinite(v) for v in losses())
    finally:
        torch.set_num_threads(threads)
    for bad in ("1.0", "-0.1"):
        monkeypatch.setattr(sys, "argv", argv[:argv.index("--patch-drop") + 1] + [bad] + argv[-4:])
        try:
            with pytest.raises(ValueError, match="patch_drop_rate"):
                T.main()
        finally:
            torch.set_num_threads(threads)
