"""Attention rollout without a GPU: rollout.rollout_from_probs in fp64 against an independent matrix-product form of
the definition on the oracle's probabilities (micro, tiny), the fixture tests/golden/rollout_micro.npz (from the
reference module's own .attention_probs, gen_rollout_golden.py), the host path of
VisionTransformer.attention_rollout against that fixture, train.py --eval-only --rollout-out on --device cpu, the
exported symbols and tests/host_abi_rollout_check.c (ABI still 18, the refusals)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O
from VisionTransformer import _lib, _ops, config, rollout, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FUSIONS = ("mean", "max", "min")


def matrix_rollout(probs, token, fuse):
    """The definition as a matrix product, written independently of rollout.py: A_l = rows-normalised (F_l + I),
    R = A_L ... A_1, row `token`."""
    R = None
    for p in probs:
        F = {"mean": lambda t: t.sum(1) / t.shape[1], "max": lambda t: t.max(1).values,
             "min": lambda t: t.min(1).values}[fuse](p)
        A = F + torch.eye(F.shape[-1], dtype=F.dtype)
        A = A / A.sum(-1, keepdim=True)
        R = A if R is None else A @ R
    return R[:, token, :]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, ocfg in (("micro", O.make_config("micro", img=32, batch=4)),
                       ("tiny", O.make_config("tiny", img=64, batch=8))):
        st = O.init_state(ocfg, seed=0)
        x, _ = O.synthetic_batch(ocfg)
        _, p64 = O.forward(st, x, ocfg, keep_probs=True, dtype=torch.float64)
        out[name] = (ocfg, st, x, p64)
    return out


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_recurrence_equals_product(name, cases):
    ocfg, _, _, p64 = cases[name]
    T = ocfg.T
    for fuse in FUSIONS:
        for token in (0, T // 2, T - 1):
            got, layers = rollout.rollout_from_probs(p64, token, fuse, return_layers=True)
            want = matrix_rollout(p64, token, fuse)
            assert got.dtype == torch.float64 and got.shape == (ocfg.batch_size, T)
            assert float((got - want).abs().max()) <= 1e-12
            assert float((got.sum(-1) - 1).abs().max()) <= 1e-12          # every map sums to 1
            assert layers.shape == (ocfg.num_blocks, ocfg.batch_size, T) and torch.equal(layers[0], got)
            # entry l: the chain through blocks l .. L-1 only
            assert float((layers[-1] - matrix_rollout(p64[-1:], token, fuse)).abs().max()) <= 1e-12


def test_one_token_and_bad_arguments():
    one = [torch.ones(3, 2, 1, 1, dtype=torch.float64)] * 4
    for fuse in FUSIONS:
        assert torch.equal(rollout.rollout_from_probs(one, 0, fuse), torch.ones(3, 1, dtype=torch.float64))
    p = torch.softmax(torch.randn(2, 3, 5, 5), -1)
    assert rollout.rollout_from_probs([p]).dtype == torch.float32         # the dtype of its input
    for bad in (dict(token=5), dict(token=-1), dict(token=1.0), dict(token=True), dict(head_fusion="median")):
        with pytest.raises(ValueError):
            rollout.rollout_from_probs([p], **bad)
    for probs in ([], [p, None], [p, p[:, :, :4]], [p, p[:, :2]], [p[0]]):
        with pytest.raises(ValueError):
            rollout.rollout_from_probs(probs)


def test_fixture_against_the_oracle(cases):
    """The fixture (reference module, fp64) and the oracle's probabilities give the same maps."""
    ocfg, _, _, p64 = cases["micro"]
    gold = np.load(os.path.join(GOLDEN, "rollout_micro.npz"))
    for fuse in FUSIONS:
        for token in (0, ocfg.T - 1):
            g = torch.from_numpy(gold[f"{fuse}_{token}"])
            assert g.dtype == torch.float64 and g.shape == (4, 5)
            assert float((rollout.rollout_from_probs(p64, token, fuse) - g).abs().max()) <= 1e-12
            assert 0 < float(gold[f"err32_{fuse}_{token}"]) < 1e-5


def _micro_model(st, ocfg):
    c = config.ViTConfig(3, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size, ocfg.patch_size, ocfg.num_heads,
                         ocfg.num_blocks, "cpu", ocfg.batch_size)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st)
    return m


def test_host_path_against_the_fixture(cases):
    ocfg, st, x, _ = cases["micro"]
    T = ocfg.T
    gold = np.load(os.path.join(GOLDEN, "rollout_micro.npz"))
    m = _micro_model(st, ocfg).train()
    m.store_attention_probs = False
    for fuse in FUSIONS:
        for token in (0, T - 1):
            logits, maps, layers = m.attention_rollout(x, token=token, head_fusion=fuse, return_layers=True)
            assert maps.dtype == torch.float32 and maps.shape == (4, T) and not maps.requires_grad
            gate = max(2 * float(gold[f"err32_{fuse}_{token}"]), T * 2.0 ** -24)
            assert float((maps.double() - torch.from_numpy(gold[f"{fuse}_{token}"])).abs().max()) <= gate
            assert layers.shape == (ocfg.num_blocks, 4, T) and torch.equal(layers[0], maps)
    assert m.training and m.store_attention_probs is False      # left as they were
    m.eval()
    m.store_attention_probs = True
    with torch.no_grad():
        assert torch.equal(m(x), logits)                        # the host path's logits are model(x)'s
    for kw in ({"token": T}, {"token": -1}, {"head_fusion": "sum"}):
        with pytest.raises(ValueError):
            m.attention_rollout(x, **kw)
    pm = m.patch_map(maps, x.shape[2:])
    assert pm.shape == (4, 2, 2) and torch.equal(pm.reshape(4, 4), maps[:, :4])


def test_train_eval_only_rollout_out_on_the_host_path(tmp_path, monkeypatch, capsys):
    import train as T
    monkeypatch.setattr(T, "device", "cpu")
    cfg = config.ViTConfig(3, 10, 4, 192, 16, 3, 12, "cpu", 4)
    torch.manual_seed(3)
    model = vit.VisionTransformer(cfg)
    ck = tmp_path / "ck"
    ck.mkdir()
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, ck / "0.pt")
    out = str(tmp_path / "maps.npz")
    common = ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "4", "--test-size", "7",
              "--workers", "0", "--checkpoint-dir", str(ck)]
    monkeypatch.setattr(sys, "argv", common + ["--eval-only", "--rollout-out", out])
    T.main()
    assert '"top1"' in capsys.readouterr().out
    z = np.load(out)
    assert z["maps"].shape == (4, 2, 2) and z["maps"].dtype == np.float32      # default K: one batch
    assert z["pred"].shape == (4,) and z["label"].shape == (4,)
    x, y = next(iter(torch.utils.data.DataLoader(T.SyntheticImages(7, 3, 32, 10, seed=10_000), batch_size=4)))
    logits, maps = model.attention_rollout(x)
    assert np.array_equal(z["maps"], model.patch_map(maps, (32, 32)).numpy())
    assert np.array_equal(z["pred"], logits.argmax(-1).numpy()) and np.array_equal(z["label"], y.numpy())
    assert np.abs(z["maps"].sum((1, 2)) + maps[:, 4].numpy() - 1).max() < 1e-5
    monkeypatch.setattr(sys, "argv", common + ["--eval-only", "--rollout-out", out, "--rollout-images", "6",
                                               "--rollout-fusion", "min", "--rollout-token", "4"])
    T.main()
    z = np.load(out)
    assert z["maps"].shape == (6, 2, 2) and z["pred"].shape == (6,) and z["label"].shape == (6,)
    monkeypatch.setattr(sys, "argv", common + ["--rollout-out", out])           # needs --eval-only
    with pytest.raises(SystemExit):
        T.main()


def test_the_entry_points_are_exported_and_the_abi_is_still_18():
    assert _lib.ABI_VERSION == 18 and _lib.load().vit_abi_version() == 18
    for name in ("vit_attn_rollout_workspace_bytes", "vit_attn_rollout_step", "vit_attn_rollout_step_form"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert _ops.ROLLOUT_FUSE == {"mean": 0, "max": 1, "min": 2}
    w = _ops.attn_rollout_workspace_bytes(2, 197, 12, 64, torch.bfloat16, 0)
    assert w == 2 * 197 * (7 + 1) * 4


def test_host_abi_rollout_checker_c(tmp_path):
    """tests/host_abi_rollout_check.c (gcc, no GPU): the ABI is still 18, the constants, the workspace grows with B and
    T, and vit_attn_rollout_step refuses hd / T / fuse out of range, r_in == r_out and every NULL among its required
    pointers, each with a message naming it."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_rollout_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_rollout_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout
