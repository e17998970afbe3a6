"""Knowledge distillation without a GPU: the host twin of optim.distillation_loss against an independent fp64
spelling of the formula and its closed-form gradient, the lowest-index tie rule, the ValueErrors, vit.load_teacher's
checks, train.py --device cpu with a teacher (and its resume and argument errors), and
tests/host_abi_distill_check.c (the prototype, the two enum values and the refusals of vit_softmax_xent_distill)."""
import json
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from VisionTransformer import _lib, config, vit
from VisionTransformer.optim import MixedLabels, dense_target, distillation_loss, lowest_argmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rows, classes, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, classes, generator=g, dtype=torch.float64) * 3
    z = torch.randn(rows, classes, generator=g, dtype=torch.float64) * 3
    a = torch.randint(0, classes, (rows,), generator=g)
    b = torch.randint(0, classes, (rows,), generator=g)
    lam = torch.rand(rows, generator=g)
    lam[0] = 1.0
    if rows > 1:
        lam[1] = 0.0
    return x, z, a, b, lam


def _spelled_out(x, z, t, kind, alpha, tau):
    """(loss, dlogits) from the definitions, with explicit sums and no torch loss function: base_r = lse(x) - sum t x,
    soft d_r = tau^2 sum q_tau (log q_tau - log p_tau), hard d_r = lse(x) - x[yhat], and the closed-form gradient
    ((1 - alpha) (p - t) + alpha g) / rows."""
    rows, C = x.shape

    def softmax(v):
        e = torch.exp(v - v.max(-1, keepdim=True).values)
        return e / e.sum(-1, keepdim=True)

    lse = torch.log(torch.exp(x - x.max(-1, keepdim=True).values).sum(-1)) + x.max(-1).values
    p = softmax(x)
    base = lse - (t * x).sum(-1)
    if kind == "soft":
        pt, qt = softmax(x / tau), softmax(z / tau)
        d = tau ** 2 * (qt * (torch.log(qt) - torch.log(pt))).sum(-1)
        g = tau * (pt - qt)
    else:
        yhat = torch.tensor([min(j for j in range(C) if z[i, j] == z[i].max()) for i in range(rows)])
        onehot = torch.zeros_like(x)
        onehot[torch.arange(rows), yhat] = 1.0
        d = lse - x[torch.arange(rows), yhat]
        g = p - onehot
    loss = ((1 - alpha) * base + alpha * d).mean()
    return loss, ((1 - alpha) * (p - t) + alpha * g) / rows


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("rows,classes", [(1, 4), (5, 1), (8, 10), (37, 257)])
def test_host_twin_against_the_definitions(rows, classes, kind):
    x, z, a, b, lam = _case(rows, classes)
    for tau in (0.5, 1.0, 4.0):
        for alpha in (0.0, 0.5, 1.0):
            for labels, eps in ((a, 0.0), (a, 0.1), (MixedLabels(a, b, lam), 0.1)):
                t = dense_target(labels, classes, eps, dtype=torch.float64)
                xr = x.clone().requires_grad_(True)
                loss = distillation_loss(xr, labels, z, kind=kind, alpha=alpha, tau=tau, label_smoothing=eps)
                loss.backward()
                lref, gref = _spelled_out(x, z, t, kind, alpha, tau)
                assert abs(loss.item() - lref.item()) <= 1e-12 * max(1.0, abs(lref.item())), (tau, alpha, eps)
                assert float((xr.grad - gref).abs().max()) <= 1e-12 * max(1.0, tau), (tau, alpha, eps)


def test_host_twin_alpha_zero_is_cross_entropy_and_the_teacher_gets_no_gradient():
    from VisionTransformer.optim import cross_entropy
    x, z, a, b, lam = _case(8, 10, seed=1)
    x, z = x.float(), z.float()
    labels = MixedLabels(a, b, lam)
    zr = z.clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    loss = distillation_loss(xr, labels, zr, alpha=0.0, label_smoothing=0.1)
    assert abs(loss.item() - cross_entropy(x, labels, 0.1).item()) <= 1e-6
    distillation_loss(xr, labels, zr, kind="soft", alpha=0.7, tau=2.0).backward()
    assert zr.grad is None and xr.grad is not None
    # teacher == student: the soft term and its gradient vanish
    half = distillation_loss(x, labels, x.clone(), alpha=0.5, tau=3.0, label_smoothing=0.1)
    assert abs(half.item() - 0.5 * cross_entropy(x, labels, 0.1).item()) <= 1e-6


def test_lowest_index_tie_rule():
    z = torch.zeros(4, 7)
    z[0, 0] = z[0, 6] = 2.0            # first and last
    z[1, 3] = z[1, 4] = 2.0            # neighbours
    z[2, :] = 1.5                      # every index
    z[3, 5] = 1.0                      # no tie
    assert lowest_argmax(z).tolist() == [0, 3, 0, 5]
    x = torch.randn(4, 7, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    a = torch.zeros(4, dtype=torch.long)
    loss = distillation_loss(x, a, z.double(), kind="hard", alpha=1.0)
    ref = torch.nn.functional.cross_entropy(x, torch.tensor([0, 3, 0, 5]))
    assert abs(loss.item() - ref.item()) <= 1e-12


def test_value_errors():
    x, z, a, _, _ = _case(4, 5)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(kind="medium"), "kind"), (dict(kind=0), "kind"), (dict(alpha=-0.1), "alpha"),
                     (dict(alpha=1.1), "alpha"), (dict(alpha=nan), "alpha"), (dict(tau=0.0), "tau"),
                     (dict(tau=-2.0), "tau"), (dict(tau=inf), "tau"), (dict(tau=nan), "tau"),
                     (dict(label_smoothing=1.0), "label_smoothing")):
        with pytest.raises(ValueError, match=word):
            distillation_loss(x, a, z, **kw)
    with pytest.raises(ValueError, match="shape"):
        distillation_loss(x, a, z[:, :3])


# ---- load_teacher ---------------------------------------------------------------------------------------------------
def _cfg(D=64, H=4, L=2, classes=10, batch=2, dtype=torch.float32):
    return config.ViTConfig(3, classes, 4, D, 16, H, L, "cpu", batch, precision=dtype)


def test_load_teacher(tmp_path):
    tcfg = _cfg(D=128, H=2, L=3)
    torch.manual_seed(3)
    src = vit.VisionTransformer(tcfg)
    st = {k: v.clone() for k, v in src.state_dict().items()}
    ck = tmp_path / "ck"
    ck.mkdir()
    torch.save({"model_state_dict": {k: torch.zeros_like(v) for k, v in st.items()}}, ck / "9.pt")
    torch.save({"model_state_dict": st, "ema_state_dict": {k: v * 0.5 for k, v in st.items()}}, ck / "10.pt")
    student = vit.VisionTransformer(_cfg())
    for where in (str(ck), ck, str(ck / "10.pt")):                # a directory (its newest N.pt, by number) or a file
        t = vit.load_teacher(tcfg, where, student=student)
        assert all(torch.equal(p, st[k]) for k, p in t.named_parameters())
        assert not t.training and t.store_attention_probs is False
        assert all(not p.requires_grad for p in t.parameters())
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        z1, z2 = t(x), t(x)
    assert torch.equal(z1, z2) and z1.grad_fn is None and z1.shape == (2, 10)      # eval mode: no dropout
    e = vit.load_teacher(tcfg, ck, ema=True, device="cpu")
    assert all(torch.equal(p, st[k] * 0.5) for k, p in e.named_parameters())
    with pytest.raises(KeyError, match="ema_state_dict"):
        vit.load_teacher(tcfg, ck / "9.pt", ema=True)
    with pytest.raises(ValueError, match="num_classes"):
        vit.load_teacher(_cfg(D=128, H=2, L=3, classes=7), ck, student=student)
    with pytest.raises(ValueError, match="batch_size"):
        vit.load_teacher(_cfg(D=128, H=2, L=3, batch=4), ck, student=student.vit_config)
    with pytest.raises(ValueError, match="does not hold"):
        vit.load_teacher(_cfg(), ck)                               # another shape than the file's
    with pytest.raises(FileNotFoundError):
        vit.load_teacher(tcfg, tmp_path / "nothing")
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        vit.load_teacher(tcfg, tmp_path / "empty")
    # one distillation step on the host: the student learns, the teacher does not move
    opt = torch.optim.AdamW(student.parameters(), lr=1e-3)
    y = torch.tensor([1, 7])
    loss = distillation_loss(student(x), y, z1, kind="soft", alpha=0.5, tau=2.0, label_smoothing=0.1)
    loss.backward()
    opt.step()
    assert math.isfinite(loss.item())
    assert all(p.grad is None and torch.equal(p, st[k]) for k, p in t.named_parameters())


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_stays_18_with_the_added_export():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.vit_abi_version() == 18
    assert "vit_softmax_xent_distill" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "vit_softmax_xent_distill")
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "#define VIT_ABI_VERSION 18" in hdr
    assert "VIT_DISTILL_SOFT = 0, VIT_DISTILL_HARD = 1" in hdr
    assert (_lib.DISTILL_SOFT, _lib.DISTILL_HARD) == (0, 1)


def test_host_abi_distill_checker_c(tmp_path):
    """tests/host_abi_distill_check.c (gcc, no GPU): the symbol has the header's prototype, ABI 18, the enum values,
    and every refusal returns VIT_ERR_INVALID with a vit_last_error() message naming the entry point."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    libdir = os.path.join(ROOT, "vision-transformer_amd", "VisionTransformer")
    exe = str(tmp_path / "host_abi_distill_check")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_abi_distill_check.c"), "-o", exe, "-L", libdir, "-lvit_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all checks passed (ABI 18)" in r.stdout


# ---- train.py on the host path --------------------------------------------------------------------------------------
def test_train_main_with_a_teacher_on_cpu_and_resume(tmp_path, monkeypatch):
    import train as T
    monkeypatch.setattr(T, "device", T.device)           # main() assigns the module global: restored afterwards
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    threads = torch.get_num_threads()
    common = ["train.py", "--device", "cpu", "--model", "tiny", "--img", "32", "--batch", "2", "--steps", "2",
              "--epochs", "0", "--train-size", "4", "--test-size", "2", "--workers", "0", "--threads", "2"]
    tck = str(tmp_path / "teacher_ck")
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    student = common + ["--label-smoothing", "0.1", "--mixup", "0.8", "--teacher-checkpoint", tck, "--distill", "soft",
                        "--distill-alpha", "0.3", "--distill-tau", "2", "--log-dir", logs, "--checkpoint-dir", ck]
    calls = []
    real = T.distillation_loss

    def spy(logits, labels, tz, **kw):
        loss = real(logits, labels, tz, **kw)
        calls.append((kw, tz.requires_grad, float(loss.detach())))
        return loss

    monkeypatch.setattr(T, "distillation_loss", spy)

    def losses():
        rows = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
        return [r["value"] for r in rows if r["tag"] == "Loss/train_batch"]

    try:
        monkeypatch.setattr(sys, "argv", common + ["--log-dir", str(tmp_path / "teacher_logs"), "--checkpoint-dir", tck])
        T.main()                                         # the teacher: two plain steps
        assert not calls and T.search_checkpoint(tck) == 0
        monkeypatch.setattr(sys, "argv", student)
        T.main()
        assert len(calls) == 2
        assert all(c[0] == dict(kind="soft", alpha=0.3, tau=2.0, label_smoothing=0.1) and not c[1] for c in calls)
        assert losses() == pytest.approx([c[2] for c in calls], rel=1e-6)       # the combined loss is the one logged
        ckpt = torch.load(os.path.join(ck, "0.pt"), map_location="cpu", weights_only=True)
        assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
        assert ckpt["loss"] == pytest.approx(sum(c[2] for c in calls), rel=1e-5)
        T.main()                                         # finds the student's checkpoint and goes on from it
        assert len(calls) == 4 and all(math.isfinite(v) for v in losses())
        assert torch.load(os.path.join(ck, "0.pt"), map_location="cpu", weights_only=True)["step"] == 4
        # a teacher of another preset than the checkpoint's: a clear exit, not a traceback
        monkeypatch.setattr(sys, "argv", student + ["--teacher-model", "small"])
        with pytest.raises(SystemExit) as e:
            T.main()
        assert e.value.code == 2
        # the distillation flags without a teacher, and values outside their ranges: argument errors
        for argv in (common + ["--distill", "soft"], common + ["--distill-alpha", "0.5"], common + ["--distill-tau", "2"],
                     common + ["--teacher-model", "tiny"], common + ["--teacher-ema"], common + ["--teacher-dtype", "bf16"],
                     student + ["--distill-alpha", "1.5"], student + ["--distill-tau", "0"]):
            monkeypatch.setattr(sys, "argv", argv)
            with pytest.raises(SystemExit) as e:
                T.main()
            assert e.value.code == 2, argv
        assert len(calls) == 4
    finally:
        torch.set_num_threads(threads)
