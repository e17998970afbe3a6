"""Knowledge distillation on the MI355X: vit_softmax_xent_distill against the torch formula in fp64 on the kernel's own
fp32 inputs, its bitwise conditions (alpha = 0 is vit_softmax_xent_mixed, teacher == student halves it, repeats), the
lowest-index tie rule, guards, NaN containment and refusals; optim.distillation_loss and vit.load_teacher on a micro
student with a wider and deeper teacher; train() and train.py with a teacher.

Gates: the project's xent gates (tests/test_gpu_contract.py::test_softmax_xent).  Loss within 1e-5 * max(1, |ref|);
|dlogits - ref| and the row sums of dlogits within 1e-6 * max(1, G), G = (1 - alpha) + alpha * tau for the soft kind
and 1 for the hard one: G bounds a gradient element's coefficient, and each term's rounding error scales with its
coefficient.  Every case prints its worst error over gate.

Measured on the MI355X over every case of test_distill_kernel_against_fp64: the worst loss error was 0.013 of its
gate ((65, 64), soft, tau 1, alpha 1), the worst dlogits error 0.073 ((3, 257), hard, alpha 0.5, mixed labels) and the
worst row sum 0.171 ((3, 256), hard, alpha 1)."""
import json
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _lib, _ops, config, data, vit
    from VisionTransformer.optim import (FusedAdamW, MixedLabels, cross_entropy, dense_target, distillation_loss,
                                         lowest_argmax)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAME = "vit_softmax_xent_distill"
KINDS = ["soft", "hard"]
TAUS = [0.5, 1.0, 4.0]
ALPHAS = [0.5, 1.0]


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _grid(rows, classes):
    return (torch.randn(rows, classes, device=DEV) * 4 * 1024).round() / 1024      # a 2^-10 grid: shifts are exact


_CASES = {}


def _case(rows, classes, extreme=False):
    """test_softmax_xent's logits and labels and test_softmax_xent_mixed's partner labels and weights, plus teacher
    logits from a second draw of the same recipe; `extreme`: the teacher's 80 and -80 sit at other columns than the
    student's.  Made once per shape and never written to."""
    key = (rows, classes, extreme)
    if key in _CASES:
        return _CASES[key]
    torch.manual_seed(16 + classes)
    lg = _grid(rows, classes)
    idx = torch.arange(rows, device=DEV)
    if extreme:
        lg = lg.clamp(-60, 60)
        lg[idx, idx % classes] = 80.0
        lg[idx, (idx + 5) % classes] = -80.0
    lb = torch.randint(0, classes, (rows,), device=DEV)
    lb[0] = 0
    lb[-1] = classes - 1 if rows > 1 else 0
    if rows > 2:
        lb[1] = classes - 1
    lb2 = torch.randint(0, classes, (rows,), device=DEV)
    lam = torch.rand(rows, device=DEV)
    exact = [0.0, 1.0, 0.5]
    for i in range(min(rows, 6)):
        lam[i] = exact[i % 3]
    if rows == 1:
        lam[0] = 0.5
    lb2[rows // 2] = lb[rows // 2]
    tz = _grid(rows, classes)
    if extreme:
        tz = tz.clamp(-60, 60)
        tz[idx, (idx + 2) % classes] = 80.0
        tz[idx, (idx + 9) % classes] = -80.0
    _CASES[key] = (lg, tz, lb, lb2, lam)
    return _CASES[key]


def _gate_G(kind, alpha, tau):
    return max(1.0, (1.0 - alpha) + alpha * tau) if kind == "soft" else 1.0


def _reference(lg, tz, target, eps, kind, alpha, tau):
    """The torch formula in fp64 on the fp32 inputs: (loss, dlogits)."""
    x = lg.double().requires_grad_(True)
    z = tz.double()
    base = F.cross_entropy(x, target, label_smoothing=eps)
    if kind == "soft":
        d = F.kl_div(F.log_softmax(x / tau, -1), F.log_softmax(z / tau, -1), reduction="batchmean",
                     log_target=True) * tau ** 2
    else:
        d = F.cross_entropy(x, lowest_argmax(z))
    loss = (1.0 - alpha) * base + alpha * d
    loss.backward()
    return loss.detach(), x.grad


def _check(lg, tz, labels, eps, kind, alpha, tau, what=""):
    """One kernel call against the fp64 reference at the gates; returns (loss, dlogits, worst error over gate)."""
    classes = lg.shape[1]
    mixed = isinstance(labels, MixedLabels)
    a, b, lam = (labels.a, labels.b, labels.lam) if mixed else (labels, None, None)
    loss, dl = _ops.softmax_xent_distill(lg, tz, a, b, lam, eps, kind, alpha, tau)
    lref, gref = _reference(lg, tz, dense_target(labels, classes, dtype=torch.float64), eps, kind, alpha, tau)
    G = _gate_G(kind, alpha, tau)
    e_loss = abs(loss.item() - lref.item()) / (1e-5 * max(1.0, abs(lref.item())))
    e_dl = float((dl.double() - gref).abs().max()) / (1e-6 * G)
    e_sum = float(dl.double().sum(-1).abs().max()) / (1e-6 * G)
    print(f"{what}{kind} tau {tau} alpha {alpha} eps {eps} {'mixed' if mixed else 'plain'}: loss {loss.item():.7f} "
          f"ref {lref.item():.7f}; error over gate: loss {e_loss:.3f}, dlogits {e_dl:.3f}, row sums {e_sum:.3f}")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
    assert e_loss <= 1.0 and e_dl <= 1.0 and e_sum <= 1.0, (e_loss, e_dl, e_sum)
    return loss, dl, max(e_loss, e_dl, e_sum)


SHAPES = [(1, 4, False), (8, 10, False), (37, 257, True), (300, 1000, False),
          (65, 63, False), (65, 64, False), (65, 65, False), (5, 1, False),
          (3, 255, False), (3, 256, False), (3, 257, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,classes,extreme", SHAPES)
def test_distill_kernel_against_fp64(rows, classes, extreme, kind):
    """Every tau x alpha x {hard labels, mixed labels smoothed by 0.1} of one shape and kind."""
    lg, tz, lb, lb2, lam = _case(rows, classes, extreme)
    worst = 0.0
    for tau in TAUS:
        for alpha in ALPHAS:
            for labels, eps in ((lb, 0.0), (MixedLabels(lb, lb2, lam), 0.1)):
                worst = max(worst, _check(lg, tz, labels, eps, kind, alpha, tau, f"{rows}x{classes} ")[2])
    print(f"{rows}x{classes} {kind}: worst error over gate {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,classes,extreme", SHAPES[:4])
def test_distill_kernel_shift_invariance(rows, classes, extreme, kind):
    """The sibling test's lg - 16 check, student and teacher shifted independently (exact on the 2^-10 grid): both
    maxima cancel, so the results agree to rounding."""
    lg, tz, lb, lb2, lam = _case(rows, classes, extreme)
    labels = MixedLabels(lb, lb2, lam)
    for tau in TAUS:
        G = _gate_G(kind, 0.5, tau)
        loss, dl, _ = _check(lg, tz, labels, 0.1, kind, 0.5, tau)
        for ds, dt in ((-16.0, 0.0), (0.0, -16.0), (-16.0, 8.0)):
            loss_s, dl_s, _ = _check(lg + ds, tz + dt, labels, 0.1, kind, 0.5, tau, f"shift {ds} {dt} ")
            assert abs(loss.item() - loss_s.item()) <= 1e-5 * max(1.0, abs(loss.item()))
            assert float((dl - dl_s).abs().max()) <= 1e-6 * G


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,classes,extreme", SHAPES)
def test_alpha_zero_is_the_mixed_kernel_bitwise(rows, classes, extreme, kind):
    lg, tz, lb, lb2, lam = _case(rows, classes, extreme)
    for a, b, l, eps in ((lb, None, None, 0.0), (lb, None, None, 0.1), (lb, lb2, lam, 0.0), (lb, lb2, lam, 0.1)):
        loss_m, dl_m = _ops.softmax_xent_mixed(lg, a, b, l, eps)
        for tau in TAUS:
            loss, dl = _ops.softmax_xent_distill(lg, tz, a, b, l, eps, kind, 0.0, tau)
            assert torch.equal(_bits(loss), _bits(loss_m)) and torch.equal(_bits(dl), _bits(dl_m)), (eps, tau)


@pytest.mark.parametrize("rows,classes,extreme", SHAPES)
def test_teacher_equal_to_student_halves_the_mixed_gradient_bitwise(rows, classes, extreme):
    """Soft, alpha = 0.5, teacher == student (same values, another buffer): the KL term and its gradient are exactly
    zero, so dlogits is 0.5 x the mixed kernel's, bit for bit."""
    lg, _, lb, lb2, lam = _case(rows, classes, extreme)
    _, dl_m = _ops.softmax_xent_mixed(lg, lb, lb2, lam, 0.1)
    for tau in TAUS:
        loss, dl = _ops.softmax_xent_distill(lg, lg.clone(), lb, lb2, lam, 0.1, "soft", 0.5, tau)
        assert torch.equal(_bits(dl), _bits(0.5 * dl_m)), tau
        assert bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("kind", KINDS)
def test_repeats_are_bitwise(kind):
    lg, tz, lb, lb2, lam = _case(300, 1000)
    first = _ops.softmax_xent_distill(lg, tz, lb, lb2, lam, 0.1, kind, 0.5, 4.0)
    for _ in range(3):
        again = _ops.softmax_xent_distill(lg, tz, lb, lb2, lam, 0.1, kind, 0.5, 4.0)
        assert torch.equal(_bits(first[0]), _bits(again[0])) and torch.equal(_bits(first[1]), _bits(again[1]))


@pytest.mark.parametrize("rows,classes,extreme", SHAPES[:4])
def test_hard_alpha_one_is_the_plain_kernel_on_the_teachers_labels(rows, classes, extreme):
    lg, tz, lb, _, _ = _case(rows, classes, extreme)
    yhat = lowest_argmax(tz)
    loss, dl = _ops.softmax_xent_distill(lg, tz, lb, None, None, 0.0, "hard", 1.0, 1.0)
    loss_o, dl_o = _ops.softmax_xent(lg, yhat)
    assert abs(loss.item() - loss_o.item()) <= 1e-5 * max(1.0, abs(loss_o.item()))
    assert float((dl - dl_o).abs().max()) <= 1e-6


@pytest.mark.parametrize("classes", [5, 257, 1000])
def test_hard_ties_take_the_lowest_index(classes):
    """Teacher rows whose maximum occurs at {0 and C - 1}, at {3, 4} and at every index: yhat is the lowest, read back
    from the gradient (alpha = 1: dlogits * rows = p - onehot(yhat) is negative at yhat alone)."""
    torch.manual_seed(classes)
    lg = _grid(3, classes).clamp(-2, 2)                     # p < 1 everywhere: p - onehot(yhat) < 0 at yhat
    tz = _grid(3, classes).clamp(-30, 30)
    tz[0, 0] = tz[0, classes - 1] = 40.0
    tz[1, 3] = tz[1, 4] = 40.0
    tz[2, :] = 1.5
    lb = torch.zeros(3, dtype=torch.int64, device=DEV)
    loss, dl = _ops.softmax_xent_distill(lg, tz, lb, None, None, 0.0, "hard", 1.0, 1.0)
    neg = [torch.nonzero(dl[i] < 0).flatten().tolist() for i in range(3)]
    assert neg == [[0], [3], [0]], neg
    assert lowest_argmax(tz).tolist() == [0, 3, 0]
    lref, gref = _reference(lg, tz, dense_target(lb, classes, dtype=torch.float64), 0.0, "hard", 1.0, 1.0)
    assert abs(loss.item() - lref.item()) <= 1e-5 * max(1.0, abs(lref.item()))
    assert float((dl.double() - gref).abs().max()) <= 1e-6


def _raw(lg, tz, a, b, lam, eps, kind, alpha, tau, rows, classes, loss, dl, ws):
    """The C entry point itself, past the Python wrapper's own checks."""
    p = _ops._ptr
    _lib.call(NAME, p(lg), p(tz), p(a), p(b), p(lam), eps, kind, alpha, tau, rows, classes, p(loss), p(dl), p(ws),
              _ops._stream())


@pytest.mark.parametrize("kind", [0, 1], ids=KINDS)
@pytest.mark.parametrize("rows,classes", [(3, 257), (65, 63), (5, 1)])
def test_guards_stay_untouched(rows, classes, kind):
    """dlogits, workspace and loss inside NaN-filled buffers: the sentinels around them stay NaN, and the results are
    those of the wrapper's own buffers."""
    lg, tz, lb, lb2, lam = _case(rows, classes)
    guard, n = 64, rows * classes
    nan = float("nan")
    big_dl = torch.full((n + 2 * guard,), nan, device=DEV)
    big_ws = torch.full((rows + 2 * guard,), nan, device=DEV)
    big_loss = torch.full((1 + 2 * guard,), nan, device=DEV)
    dl, ws, loss = big_dl[guard:guard + n], big_ws[guard:guard + rows], big_loss[guard:guard + 1]
    _raw(lg, tz, lb, lb2, lam, 0.1, kind, 0.5, 2.0, rows, classes, loss, dl, ws)
    torch.cuda.synchronize()
    for big, inner in ((big_dl, n), (big_ws, rows), (big_loss, 1)):
        assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + inner:]).all())
        assert bool(torch.isfinite(big[guard:guard + inner]).all())
    loss_w, dl_w = _ops.softmax_xent_distill(lg, tz, lb, lb2, lam, 0.1, KINDS[kind], 0.5, 2.0)
    assert torch.equal(_bits(loss), _bits(loss_w)) and torch.equal(_bits(dl.view(rows, classes)), _bits(dl_w))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_nan_containment(kind, alpha):
    """A NaN in student row 0, and separately in teacher row 0: row 0 of dlogits and the loss are NaN, rows >= 1 keep
    the bits of the NaN-free run.  An out-of-range label gives a NaN loss."""
    lg, tz, lb, lb2, lam = _case(37, 257, True)
    args = (lb, lb2, lam, 0.1, kind, alpha, 2.0)
    _, dl0 = _ops.softmax_xent_distill(lg, tz, *args)
    for which in ("student", "teacher"):
        x, z = lg.clone(), tz.clone()
        (x if which == "student" else z)[0, 100] = float("nan")
        loss, dl = _ops.softmax_xent_distill(x, z, *args)
        assert math.isnan(loss.item()), which
        assert bool(torch.isnan(dl[0]).all()), which
        assert torch.equal(_bits(dl[1:]), _bits(dl0[1:])), which
    for bad in (-1, 257, 2 ** 40):
        la = lb.clone()
        la[3] = bad
        loss, dl = _ops.softmax_xent_distill(lg, tz, la, None, None, 0.0, kind, alpha, 2.0)
        assert math.isnan(loss.item()), bad
        assert torch.equal(_bits(dl[4:]), _bits(_ops.softmax_xent_distill(lg, tz, lb, None, None, 0.0, kind, alpha,
                                                                          2.0)[1][4:]))


def test_refusals_launch_nothing():
    """Every refusal of the header comment comes back as RuntimeError naming the entry point, and the outputs keep their
    sentinels.  Host-side argument checks only: every pointer that is not None is a live device buffer."""
    rows, classes = 8, 10
    lg, tz, lb, lb2, lam = _case(rows, classes)
    loss = torch.full((1,), -7.0, device=DEV)
    dl = torch.full((rows, classes), -7.0, device=DEV)
    ws = torch.full((rows,), -7.0, device=DEV)
    good = dict(lg=lg, tz=tz, a=lb, b=lb2, lam=lam, eps=0.1, kind=0, alpha=0.5, tau=1.0, rows=rows, classes=classes,
                loss=loss, dl=dl, ws=ws)
    nan, inf = float("nan"), float("inf")
    bad = [dict(lg=None), dict(tz=None), dict(a=None), dict(loss=None), dict(dl=None), dict(ws=None),
           dict(rows=0), dict(rows=-1), dict(classes=0), dict(classes=-5), dict(rows=2 ** 31),
           dict(eps=1.0), dict(eps=-0.1), dict(eps=nan), dict(b=None),
           dict(kind=2), dict(kind=-1), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=nan),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(tau=nan)]
    for change in bad:
        with pytest.raises(RuntimeError, match=NAME):
            _raw(**{**good, **change})
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((dl == -7.0).all()) and bool((ws == -7.0).all())
    _raw(**good)                                        # and the unchanged arguments are accepted
    assert math.isfinite(loss.item())
    # the wrapper and the public function refuse with ValueError before the library is reached
    for kw in (dict(kind="medium"), dict(alpha=1.5), dict(alpha=nan), dict(tau=0.0), dict(tau=inf)):
        with pytest.raises(ValueError):
            _ops.softmax_xent_distill(lg, tz, lb, **kw)
        with pytest.raises(ValueError):
            distillation_loss(lg, lb, tz, **kw)
    with pytest.raises(ValueError, match="shape"):
        _ops.softmax_xent_distill(lg, tz[:, :5].contiguous(), lb)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def _vit_config(ocfg, dtype):
    return config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                            ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)


def _teacher_ocfg(**kw):
    """Another width and depth than the micro student's (64, 4 heads, 2 blocks)."""
    t = O.make_config("micro", blocks=3, **kw)
    t.embedding_size, t.num_heads = 128, 2
    return t


def _save_teacher(ocfg, dtype, path, seed=5):
    os.makedirs(path, exist_ok=True)
    st = O.init_state(ocfg, seed=seed)
    older = {k: torch.zeros_like(v) for k, v in st.items()}
    torch.save({"model_state_dict": older}, os.path.join(path, "3.pt"))
    torch.save({"model_state_dict": st, "ema_state_dict": {k: v * 0.5 for k, v in st.items()}},
               os.path.join(path, "10.pt"))                       # the newest by number, not by name order
    return st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_model_level_distillation(tmp_path, dtype, kind):
    ocfg = O.make_config("micro")
    tcfg = _teacher_ocfg()
    ck = str(tmp_path / "teacher")
    st_t = _save_teacher(tcfg, dtype, ck)
    student = vit.VisionTransformer(_vit_config(ocfg, dtype))
    student.load_state_dict(O.init_state(ocfg, seed=0))
    student = student.to(DEV).eval()
    student.store_attention_probs = False
    teacher = vit.load_teacher(_vit_config(tcfg, dtype), ck, student=student, device=DEV)
    assert not teacher.training and teacher.store_attention_probs is False
    assert all(not p.requires_grad for p in teacher.parameters())
    assert all(torch.equal(p.detach().cpu(), st_t[k]) for k, p in teacher.named_parameters())      # 10.pt, not 3.pt
    before = {k: p.detach().clone() for k, p in teacher.named_parameters()}
    x, y = O.synthetic_batch(ocfg)
    x = x.to(DEV)
    labels = MixedLabels(y.to(DEV), y.flip(0).to(DEV), torch.tensor([0.3, 1.0, 0.0, 0.5], device=DEV))
    with torch.no_grad():
        tz = teacher(x)
        tz2 = teacher(x)
    assert tz.grad_fn is None and not tz.requires_grad
    assert torch.equal(_bits(tz), _bits(tz2))
    alpha, tau, eps = 0.5, 2.0, 0.1
    opt = FusedAdamW(student.parameters(), lr=1e-3)

    logits = student(x)
    loss = distillation_loss(logits, labels, tz, kind=kind, alpha=alpha, tau=tau, label_smoothing=eps)
    lref, _ = _reference(logits.detach(), tz, dense_target(labels, ocfg.num_classes, dtype=torch.float64), eps, kind,
                         alpha, tau)
    print(f"{dtype} {kind}: loss {loss.item():.7f} ref {lref.item():.7f}")
    assert abs(loss.item() - lref.item()) <= 1e-5 * max(1.0, abs(lref.item()))
    assert abs(loss.item() - cross_entropy(logits.detach(), labels, eps).item()) > 1e-4       # the teacher term is in it
    loss.backward()
    got = {k: p.grad.detach().clone() for k, p in student.named_parameters()}

    # the same gradients from the kernel's dlogits through the engine's backward: no tolerance
    opt.zero_grad(set_to_none=True)
    logits2 = student(x)
    assert torch.equal(_bits(logits2), _bits(logits))
    loss_k, dl_k = _ops.softmax_xent_distill(logits2.detach().contiguous().float(), tz.float(), labels.a, labels.b, labels.lam, eps,
                                             kind, alpha, tau)
    assert torch.equal(_bits(loss_k.view(())), _bits(loss))
    logits2.backward(gradient=dl_k.to(logits2.dtype))
    for k, p in student.named_parameters():
        assert torch.equal(_bits(p.grad), _bits(got[k])), k
    # a teacher passed with requires_grad set is detached all the same
    tz_g = tz.clone().requires_grad_(True)
    distillation_loss(student(x), labels, tz_g, kind=kind, alpha=alpha, tau=tau).backward()
    assert tz_g.grad is None

    opt.step()
    torch.cuda.synchronize()
    for k, p in teacher.named_parameters():
        assert p.grad is None and torch.equal(_bits(p), _bits(before[k])), k


def test_load_teacher_checks(tmp_path):
    ocfg = O.make_config("micro")
    tcfg = _teacher_ocfg()
    ck = str(tmp_path / "teacher")
    st = _save_teacher(tcfg, torch.float32, ck)
    scfg = _vit_config(ocfg, torch.float32)
    with pytest.raises(ValueError, match="num_classes"):
        vit.load_teacher(_vit_config(_teacher_ocfg(num_classes=7), torch.float32), ck, student=scfg, device=DEV)
    with pytest.raises(ValueError, match="batch_size"):
        vit.load_teacher(_vit_config(_teacher_ocfg(batch=2), torch.float32), ck, student=scfg, device=DEV)
    with pytest.raises(FileNotFoundError):
        vit.load_teacher(_vit_config(tcfg, torch.float32), str(tmp_path / "nothing"), device=DEV)
    with pytest.raises(ValueError, match="does not hold"):
        vit.load_teacher(scfg, ck, device=DEV)                     # the student's shape against the teacher's file
    ema = vit.load_teacher(_vit_config(tcfg, torch.float32), os.path.join(ck, "10.pt"), ema=True, device=DEV)
    k = "mlp.3.weight"
    assert torch.equal(dict(ema.named_parameters())[k].cpu(), st[k] * 0.5)
    with pytest.raises(KeyError, match="ema_state_dict"):
        vit.load_teacher(_vit_config(tcfg, torch.float32), os.path.join(ck, "3.pt"), ema=True, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# train() and train.py
# ---------------------------------------------------------------------------------------------------------------------
TINY = dict(classes=10, patches=4, img=32, batch=4)


def _tiny_config(dtype=torch.float32):
    D, H, L = config.PRESETS["tiny"]
    return config.ViTConfig(3, TINY["classes"], TINY["patches"], D, 16, H, L, "cpu", TINY["batch"], precision=dtype)


def _train_module():
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    return T


def _loaders(T):
    loader = torch.utils.data.DataLoader(T.SyntheticImages(16, 3, TINY["img"], TINY["classes"], seed=3),
                                         batch_size=TINY["batch"], drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, TINY["img"], TINY["classes"], seed=4),
                                              batch_size=TINY["batch"])
    return loader, test_loader


@pytest.fixture(scope="module")
def teacher_dir(tmp_path_factory):
    """A tiny teacher trained for three steps by train() itself."""
    T = _train_module()
    root = tmp_path_factory.mktemp("teacher")
    loader, test_loader = _loaders(T)
    T.train(_tiny_config(), loader, test_loader, epochs=0, eval_iter=0, log_dir=str(root / "logs"),
            checkpoint_dir=str(root / "ck"), lr=1e-3, max_steps=3)
    return str(root / "ck")


def _logged(logs):
    rows = [json.loads(l) for l in open(os.path.join(logs, "scalars.jsonl"))]
    return [(r["step"], r["value"]) for r in rows if r["tag"] == "Loss/train_batch"]


def test_train_with_a_teacher_and_resume(tmp_path, monkeypatch, teacher_dir):
    T = _train_module()
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = _tiny_config()
    teacher = vit.load_teacher(_tiny_config(), teacher_dir, student=cfg, device=DEV)
    before = {k: p.detach().clone() for k, p in teacher.named_parameters()}
    seen = []
    real = T.distillation_loss

    def spy(logits, labels, tz, **kw):
        loss = real(logits, labels, tz, **kw)
        seen.append((kw, isinstance(labels, MixedLabels), tz.requires_grad, loss.detach()))
        return loss

    monkeypatch.setattr(T, "distillation_loss", spy)
    loader, test_loader = _loaders(T)
    for kind in KINDS:
        ck, logs = str(tmp_path / f"ck_{kind}"), str(tmp_path / f"logs_{kind}")
        kw = dict(eval_iter=1, log_dir=logs, checkpoint_dir=ck, lr=1e-3, max_steps=2, label_smoothing=0.1,
                  mix=data.BatchMix(0.8, 1.0, per_image=True, seed=5), teacher=teacher, distill=kind,
                  distill_alpha=0.4, distill_tau=2.0)
        del seen[:]
        last = T.train(cfg, loader, test_loader, epochs=0, **kw)
        assert len(seen) == 2 and all(s[0] == dict(kind=kind, alpha=0.4, tau=2.0, label_smoothing=0.1) for s in seen)
        assert all(s[1] and not s[2] for s in seen)                  # mixed labels reach the loss; no teacher gradient
        values = [float(s[3]) for s in seen]
        assert [s for s, _ in _logged(logs)] == [0, 1]
        assert [v for _, v in _logged(logs)] == pytest.approx(values, rel=1e-6)     # the combined loss is the one logged
        assert last == pytest.approx(sum(values), rel=1e-5)
        ckpt = torch.load(os.path.join(ck, "0.pt"), map_location="cpu", weights_only=True)
        assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}       # today's keys
        assert ckpt["loss"] == pytest.approx(sum(values), rel=1e-5) and ckpt["step"] == 2
        fresh = vit.VisionTransformer(cfg)
        assert set(ckpt["model_state_dict"]) == set(fresh.state_dict())
        fresh.load_state_dict(ckpt["model_state_dict"])
        # resume: the newest checkpoint is found, the step counter goes on, and the teacher is still the loss's
        T.train(cfg, loader, test_loader, epochs=1, **kw)
        assert sorted(os.listdir(ck)) == ["0.pt", "1.pt"]
        ckpt1 = torch.load(os.path.join(ck, "1.pt"), map_location="cpu", weights_only=True)
        assert ckpt1["step"] == 6 and math.isfinite(ckpt1["loss"]) and len(seen) == 6
        assert [s for s, _ in _logged(logs)] == [0, 1, 2, 3, 4, 5]
    for k, p in teacher.named_parameters():
        assert p.grad is None and torch.equal(_bits(p), _bits(before[k])), k
    with pytest.raises(ValueError, match="alpha"):
        T.train(cfg, loader, test_loader, epochs=0, **{**kw, "distill_alpha": 1.5})
    with pytest.raises(ValueError, match="batch_size"):
        bad = config.ViTConfig(3, 10, 4, 192, 16, 3, 12, "cpu", 2)
        T.train(bad, loader, test_loader, epochs=0, **kw)
    sec, loss = T.time_steps(cfg, 2, 1, dev="cuda", label_smoothing=0.1, teacher=teacher, distill="soft",
                             distill_alpha=0.4, distill_tau=2.0)
    assert sec > 0 and math.isfinite(loss)


def test_train_py_with_a_teacher_checkpoint(tmp_path, monkeypatch, teacher_dir):
    """train.py --teacher-checkpoint end to end, in this process as the other train.py tests run it."""
    T = _train_module()
    monkeypatch.setattr(T, "device", T.device)
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    argv = ["train.py", "--model", "tiny", "--img", "32", "--batch", "4", "--steps", "2", "--epochs", "0",
            "--train-size", "8", "--test-size", "4", "--workers", "0", "--label-smoothing", "0.1", "--mixup", "0.8",
            "--teacher-checkpoint", teacher_dir, "--teacher-dtype", "bf16", "--distill", "soft", "--distill-alpha",
            "0.3", "--distill-tau", "3", "--log-dir", logs, "--checkpoint-dir", ck]
    monkeypatch.setattr(sys, "argv", argv)
    calls = []
    real = T.distillation_loss
    monkeypatch.setattr(T, "distillation_loss", lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1])
    T.main()
    assert len(calls) == 2 and calls[0] == dict(kind="soft", alpha=0.3, tau=3.0, label_smoothing=0.1)
    values = [v for _, v in _logged(logs)]
    assert len(values) == 2 and all(math.isfinite(v) and v > 0 for v in values)
    ckpt = torch.load(os.path.join(ck, "0.pt"), map_location="cpu", weights_only=True)
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step"}
    monkeypatch.setattr(sys, "argv", [a for a in argv if a not in ("--teacher-checkpoint", teacher_dir)])
    with pytest.raises(SystemExit) as e:
        T.main()
    assert e.value.code == 2
