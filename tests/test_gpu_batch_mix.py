"""Label smoothing, mixup and CutMix on the MI355X: vit_softmax_xent_mixed against F.cross_entropy on the dense fp64
target, vit_mix_batch against an fp64 mix of the stored inputs (both access forms, both dtypes, box edges inside a
16-byte unit, NaN / inf that must not leak), data.BatchMix and data.DeviceBatches(mix=) against the host path, and the
whole step (mixed input, smoothed two-label loss) against the oracle, plus train() with the three options on.

Gates.  Loss: the project's xent gates (tests/test_gpu_contract.py::test_softmax_xent).  Mix: elements inside the box
and elements of a w == 1 image are copies, so bitwise; a blended element w * a + (1 - w) * b takes three fp32
roundings (1 - w, its product with b, the fused multiply-add), each at most 2^-24 of a term bounded by |a| + |b|, so
4 * 2^-24 * (|a| + |b|) holds with room (a CPU check of the fused and the unfused fp32 orders peaked at 0.46 of it;
measured on the device: at most 0.30 of it).  A bf16 result is that fp32 value rounded once more: half a bf16 ulp,
at most 2^-8 * |ref| (reached at the bottom of a binade: measured 0.996 of the gate), plus the fp32 part, for which
the gate allows 8 * 2^-24 * (|a| + |b|)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops, config, data, vit
    from VisionTransformer.optim import CrossEntropyLoss, FusedAdamW, MixedLabels, cross_entropy, dense_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# loss kernel
# ---------------------------------------------------------------------------------------------------------------------
def _xent_case(rows, classes, extreme):
    """test_softmax_xent's logits and labels, plus partner labels and weights: lam holds exact 0, 1 and 0.5 and one
    row has a == b."""
    torch.manual_seed(16 + classes)
    lg = (torch.randn(rows, classes, device=DEV) * 4 * 1024).round() / 1024    # a 2^-10 grid: shifts are exact
    if extreme:
        lg = lg.clamp(-60, 60)
        idx = torch.arange(rows, device=DEV)
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
    for i in range(rows):
        if i < 3:
            lam[i] = exact[i]
        elif i < 6:
            lam[i] = exact[i - 3]
    if rows == 1:
        lam[0] = 0.5
    lb2[rows // 2] = lb[rows // 2]                                             # a == b (lam there is whatever it is)
    return lg, lb, lb2, lam


@pytest.mark.parametrize("mode", ["smooth", "mix", "both", "plain"])
@pytest.mark.parametrize("rows,classes,extreme", [(1, 4, False), (8, 10, False), (37, 257, True), (300, 1000, False)])
def test_softmax_xent_mixed(rows, classes, extreme, mode):
    lg, lb, lb2, lam = _xent_case(rows, classes, extreme)
    eps = 0.1 if mode in ("smooth", "both") else 0.0
    b, l = (lb2, lam) if mode in ("mix", "both") else (None, None)
    target = dense_target(MixedLabels(lb, lb2, lam) if b is not None else lb, classes, dtype=torch.float64)

    def check(logits):
        loss, dl = _ops.softmax_xent_mixed(logits.contiguous(), lb, b, l, eps)
        loss2, dl2 = _ops.softmax_xent_mixed(logits.contiguous(), lb, b, l, eps)
        assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(dl), _bits(dl2))      # repeatable
        lr_ = logits.double().requires_grad_(True)
        lref = F.cross_entropy(lr_, target, label_smoothing=eps)
        lref.backward()
        print(f"{mode} {rows}x{classes}: loss {loss.item():.7f} ref {lref.item():.7f}, "
              f"|dl - ref| {float((dl.double() - lr_.grad).abs().max()):.3e}, "
              f"row sums {float(dl.double().sum(-1).abs().max()):.3e}")
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
        assert abs(loss.item() - lref.item()) <= 1e-5 * max(1.0, abs(lref.item()))
        assert float((dl.double() - lr_.grad).abs().max()) <= 1e-6
        assert float(dl.double().sum(-1).abs().max()) <= 1e-6
        return loss, dl

    loss, dl = check(lg)
    loss_s, dl_s = check(lg - 16.0)                                     # exact in fp32 (|x| <= 96, 2^-10 grid)
    assert abs(loss.item() - loss_s.item()) <= 1e-5 * max(1.0, abs(loss.item()))
    assert float((dl - dl_s).abs().max()) <= 1e-6
    if mode == "plain":                                                  # eps = 0, NULL labels_b / lam: the old kernel
        loss_o, dl_o = _ops.softmax_xent(lg.contiguous(), lb)
        assert abs(loss.item() - loss_o.item()) <= 1e-5 * max(1.0, abs(loss_o.item()))
        assert float((dl - dl_o).abs().max()) <= 1e-6


def test_cross_entropy_default_is_the_old_kernel_bitwise_and_the_new_paths_differentiate():
    lg, lb, lb2, lam = _xent_case(37, 257, True)
    loss_o, dl_o = _ops.softmax_xent(lg.contiguous(), lb)
    for fn in (lambda x: cross_entropy(x, lb), lambda x: cross_entropy(x, lb, 0.0), lambda x: CrossEntropyLoss()(x, lb)):
        x = lg.clone().requires_grad_(True)
        loss = fn(x)
        loss.backward()
        assert torch.equal(_bits(loss), _bits(loss_o.view(()))) and torch.equal(_bits(x.grad), _bits(dl_o))
    # smoothing / MixedLabels through autograd: the gradient is the kernel's dlogits, scaled by the upstream gradient
    x = lg.clone().requires_grad_(True)
    loss = cross_entropy(x, MixedLabels(lb, lb2, lam), label_smoothing=0.1)
    (2.0 * loss).backward()
    loss_k, dl_k = _ops.softmax_xent_mixed(lg.contiguous(), lb, lb2, lam, 0.1)
    assert torch.equal(_bits(loss), _bits(loss_k.view(()))) and torch.equal(_bits(x.grad), _bits(dl_k * 2.0))
    x = lg.clone().requires_grad_(True)
    CrossEntropyLoss(label_smoothing=0.1)(x, lb).backward()
    assert torch.equal(_bits(x.grad), _bits(_ops.softmax_xent_mixed(lg.contiguous(), lb, None, None, 0.1)[1]))
    with pytest.raises(ValueError, match="labels_b"):
        _ops.softmax_xent_mixed(lg.contiguous(), lb, None, lam, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# mix kernel
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 8, 8), (5, 7, 30), (4, 16, 16), (8, 64, 64)]
DTYPES = [torch.float32, torch.bfloat16]


def _row_specs(H, W):
    """(w, y0, y1, x0, x1): w in {1, 0, 0.5, 0.3}; an empty box, the whole image, the single pixel (H-1, W-1), a box
    whose x0 and x1 are odd (both edges inside a 16-byte unit), and a row with both a box and w = 0.3."""
    odd_hi = W - 1 if (W - 1) % 2 == 1 else W - 2
    return [(1.0, 0, 0, 0, 0), (0.0, 0, 0, 0, 0), (0.5, 0, 0, 0, 0), (0.3, 0, 0, 0, 0), (1.0, 0, H, 0, W),
            (1.0, H - 1, H, W - 1, W), (1.0, 1, H - 1, 1, odd_hi), (0.3, 2, 5, 3, odd_hi - 2)]


def _tables(B, H, W):
    """Tables of B rows that together cover every row spec; the first pairs image i with B - 1 - i (B = 1 and the
    middle image of B = 5 are their own partners), the others with i + 1."""
    specs = _row_specs(H, W)
    out = []
    for k in range(math.ceil(len(specs) / B)):
        rows = [specs[(k * B + i) % len(specs)] for i in range(B)]
        src = [B - 1 - i for i in range(B)] if k == 0 else [(i + 1) % B for i in range(B)]
        out.append((src, *[list(c) for c in zip(*rows)]))
    return out


def _input(B, H, W, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * B + H)
    return torch.randn(B, 3, H, W, generator=g).to(dtype).to(DEV)


def _masks(tab, B, H, W):
    src, w, y0, y1, x0, x1 = (torch.as_tensor(np.asarray(c)) for c in tab)
    ys, xs = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    col = lambda v: v.view(B, 1, 1, 1)      # noqa: E731
    box = ((ys >= col(y0)) & (ys < col(y1)) & (xs >= col(x0)) & (xs < col(x1))).expand(B, 3, H, W)
    return src.long(), w.float(), box


def _check_mix(out, x, tab, only_copies=False):
    """`out` against the fp64 mix of the stored `x` under the table: copies bitwise, blends within the gate."""
    B, _, H, W = x.shape
    xc, oc = x.cpu(), out.cpu()
    src, w, box = _masks(tab, B, H, W)
    xs = xc[src]
    keep = (w == 1.0).view(B, 1, 1, 1).expand_as(box) & ~box
    assert torch.equal(_bits(oc)[box], _bits(xs)[box])
    assert torch.equal(_bits(oc)[keep], _bits(xc)[keep])
    if only_copies:
        return 0.0
    blend = ~box & ~keep
    w64 = w.double().view(B, 1, 1, 1)
    a, b = xc.double(), xs.double()
    ref = w64 * a + (1.0 - w64) * b
    mag = a.abs() + b.abs()
    if x.dtype == torch.float32:
        gate = 4 * 2.0 ** -24 * mag
    else:
        gate = 2.0 ** -8 * ref.abs() + 8 * 2.0 ** -24 * mag
    err = (oc.double() - ref).abs()
    assert bool((err[blend] <= gate[blend]).all()), float((err[blend] / gate[blend].clamp_min(1e-300)).max())
    return float((err[blend] / gate[blend].clamp_min(1e-300)).max()) if bool(blend.any()) else 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_mix_batch_against_fp64(B, H, W, dtype):
    x = _input(B, H, W, dtype)
    x0 = x.clone()
    n = x.numel()
    worst = 0.0
    for tab in _tables(B, H, W):
        out = _ops.mix_batch(x, tab)
        worst = max(worst, _check_mix(out, x, tab))
        assert torch.equal(_bits(x), _bits(x0))                                          # x unchanged
        assert torch.equal(_bits(_ops.mix_batch(x, tab)), _bits(out))                    # twice in a row
        # out inside a larger sentinel-filled buffer: the guards stay intact
        guard = 64
        big = torch.full((n + 2 * guard,), -7.0, dtype=dtype, device=DEV)
        inner = big[guard:guard + n].view_as(x)
        assert _ops.mix_batch(x, tab, out=inner) is inner
        assert torch.equal(_bits(inner), _bits(out))
        assert bool((big[:guard] == -7.0).all()) and bool((big[guard + n:] == -7.0).all())
        # x and out one element off a 16-byte boundary: the element form, bitwise the aligned result
        xb = torch.full((n + 16,), 3.0, dtype=dtype, device=DEV)
        ob = torch.full((n + 16,), -7.0, dtype=dtype, device=DEV)
        xm, om = xb[1:1 + n].view_as(x), ob[1:1 + n].view_as(x)
        assert xm.data_ptr() % 16 != 0 and om.data_ptr() % 16 != 0
        xm.copy_(x)
        _ops.mix_batch(xm, tab, out=om)
        assert torch.equal(_bits(om), _bits(out))
        assert float(ob[0]) == -7.0 and bool((ob[1 + n:] == -7.0).all()) and bool((xb[1 + n:] == 3.0).all())
        # only one of the two misaligned: still the element form, still the same bits
        assert torch.equal(_bits(_ops.mix_batch(xm, tab)), _bits(out))
    print(f"{dtype} {(B, H, W)}: worst blend error = {worst:.3f} of the gate")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_mix_batch_does_not_read_the_partner_outside_a_w1_box(B, H, W, dtype):
    """NaN and inf planted in x[src] outside the boxes of the w == 1 rows: those rows' outputs stay bitwise x[i]
    there (and x[src] inside the box)."""
    x = _input(B, H, W, dtype, seed=1)
    for tab in _tables(B, H, W):
        src, w, box = _masks(tab, B, H, W)
        xp = x.cpu().clone()
        poison = torch.where(torch.arange(H * W).view(1, H, W) % 2 == 0, float("nan"), float("inf")).to(dtype)
        for i in range(B):
            if float(w[i]) == 1.0 and int(src[i]) != i:
                s = int(src[i])
                xp[s] = torch.where(box[i], xp[s], poison.expand(3, H, W))
        xp = xp.to(DEV)
        out = _ops.mix_batch(xp, tab).cpu()
        xpc = xp.cpu()
        for i in range(B):
            if float(w[i]) == 1.0:
                want = torch.where(box[i], xpc[int(src[i])], xpc[i])
                assert torch.equal(_bits(out[i]), _bits(want)), (i, tab)


def test_mix_batch_refusals_on_the_device():
    x = _input(4, 16, 16, torch.float32)
    tab = _tables(4, 16, 16)[0]
    with pytest.raises(RuntimeError, match="overlap"):
        _ops.mix_batch(x, tab, out=x)
    with pytest.raises(ValueError, match="mix table"):
        _ops.mix_batch(x, ([4, 0, 0, 0], *tab[1:]))
    with pytest.raises(TypeError):
        _ops.mix_batch(x.half(), tab)


# ---------------------------------------------------------------------------------------------------------------------
# BatchMix / DeviceBatches on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_batch_mix_device_against_host_path(dtype):
    B, H, W = 6, 16, 24
    x = _input(B, H, W, dtype, seed=2)
    y = torch.randint(0, 10, (B,), device=DEV)
    x0 = x.clone()
    for per_image in (False, True):
        on_dev, on_host, twin = (data.BatchMix(0.8, 1.0, per_image=per_image, seed=11) for _ in range(3))
        for _ in range(4):
            out, labels = on_dev(x, y)
            out_h, labels_h = on_host(x.cpu(), y.cpu())
            tab = twin.draw(B, H, W)
            assert torch.equal(_bits(x), _bits(x0)) and out.dtype == dtype and out.is_cuda
            _check_mix(out, x, tab[:6])
            _check_mix(out_h, x.cpu(), tab[:6])
            assert isinstance(labels, MixedLabels) and all(t.is_cuda for t in labels)
            for got, want in zip(labels, labels_h):
                assert got.dtype == want.dtype and torch.equal(got.cpu(), want)
            assert torch.equal(labels.a, y) and torch.equal(labels.b, y.flip(0))
            assert np.array_equal(labels.lam.cpu().numpy(), tab.lam)


def test_device_batches_with_mix():
    """Three batches of SyntheticRawImages, unshuffled, 32x32 -> 64: the mixing iterator equals the unmixed iterator's
    batches mixed on the host by an equally seeded BatchMix."""
    ds = data.SyntheticRawImages(12, size=(32, 32, 3), classes=10, seed=4)
    mk = lambda: data.raw_loader(ds, batch_size=4, shuffle=False, num_workers=0, pin_memory=True)     # noqa: E731
    plain = [(x.cpu(), y.cpu()) for x, y in data.DeviceBatches(mk(), data.GpuImageTransform(64), "cuda")]
    mixed = []
    for x, y in data.DeviceBatches(mk(), data.GpuImageTransform(64), "cuda",
                                   mix=data.BatchMix(0.8, 1.0, per_image=True, seed=9)):
        assert isinstance(y, MixedLabels) and x.is_cuda and all(t.is_cuda for t in y)
        mixed.append((x.cpu(), MixedLabels(*(t.cpu() for t in y))))
    assert len(plain) == len(mixed) == 3
    host, twin = (data.BatchMix(0.8, 1.0, per_image=True, seed=9) for _ in range(2))
    for (x, y), (xm, ym) in zip(plain, mixed):
        xh, yh = host(x, y)
        tab = twin.draw(4, 64, 64)
        _check_mix(xm, x, tab[:6])
        _check_mix(xh, x, tab[:6])
        assert all(torch.equal(a, b) for a, b in zip(ym, yh))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _model(ocfg, dtype=torch.float32):
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)
    torch.manual_seed(0)
    return vit.VisionTransformer(c).to(DEV)


def _oracle_mixed(st, x_mixed, labels, ocfg, eps, **kw):
    """O.forward on the mixed input with autograd parameters, then F.cross_entropy on the dense target."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in st.items()}
    logits = O.forward(params, x_mixed, ocfg, **kw)
    loss = F.cross_entropy(logits, dense_target(labels, ocfg.num_classes, dtype=logits.dtype), label_smoothing=eps)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in params.items()}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(b.double().norm(), 1e-30))


def test_mixed_smoothed_step_fp32_vs_oracle():
    """test_hd64_fp32_vs_oracle's model (D = 128, H = 2, L = 2, 64x64, fp32, train mode, and its batch of 3, so the
    forward takes the paths it takes there) on a BatchMix(0.8, 1.0, per_image) input with the smoothed two-label loss,
    at that test's gates: logits 1e-4, loss 1e-5, gradients 2e-4 scaled."""
    ocfg = O.make_config("micro", img=64, batch=3, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    st = O.init_state(ocfg, seed=1)
    m = _model(ocfg)
    m.load_state_dict(st)
    m.train(True)
    x, y = O.synthetic_batch(ocfg)
    xm, labels = data.BatchMix(mixup_alpha=0.8, cutmix_alpha=1.0, per_image=True, seed=21)(x.to(DEV), y.to(DEV))
    assert not torch.equal(xm.cpu(), x)
    torch.manual_seed(42)
    base_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(42)
    logits = m(xm)
    loss = cross_entropy(logits, labels, label_smoothing=0.1)
    loss.backward()
    cpu_labels = MixedLabels(*(t.cpu() for t in labels))
    lg_ref, loss_ref, g_ref = _oracle_mixed(st, xm.cpu(), cpu_labels, ocfg, 0.1, train=True, seed=base_seed)
    print(f"logits {float((logits.detach().cpu() - lg_ref).abs().max()):.3e}, loss {abs(loss.item() - loss_ref.item()):.3e}")
    assert (logits.detach().cpu() - lg_ref).abs().max().item() < 1e-4
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    for k, p in m.named_parameters():
        err = (p.grad.cpu() - g_ref[k]).abs().max().item()
        assert err <= 2e-4 * max(1.0, g_ref[k].abs().max().item()), (k, err)
    # and the loss is not the hard-label one
    assert abs(loss.item() - F.cross_entropy(lg_ref, y).item()) > 1e-3


def test_mixed_smoothed_step_bf16_vs_oracle_same_rounding():
    """The bf16 engine (hd = 64) on the same kind of input and loss, in test_bf16_vs_oracle_same_rounding's gate form:
    logits within 1e-2 (norm-wise) of the bf16-rounding oracle, every gradient's error against the fp32 oracle no worse
    than max(1e-2, 2x) that oracle's own."""
    ocfg = O.make_config("micro", img=64, batch=4, blocks=2)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    st = O.init_state(ocfg, seed=2)
    m = _model(ocfg, dtype=torch.bfloat16)
    m.load_state_dict(st)
    m.eval()
    x, y = O.synthetic_batch(ocfg)
    xm, labels = data.BatchMix(mixup_alpha=0.8, cutmix_alpha=1.0, per_image=True, seed=22)(x.to(DEV), y.to(DEV))
    logits = m(xm)
    loss = cross_entropy(logits, labels, label_smoothing=0.1)
    loss.backward()
    cpu_labels = MixedLabels(*(t.cpu() for t in labels))
    lg_bf, _, g_bf = _oracle_mixed(st, xm.cpu(), cpu_labels, ocfg, 0.1, bf16=True)
    lg_32, loss_32, g_32 = _oracle_mixed(st, xm.cpu(), cpu_labels, ocfg, 0.1)
    assert _rel(logits.detach().cpu(), lg_bf) < 1e-2
    assert abs(loss.item() - loss_32.item()) < 0.1
    for k, p in m.named_parameters():
        ours, ora = _rel(p.grad.cpu(), g_32[k]), _rel(g_bf[k], g_32[k])
        assert ours <= max(1e-2, 2 * ora), (k, ours, ora)


def test_train_with_smoothing_mixup_cutmix_clipping_and_ema(tmp_path):
    """Two short epochs of train() with label smoothing, mixup and CutMix, FusedAdamW clipping and keeping an EMA: a
    finite loss, validation on the unmixed loader, a checkpoint that reloads."""
    sys.path.insert(0, os.path.join(ROOT, "vision-transformer_amd"))
    import train as T
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4, precision=torch.bfloat16)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(16, 3, 64, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, 64, 10, seed=4), batch_size=4)
    seen = []
    real_evaluate = T.evaluate

    def spy(model, ld, fn, avg=None):
        seen.append(ld)
        return real_evaluate(model, ld, fn, avg)

    T.evaluate = spy
    try:
        ck, logs = str(tmp_path / "ck"), str(tmp_path / "logs")
        last = T.train(cfg, loader, test_loader, epochs=1, eval_iter=1, log_dir=logs, checkpoint_dir=ck, lr=1e-3,
                       max_grad_norm=1.0, ema_decay=0.99, label_smoothing=0.1,
                       mix=data.BatchMix(0.8, 1.0, per_image=True, seed=5))
    finally:
        T.evaluate = real_evaluate
    assert math.isfinite(last) and last > 0
    assert len(seen) == 2 and all(ld is test_loader for ld in seen)
    assert sorted(os.listdir(ck)) == ["0.pt", "1.pt"]
    ckpt = torch.load(os.path.join(ck, "1.pt"), map_location="cpu", weights_only=True)
    assert ckpt["step"] == 8 and math.isfinite(ckpt["loss"]) and "ema_state_dict" in ckpt
    fresh = vit.VisionTransformer(cfg)
    fresh.load_state_dict(ckpt["model_state_dict"])
    fresh.load_state_dict(ckpt["ema_state_dict"])
    opt = FusedAdamW(fresh.parameters(), lr=1e-3, ema_decay=0.99, max_grad_norm=1.0)
    opt.load_state_dict(ckpt["optimizer_state_dict"])
    sec, loss = T.time_steps(cfg, 2, 1, dev="cuda", label_smoothing=0.1, mix=data.BatchMix(0.8, 1.0))
    assert sec > 0 and math.isfinite(loss)
