"""GPU tests of the validation metrics: vit_eval_update against the sort-by-key reference of tests/eval_reference.py
(integers compared with ==, the loss with test_softmax_xent's gate), its ties, NaNs, row stride, ignored labels,
accumulation, repeatability and NULL confusion matrix; DeviceMetrics on the device against itself on the host;
validate() on the tiny model; and train(val_topk=...)."""
import functools
import json

import numpy as np
import pytest
import torch

from eval_reference import loss_gate, nan_cases, reference, tie_cases, xent_logits
from VisionTransformer import _ops, config, vit
from VisionTransformer import metrics as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

XENT_SHAPES = [(1, 4, False), (8, 10, False), (37, 257, True), (300, 1000, False)]      # test_softmax_xent's
EDGE_SHAPES = [(65, 63, False), (65, 64, False), (65, 65, False), (5, 1, False)]


@functools.lru_cache(maxsize=None)
def _case(rows, classes, extreme):
    """Logits, labels and their reference at the largest maxk, computed once and shared (nothing mutates them)."""
    lg, lb = xent_logits(rows, classes, extreme)
    return lg, lb, reference(lg, lb, min(16, classes))


def _counts(ref, maxk):
    return ref["counts"][:2 + maxk]


def _state(classes, maxk, confusion=True):
    return (torch.zeros(2 + maxk, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV),
            torch.zeros(classes, classes, dtype=torch.int64, device=DEV) if confusion else None)


def _run(lg, lb, maxk, state=None, confusion=True, rows=None):
    """One vit_eval_update on device copies; returns everything on the host."""
    lg = lg if lg.is_cuda else lg.to(DEV)
    lb = lb if lb.is_cuda else lb.to(DEV)
    counts, loss, cm = state if state is not None else _state(lg.shape[1], maxk, confusion)
    pred, rank, row_loss = _ops.eval_update(lg, lb, counts, loss, cm, rows=rows, maxk=maxk)
    torch.cuda.synchronize()
    return {"pred": pred.cpu().numpy(), "rank": rank.cpu().numpy(), "row_loss": row_loss.cpu(),
            "counts": counts.cpu().numpy(), "loss_sum": float(loss.cpu()), "loss_bits": int(loss.cpu().view(torch.int64)),
            "confusion": None if cm is None else cm.cpu().numpy()}


def _assert_integers(got, ref, maxk):
    assert got["pred"].dtype == np.int64 and got["rank"].dtype == np.int32
    assert (got["pred"] == ref["pred"]).all()
    assert (got["rank"] == ref["rank"]).all()
    assert (got["counts"] == _counts(ref, maxk)).all()
    if got["confusion"] is not None:
        assert (got["confusion"] == ref["confusion"]).all()


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("rows,classes,extreme", XENT_SHAPES + EDGE_SHAPES)
def test_kernel_against_the_reference(rows, classes, extreme):
    """test_softmax_xent's shapes and logits, then one past a wave of rows around a wave of columns, and one class;
    maxk in {1, min(5, classes), min(16, classes)}."""
    lg, lb, ref = _case(rows, classes, extreme)
    lref = float(torch.nn.functional.cross_entropy(lg.double(), lb))
    for maxk in sorted({1, min(5, classes), min(16, classes)}):
        got = _run(lg, lb, maxk)
        _assert_integers(got, ref, maxk)
        assert got["counts"][0] == rows and got["counts"][1] == 0
        mean = got["loss_sum"] / got["counts"][0]
        print(f"rows {rows} classes {classes} maxk {maxk}: loss {mean!r} ref {lref!r}")
        assert loss_gate(mean, lref), (mean, lref)
        want = float(got["row_loss"].double().sum())
        assert _rel(got["loss_sum"], want) <= 1e-12 or got["loss_sum"] == want


def test_ties():
    x, y = tie_cases()
    ref = reference(x, y, 10)
    for maxk in (1, 5, 10):
        got = _run(x, y, maxk)
        _assert_integers(got, ref, maxk)
    assert ((got["rank"] == 0) == (got["pred"] == y.numpy())).all()
    assert got["pred"][3] == 0 and got["rank"][3] == 7             # a row of zeros
    assert got["pred"][4] == 0 and got["pred"][5] == 0             # -0.0 beside +0.0


def test_nan():
    x, y = nan_cases()
    got = _run(x, y, 5)
    assert (got["pred"] == torch.argmax(x, 1).numpy()).all()      # torch.argmax of the CPU copy
    _assert_integers(got, reference(x, y, 5), 5)


@pytest.mark.parametrize("rows,classes,extreme", [(37, 257, True), (65, 63, False)])
def test_row_stride(rows, classes, extreme):
    """ld = classes + 3 with NaN in the padding columns: the result of the contiguous case, bit for bit."""
    lg, lb, ref = _case(rows, classes, extreme)
    maxk = min(5, classes)
    wide = torch.full((rows, classes + 3), float("nan"), device=DEV)
    wide[:, :classes] = lg.to(DEV)
    view = wide[:, :classes]
    assert view.stride(0) == classes + 3
    got, flat = _run(view, lb, maxk), _run(lg, lb, maxk)
    _assert_integers(got, ref, maxk)
    assert got["loss_bits"] == flat["loss_bits"] and torch.equal(got["row_loss"], flat["row_loss"])


def test_ignored_labels():
    """Labels -1, classes and classes + 7 index nothing.  The matrix is a view into a larger buffer with 8 guard rows
    of a sentinel on each side, so a wrong index would land in allocated memory and show."""
    rows, classes, maxk = 37, 10, 5
    lg, lb = xent_logits(rows, classes, False, seed=77)
    lb = lb.clone()
    bad = {2: -1, 11: classes, 12: classes + 7, 36: -1}
    for i, v in bad.items():
        lb[i] = v
    ref = reference(lg, lb, maxk)
    buf = torch.full((8 + classes + 8, classes), -77, dtype=torch.int64, device=DEV)
    cm = buf[8:8 + classes]
    cm.zero_()
    counts, loss, _ = _state(classes, maxk, confusion=False)
    got = _run(lg, lb, maxk, state=(counts, loss, cm))
    _assert_integers(got, ref, maxk)
    assert got["counts"][1] == len(bad) and got["counts"][0] == rows - len(bad)
    assert bool((buf[:8] == -77).all()) and bool((buf[8 + classes:] == -77).all())
    assert all(got["rank"][i] == -1 and got["row_loss"][i] == 0 for i in bad)
    keep = [i for i in range(rows) if i not in bad]
    clean = _run(lg[keep], lb[keep], maxk)                         # the scored rows are unaffected
    assert (got["rank"][keep] == clean["rank"]).all() and torch.equal(got["row_loss"][keep], clean["row_loss"])
    assert (got["confusion"] == clean["confusion"]).all() and (got["counts"][2:] == clean["counts"][2:]).all()


def test_accumulation_over_splits():
    """Rows [0, 100), [100, 101) and [101, 300) of the (300, 1000) case into one state: the single call's integers
    exactly, its loss sum to 1e-12 relative."""
    lg, lb, ref = _case(300, 1000, False)
    maxk = 5
    whole = _run(lg, lb, maxk)
    state = _state(1000, maxk)
    d_lg, d_lb = lg.to(DEV), lb.to(DEV)
    for lo, hi in ((0, 100), (100, 101), (101, 300)):
        part = _run(d_lg[lo:hi], d_lb[lo:hi], maxk, state=state)
        assert (part["pred"] == ref["pred"][lo:hi]).all() and (part["rank"] == ref["rank"][lo:hi]).all()
    assert (part["counts"] == whole["counts"]).all() and (part["counts"] == _counts(ref, maxk)).all()
    assert (part["confusion"] == whole["confusion"]).all()
    assert _rel(part["loss_sum"], whole["loss_sum"]) <= 1e-12


def test_repeatable_and_null_confusion():
    """Two runs from a zeroed state are bitwise equal, the loss sum included; without a matrix everything else is the
    same."""
    lg, lb, ref = _case(300, 1000, False)
    a, b, c = _run(lg, lb, 16), _run(lg, lb, 16), _run(lg, lb, 16, confusion=False)
    assert c["confusion"] is None
    _assert_integers(c, ref, 16)
    for other in (b, c):
        assert a["loss_bits"] == other["loss_bits"] and torch.equal(a["row_loss"], other["row_loss"])
        assert (a["pred"] == other["pred"]).all() and (a["rank"] == other["rank"]).all()
        assert (a["counts"] == other["counts"]).all()
    assert (a["confusion"] == b["confusion"]).all()


def test_device_metrics_against_the_host_twin():
    """Three batches, `rows=` on the last, ties and an ignored label among them: the object on the device against the
    same object fed CPU copies."""
    g = torch.Generator().manual_seed(21)
    batches = []
    for b in range(3):
        x = (torch.randn(32, 10, generator=g) * 4).round() / 4     # a coarse grid: ties occur
        y = torch.randint(0, 10, (32,), generator=g)
        batches.append((x, y))
    batches[1][1][5] = -1
    dev, host = M.DeviceMetrics(10, topk=(1, 5), device=DEV), M.DeviceMetrics(10, topk=(1, 5))
    for i, (x, y) in enumerate(batches):
        rows = 20 if i == 2 else None
        assert dev.update(x.to(DEV), y.to(DEV), rows=rows) is None
        host.update(x, y, rows=rows)
    got, want = dev.compute(), host.compute()
    assert dev.host_reads == 1
    assert got["n"] == want["n"] == 32 + 31 + 20 and got["ignored"] == want["ignored"] == 1
    assert got["top1"] == want["top1"] and got["top5"] == want["top5"] and got["support"] == want["support"]
    assert torch.equal(got["confusion"], want["confusion"]) and not got["confusion"].is_cuda
    assert loss_gate(got["loss"], want["loss"])
    for k in ("precision", "recall", "f1"):
        assert np.abs(np.array(got[k]) - np.array(want[k])).max() <= 1e-12
        for avg in ("macro", "weighted"):
            assert abs(got[avg][k] - want[avg][k]) <= 1e-12
    dev.reset()
    assert dev.compute()["n"] == 0
    with pytest.raises(ValueError, match="topk"):
        M.DeviceMetrics(4, topk=(1, 5), device=DEV)


class _Recorded(M.DeviceMetrics):
    made = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        _Recorded.made.append(self)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_validate_on_the_tiny_model(dtype, monkeypatch):
    """ViT-Tiny 64^2 B 8 on 13 samples (a padded last batch): the integers of the reference on the logits of a plain
    model(x) loop over the same batches, top1 == evaluate(..., accuracy_score), one host read."""
    import train as T
    from sklearn.metrics import accuracy_score
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(M, "DeviceMetrics", _Recorded)
    _Recorded.made = []
    cfg = config.ViTConfig(3, 10, 16, 192, 16, 3, 12, "cpu", 8, precision=dtype)
    torch.manual_seed(0)
    model = vit.VisionTransformer(cfg).to(DEV).eval()
    ts = T.SyntheticImages(13, 3, 64, 10, seed=7)
    loader = torch.utils.data.DataLoader(ts, batch_size=8)
    out = T.validate(model, loader, topk=(1, 5), confusion=True)
    assert len(_Recorded.made) == 1 and _Recorded.made[0].host_reads == 1
    assert not model.training
    x, y = next(iter(torch.utils.data.DataLoader(ts, batch_size=13)))
    with torch.no_grad():
        xp = torch.cat([x, x[-1:].expand(3, 3, 64, 64)]).to(DEV)
        logits = torch.cat([model(xp[i:i + 8]) for i in range(0, 16, 8)])[:13].float().cpu()
    ref = reference(logits, y, 5)
    assert out["n"] == 13 and out["ignored"] == 0
    assert out["top1"] == ref["counts"][2] / 13 and out["top5"] == ref["counts"][2:7].sum() / 13
    assert (out["confusion"].numpy() == ref["confusion"]).all()
    assert loss_gate(out["loss"], float(torch.nn.functional.cross_entropy(logits.double(), y)))
    acc = T.evaluate(model, loader, accuracy_score)
    assert abs(out["top1"] - acc) <= 1e-12


def test_train_with_val_topk(tmp_path, monkeypatch):
    """train(val_topk=(1, 3), val_confusion=True, ema_decay=0.9), 2 epochs of 2 steps: the tags and the checkpoint key
    are there and val?acc is the rounded top-1; with val_topk=None the tags and keys are the loop's own."""
    import train as T
    monkeypatch.setattr(T, "device", "cuda")
    monkeypatch.setattr(T, "_writer", T._JsonlWriter)
    cfg = config.ViTConfig(3, 10, 16, 128, 16, 2, 2, "cpu", 4)
    loader = torch.utils.data.DataLoader(T.SyntheticImages(8, 3, 64, 10, seed=3), batch_size=4, drop_last=True)
    test_loader = torch.utils.data.DataLoader(T.SyntheticImages(13, 3, 64, 10, seed=4), batch_size=4)

    def run(name, **kw):
        T.train(cfg, loader, test_loader, epochs=1, eval_iter=1, log_dir=str(tmp_path / name), max_steps=2,
                checkpoint_dir=str(tmp_path / (name + "_ck")), lr=1e-3, ema_decay=0.9, **kw)
        ck = torch.load(tmp_path / (name + "_ck") / "1.pt", map_location="cpu", weights_only=True)
        return ck, [json.loads(ln) for ln in open(tmp_path / name / "scalars.jsonl")]

    base = {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "step", "ema_state_dict"}
    ck, tags = run("plain")
    assert set(ck) == base and {t["tag"] for t in tags} == {"Loss/train_batch", "val?acc"}
    ck, tags = run("val", val_topk=(1, 3), val_confusion=True)
    assert set(ck) == base | {"val_metrics"}
    assert {t["tag"] for t in tags} == {"Loss/train_batch", "val?acc", "Loss/val", "Acc1/val", "Acc3/val"}
    vm = ck["val_metrics"]
    last = {t["tag"]: t["value"] for t in tags if t["step"] == 1 and t["tag"] != "Loss/train_batch"}
    assert vm["n"] == 13 and np.array(vm["confusion"]).shape == (10, 10) and np.array(vm["confusion"]).sum() == 13
    assert last["val?acc"] == round(vm["top1"], 2)
    assert last["Acc1/val"] == vm["top1"] and last["Acc3/val"] == vm["top3"] and last["Loss/val"] == vm["loss"]
