"""Validation metrics whose state stays on the device until the epoch ends (include/vit_hip.h "vit_eval_update").

`DeviceMetrics` accumulates, per batch of logits and with no host read, the scored and ignored row counts, the rank
histogram of the labels (top-k for every k up to 16), the fp64 sum of the cross-entropy row terms and the confusion
matrix.  `compute()` is the one transfer; it derives the loss, the top-k accuracies and per-class precision / recall /
f1 / support with their macro and weighted averages (scikit-learn's `zero_division=0` conventions, over all
`num_classes` classes).

Order of a row's entries, one rule for the prediction and for every top-k: entry c precedes entry d when x[c] > x[d],
or when they compare equal and c < d; a NaN is greater than every number and equal to another NaN.  The prediction is
the first entry (torch.argmax on the CPU), the rank of a label the number of entries that precede it, top-k is
rank < k.  A label outside [0, num_classes) is ignored and counted as such.

Device tensors go through the HIP kernels; CPU tensors through `eval_update_host`, the same semantics in torch ops (the
host path of train.py uses it)."""
import torch
import torch.distributed as dist

from . import _lib, _ops


def eval_update_host(logits, labels, counts, loss_sum, confusion=None, rows=None, maxk=None):
    """The host twin of _ops.eval_update: same arguments (CPU tensors), same accumulation, same return value."""
    classes = logits.shape[1]
    rows = logits.shape[0] if rows is None else int(rows)
    maxk = counts.numel() - 2 if maxk is None else int(maxk)
    if not 0 < rows <= logits.shape[0] or labels.numel() < rows:
        raise ValueError(f"rows = {rows} needs that many rows of logits and labels (got {logits.shape[0]}, "
                         f"{labels.numel()})")
    if not 1 <= maxk <= min(classes, _lib.EVAL_MAXK):
        raise ValueError(f"maxk must lie in [1, min(classes, {_lib.EVAL_MAXK})] (got {maxk} for {classes} classes)")
    x = logits[:rows].float()
    y = labels[:rows].to(torch.int64)
    nan = torch.isnan(x)
    pred = torch.where(nan.any(1), nan.to(torch.int8).argmax(1), x.argmax(1))
    scored = (y >= 0) & (y < classes)
    ys = torch.where(scored, y, torch.zeros_like(y)).unsqueeze(1)
    xy, ny = x.gather(1, ys), nan.gather(1, ys)
    gt = (nan & ~ny) | (~nan & ~ny & (x > xy))
    eq = (nan & ny) | (x == xy)
    first = torch.arange(classes).unsqueeze(0) < ys
    rank = (gt | (eq & first)).sum(1).to(torch.int32)
    rank = torch.where(scored, rank, torch.full_like(rank, -1))
    row_loss = torch.where(scored, torch.logsumexp(x, 1) - xy.squeeze(1), torch.zeros(rows))
    counts[0] += int(scored.sum())
    counts[1] += rows - int(scored.sum())
    r = rank[scored].to(torch.int64)
    counts[2:2 + maxk] += torch.bincount(r[r < maxk], minlength=maxk)
    loss_sum += row_loss.double().sum()
    if confusion is not None:
        cell = ys.squeeze(1)[scored] * classes + pred[scored]
        confusion.view(-1)[:classes * classes] += torch.bincount(cell, minlength=classes * classes)
    return pred, rank, row_loss


def _ratio(num, den):
    """num / den elementwise in fp64, 0 where den == 0 (scikit-learn's zero_division=0)."""
    num, den = num.double(), den.double()
    return torch.where(den > 0, num / den.clamp(min=1), torch.zeros_like(num))


def class_report(confusion):
    """Per-class precision / recall / f1 / support and their macro and weighted averages from a confusion matrix (row =
    label, column = prediction), as sklearn.metrics.precision_recall_fscore_support(labels=range(classes),
    zero_division=0) gives them."""
    cm = confusion.to(torch.int64)
    tp, support, predicted = cm.diagonal(), cm.sum(1), cm.sum(0)
    per = {"precision": _ratio(tp, predicted), "recall": _ratio(tp, support), "f1": _ratio(2 * tp, predicted + support)}
    total = support.sum()
    out = {k: v.tolist() for k, v in per.items()}
    out["support"] = support.tolist()
    out["macro"] = {k: float(v.mean()) for k, v in per.items()}
    out["weighted"] = {k: float(_ratio((v * support.double()).sum(), total)) for k, v in per.items()}
    return out


def jsonable(result):
    """A compute() dict with the confusion matrix as nested lists: what a checkpoint or a JSON line stores."""
    return {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in result.items()}


class DeviceMetrics:
    """DeviceMetrics(num_classes, topk=(1, 5), confusion=True, device=None, keep_predictions=False).

    update(logits, labels, rows=None) scores the first `rows` rows of a batch and returns nothing; reset() zeroes the
    state; all_reduce(group=None) sums it over the ranks of a process group (two tensor all-reduces, gloo or nccl, no
    pickled objects); compute() copies the state to the host once, counts that in `host_reads`, and returns
    {n, ignored, loss, top{k}..., confusion (CPU int64 tensor, when kept), precision, recall, f1, support (lists per
    class), macro, weighted ({precision, recall, f1})}.  With `keep_predictions` every batch's predictions stay on the
    device and predictions() returns them as one tensor."""

    def __init__(self, num_classes, topk=(1, 5), confusion=True, device=None, keep_predictions=False):
        self.num_classes = int(num_classes)
        self.topk = tuple(sorted({int(k) for k in topk}))
        if self.num_classes < 1 or not self.topk:
            raise ValueError("DeviceMetrics needs at least one class and one k")
        if self.topk[0] < 1 or self.topk[-1] > min(self.num_classes, _lib.EVAL_MAXK):
            raise ValueError(f"topk entries must lie in [1, min(num_classes, {_lib.EVAL_MAXK})] (got {self.topk} for "
                             f"{self.num_classes} classes)")
        self.maxk = self.topk[-1]
        self.device = torch.device(device if device is not None else "cpu")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # one buffer, so that compute() is one transfer: the fp64 loss sum's bits, the counts, the confusion matrix
        cells = self.num_classes ** 2 if confusion else 0
        self._state = torch.zeros(3 + self.maxk + cells, dtype=torch.int64, device=self.device)
        self.loss_sum = self._state[:1].view(torch.float64)
        self.counts = self._state[1:3 + self.maxk]
        self.confusion = self._state[3 + self.maxk:].view(self.num_classes, self.num_classes) if confusion else None
        self.keep_predictions = bool(keep_predictions)
        self._preds = []
        self.host_reads = 0

    def reset(self):
        self._state.zero_()
        self._preds = []

    def update(self, logits, labels, rows=None):
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"logits must be [rows, {self.num_classes}] (got {tuple(logits.shape)})")
        if logits.device != self.device or labels.device != self.device:
            raise ValueError(f"logits and labels must be on {self.device} (got {logits.device}, {labels.device})")
        logits = logits.detach()
        if logits.dtype != torch.float32:
            logits = logits.float()
        if self.num_classes > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        labels = labels.detach().to(torch.int64).contiguous()
        update = _ops.eval_update if self.device.type == "cuda" else eval_update_host
        pred, _, _ = update(logits, labels, self.counts, self.loss_sum, self.confusion, rows=rows, maxk=self.maxk)
        if self.keep_predictions:
            self._preds.append(pred)

    def all_reduce(self, group=None):
        dist.all_reduce(self._state[1:], group=group)
        dist.all_reduce(self.loss_sum, group=group)

    def predictions(self):
        if not self.keep_predictions:
            raise RuntimeError("DeviceMetrics was built without keep_predictions=True")
        return torch.cat(self._preds) if self._preds else torch.zeros(0, dtype=torch.int64, device=self.device)

    def compute(self):
        host = self._state.to("cpu")
        self.host_reads += 1
        counts = host[1:3 + self.maxk]
        n = int(counts[0])
        out = {"n": n, "ignored": int(counts[1]),
               "loss": float(host[:1].view(torch.float64)) / n if n else 0.0}
        hits = counts[2:].cumsum(0)
        for k in self.topk:
            out[f"top{k}"] = float(hits[k - 1]) / n if n else 0.0
        if self.confusion is not None:
            out["confusion"] = host[3 + self.maxk:].view(self.num_classes, self.num_classes).clone()
            out.update(class_report(out["confusion"]))
        return out
