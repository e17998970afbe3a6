"""The reference of the validation-metric tests (tests/test_eval_metrics_cpu.py, tests/test_gpu_eval_metrics.py),
written from the rules of include/vit_hip.h "vit_eval_update" and from nothing else: sort each row by the key
(is-NaN, value, minus index), largest first; the prediction is the first entry and the rank of a label its position."""
import numpy as np
import torch


def reference(logits, labels, maxk):
    """pred int64 [R], rank int32 [R] (-1: label outside [0, C)), counts int64 [2 + maxk], confusion int64 [C, C] of
    `logits` ([R, C], any float tensor or array) and `labels` ([R] integers), all numpy."""
    x = np.asarray(torch.as_tensor(logits).detach().cpu().float().numpy())
    y = [int(v) for v in torch.as_tensor(labels).detach().cpu().tolist()]
    R, C = x.shape
    pred, rank = np.zeros(R, np.int64), np.zeros(R, np.int32)
    counts, confusion = np.zeros(2 + maxk, np.int64), np.zeros((C, C), np.int64)
    for i in range(R):
        row = x[i].tolist()
        order = sorted(range(C), key=lambda c: (row[c] != row[c], 0.0 if row[c] != row[c] else row[c], -c),
                       reverse=True)
        pred[i] = order[0]
        if not 0 <= y[i] < C:
            rank[i] = -1
            counts[1] += 1
            continue
        rank[i] = order.index(y[i])
        counts[0] += 1
        if rank[i] < maxk:
            counts[2 + rank[i]] += 1
        confusion[y[i], pred[i]] += 1
    return {"pred": pred, "rank": rank, "counts": counts, "confusion": confusion}


def xent_logits(rows, classes, extreme, seed=None):
    """tests/test_gpu_contract.py::test_softmax_xent's logits and labels, on the CPU: a 2^-10 grid of N(0, 16) draws;
    `extreme` clamps to +-60 and plants an 80 and a -80 in every row.  Labels include class 0 and classes - 1."""
    g = torch.Generator().manual_seed(16 + classes if seed is None else seed)
    lg = (torch.randn(rows, classes, generator=g) * 4 * 1024).round() / 1024
    if extreme:
        lg = lg.clamp(-60, 60)
        idx = torch.arange(rows)
        lg[idx, idx % classes] = 80.0
        lg[idx, (idx + 5) % classes] = -80.0
    lb = torch.randint(0, classes, (rows,), generator=g)
    lb[0] = 0
    lb[-1] = classes - 1 if rows > 1 else 0
    if rows > 2:
        lb[1] = classes - 1
    return lg, lb


def loss_gate(got, ref):
    """The project's xent gate (test_softmax_xent): |got - ref| <= 1e-5 * max(1, |ref|)."""
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def tie_cases():
    """(name, logits [R, 10], labels [R]) with ties: draws from {-1, 0, 1} at (64, 10), a row of zeros among them, and
    -0.0 beside +0.0."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-1, 2, (64, 10), generator=g).float()
    x[3] = 0.0
    x[4] = torch.tensor([0.0, -0.0] * 5)
    x[5] = torch.tensor([-0.0, 0.0] * 5)
    x[6] = torch.tensor([-1.0, -0.0, 0.0, -1.0, 0.0, -0.0, -1.0, -1.0, -1.0, -1.0])
    y = torch.randint(0, 10, (64,), generator=g)
    y[3], y[4], y[5], y[6] = 7, 1, 0, 2
    return x, y


def nan_cases():
    """Rows with one NaN and with two, the label on a NaN, before it and after it, among random rows."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(12, 10, generator=g)
    y = torch.randint(0, 10, (12,), generator=g)
    nan = float("nan")
    x[0, 4] = nan
    y[0] = 4
    x[1, 9] = nan
    y[1] = 0
    x[2, 0] = nan
    y[2] = 9
    x[3, 2] = x[3, 7] = nan
    y[3] = 7                                   # the second NaN: one entry precedes it
    x[4, 2] = x[4, 7] = nan
    y[4] = 2
    x[5, 0] = x[5, 9] = nan
    y[5] = 5                                   # a number: both NaNs precede it
    x[6, 3] = nan
    x[6, 5] = float("inf")
    y[6] = 5                                   # +inf ranks after the NaN
    return x, y
