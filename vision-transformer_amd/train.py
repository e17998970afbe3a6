"""Training entry point — drop-in for the reference's src/train.py (run from this directory, like the reference).

Same public functions: `evaluate(model, test_loader, eval_func, avg=None)` (train.py:29-44),
`search_checkpoint(dir)` (:52-58), `train(configs, train_loader, test_loader, epochs, eval_iter, log_dir,
checkpoint_dir, lr=1e-4)` (:60-119), and the same checkpoint dict {epoch, model_state_dict, optimizer_state_dict,
loss, step} (:107-113), so checkpoints interchange with the reference (per-head state_dict keys, torch AdamW state
keys).  The hot loop (:89-102) runs on the MI355X path: fused HIP forward/backward, fused softmax cross-entropy,
FusedAdamW (one multi-tensor launch), and — under torchrun — gradient all-reduce over RCCL overlapped with the
backward.  The per-step `loss.item()` host sync of the reference is kept only when logging asks for it.
Without a GPU (or with `--device cpu`) the same loop runs the package's host path (VisionTransformer/_cpu.py, plain
torch ops on all host cores, torch.optim.AdamW) — the reference's own behaviour (train.py:26,80) and BASELINE config 1
(ViT-Tiny/16 64^2 B8 fp32, `python train.py --device cpu`).

Differences (documented in DESIGN.md): hyper-parameters come from flags instead of hard-coded constants (the
reference's TODO at :124-125); data defaults to a synthetic CIFAR-shaped stream because the container has no network
(CIFAR10(download=True) at :157-159 cannot run).  `--data cifar10-bin --data-root R` reads CIFAR-10's binary batches,
`--data folder --data-root R` a folder-per-class image tree (BrainTumorDataset.py), `--data synthetic-u8` random uint8
images; on the GPU those run the reference transform (convert RGB -> Resize((S, S)) -> ToTensor, train.py:151-155)
as one kernel per batch (VisionTransformer/data.py, bit-exact with Pillow), on the host with Pillow per image.
tensorboard is used when importable, else scalars go to a JSONL file.
"""
import argparse
import contextlib
import glob
import json
import os
import re
import time

import torch
import torch.distributed as dist

from VisionTransformer import config, vit
from VisionTransformer.optim import (LRSchedule, MixedLabels, cross_entropy, distillation_loss, make_optimizer,
                                     param_groups_layer_decay, param_groups_weight_decay)

device = "cuda" if torch.cuda.is_available() else "cpu"


class _JsonlWriter:
    """Minimal stand-in for tensorboard's SummaryWriter (tensorboard is not installed in this image)."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.f = open(os.path.join(log_dir, "scalars.jsonl"), "a")

    def add_scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step), "t": time.time()}) + "\n")
        self.f.flush()


def _writer(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=log_dir, flush_secs=10)
    except Exception:
        return _JsonlWriter(log_dir)


class ShardSampler(torch.utils.data.Sampler):
    """Rank `rank` of `world` reads indices rank, rank + world, ... < n in order: the shards partition the set exactly
    (DistributedSampler instead pads every shard to equal length with duplicates), so a sharded evaluate() scores
    every test sample once."""

    def __init__(self, dataset, rank=None, world=None):
        r, w = _rank_world()
        self.n = len(dataset)
        self.rank = r if rank is None else rank
        self.world = w if world is None else world

    def __iter__(self):
        return iter(range(self.rank, self.n, self.world))

    def __len__(self):
        return len(range(self.rank, self.n, self.world))


def _sampler_of(loader):
    for obj in (loader, getattr(loader, "loader", None)):
        if obj is None:
            continue
        for s in (getattr(obj, "sampler", None), getattr(getattr(obj, "batch_sampler", None), "sampler", None)):
            if isinstance(s, (torch.utils.data.DistributedSampler, ShardSampler)):
                return s
    return None


@torch.no_grad()
def evaluate(model, test_loader, eval_func, avg=None):
    """Mean over batches of eval_func(labels, argmax(logits)) (train.py:29-44).

    A partial last batch is padded to the model's batch size (the CLS parameter is batch-shaped, vit.py:32,41) and
    only its real rows are scored; the reference would raise there.  With such a batch the score is eval_func over
    the whole set (every sample weighted once, the same value a data-parallel run returns) instead of the mean of
    per-batch scores, which is kept whenever every batch is full (the reference's only working case).

    Under data parallelism (an initialized process group of world size > 1) every rank scores its own shard of the test
    set, the (label, prediction) pairs of all ranks are gathered, and eval_func runs once over the whole set, so every
    rank returns the same score — for accuracy, the exact whole-set accuracy.  Each sample counts once: a ShardSampler
    shard has no duplicates, and the padding duplicates DistributedSampler appends (the trailing samples of a shard
    whose global position is >= len(dataset)) are dropped."""
    model.eval()
    score = 0.0
    n = 0
    labs, preds = [], []
    pad_to = getattr(getattr(model, "vit_config", None), "batch_size", None)
    for tensors, labels in test_loader:
        rows = tensors.shape[0]
        if pad_to is not None and rows < pad_to:
            fill = tensors[-1:].expand(pad_to - rows, *tensors.shape[1:])
            tensors = torch.cat([tensors, fill], 0)
        logits = model(tensors.to(device, non_blocking=True))[:rows]
        predictions = torch.argmax(logits, axis=-1).to("cpu")
        labels = labels.to("cpu")
        labs.append(labels)
        preds.append(predictions)
        if avg is None:
            score += eval_func(labels, predictions)
        else:
            score += eval_func(labels, predictions, average=avg, zero_division=0.0)
        n += 1
    model.train()
    rank, world = _rank_world()
    lab = torch.cat(labs) if labs else torch.zeros(0, dtype=torch.long)
    pred = torch.cat(preds) if preds else torch.zeros(0, dtype=torch.long)
    if world == 1:
        if pad_to is None or all(len(v) == pad_to for v in labs):
            return score / max(n, 1)             # the reference's mean of per-batch scores (full batches only)
        # a padded partial batch: score the whole set once, as the data-parallel case does, so the same model reports
        # the same score on one rank and on many (a mean of per-batch scores would weight the partial batch fully)
        if avg is None:
            return float(eval_func(lab, pred))
        return float(eval_func(lab, pred, average=avg, zero_division=0.0))
    s = _sampler_of(test_loader)
    if isinstance(s, torch.utils.data.DistributedSampler) and not s.drop_last:
        keep = len(range(rank, len(s.dataset), world))           # the shard's samples before the padding
        lab, pred = lab[:keep], pred[:keep]
    gathered = [None] * world
    dist.all_gather_object(gathered, (lab.tolist(), pred.tolist()))
    all_lab = torch.tensor([v for g in gathered for v in g[0]], dtype=torch.long)
    all_pred = torch.tensor([v for g in gathered for v in g[1]], dtype=torch.long)
    if avg is None:
        return float(eval_func(all_lab, all_pred))
    return float(eval_func(all_lab, all_pred, average=avg, zero_division=0.0))


@torch.no_grad()
def validate(model, test_loader, topk=(1, 5), confusion=True):
    """Validation loss, top-k accuracies and the confusion matrix over `test_loader`, with no host read inside the
    loop (not in the reference, whose evaluate() above yields one score): every batch's logits are scored on the
    device into a metrics.DeviceMetrics, and its compute() dict — n, ignored, loss, top{k}, confusion, per-class
    precision / recall / f1 / support, macro and weighted averages — is returned after one transfer.

    Eval mode, restored afterwards.  A partial last batch is padded as evaluate() pads it and the padding is not
    scored.  Under data parallelism every rank scores its shard, the state is all-reduced once and every rank returns
    the whole-set result; each sample counts once: of a DistributedSampler's padded shard only the first
    len(range(rank, len(dataset), world)) rows are scored (evaluate()'s rule)."""
    from VisionTransformer.metrics import DeviceMetrics
    was_training = model.training
    model.eval()
    pad_to = getattr(getattr(model, "vit_config", None), "batch_size", None)
    metrics = None                                    # made at the first batch: the logits name the class count
    rank, world = _rank_world()
    keep = None                                       # rows of this rank's shard that are samples, not sampler padding
    s = _sampler_of(test_loader)
    if world > 1 and isinstance(s, torch.utils.data.DistributedSampler) and not s.drop_last:
        keep = len(range(rank, len(s.dataset), world))
    seen = 0
    for tensors, labels in test_loader:
        rows = tensors.shape[0]
        if pad_to is not None and rows < pad_to:
            fill = tensors[-1:].expand(pad_to - rows, *tensors.shape[1:])
            tensors = torch.cat([tensors, fill], 0)
        logits = model(tensors.to(device, non_blocking=True))
        if metrics is None:
            metrics = DeviceMetrics(logits.shape[1], topk=topk, confusion=confusion, device=logits.device)
        score = rows if keep is None else max(0, min(rows, keep - seen))
        seen += rows
        if score:
            metrics.update(logits, labels.to(logits.device, non_blocking=True), rows=score)
    model.train(was_training)
    if metrics is None:                               # an empty shard still joins the all-reduce
        classes = getattr(getattr(model, "vit_config", None), "num_classes", None)
        if classes is None:
            raise ValueError("validate(): the test loader yielded no batch")
        metrics = DeviceMetrics(classes, topk=topk, confusion=confusion, device=device)
    if world > 1:
        metrics.all_reduce()
    return metrics.compute()


@torch.no_grad()
def rollout_maps(model, test_loader, images=None, head_fusion="mean", token=0):
    """Attention-rollout maps of the first `images` validation images (default: one batch) through
    model.attention_rollout: {"maps": [K, H / P, W / P] float32, "pred": [K] int64, "label": [K] int64} as numpy
    arrays.  Whole batches are run (a partial one padded as validate() pads it) and the result is cut to K; fewer when
    the loader holds fewer."""
    B = model.vit_config.batch_size
    K = B if images is None else int(images)
    if K <= 0:
        raise ValueError(f"rollout_maps: images must be positive, got {images}")
    maps, preds, labs, got = [], [], [], 0
    for tensors, labels in test_loader:
        if got >= K:
            break
        rows = tensors.shape[0]
        if rows < B:
            fill = tensors[-1:].expand(B - rows, *tensors.shape[1:])
            tensors = torch.cat([tensors, fill], 0)
        logits, m = model.attention_rollout(tensors.to(device, non_blocking=True), token, head_fusion)
        maps.append(model.patch_map(m, tensors.shape[2:])[:rows].float().cpu())
        preds.append(torch.argmax(logits[:rows], dim=-1).cpu())
        labs.append(labels.cpu().long())
        got += rows
    if not maps:
        raise ValueError("rollout_maps: the test loader yielded no batch")
    return {"maps": torch.cat(maps)[:K].numpy(), "pred": torch.cat(preds)[:K].numpy(),
            "label": torch.cat(labs)[:K].numpy()}


def _set_epoch(loader, epoch):
    """DistributedSampler.set_epoch on the loader's sampler (also behind data.DeviceBatches), so each epoch draws a
    new shard order on every rank."""
    for obj in (loader, getattr(loader, "loader", None)):
        if obj is None:
            continue
        for s in (getattr(obj, "sampler", None), getattr(getattr(obj, "batch_sampler", None), "sampler", None)):
            if isinstance(s, torch.utils.data.DistributedSampler):
                s.set_epoch(epoch)
                return True
    return False


def search_checkpoint(dir):
    """Highest N of the N.pt files in dir, or None (train.py:52-58)."""
    epochs = glob.glob(os.path.join(dir, "*.pt"))
    if len(epochs) == 0:
        return None
    names = [os.path.basename(e) for e in epochs]
    nums = [int(m.group(1)) for m in (re.match(r"(\d+)(?=\.pt)", nm) for nm in names) if m]
    return max(nums) if nums else None


class SyntheticImages(torch.utils.data.Dataset):
    """Deterministic N(0,1) images with uniform labels (the bench/parity input distribution)."""

    def __init__(self, n, channels, img, classes, seed):
        self.n, self.shape, self.classes, self.seed = n, (channels, img, img), classes, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        return torch.randn(self.shape, generator=g), int(torch.randint(0, self.classes, (1,), generator=g))


def replica_seed(rank, base=0):
    """CPU RNG seed of data-parallel replica `rank` after the identically seeded init (host path): rank 0 keeps
    `base`, so a one-rank job draws what a plain run draws."""
    return base if rank == 0 else (base + 0x9E3779B1 * rank) % (2 ** 63 - 1)


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _optimizer(model, lr, dev, opt="adamw", weight_decay=1e-4, no_decay_1d=False, layer_decay=None,
               fuse_groups=False, **kw):
    """make_optimizer over the model's parameters: one group as the reference has it, with `no_decay_1d`
    param_groups_weight_decay's two, or with `layer_decay` param_groups_layer_decay's (timm's: `no_decay_1d`'s split
    inside every layer), stepped in one launch."""
    if layer_decay is not None:
        params = param_groups_layer_decay(model, weight_decay, layer_decay)
        fuse_groups = True
    else:
        params = param_groups_weight_decay(model, weight_decay) if no_decay_1d else model.parameters()
    if fuse_groups:
        kw["fuse_groups"] = True
    return make_optimizer(params, lr=lr, weight_decay=weight_decay, device=dev, opt=opt, **kw)


def _schedule(optimizer, sched, layer_decay, total_steps, warmup_steps, warmup_lr, min_lr):
    """The LRSchedule the flags ask for, or None: `sched` names it, and layer decay without one takes a constant
    schedule, through which param_groups_layer_decay's `lr_scale` reaches `group["lr"]`."""
    if sched is None and layer_decay is None:
        if warmup_steps or warmup_lr or min_lr:
            raise ValueError("warmup_steps, warmup_lr and min_lr belong to a schedule (sched='constant' or 'cosine')")
        return None
    return LRSchedule(optimizer, sched or "constant", total_steps, warmup_steps, warmup_lr, min_lr)


def _check_teacher(teacher, configs, distill, distill_alpha, distill_tau):
    """The conditions of a distillation run, before anything is built: the loss's arguments, and a frozen eval-mode
    teacher that scores the student's classes on the student's batch."""
    if teacher is None:
        return
    from VisionTransformer._ops import check_distill_args
    check_distill_args(distill, distill_alpha, distill_tau)
    tc = teacher.vit_config
    for field in ("num_classes", "batch_size"):
        if getattr(tc, field) != getattr(configs, field):
            raise ValueError(f"the teacher's {field} ({getattr(tc, field)}) differs from the student's "
                             f"({getattr(configs, field)})")
    if teacher.training or any(p.requires_grad for p in teacher.parameters()):
        raise ValueError("the teacher must be frozen and in eval mode (vit.load_teacher)")


def train(configs, train_loader, test_loader, epochs, eval_iter, log_dir, checkpoint_dir, lr=1e-4,
          log_every=1, max_steps=None, reference_loop=False, max_grad_norm=None, ema_decay=None,
          label_smoothing=0.0, mix=None, opt="adamw", weight_decay=1e-4, no_decay_1d=False, always_adapt=False,
          trust_clip=False, sched=None, warmup_steps=0, warmup_lr=0.0, min_lr=0.0, layer_decay=None,
          fuse_groups=False, val_topk=None, val_confusion=False, teacher=None, distill="soft", distill_alpha=0.5,
          distill_tau=1.0):
    """The reference training loop (train.py:60-119) on the HIP path.  Returns the last epoch's summed loss.

    Defaults keep the GPU busy: no host sync inside the epoch — the epoch loss is summed on the device and the per-step
    "Loss/train_batch" scalars (every `log_every` steps, train.py:98) stay on the device until the epoch ends, when they
    are written in one transfer; validation runs every `eval_iter` epochs and a resumed run continues its step counter.
    `reference_loop=True` restores the reference's bookkeeping exactly: validation after every epoch (its eval_iter
    gate is commented out, train.py:114), `iteration` restarting at 0 on resume (train.py:67; the checkpoint's `step`
    is not read back) and the epoch loss as the host sum of each step's loss.item() (train.py:97-99: one host sync
    per step).  Under data parallelism a DistributedSampler gets `set_epoch(epoch)` every epoch and `evaluate`
    all-reduces its counts.

    `max_grad_norm` (not in the reference, whose loop has no clipping, train.py:94-96): clip by global gradient norm
    inside the optimizer step (optim.make_optimizer).  "GradNorm/train_batch" — the norm before clipping — is then
    logged at the loss's cadence and, like it, stays on the device until the epoch ends (`reference_loop`: per step,
    with its sync); rank 0 prints how many steps the epoch skipped for a non-finite norm.

    `ema_decay` (not in the reference either): the optimizer keeps an exponential moving average of the weights inside
    its step (optim.make_optimizer), validation scores the EMA weights (swapped in for `evaluate` and out again), and
    the checkpoint dict gains one key, "ema_state_dict" — the model's state_dict with the EMA in place of every trained
    parameter.  Resuming needs nothing more: the EMA is part of "optimizer_state_dict".

    `label_smoothing` and `mix` (not in the reference, whose loss is the plain cross entropy of the hard labels,
    train.py:81): the training loss is cross_entropy(..., label_smoothing=), and `mix` (a data.BatchMix) mixes every
    batch after it reached the device — mixup / CutMix, labels as MixedLabels — unless the loader already yielded
    MixedLabels (data.DeviceBatches(mix=...) stages the mix one batch ahead).  The logged "Loss/train_batch", the epoch
    loss and the checkpoint's "loss" are then the smoothed / mixed loss, not the hard-label cross entropy.  evaluate()
    and validation see unmixed data and hard labels.  Under data parallelism nothing more is needed: the mix is
    per-rank input work before the forward, and BatchMix seeds itself per rank.

    `opt`, `weight_decay`, `no_decay_1d`, `always_adapt`, `trust_clip` (not in the reference, which trains with
    AdamW(weight_decay=1e-4) over one group, train.py:66): `opt="lamb"` steps with LAMB (optim.FusedLamb; Lamb on the
    host path), `no_decay_1d` puts biases, norm weights and the two embeddings into a `weight_decay = 0` group
    (optim.param_groups_weight_decay), and the two flags are LAMB's.  The checkpoint dict is the same either way.

    `sched`, `warmup_steps`, `warmup_lr`, `min_lr` (not in the reference, which trains at one constant rate): an
    optim.LRSchedule ("constant" or "cosine", linear warmup first) over `lr`, stepped after every optimizer step;
    its length is the number of optimizer steps the run takes, (epochs + 1) epochs of min(len(train_loader),
    max_steps) steps.  "LR/train_batch", the rate each step was taken at (the first group's, before its `lr_scale`;
    a host value, no sync), is logged at the loss's cadence, and the checkpoint dict gains one key, "lr_schedule",
    restored on resume.  `layer_decay`: optim.param_groups_layer_decay's groups, stepped in one launch (`fuse_groups`),
    under a constant schedule unless one is named.  `fuse_groups` alone steps whatever groups there are in one launch.
    With none of these the optimizer, its groups, its launches and the checkpoint dict are the reference's.

    `val_topk`, `val_confusion` (not in the reference, whose validation is one accuracy): with a tuple of k the
    epoch's validation is validate() instead of evaluate() — on the EMA weights when there are any — with no host read
    until its end.  "val?acc" is then its top-1, rounded as before, "Loss/val" and "Acc{k}/val" are logged and printed
    beside it, and the checkpoint dict gains one key, "val_metrics": validate()'s dict, the confusion matrix as nested
    lists.  k = 1 is always among the k.  None (the default) is the loop, the tags and the checkpoint dict above.

    `teacher`, `distill`, `distill_alpha`, `distill_tau` (not in the reference): knowledge distillation.  `teacher` is
    a frozen model (vit.load_teacher) on the run's device with the student's class count and batch size; every step
    runs it under no_grad on the batch the student sees — after mixup / CutMix, as DeiT does; in eval mode, so on every
    patch even under patch dropout — and the loss is optim.distillation_loss(logits, labels, teacher logits,
    kind=distill, alpha=distill_alpha, tau=distill_tau, label_smoothing=label_smoothing).  The logged
    "Loss/train_batch", the epoch loss and the checkpoint's "loss" are that combined loss.  The teacher is in no
    optimizer, EMA, gradient bucket or checkpoint, and validation scores the student.  None (the default) is the loop,
    its launches, its tags and the checkpoint dict above."""
    _check_teacher(teacher, configs, distill, distill_alpha, distill_tau)
    rank, world = _rank_world()
    saved_epoch = search_checkpoint(checkpoint_dir)
    torch.manual_seed(0)                              # identical init on every rank
    model = vit.VisionTransformer(configs)
    opt_kw = dict(opt=opt, weight_decay=weight_decay, no_decay_1d=no_decay_1d, always_adapt=always_adapt,
                  trust_clip=trust_clip, max_grad_norm=max_grad_norm, ema_decay=ema_decay, layer_decay=layer_decay,
                  fuse_groups=fuse_groups)
    optimizer = _optimizer(model, lr, device, **opt_kw)
    total_steps = 0
    if sched is not None or layer_decay is not None:      # the optimizer steps of a run from scratch: epochs 0 .. `epochs`
        total_steps = (epochs + 1) * (min(len(train_loader), max_steps) if max_steps else len(train_loader))
    sched_args = (sched, layer_decay, total_steps, warmup_steps, warmup_lr, min_lr)
    schedule = _schedule(optimizer, *sched_args)
    iteration = 0
    if saved_epoch is not None:
        print(f"Checkpoint Found. Loading model from epoch {saved_epoch}")
        ckpt = torch.load(os.path.join(checkpoint_dir, f"{saved_epoch}.pt"), map_location="cpu", weights_only=True)
        model.load_state_dict(ckpt["model_state_dict"])
        model = model.to(device)
        optimizer = _optimizer(model, lr, device, **opt_kw)
        optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        schedule = _schedule(optimizer, *sched_args)
        if schedule is not None and "lr_schedule" in ckpt:
            schedule.load_state_dict(ckpt["lr_schedule"])
        iteration = 0 if reference_loop else int(ckpt.get("step", 0))
    else:
        saved_epoch = 0
        model = model.to(device)
    net = model
    if world > 1:
        if device == "cpu":      # host path: standard autograd, so torch's own DDP (gloo) applies
            net = torch.nn.parallel.DistributedDataParallel(model)
            # the host dropout (F.dropout, transformer.py:47,59) draws from the CPU RNG, seeded identically above
            # for identical init: give each replica its own stream, or all ranks mask their images alike
            torch.manual_seed(replica_seed(rank))
        else:
            model.enable_data_parallel()      # the engine folds the rank into its dropout seed
    writer = _writer(log_dir) if rank == 0 else None
    running_loss = 0.0
    clip = max_grad_norm is not None
    skipped_before = 0
    for epoch in range(saved_epoch, epochs + 1):
        _set_epoch(train_loader, epoch)
        loss_sum = torch.zeros((), device=device)
        host_loss = 0.0
        logged = []                                   # (iteration, device loss) written at the epoch's end
        logged_norm = []                              # (iteration, device gradient norm), likewise
        t0 = time.time()
        nb = 0
        for tensors, labels in train_loader:
            tensors = tensors.to(device, non_blocking=True)
            if not isinstance(labels, MixedLabels):   # else the loader mixed already (data.DeviceBatches(mix=))
                labels = labels.to(device, non_blocking=True)
                if mix is not None:
                    tensors, labels = mix(tensors, labels)
            if teacher is None:
                logits = net(tensors)
                loss = cross_entropy(logits, labels, label_smoothing)
            else:
                with torch.no_grad():
                    teacher_logits = teacher(tensors)
                loss = distillation_loss(net(tensors), labels, teacher_logits, kind=distill, alpha=distill_alpha,
                                         tau=distill_tau, label_smoothing=label_smoothing)
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            optimizer.step()
            if schedule is not None:
                if writer is not None and (reference_loop or (log_every and iteration % log_every == 0)):
                    writer.add_scalar("LR/train_batch", schedule.last_lr(), iteration)
                schedule.step()
            if reference_loop:
                host_loss += loss.item()
                if writer is not None:
                    writer.add_scalar("Loss/train_batch", loss.item(), iteration)
                    if clip:
                        writer.add_scalar("GradNorm/train_batch", optimizer.grad_norm().item(), iteration)
            else:
                loss_sum += loss.detach()
                if writer is not None and log_every and iteration % log_every == 0:
                    logged.append((iteration, loss.detach()))
                    if clip:
                        logged_norm.append((iteration, optimizer.grad_norm()))
            iteration += 1
            nb += 1
            if max_steps and nb >= max_steps:
                break
        if logged:
            for (it, _), v in zip(logged, torch.stack([v for _, v in logged]).tolist()):
                writer.add_scalar("Loss/train_batch", v, it)
        if logged_norm:
            for (it, _), v in zip(logged_norm, torch.stack([v for _, v in logged_norm]).tolist()):
                writer.add_scalar("GradNorm/train_batch", v, it)
        running_loss = host_loss if reference_loop else float(loss_sum.item())
        dt = time.time() - t0
        acc = None
        val = None
        if test_loader is not None and (reference_loop or (eval_iter and epoch % eval_iter == 0)):
            with optimizer.ema_weights() if ema_decay is not None else contextlib.nullcontext():
                if val_topk is None:
                    from sklearn.metrics import accuracy_score
                    acc = round(float(evaluate(model, test_loader, accuracy_score)), 2)
                else:
                    val = validate(model, test_loader, topk=(1, *val_topk), confusion=val_confusion)
                    acc = round(float(val["top1"]), 2)
            if writer is not None:
                writer.add_scalar("val?acc", acc, epoch)
                if val is not None:
                    writer.add_scalar("Loss/val", val["loss"], epoch)
                    for k in sorted({1, *val_topk}):
                        writer.add_scalar(f"Acc{k}/val", val[f"top{k}"], epoch)
        if rank == 0:
            os.makedirs(checkpoint_dir, exist_ok=True)
            ckpt = {"epoch": epoch, "model_state_dict": model.state_dict(),
                    "optimizer_state_dict": optimizer.state_dict(), "loss": running_loss, "step": iteration}
            if ema_decay is not None:
                ckpt["ema_state_dict"] = optimizer.ema_state_dict(model)
            if schedule is not None:
                ckpt["lr_schedule"] = schedule.state_dict()
            if val is not None:
                from VisionTransformer.metrics import jsonable
                ckpt["val_metrics"] = jsonable(val)
            torch.save(ckpt, os.path.join(checkpoint_dir, f"{epoch}.pt"))
            ips = nb * configs.batch_size * world / max(dt, 1e-9)
            print(f"Epoch {epoch}, curr loss: {running_loss:.4f}, mean_accuracy: {acc}, "
                  f"{nb} steps in {dt:.2f}s ({ips:.1f} img/s over {world} GPU(s))", flush=True)
            if val is not None:
                accs = ", ".join(f"top{k}: {val[f'top{k}']:.4f}" for k in sorted({1, *val_topk}))
                print(f"Epoch {epoch}, val loss: {val['loss']:.4f}, {accs} over {val['n']} samples", flush=True)
            if clip:
                skipped = int(optimizer.skipped_steps().item())
                print(f"Epoch {epoch}, steps skipped for a non-finite gradient norm: {skipped - skipped_before}",
                      flush=True)
                skipped_before = skipped
    return running_loss


def eval_only(configs, test_loader, checkpoint_dir, topk=(1, 5), confusion=True, ema=False, rollout=None):
    """validate() once on the newest checkpoint of `checkpoint_dir` (its "ema_state_dict" with `ema`): the compute()
    dict with the checkpoint's epoch as "epoch".  Raises FileNotFoundError when the directory holds no checkpoint.
    `rollout`: a dict of rollout_maps() keywords plus "out"; rank 0 then writes that function's arrays to the .npz
    file `out` after the validation pass."""
    saved_epoch = search_checkpoint(checkpoint_dir)
    if saved_epoch is None:
        raise FileNotFoundError(f"no checkpoint (N.pt) in {checkpoint_dir!r} to evaluate")
    ckpt = torch.load(os.path.join(checkpoint_dir, f"{saved_epoch}.pt"), map_location="cpu", weights_only=True)
    key = "ema_state_dict" if ema else "model_state_dict"
    if key not in ckpt:
        raise KeyError(f"checkpoint {saved_epoch}.pt has no {key!r} (it was trained without a weight EMA)")
    torch.manual_seed(0)
    model = vit.VisionTransformer(configs)
    model.load_state_dict(ckpt[key])
    model = model.to(device)
    result = validate(model, test_loader, topk=topk, confusion=confusion)
    result["epoch"] = saved_epoch
    if rollout is not None and _rank_world()[0] == 0:
        import numpy as np
        kw = dict(rollout)
        np.savez(kw.pop("out"), **rollout_maps(model, test_loader, **kw))
    return result


def time_steps(configs, steps, warmup, lr=1e-4, dev=None, seed=1234, max_grad_norm=None, ema_decay=None,
               label_smoothing=0.0, mix=None, opt="adamw", weight_decay=1e-4, no_decay_1d=False, always_adapt=False,
               trust_clip=False, layer_decay=None, fuse_groups=False, teacher=None, distill="soft", distill_alpha=0.5,
               distill_tau=1.0):
    """The hot loop body (train.py:91-98: forward, CE loss, zero_grad(set_to_none), backward, AdamW step) on one
    synthetic batch already resident on `dev`, dropout on; returns (seconds per timed step, last loss).  This is the
    repo's own CPU training step that bench.py's `cpu_baseline` times (BASELINE config 1).  Unclipped unless
    `max_grad_norm` is given, and without a weight EMA unless `ema_decay` is.  With `mix` (a data.BatchMix) every step
    first mixes the resident batch, and `label_smoothing` goes to the loss, as in train().  `opt`, `weight_decay`,
    `no_decay_1d`, `always_adapt`, `trust_clip`, `layer_decay` and `fuse_groups` choose the optimizer as in train()
    (with `layer_decay` under a constant schedule, applied once: the rates do not move while timing).  `teacher`,
    `distill`, `distill_alpha` and `distill_tau` are train()'s: the step then runs the teacher's forward under no_grad
    and optim.distillation_loss."""
    _check_teacher(teacher, configs, distill, distill_alpha, distill_tau)
    dev = torch.device(dev or device)
    torch.manual_seed(0)
    model = vit.VisionTransformer(configs).to(dev).train()
    opt = _optimizer(model, lr, dev, opt=opt, weight_decay=weight_decay, no_decay_1d=no_decay_1d,
                     always_adapt=always_adapt, trust_clip=trust_clip, max_grad_norm=max_grad_norm, ema_decay=ema_decay,
                     layer_decay=layer_decay, fuse_groups=fuse_groups)
    _schedule(opt, None, layer_decay, 0, 0, 0.0, 0.0)
    g = torch.Generator().manual_seed(seed)
    n_img = int(round((configs.num_patches ** 0.5) * configs.patch_size))
    x = torch.randn(configs.batch_size, configs.input_channels, n_img, n_img, generator=g).to(dev)
    y = torch.randint(0, configs.num_classes, (configs.batch_size,), generator=g).to(dev)
    loss = None
    t0 = time.perf_counter()
    for i in range(warmup + steps):
        if i == warmup:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        xb, yb = (x, y) if mix is None else mix(x, y)
        if teacher is None:
            loss = cross_entropy(model(xb), yb, label_smoothing)
        else:
            with torch.no_grad():
                teacher_logits = teacher(xb)
            loss = distillation_loss(model(xb), yb, teacher_logits, kind=distill, alpha=distill_alpha, tau=distill_tau,
                                     label_smoothing=label_smoothing)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    last = float(loss.item())
    return (time.perf_counter() - t0) / max(steps, 1), last


def main():
    ap = argparse.ArgumentParser(description="ViT training on MI355X (drop-in for the reference src/train.py)")
    ap.add_argument("--model", default="tiny", choices=sorted(config.PRESETS))
    ap.add_argument("--img", type=int, default=64)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8, help="per-GPU batch (CLS parameter is batch-shaped)")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="max steps per epoch")
    ap.add_argument("--train-size", type=int, default=512)
    ap.add_argument("--test-size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--eval-iter", type=int, default=1)
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="FLOAT",
                    help="clip gradients to this global L2 norm inside the optimizer step and log GradNorm/train_batch "
                         "(default: no clipping, as the reference)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="FLOAT",
                    help="keep an exponential moving average of the weights with this decay inside the optimizer "
                         "step, validate on it and save it as ema_state_dict (default: none, as the reference)")
    ap.add_argument("--opt", default="adamw", choices=["adamw", "lamb"],
                    help="optimizer: AdamW as the reference, or LAMB (per-tensor trust ratios, for large batches)")
    ap.add_argument("--weight-decay", type=float, default=1e-4, metavar="F",
                    help="decoupled weight decay (default 1e-4, the reference's)")
    ap.add_argument("--no-decay-1d", action="store_true",
                    help="no weight decay on biases, norm weights and the cls / position embeddings (timm's rule; "
                         "default: every parameter decays, as the reference)")
    ap.add_argument("--lamb-always-adapt", action="store_true",
                    help="LAMB: apply the trust ratio to tensors without weight decay too")
    ap.add_argument("--lamb-trust-clip", action="store_true", help="LAMB: bound every trust ratio by 1")
    ap.add_argument("--sched", default=None, choices=["constant", "cosine"],
                    help="per-step learning-rate schedule over --lr, after a linear warmup (default: none, one "
                         "constant rate as the reference)")
    ap.add_argument("--warmup-steps", type=int, default=0, metavar="N", help="with --sched: optimizer steps of warmup")
    ap.add_argument("--warmup-lr", type=float, default=0.0, metavar="F", help="with --sched: the rate the warmup starts at")
    ap.add_argument("--min-lr", type=float, default=0.0, metavar="F", help="with --sched cosine: the rate it ends at")
    ap.add_argument("--layer-decay", type=float, default=None, metavar="F",
                    help="layer-wise learning-rate decay: the head at --lr, every layer below at F times the rate of "
                         "the one above (timm's rule; turns --fuse-groups on; default: none)")
    ap.add_argument("--fuse-groups", action="store_true",
                    help="step every param group in one launch instead of one launch per group")
    ap.add_argument("--patch-drop", type=float, default=0.0, metavar="RATE",
                    help="patch dropout: each training image keeps max(1, int(N * (1 - RATE))) of its N patch tokens "
                         "(patch 0 and a random subset) plus CLS, and the blocks run on those alone (timm's "
                         "patch_drop_rate; default 0: off, as the reference); evaluation uses every token")
    ap.add_argument("--drop-path", type=float, default=0.0, metavar="RATE",
                    help="stochastic depth: drop each residual branch per image, block l of L at rate RATE * l / (L - 1) "
                         "(timm's linear rule; DeiT-B trains with 0.1; default 0: off, as the reference)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="F",
                    help="label smoothing of the training loss (default 0: the reference's plain cross entropy)")
    ap.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA",
                    help="mixup with lambda ~ Beta(ALPHA, ALPHA) on the training batches (default 0: off)")
    ap.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA",
                    help="CutMix with lambda ~ Beta(ALPHA, ALPHA) on the training batches (default 0: off)")
    ap.add_argument("--mix-prob", type=float, default=1.0, metavar="P",
                    help="probability that a batch is mixed at all (with --mixup / --cutmix)")
    ap.add_argument("--mix-switch-prob", type=float, default=0.5, metavar="P",
                    help="probability of CutMix when both --mixup and --cutmix are on")
    ap.add_argument("--random-resized-crop", action="store_true",
                    help="train on a random crop of --crop-scale of the area and --crop-ratio aspect, resized to --img "
                         "(torchvision's RandomResizedCrop; inside the resize launch on cuda; default: off)")
    ap.add_argument("--crop-scale", type=float, nargs=2, default=(0.08, 1.0), metavar=("LO", "HI"))
    ap.add_argument("--crop-ratio", type=float, nargs=2, default=(3 / 4, 4 / 3), metavar=("LO", "HI"))
    ap.add_argument("--hflip", type=float, default=0.0, metavar="P",
                    help="probability of a horizontal flip of a training image (default 0: off)")
    ap.add_argument("--random-erase", type=float, default=0.0, metavar="P",
                    help="probability of erasing a random box of a training image with 0 after the normalize (timm's "
                         "RandomErasing, mode const; default 0: off)")
    ap.add_argument("--rand-augment", default=None, metavar="STR",
                    help="RandAugment between the flip and ToTensor, as timm's --aa string, e.g. rand-m9-mstd0.5-inc1 "
                         "(keys m, n, mstd, inc, p); needs --random-resized-crop, --hflip or --random-erase, whose "
                         "transform it runs in; training images only (default: off)")
    ap.add_argument("--mean", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="with --std: normalize training and test images per channel, (x - mean) / std")
    ap.add_argument("--std", type=float, nargs=3, default=None, metavar=("R", "G", "B"))
    ap.add_argument("--val-topk", type=int, nargs="+", default=None, metavar="K",
                    help="validate on the device: loss, top-K accuracies (top-1 always) and precision / recall, read "
                         "once per validation, logged as Loss/val and Acc{K}/val and saved as the checkpoint's "
                         "val_metrics (default: the reference's accuracy-only evaluate)")
    ap.add_argument("--val-confusion", action="store_true",
                    help="with --val-topk or --eval-only: also the confusion matrix and per-class precision / recall / f1")
    ap.add_argument("--eval-only", action="store_true",
                    help="load the newest checkpoint of --checkpoint-dir (its EMA weights with --ema-decay), validate "
                         "once, print the metrics as one JSON line and exit")
    ap.add_argument("--rollout-out", default=None, metavar="FILE.npz",
                    help="with --eval-only: after the validation pass write the attention-rollout maps of the first "
                         "validation images (maps [K, H/P, W/P] float32, pred [K], label [K]) to this .npz file")
    ap.add_argument("--rollout-images", type=int, default=None, metavar="K",
                    help="with --rollout-out: how many images (default: one batch)")
    ap.add_argument("--rollout-fusion", default="mean", choices=["mean", "max", "min"],
                    help="with --rollout-out: how the heads' attention is fused")
    ap.add_argument("--rollout-token", type=int, default=0, metavar="I",
                    help="with --rollout-out: the token whose rollout is taken (0: the one the classifier reads; the "
                         "CLS token is the last)")
    ap.add_argument("--teacher-checkpoint", default=None, metavar="PATH",
                    help="knowledge distillation: train against the logits of the frozen model in this checkpoint file "
                         "or directory (its newest N.pt), run under no_grad on every training batch (default: none)")
    ap.add_argument("--teacher-model", default=None, choices=sorted(config.PRESETS),
                    help="with --teacher-checkpoint: the teacher's preset (default: --model)")
    ap.add_argument("--teacher-dtype", default=None, choices=["fp32", "bf16"],
                    help="with --teacher-checkpoint: the teacher's compute dtype (default: --dtype)")
    ap.add_argument("--teacher-ema", action="store_true",
                    help="with --teacher-checkpoint: load the checkpoint's ema_state_dict")
    ap.add_argument("--distill", default=None, choices=["soft", "hard"],
                    help="with --teacher-checkpoint: soft (default) = tau^2 * KL(teacher || student) at temperature "
                         "--distill-tau, hard = cross entropy against the teacher's arg max")
    ap.add_argument("--distill-alpha", type=float, default=None, metavar="F",
                    help="with --teacher-checkpoint: loss = (1 - F) * cross entropy + F * distillation term (default 0.5)")
    ap.add_argument("--distill-tau", type=float, default=None, metavar="F",
                    help="with --teacher-checkpoint: temperature of the soft term (default 1)")
    ap.add_argument("--reference-loop", action="store_true",
                    help="the reference's loop bookkeeping exactly: validate every epoch, restart the step counter on "
                         "resume, host-summed loss (train.py:60-119)")
    ap.add_argument("--data", default="synthetic", choices=["synthetic", "synthetic-u8", "cifar10-bin", "folder"],
                    help="synthetic: N(0,1) float images at --img; the others decode uint8 images and apply the "
                         "reference transform (GPU kernel on cuda, Pillow on cpu)")
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--checkpoint-dir", default="../checkpoints")
    ap.add_argument("--log-dir", default="../logs")
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"],
                    help="auto = cuda when a ROCm GPU is present, else cpu (train.py:26)")
    ap.add_argument("--threads", type=int, default=0, help="host-path threads (0 = every core this process may use)")
    ap.add_argument("--bench", action="store_true",
                    help="time --steps steps (after --warmup) on one resident synthetic batch; print one JSON line")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    global device
    if args.device != "auto":
        device = args.device
    if device == "cpu":
        torch.set_num_threads(args.threads or len(os.sched_getaffinity(0)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        if device == "cuda":
            local = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    rank, world = _rank_world()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    n_patches = (args.img // args.patch) ** 2
    D, H, L = config.PRESETS[args.model]
    cfg = config.ViTConfig(input_channels=3, num_classes=args.classes, num_patches=n_patches, embedding_size=D,
                           patch_size=args.patch, num_heads=H, num_blocks=L, precision=dtype,
                           batch_size=args.batch, device="cpu", drop_path_rate=args.drop_path,
                           patch_drop_rate=args.patch_drop)
    mix = None
    if args.mixup > 0 or args.cutmix > 0:
        from VisionTransformer.data import BatchMix
        mix = BatchMix(args.mixup, args.cutmix, prob=args.mix_prob, switch_prob=args.mix_switch_prob)
    augmenting = args.random_resized_crop or args.hflip > 0 or args.random_erase > 0
    if (args.mean is None) != (args.std is None):
        ap.error("--mean and --std go together")
    if args.data == "synthetic" and (augmenting or args.mean is not None):
        ap.error("--random-resized-crop, --hflip, --random-erase, --mean and --std act in the image path, and "
                 "--data synthetic feeds float tensors and has none: use --data synthetic-u8, cifar10-bin or folder")
    augment = None
    if augmenting:
        from VisionTransformer.data import TrainAugment
        augment = TrainAugment(scale=tuple(args.crop_scale) if args.random_resized_crop else None,
                               ratio=tuple(args.crop_ratio), hflip=args.hflip, erase_prob=args.random_erase)
    rand_augment = None
    if args.rand_augment is not None:
        if not augmenting:
            ap.error("--rand-augment runs inside the augmenting transform: give --random-resized-crop, --hflip or "
                     "--random-erase with it")
        from VisionTransformer.data import RandAugment
        try:
            rand_augment = RandAugment.from_config(args.rand_augment)
        except ValueError as e:
            ap.error(str(e))
    # only a run with --rand-augment passes the keyword: every other run calls the transforms as it always did
    ra_kw = {} if rand_augment is None else {"rand_augment": rand_augment}
    if args.opt != "lamb" and (args.lamb_always_adapt or args.lamb_trust_clip):
        ap.error("--lamb-always-adapt and --lamb-trust-clip need --opt lamb")
    opt_args = dict(opt=args.opt, weight_decay=args.weight_decay, no_decay_1d=args.no_decay_1d,
                    always_adapt=args.lamb_always_adapt, trust_clip=args.lamb_trust_clip, layer_decay=args.layer_decay,
                    fuse_groups=args.fuse_groups)
    if args.sched is None and args.layer_decay is None and (args.warmup_steps or args.warmup_lr or args.min_lr):
        ap.error("--warmup-steps, --warmup-lr and --min-lr need --sched")
    if args.rollout_out is not None and not args.eval_only:
        ap.error("--rollout-out needs --eval-only")
    if args.rollout_out is None and (args.rollout_images is not None or args.rollout_fusion != "mean"
                                     or args.rollout_token != 0):
        ap.error("--rollout-images, --rollout-fusion and --rollout-token need --rollout-out")
    if args.rollout_images is not None and args.rollout_images <= 0:
        ap.error("--rollout-images must be positive")
    if not 0 <= args.rollout_token <= n_patches:
        ap.error(f"--rollout-token must lie in [0, {n_patches}]")
    teacher_flags = (args.teacher_model, args.teacher_dtype, args.distill, args.distill_alpha, args.distill_tau)
    if args.teacher_checkpoint is None and (args.teacher_ema or any(v is not None for v in teacher_flags)):
        ap.error("--teacher-model, --teacher-dtype, --teacher-ema, --distill, --distill-alpha and --distill-tau need "
                 "--teacher-checkpoint")
    distill_kw = {}
    if args.teacher_checkpoint is not None and not args.eval_only:
        from VisionTransformer._ops import check_distill_args
        distill_kw = dict(distill=args.distill or "soft",
                          distill_alpha=0.5 if args.distill_alpha is None else args.distill_alpha,
                          distill_tau=1.0 if args.distill_tau is None else args.distill_tau)
        try:
            check_distill_args(*distill_kw.values())
        except ValueError as e:
            ap.error(str(e))
        tD, tH, tL = config.PRESETS[args.teacher_model or args.model]
        tdtype = dtype if args.teacher_dtype is None else \
            (torch.bfloat16 if args.teacher_dtype == "bf16" else torch.float32)
        tcfg = config.ViTConfig(input_channels=3, num_classes=args.classes, num_patches=n_patches, embedding_size=tD,
                                patch_size=args.patch, num_heads=tH, num_blocks=tL, precision=tdtype,
                                batch_size=args.batch, device="cpu")
        try:
            distill_kw["teacher"] = vit.load_teacher(tcfg, args.teacher_checkpoint, student=cfg, ema=args.teacher_ema,
                                                     device=device)
        except (FileNotFoundError, KeyError, ValueError) as e:
            ap.exit(2, f"train.py --teacher-checkpoint: {e}\n")
    if args.bench:
        steps = args.steps or 30
        sec, last = time_steps(cfg, steps, args.warmup, lr=args.lr, max_grad_norm=args.clip_grad_norm,
                               ema_decay=args.ema_decay, label_smoothing=args.label_smoothing, mix=mix, **opt_args,
                               **distill_kw)
        print(json.dumps({"device": device, "model": args.model, "img": args.img, "batch": args.batch,
                          "dtype": args.dtype, "threads": torch.get_num_threads(), "warmup": args.warmup,
                          "steps": steps, "ms_per_step": round(sec * 1e3, 3),
                          "images_per_s": round(args.batch / sec, 3), "final_loss": round(last, 5)}), flush=True)
        return
    pin = device == "cuda"
    if args.data == "synthetic":
        train_set = SyntheticImages(args.train_size, 3, args.img, args.classes, seed=1 + rank)
        test_set = SyntheticImages(args.test_size, 3, args.img, args.classes, seed=10_000)
    else:
        from VisionTransformer import data as D
        if args.data == "cifar10-bin":
            train_set, test_set = D.CIFAR10Bin(args.data_root, True), D.CIFAR10Bin(args.data_root, False)
        elif args.data == "folder":
            train_set = D.BrainTumorDataset(args.data_root, train=True, transform=D.decode)
            test_set = D.BrainTumorDataset(args.data_root, train=False, transform=D.decode)
        else:
            train_set = D.SyntheticRawImages(args.train_size, (32, 32, 3), args.classes, seed=1 + rank)
            test_set = D.SyntheticRawImages(args.test_size, (32, 32, 3), args.classes, seed=10_000)
    sampler = torch.utils.data.DistributedSampler(train_set) if world > 1 else None
    # the test set is sharded too (each sample on exactly one rank); evaluate() gathers the predictions
    tsampler = ShardSampler(test_set) if world > 1 else None
    if args.data != "synthetic" and device == "cuda":
        from VisionTransformer import data as D
        # one transform (and coefficient workspace) per loader: each stages its batches on its own side stream
        # the augmentation is part of the resize launch, staged before the mix: erase precedes mixup, as in timm
        train_tf = D.GpuTrainTransform(args.img, augment, mean=args.mean, std=args.std, **ra_kw) if augment is not None \
            else D.GpuImageTransform(args.img, mean=args.mean, std=args.std)
        train_loader = D.DeviceBatches(D.raw_loader(train_set, args.batch, shuffle=True, num_workers=args.workers,
                                                    sampler=sampler), train_tf, device, mix=mix)
        test_loader = D.DeviceBatches(D.raw_loader(test_set, args.batch, shuffle=False, num_workers=args.workers,
                                                   drop_last=False, sampler=tsampler),
                                      D.GpuImageTransform(args.img, mean=args.mean, std=args.std), device)
    else:
        if args.data != "synthetic":
            from VisionTransformer import data as D
            plain = D.host_transform(args.img, mean=args.mean, std=args.std)
            train_tf = D.host_train_transform(args.img, augment, args.mean, args.std, **ra_kw) if augment is not None \
                else plain
            train_set, test_set = D.Transformed(train_set, train_tf), D.Transformed(test_set, plain)
        train_loader = torch.utils.data.DataLoader(train_set, batch_size=args.batch, shuffle=sampler is None,
                                                   sampler=sampler, num_workers=args.workers, drop_last=True,
                                                   pin_memory=pin)
        # a partial last test batch is padded by evaluate() (the CLS parameter is batch-shaped)
        test_loader = torch.utils.data.DataLoader(test_set, batch_size=args.batch, num_workers=args.workers,
                                                  sampler=tsampler, drop_last=False, pin_memory=pin)
    if args.eval_only:
        from VisionTransformer.metrics import jsonable
        try:
            result = eval_only(cfg, test_loader, args.checkpoint_dir, topk=tuple({1, *(args.val_topk or ())}),
                               confusion=args.val_confusion, ema=args.ema_decay is not None,
                               rollout=None if args.rollout_out is None else dict(
                                   out=args.rollout_out, images=args.rollout_images,
                                   head_fusion=args.rollout_fusion, token=args.rollout_token))
        except (FileNotFoundError, KeyError) as e:
            ap.exit(2, f"train.py --eval-only: {e}\n")
        if rank == 0:
            print(json.dumps(jsonable(result)), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    train(cfg, train_loader, test_loader, args.epochs, args.eval_iter, args.log_dir, args.checkpoint_dir,
          lr=args.lr, max_steps=args.steps, reference_loop=args.reference_loop, max_grad_norm=args.clip_grad_norm,
          ema_decay=args.ema_decay, label_smoothing=args.label_smoothing, mix=mix, sched=args.sched,
          warmup_steps=args.warmup_steps, warmup_lr=args.warmup_lr, min_lr=args.min_lr,
          val_topk=tuple(args.val_topk) if args.val_topk else None, val_confusion=args.val_confusion, **opt_args,
          **distill_kw)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
