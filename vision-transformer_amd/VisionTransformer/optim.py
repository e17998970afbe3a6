"""Fused optimizer and loss for the training step (train.py:66,81,93,96).

FusedAdamW: torch.optim.AdamW semantics (decoupled weight decay, bias-corrected moments, amsgrad off) in ONE
multi-tensor HIP launch over every parameter; the same kernel refreshes the compute-dtype shadow weights the fused
engine reads (bf16 copies of the fp32 masters), so no separate cast pass runs per step.  The optimizer state keys
('step', 'exp_avg', 'exp_avg_sq') are those of torch.optim.AdamW, so `optimizer.state_dict()` checkpoints are
interchangeable with the reference's (train.py:73,110).

CrossEntropyLoss: nn.CrossEntropyLoss() (mean) as one fused softmax + NLL + gradient kernel; with `label_smoothing`
and / or MixedLabels (mixup / CutMix) the same against a smoothed two-label target that is never materialised.
"""
import collections
import contextlib
import ctypes
import math
import struct
import typing

import torch
import torch.nn as nn

from . import _ops
from ._engine import shadow_of


def _check_hyper(name, lr, eps, betas):
    if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
        raise ValueError(f"invalid {name} hyper-parameters")


def _check_ema_decay(ema_decay):
    if ema_decay is not None and not (0 < ema_decay < 1):
        raise ValueError(f"ema_decay must be None or lie strictly between 0 and 1 (got {ema_decay!r})")


class _EmaSurface:
    """What FusedAdamW(ema_decay=...) and the host path's EmaAdamW share: the EMA lives in `state[p]["ema"]`, and
    `swap_ema()` (theirs) exchanges it with the weights."""

    _ema_swapped = False

    def _refuse_step_while_swapped(self):
        if self._ema_swapped:
            raise RuntimeError("step() while the EMA weights are swapped in: leave ema_weights() (or call swap_ema() "
                               "again) first, or the update would train the average and average the raw weights")

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the block on the EMA weights: swap them in, and swap the trained weights back in a `finally`."""
        if self._ema_swapped:
            raise RuntimeError("ema_weights(): the EMA weights are already swapped in (no nesting)")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self, model):
        """`model.state_dict()` with every parameter that has an EMA replaced by a clone of it (read without a swap;
        while the EMA weights are swapped in, the parameters themselves hold those values)."""
        out = model.state_dict()
        for name, p in model.named_parameters():
            e = self.state[p].get("ema") if p in self.state else None
            if e is not None and name in out:
                out[name] = (p if self._ema_swapped else e).detach().clone()
        return out


def _closure_loss(closure):
    if closure is None:
        return None
    with torch.enable_grad():
        return closure()


class _StepTable:
    """One cached launch of the fused step: the device chunk table over the parameters `params` (and, where any of
    them has an EMA, the EMA pointer array cut alike), with what valid() compares to tell that it still describes
    them.  `keep` holds every tensor whose pointer the device table carries.  `sizes` is None here and the merged
    table's own (_GroupedTable).  `lamb` is FusedLamb's: the tensor index of the table and the buffers its three
    launches pass along (_LambIndex), made at the table's first LAMB step and None for ever under plain AdamW.  A table
    built in the place of `old` over the very same parameters (new gradient tensors, a new EMA) inherits it: same
    tensors, same cut, and the ratios of the last step stay readable through a skipped one."""

    __slots__ = ("version", "params", "grads", "grad_ptrs", "param_ptrs", "moments", "emas", "dev_tab", "ema_dev",
                 "nchunks", "shadow_dtype", "device", "keep", "lamb", "sizes")

    @classmethod
    def build(cls, opt, ps, old=None):
        state, tab = opt.state, cls()
        shadows = [shadow_of(p) for p in ps]
        # one shadow dtype per table, the first there is: the kernel writes no shadow of another
        tab.shadow_dtype = sdt = next((s.dtype for s in shadows if s is not None), torch.float32)
        tab.version, tab.params, tab.device = opt._version, list(ps), ps[0].device
        tab.grads = [p.grad for p in ps]
        tab.moments = [(state[p]["exp_avg"], state[p]["exp_avg_sq"]) for p in ps]
        tab.keep = [(p, g, m, v, s if (s is not None and s.dtype == sdt) else None)
                    for p, g, (m, v), s in zip(ps, tab.grads, tab.moments, shadows)]
        if not all(t.is_contiguous() for _, g, m, v, _ in tab.keep for t in (g, m, v)):
            raise RuntimeError("FusedAdamW: non-contiguous grad/state")
        tab.dev_tab, tab.nchunks = _ops.build_chunk_table(tab.keep, tab.device)
        tab.emas, tab.ema_dev = [state[p].get("ema") for p in ps], None
        if all(e is None for e in tab.emas):
            tab.emas = None
        else:
            tab.ema_dev, _ = _ops.build_ema_pointers(list(zip(ps, tab.emas)), tab.device)
        tab.param_ptrs, tab.grad_ptrs = [p.data_ptr() for p in ps], [g.data_ptr() for g in tab.grads]
        tab.sizes = tab.lamb = None
        if (old is not None and old.lamb is not None and old.lamb.chunk == _ops.CHUNK and tab.device == old.device
                and len(old.params) == len(ps) and all(a is b for a, b in zip(old.params, ps))):
            tab.lamb = old.lamb
        return tab

    def lamb_index(self):
        if self.lamb is None:
            first, owner, ntensors, nchunks = _ops.build_tensor_index(self.keep, self.device)
            if nchunks != self.nchunks:
                raise RuntimeError("FusedLamb: the tensor index disagrees with the chunk table")
            self.lamb = _LambIndex(first, owner, ntensors,
                                   torch.zeros(2 * nchunks, dtype=torch.float64, device=self.device),
                                   torch.ones(ntensors, dtype=torch.float32, device=self.device), _ops.CHUNK)
        return self.lamb

    def valid(self, opt, ps, sizes=None):
        """Same optimizer version, same parameters (for the merged table each group bringing as many as `sizes` says;
        no sizes for any other), every parameter still holds the same .grad tensor object and the same moment tensor
        objects as when the table was built, and no parameter's or gradient's storage moved (`p.data = ...` re-points
        storage without changing any object identity).  Two data_ptr() per parameter plus
        identity checks: this runs every step.  The engine's shadows change only when it rebuilds its buffers, and
        then every gradient view is a new object too.  A table built with EMA pointers also wants every parameter's
        `state[p]["ema"]` to be the tensor object it points at; one built without serves only the EMA-less step."""
        if self.version != opt._version or len(self.params) != len(ps) or self.sizes != sizes:
            return False
        state = opt.state
        if self.emas is None:      # a table without EMA pointers serves only the EMA-less step (no per-parameter work)
            if opt.ema_decay is not None:
                return False
        elif any(state[a].get("ema") is not e for a, e in zip(self.params, self.emas)):
            return False
        for a, b, g, ptr, (m, v), gp in zip(self.params, ps, self.grads, self.param_ptrs, self.moments,
                                            self.grad_ptrs):
            # the gradient's storage too: `p.grad.data = t` / `p.grad.set_(...)` keep the .grad object
            if a is not b or a.grad is not g or a.data_ptr() != ptr or g.data_ptr() != gp:
                return False
            st = state[a]
            if st["exp_avg"] is not m or st["exp_avg_sq"] is not v:
                return False
        return True


class _GroupedTable(_StepTable):
    """The merged table of a `fuse_groups` step: the stepping parameters of every group, each group's consecutive, in
    one chunk table, with the device maps chunk -> group and tensor -> group beside it (indices modulo
    _lib.OPT_MAX_GROUPS) and `spans`, one _Span per launch of at most that many groups.  `sizes` is how many
    parameters each group brought, which valid() compares too.  No hyper-parameter is part of it.  The chunks come in
    the order the per-group tables list them, so a norm pass over this table leaves the partials, and with them the
    norm's bits, of one over those."""

    __slots__ = ("group_of_chunk", "group_of_tensor", "spans")

    @classmethod
    def build_grouped(cls, opt, ps, sizes, old=None):
        tab = cls.build(opt, ps, old)
        tab.sizes = list(sizes)
        tab.group_of_chunk, tab.group_of_tensor, bounds = _ops.build_group_index(tab.keep, sizes, tab.device)
        if bounds[-1][1] != tab.nchunks:
            raise RuntimeError("FusedAdamW: the group index disagrees with the chunk table")
        cap, size = _ops._lib.OPT_MAX_GROUPS, ctypes.sizeof(_ops._lib.TensorChunk)
        tab.spans = []
        for g0 in range(0, len(sizes), cap):
            g1 = min(g0 + cap, len(sizes))
            (t0, c0), (t1, c1) = bounds[g0], bounds[g1]
            if c1 > c0:
                tab.spans.append(_Span(g0, g1, c0, c1, t0, t1, tab.dev_tab[c0 * size:c1 * size],
                                       tab.group_of_chunk[c0:c1],
                                       tab.ema_dev[c0:c1] if tab.ema_dev is not None else None))
        return tab

    @staticmethod
    def fusable(ps):
        """One device and one shadow dtype over `ps`: what one launch can serve."""
        if len({p.device for p in ps}) != 1:
            return False
        return len({s.dtype for s in map(shadow_of, ps) if s is not None}) <= 1


# groups [g0, g1) of a merged table: its chunks [c0, c1) and tensors [t0, t1), and the slices of the chunk table, of
# group_of_chunk and of the EMA pointers (None without) that one launch over them takes
_Span = collections.namedtuple("_Span", "g0 g1 c0 c1 t0 t1 rows group_of_chunk ema_dev")
# tensor_first int32 [ntensors + 1], tensor_of_chunk int32 [nchunks], the fp64 [2 * nchunks] norm partials, the fp32
# [ntensors] trust ratios (ones until a step writes them): all on the table's device, sized once; `chunk` is the
# _ops.CHUNK they were cut with
_LambIndex = collections.namedtuple("_LambIndex", "tensor_first tensor_of_chunk ntensors partial trust chunk")
_SwapKey = collections.namedtuple("_SwapKey", "param ptr ema shadow")      # what a parameter's swap entry was cut from
_SwapTable = collections.namedtuple("_SwapTable", "dev_tab ema_dev nchunks shadow_dtype keep")


class _SwapTables:
    """swap_ema()'s launches: every parameter that has an EMA exactly once, one table per (device, shadow dtype), in
    practice one.  Valid while the optimizer's version and every parameter's storage, EMA tensor object and shadow
    object are those it was built from."""

    __slots__ = ("version", "keys", "tables")

    def __init__(self, opt, ps):
        self.version = opt._version
        self.keys = [_SwapKey(p, p.data_ptr(), opt.state[p]["ema"], shadow_of(p)) for p in ps]
        groups = {}
        for k in self.keys:
            groups.setdefault((k.param.device, k.shadow.dtype if k.shadow is not None else None), []).append(k)
        for dev in {d for d, _ in groups}:      # shadow-less parameters ride in their device's first table
            bare = groups.pop((dev, None), None)
            if bare:
                key = next(((d, s) for d, s in groups if d == dev), (dev, torch.float32))
                groups.setdefault(key, []).extend(bare)
        self.tables = []
        for (dev, sdt), keys in groups.items():
            dev_tab, n = _ops.build_chunk_table([(k.param.detach(), None, None, None, k.shadow) for k in keys], dev)
            ema_dev, _ = _ops.build_ema_pointers([(k.param, k.ema) for k in keys], dev)
            self.tables.append(_SwapTable(dev_tab, ema_dev, n, sdt, keys))

    def valid(self, opt, ps):
        return self.version == opt._version and len(self.keys) == len(ps) and all(
            k.param is p and p.data_ptr() == k.ptr and opt.state[p]["ema"] is k.ema and shadow_of(p) is k.shadow
            for k, p in zip(self.keys, ps))


class FusedAdamW(_EmaSurface, torch.optim.Optimizer):
    """Step bookkeeping stays on the host: each group's per-parameter 'step' entries are 0-d views of ONE CPU
    tensor (torch AdamW's state format, so `state_dict()` / `load_state_dict()` interchange with it), advanced by a
    single in-place add per step, with a host-side mirror of the counts for the bias corrections — no per-parameter
    `.item()` or `+= 1` on the step path.  Device chunk tables (_StepTable) are cached per (group, step count) and hold
    references to every tensor whose pointer they carry.  A cached table is reused while the optimizer's version
    (bumped by load_state_dict / add_param_group / fresh state) is unchanged and every parameter still has the very
    same .grad tensor object, the same moment tensor objects and every parameter the storage it was tabled with, so
    `p.data = other` or a replaced moment tensor rebuilds the table by itself (one data_ptr() per parameter per step,
    no per-step pointer signature of gradients and moments).

    Gradient clipping (`max_grad_norm`, off by default; the reference has none, train.py:94-96).  With a positive
    `max_grad_norm` the step clips by the global L2 norm of grad_scale * grad over every parameter with a gradient
    in every param group, as `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` followed by the plain step
    would, without a pass that rewrites the gradients and without a host sync: a norm kernel over the same chunk
    tables, a one-workgroup finish that leaves (norm, coef, skip, skipped total) in device memory, and the AdamW
    kernel reading coef and skip from there.  `max_grad_norm` is an attribute like `grad_scale`, not a
    `param_groups` key, so `state_dict()` stays interchangeable with torch AdamW.  `grad_norm()` and
    `skipped_steps()` return device copies of the last step's norm and the count of skipped steps.
    `skip_nonfinite` (default on): a step whose norm is inf or NaN changes no parameter, moment or shadow; off, the
    non-finite coefficient reaches the update as it would in torch.  Deviation: the host never learns of a skip, so
    the `step` counters advance on a skipped step too, and the bias corrections of later steps are those of step
    t + 1.  With `ema_decay` the EMA does not move on a skipped step either.

    Weight EMA (`ema_decay`, off by default; the reference has none).  With 0 < ema_decay < 1 the same launch keeps an
    exponential moving average of every stepped parameter in `state[p]["ema"]` (fp32, contiguous): created with the
    moments as a clone of the weights before the first update, then ema += (1 - ema_decay) * (p_new - ema) after each
    (timm's ModelEmaV2 order), read and written by the AdamW kernel while p_new is in a register.  A parameter that
    has moments but no "ema" (a loaded torch AdamW checkpoint) gets one cloned from its value at the next step.
    `ema_decay` is an attribute, not a `param_groups` key, and may be changed between steps; torch AdamW's
    load_state_dict carries the extra state key along and its step() ignores it.  `swap_ema()` exchanges weights and
    EMA in place, shadows included, so the fused engine evaluates the EMA with no repack and no rebuild;
    `ema_weights()` is the context manager around it (step() raises inside), and `ema_state_dict(model)` reads the
    EMA out without swapping.  Data parallel needs nothing more: every rank holds bitwise the same gradients after
    the all-reduce, hence the same weights and the same EMA.

    `fuse_groups` (off by default; an attribute, not a `param_groups` key).  step() launches once per param group,
    which is one launch for the reference's single group and 28 for a ViT-B under layer-wise learning-rate decay
    (param_groups_layer_decay).  With `fuse_groups` every group goes in ONE launch (one per 64 groups): a merged chunk
    table under the key ("groups", "all"), each chunk naming its group, and the groups' hyper-parameters, read from
    `param_groups` at every step, passed to the kernel by value (include/vit_hip.h "Grouped optimizer steps"), so a
    scheduler that rewrites `group["lr"]` every step rebuilds nothing and copies nothing.  Bit for bit the per-group
    step.  A step in which some group holds parameters at different step counts (a parameter whose first gradient
    came late), or whose parameters span devices or shadow dtypes, runs per group as with `fuse_groups` off.

    One step path: _plan() yields each group's stepping parameters by step count, _run_per_group() or _run_grouped()
    launches them (the second falls back on the first), _norm_pass() is the clipped step's norm over whichever tables
    there are, and _group_spec() is the one reader of a group's hyper-parameters.  A subclass changes the update by
    overriding _group_spec(), _adamw() and _grouped_launch() (FusedLamb)."""

    # its kernel writes the engines' compute-dtype shadows along with the masters: no repack follows a step
    # (_engine._after_optimizer_step marks them stale after every other optimizer's)
    refreshes_shadows = True
    fuse_groups = False       # the instance's keyword; here for an optimizer unpickled from before it existed

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
                 max_grad_norm=None, skip_nonfinite=True, ema_decay=None, fuse_groups=False):
        _check_hyper("AdamW", lr, eps, betas)
        _check_max_grad_norm(max_grad_norm)
        _check_ema_decay(ema_decay)
        self._version = 0
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale
        self.fuse_groups = fuse_groups
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self.ema_decay = ema_decay
        self._swap_tables = None  # swap_ema()'s own tables: every parameter with an EMA exactly once
        self._tables = {}
        self._steps = {}          # group index -> (params list, steps tensor [n] f32 CPU, host list of ints)
        self._partial = None      # f64 [chunks of every table]: the norm pass's per-chunk sums
        self._clip = None         # f32 [4] device: norm, coef, skip, skipped total (vit_grad_clip_finish)

    def invalidate(self):
        """Drop every cached chunk table, the norm pass's partial buffer and the step mirror (parameters re-pointed
        outside any engine).  The 4-float clip state stays: it points at nothing, and it carries the skipped-step
        count."""
        self._version += 1
        self._tables = {}
        self._steps = {}
        self._partial = None
        self._swap_tables = None

    # ---- gradient clipping --------------------------------------------------------------------------------------
    def _clip_state(self, device=None):
        if device is None:
            device = next(p.device for g in self.param_groups for p in g["params"])
        if self._clip is None or self._clip.device != device:
            self._clip = torch.zeros(4, dtype=torch.float32, device=device)
        return self._clip

    def grad_norm(self):
        """The last clipped step's global gradient norm (before clipping): a fresh 0-d device tensor, copied on the
        current stream, so a caller can keep one per step and read them all later without a sync in between."""
        return self._clip_state()[0].clone()

    def skipped_steps(self):
        """How many steps were skipped for a non-finite norm so far: a fresh 0-d device tensor, as grad_norm()."""
        return self._clip_state()[3].clone()

    def _norm_pass(self, tabs):
        """The clip block of a step over `tabs` (the per-group tables, or the one merged table): grad_sumsq per table
        into consecutive slices of one partial buffer, sized here, and one finish — on the current stream, which the
        engine's backward() has already made wait for the weight-gradient stream and the all-reduce handles."""
        _check_max_grad_norm(self.max_grad_norm)
        device = tabs[0].device
        if any(tab.device != device for tab in tabs):
            raise RuntimeError("FusedAdamW: a global gradient norm needs every parameter on one device")
        total = sum(tab.nchunks for tab in tabs)
        if self._partial is None or self._partial.device != device or self._partial.numel() < total:
            self._partial = torch.empty(total, dtype=torch.float64, device=device)
        clip = self._clip_state(device)
        off = 0
        for tab in tabs:
            _ops.grad_sumsq(tab.dev_tab, tab.nchunks, self.grad_scale, self._partial[off:off + tab.nchunks])
            off += tab.nchunks
        _ops.grad_clip_finish(self._partial, total, self.max_grad_norm, clip, self.skip_nonfinite)
        return clip

    # ---- launches -----------------------------------------------------------------------------------------------
    def _group_spec(self, group, t):
        """A group's vit_opt_group at step count `t`: (lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2,
        flags).  The one reader of a group's hyper-parameters: the per-group and the grouped launches take them from
        here, read from `param_groups` at every step."""
        b1, b2 = group["betas"]
        return (group["lr"], b1, b2, group["eps"], group["weight_decay"], 1.0 - b1 ** t, 1.0 - b2 ** t, 0)

    def _adamw(self, tab, spec, clip=None):
        """The update of one table's parameters, all of the group and at the step count of `spec`."""
        lr, b1, b2, eps, wd, bc1, bc2, _ = spec
        if self.ema_decay is not None:
            _ops.adamw_ema(tab.dev_tab, tab.ema_dev, tab.nchunks, lr, b1, b2, eps, wd, bc1, bc2, self.grad_scale,
                           tab.shadow_dtype, self.ema_decay, clip=clip)
            return
        _ops.adamw(tab.dev_tab, tab.nchunks, lr, b1, b2, eps, wd, bc1, bc2, self.grad_scale, tab.shadow_dtype,
                   clip=clip)

    def _grouped_launch(self, tab, specs, span, clip):
        """The update of one span of the merged table, whose groups are those of `specs`."""
        ema = self.ema_decay is not None
        _ops.adamw_groups(span.rows, span.group_of_chunk, span.c1 - span.c0, specs, self.grad_scale, tab.shadow_dtype,
                          ema_dev=span.ema_dev if ema else None, ema_decay=self.ema_decay if ema else None, clip=clip)

    # ---- step counters ------------------------------------------------------------------------------------------
    def _step_state(self, gi, group):
        ent = self._steps.get(gi)
        ps = group["params"]
        if ent is not None and len(ent[0]) == len(ps) and all(a is b for a, b in zip(ent[0], ps)):
            return ent[1], ent[2]
        host = [int(float(self.state[p]["step"])) if "step" in self.state[p] else 0 for p in ps]
        buf = torch.tensor(host, dtype=torch.float32)
        for i, p in enumerate(ps):
            if "step" in self.state[p]:
                self.state[p]["step"] = buf[i]
        self._steps[gi] = (list(ps), buf, host)
        return buf, host

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.invalidate()         # the moments are new tensors: every cached chunk table is stale

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):
            self.invalidate()

    def _make_state(self, plist, ema):
        """Moments, and with `ema` an EMA, for every parameter of `plist` that has none yet.  True if any was made."""
        fresh = False
        for p in plist:
            if not p.is_cuda or p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise RuntimeError("FusedAdamW: parameters and grads must be float32 on a ROCm device")
            if p.grad.is_sparse:
                raise RuntimeError("FusedAdamW does not support sparse gradients")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                fresh = True
            if ema and "ema" not in st:      # with the moments, or at the first step after a torch checkpoint
                st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
                fresh = True
        return fresh

    def _advance(self, gi, group, idx):
        """One in-place add on the shared tensor, the host mirror in Python ints.  Returns {step count: [params]}."""
        ps_all = group["params"]
        buf, host = self._step_state(gi, group)
        if len(idx) == len(ps_all):
            buf += 1
        else:
            buf[torch.tensor(idx)] += 1
        by_step = {}
        for i in idx:
            host[i] += 1
            by_step.setdefault(host[i], []).append(ps_all[i])
        return by_step

    def _table(self, key, ps, sizes=None):
        """The cached table under `key` while it still describes `ps` (_StepTable.valid), else a new one in its place.
        With `sizes` (how many of `ps` each group brings) the merged table of a grouped step, or None, and nothing
        built, where one launch cannot serve `ps`."""
        old = self._tables.get(key)
        if old is not None and old.valid(self, ps, sizes):
            return old
        if sizes is None:
            tab = _StepTable.build(self, ps, old)
        elif _GroupedTable.fusable(ps):
            tab = _GroupedTable.build_grouped(self, ps, sizes, old)
        else:
            return None
        self._tables[key] = tab
        return tab

    def _plan(self):
        """(gi, group, {step count: [params]}) for every group with stepping parameters, in order, its state made and
        its counters advanced.  A generator: the unclipped per-group step launches group k before group k + 1 is
        prepared, so the device works under the host's bookkeeping on a path that is host-bound with 28 groups."""
        ema = self.ema_decay is not None
        for gi, group in enumerate(self.param_groups):
            ps_all = group["params"]
            idx = [i for i, p in enumerate(ps_all) if p.grad is not None]
            if not idx:
                continue
            if self._make_state([ps_all[i] for i in idx], ema):
                self.invalidate()
            yield gi, group, self._advance(gi, group, idx)

    def _run_per_group(self, plan):
        """One launch (set) per group and step count.  A clipped step's norm spans every table: it launches once they
        all exist."""
        clipped, work = self.max_grad_norm is not None, []
        for gi, group, by_step in plan:
            for t, ps in by_step.items():
                # one table for the whole group while every parameter has the same step count, else one per count
                tab = self._table((gi, "all") if len(by_step) == 1 else (gi, "t", t), ps)
                if clipped:
                    work.append((tab, group, t))
                else:
                    self._adamw(tab, self._group_spec(group, t))
        if work:
            clip = self._norm_pass([tab for tab, _, _ in work])
            for tab, group, t in work:
                self._adamw(tab, self._group_spec(group, t), clip)

    def _run_grouped(self, plan):
        """Every group of `plan` in one grouped launch per _lib.OPT_MAX_GROUPS groups, over one merged table (cached
        under ("groups", "all")).  False, and nothing launched, where that cannot be: some group's stepping parameters
        are at different step counts, or the parameters span devices or shadow dtypes."""
        if not plan or any(len(by_step) != 1 for _, _, by_step in plan):
            return False
        stepping = [next(iter(by_step.values())) for _, _, by_step in plan]
        tab = self._table(("groups", "all"), [p for ps in stepping for p in ps], [len(ps) for ps in stepping])
        if tab is None:
            return False
        clip = self._norm_pass([tab]) if self.max_grad_norm is not None else None
        specs = [self._group_spec(group, next(iter(by_step))) for _, group, by_step in plan]
        for span in tab.spans:
            self._grouped_launch(tab, specs[span.g0:span.g1], span, clip)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        self._refuse_step_while_swapped()
        _check_ema_decay(self.ema_decay)
        plan = self._plan()
        if self.fuse_groups:      # the whole plan first; a step it cannot serve goes per group, as with fuse_groups off
            plan = list(plan)
            if self._run_grouped(plan):
                return loss
        self._run_per_group(plan)
        return loss

    # ---- weight EMA ---------------------------------------------------------------------------------------------
    def _ema_params(self):
        state = self.state       # .get: looking must not create an (empty) state entry for a parameter that has none
        return [p for g in self.param_groups for p in g["params"] if (state.get(p) or {}).get("ema") is not None]

    def _ema_swap_tables(self):
        """Chunk tables for vit_ema_swap, of their own whichever step tables exist: those carry gradient pointers, go
        stale with zero_grad(set_to_none=True), and two of them may hold the same parameter."""
        ps = self._ema_params()
        cached = self._swap_tables
        if cached is None or not cached.valid(self, ps):
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps):
                raise RuntimeError("FusedAdamW: parameters must be contiguous float32 on a ROCm device")
            cached = self._swap_tables = _SwapTables(self, ps)
        return cached.tables

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter that has an EMA with it, in place, and refresh its compute-dtype shadow from the
        new value: one launch per table, no repack, no engine rebuild (the engine reads the same buffers).  A second
        call restores every bit.  Parameters without an EMA are left alone."""
        for tab in self._ema_swap_tables():
            _ops.ema_swap(tab.dev_tab, tab.ema_dev, tab.nchunks, tab.shadow_dtype)
        self._ema_swapped = not self._ema_swapped


_LAMB_GROUP_KEYS = ("always_adapt", "trust_clip")
_ADAPT, _TRUST_CLIP = _ops._lib.OPT_ADAPT, _ops._lib.OPT_TRUST_CLIP      # a spec's flag bits (vit_opt_group.flags)


def _as_f32(x):
    """The value a Python float takes as a `float` argument of the library."""
    return struct.unpack("f", struct.pack("f", x))[0]


def _check_lamb_flags(group):
    for k in _LAMB_GROUP_KEYS:
        if not isinstance(group[k], bool):
            raise ValueError(f"{k} must be a bool (got {group[k]!r})")


def _lamb_flags(always_adapt, trust_clip):
    """The two LAMB keys of `param_groups` as a constructor's defaults, checked."""
    flags = dict(always_adapt=always_adapt, trust_clip=trust_clip)
    _check_lamb_flags(flags)
    return flags


class _LambGroups:
    """What FusedLamb and the host path's Lamb share of the two LAMB keys: a loaded group that lacks them (a torch
    AdamW / FusedAdamW checkpoint has neither) keeps this optimizer's current values."""

    def load_state_dict(self, state_dict):
        mine = [{k: g[k] for k in _LAMB_GROUP_KEYS} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, kept in zip(self.param_groups, mine):
            for k, v in kept.items():
                group.setdefault(k, v)


class FusedLamb(_LambGroups, FusedAdamW):
    """LAMB (timm's Lamb / NVIDIA's FusedLAMB, bias correction on; the reference has none) over FusedAdamW's tables,
    counters, clipping, EMA and swap: only the per-table launch differs.  For a tensor w of a group at step count t

        g = grad * grad_scale * coef          m = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g^2
        u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + weight_decay * w
        r = |w| / |u| where both norms are positive, else 1      (r = 1 if weight_decay == 0 and not always_adapt)
        r = min(r, 1) with trust_clip                             w -= lr * r * u

    in three launches per table (include/vit_hip.h "LAMB"): the moments and per-chunk fp64 norm partials, one workgroup
    per tensor turning them into a ratio, and the update, which forms u again instead of reading it back.  Every group
    goes through them, a `weight_decay == 0` group too: its ratios are written as 1 by the second launch, so there is
    one set of kernels and one set of bits to test.  `always_adapt` and `trust_clip` are `param_groups`
    keys, per group and serialised with it; the state keys are FusedAdamW's, so checkpoints interchange with it and
    with torch.optim.AdamW (a loaded group that lacks the two keys keeps this optimizer's current values).  On a step
    skipped for a non-finite norm none of the three launches writes anything.  `trust_ratios()` reads the last step's
    ratios without a sync."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False,
                 trust_clip=False, grad_scale=1.0, max_grad_norm=None, skip_nonfinite=True, ema_decay=None,
                 fuse_groups=False):
        flags = _lamb_flags(always_adapt, trust_clip)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay,
                         fuse_groups=fuse_groups)
        self.defaults.update(flags)
        for group in self.param_groups:
            for k, v in flags.items():
                group.setdefault(k, v)
        self._stepped = []        # the tables of the last step, for trust_ratios()

    @torch.no_grad()
    def step(self, closure=None):
        self._stepped = []        # (not in invalidate(): a later group's fresh state invalidates in mid-step)
        return super().step(closure)

    def _group_spec(self, group, t):
        """FusedAdamW's with the betas as the kernels receive them, rounded to fp32, and the group's flags."""
        _check_lamb_flags(group)
        # The recurrence runs with 1 - fl32(b2), which is 1.3e-5 (relative) away from 1 - 0.999, so bias corrections
        # formed from the unrounded betas would leave sqrt(v_hat), u and with it every ratio off by 6e-6 in the first
        # steps.  From the rounded ones the step is exactly LAMB with betas 1e-8 away from the group's.
        b1, b2 = group["betas"]
        b1, b2, wd = _as_f32(b1), _as_f32(b2), group["weight_decay"]
        flags = (_ADAPT if wd != 0 or group["always_adapt"] else 0) | (_TRUST_CLIP if group["trust_clip"] else 0)
        return (group["lr"], b1, b2, group["eps"], wd, 1.0 - b1 ** t, 1.0 - b2 ** t, flags)

    def _adamw(self, tab, spec, clip=None):
        """The three LAMB launches over one table's parameters, all of the group and at the step count of `spec`."""
        lr, b1, b2, eps, wd, bc1, bc2, flags = spec
        ix = tab.lamb_index()
        ema = self.ema_decay is not None
        _ops.lamb_moments(tab.dev_tab, tab.nchunks, b1, b2, eps, wd, bc1, bc2, self.grad_scale, ix.partial, clip=clip)
        _ops.lamb_trust(ix.partial, ix.tensor_first, ix.ntensors, ix.trust, adapt=flags & _ADAPT,      # truth values
                        trust_clip=flags & _TRUST_CLIP, clip=clip)
        _ops.lamb_update(tab.dev_tab, ix.tensor_of_chunk, ix.trust, tab.nchunks, lr, eps, wd, bc1, bc2,
                         tab.shadow_dtype, ema_dev=tab.ema_dev if ema else None,
                         ema_decay=self.ema_decay if ema else None, clip=clip)
        self._stepped.append(tab)

    def _grouped_launch(self, tab, specs, span, clip):
        """The three LAMB launches over one span of the merged table.  The partials, the tensor index and the ratios
        are the whole table's: the slices keep their absolute indices."""
        c0, c1, t0, t1, rows, of_chunk = span.c0, span.c1, span.t0, span.t1, span.rows, span.group_of_chunk
        ix = tab.lamb_index()
        ema = self.ema_decay is not None
        _ops.lamb_moments_groups(rows, of_chunk, c1 - c0, specs, self.grad_scale, ix.partial[2 * c0:2 * c1], clip=clip)
        _ops.lamb_trust_groups(ix.partial, ix.tensor_first[t0:t1 + 1], tab.group_of_tensor[t0:t1], t1 - t0, specs,
                               ix.trust[t0:t1], clip=clip)
        _ops.lamb_update_groups(rows, ix.tensor_of_chunk[c0:c1], ix.trust, of_chunk, c1 - c0, specs, tab.shadow_dtype,
                                ema_dev=span.ema_dev if ema else None,
                                ema_decay=self.ema_decay if ema else None, clip=clip)
        if not self._stepped or self._stepped[-1] is not tab:
            self._stepped.append(tab)

    def trust_ratios(self):
        """{parameter: its trust ratio r in the last step}, for every parameter that step updated: fresh 0-d device
        tensors (views of one copy per table, made on the current stream), so a caller can keep them and read them
        later without a sync in between, as with grad_norm().  1 where the rule says 1."""
        out = {}
        for tab in self._stepped:
            r = tab.lamb.trust.clone()
            out.update((p, r[i]) for i, p in enumerate(tab.params))
        return out


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, dlogits = _ops.softmax_xent(logits.contiguous().float(), labels.contiguous().long())
        ctx.save_for_backward(dlogits)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


class MixedLabels(typing.NamedTuple):
    """The labels of a mixed batch (data.BatchMix): row i's target is lam[i] * onehot(a[i]) + (1 - lam[i]) *
    onehot(b[i]).  `a`, `b` int64 [rows], `lam` float32 [rows], all on the logits' device."""
    a: torch.Tensor
    b: torch.Tensor
    lam: torch.Tensor


def dense_target(labels, classes, label_smoothing=0.0, dtype=torch.float32):
    """The [rows, classes] target that cross_entropy's kernel never builds: (1 - eps) * (lam * onehot(a) + (1 - lam) *
    onehot(b)) + eps / classes for MixedLabels, the smoothed one-hot for a label tensor.  The host path and the tests
    use it."""
    if isinstance(labels, MixedLabels):
        a, b, lam = labels.a.long(), labels.b.long(), labels.lam.to(dtype)
    else:
        a = b = labels.long()
        lam = torch.ones(a.shape[0], dtype=dtype, device=a.device)
    t = torch.zeros(a.shape[0], classes, dtype=dtype, device=a.device)
    t.scatter_add_(1, a[:, None], lam[:, None])
    t.scatter_add_(1, b[:, None], (1 - lam)[:, None])
    return t * (1.0 - label_smoothing) + label_smoothing / classes


class _XentMixedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, a, b, lam, smoothing):
        loss, dlogits = _ops.softmax_xent_mixed(logits.contiguous().float(), a, b, lam, smoothing)
        ctx.save_for_backward(dlogits)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None, None


def _check_label_smoothing(label_smoothing):
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1) (got {label_smoothing!r})")


def cross_entropy(logits, labels, label_smoothing=0.0):
    """mean softmax cross-entropy (nn.CrossEntropyLoss() default) — fused HIP kernel, gradient precomputed; host
    tensors (the CPU path) use torch's own.

    `label_smoothing` (torch's keyword) and `labels` given as MixedLabels (mixup / CutMix, data.BatchMix) are not in
    the reference (train.py:81).  A label tensor with label_smoothing == 0 runs vit_softmax_xent exactly as before;
    anything else runs vit_softmax_xent_mixed, which forms the smoothed two-label target on the fly.  On the host:
    F.cross_entropy(..., label_smoothing=), on the dense two-hot target for MixedLabels."""
    _check_label_smoothing(label_smoothing)
    mixed = isinstance(labels, MixedLabels)
    if not logits.is_cuda:
        if mixed:
            return nn.functional.cross_entropy(logits, dense_target(labels, logits.shape[-1], dtype=logits.dtype),
                                               label_smoothing=label_smoothing)
        if label_smoothing == 0.0:
            return nn.functional.cross_entropy(logits, labels)
        return nn.functional.cross_entropy(logits, labels, label_smoothing=label_smoothing)
    if not mixed:
        if label_smoothing == 0.0:
            return _XentFn.apply(logits, labels)
        return _XentMixedFn.apply(logits, labels.contiguous().long(), None, None, float(label_smoothing))
    return _XentMixedFn.apply(logits, labels.a.contiguous().long(), labels.b.contiguous().long(),
                              labels.lam.contiguous().float(), float(label_smoothing))


class _DistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, teacher_logits, a, b, lam, smoothing, kind, alpha, tau):
        loss, dlogits = _ops.softmax_xent_distill(logits.contiguous().float(), teacher_logits, a, b, lam, smoothing,
                                                  kind, alpha, tau)
        ctx.save_for_backward(dlogits)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * g,) + (None,) * 8


def lowest_argmax(z):
    """[rows] int64: the lowest index at which each row of `z` attains its maximum (torch.argmax leaves the choice
    among ties open)."""
    C = z.shape[-1]
    idx = torch.arange(C, device=z.device).expand_as(z)
    return torch.where(z == z.max(dim=-1, keepdim=True).values, idx, C).min(dim=-1).values


def distillation_loss(logits, labels, teacher_logits, *, kind="soft", alpha=0.5, tau=1.0, label_smoothing=0.0):
    """(1 - alpha) * cross_entropy(logits, labels, label_smoothing) + alpha * d, the loss of a student trained against
    the logits of a frozen teacher (Hinton et al. 2015; DeiT, Touvron et al. 2021) — one fused HIP kernel
    (vit_softmax_xent_distill), gradient precomputed; not in the reference.

    kind "soft": d = tau^2 * KL(softmax(teacher / tau) || softmax(logits / tau)), summed over the classes and averaged
    over the rows: F.kl_div(log_softmax(logits / tau), log_softmax(teacher / tau), reduction="batchmean",
    log_target=True) * tau^2.  DeiT's script divides the sum by rows * classes instead; scale `alpha` for its weighting.
    kind "hard": d = cross_entropy(logits, yhat), yhat the lowest index of each teacher row's maximum; `tau` is unused.
    `labels`: a label tensor or MixedLabels, as cross_entropy takes them.  `teacher_logits` is detached whatever the
    caller passes: no gradient reaches the teacher.  Host tensors run the same formula in torch ops."""
    _ops.check_distill_args(kind, alpha, tau)
    _check_label_smoothing(label_smoothing)
    if teacher_logits.shape != logits.shape:
        raise ValueError(f"teacher_logits must have the logits' shape {tuple(logits.shape)} "
                         f"(got {tuple(teacher_logits.shape)})")
    z = teacher_logits.detach()
    mixed = isinstance(labels, MixedLabels)
    if not logits.is_cuda:
        F = nn.functional
        z = z.to(logits.dtype)
        base = F.cross_entropy(logits, dense_target(labels, logits.shape[-1], label_smoothing, dtype=logits.dtype))
        if kind == "soft":
            d = F.kl_div(F.log_softmax(logits / tau, dim=-1), F.log_softmax(z / tau, dim=-1), reduction="batchmean",
                         log_target=True) * tau ** 2
        else:
            d = F.cross_entropy(logits, lowest_argmax(z))
        return (1.0 - alpha) * base + alpha * d
    z = z.contiguous().float()
    if mixed:
        a, b, lam = labels.a.contiguous().long(), labels.b.contiguous().long(), labels.lam.contiguous().float()
    else:
        a, b, lam = labels.contiguous().long(), None, None
    return _DistillFn.apply(logits, z, a, b, lam, float(label_smoothing), kind, float(alpha), float(tau))


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is not None and not (0 < max_grad_norm < math.inf):
        raise ValueError(f"max_grad_norm must be None or a positive finite number (got {max_grad_norm!r})")


class _HostClip:
    """What the host path's ClippedAdamW and EmaAdamW share: clip_grad_norm_ before the step, the skip of a step
    whose norm is not finite, and the norm and skip count that grad_norm() / skipped_steps() report."""

    def _init_clip(self, max_grad_norm, skip_nonfinite):
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self._norm = torch.zeros(())
        self._skipped = 0

    def _clip_grads(self, params):
        """Clip the gradients of `params` in place.  True when the step is to be skipped for a non-finite norm."""
        self._norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm).detach().clone()
        skip = self.skip_nonfinite and not bool(torch.isfinite(self._norm))
        self._skipped += skip
        return skip

    def grad_norm(self):
        return self._norm.clone()

    def skipped_steps(self):
        return torch.tensor(float(self._skipped))


class ClippedAdamW(_HostClip, torch.optim.AdamW):
    """The host path's counterpart of FusedAdamW(max_grad_norm=...): torch.optim.AdamW whose step() first runs
    torch.nn.utils.clip_grad_norm_ over every parameter with a gradient, and with `skip_nonfinite` leaves parameters
    and state alone when that norm is inf or NaN (the gradients are still scaled by the non-finite step's
    coefficient, as clip_grad_norm_ does; zero_grad() discards them).  `max_grad_norm` is an attribute, not a
    `param_groups` key: state_dict() is torch AdamW's."""

    def __init__(self, params, max_grad_norm, skip_nonfinite=True, **kwargs):
        _check_max_grad_norm(max_grad_norm)
        if max_grad_norm is None:
            raise ValueError("ClippedAdamW needs a max_grad_norm; use torch.optim.AdamW to train unclipped")
        super().__init__(params, **kwargs)
        self._init_clip(max_grad_norm, skip_nonfinite)

    def step(self, closure=None):
        loss = _closure_loss(closure)
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if params and not self._clip_grads(params):
            super().step()
        return loss


class EmaAdamW(_EmaSurface, _HostClip, torch.optim.AdamW):
    """The host path's counterpart of FusedAdamW(ema_decay=...), in torch ops: torch.optim.AdamW whose step() then
    moves `state[p]["ema"]` by ema += (1 - ema_decay) * (p_new - ema) for every parameter it stepped.  Same
    initialisation (a clone of the weights before the parameter's first update here), same surface (`ema_decay`
    attribute, swap_ema(), ema_weights(), ema_state_dict(model)).  With `max_grad_norm` it clips first as ClippedAdamW
    does, and a step skipped for a non-finite norm leaves the EMA alone too."""

    def __init__(self, params, ema_decay, max_grad_norm=None, skip_nonfinite=True, **kwargs):
        _check_ema_decay(ema_decay)
        _check_max_grad_norm(max_grad_norm)
        if ema_decay is None:
            raise ValueError("EmaAdamW needs an ema_decay; use torch.optim.AdamW or ClippedAdamW to train without")
        super().__init__(params, **kwargs)
        self.ema_decay = ema_decay
        self._init_clip(max_grad_norm, skip_nonfinite)

    def step(self, closure=None):
        loss = _closure_loss(closure)
        self._refuse_step_while_swapped()
        _check_ema_decay(self.ema_decay)
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not params or (self.max_grad_norm is not None and self._clip_grads(params)):
            return loss
        # torch's step() creates its state only where there is none at all, so a new EMA joins the state after it
        new = [(p, p.detach().clone(memory_format=torch.contiguous_format)) for p in params
               if "ema" not in self.state.get(p, ())]
        super().step()
        for p, e in new:
            self.state[p]["ema"] = e
        w = 1.0 - float(self.ema_decay)
        with torch.no_grad():
            for p in params:
                e = self.state[p]["ema"]
                e.add_(p.detach() - e, alpha=w)
        return loss

    @torch.no_grad()
    def swap_ema(self):
        for g in self.param_groups:
            for p in g["params"]:
                e = self.state[p].get("ema") if p in self.state else None
                if e is not None:
                    old = p.detach().clone()
                    p.copy_(e)
                    e.copy_(old)
        self._ema_swapped = not self._ema_swapped


class Lamb(_LambGroups, _EmaSurface, _HostClip, torch.optim.Optimizer):
    """The host path's counterpart of FusedLamb, in torch ops on whatever device and dtype the parameters have: the
    same formulas (FusedLamb's docstring), defaults, `param_groups` keys and state keys, `max_grad_norm` /
    `skip_nonfinite` as ClippedAdamW has them, `ema_decay` and the swap surface as EmaAdamW, and trust_ratios().  As
    on the host path's AdamW classes a skipped step does not advance the `step` counters."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False,
                 trust_clip=False, max_grad_norm=None, skip_nonfinite=True, ema_decay=None):
        _check_hyper("LAMB", lr, eps, betas)
        flags = _lamb_flags(always_adapt, trust_clip)
        _check_max_grad_norm(max_grad_norm)
        _check_ema_decay(ema_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **flags))
        self.ema_decay = ema_decay
        self._init_clip(max_grad_norm, skip_nonfinite)
        self._ratios = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        self._refuse_step_while_swapped()
        _check_ema_decay(self.ema_decay)
        _check_max_grad_norm(self.max_grad_norm)
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not params or (self.max_grad_norm is not None and self._clip_grads(params)):
            return loss
        self._ratios = {}
        for group in self.param_groups:
            _check_lamb_flags(group)
            (b1, b2), lr, eps, wd = group["betas"], group["lr"], group["eps"], group["weight_decay"]
            adapt = wd != 0 or group["always_adapt"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients")
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if self.ema_decay is not None and "ema" not in st:
                    st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
                st["step"] += 1
                t = int(float(st["step"]))
                m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
                m.mul_(b1).add_(g, alpha=1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                u = (m / (1.0 - b1 ** t)) / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
                if wd != 0:
                    u = u.add(p, alpha=wd)
                r = torch.ones((), dtype=p.dtype, device=p.device)
                if adapt:
                    wn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
                    r = torch.where((wn > 0) & (un > 0), wn / un, r)
                if group["trust_clip"]:
                    r = r.clamp(max=1.0)
                p.add_(u * r, alpha=-lr)
                self._ratios[p] = r
                if self.ema_decay is not None:
                    e = st["ema"]
                    e.add_(p - e, alpha=1.0 - float(self.ema_decay))
        return loss

    def trust_ratios(self):
        """{parameter: its trust ratio in the last step} as fresh 0-d tensors, as FusedLamb.trust_ratios()."""
        return {p: r.clone() for p, r in self._ratios.items()}

    swap_ema = EmaAdamW.swap_ema


def _decays(name, p, no_decay):
    """param_groups_weight_decay's rule: does the parameter `p` called `name` take weight decay?"""
    listed = name in no_decay or name.rsplit(".", 1)[-1] in no_decay
    return not (p.ndim <= 1 or name.endswith(".bias") or listed)


def param_groups_weight_decay(model, weight_decay, no_decay=("cls_tkn_embd", "pos_embd")):
    """timm's split of a model's trainable parameters into two `param_groups`: `weight_decay = 0` for every parameter
    with `ndim <= 1`, every one whose name ends in ".bias", and every one named in `no_decay` (by its full name or by
    the last component of it, so "pos_embd" names "emdeddings.pos_embd"); `weight_decay` for everything else.
    Parameters with requires_grad off are left out.  LAMB's rule for `weight_decay == 0` tensors (no trust ratio)
    only bites where biases and norm weights sit in such a group; nothing calls this unless asked to."""
    plain, decay = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (plain, decay)[_decays(name, p, no_decay)].append(p)
    return [{"params": plain, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def _layer_id(name, num_blocks):
    """timm's layer id on this model's tree: the embeddings 0, encoder block l is l + 1, everything else (the head)
    num_blocks + 1."""
    parts = name.split(".")
    if parts[0] == "emdeddings":
        return 0
    if parts[:2] == ["transformer_encoder", "blocks"] and len(parts) > 2 and parts[2].isdigit():
        return int(parts[2]) + 1
    return num_blocks + 1


def param_groups_layer_decay(model, weight_decay, layer_decay, no_decay=("cls_tkn_embd", "pos_embd")):
    """timm's layer-wise learning-rate decay (BEiT / MAE / DeiT-III fine-tuning) as `param_groups`: a parameter of
    layer i of L + 2 (the embeddings are layer 0, `transformer_encoder.blocks.{l}` is l + 1, the `mlp` head L + 1) goes
    into a group with `lr_scale = layer_decay ** (L + 1 - i)`, so the head trains at the full rate and every layer
    below it at `layer_decay` times the rate of the one above.  Within a layer param_groups_weight_decay's rule splits
    decay from no decay; the groups come in ascending layer order, no-decay first, empty ones dropped, parameters
    with requires_grad off left out.  `lr_scale` takes effect through LRSchedule, which sets
    `group["lr"] = value * lr_scale` (kind "constant" for a fixed rate)."""
    if not 0.0 < layer_decay <= 1.0:
        raise ValueError(f"layer_decay must lie in (0, 1] (got {layer_decay!r})")
    L = len(model.transformer_encoder.blocks)
    layers = [([], []) for _ in range(L + 2)]      # per layer: (no decay, decay)
    for name, p in model.named_parameters():
        if p.requires_grad:
            layers[_layer_id(name, L)][_decays(name, p, no_decay)].append(p)
    return [{"params": ps, "weight_decay": wd, "lr_scale": layer_decay ** (L + 1 - i)}
            for i, pair in enumerate(layers) for ps, wd in zip(pair, (0.0, weight_decay)) if ps]


class LRSchedule:
    """A per-step learning-rate schedule with linear warmup over any torch.optim.Optimizer: timm's CosineLRScheduler
    with `warmup_prefix=True`, `t_in_epochs=False` and `t_initial = total_steps - warmup_steps` (kind "cosine"), or a
    constant rate after the same warmup (kind "constant").  Stepped once per optimizer step, not per epoch.  A group's
    base rate is `group.setdefault("initial_lr", group["lr"])` (torch's convention; it survives load_state_dict).  For
    the update with 0-based index t, W = warmup_steps, N = total_steps:

        t < W:      v = warmup_lr + (base - warmup_lr) * t / W
        W <= t < N: v = min_lr + (base - min_lr) * (1 + cos(pi * (t - W) / (N - W))) / 2      (constant: v = base)
        t >= N:     v = min_lr                                                                (constant: v = base)

    in Python doubles, and `group["lr"] = v * group.get("lr_scale", 1.0)` (param_groups_layer_decay's scale).
    Constructing it applies t = 0; step() advances t and applies; set_step(t) applies at a given t; state_dict()
    carries only t.  On the device nothing is copied: FusedAdamW reads `group["lr"]` at every step."""

    KINDS = ("constant", "cosine")

    def __init__(self, optimizer, kind, total_steps, warmup_steps=0, warmup_lr=0.0, min_lr=0.0):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {self.KINDS} (got {kind!r})")
        if total_steps < 0 or warmup_steps < 0 or warmup_lr < 0 or min_lr < 0:
            raise ValueError("total_steps, warmup_steps, warmup_lr and min_lr must not be negative")
        if warmup_steps > total_steps:
            raise ValueError(f"warmup_steps ({warmup_steps}) exceeds total_steps ({total_steps})")
        self.optimizer, self.kind = optimizer, kind
        self.total_steps, self.warmup_steps = int(total_steps), int(warmup_steps)
        self.warmup_lr, self.min_lr = float(warmup_lr), float(min_lr)
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
        self.set_step(0)

    def value(self, base, t):
        """The rate at update `t` of a group whose base rate is `base`, before its lr_scale."""
        W, N = self.warmup_steps, self.total_steps
        if t < W:
            return self.warmup_lr + (base - self.warmup_lr) * t / W
        if self.kind == "constant":
            return base
        if t >= N:
            return self.min_lr
        return self.min_lr + 0.5 * (base - self.min_lr) * (1.0 + math.cos(math.pi * (t - W) / (N - W)))

    def set_step(self, t):
        self.t = int(t)
        for group in self.optimizer.param_groups:
            base = group.setdefault("initial_lr", group["lr"])
            group["lr"] = self.value(base, self.t) * group.get("lr_scale", 1.0)

    def step(self):
        self.set_step(self.t + 1)

    def last_lr(self):
        """The first group's rate before its lr_scale: what train() logs."""
        group = self.optimizer.param_groups[0]
        return self.value(group["initial_lr"], self.t)

    def state_dict(self):
        return {"t": self.t}

    def load_state_dict(self, state_dict):
        self.set_step(state_dict["t"])


def make_optimizer(params, lr=1e-4, weight_decay=1e-4, device="cuda", max_grad_norm=None, skip_nonfinite=True,
                   ema_decay=None, opt="adamw", always_adapt=False, trust_clip=False, fuse_groups=False):
    """The reference's optimizer (train.py:66, AdamW(lr, weight_decay=1e-4)): FusedAdamW on a ROCm device,
    torch.optim.AdamW on the host path.  `max_grad_norm` (not in the reference) clips by global gradient norm inside
    the step: FusedAdamW's own keyword on the device, ClippedAdamW on the host.  `ema_decay` (not in the reference
    either) keeps an EMA of the weights inside the step: FusedAdamW's keyword on the device, EmaAdamW on the host.
    `opt="lamb"` (not in the reference) gives FusedLamb on the device and Lamb on the host, with `always_adapt` and
    `trust_clip` as their group defaults; `params` may be param_groups_weight_decay()'s or
    param_groups_layer_decay()'s groups.  `fuse_groups` is FusedAdamW's / FusedLamb's keyword: every group in one
    launch; the host path ignores it."""
    if opt not in ("adamw", "lamb"):
        raise ValueError(f"opt must be 'adamw' or 'lamb' (got {opt!r})")
    if opt == "lamb":
        cls, kw = (Lamb, {}) if torch.device(device).type == "cpu" else (FusedLamb, dict(fuse_groups=fuse_groups))
        return cls(params, lr=lr, weight_decay=weight_decay, always_adapt=always_adapt, trust_clip=trust_clip,
                   max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, **kw)
    if always_adapt or trust_clip:
        raise ValueError("always_adapt and trust_clip belong to opt='lamb'")
    if torch.device(device).type == "cpu":
        if ema_decay is not None:
            return EmaAdamW(params, ema_decay, max_grad_norm, skip_nonfinite, lr=lr, weight_decay=weight_decay)
        if max_grad_norm is None:
            return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay)
        return ClippedAdamW(params, max_grad_norm, skip_nonfinite, lr=lr, weight_decay=weight_decay)
    return FusedAdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                      skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, fuse_groups=fuse_groups)


class CrossEntropyLoss(nn.Module):
    """Drop-in for nn.CrossEntropyLoss() as used by the reference (train.py:81): mean reduction, no weights.
    `label_smoothing` mirrors torch's keyword; `labels` may be MixedLabels (cross_entropy)."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        _check_label_smoothing(label_smoothing)
        self.label_smoothing = label_smoothing

    def forward(self, logits, labels):
        return cross_entropy(logits, labels, self.label_smoothing)
