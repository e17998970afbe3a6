"""Fused optimizer and loss for the training step (train.py:66,81,93,96).

FusedAdamW: torch.optim.AdamW semantics (decoupled weight decay, bias-corrected moments, amsgrad off) in ONE
multi-tensor HIP launch over every parameter; the same kernel refreshes the compute-dtype shadow weights the fused
engine reads (bf16 copies of the fp32 masters), so no separate cast pass runs per step.  The optimizer state keys
('step', 'exp_avg', 'exp_avg_sq') are those of torch.optim.AdamW, so `optimizer.state_dict()` checkpoints are
interchangeable with the reference's (train.py:73,110).

CrossEntropyLoss: nn.CrossEntropyLoss() (mean) as one fused softmax + NLL + gradient kernel.
"""
import contextlib
import math

import torch
import torch.nn as nn

from . import _ops
from ._engine import shadow_of


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


class FusedAdamW(_EmaSurface, torch.optim.Optimizer):
    """Step bookkeeping stays on the host: each group's per-parameter 'step' entries are 0-d views of ONE CPU
    tensor (torch AdamW's state format, so `state_dict()` / `load_state_dict()` interchange with it), advanced by a
    single in-place add per step, with a host-side mirror of the counts for the bias corrections — no per-parameter
    `.item()` or `+= 1` on the step path.  Device chunk tables are cached per (group, step-count class) and hold
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
    the all-reduce, hence the same weights and the same EMA."""

    # its kernel writes the engines' compute-dtype shadows along with the masters: no repack follows a step
    # (_engine._after_optimizer_step marks them stale after every other optimizer's)
    refreshes_shadows = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
                 max_grad_norm=None, skip_nonfinite=True, ema_decay=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        _check_max_grad_norm(max_grad_norm)
        _check_ema_decay(ema_decay)
        self._version = 0
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale
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

    def _clipped_launch(self, work):
        """grad_sumsq per table into consecutive slices of one partial buffer, one finish, the clipped update per
        table — all on the current stream, which the engine's backward() has already made wait for the weight-
        gradient stream and the all-reduce handles."""
        _check_max_grad_norm(self.max_grad_norm)
        device = work[0][5]
        if any(w[5] != device for w in work):
            raise RuntimeError("FusedAdamW: a global gradient norm needs every parameter on one device")
        total = sum(w[1] for w in work)
        if self._partial is None or self._partial.device != device or self._partial.numel() < total:
            self._partial = torch.empty(total, dtype=torch.float64, device=device)
        clip = self._clip_state(device)
        off = 0
        for dev_tab, n, *_ in work:
            _ops.grad_sumsq(dev_tab, n, self.grad_scale, self._partial[off:off + n])
            off += n
        _ops.grad_clip_finish(self._partial, total, self.max_grad_norm, clip, self.skip_nonfinite)
        for dev_tab, n, sdt, group, t, _, ema_dev in work:
            self._adamw(dev_tab, n, sdt, group, t, clip, ema_dev)

    def _adamw(self, dev_tab, n, sdt, group, t, clip=None, ema_dev=None):
        b1, b2 = group["betas"]
        if self.ema_decay is not None:
            _ops.adamw_ema(dev_tab, ema_dev, n, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                           1.0 - b1 ** t, 1.0 - b2 ** t, self.grad_scale, sdt, self.ema_decay, clip=clip)
            return
        _ops.adamw(dev_tab, n, group["lr"], b1, b2, group["eps"], group["weight_decay"], 1.0 - b1 ** t,
                   1.0 - b2 ** t, self.grad_scale, sdt, clip=clip)

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

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse_step_while_swapped()
        ema = self.ema_decay is not None
        if ema:
            _check_ema_decay(self.ema_decay)
        clipped, work = self.max_grad_norm is not None, []
        for gi, group in enumerate(self.param_groups):
            ps_all = group["params"]
            idx = [i for i, p in enumerate(ps_all) if p.grad is not None]
            if not idx:
                continue
            plist = [ps_all[i] for i in idx]
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
            if fresh:
                self.invalidate()
            buf, host = self._step_state(gi, group)
            # advance the counters: one in-place add on the shared tensor, host mirror in Python ints
            if len(idx) == len(ps_all):
                buf += 1
            else:
                buf[torch.tensor(idx)] += 1
            by_step = {}
            for i in idx:
                host[i] += 1
                by_step.setdefault(host[i], []).append(ps_all[i])
            for t, ps in by_step.items():
                # one table for the whole group while every parameter has the same step count, else one per count
                key = (gi, "all") if len(by_step) == 1 else (gi, "t", t)
                tab = self._tables.get(key)
                if tab is not None and not self._table_valid(tab, ps):
                    tab = None
                if tab is None:
                    shadows = [shadow_of(p) for p in ps]
                    sdt = next((s.dtype for s in shadows if s is not None), torch.float32)
                    shadows = [s if (s is not None and s.dtype == sdt) else None for s in shadows]
                    entries = [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"], s)
                               for p, s in zip(ps, shadows)]
                    for p, g, m, v, _ in entries:
                        for tt in (g, m, v):
                            if not tt.is_contiguous():
                                raise RuntimeError("FusedAdamW: non-contiguous grad/state")
                    dev_tab, n = _ops.build_chunk_table(entries, ps[0].device)
                    emas = [self.state[p].get("ema") for p in ps]
                    if all(e is None for e in emas):
                        emas = ema_dev = None
                    else:
                        ema_dev, _ = _ops.build_ema_pointers(list(zip(ps, emas)), ps[0].device)
                    # entries keep every tabled tensor alive; the raw shadow list is what the identity check compares
                    tab = (self._version, list(ps), [p.grad for p in ps], [shadow_of(p) for p in ps], dev_tab, n,
                           sdt, entries, [p.data_ptr() for p in ps],
                           [(self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in ps],
                           [p.grad.data_ptr() for p in ps], emas, ema_dev)
                    self._tables[key] = tab
                dev_tab, n, sdt, ema_dev = tab[4], tab[5], tab[6], tab[12]
                if clipped:      # the norm spans every table: launch once they all exist
                    work.append((dev_tab, n, sdt, group, t, ps[0].device, ema_dev))
                else:
                    self._adamw(dev_tab, n, sdt, group, t, None, ema_dev)
        if work:
            self._clipped_launch(work)
        return loss

    def _table_valid(self, tab, ps):
        """Same optimizer version, same parameters, every parameter still holds the same .grad tensor object and the
        same moment tensor objects as when the table was built, and no parameter's or gradient's storage moved (`p.data = ...`
        re-points storage without changing any object identity).  Two data_ptr() per parameter plus
        identity checks: this runs every step.  The engine's shadows change only when it rebuilds its buffers, and
        then every gradient view is a new object too.  A table built with EMA pointers also wants every parameter's
        `state[p]["ema"]` to be the tensor object it points at; one built without serves only the EMA-less step."""
        ver, tps, grads, ptrs, moments, gptrs = tab[0], tab[1], tab[2], tab[8], tab[9], tab[10]
        if ver != self._version or len(tps) != len(ps):
            return False
        emas = tab[11]
        if emas is None:      # a table without EMA pointers serves only the EMA-less step (no per-parameter work)
            if self.ema_decay is not None:
                return False
        elif any(self.state[a].get("ema") is not e for a, e in zip(tps, emas)):
            return False
        state = self.state
        for a, b, g, ptr, (m, v), gp in zip(tps, ps, grads, ptrs, moments, gptrs):
            # the gradient's storage too: `p.grad.data = t` / `p.grad.set_(...)` keep the .grad object
            if a is not b or a.grad is not g or a.data_ptr() != ptr or g.data_ptr() != gp:
                return False
            st = state[a]
            if st["exp_avg"] is not m or st["exp_avg_sq"] is not v:
                return False
        return True

    # ---- weight EMA ---------------------------------------------------------------------------------------------
    def _ema_swap_tables(self):
        """Chunk tables for vit_ema_swap: every parameter that has an EMA exactly once, whichever step tables exist
        (those carry gradient pointers, go stale with zero_grad(set_to_none=True), and two of them may hold the same
        parameter).  One table per (device, shadow dtype), in practice one.  Reused while the optimizer's version, every
        parameter's storage, EMA tensor object and shadow object are those it was built from."""
        state = self.state       # .get: looking must not create an (empty) state entry for a parameter that has none
        ps = [p for g in self.param_groups for p in g["params"] if (state.get(p) or {}).get("ema") is not None]
        cached = self._swap_tables
        if cached is not None and cached[0] == self._version and len(cached[1]) == len(ps) and all(
                a is b and a.data_ptr() == ptr and self.state[a]["ema"] is e and shadow_of(a) is s
                for (a, ptr, e, s), b in zip(cached[1], ps)):
            return cached[2]
        groups = {}
        for p in ps:
            s = shadow_of(p)
            groups.setdefault((p.device, s.dtype if s is not None else None), []).append((p, self.state[p]["ema"], s))
        for dev in {d for d, _ in groups}:      # shadow-less parameters ride in their device's first table
            bare = groups.pop((dev, None), None)
            if bare:
                key = next((k for k in groups if k[0] == dev), (dev, torch.float32))
                groups.setdefault(key, []).extend(bare)
        tables = []
        for (dev, sdt), ents in groups.items():
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p, _, _ in ents):
                raise RuntimeError("FusedAdamW: parameters must be contiguous float32 on a ROCm device")
            dev_tab, n = _ops.build_chunk_table([(p.detach(), None, None, None, s) for p, _, s in ents], dev)
            ema_dev, _ = _ops.build_ema_pointers([(p, e) for p, e, _ in ents], dev)
            tables.append((dev_tab, ema_dev, n, sdt, ents))
        self._swap_tables = (self._version, [(p, p.data_ptr(), self.state[p]["ema"], shadow_of(p)) for p in ps], tables)
        return tables

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter that has an EMA with it, in place, and refresh its compute-dtype shadow from the
        new value: one launch per table, no repack, no engine rebuild (the engine reads the same buffers).  A second
        call restores every bit.  Parameters without an EMA are left alone."""
        for dev_tab, ema_dev, n, sdt, _ in self._ema_swap_tables():
            _ops.ema_swap(dev_tab, ema_dev, n, sdt)
        self._ema_swapped = not self._ema_swapped


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


def cross_entropy(logits, labels):
    """mean softmax cross-entropy (nn.CrossEntropyLoss() default) — fused HIP kernel, gradient precomputed; host
    tensors (the CPU path) use torch's own."""
    if not logits.is_cuda:
        return nn.functional.cross_entropy(logits, labels)
    return _XentFn.apply(logits, labels)


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is not None and not (0 < max_grad_norm < math.inf):
        raise ValueError(f"max_grad_norm must be None or a positive finite number (got {max_grad_norm!r})")


class ClippedAdamW(torch.optim.AdamW):
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
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self._norm = torch.zeros(())
        self._skipped = 0

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not params:
            return loss
        self._norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm).detach().clone()
        if self.skip_nonfinite and not bool(torch.isfinite(self._norm)):
            self._skipped += 1
            return loss
        super().step()
        return loss

    def grad_norm(self):
        return self._norm.clone()

    def skipped_steps(self):
        return torch.tensor(float(self._skipped))


class EmaAdamW(_EmaSurface, torch.optim.AdamW):
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
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self._norm = torch.zeros(())
        self._skipped = 0

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse_step_while_swapped()
        _check_ema_decay(self.ema_decay)
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not params:
            return loss
        if self.max_grad_norm is not None:
            self._norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm).detach().clone()
            if self.skip_nonfinite and not bool(torch.isfinite(self._norm)):
                self._skipped += 1
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

    def grad_norm(self):
        return self._norm.clone()

    def skipped_steps(self):
        return torch.tensor(float(self._skipped))


def make_optimizer(params, lr=1e-4, weight_decay=1e-4, device="cuda", max_grad_norm=None, skip_nonfinite=True,
                   ema_decay=None):
    """The reference's optimizer (train.py:66, AdamW(lr, weight_decay=1e-4)): FusedAdamW on a ROCm device,
    torch.optim.AdamW on the host path.  `max_grad_norm` (not in the reference) clips by global gradient norm inside
    the step: FusedAdamW's own keyword on the device, ClippedAdamW on the host.  `ema_decay` (not in the reference
    either) keeps an EMA of the weights inside the step: FusedAdamW's keyword on the device, EmaAdamW on the host."""
    if torch.device(device).type == "cpu":
        if ema_decay is not None:
            return EmaAdamW(params, ema_decay, max_grad_norm, skip_nonfinite, lr=lr, weight_decay=weight_decay)
        if max_grad_norm is None:
            return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay)
        return ClippedAdamW(params, max_grad_norm, skip_nonfinite, lr=lr, weight_decay=weight_decay)
    return FusedAdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                      skip_nonfinite=skip_nonfinite, ema_decay=ema_decay)


class CrossEntropyLoss(nn.Module):
    """Drop-in for nn.CrossEntropyLoss() as used by the reference (train.py:81): mean reduction, no weights."""

    def forward(self, logits, labels):
        return cross_entropy(logits, labels)
