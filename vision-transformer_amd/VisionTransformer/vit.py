"""PatchEmbedding and VisionTransformer — drop-in for src/VisionTransformer/vit.py.

Same constructors, attribute names (including the reference's `emdeddings` spelling), parameters, state_dict keys and
init draw order as the reference (vit.py:9-80).  `VisionTransformer.forward` runs the fused MI355X engine
(`_engine.Engine`): patch im2col + MFMA GEMM with bias/pos epilogue, L encoder blocks of fused kernels, and the
classifier MLP on token 0 (the first PATCH token, because the CLS token is appended last — vit.py:41,80).

Extra (additive) API:
  * `model.compute_dtype` — from ViTConfig (bf16 or fp32 arithmetic);
  * `model.store_attention_probs` — each block's `multi_head.attention_probs` [B, H, T, T] (transformer.py:48, which
    the reference fills on every forward).  None (default) = auto: filled whenever all blocks' probabilities
    together take at most `ATTENTION_PROBS_AUTO_BYTES` (256 MiB: C1 always, ViT-B/16 224² up to 12 images), left
    None above that (ViT-B/16 B=256 would write 477 MB per layer per step).  A forward that stores them runs the
    probability-writing attention kernel and no query-0 / two-chain shortcuts; set False for small-batch latency
    runs.  True / False force it on / off;
  * `model.enable_data_parallel(group=None, force=False)` — all-reduce (average) gradients over `torch.distributed`
    (RCCL) bucket-by-bucket while the backward is still running.  Use this instead of wrapping the model in
    `torch.nn.parallel.DistributedDataParallel` (which is detected and refused: the fused engine is one autograd
    node, so DDP's per-parameter reducer hooks would never fire);
  * `model.hip_engine` — the engine (flat gradient / shadow-weight buffers).  Every forward checks, on the host,
    that its cached state still belongs to the module's weights, and detects by itself:
      - in-place writes on the parameters that autograd versions (`p.mul_()` / `p.copy_()` / `nn.init.*` under
        `no_grad`, writes through `state_dict()` tensors, plain `load_state_dict`, `vector_to_parameters`, torch
        for-loop / foreach optimizers), and the step of any optimizer other than FusedAdamW, torch's `fused=True`
        ones included (they bump no version; an optimizer step hook reports them): the shadow weights are
        repacked;
      - re-pointed storage (`p.data = t`, `model.to(device)`, `model.double().float()`), by each parameter's
        address, and replaced objects (`model.mlp[3] = nn.Linear(4 * D, nc)` — `vit_config.num_classes` then
        follows the new head —, `module.weight = nn.Parameter(...)`, `load_state_dict(assign=True)`), by
        identity against the module tree: the engine rebuilds its buffers around the current parameters
        (gradients already accumulated are carried over by the next backward).  A replacement must keep the
        shape the config gives the parameter, the head's class count apart.
    NOT detected: in-place writes that bump no version counter — through `p.data` (`p.data.mul_()`,
    `p.data.copy_()`), and on the device `torch.optim.swa_utils.AveragedModel.update_parameters` after its first
    call (torch's `_foreach_lerp_` kernel; the first call copies, which is versioned).  Call
    `model.hip_engine.repack()` after them (a no-op before the first forward, which packs anyway).  Nor storage
    re-pointed twice between two forwards that lands on the address it started from.
    An EMA of the weights needs neither `AveragedModel` nor `repack()`: `FusedAdamW(ema_decay=...)` keeps it inside
    the optimizer's launch, and its `ema_weights()` swaps it in and out of this model's own buffers, shadows included
    (optim.py).  `AveragedModel` still works, with the `repack()` above.

  * `model.attention_rollout(x, token=0, head_fusion="mean")` — (logits, [B, T] attention-rollout maps of the token
    the classifier reads) without any [B, H, T, T] tensor on the device, and `model.patch_map(maps, image_hw)` to lay
    them out as patch images (rollout.py);
  * `model.drop_path_rates` — stochastic depth: a list of one rate per encoder block, built from
    `ViTConfig(drop_path_rate=...)` by timm's linspace rule and settable (a list of `num_blocks` numbers in [0, 1)).
    In training mode each block drops each of its two residual branches per image with its rate and scales the
    kept ones by 1 / (1 - rate) (timm's `drop_path`, scale_by_keep=True), inside the proj / fc2 GEMM epilogues; in
    eval mode and at rate 0 nothing changes.  Plain attributes, no parameter or buffer: `state_dict()` and
    checkpoints are unchanged;
  * `model.patch_drop_rate` — patch dropout (timm's patch_drop_rate), from `ViTConfig(patch_drop_rate=...)` and
    settable (a number in [0, 1)).  In training mode every image keeps `config.patch_keep_count(N, rate)` of its N
    patch tokens — patch 0, the token the classifier reads, always, the others a uniform random subset drawn per image
    and per step on the device (vit_patch_keep, no host sync) — plus the CLS token, in ascending order with CLS last;
    the selection happens after `+ pos`, dropped patches are never embedded, and every block runs on T' = K + 1
    tokens.  `model(x, keep_indices=idx)` takes the table from the caller instead (int32 / int64 [B, K], ascending,
    column 0 equal to 0; checked for shape and dtype only), and `model.last_patch_keep` is the table the last
    training forward used ([B, K] int32 on the model's device, None before one).  Eval mode and rate 0 are exactly the
    model without the keyword.  A plain attribute: `state_dict()` and checkpoints are unchanged.

Device semantics (the reference picks 'cuda' or 'cpu', train.py:26): a model on a ROCm device runs the fused HIP
engine and fails loudly when libvit_hip.so is missing; a model on the CPU runs the host path `_cpu.py` (plain torch
ops, standard autograd).  A CUDA input never falls back to the host path.

Gradient semantics kept from the reference module: `requires_grad=False` parameters get no gradient (`.grad` stays
None and their weight-gradient GEMMs are skipped), `x.requires_grad` yields the input gradient, and parameter hooks
(`register_hook`, `register_post_accumulate_grad_hook`) run once per backward, after the gradients are complete.
"""
import copy
import os

import torch
import torch.nn as nn

from . import _cpu
from . import _functional as Fh
from . import config as _config  # noqa: F401  (reference module imports config alongside transformer)
from . import rollout as _rollout
from . import transformer
from ._engine import Engine, ViTFunction

# store_attention_probs=None (auto) fills attention_probs when B * H * T^2 * 4 bytes * blocks fits in this budget
# (environment VIT_ATTENTION_PROBS_AUTO_BYTES overrides it, and reaches spawned worker processes too)
ATTENTION_PROBS_AUTO_BYTES = int(os.environ.get("VIT_ATTENTION_PROBS_AUTO_BYTES", 256 << 20))


class PatchEmbedding(nn.Module):
    def __init__(self, input_channels, embedding_size, patch_size, batch_size, num_patches, precision, device):
        super().__init__()
        # master weights are fp32 regardless of `precision` (which selects the compute dtype instead)
        self.sequence = nn.Sequential(
            nn.Conv2d(in_channels=input_channels, out_channels=embedding_size, kernel_size=patch_size,
                      stride=patch_size, device=device, dtype=torch.float32),
            nn.Flatten(2),
        )
        self.cls_tkn_embd = nn.Parameter(torch.randn(size=(batch_size, 1, embedding_size), device=device),
                                         requires_grad=True)
        self.pos_embd = nn.Parameter(torch.randn(size=(1, num_patches + 1, embedding_size), device=device),
                                     requires_grad=True)
        self.patch_size = patch_size
        self.compute_dtype = precision if precision in (torch.float32, torch.bfloat16) else torch.float32

    def forward(self, x):
        conv = self.sequence[0]
        return Fh.patch_embed(x, conv.weight, conv.bias, self.cls_tkn_embd, self.pos_embd, self.patch_size,
                              self.compute_dtype)


class VisionTransformer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.vit_config = config
        self.compute_dtype = getattr(config, "compute_dtype", None) or (
            config.precision if config.precision in (torch.float32, torch.bfloat16) else torch.float32)
        self.emdeddings = PatchEmbedding(
            input_channels=config.input_channels,
            embedding_size=config.embedding_size,
            patch_size=config.patch_size,
            num_patches=config.num_patches,
            precision=self.compute_dtype,
            batch_size=config.batch_size,
            device=config.device,
        )
        self.transformer_encoder = transformer.TransformerEncoder(
            embedding_size=config.embedding_size,
            num_heads=config.num_heads,
            num_blocks=config.num_blocks,
            block_size=config.num_patches + 1,
        )
        self.mlp = nn.Sequential(
            nn.Linear(config.embedding_size, 4 * config.embedding_size),
            nn.GELU(),
            nn.LayerNorm(4 * config.embedding_size),
            nn.Linear(4 * config.embedding_size, config.num_classes),
        )
        self.store_attention_probs = None        # auto (module docstring); True / False force it
        self.drop_path_rates = _config.drop_path_rates(getattr(config, "drop_path_rate", 0.0), config.num_blocks)
        self.patch_drop_rate = getattr(config, "patch_drop_rate", 0.0)
        self.last_patch_keep = None
        self._engine = None
        self._anchor = None

    @property
    def patch_drop_rate(self):
        """Patch-dropout rate of training forwards (module docstring); assign a number in [0, 1)."""
        return self.__dict__.get("_patch_drop_rate", 0.0)       # (0: a model pickled before the attribute)

    @patch_drop_rate.setter
    def patch_drop_rate(self, rate):
        self.__dict__["_patch_drop_rate"] = _config.check_patch_drop_rate(rate)

    @property
    def vit_config(self):
        """The config the model was built from, with `num_classes` following the classifier head the module holds
        now (`model.mlp[3] = nn.Linear(4 * D, nc)`): a model built from it loads this model's state_dict.  The
        constructor's config object itself, which other models may share, is never written."""
        d = self.__dict__
        cfg = d["_vit_config"] if "_vit_config" in d else d["vit_config"]      # (a model pickled before the property)
        mlp = self._modules.get("mlp")
        w = getattr(mlp[3], "weight", None) if mlp is not None and len(mlp) > 3 else None
        if w is not None and w.dim() == 2 and w.shape[0] != cfg.num_classes:
            cfg = copy.copy(cfg)
            cfg.num_classes = w.shape[0]
            d["_vit_config"] = cfg
        return cfg

    @vit_config.setter
    def vit_config(self, config):
        self.__dict__["_vit_config"] = config

    @property
    def drop_path_rates(self):
        """Stochastic-depth rate of every encoder block (module docstring), as a copy: assign a whole list of
        num_blocks rates to change them, so that every entry is validated."""
        rates = self.__dict__.get("_drop_path_rates")        # (None: a model pickled before the attribute)
        return list(rates) if rates is not None else [0.0] * self.vit_config.num_blocks

    @drop_path_rates.setter
    def drop_path_rates(self, rates):
        rates = [_config.check_drop_path_rate(p, f"drop_path_rates[{i}]") for i, p in enumerate(rates)]
        n = self.vit_config.num_blocks
        if len(rates) != n:
            raise ValueError(f"drop_path_rates needs one rate per encoder block ({n}), got {len(rates)}")
        self.__dict__["_drop_path_rates"] = rates

    @property
    def hip_engine(self):
        if self._engine is None:
            self._engine = Engine(self)
        return self._engine

    def enable_data_parallel(self, group=None, force=False, grad_dtype=torch.float32, launch_mode="auto"):
        """Average gradients across the process group with RCCL, bucketed per block, overlapped with backward.
        `force` keeps the all-reduce path on even for a world of one rank (tests the collective on one GPU).
        `grad_dtype=torch.bfloat16` sends each bucket as bf16 (half the xGMI ring bytes): the fp32 gradients are
        rounded to bf16, averaged in bf16 and widened back; master weights and optimizer state stay fp32.
        `launch_mode` of the backward's GEMMs and fused attention backward beside the collectives: "shared" (one
        workgroup per item, VIT_FLAG_SHARED_CUS), "persistent" (one workgroup per CU) or "auto" = persistent: with
        CU-holding kernels beside the backward in place of RCCL's (tools/cu_hog_ab.py) the persistent grids stayed
        0.2-0.3 ms/step faster than the shared-CU launch, whose own cost is 0.4-0.7 ms/step (no N > 1
        measurement exists yet).  Results are bitwise the same in every mode."""
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("enable_data_parallel: torch.distributed is not initialised")
        if grad_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("enable_data_parallel: grad_dtype must be torch.float32 or torch.bfloat16")
        if launch_mode not in ("auto", "shared", "persistent"):
            raise ValueError("enable_data_parallel: launch_mode must be 'auto', 'shared' or 'persistent'")
        eng = self.hip_engine
        eng.ddp_group = group
        eng.comm_dtype = grad_dtype
        eng.ddp_enabled = bool(force) or dist.get_world_size(group) > 1
        # "shared": the backward's kernels launch one workgroup per item instead of a persistent one-per-CU grid
        # (VIT_FLAG_SHARED_CUS, vit_hip.h), so RCCL's all-reduce kernels beside them never wait for a whole grid
        eng.shared_cus = eng.ddp_enabled and launch_mode == "shared"
        # each replica draws its own dropout masks (the rank is folded into the forward's dropout seed)
        eng.dropout_rank = dist.get_rank(group) if eng.ddp_enabled else 0
        return self

    # the engine holds a weakref to its model and views of the parameters: never copy or pickle it (a deep copy or
    # an unpickled model builds its own engine on first use)
    def __getstate__(self):
        state = dict(super().__getstate__())
        state["_engine"] = None
        state["_anchor"] = None
        return state

    def __deepcopy__(self, memo):
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            object.__setattr__(new, k, copy.deepcopy(v, memo))
        return new

    def wants_attention_probs(self, batch):
        """Whether a forward over `batch` images fills every block's `multi_head.attention_probs`: the
        store_attention_probs setting, or with None (auto) whether they fit in ATTENTION_PROBS_AUTO_BYTES."""
        s = self.store_attention_probs
        if s is not None:
            return bool(s)
        c = self.vit_config
        T = c.num_patches + 1
        return batch * c.num_heads * T * T * 4 * c.num_blocks <= ATTENTION_PROBS_AUTO_BYTES

    def _check_not_ddp_wrapped(self):
        from torch.nn.parallel import DistributedDataParallel as DDP
        active = DDP._get_active_ddp_module()
        if active is not None and any(m is self for m in active.module.modules()):
            raise RuntimeError(
                "VisionTransformer must not be wrapped in torch.nn.parallel.DistributedDataParallel: the fused HIP "
                "engine is a single autograd node, so DDP's per-parameter reducer would never see the gradients. "
                "Call model.enable_data_parallel() instead (bucketed RCCL all-reduce overlapped with the backward).")

    def forward(self, x, keep_indices=None):
        if not x.is_cuda and all(not p.is_cuda for p in (self.mlp[3].weight, self.emdeddings.pos_embd)):
            # host path: the model lives on the CPU (train.py:26)
            return _cpu.vit_forward(self, x, keep_indices=keep_indices)
        self._check_not_ddp_wrapped()
        eng = self.hip_engine
        want_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if want_grad:
            if self._anchor is None or self._anchor.device != x.device:
                self._anchor = torch.zeros((), device=x.device, requires_grad=True)
            return ViTFunction.apply(x, self._anchor, eng, self.training, self.wants_attention_probs(x.shape[0]),
                                     keep_indices)
        logits, _ = eng.forward(x, self.training, save=False, want_probs=self.wants_attention_probs(x.shape[0]),
                                keep=keep_indices)
        return logits

    def attention_rollout(self, x, token=0, head_fusion="mean", return_layers=False, fast_attention=False):
        """(logits, maps [B, T] fp32): the attention rollout of `token` (rollout.py; 0 is the token the classifier
        reads, T - 1 the CLS token) for every image of x, from an eval-mode forward under no_grad — no dropout, no
        drop path, whatever `model.training` says; neither it nor `store_attention_probs` is changed.  With
        `return_layers` also [L, B, T] fp32: entry l is the chain after block l's step, entry 0 the maps.
        On a ROCm device no [B, H, T, T] tensor exists at any time: the forward keeps each block's qkv
        (`Engine.forward(keep_qkv=True)`; its logits are bitwise those of a `store_attention_probs = True` forward) and
        `Engine.rollout` forms the chain from them, one HIP launch pair per block, with no host sync.  A model on the
        CPU stores the probabilities and goes through `rollout.rollout_from_probs`.  `head_fusion`: "mean", "max" or
        "min" over the heads.  `fast_attention` (device only): the forward runs the attention kernel of a plain
        forward instead of the probability-storing forward's — in bf16 at head size 64 the MFMA kernel, which makes
        the call 5.6x faster at ViT-B/16 B 256; logits and maps are then those of a plain forward's
        kernels: another valid bf16 evaluation of the model, no longer bitwise the probability-storing forward's."""
        T = self.vit_config.num_patches + 1
        token = _rollout.check_rollout_args(token, head_fusion, T)
        with torch.no_grad():
            if not x.is_cuda and all(not p.is_cuda for p in (self.mlp[3].weight, self.emdeddings.pos_embd)):
                logits = _cpu.vit_forward(self, x, training=False, want_probs=True)
                probs = [blk.multi_head.attention_probs for blk in self.transformer_encoder.blocks]
                maps, layers = _rollout.rollout_from_probs([p.float() for p in probs], token, head_fusion, True)
            else:
                eng = self.hip_engine
                logits, _, qkvs = eng.forward(x, False, save=False, keep_qkv="fast" if fast_attention else True)
                maps, layers = eng.rollout(qkvs, token, head_fusion, trace=True) if return_layers else \
                    (eng.rollout(qkvs, token, head_fusion), None)
        return (logits, maps, layers) if return_layers else (logits, maps)

    def patch_map(self, maps, image_hw):
        """[B, T] token maps (attention_rollout) as [B, H / P, W / P] images of the patches: the CLS entry (index N,
        appended last) is dropped and the N patch entries are laid out row-major, as the patch embedding flattens
        them (vit.py:29).  `image_hw`: the (H, W) of the input images."""
        P = self.vit_config.patch_size
        gh, gw = int(image_hw[0]) // P, int(image_hw[1]) // P
        N = self.vit_config.num_patches
        if maps.dim() != 2 or maps.shape[1] != N + 1 or gh * gw != N:
            raise ValueError(f"patch_map: maps must be [B, {N + 1}] and image_hw give {N} patches of {P} x {P}, got "
                             f"{tuple(maps.shape)} and {gh} x {gw}")
        return maps[:, :N].reshape(maps.shape[0], gh, gw)


def load_teacher(config, checkpoint, *, student=None, ema=False, device=None):
    """The frozen teacher of a distillation run (optim.distillation_loss): a VisionTransformer(config) with the
    "model_state_dict" (`ema`: the "ema_state_dict") of `checkpoint` — a checkpoint file, or a directory, of which the
    newest N.pt is read as train.search_checkpoint finds it — moved to `device`, in eval mode, every parameter with
    requires_grad False, and `store_attention_probs` False: its forward under no_grad keeps no tape and no
    probabilities.  `student` (a ViTConfig or a model): the teacher must share its num_classes, and its batch_size
    because the CLS parameter is batch-shaped (vit.py:32); preset, depth, width, patch size and compute dtype are the
    teacher's own, as long as it takes the student's input."""
    import glob
    import re
    if student is not None:
        s = getattr(student, "vit_config", student)
        for field in ("num_classes", "batch_size"):
            if getattr(config, field) != getattr(s, field):
                raise ValueError(f"load_teacher: the teacher's {field} ({getattr(config, field)}) differs from the "
                                 f"student's ({getattr(s, field)}): the two models must score the same classes on the "
                                 "same batch (the CLS parameter is batch-shaped)")
    path = os.fspath(checkpoint)
    if os.path.isdir(path):
        nums = [int(m.group(1)) for m in (re.match(r"(\d+)(?=\.pt)", os.path.basename(f))
                                          for f in glob.glob(os.path.join(path, "*.pt"))) if m]
        if not nums:
            raise FileNotFoundError(f"load_teacher: no checkpoint (N.pt) in {path!r}")
        path = os.path.join(path, f"{max(nums)}.pt")
    elif not os.path.isfile(path):
        raise FileNotFoundError(f"load_teacher: no checkpoint at {path!r}")
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    key = "ema_state_dict" if ema else "model_state_dict"
    if key not in ckpt:
        raise KeyError(f"load_teacher: {path!r} has no {key!r}"
                       + (" (it was trained without a weight EMA)" if ema else ""))
    model = VisionTransformer(config)
    try:
        model.load_state_dict(ckpt[key])
    except RuntimeError as e:
        raise ValueError(f"load_teacher: {path!r} does not hold a model of {config!r}: {e}") from None
    if device is not None:
        model = model.to(device)
    model.eval()
    model.requires_grad_(False)
    model.store_attention_probs = False
    return model
