"""Fused whole-model engine behind `VisionTransformer.forward` (the training hot path).

One autograd node covers the whole network: the forward (vit.py:77-80 -> transformer.py:76-79 per block ->
vit.py:69-74) runs as a fixed sequence of libvit_hip kernels on the current HIP stream and keeps every activation
the backward needs resident in HBM (ViT-B/16 at B=256 bf16: ~10 GB of 288 GB); the backward replays the block
sequence in reverse and writes every parameter gradient straight into ONE flat fp32 gradient buffer whose views are
exposed as `param.grad`.

Layouts (device):
  * master weights: the module's own fp32 nn.Parameters, untouched (state_dict/optimizer compatibility with the
    reference keys, including per-head `heads.{h}.{key,query,value}.weight`);
  * compute shadow: one buffer in the compute dtype holding, per block, the FUSED QKV matrix [3D, D] (query rows of
    every head, then keys, then values), proj [D, D], fc1 [4D, D], fc2 [D, 4D], and the patch-embedding matrix
    [D, C*P*P]; refreshed by the fused AdamW kernel (or a pack kernel after any external write);
  * gradients: one flat fp32 buffer ordered head | block L-1 | ... | block 0 | embedding, i.e. in the order the
    backward produces them, so data-parallel all-reduce buckets are contiguous ranges launched as soon as a block's
    backward is enqueued (RCCL on its own stream, overlapping the remaining backward).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import weakref
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist
from torch.optim.optimizer import register_optimizer_step_post_hook
from torch.utils.weak import WeakIdKeyDictionary

from . import _lib, _ops
from . import config as _config
from ._ops import ACT_NONE, ACT_RELU

# parameter -> its compute-dtype shadow view (refreshed by FusedAdamW's kernel).  Kept beside the parameters, not as
# attributes on them, so models stay picklable / deep-copyable (torch.save(model), EMA snapshots).
SHADOWS = WeakIdKeyDictionary()


def shadow_of(p):
    return SHADOWS.get(p)


# id(parameter) -> (weak reference to it, weak reference to the engine that captured it): which engines an optimizer
# step wrote to.  Keyed by id for a plain dict lookup per parameter per step; an entry leaves with its parameter.
_ENGINE_OF = {}


def _after_optimizer_step(optimizer, args, kwargs):
    """After the step of any optimizer but FusedAdamW, the shadows of the engines it wrote to are stale.  The version
    counters say so for torch's for-loop and foreach optimizers; its fused ones (`AdamW(fused=True)`, ...) update the
    parameters in one kernel that bumps no version counter, so ensure_ready() could not tell.  Host work only."""
    if getattr(optimizer, "refreshes_shadows", False):
        return
    for group in optimizer.param_groups:
        for p in group["params"]:
            ent = _ENGINE_OF.get(id(p))
            if ent is not None and ent[0]() is p:
                eng = ent[1]()
                if eng is not None:
                    eng._ver_sig = None


register_optimizer_step_post_hook(_after_optimizer_step)


DROPOUT_P = 0.2          # transformer.py:35,53 (config.dropout is stored but unused by the reference)
LN_EPS = 1e-5
PROBS_SCRATCH_BYTES = 64 << 20   # Engine._attn_fwd_as_stored: probabilities of a few images at a time, then dropped
ALIGN = 64               # elements; every sub-tensor of the flat buffers starts 256-B aligned


def _hash_u32(seed, idx):
    """Python twin of the device `vit_hash_u32` (murmur3 fmix32 of idx*golden + seed)."""
    x = (idx * 0x9E3779B1 + seed) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def site_seed(base_seed, layer, site):
    """Dropout seed of (layer, site); site 0 = MHA output (transformer.py:47), 1 = FFN output (:59)."""
    return _hash_u32((base_seed * 0x632BE5AB + 0x1234567) & 0xFFFFFFFF, layer * 2 + site)


def dropout_seed(base_seed, rank=0):
    """Base dropout seed of one forward on data-parallel replica `rank`: the seed drawn from the CPU RNG, with the
    rank hashed in for rank > 0 (rank 0 keeps the single-process seed, so a one-rank job is bitwise a plain run).
    Each replica's masks are then a different counter-hash stream, as independent torch bernoulli draws per rank
    would be (transformer.py:40,59 under an 8-way split of the batch)."""
    if rank == 0:
        return base_seed
    return _hash_u32((base_seed ^ 0x5BD1E995) & 0xFFFFFFFF, 0x27D4EB2F + rank) & 0x7FFFFFFF


def path_keep(base_seed, L, layer, site, B, p):
    """Python twin of the drop-path draw of vit_drop_path_rows: bool [B], image b keeps the branch of (layer, site)
    iff vit_hash_u32(site_seed(base_seed, L + layer, site), b) >= threshold(p).  `base_seed`: the forward's seed after
    dropout_seed; layers L .. 2L-1 keep these streams apart from the element dropout's (0 .. L-1).  The threshold is
    the library's: of p as the fp32 value it receives."""
    thr = min(int(ctypes.c_float(p).value * 4294967296.0), 0xFFFFFFFF)
    s = site_seed(base_seed, L + layer, site)
    return torch.tensor([_hash_u32(s, b) >= thr for b in range(B)], dtype=torch.bool)


def _keep_scale(p):
    """(the element dropout's p folded with a block's drop-path rate, its 1 / keep probability): what the backward's
    consumers of a bare-masked gradient apply.  Rate 0 gives DROPOUT_P and 1 / (1 - DROPOUT_P) as they always were."""
    if p == 0.0:
        return DROPOUT_P, 1.0 / (1.0 - DROPOUT_P)
    keep = (1.0 - DROPOUT_P) * (1.0 - p)
    return 1.0 - keep, 1.0 / keep


class _Region:
    def __init__(self):
        self.size = 0
        self.items = []

    def add(self, name, numel):
        off = self.size
        self.items.append((name, off, numel))
        self.size = off + ((numel + ALIGN - 1) // ALIGN) * ALIGN
        return off


def split_k_for(m, n, k, dtype=torch.bfloat16):
    """K split for a weight-gradient GEMM (reduction over B*T rows), chosen by the library for the kernel it will
    run (vit_gemm_split_k_hint: one round of output tiles x K-slices over the 256 CUs)."""
    return int(_lib.load().vit_gemm_split_k_hint(m, n, k, _ops.dtype_code(dtype)))


def head_split_for(m, n, k):
    """K split for the classifier head's fp32 GEMMs (M = batch rows only): ~1024 workgroups of the 64x64 fp32
    tile, each slice >= 4 k-steps of 32 (128 k).  Without it these few-tile GEMMs run one long dependent k-loop per
    CU."""
    tiles = ((m + 63) // 64) * ((n + 63) // 64)
    nkt = (k + 31) // 32
    return max(1, min((1024 + tiles - 1) // tiles, nkt // 4, 32))


class Tape:
    """Activations saved by a training forward (`blocks`: one BlockActs per encoder block)."""
    __slots__ = ("B", "cols", "blocks", "z", "u", "gz", "zn", "mh", "rh", "seed", "training", "x_shape", "x_dtype",
                 "x_grad", "pruned", "row0", "path_rates", "T", "K", "idx", "inv")


# per-block gradient regions, in their order in the flat gradient buffer (qkv_w: the fused [3D, D] matrix of every head)
BLOCK_REGIONS = ("qkv_w", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln1_w", "ln1_b", "ln2_w", "ln2_b")


class BlockActs(NamedTuple):
    """The tensors one encoder block's forward writes (Engine._block_bufs allocates them, block_forward fills them)
    and, on the tape, what block_backward reads.  M = B*T rows; R = M, or B in the pruned last block (token-0 rows)."""
    x_in: torch.Tensor      # [M, D] block input
    a1: torch.Tensor        # [M, D] ln1(x_in), with mean / rstd m1, r1 [M] (fp32)
    m1: torch.Tensor
    r1: torch.Tensor
    qkv: torch.Tensor       # [M, 3D]
    o: torch.Tensor         # [M, D] attention output
    o32: Optional[torch.Tensor]   # [M, D] fp32 O, where the attention backward takes it (attn_bwd_uses_o32)
    lse: torch.Tensor       # [B, H, T] fp32
    x_mid: torch.Tensor     # [R, D] x_in + drop(proj(o))
    a2: torch.Tensor        # [R, D] ln2(x_mid), with m2, r2 [R]
    m2: torch.Tensor
    r2: torch.Tensor
    h: torch.Tensor         # [R, 4D] relu(fc1(a2))
    hm: Optional[torch.Tensor]    # mask4 of h > 0 (saving forwards)
    pm: Optional[torch.Tensor]    # mask4 keep bits of the proj dropout (saving training forwards)
    fm: Optional[torch.Tensor]    # ... and of the fc2 dropout

    def images(self, b0, B, T):
        """Images b0 .. b0+B-1 of this whole-batch (unpruned) record, as views: T rows per image, lse by image, the
        mask4 tensors by 4-row group (b0*T and B*T multiples of 4)."""
        r0, R = b0 * T, B * T
        D = self.x_mid.shape[1]

        def rows(t):
            return None if t is None else t[r0:r0 + R]

        def bits(mask, n):          # the byte range of rows r0 .. r0+R-1 in the VIT_MASK4 of an [.., n] tensor
            if mask is None:
                return None
            off = (r0 // 4) * ((n + 3) // 4) * 4
            return mask[off:off + _ops.mask4_bytes(R, n)]

        s = self
        return BlockActs(x_in=rows(s.x_in), a1=rows(s.a1), m1=rows(s.m1), r1=rows(s.r1), qkv=rows(s.qkv), o=rows(s.o),
                         o32=rows(s.o32), lse=s.lse[b0:b0 + B], x_mid=rows(s.x_mid), a2=rows(s.a2), m2=rows(s.m2),
                         r2=rows(s.r2), h=rows(s.h), hm=bits(s.hm, 4 * D), pm=bits(s.pm, D), fm=bits(s.fm, D))


class Engine:
    def __init__(self, model):
        self.model_ref = weakref.ref(model)
        cfg = model.vit_config
        self.C, self.P = cfg.input_channels, cfg.patch_size
        self.D, self.H, self.L = cfg.embedding_size, cfg.num_heads, cfg.num_blocks
        self.hd = self.D // self.H
        self.N = cfg.num_patches
        self.T = self.N + 1
        self.nc = cfg.num_classes
        self.B = cfg.batch_size
        self.CPP = self.C * self.P * self.P
        self.dtype = model.compute_dtype
        self.scale = float(self.hd) ** 0.5          # MULTIPLIED (transformer.py:24)
        self.device = None
        self.params = None
        self.ddp_group = None
        self.ddp_enabled = False
        # dtype the gradient buckets travel in over RCCL (enable_data_parallel(grad_dtype=...)): fp32, or bf16 (half
        # the ring bytes; the buffer is averaged in bf16 and widened back into the fp32 gradients)
        self.comm_dtype = torch.float32
        # when set (bench.py, last timed step): HIP events around the bucket waits at the end of the backward, i.e.
        # the communication time the backward did not hide ("exposed"); read with comm_exposed_ms()
        self.time_comm = False
        self._comm_events = None
        self._works = []
        self._ws = [None, None]      # grow-only fp32 scratch: main stream, weight-gradient side stream (_workspace)
        self._tok = None
        self._ptr_sig = None
        self._ver_sig = None
        self.stats = {"packs": 0, "split_forwards": 0}      # repacks; forwards that ran as chains on several streams
        # callable(family, phase, flop, nbytes) around the hot launches (bench.py's live HIP-event roofline):
        # phase 0 before the launch with its algorithmic FLOPs / HBM bytes, phase 1 after it, same stream
        self.profile_hook = None
        # roctx ranges named by kernel family around the same launches (torch.cuda.nvtx is roctx on ROCm): visible in
        # `rocprofv3 --marker-trace` timelines.  Off by default (a host call per launch).
        self.trace_ranges = False
        # weight-gradient GEMMs on a side stream (an attribute for A/B runs and tests).  On by default since round 5:
        # interleaved A/B on one box, ViT-B/16 B=256: 31.53 vs 32.05 ms/step (profiles/r9g_concurrent_wgrad_ab.log;
        # in round 1, with slower kernels, it had measured 41.3 vs 40.5 ms and was left off)
        self.concurrent_wgrad = True
        # the forward's encoder blocks as two half-batch chains on two HIP streams (_forward_blocks_split): each fills
        # the other's idle CUs (partial last rounds of tiles, kernel drains); outputs bitwise those of one chain
        self.fwd_streams = 2
        self._fwd_pair = None
        # backward kernels share the CUs with RCCL collectives (set by enable_data_parallel on the nccl backend;
        # an attribute, so A/B runs can force either launch mode)
        self.shared_cus = False
        self._wstream = None
        # the last block's post-attention part on the B token-0 rows only (see forward); False: every row (tests)
        self.prune_last = True
        # ... and its attention on query 0 alone (vit_attn_fwd_row0 / vit_attn_bwd_row0); False: the full attention
        # kernels with the output gradient zero outside row 0 (A/B runs; set it between steps, not between a forward
        # and its backward)
        self.row0_attention = True
        # data-parallel replica index folded into the dropout seed (enable_data_parallel sets the group rank): every
        # rank draws the same base seed from its identically seeded CPU RNG, so without it all replicas would apply
        # the same keep masks to different images.  0 (rank 0, single process) leaves the seed unchanged.
        self.dropout_rank = 0
        # .grad views set at the end of backward() instead of its start when every grad was None (_attach_grads);
        # an attribute for A/B runs
        self.defer_grad_attach = True
        self._pending_views = None
        # left by backward() for run_param_hooks(): the gradients from before an accumulating backward with
        # `register_hook` hooks, and the frozen per-head views inside a QKV region that was rewritten
        self._acc_old = None
        self._frozen_keep = None

    # ------------------------------------------------------------------------------------------------------------
    # layout
    # ------------------------------------------------------------------------------------------------------------
    def _collect(self, model):
        """name -> Parameter for the fused layout, following the reference module tree."""
        enc = model.transformer_encoder.blocks
        emb = model.emdeddings
        p = {"conv_w": emb.sequence[0].weight, "conv_b": emb.sequence[0].bias,
             "cls": emb.cls_tkn_embd, "pos": emb.pos_embd,
             "h0_w": model.mlp[0].weight, "h0_b": model.mlp[0].bias,
             "hln_w": model.mlp[2].weight, "hln_b": model.mlp[2].bias,
             "h3_w": model.mlp[3].weight, "h3_b": model.mlp[3].bias}
        for l, blk in enumerate(enc):
            mh = blk.multi_head
            for h, head in enumerate(mh.heads):
                p[f"{l}.q{h}"] = head.query.weight
                p[f"{l}.k{h}"] = head.key.weight
                p[f"{l}.v{h}"] = head.value.weight
            p[f"{l}.proj_w"], p[f"{l}.proj_b"] = mh.proj.weight, mh.proj.bias
            p[f"{l}.fc1_w"], p[f"{l}.fc1_b"] = blk.ffwd.mlp[0].weight, blk.ffwd.mlp[0].bias
            p[f"{l}.fc2_w"], p[f"{l}.fc2_b"] = blk.ffwd.mlp[2].weight, blk.ffwd.mlp[2].bias
            p[f"{l}.ln1_w"], p[f"{l}.ln1_b"] = blk.ln1.weight, blk.ln1.bias
            p[f"{l}.ln2_w"], p[f"{l}.ln2_b"] = blk.ln2.weight, blk.ln2.bias
        return p

    def _expected_shape(self, name, nc, batch):
        """Shape the config gives parameter `name` of _collect (the head's width `nc` and the CLS parameter's batch
        rows are the module's own)."""
        D, hd = self.D, self.hd
        short = name.rpartition(".")[2]
        if short[:1] in ("q", "k", "v") and short[1:].isdigit():
            return (hd, D)
        if short in ("proj_b", "fc2_b", "ln1_w", "ln1_b", "ln2_w", "ln2_b", "conv_b"):
            return (D,)
        if short in ("fc1_b", "h0_b", "hln_w", "hln_b"):
            return (4 * D,)
        return {"conv_w": (D, self.C, self.P, self.P), "cls": (batch, 1, D), "pos": (1, self.T, D),
                "h0_w": (4 * D, D), "h3_w": (nc, 4 * D), "h3_b": (nc,), "proj_w": (D, D), "fc1_w": (4 * D, D),
                "fc2_w": (D, 4 * D)}[short]

    def _build(self, model, device):
        D, hd, L = self.D, self.hd, self.L
        params = self._collect(model)
        # the classifier's width follows the head the module holds now (`model.mlp[3] = nn.Linear(4 * D, nc)`, the
        # fine-tuning recipe); every other shape is fixed by the config, and the kernels trust it
        self.nc = nc = params["h3_w"].shape[0]
        for n, t in params.items():
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"parameter {n} must be contiguous float32 master weights (got {t.dtype})")
            if t.device != device:
                raise RuntimeError(f"parameter {n} is on {t.device}, expected {device}; call model.to(device)")
            if tuple(t.shape) != self._expected_shape(n, nc, t.shape[0]):
                raise RuntimeError(f"parameter {n} has shape {tuple(t.shape)}, but the config gives "
                                   f"{self._expected_shape(n, nc, t.shape[0])}")

        def shape(name):       # of a region: its parameter's, but for the fused QKV and the conv-as-GEMM matrices
            if name.endswith(".qkv_w"):
                return (3 * D, D)
            return (D, self.CPP) if name == "conv_w" else tuple(params[name].shape)

        # ---- gradient layout: head | blocks L-1..0 | embedding
        g = _Region()

        def grads(names):
            start = g.size
            for n in names:
                g.add(n, math.prod(shape(n)))
            return start, g.size

        self.head_range = grads(("h0_w", "h0_b", "hln_w", "hln_b", "h3_w", "h3_b"))
        self.block_range = {l: grads([f"{l}.{n}" for n in BLOCK_REGIONS]) for l in reversed(range(L))}
        self.embed_range = grads(("conv_w", "conv_b", "cls", "pos"))
        self.G = torch.zeros(g.size, dtype=torch.float32, device=device)
        # ---- compute shadow layout: the blocks' matrices, then the patch embedding's
        s = _Region()
        for name in [f"{l}.{n}" for l in range(L) for n in BLOCK_REGIONS] + ["conv_w"]:
            if len(shape(name)) == 2:
                s.add(name, math.prod(shape(name)))
        self.W = torch.empty(s.size, dtype=self.dtype, device=device)
        # fused compute/grad views
        self.gw = {n: self.G[o:o + k].view(shape(n)) for n, o, k in g.items}
        self.ww = {n: self.W[o:o + k].view(shape(n)) for n, o, k in s.items}

        # per-parameter grad view + shadow view (the optimizer refreshes the shadow in its kernel)
        self.grad_views = []
        self.grad_region = []           # gradient region (key of self.gw / self.owners) of each grad view
        self.owners = {}                # which parameters feed each region (a fused QKV region: 3H per-head ones)
        self.pack_entries = []
        me = weakref.ref(self)
        for name, p in params.items():
            key, rows = name, slice(None)
            l, _, short = name.partition(".")
            if short[:1] in ("q", "k", "v") and short[1:].isdigit():    # head `h`'s hd rows of the fused QKV region
                key = f"{l}.qkv_w"
                r0 = "qkv".index(short[0]) * D + int(short[1:]) * hd
                rows = slice(r0, r0 + hd)
            gv = self.gw[key][rows].view(p.shape)
            sv = self.ww[key][rows].view(p.shape) if key in self.ww else None
            self.grad_views.append((p, gv))
            self.grad_region.append(key)
            self.owners.setdefault(key, []).append(p)
            SHADOWS[p] = sv
            _ENGINE_OF[id(p)] = (weakref.ref(p, lambda _, k=id(p): _ENGINE_OF.pop(k, None)), me)
            if sv is not None:
                self.pack_entries.append((p, sv))
        self.params = params
        self.param_list = list(params.values())
        self.device = device
        self._pack_table = None
        self._ptr_sig = self._pointer_signature()
        self._ver_sig = None
        # the module tree as it stands: every (container dict, key, object) of a submodule or a parameter, for
        # _tree_changed()
        self._tree = [(d, k, o) for mod in model.modules() for d in (mod._modules, mod._parameters)
                      for k, o in d.items()]

    def _pointer_signature(self):
        return tuple(p.data_ptr() for p in self.param_list)

    def _version_signature(self):
        return sum(p._version for p in self.param_list)

    def _tree_changed(self):
        """Whether the module tree no longer holds the very objects captured at _build: a replaced submodule
        (`model.mlp[3] = nn.Linear(...)`), a replaced Parameter (`module.weight = nn.Parameter(...)`,
        `load_state_dict(assign=True)`).  Neither moves a captured parameter's storage or version, so the two
        signatures cannot see it.  One dict lookup and identity test per submodule and parameter, host only."""
        for d, k, o in self._tree:
            if d.get(k) is not o:
                return True
        return False

    def ensure_ready(self, device):
        model = self.model_ref()
        if model is None or getattr(model, "_engine", None) is not self:
            raise RuntimeError("this engine does not belong to the model it is called for (copied engine?); "
                               "models must build their own engine (VisionTransformer.hip_engine)")
        if (self.params is None or self.device != device or self._tree_changed()
                or self._pointer_signature() != self._ptr_sig):
            self._build(model, device)
        ver = self._version_signature()
        if ver != self._ver_sig:
            self.repack()
            self._ver_sig = ver

    def repack(self):
        """shadow <- compute-dtype copy of the fp32 master matrices (one multi-tensor launch).  Before the first
        forward there is no shadow yet and nothing to do: the first build packs."""
        if self.params is None:
            return
        if self._pack_table is None:
            entries = [(p.detach(), None, None, None, sv) for p, sv in self.pack_entries]
            self._pack_table = _ops.build_chunk_table(entries, self.device)
        tab, n = self._pack_table
        _ops.pack(tab, n, self.dtype)
        self.stats["packs"] += 1

    # ------------------------------------------------------------------------------------------------------------
    def _token_rows(self, name, M, D, dt, T, dev):
        """[M, D] buffer that is zero outside the token-0 rows b*T (the pruned last block's attention-backward operands):
        allocated zeroed once per shape; every use writes exactly rows b*T again, so the rest stays zero and no
        M x D fill runs per step."""
        key = (name, M, D, dt, T, dev)
        buf = self._tok.get(key) if self._tok is not None else None
        if buf is None:
            if self._tok is None:
                self._tok = {}
            buf = self._tok[key] = torch.zeros(M, D, dtype=dt, device=dev)
        return buf

    def _workspace(self, nbytes, side=False):
        """Grow-only fp32 scratch of >= nbytes: the main stream's, or (`side`) the weight-gradient stream's."""
        ws = self._ws[side]
        if ws is None or ws.numel() * 4 < nbytes:
            ws = self._ws[side] = torch.empty(max(nbytes // 4 + 1, 1 << 20), dtype=torch.float32, device=self.device)
        return ws

    def _split_ws(self, split, m, n, side=False):
        """The split-K slabs of an [m, n] GEMM: `split` fp32 copies of the output (None without a split)."""
        return self._workspace(split * m * n * 4, side) if split > 1 else None

    def _side_stream(self):
        """HIP stream for the weight-gradient GEMMs of the backward (None: run them in order on the current stream).
        A weight gradient depends only on tensors the current stream has already produced and nothing reads it
        before the bucket all-reduce / the optimizer step, so on its own stream it runs beside the dgrad / attention
        / LayerNorm chain and fills the CUs that chain leaves idle (partial last rounds of tiles, memory-bound
        kernels).  Same kernels, same inputs: the gradients are bitwise those of the in-order schedule."""
        if not self.concurrent_wgrad or self.device is None or self.device.type != "cuda":
            return None
        if self._wstream is None or self._wstream.device != self.device:
            self._wstream = torch.cuda.Stream(device=self.device)
        return self._wstream

    def _mark(self, fam, phase, flop=0.0, nbytes=0.0):
        h = self.profile_hook
        if h is not None:
            h(fam, phase, flop, nbytes)
        if self.trace_ranges:
            if phase == 0:
                torch.cuda.nvtx.range_push(fam)
            else:
                torch.cuda.nvtx.range_pop()

    def _wgrad(self, dy, x, out, m, n, k, ld_dy, ld_x, beta, side=None, fam=None, alpha=1.0):
        """out[m][n] (+)= alpha sum_r dy[r][i] x[r][j]: weight gradient, reduction over B*T rows, split-K.  With `side`
        it runs on that stream after everything already enqueued on the current one."""
        split = split_k_for(m, n, k, dy.dtype)
        ws = self._split_ws(split, m, n, side is not None)
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(self.device))
        elif fam:
            self._mark(fam, 0, 2.0 * m * n * k, (m + n) * k * dy.element_size() + m * n * 4 * (1 + (beta != 0)))
        _ops.gemm(dy, x, out, m, n, k, ld_dy, ld_x, out.stride(0), a_kcontig=False, b_kcontig=False, beta=beta,
                  alpha=alpha, split_k=split, workspace=ws, stream=side)
        if side is not None:
            for t in (dy, x) if ws is None else (dy, x, ws):
                t.record_stream(side)      # the caching allocator must not hand these out before `side` is done
        elif fam:
            self._mark(fam, 1)

    def _gemm_rows(self, pr, a, b, c, m, n, k, lda, ldb, ldc, **kw):
        """A token-row GEMM; `pr` (the pruned last block, m = B rows): split-K over the otherwise idle CUs — a few
        256x256 tiles would each run one long k-loop on one CU."""
        split = split_k_for(m, n, k, a.dtype) if pr else 1
        return _ops.gemm(a, b, c, m, n, k, lda, ldb, ldc, split_k=split, workspace=self._split_ws(split, m, n), **kw)

    def _head_gemm(self, a, b, c, m, n, k, lda, ldb, ldc, **kw):
        split = head_split_for(m, n, k)
        _ops.gemm(a, b, c, m, n, k, lda, ldb, ldc, split_k=split, workspace=self._split_ws(split, m, n), **kw)

    def _head_linear(self, x, w, bias):
        m, k = x.shape
        n = w.shape[0]
        y = torch.empty(m, n, dtype=x.dtype, device=x.device)
        self._head_gemm(x, w, y, m, n, k, x.stride(0), w.stride(0), n, bias=bias)
        return y

    def _attach_grads(self):
        """Expose the flat gradient buffer as param.grad of every parameter that requires grad (frozen ones keep
        .grad untouched, as autograd would); returns beta (1.0 accumulate / 0.0 overwrite)."""
        views = [(p, gv) for p, gv in self.grad_views if p.requires_grad]
        live = [p.grad is not None and p.grad.data_ptr() == gv.data_ptr() for p, gv in views]
        if all(live):
            return 1.0
        if not any(p.grad is not None for p, _ in views):
            if not self.defer_grad_attach:
                for p, gv in views:
                    p.grad = gv
                return 0.0
            # the common case after zero_grad(set_to_none=True): the ~0.3 ms of .grad setter calls is deferred to
            # the end of backward() (_attach_pending), after the head and block kernels are enqueued — host work off
            # the forward -> backward turn, where a profiled run (slower launches) left the GPU idle; nothing reads
            # the views before then (interleaved A/B without a profiler: within noise, profiles/r22_*)
            self._pending_views = views
            return 0.0
        # mixed: zero the regions whose grad was dropped/replaced, keep accumulating elsewhere
        for (p, gv), ok in zip(views, live):
            if not ok:
                if p.grad is not None:
                    gv.copy_(p.grad)
                else:
                    gv.zero_()
                p.grad = gv
        return 1.0

    def _attach_pending(self):
        views, self._pending_views = self._pending_views, None
        for p, gv in views or ():
            p.grad = gv

    # ------------------------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------------------------
    def forward(self, x, training, save, want_probs=False, keep_qkv=False, keep=None):
        """(logits, tape).  Patch dropout (a training forward with model.patch_drop_rate > 0, or `keep`: the caller's
        own table, int32 / int64 [B, K] on the device, ascending, column 0 equal to 0, checked for shape and dtype only):
        the embedding computes the kept patches alone and every block runs on T' = K + 1 tokens per image; the tape
        records T', K and the table, which is all the backward reads.
        `keep_qkv`: (logits, tape, qkvs) with every block's qkv [B*T, 3D], first block to last
        (rollout()'s input).  Such a forward runs as a probability-storing one does — one chain, every block's full
        QKV GEMM and full attention, the pruned block's too — so its logits are bitwise that forward's.
        keep_qkv="fast" differs in one thing: the attention is the kernel a plain forward runs (MFMA in bf16 at hd 64,
        5.6x faster end to end at ViT-B/16 B 256), so the logits and the later blocks' qkv are another valid bf16
        evaluation — a plain forward's kernels — and not the probability-storing forward's bits."""
        if not x.is_cuda:
            raise RuntimeError("VisionTransformer (HIP path) needs the input on a ROCm device; there is no CPU path")
        if x.dim() != 4 or x.shape[1] != self.C or x.shape[2] % self.P or x.shape[3] % self.P:
            raise RuntimeError(f"expected input [B, {self.C}, H, W] with H, W multiples of {self.P}, got "
                               f"{tuple(x.shape)}")
        B = x.shape[0]
        self.ensure_ready(x.device)
        if (x.shape[2] // self.P) * (x.shape[3] // self.P) != self.N:
            raise RuntimeError(f"image gives {(x.shape[2] // self.P) * (x.shape[3] // self.P)} patches but "
                               f"config.num_patches = {self.N} (pos_embd has {self.T} rows)")
        if B != self.params["cls"].shape[0]:
            # the reference concatenates a batch-shaped CLS parameter (vit.py:32,41) and fails the same way
            raise RuntimeError(f"batch size {B} != config.batch_size {self.params['cls'].shape[0]} "
                               "(the CLS token parameter is batch-shaped)")
        x = x.contiguous()
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        D, N, L, dt = self.D, self.N, self.L, self.dtype
        prm = self.params
        seed = dropout_seed(int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), self.dropout_rank) if training else 0
        tape = Tape() if save else None
        # Patch dropout: the table of this forward (idx [B, K]: the kept patches, ascending; inv [B, N]: a patch's row
        # or -1), drawn on the stream from the forward's seed with no host sync, or the caller's.  Without one (eval,
        # rate 0) T and K are the model's and every launch is the one it always was.
        rate = self.model_ref().patch_drop_rate if training else 0.0
        idx = inv = posg = None
        if keep is not None:
            if not training:
                raise ValueError("keep: patch dropout is training-only (the model is in eval mode)")
            if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.int32, torch.int64):
                raise TypeError("keep must be an int32 or int64 tensor")
            if keep.dim() != 2 or keep.shape[0] != B or not 1 <= keep.shape[1] <= N or keep.device != x.device:
                raise ValueError(f"keep must be [B, K] = [{B}, 1..{N}] on {x.device}, got {tuple(keep.shape)} on "
                                 f"{keep.device}")
            idx = keep.clamp(0, N - 1).to(torch.int32).contiguous()
            inv = torch.full((B, N), -1, dtype=torch.int32, device=x.device)
            inv.scatter_(1, idx.long(), torch.arange(idx.shape[1], dtype=torch.int32, device=x.device).expand(B, -1))
        elif rate > 0.0:
            idx, inv = _ops.patch_keep(seed, L, B, N, _config.patch_keep_count(N, rate), x.device)
        K = N if idx is None else idx.shape[1]
        T = K + 1
        if idx is not None:
            # the fp32 residual rows of the gathered embedding GEMM: pos of every kept patch (vit_gather_pos)
            posg = _ops.gather_pos(prm["pos"], idx, N)
        if training:
            self.model_ref().last_patch_keep = idx
        # Stochastic depth (model.drop_path_rates, training only): one launch fills the per-row factor table of every
        # (block, site) — 1 / (1 - p_l) on the rows of the images that keep the branch, 0 on the others — which the
        # proj / fc2 GEMMs of the blocks with p_l > 0 apply in their epilogue (vit_gemm_rowscale).  All rates 0: no
        # table, and every launch is the one it always was.
        rates = [float(p) for p in self.model_ref().drop_path_rates] if training else []
        path = _ops.drop_path_rows(seed, rates, B, T, x.device) if any(rates) else None
        # block l's [2, B*T] slice of the table, None where its rate is 0
        paths = [path[l] if path is not None and rates[l] > 0.0 else None for l in range(L)]

        blocks = []
        # The classifier reads token 0 of the last block's output only (vit.py:80), and everything after the last
        # attention is per token: the last block's proj / LN2 / MLP (and their backward) run on the B token-0 rows
        # (rows b*T, row stride T*D; dropout bits drawn at the full tensor's indices) — the same logits, loss and
        # gradients as computing all B*T rows and discarding the rest.  `prune_last = False` computes every row.
        prune = self.prune_last
        nc = self.fwd_streams
        cols = torch.empty(B * K, self.CPP, dtype=dt, device=x.device)
        xcur = torch.empty(B * T, D, dtype=dt, device=x.device)
        qkvs = []
        if (nc > 1 and not want_probs and not keep_qkv and self.profile_hook is None and B % (4 * nc) == 0
                and ((B // nc) * T) % 4 == 0):
            self.stats["split_forwards"] += 1
            xcur = self._forward_blocks_split(x, cols, xcur, B, training, seed, save, prune, blocks, nc,
                                              paths=paths, T=T, idx=idx, posg=posg)
        else:
            self._embed(x, cols, xcur, 0, B, idx, posg)
            for l in range(L):
                xcur, saved = self.block_forward(l, xcur, B, training, seed, save, want_probs,
                                                 pr=prune and l == L - 1, path_scale=paths[l], keep_qkv=keep_qkv,
                                                 T=T)
                if keep_qkv:
                    qkvs.append(saved.qkv)
                if save:
                    blocks.append(saved)
        # classifier on token 0 (= first PATCH, vit.py:80): Linear -> GELU(erf) -> LayerNorm(4D) -> Linear, fp32
        z = torch.empty(B, D, dtype=torch.float32, device=x.device)
        _ops.copy2d(xcur, D if prune else T * D, z, D, B, D)
        u = self._head_linear(z, prm["h0_w"], prm["h0_b"])
        gz = _ops.gelu_fwd(u)
        zn, mh, rh = _ops.layernorm_fwd(gz, prm["hln_w"], prm["hln_b"], eps=LN_EPS)
        logits = self._head_linear(zn, prm["h3_w"], prm["h3_b"])
        if save:
            tape.B, tape.cols, tape.blocks = B, cols, blocks
            tape.x_shape, tape.x_dtype = tuple(x.shape), x.dtype
            tape.z, tape.u, tape.gz, tape.zn, tape.mh, tape.rh = z, u, gz, zn, mh, rh
            tape.seed, tape.training, tape.pruned = seed, training, prune
            # which attention the pruned block's forward ran (query 0 alone, or the full kernels): its backward must
            # be the matching one whatever row0_attention says by then (the row-0 forward writes only rows b*T)
            tape.row0 = prune and self.row0_attention and not want_probs and not keep_qkv
            # ... and the drop-path rates its keep bits were drawn with: the backward's scalars follow the forward,
            # whatever model.drop_path_rates says by then
            tape.path_rates = rates if path is not None else None
            # ... and the token count and keep table of this forward (patch dropout; idx / inv None without one)
            tape.T, tape.K, tape.idx, tape.inv = T, K, idx, inv
        return (logits, tape, qkvs) if keep_qkv else (logits, tape)

    def _block_bufs(self, x_in, B, training, save, pr=False, q0only=False, T=None):
        """Every tensor the forward of one block writes for the B images of x_in: (BlockActs, x_out).  The only place
        that says which exist and how large they are.  `pr` (the pruned last block): the post-attention tensors and
        masks on the B token-0 rows; `q0only`: its attention runs on query 0 alone (no fp32 O).  The masks exist only
        where a backward will read them: hm (ReLU) on a saving forward, pm / fm (dropout keep bits) on a saving
        training one; o32 where the attention backward at this shape takes it.  `T`: tokens per image of this forward
        (None: the model's N + 1)."""
        D, H, hd, dt = self.D, self.H, self.hd, self.dtype
        T = self.T if T is None else T
        M = B * T
        R = B if pr else M
        dev = x_in.device
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)   # noqa: E731
        f32 = torch.float32
        acts = BlockActs(
            x_in=x_in, a1=e(M, D), m1=e(M, dtype=f32), r1=e(M, dtype=f32), qkv=e(M, 3 * D), o=e(M, D),
            o32=e(M, D, dtype=f32) if save and not q0only and _ops.attn_bwd_uses_o32(B, T, H, hd, dt) else None,
            lse=e(B, H, T, dtype=f32), x_mid=e(R, D), a2=e(R, D), m2=e(R, dtype=f32), r2=e(R, dtype=f32),
            h=e(R, 4 * D), hm=_ops.mask4_empty(R, 4 * D, dev) if save else None,
            pm=_ops.mask4_empty(R, D, dev) if save and training else None,
            fm=_ops.mask4_empty(R, D, dev) if save and training else None)
        return acts, e(R, D)

    def _embed(self, x, cols, xcur, b0, B, idx=None, posg=None):
        """Patch embedding (vit.py:21-29, 39-42) of images b0 .. b0+B-1 into their rows of the whole-batch cols /
        xcur: im2col, the conv as a GEMM with conv bias + pos and the (b, n) -> b*T + n row remap in its epilogue,
        then the CLS rows (appended LAST, vit.py:41).  `idx` (patch dropout, the whole batch's [B, K] table, with
        `posg` = pos of every kept patch): only the kept patches are read and embedded — the same GEMM epilogue with
        the gathered rows as its residual, hence the same single rounding of acc + bias + pos, into T' = K + 1 rows per
        image; the CLS rows still carry pos[N]."""
        D, T, N, dt = self.D, self.T, self.N, self.dtype
        es = 2 if dt == torch.bfloat16 else 4
        prm = self.params
        if idx is not None:
            K = idx.shape[1]
            cl = cols[b0 * K:(b0 + B) * K]
            xc = xcur[b0 * (K + 1):(b0 + B) * (K + 1)]
            _ops.im2col_gather(x[b0:b0 + B], self.P, dt, idx[b0:b0 + B], cols=cl)
            self._mark("gemm_fwd", 0, 2.0 * B * K * D * self.CPP, (B * K + D) * self.CPP * es + B * K * D * (es + 4))
            _ops.gemm(cl, self.ww["conv_w"], xc, B * K, D, self.CPP, self.CPP, self.CPP, D, bias=prm["conv_b"],
                      res=posg[b0 * K:(b0 + B) * K], ldres=D, res_rowmod=B * K, out_group=(K, K + 1))
            self._mark("gemm_fwd", 1)
            # vit_embed_cls adds row T' - 1 of the table it is given: handed pos from row N - K on, that is pos[N]
            _ops.embed_cls(prm["cls"].reshape(-1, D)[b0:b0 + B], prm["pos"].view(T, D)[N - K:], xc, B, K + 1, D)
            return
        cl = cols[b0 * N:(b0 + B) * N]
        xc = xcur[b0 * T:(b0 + B) * T]
        _ops.im2col(x[b0:b0 + B], self.P, dt, cols=cl)                                # vit.py:21-29 as GEMM
        self._mark("gemm_fwd", 0, 2.0 * B * N * D * self.CPP, (B * N + D) * self.CPP * es + B * N * D * es)
        _ops.gemm(cl, self.ww["conv_w"], xc, B * N, D, self.CPP, self.CPP, self.CPP, D, bias=prm["conv_b"],
                  res=prm["pos"].view(T, D), ldres=D, res_rowmod=N, out_group=(N, T))  # + pos, rows -> b*T+n
        self._mark("gemm_fwd", 1)
        _ops.embed_cls(prm["cls"].reshape(-1, D)[b0:b0 + B], prm["pos"], xc, B, T, D)  # CLS appended LAST

    def _forward_blocks_split(self, x, cols, xcur, B, training, seed, save, prune, blocks, nc=2, *, paths=None,
                              T=None, idx=None, posg=None):
        """The patch embedding and the encoder blocks as nc chains of B/nc images on nc HIP streams (default two),
        into the whole-batch cols / xcur allocated on the current stream, up to the last block's output, which the
        current stream then waits for.  Every kernel is the one-chain forward's on a row range (rows are
        independent; dropout indices are the whole batch's), so the outputs are bitwise the same; the chains fill
        each other's idle CUs.  The blocks' outputs are whole-batch buffers allocated on the current stream and
        recorded on every chain stream.  `paths`: per block, its slice of the drop-path factor table (forward) or
        None; a chain's GEMMs read the whole batch's slice at their rows.  `T`: tokens per image of this forward (None:
        the model's); `idx` / `posg` (patch dropout): the whole batch's keep table and gathered pos rows, of which
        each chain's embedding takes its images'."""
        paths = paths if paths is not None else [None] * self.L
        T, L = self.T if T is None else T, self.L
        dev = xcur.device
        cur = torch.cuda.current_stream(dev)
        if self._fwd_pair is None or len(self._fwd_pair) != nc or self._fwd_pair[0].device != dev:
            self._fwd_pair = tuple(torch.cuda.Stream(device=dev) for _ in range(nc))
        streams = self._fwd_pair
        for st in streams:
            st.wait_stream(cur)
        Bh, Mh = B // nc, (B // nc) * T

        def on_chains(tensors):
            for t in tensors:
                if t is not None:
                    for st in streams:
                        t.record_stream(st)

        on_chains((x, cols, xcur, idx, posg, *paths))         # (views of one table: each records its storage)
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                self._embed(x, cols, xcur, i * Bh, Bh, idx, posg)
        # the ring attention forward of one chain on 3/4 of the CUs, so the other chain's GEMMs run beside it instead
        # of waiting for the whole latency-bound kernel (one box, interleaved: 30.50 -> 30.19 ms/step; 1/2 and 7/8 of
        # the CUs gain less) — unless the caller set the attn_fwd_grid option itself.  Passed per call (vit_attn_fwd's
        # max_wgs, ABI 14): no process-wide state changes, so concurrent forwards on other threads are unaffected.
        wgs = 0
        if _lib.get_option("attn_fwd_grid") == 0:
            wgs = max(1, torch.cuda.get_device_properties(dev).multi_processor_count * 3 // 4)
        # the pruned last block runs whole-batch after the join: split, its B token-0 rows would become two GEMMs of
        # B/2 rows (below the 256-row tile: the slow small-M kernels)
        nsplit = L - 1 if prune else L
        # without a tape (no_grad / eval) nothing outlives the next block: two buffer sets, ping-ponged.  Each chain
        # reads and writes only its own rows, in order on its own stream, so block l + 2 may overwrite block l's rows
        # of a chain once that chain's block l + 1 consumed them (fresh sets per block, each recorded on
        # both streams, let the caching allocator hold up to L blocks of activations while the host runs ahead)
        ping = None if save else [self._block_bufs(xcur, B, training, save, T=T) for _ in range(2)]
        for acts, x_out in ping or ():
            on_chains((*acts, x_out))
        for l in range(nsplit):
            if save:
                acts, x_out = self._block_bufs(xcur, B, training, save, T=T)
                on_chains((*acts, x_out))
            else:
                acts, x_out = ping[l % 2]
                acts = acts._replace(x_in=xcur)
            for i, st in enumerate(streams):
                with torch.cuda.stream(st):
                    part = acts.images(i * Bh, Bh, T)
                    self.block_forward(l, part.x_in, Bh, training, seed, save, out=(part, x_out[i * Mh:(i + 1) * Mh]),
                                       row0=i * Mh, attn_wgs=wgs, path_scale=paths[l], T=T)
            if save:
                blocks.append(acts)
            xcur = x_out
        if nsplit < L:
            q0only = self.row0_attention
            acts, x_out = self._block_bufs(xcur, B, training, save, True, q0only, T)
            whole = (acts.x_in, acts.a1, acts.m1, acts.r1, acts.qkv)
            if q0only:
                # the pruned block's ln1 and K / V GEMM are whole-row work: per chain too
                on_chains(whole)
                for i, st in enumerate(streams):
                    with torch.cuda.stream(st):
                        self._ln1_qkv(L - 1, *(t[i * Mh:(i + 1) * Mh] for t in whole), True)
        for st in streams:
            cur.wait_stream(st)
        if nsplit < L:
            if not q0only:
                self._ln1_qkv(L - 1, *whole, False)
            xcur = self._attend_ffn(L - 1, acts, x_out, B, training, seed, save, False, True, q0only,
                                    path_scale=paths[L - 1], T=T)
            if save:
                blocks.append(acts)
        return xcur

    def block_forward(self, l, x_in, B, training, seed, save, want_probs=False, *, pr=False, out=None, row0=0,
                      attn_wgs=0, path_scale=None, keep_qkv=False, T=None):
        """Block l (transformer.py:76-79) on x_in [B*T, D] (compute dtype): x_mid = x_in + drop(MHA(ln1(x_in))),
        x_out = x_mid + drop(FFN(ln2(x_mid))).  `pr`: the post-attention part on the B token-0 rows only (the pruned
        last block).  Returns (x_out, saved): `saved` is the BlockActs block_backward needs (None unless `save`).
        `out` (the two-stream forward, _forward_blocks_split): the (BlockActs, x_out) to write into instead of fresh
        ones — a row range (BlockActs.images) of the whole batch's, x_in being its row `row0`: the dropout bits are
        drawn at the whole batch's indices.  `path_scale` (drop path): this block's [2, rows] slice of the whole
        batch's factor table (_ops.drop_path_rows), site 0 for the attention branch and 1 for the FFN's, read at the
        dropout's row indices; None: no drop path.  `keep_qkv` (forward): the block as a probability-storing forward
        runs it, and `saved` is returned without `save` too.  `T`: tokens per image of x_in (None: the model's N + 1;
        under patch dropout the forward's K + 1)."""
        # the pruned block's attention on query 0 alone
        q0only = pr and self.row0_attention and not want_probs and not keep_qkv
        a, x_out = out if out is not None else self._block_bufs(x_in, B, training, save, pr, q0only, T)
        self._ln1_qkv(l, a.x_in, a.a1, a.m1, a.r1, a.qkv, q0only)
        self._attend_ffn(l, a, x_out, B, training, seed, save, want_probs, pr, q0only, row0, attn_wgs,
                         path_scale=path_scale, keep_qkv=keep_qkv, T=T)
        return x_out, a if save or keep_qkv else None

    def _ln1_qkv(self, l, x_in, a1, m1, r1, qkv, kv_only):
        """The part of block l before its attention that is whole-row work: a1 = ln1(x_in), then qkv = a1 Wqkv^T —
        `kv_only` (the pruned block with the query-0 attention): its K / V columns D..3D only; _attend_ffn adds Q of
        the token-0 rows, the only Q rows that attention reads."""
        D = self.D
        M = x_in.shape[0]
        es = 2 if self.dtype == torch.bfloat16 else 4
        mk = self._mark
        wq = self.ww[f"{l}.qkv_w"]
        mk("ln_fwd", 0, 0.0, 2 * M * D * es + 8 * M)
        _ops.layernorm_fwd(x_in, self.params[f"{l}.ln1_w"], self.params[f"{l}.ln1_b"], eps=LN_EPS, y=a1, mean=m1,
                           rstd=r1)
        mk("ln_fwd", 1)
        if kv_only:
            mk("gemm_fwd", 0, 2.0 * M * 2 * D * D, (M * D + 2 * D * D + 2 * M * D) * es)
            _ops.gemm(a1, wq[D:], qkv[:, D:], M, 2 * D, D, D, D, 3 * D)
        else:
            mk("gemm_fwd", 0, 2.0 * M * 3 * D * D, (M * D + 3 * D * D + 3 * M * D) * es)
            _ops.gemm(a1, wq, qkv, M, 3 * D, D, D, D, 3 * D)
        mk("gemm_fwd", 1)

    def _attn_fwd_as_stored(self, a, B):
        """keep_qkv's attention: the kernel of a probability-storing forward, hence that forward's bits in a.o,
        without its [B, H, T, T] tensor.  vit_attn_fwd chooses by `probs` between the MFMA and the probability-writing
        kernel where both exist (bf16 at hd 64); there the images go through a few at a time — (image, head) items are
        independent, so the bits are the whole batch's — with their probabilities in one scratch of at most
        PROBS_SCRATCH_BYTES.  Everywhere else the one kernel there is runs, with no probabilities at all."""
        T, H, hd = self.T, self.H, self.hd
        if not (self.dtype == torch.bfloat16 and hd == 64):
            _ops.attn_fwd(a.qkv, B, T, H, hd, self.scale, o=a.o, lse=a.lse, o32=a.o32)
            return
        n = max(1, min(B, PROBS_SCRATCH_BYTES // (H * T * T * 4)))
        scratch = torch.empty(n, H, T, T, dtype=torch.float32, device=a.qkv.device)
        for b0 in range(0, B, n):
            nb = min(n, B - b0)
            rows = slice(b0 * T, (b0 + nb) * T)
            _ops.attn_fwd(a.qkv[rows], nb, T, H, hd, self.scale, o=a.o[rows], lse=a.lse[b0:b0 + nb], probs=scratch,
                          o32=None if a.o32 is None else a.o32[rows])

    def rollout(self, qkvs, token=0, fuse="mean", trace=False):
        """Attention rollout of `token` from a keep_qkv forward's qkvs: [B, T] fp32 — row `token` of A_L ... A_1 with
        A_l = the head-fused attention of block l plus the identity, rows re-normalised (vit_hip.h "Attention
        rollout").  One vit_attn_rollout_step per block, last block first, on the current stream with no host sync;
        two [B, T] vectors alternate over one workspace.  `trace`: also [L, B, T], entry l the vector after block
        l's step (entry 0 is the map)."""
        T, H, hd, L = self.T, self.H, self.hd, self.L
        if len(qkvs) != L:
            raise ValueError(f"rollout: {len(qkvs)} qkv tensors for {L} blocks")
        if not 0 <= int(token) < T:
            raise ValueError(f"rollout: token {token} outside [0, {T})")
        if fuse not in _ops.ROLLOUT_FUSE:
            raise ValueError(f"rollout: head fusion {fuse!r} is not one of {sorted(_ops.ROLLOUT_FUSE)}")
        code = _ops.ROLLOUT_FUSE[fuse]
        dev = qkvs[0].device
        B = qkvs[0].shape[0] // T
        need = _ops.attn_rollout_workspace_bytes(B, T, H, hd, qkvs[0].dtype, code)
        ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
        steps = torch.empty(L, B, T, dtype=torch.float32, device=dev) if trace else None
        pair = [torch.zeros(B, T, dtype=torch.float32, device=dev), torch.empty(B, T, dtype=torch.float32, device=dev)]
        pair[0][:, int(token)] = 1.0
        r = pair[0]
        for l in range(L - 1, -1, -1):
            out = steps[l] if trace else pair[1] if r is pair[0] else pair[0]
            r = _ops.attn_rollout_step(qkvs[l], r, B, T, H, hd, self.scale, code, r_out=out, workspace=ws)
        return (r, steps) if trace else r

    def _attend_ffn(self, l, a, x_out, B, training, seed, save, want_probs, pr, q0only, row0=0, attn_wgs=0, *,
                    path_scale=None, keep_qkv=False, T=None):
        """The rest of block l's forward from _ln1_qkv's a.a1 / a.qkv: attention, proj + residual, ln2, FFN +
        residual into x_out (arguments as block_forward's); returns x_out."""
        D, H, hd, dt = self.D, self.H, self.hd, self.dtype
        T = self.T if T is None else T
        M = B * T
        es = 2 if dt == torch.bfloat16 else 4
        prm = self.params
        mk = self._mark
        drop_p = DROPOUT_P if training else 0.0
        blk = self.model_ref().transformer_encoder.blocks[l]
        probs = None
        if want_probs:
            probs = torch.empty(B, H, T, T, dtype=torch.float32, device=x_out.device)
        if q0only:
            # ... which reads Q of the token-0 rows only (split-K over the idle CUs); the other Q rows of qkv are
            # never read
            mk("gemm_fwd", 0, 2.0 * B * D * D, (2 * B * D + D * D) * es)
            self._gemm_rows(True, a.a1, self.ww[f"{l}.qkv_w"], a.qkv, B, D, D, T * D, D, T * 3 * D)
            mk("gemm_fwd", 1)
            # the pruned last block: only attention output row 0 of every image is read (the classifier reads token 0,
            # everything after the attention is per token), and every softmax row is independent -> query 0 alone,
            # O(T hd) per (image, head); o rows b*T and lse[:, :, 0] are written
            mk("attn_fwd", 0, 4.0 * B * H * T * hd, 2 * M * D * es + 2 * B * D * es + 4 * B * H)
            _ops.attn_fwd_row0(a.qkv, B, T, H, hd, self.scale, o=a.o, lse=a.lse)
            mk("attn_fwd", 1)
        elif keep_qkv and keep_qkv != "fast" and not want_probs:
            self._attn_fwd_as_stored(a, B)
        else:
            # a.o32 (training forward in bf16 with the tiled T > 256 backward): also keep O unrounded for its exact
            # delta; the fused T <= 256 backward forms delta from P and dP itself (vit_hip.h)
            mk("attn_fwd", 0, 4.0 * B * H * T * T * hd, 4 * M * D * es + 4 * B * H * T + (4 * M * D if a.o32 is not None
                                                                                         else 0))
            _ops.attn_fwd(a.qkv, B, T, H, hd, self.scale, o=a.o, lse=a.lse, probs=probs, o32=a.o32, max_wgs=attn_wgs)
            mk("attn_fwd", 1)
        blk.multi_head.attention_probs = probs
        blk.multi_head._probs_skipped = probs is None       # a later read warns once (transformer.py)
        # rows of the post-attention part: all M, or (last block, pruned) the B token-0 rows b*T
        R, rs = (B, T) if pr else (M, 1)
        mk("gemm_fwd", 0, 2.0 * R * D * D, (3 * R * D + D * D) * es)
        self._gemm_rows(pr, a.o, self.ww[f"{l}.proj_w"], a.x_mid, R, D, D, rs * D, D, D, bias=prm[f"{l}.proj_b"],
                        res=a.x_in, ldres=rs * D, dropout_p=drop_p, seed=site_seed(seed, l, 0),
                        drop_row_stride=rs, mask_out=a.pm, drop_row0=row0,
                        row_scale=None if path_scale is None else path_scale[0])
        mk("gemm_fwd", 1)
        mk("ln_fwd", 0, 0.0, 2 * R * D * es + 8 * R)
        _ops.layernorm_fwd(a.x_mid, prm[f"{l}.ln2_w"], prm[f"{l}.ln2_b"], eps=LN_EPS, y=a.a2, mean=a.m2, rstd=a.r2)
        mk("ln_fwd", 1)
        # a.hm, saved for the backward: the ReLU mask as 1 bit per element (mask4, read by fc2's dgrad epilogue
        # instead of re-reading h: 1/16 of the bytes)
        mk("gemm_fwd", 0, 2.0 * R * 4 * D * D, (R * D + 4 * D * D + 4 * R * D) * es + (R * D // 2 if save else 0))
        self._gemm_rows(pr, a.a2, self.ww[f"{l}.fc1_w"], a.h, R, 4 * D, D, D, D, 4 * D, bias=prm[f"{l}.fc1_b"],
                        act=ACT_RELU, mask_out=a.hm)
        mk("gemm_fwd", 1)
        mk("gemm_fwd", 0, 2.0 * R * 4 * D * D, (4 * R * D + 4 * D * D + 2 * R * D) * es)
        self._gemm_rows(pr, a.h, self.ww[f"{l}.fc2_w"], x_out, R, D, 4 * D, 4 * D, 4 * D, D, bias=prm[f"{l}.fc2_b"],
                        res=a.x_mid, ldres=D, dropout_p=drop_p, seed=site_seed(seed, l, 1), drop_row_stride=rs,
                        mask_out=a.fm, drop_row0=row0, row_scale=None if path_scale is None else path_scale[1])
        mk("gemm_fwd", 1)
        return x_out

    # ------------------------------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------------------------------
    def _bucket_ready(self, rng, side=None):
        """Launch the all-reduce of one contiguous gradient range (RCCL stream waits on the compute stream, and on
        the weight-gradient stream `side` when there is one).  With comm_dtype bf16 the range is first rounded into
        a bf16 buffer (on the stream that produced it), which is what travels and is averaged."""
        if not self.ddp_enabled:
            return
        a, b = rng
        bf = self.comm_dtype == torch.bfloat16
        # RCCL: native average, issued from `side` when there is one (the main chain does not wait).  gloo (CPU tests):
        # from the current stream, after `side`; a sum, scaled after the wait.
        nccl = dist.get_backend(self.ddp_group) == "nccl"
        issue_on = contextlib.nullcontext()
        if side is not None:
            cur = torch.cuda.current_stream(self.device)
            if nccl:
                side.wait_stream(cur)
                issue_on = torch.cuda.stream(side)
            else:
                cur.wait_stream(side)
        with issue_on:
            buf = self.G[a:b].to(torch.bfloat16) if bf else self.G[a:b]
            w = dist.all_reduce(buf, op=dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM, group=self.ddp_group,
                                async_op=True)
        self._works.append((w, rng, buf if bf else None, not nccl))

    def _finish_buckets(self):
        if not self._works:
            return
        world = dist.get_world_size(self.ddp_group) if self.ddp_enabled else 1
        ev = None
        if self.time_comm and self.device is not None and self.device.type == "cuda":
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()                      # every backward kernel is enqueued before this point
        for w, (a, b), buf, scale in self._works:
            w.wait()                            # nccl: the current stream waits for the collective
            if buf is not None:
                self.G[a:b].copy_(buf)          # bf16 average -> fp32 gradients
                if buf.is_cuda:                 # may have been allocated on the weight-gradient stream
                    buf.record_stream(torch.cuda.current_stream(buf.device))
            if scale:
                self.G[a:b].mul_(1.0 / world)
        if ev is not None:
            ev[1].record()
        self._comm_events = ev
        self._works = []

    def comm_exposed_ms(self):
        """Milliseconds the compute stream spent, after the last backward kernel, waiting for the gradient
        all-reduce of the most recent backward with time_comm set (None if not measured).  Synchronizes."""
        if self._comm_events is None:
            return None
        self._comm_events[1].synchronize()
        return self._comm_events[0].elapsed_time(self._comm_events[1])

    def backward(self, tape, dlogits):
        D, L, dt = self.D, self.L, self.dtype
        # tokens per image and patches kept of the forward being differentiated: the tape's, never the model's
        T, K = tape.T, tape.K
        B = tape.B
        M = B * T
        prm, gw = self.params, self.gw
        # decided at backward time: the reference calls zero_grad(set_to_none=True) between forward and backward
        self._pending_views = None
        beta = self._attach_grads()
        # Accumulating into existing .grad (no zero_grad between backwards) with `register_hook` hooks present:
        # autograd applies such a hook to THIS backward's gradient only, then accumulates.  Keep the old gradients
        # aside, let the kernels overwrite the buffer with the increment (beta 0), and let run_param_hooks() hook
        # the increment and add the old values back (old + increment is the same single fp32 rounding the beta=1
        # epilogues do, so hook-free parameters keep their bits).
        self._acc_old = None
        if beta == 1.0 and any(p.requires_grad and p._backward_hooks for p, _ in self.grad_views):
            self._acc_old = self.G.clone()
            beta = 0.0
        req = {k: any(p.requires_grad for p in ps) for k, ps in self.owners.items()}
        # a frozen per-head parameter whose .grad is still a view of G shares the fused QKV gradient region with the
        # heads that do train; that region is rewritten as a whole, so keep the frozen view's value aside (autograd
        # leaves a frozen parameter's .grad untouched).  Only such views: a region whose owners are all frozen is
        # never written.
        self._frozen_keep = [] if self._acc_old is not None else [
            (gv, gv.clone()) for (p, gv), key in zip(self.grad_views, self.grad_region)
            if not p.requires_grad and req[key] and p.grad is not None and p.grad.data_ptr() == gv.data_ptr()]
        # the backward stops at the first block below which nothing (parameters, input image) needs a gradient
        below = tape.x_grad or any(req[k] for k in ("conv_w", "conv_b", "cls", "pos"))
        need_from = {}
        for l in range(L):
            below = below or any(req[f"{l}.{n}"] for n in BLOCK_REGIONS)
            need_from[l] = below
        dev = dlogits.device
        dlogits = dlogits.contiguous().float()
        nc = self.nc
        side = self._side_stream()
        # ---- head (fp32)
        dzn = torch.empty(B, 4 * D, dtype=torch.float32, device=dev)
        self._head_gemm(dlogits, prm["h3_w"], dzn, B, 4 * D, nc, nc, 4 * D, 4 * D, b_kcontig=False)
        if req["h3_w"]:
            self._wgrad(dlogits, tape.zn, gw["h3_w"], nc, 4 * D, B, nc, 4 * D, beta, side)
        if req["h3_b"]:
            _ops.colsum(dlogits, B, nc, nc, gw["h3_b"], beta=beta)
        dgz = torch.empty_like(tape.gz)
        part = _ops.layernorm_bwd(dzn, tape.gz, prm["hln_w"], tape.mh, tape.rh, dgz)
        _ops.colsum(part[0], part.shape[1], 4 * D, 4 * D, gw["hln_w"], beta=beta)
        _ops.colsum(part[1], part.shape[1], 4 * D, 4 * D, gw["hln_b"], beta=beta)
        du = _ops.gelu_bwd(tape.u, dgz)
        dz = torch.empty(B, D, dtype=torch.float32, device=dev)
        self._head_gemm(du, prm["h0_w"], dz, B, D, 4 * D, 4 * D, D, D, b_kcontig=False)
        if req["h0_w"]:
            self._wgrad(du, tape.z, gw["h0_w"], 4 * D, D, B, 4 * D, D, beta, side)
        if req["h0_b"]:
            _ops.colsum(du, B, 4 * D, 4 * D, gw["h0_b"], beta=beta)
        self._bucket_ready(self.head_range, side)
        if not need_from[L - 1]:
            if side is not None:
                torch.cuda.current_stream(dev).wait_stream(side)      # the head's weight gradients are in G
            self._finish_buckets()
            self._attach_pending()
            return None
        # ---- d(encoder output): only token-0 rows are nonzero.  Pruned (see forward): the last block's FFN / proj
        # backward runs on those B rows; otherwise on all M rows, zero outside them.
        pruned = tape.pruned
        R0 = B if pruned else M
        dx = (torch.empty if pruned else torch.zeros)(R0, D, dtype=dt, device=dev)
        _ops.copy2d(dz, D, dx, D if pruned else T * D, B, D)
        # Dropout backward as a bare mask (exact in bf16); its 1/(1-p) goes into every consumer of the masked gradient
        # (GEMM alpha, column-sum alpha, the LN kernels' bias-gradient sums) instead of a rounding of its own.  The
        # keep bits are the ones the forward's GEMM epilogues saved (mask4), not a re-hash (block_backward).
        if tape.training:
            g1 = _ops.mask4_apply(dx, torch.empty_like(dx), tape.blocks[L - 1].fm, 1.0)
        else:
            g1 = dx
        g1_summed = False          # block L-1's fc2 bias gradient: g1 comes from the head (plain column sum below)
        # drop path: the saved keep bits already hold "element kept and the image's branch kept", so the backward
        # differs only in the scalar 1 / ((1 - p_drop)(1 - p_l)) of each block, from the forward's own rates
        rates = tape.path_rates or [0.0] * L
        for l in reversed(range(L)):
            if not need_from[l]:
                break
            prev_mask = tape.blocks[l - 1].fm if (tape.training and l > 0) else None
            dx, g1n = self.block_backward(l, tape.blocks[l], dx, g1, g1_summed, beta, req, side, tape.training, B,
                                          pruned and l == L - 1, chain_prev=l > 0, prev_mask=prev_mask,
                                          row0=tape.row0 and l == L - 1, path_rate=rates[l],
                                          prev_path_rate=rates[l - 1] if l > 0 else 0.0, T=T)
            g1_summed = l > 0
            self._bucket_ready(self.block_range[l], side)
            g1 = g1n if g1n is not None else dx
        dimg = None
        if need_from[0]:
            # ---- embedding (vit.py:39-42): dx = d(x0) [B*T, D]; K = T - 1 patch rows per image — all N patches, or
            # under patch dropout the kept ones (tape.idx / tape.inv), whose gradients are scattered back
            if req["cls"]:
                _ops.copy2d(dx[K:], T * D, gw["cls"].view(B, D), D, B, D, beta=beta)       # CLS row of every image
            if req["pos"]:
                if tape.inv is None:
                    _ops.colsum(dx, B, T * D, T * D, gw["pos"].view(-1), beta=beta)        # pos: sum over the batch
                else:                         # ... over the images that kept the position (vit_pos_grad_gather)
                    _ops.pos_grad_gather(dx, tape.inv, K, gw["pos"], beta=beta)
            dpatch = torch.empty(B * K, D, dtype=dt, device=dev)
            _ops.copy2d(dx, D, dpatch, D, B * K, D, group=(K, T))
            if req["conv_b"]:
                _ops.colsum(dpatch, B * K, D, D, gw["conv_b"], beta=beta)
            if req["conv_w"]:
                self._wgrad(dpatch, tape.cols, gw["conv_w"], D, self.CPP, B * K, D, self.CPP, beta, side,
                            "gemm_wgrad")
            if tape.x_grad:                   # input-image gradient: conv dgrad = dpatch W, scattered back (col2im)
                dcols = torch.empty(B * K, self.CPP, dtype=dt, device=dev)
                _ops.gemm(dpatch, self.ww["conv_w"], dcols, B * K, self.CPP, D, D, self.CPP, self.CPP,
                          b_kcontig=False)
                dimg = torch.empty(tape.x_shape, dtype=tape.x_dtype, device=dev)
                if tape.inv is None:
                    _ops.col2im(dcols, dimg, self.P)
                else:                         # zeros under the dropped patches (vit_col2im_scatter)
                    _ops.col2im_scatter(dcols, tape.inv, K, dimg, self.P)
        self._bucket_ready(self.embed_range, side)
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)      # every weight gradient is in G before the step
        self._finish_buckets()
        self._attach_pending()
        return dimg

    def block_backward(self, l, acts, dx, g1, g1_summed, beta, req, side, training, B, pr=False, chain_prev=False,
                       prev_mask=None, row0=None, *, path_rate=0.0, prev_path_rate=0.0, T=None):
        """Backward of block l (`acts`: its forward's BlockActs) from d(x_out) = dx and g1 = the fc2-dropout-masked dx
        (dx itself in eval).  Writes the block's weight gradients into the flat buffer (beta: 0 overwrite / 1
        accumulate; req: which regions want a gradient) and returns (dx_in, g1n).  `chain_prev`: there is a block l-1
        below, so the ln1 backward also emits block l-1's fc2 bias-gradient column sums and — in training, from its
        keep bits `prev_mask` — g1n, the next block's masked gradient (None otherwise).  `g1_summed`: this block's fc2
        bias gradient was already summed by the block above.  `pr`: the pruned last block (dx / g1 are its B token-0
        rows).  `row0`: its forward ran the query-0 attention (Tape.row0; None: pr and self.row0_attention, for
        direct callers).  `path_rate` / `prev_path_rate`: the drop-path rates the forward of this block / of block
        l-1 ran with (Tape.path_rates): they enter only the 1 / keep-probability scalars of the masked gradients'
        consumers, the masks themselves being the forward's combined keep bits."""
        if row0 is None:
            row0 = pr and self.row0_attention
        D, H, hd, dt = self.D, self.H, self.hd, self.dtype
        T = self.T if T is None else T               # tokens per image of the forward (Tape.T under patch dropout)
        M = B * T
        gw = self.gw
        prm = self.params
        es = 2 if dt == torch.bfloat16 else 4
        mk = self._mark
        dev = dx.device
        drop_p, gs = _keep_scale(path_rate) if training else (DROPOUT_P, 1.0)
        prev_drop_p = _keep_scale(prev_path_rate)[0] if training else DROPOUT_P
        R, rs = (B, T) if pr else (M, 1)
        # FFN: x_out = x_mid + drop(relu(ln2(x_mid) W1^T + b1) W2^T + b2)
        if req[f"{l}.fc2_w"]:
            self._wgrad(g1, acts.h, gw[f"{l}.fc2_w"], D, 4 * D, R, D, 4 * D, beta, side, "gemm_wgrad", alpha=gs)
        if not g1_summed:
            _ops.colsum(g1, R, D, D, gw[f"{l}.fc2_b"], beta=beta, alpha=gs)
        dh = torch.empty(R, 4 * D, dtype=dt, device=dev)
        dh_part = torch.empty(_ops.colsum_part_rows(R), 4 * D, dtype=torch.float32, device=dev)
        # relu backward and the fc1 bias-gradient column sums fused into the dgrad epilogue
        mk("gemm_dgrad", 0, 2.0 * R * 4 * D * D, (R * D + 4 * D * D + 4 * R * D) * es + R * D // 2)
        self._gemm_rows(pr, g1, self.ww[f"{l}.fc2_w"], dh, R, 4 * D, D, D, 4 * D, 4 * D, b_kcontig=False, aux=acts.hm,
                        colsum_part=dh_part, alpha=gs, shared_cus=self.shared_cus)
        mk("gemm_dgrad", 1)
        cs_jobs = [(dh_part, [gw[f"{l}.fc1_b"]], beta)]      # this block's bias / LN-affine sums: one launch below
        if req[f"{l}.fc1_w"]:
            self._wgrad(dh, acts.a2, gw[f"{l}.fc1_w"], 4 * D, D, R, 4 * D, D, beta, side, "gemm_wgrad")
        da2 = torch.empty(R, D, dtype=dt, device=dev)
        mk("gemm_dgrad", 0, 2.0 * R * 4 * D * D, (4 * R * D + 4 * D * D + R * D) * es)
        self._gemm_rows(pr, dh, self.ww[f"{l}.fc1_w"], da2, R, D, 4 * D, 4 * D, D, D, b_kcontig=False,
                        shared_cus=self.shared_cus)
        mk("gemm_dgrad", 1)
        dx_mid = torch.empty(R, D, dtype=dt, device=dev)
        g0 = torch.empty(R, D, dtype=dt, device=dev) if training else None
        # ln2 backward + residual add + dropout backward of the MHA branch; its third partial set is the column
        # sums of g0 as stored = the proj bias gradient
        mk("ln_bwd", 0, 0.0, (3 + 1 + (g0 is not None)) * R * D * es + 8 * R + R * D // 8)
        part = _ops.layernorm_bwd(da2, acts.x_mid, prm[f"{l}.ln2_w"], acts.m2, acts.r2, dx_mid, dres=dx, drop_out=g0,
                                  drop_p=drop_p, drop_mask=acts.pm, osum=True)
        mk("ln_bwd", 1)
        cs_jobs.append((part, [gw[f"{l}.ln2_w"], gw[f"{l}.ln2_b"], gw[f"{l}.proj_b"]], beta))
        if g0 is None:
            g0 = dx_mid
        # MHA: x_mid = x_in + drop(attn(ln1(x_in)) Wp^T + bp)
        if req[f"{l}.proj_w"]:
            self._wgrad(g0, acts.o, gw[f"{l}.proj_w"], D, D, R, D, rs * D, beta, side, "gemm_wgrad", alpha=gs)
        do = torch.empty(R, D, dtype=dt, device=dev)
        mk("gemm_dgrad", 0, 2.0 * R * D * D, (2 * R * D + D * D) * es)
        self._gemm_rows(pr, g0, self.ww[f"{l}.proj_w"], do, R, D, D, D, D, D, b_kcontig=False, alpha=gs,
                        shared_cus=self.shared_cus)
        mk("gemm_dgrad", 1)
        if pr:
            # the ln1 backward's residual gradient on all M rows (zero outside the token-0 rows)
            dxm_full = self._token_rows("dxm", M, D, dt, T, dev)
            _ops.copy2d(dx_mid, D, dxm_full, T * D, B, D)
            dx_mid = dxm_full
        if row0:
            # attention backward from the row-0 output gradients alone (the forward computed row 0 only): dQ row 0, all
            # of dK / dV; the dQ rows 1..T-1 of this buffer are never written, so they stay zero for the dgrad /
            # wgrad GEMMs below
            dqkv = self._token_rows("dqkv", M, 3 * D, dt, T, dev)
            mk("attn_bwd", 0, 10.0 * B * H * T * hd, 4 * M * D * es + 4 * B * D * es + 4 * B * H)
            _ops.attn_bwd_row0(acts.qkv, do, D, dqkv, B, T, H, hd, self.scale)
            mk("attn_bwd", 1)
        else:
            if pr:
                # back to all M rows for the full attention backward (zero outside the token-0 rows)
                do_full = self._token_rows("do", M, D, dt, T, dev)
                _ops.copy2d(do, D, do_full, T * D, B, D)
                do = do_full
            if acts.o32 is None and _ops.attn_bwd_uses_o32(B, T, H, hd, dt):
                # the forward chose the fused backward (no fp32 O kept) and a library option changed since: the tiled
                # backward would form delta from the bf16 O, inexact under saturated softmax
                raise RuntimeError("attention backward needs the fp32 O that this forward did not keep: the "
                                   "attn_bwd_split library option changed between forward and backward")
            # bytes: qkv, dO, dqkv (+ O and o32 for the tiled backward's delta pass)
            mk("attn_bwd", 0, 10.0 * B * H * T * T * hd,
               7 * M * D * es + 4 * B * H * T + (M * D * es + 4 * M * D if acts.o32 is not None else 0))
            dqkv = _ops.attn_bwd(acts.qkv, acts.o, do, acts.lse, B, T, H, hd, self.scale,
                                 workspace=self._workspace(_ops.attn_bwd_workspace_bytes(B, T, H, hd, dt)),
                                 o32=acts.o32, shared_cus=self.shared_cus)
            mk("attn_bwd", 1)
        wq = self.ww[f"{l}.qkv_w"]
        da1 = torch.empty(M, D, dtype=dt, device=dev)
        if row0:
            # dQ is zero outside the token-0 rows: the K / V part over every row, the Q part over the B token-0 rows
            # (weight gradient: its own K = B GEMM; input gradient: added onto those rows of da1 by the residual
            # epilogue, in place)
            if req[f"{l}.qkv_w"]:
                gq = gw[f"{l}.qkv_w"]
                self._wgrad(dqkv[:, D:], acts.a1, gq[D:], 2 * D, D, M, 3 * D, D, beta, side, "gemm_wgrad")
                self._wgrad(dqkv, acts.a1, gq[:D], D, D, B, T * 3 * D, T * D, beta, side, "gemm_wgrad")
            mk("gemm_dgrad", 0, 2.0 * M * 2 * D * D, (2 * M * D + 2 * D * D + M * D) * es)
            _ops.gemm(dqkv[:, D:], wq[D:], da1, M, D, 2 * D, 3 * D, D, D, b_kcontig=False, shared_cus=self.shared_cus)
            mk("gemm_dgrad", 1)
            mk("gemm_dgrad", 0, 2.0 * B * D * D, (3 * B * D + D * D) * es)
            self._gemm_rows(True, dqkv, wq, da1, B, D, D, T * 3 * D, D, T * D, b_kcontig=False, res=da1,
                            ldres=T * D, shared_cus=self.shared_cus)
            mk("gemm_dgrad", 1)
        else:
            if req[f"{l}.qkv_w"]:
                self._wgrad(dqkv, acts.a1, gw[f"{l}.qkv_w"], 3 * D, D, M, 3 * D, D, beta, side, "gemm_wgrad")
            mk("gemm_dgrad", 0, 2.0 * M * 3 * D * D, (3 * M * D + 3 * D * D + M * D) * es)
            _ops.gemm(dqkv, wq, da1, M, D, 3 * D, 3 * D, D, D, b_kcontig=False, shared_cus=self.shared_cus)
            mk("gemm_dgrad", 1)
        dx_in = torch.empty(M, D, dtype=dt, device=dev)
        g1n = torch.empty(M, D, dtype=dt, device=dev) if (training and chain_prev) else None
        # ln1 backward; for l > 0 its third partial set is the column sums of the next g1 (g1n, or dx_in in eval)
        # = the fc2 bias gradient of block l-1
        mk("ln_bwd", 0, 0.0, (3 + 1 + (g1n is not None)) * M * D * es + 8 * M)
        part = _ops.layernorm_bwd(da1, acts.x_in, prm[f"{l}.ln1_w"], acts.m1, acts.r1, dx_in, dres=dx_mid, drop_out=g1n,
                                  drop_p=prev_drop_p, drop_mask=prev_mask if g1n is not None else None,
                                  osum=chain_prev)
        mk("ln_bwd", 1)
        outs = [gw[f"{l}.ln1_w"], gw[f"{l}.ln1_b"]] + ([gw[f"{l - 1}.fc2_b"]] if chain_prev else [])
        cs_jobs.append((part, outs, beta))
        if side is not None:
            # the partial sums are finished beside the dgrad chain too: only the bucket / optimizer read the results
            side.wait_stream(torch.cuda.current_stream(self.device))
            _ops.colsum_finish_batch(cs_jobs, stream=side)
            for job in cs_jobs:
                job[0].record_stream(side)
        else:
            _ops.colsum_finish_batch(cs_jobs)
        return dx_in, g1n

    def run_param_hooks(self):
        """Parameter hooks after the fused backward (autograd's AccumulateGrad never runs for these parameters):
        `register_hook` hooks see this backward's gradient and may replace it, then
        `register_post_accumulate_grad_hook` hooks run on the parameter — each once per backward, in registration
        order.  When the backward accumulated into existing gradients, the buffer holds the increment here
        (backward() set `_acc_old`): the hooks see the increment, then the previous gradients are added back."""
        old, self._acc_old = self._acc_old, None
        for gv, keep in self._frozen_keep or ():
            gv.copy_(keep)
        self._frozen_keep = None
        for p, gv in self.grad_views:
            if not p.requires_grad or p.grad is None:
                continue
            pre = p._backward_hooks
            if pre:
                g = p.grad
                for fn in pre.values():
                    r = fn(g)
                    if r is not None:
                        g = r
                if g is not p.grad:
                    p.grad.copy_(g)
        if old is not None:
            # the previous gradients go back under the views of the parameters this backward produced a gradient
            # for; every other view (frozen meanwhile, or in a region no kernel rewrote) gets its old value back,
            # never old + old
            for p, gv in self.grad_views:
                ov = torch.as_strided(old, gv.shape, gv.stride(), gv.storage_offset())
                if p.requires_grad and p.grad is not None and p.grad.data_ptr() == gv.data_ptr():
                    gv.add_(ov)
                else:
                    gv.copy_(ov)
        for p, gv in self.grad_views:
            if not p.requires_grad or p.grad is None:
                continue
            post = getattr(p, "_post_accumulate_grad_hooks", None)
            if post:
                for fn in post.values():
                    fn(p)


class ViTFunction(torch.autograd.Function):
    """One autograd node for the whole network; gradients land in the engine's flat buffer (param.grad views)."""

    @staticmethod
    def forward(ctx, x, anchor, engine, training, want_probs, keep=None):
        logits, tape = engine.forward(x, training, save=True, want_probs=want_probs, keep=keep)
        tape.x_grad = ctx.needs_input_grad[0]
        ctx.engine = engine
        ctx.tape = tape
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.tape is None:
            raise RuntimeError("VisionTransformer backward called twice on the same forward")
        dimg = ctx.engine.backward(ctx.tape, dlogits)
        ctx.tape = None
        ctx.engine.run_param_hooks()
        return dimg, None, None, None, None, None
