"""Every way of changing a model's weights reaches the fused engine (the layer between the nn.Module and the kernels).

The engine caches the compute-dtype shadow of the matrices, the dict of captured `Parameter` objects it reads every
bias / LayerNorm weight / `cls` / `pos` / head matrix from, and the flat gradient buffer behind `param.grad`.  A
forward trusts that state after `ensure_ready()`'s host-side checks; were one of them broken, training would run on
stale weights and nothing else in the suite would notice.

One reference for every case: a FRESHLY CONSTRUCTED model loaded from the mutated model's `state_dict()` — a new
engine, a new pack from the fp32 masters — run on the same input under the same `torch.manual_seed`.  Both sides run
the same kernels on the same bytes, so logits, loss, every named parameter's gradient and (in train mode) block 0's
dropout keep bits are compared with `torch.equal`: no tolerance.

Shape of a case: build A; one training forward + backward (the engine exists and can be stale);
`zero_grad(set_to_none=True)`; the mutation; F built from `A.vit_config` and `A.state_dict()`; run both; compare.
Each mutation runs as a training step and as a `no_grad` eval forward, at the smallest configs that reach every cached
thing: D=128 / H=2 / hd=64 (MFMA attention) in bf16 and fp32, and D=64 / H=4 / hd=16 (four per-head row views per
fused QKV matrix, generic attention) in bf16; T=17, two blocks (one full, one pruned), B=8 (the smallest batch the
two-chain forward takes).

tests/test_engine_coherence_cpu.py checks the rebuild / repack decision itself on a machine with no GPU.
"""
import pytest
import torch
import torch.nn as nn

from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import config, vit
    from VisionTransformer.optim import FusedAdamW, cross_entropy

DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32


def _hd64_cfg(img=64, batch=8, blocks=2):        # as tests/test_gpu_dropin.py's helper
    ocfg = O.make_config("micro", img=img, batch=batch, blocks=blocks)
    ocfg.embedding_size, ocfg.num_heads = 128, 2
    return ocfg


CONFIGS = {"hd64-bf16": (_hd64_cfg, BF16), "hd64-fp32": (_hd64_cfg, FP32),
           "hd16-bf16": (lambda: O.make_config("micro", img=64, batch=8, blocks=2), BF16)}
_cache = {}


def _setup(name):
    """(oracle config, dtype, init state, x, y) of a config: computed once, shared, never written."""
    if name not in _cache:
        make, dtype = CONFIGS[name]
        ocfg = make()
        x, y = O.synthetic_batch(ocfg)
        _cache[name] = (ocfg, dtype, O.init_state(ocfg, seed=21), x.to(DEV), y.to(DEV))
    return _cache[name]


def _build(name, state=None):
    ocfg, dtype, st, _, _ = _setup(name)
    c = config.ViTConfig(ocfg.input_channels, ocfg.num_classes, ocfg.num_patches, ocfg.embedding_size,
                         ocfg.patch_size, ocfg.num_heads, ocfg.num_blocks, "cpu", ocfg.batch_size, precision=dtype)
    m = vit.VisionTransformer(c)
    m.load_state_dict(st if state is None else state)
    return m.to(DEV)


def _warm(name):
    """Steps 1-3: A with an engine that has run a training step, gradients dropped."""
    A = _build(name)
    _, _, _, x, y = _setup(name)
    A.train()
    torch.manual_seed(1)
    cross_entropy(A(x), y).backward()
    A.zero_grad(set_to_none=True)
    return A, x, y


def _fresh(A):
    """The reference F: a new model from A's config as it stands, loaded from A's state_dict, frozen where A is."""
    F = vit.VisionTransformer(A.vit_config)
    F.load_state_dict(A.state_dict())
    F = F.to(DEV)
    for (k, p), (kf, q) in zip(A.named_parameters(), F.named_parameters()):
        assert k == kf
        q.requires_grad_(p.requires_grad)
    return F


def _labels(m, y):
    return y % m.vit_config.num_classes


def _run(m, x, y, train, seed=2):
    """One step of m: logits, loss and — training — block 0's proj-dropout keep bits and every gradient."""
    torch.manual_seed(seed)
    out = {}
    if not train:
        m.eval()
        with torch.no_grad():
            out["logits"] = m(x)
            out["loss"] = cross_entropy(out["logits"], _labels(m, y))
        return out
    m.train()
    logits = m(x)
    out["pm"] = logits.grad_fn.tape.blocks[0].pm.clone()
    out["logits"] = logits.detach()
    loss = cross_entropy(logits, _labels(m, y))
    loss.backward()
    out["loss"] = loss.detach()
    out["grads"] = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    return out


def _same(ra, rf):
    assert ra["logits"].shape == rf["logits"].shape
    assert torch.equal(ra["logits"], rf["logits"]), "logits"
    assert torch.equal(ra["loss"], rf["loss"]), "loss"
    if "pm" in rf:
        assert torch.equal(ra["pm"], rf["pm"]), "block 0 keep bits"
        assert sorted(ra["grads"]) == sorted(rf["grads"])
        assert rf["grads"], "the reference produced no gradient"
        bad = [k for k, g in rf["grads"].items() if not torch.equal(ra["grads"][k], g)]
        assert not bad, bad


def _compare(A, x, y, train, seed=2):
    F = _fresh(A)
    ra, rf = _run(A, x, y, train, seed), _run(F, x, y, train, seed)
    _same(ra, rf)
    return F, ra


def _other_state(A, seed=33):
    g = torch.Generator().manual_seed(seed)
    return {k: (0.05 * torch.randn(v.shape, generator=g)).to(v.device) for k, v in A.state_dict().items()}


def _blk(m, l):
    return m.transformer_encoder.blocks[l]


def _train_step(A, x, y, seed):
    A.train()
    torch.manual_seed(seed)
    cross_entropy(A(x), _labels(A, y)).backward()


# ----------------------------------------------------------------------------------------------------------------
# the mutations: name -> (function(A, x, y), what the engine must have done by the end of the next forward)
#   "repack":  the same buffers, stats["packs"] up by exactly one
#   "rebuild": a new gradient buffer, every eng.params[name] the module's current parameter
#   None:      either (only the result is checked)
# ----------------------------------------------------------------------------------------------------------------
MUTATIONS = {}


def mutation(kind):
    def deco(fn):
        MUTATIONS[fn.__name__] = (fn, kind)
        return fn
    return deco


# ---- a. no_grad in-place
@mutation("repack")
def a_mul_every_parameter(A, x, y):
    with torch.no_grad():
        for p in A.parameters():
            p.mul_(1.25)


@mutation("repack")
def a_trunc_normal_through_apply(A, x, y):
    torch.manual_seed(40)

    def init(mod):
        if isinstance(mod, nn.Linear):
            nn.init.trunc_normal_(mod.weight, std=0.05)
    A.apply(init)


@mutation("repack")
def a_copy_through_state_dict(A, x, y):
    sd = A.state_dict()
    for k, v in _other_state(A).items():
        sd[k].copy_(v)


# ---- b. load_state_dict
@mutation("repack")
def b_load_state_dict(A, x, y):
    A.load_state_dict(_other_state(A))


@mutation("rebuild")
def b_load_state_dict_assign(A, x, y):
    A.load_state_dict(_other_state(A), assign=True)


# ---- c. re-pointed storage
def _repoint(p, s):
    p.data = p.data.clone() * s


@mutation("rebuild")
def c_repoint_head_query(A, x, y):
    _repoint(_blk(A, 0).multi_head.heads[1].query.weight, 1.5)


@mutation("rebuild")
def c_repoint_fc1(A, x, y):
    _repoint(_blk(A, 1).ffwd.mlp[0].weight, 0.5)


@mutation("rebuild")
def c_repoint_bias(A, x, y):
    _repoint(_blk(A, 0).multi_head.proj.bias, -2.0)


@mutation("rebuild")
def c_repoint_pos(A, x, y):
    _repoint(A.emdeddings.pos_embd, 0.75)


@mutation("rebuild")
def c_vector_to_parameters(A, x, y):
    from torch.nn.utils import parameters_to_vector, vector_to_parameters
    vector_to_parameters(parameters_to_vector(A.parameters()) * 0.8, A.parameters())


# ---- d. replaced objects
def _new_head(A, nc, seed=41):
    torch.manual_seed(seed)
    A.mlp[3] = nn.Linear(4 * A.vit_config.embedding_size, nc).to(DEV)


@mutation("rebuild")
def d_new_head_same_classes(A, x, y):
    _new_head(A, A.vit_config.num_classes)


@mutation("rebuild")
def d_new_head_7_classes(A, x, y):
    _new_head(A, 7)
    assert A.vit_config.num_classes == 7


@mutation("rebuild")
def d_new_query_linear(A, x, y):
    c = A.vit_config
    torch.manual_seed(42)
    _blk(A, 0).multi_head.heads[1].query = nn.Linear(c.embedding_size, c.embedding_size // c.num_heads,
                                                     bias=False).to(DEV)


@mutation("rebuild")
def d_new_ln2_weight_parameter(A, x, y):
    torch.manual_seed(43)
    _blk(A, 1).ln2.weight = nn.Parameter(1.0 + 0.1 * torch.randn(A.vit_config.embedding_size, device=DEV))


@mutation("rebuild")
def d_finetune_frozen_body_new_head(A, x, y):
    A.requires_grad_(False)
    _new_head(A, A.vit_config.num_classes)


# ---- e. torch optimizers on an engine model, from a real backward's gradients
def _torch_opt_step(A, x, y, make):
    _train_step(A, x, y, seed=3)
    opt = make(A.parameters())
    opt.step()
    A.zero_grad(set_to_none=True)


@mutation("repack")
def e_sgd(A, x, y):
    _torch_opt_step(A, x, y, lambda ps: torch.optim.SGD(ps, lr=0.1))


@mutation("repack")
def e_adamw_foreach(A, x, y):
    _torch_opt_step(A, x, y, lambda ps: torch.optim.AdamW(ps, lr=1e-2, foreach=True))


@mutation("repack")
def e_adamw_fused(A, x, y):
    try:
        opt = torch.optim.AdamW(list(A.parameters()), lr=1e-2, fused=True)
    except RuntimeError as e:
        pytest.skip(f"this torch build refuses AdamW(fused=True) on this device: {e}")
    _torch_opt_step(A, x, y, lambda ps: opt)


# ---- f. FusedAdamW: the kernel-written shadows are exactly what a pack produces (no pack follows a fused step)
def _fused_steps(A, x, y, n=3, between=None, **kw):
    opt = FusedAdamW(A.parameters(), lr=1e-2, weight_decay=1e-2, **kw)
    for i in range(n):
        opt.zero_grad(set_to_none=True)
        _train_step(A, x, y, seed=10 + i)
        opt.step()
        if between is not None and i < n - 1:
            between()
    opt.zero_grad(set_to_none=True)


@mutation(None)
def f_fused_adamw_3_steps(A, x, y):
    _fused_steps(A, x, y)


@mutation(None)
def f_fused_adamw_clipped(A, x, y):
    _fused_steps(A, x, y, max_grad_norm=1.0)


@mutation(None)
def f_fused_adamw_frozen_matrix_written(A, x, y):
    w = _blk(A, 0).ffwd.mlp[2].weight
    w.requires_grad_(False)

    def write():
        with torch.no_grad():
            w.mul_(1.1)
    _fused_steps(A, x, y, between=write)


# ---- g. device round trip with a host-path forward in between
@mutation(None)
def g_cpu_forward_and_back(A, x, y):
    A.cpu()
    with torch.no_grad():
        A(x.cpu())
    A.to(DEV)


# ---- i. the documented p.data contract
@mutation("repack")
def i_data_write_then_repack(A, x, y):
    for p in A.parameters():
        p.data.mul_(0.9)
    A.hip_engine.repack()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_forward_after_mutation_equals_fresh_model(cfg, name, train):
    mutate, kind = MUTATIONS[name]
    A, x, y = _warm(cfg)
    eng = A.hip_engine
    G0, packs0 = eng.G, eng.stats["packs"]
    assert packs0 == 1
    mutate(A, x, y)
    if name.startswith("e_"):
        packs0 = eng.stats["packs"]          # the mutation's own training forward packed nothing new
        assert packs0 == 1
    _compare(A, x, y, train)
    assert A.hip_engine is eng
    if kind == "repack":
        assert eng.G is G0 and eng.stats["packs"] == packs0 + 1
    elif kind == "rebuild":
        assert eng.G is not G0
        current = eng._collect(A)
        assert all(eng.params[k] is p for k, p in current.items()) and len(current) == len(eng.params)
        assert {id(p) for p in A.parameters()} == {id(p) for p in eng.param_list}
        assert eng.stats["packs"] == packs0 + 1


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_finetune_new_head_trains_like_fresh_model(cfg):
    """The fine-tuning recipe: freeze everything, put a new head on, train it.  Only the head gets a gradient, it
    is F's under the same freezing, and one FusedAdamW(filter(requires_grad)) step moves A and F identically (the
    optimizer's cached tables follow the new gradient views)."""
    A, x, y = _warm(cfg)
    A.requires_grad_(False)
    _new_head(A, 7)
    F, ra = _compare(A, x, y, True)
    assert sorted(ra["grads"]) == ["mlp.3.bias", "mlp.3.weight"]
    assert ra["logits"].shape == (x.shape[0], 7)
    assert all(p.grad is None for k, p in A.named_parameters() if not k.startswith("mlp.3."))
    opts = [FusedAdamW(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-2) for m in (A, F)]
    for step in range(2):
        if step:
            for m, opt in zip((A, F), opts):
                opt.zero_grad(set_to_none=True)
            _same(_run(A, x, y, True, 5), _run(F, x, y, True, 5))
        for opt in opts:
            opt.step()
        sa, sf = A.state_dict(), F.state_dict()
        assert all(torch.equal(sa[k], sf[k]) for k in sf)
    assert not torch.equal(A.mlp[3].weight.grad, torch.zeros_like(A.mlp[3].weight))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_ema_of_a_fused_adamw_model(cfg):
    """h. AveragedModel(model) updated twice from a model FusedAdamW is stepping, then ema.module evaluated under
    no_grad.  Its engine has run before the first update, so it is stale by then.

    A limit, found with this test and documented in vit.py: on the device, every update after the first is torch's
    `_foreach_lerp_` kernel, which (torch 2.10) bumps no version counter, so an engine that ran BETWEEN two updates
    cannot see the later one from the host (measured at hd64-fp32: version sum 42 -> 42 across the second update,
    logits off by up to 1.9 until a pack).  As with `p.data` writes the contract is `repack()`; the last part checks
    that it holds, not that the un-repacked forward is stale."""
    from torch.optim.swa_utils import AveragedModel
    A, x, y = _warm(cfg)
    ema = AveragedModel(A)
    E = ema.module
    assert E.hip_engine is not A.hip_engine
    opt = FusedAdamW(A.parameters(), lr=1e-2, weight_decay=1e-2)

    def step_and_update(seed):
        opt.zero_grad(set_to_none=True)
        _train_step(A, x, y, seed=seed)
        opt.step()
        ema.update_parameters(A)

    _run(E, x, y, False)
    assert E.hip_engine.stats["packs"] == 1
    step_and_update(20)
    step_and_update(21)
    _compare(E, x, y, False)
    assert E.hip_engine.stats["packs"] == 2
    assert not torch.equal(E.mlp[3].weight, A.mlp[3].weight)         # a running mean by now, not a copy
    step_and_update(22)
    E.hip_engine.repack()
    _compare(E, x, y, False)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_repack_before_the_first_forward(cfg, train):
    """i. `p.data` writes then `repack()` on a model whose engine has never run: nothing to repack yet (the first
    build packs), and it must not raise."""
    A = _build(cfg)
    _, _, _, x, y = _setup(cfg)
    for p in A.parameters():
        p.data.mul_(0.9)
    A.hip_engine.repack()
    assert A.hip_engine.stats["packs"] == 0
    _compare(A, x, y, train)
    assert A.hip_engine.stats["packs"] == 1


@pytest.mark.parametrize("what", ["repointed_bias", "new_head", "both"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_rebuild_between_two_accumulating_backwards(cfg, what):
    """j. backward; re-point one bias and / or replace mlp[3]; a second backward without zero_grad.  Every untouched
    parameter's gradient is that of F running the same two backwards on the same two states (the accumulated
    gradient survives the rebuild); the new head's is the second backward's alone (its .grad was None)."""
    A = _build(cfg)
    _, _, _, x, y = _setup(cfg)
    s1 = {k: v.clone() for k, v in A.state_dict().items()}
    _train_step(A, x, y, seed=6)
    G0 = A.hip_engine.G
    if what != "new_head":
        _repoint(_blk(A, 0).multi_head.proj.bias, -2.0)
    if what != "repointed_bias":
        _new_head(A, A.vit_config.num_classes)
    s2 = {k: v.clone() for k, v in A.state_dict().items()}
    ra = _run(A, x, y, True, seed=7)
    assert A.hip_engine.G is not G0
    F = _build(cfg, s1)
    _train_step(F, x, y, seed=6)
    F.load_state_dict(s2)
    rf = _run(F, x, y, True, seed=7)
    second = _run(_build(cfg, s2), x, y, True, seed=7)
    assert torch.equal(ra["logits"], rf["logits"]) and torch.equal(ra["loss"], rf["loss"])
    assert torch.equal(ra["pm"], rf["pm"])
    assert sorted(ra["grads"]) == sorted(rf["grads"])
    for k, g in ra["grads"].items():
        ref = second["grads"][k] if k.startswith("mlp.3.") and what != "repointed_bias" else rf["grads"][k]
        assert torch.equal(g, ref), k
    k = "transformer_encoder.blocks.1.ffwd.mlp.0.weight"
    assert not torch.equal(ra["grads"][k], second["grads"][k])       # it did accumulate


# ---- pack-count invariants: what stops the hot path from silently repacking every step -----------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_no_pack_across_fused_adamw_steps(cfg):
    A, x, y = _warm(cfg)
    eng = A.hip_engine
    G0, W0 = eng.G, eng.W
    _fused_steps(A, x, y, n=5)
    assert eng.stats["packs"] == 1 and eng.G is G0 and eng.W is W0
    _compare(A, x, y, False)
    assert eng.stats["packs"] == 1


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_no_pack_between_consecutive_forwards(cfg):
    A, x, y = _warm(cfg)
    eng = A.hip_engine
    G0 = eng.G
    _run(A, x, y, False)
    _run(A, x, y, True)
    _run(A, x, y, True)                       # accumulating into live gradient views
    assert eng.stats["packs"] == 1 and eng.G is G0
