"""What `Engine.ensure_ready()` decides after each way of changing a model's weights, on the CPU (no kernel runs: the
engine's buffers are built on the host and `repack` is replaced by a counter).

The engine caches a compute-dtype shadow of the matrices, the dict of captured `Parameter` objects its forward reads
every bias / LayerNorm weight / head matrix from, and the flat gradient buffer.  After a weight change the next
`ensure_ready()` must do one of two things:

  * REPACK — the captured objects and their storage are still the module's, their values changed (an in-place write
    that autograd versions): exactly one `repack()`, no rebuild;
  * REBUILD — storage was re-pointed or an object was replaced: new buffers around the module tree's current
    parameters (`eng.G` is a new tensor, every `eng.params[name]` is the module's own), followed by the one pack of a
    fresh build.

tests/test_gpu_weight_coherence.py checks on the device that the forward after each of these computes what a freshly
built model computes.
"""
import pytest
import torch
import torch.nn as nn

from VisionTransformer import _engine, config, vit

CPU = torch.device("cpu")
D, H, NC = 64, 4, 10


def _model(seed=0):
    torch.manual_seed(seed)
    return vit.VisionTransformer(config.ViTConfig(3, NC, 4, D, 16, H, 2, "cpu", 4))


def _settle(m, monkeypatch):
    """(model, engine, packs): m's engine built on the host and settled (its first pack done), `repack` counted."""
    eng = m.hip_engine
    packs = []
    monkeypatch.setattr(eng, "repack", lambda: packs.append(1))
    eng._build(m, CPU)
    eng.ensure_ready(CPU)
    assert packs == [1]
    packs.clear()
    return m, eng, packs


@pytest.fixture
def built(monkeypatch):
    return _settle(_model(), monkeypatch)


def _assert_repacked(m, eng, packs, G0):
    eng.ensure_ready(CPU)
    assert eng.G is G0, "rebuilt, where one repack was enough"
    assert packs == [1]
    eng.ensure_ready(CPU)                    # settled: nothing more without a further change
    assert packs == [1] and eng.G is G0


def _assert_rebuilt(m, eng, packs, G0):
    eng.ensure_ready(CPU)
    assert eng.G is not G0, "the engine kept its old buffers"
    current = eng._collect(m)
    assert list(eng.params) == list(current)
    for name, p in current.items():
        assert eng.params[name] is p, name
    assert [p for p, _ in eng.grad_views] == list(current.values()) == eng.param_list
    for (p, gv), key in zip(eng.grad_views, eng.grad_region):
        assert gv.shape == p.shape and any(o is p for o in eng.owners[key])
        sv = _engine.shadow_of(p)
        if key in eng.ww:                    # the shadow of the CURRENT object is a view of the NEW buffer
            lo, hi = eng.W.data_ptr(), eng.W.data_ptr() + eng.W.numel() * eng.W.element_size()
            assert sv.shape == p.shape and lo <= sv.data_ptr() < hi
        else:
            assert sv is None
    assert {id(p) for p in m.parameters()} == {id(p) for p in eng.param_list}
    assert packs == [1]                      # the pack of the fresh build
    G1 = eng.G
    eng.ensure_ready(CPU)
    assert packs == [1] and eng.G is G1


def _other_state(m, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items()}


def _set_grads(m, seed=6):
    g = torch.Generator().manual_seed(seed)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g)


# ---- a. no_grad in-place writes: repack -------------------------------------------------------------------------
def _mul_all(m):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.25)


def _reinit(m):
    def init(mod):
        if isinstance(mod, nn.Linear):
            nn.init.trunc_normal_(mod.weight, std=0.02)
    m.apply(init)


def _through_state_dict(m):
    sd = m.state_dict()
    for k, v in _other_state(m).items():
        sd[k].copy_(v)


def _one_matrix(m):
    with torch.no_grad():
        m.transformer_encoder.blocks[1].ffwd.mlp[2].weight.add_(1.0)


def _load_plain(m):
    m.load_state_dict(_other_state(m))


def _sgd(m):
    _set_grads(m)
    torch.optim.SGD(m.parameters(), lr=0.1).step()


def _adamw_foreach(m):
    _set_grads(m)
    torch.optim.AdamW(m.parameters(), lr=1e-3, foreach=True).step()


def _adamw_fused(m):
    # one native call over every parameter that (torch 2.10) bumps no version counter: seen through the optimizer
    # step hook alone
    _set_grads(m)
    torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True).step()


@pytest.mark.parametrize("mutate", [_mul_all, _reinit, _through_state_dict, _one_matrix, _load_plain, _sgd,
                                    _adamw_foreach, _adamw_fused], ids=lambda f: f.__name__.lstrip("_"))
def test_versioned_write_repacks_once(built, mutate):
    m, eng, packs = built
    G0 = eng.G
    mutate(m)
    _assert_repacked(m, eng, packs, G0)


class _WritesNothing(torch.optim.Optimizer):
    def __init__(self, params):
        super().__init__(params, {})

    def step(self, closure=None):
        return None


class _RefreshesShadows(_WritesNothing):
    refreshes_shadows = True                 # as FusedAdamW, whose kernel writes the shadows itself


def test_optimizer_step_marks_the_shadows_stale_unless_it_refreshes_them(built):
    """Any optimizer's step is taken as a write (torch's fused ones bump no version counter), except one that
    declares it keeps the shadows fresh: a FusedAdamW step must not cost a repack."""
    m, eng, packs = built
    G0 = eng.G
    _RefreshesShadows(m.parameters()).step()
    eng.ensure_ready(CPU)
    assert packs == [] and eng.G is G0
    _WritesNothing([m.mlp[3].bias]).step()   # one parameter of the engine's is enough
    _assert_repacked(m, eng, packs, G0)
    packs.clear()
    _WritesNothing(_model(8).parameters()).step()        # another model's parameters: not this engine's business
    eng.ensure_ready(CPU)
    assert packs == []
    from VisionTransformer.optim import FusedAdamW
    assert FusedAdamW.refreshes_shadows is True


def test_averaged_model_update_repacks_once(monkeypatch):
    """`AveragedModel.update_parameters` writes the averaged copy in place (first a copy, then the running mean)."""
    from torch.optim.swa_utils import AveragedModel
    src = _model(3)
    ema = AveragedModel(src)
    m, eng, packs = _settle(ema.module, monkeypatch)
    for _ in range(2):
        _mul_all(src)
        G0 = eng.G
        ema.update_parameters(src)
        _assert_repacked(m, eng, packs, G0)
        packs.clear()


# ---- b (assign), c, d: rebuild ----------------------------------------------------------------------------------
def _load_assign(m):
    m.load_state_dict(_other_state(m), assign=True)


def _repoint(get):
    def mutate(m):
        p = get(m)
        p.data = p.data.clone() * 1.5
    mutate.__name__ = "repoint_" + get.__name__
    return mutate


def query_w(m):
    return m.transformer_encoder.blocks[0].multi_head.heads[1].query.weight


def fc1_w(m):
    return m.transformer_encoder.blocks[1].ffwd.mlp[0].weight


def proj_b(m):
    return m.transformer_encoder.blocks[0].multi_head.proj.bias


def pos(m):
    return m.emdeddings.pos_embd


def _vector_to_parameters(m):
    from torch.nn.utils import parameters_to_vector, vector_to_parameters
    vector_to_parameters(parameters_to_vector(m.parameters()) * 0.5, m.parameters())


def _double_float(m):
    m.double().float()


def _new_head(m):
    m.mlp[3] = nn.Linear(4 * D, NC)


def _new_query(m):
    m.transformer_encoder.blocks[0].multi_head.heads[1].query = nn.Linear(D, D // H, bias=False)


def _new_ln_weight(m):
    m.transformer_encoder.blocks[1].ln2.weight = nn.Parameter(torch.full((D,), 0.5))


def _new_block(m):
    m.transformer_encoder.blocks[0] = _model(7).transformer_encoder.blocks[0]


def _finetune_head(m):
    m.requires_grad_(False)
    m.mlp[3] = nn.Linear(4 * D, NC)


@pytest.mark.parametrize("mutate", [_load_assign, _repoint(query_w), _repoint(fc1_w), _repoint(proj_b), _repoint(pos),
                                    _vector_to_parameters, _double_float, _new_head, _new_query, _new_ln_weight,
                                    _new_block, _finetune_head], ids=lambda f: f.__name__.lstrip("_"))
def test_repointed_or_replaced_rebuilds(built, mutate):
    m, eng, packs = built
    G0 = eng.G
    mutate(m)
    _assert_rebuilt(m, eng, packs, G0)


def test_new_head_with_another_class_count(built):
    """A 7-class head on a 10-class model: the gradient layout, the head bucket, the engine's `nc` and the model's
    config all follow it; a config object shared with other models is left alone."""
    m, eng, packs = built
    cfg0, G0, head0, block0 = m.vit_config, eng.G, eng.head_range, dict(eng.block_range)
    m.mlp[3] = nn.Linear(4 * D, 7)
    _assert_rebuilt(m, eng, packs, G0)
    assert eng.nc == 7 and m.vit_config.num_classes == 7 and cfg0.num_classes == NC
    assert eng.gw["h3_w"].shape == (7, 4 * D) and eng.gw["h3_b"].shape == (7,)
    shrink = head0[1] - eng.head_range[1]
    assert shrink > 0 and eng.head_range[0] == 0
    assert {l: (a - shrink, b - shrink) for l, (a, b) in block0.items()} == eng.block_range
    assert eng.embed_range[1] == eng.G.numel()
    f = vit.VisionTransformer(m.vit_config)
    f.load_state_dict(m.state_dict())


def test_replacement_of_another_shape_is_refused(built):
    """Only the head's class count is the module's to choose: the kernels trust every other shape."""
    m, eng, packs = built
    m.transformer_encoder.blocks[1].ffwd.mlp[0] = nn.Linear(D, 2 * D)
    with pytest.raises(RuntimeError, match="fc1_w has shape"):
        eng.ensure_ready(CPU)


def test_grads_survive_a_rebuild(built):
    """The gradients accumulated before a rebuild are carried into the new buffer by the next backward's attach;
    the replaced head starts from zero."""
    m, eng, packs = built
    assert eng._attach_grads() == 0.0
    eng._attach_pending()
    eng.G.copy_(torch.arange(eng.G.numel(), dtype=torch.float32))
    before = {k: p.grad.clone() for k, p in m.named_parameters()}
    G0 = eng.G
    proj_b(m).data = proj_b(m).data.clone()
    m.mlp[3] = nn.Linear(4 * D, NC)
    _assert_rebuilt(m, eng, packs, G0)
    assert eng._attach_grads() == 1.0
    for k, p in m.named_parameters():
        assert p.grad.data_ptr() == dict((id(q), gv) for q, gv in eng.grad_views)[id(p)].data_ptr()
        if k.startswith("mlp.3."):
            assert torch.all(p.grad == 0), k
        else:
            assert torch.equal(p.grad, before[k]), k


def test_repack_before_the_first_build_is_a_noop():
    m = _model()
    eng = m.hip_engine
    eng.repack()                             # documented after a `p.data` write; nothing is built yet
    assert eng.params is None and eng.stats["packs"] == 0
    assert not hasattr(eng, "mark_shadow_fresh")
