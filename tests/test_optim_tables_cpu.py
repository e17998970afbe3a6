"""CPU-only checks of the fused optimizer's host tables, none of which launches anything or loads the library: the
one chunk cutter behind _ops.build_chunk_table and _ops.build_ema_pointers (tables built with device="cpu" decode
back through _lib.TensorChunk), and which user actions leave a cached step table (optim._StepTable) or swap table
(optim._SwapTables) valid.  FusedAdamW.step() itself refuses host tensors; the tables do not care where the pointers
they carry lead."""
import ctypes

import pytest
import torch

from VisionTransformer import _lib, _ops
from VisionTransformer.optim import FusedAdamW, _StepTable, _SwapTables

KEY = (0, "all")


def _decode(table, n):
    raw = table.numpy().tobytes()
    size = ctypes.sizeof(_lib.TensorChunk)
    assert len(raw) == n * size
    return [_lib.TensorChunk.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]


# ---- the cutter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,sizes,want", [
    (None, (1, 7, 8192, 8193), [(0, 1), (0, 7), (0, 8192), (0, 8192), (8192, 1)]),
    (16, (1, 16, 17), [(0, 1), (0, 16), (0, 16), (16, 1)])])
def test_both_builders_cut_at_the_same_boundaries(monkeypatch, chunk, sizes, want):
    """Chunk sizes in entry order, every p / g / m / v pointer at data_ptr() + 4 * offset (the bf16 shadow at
    2 * offset), one EMA pointer per chunk at the same offsets and NULL exactly on the chunk of the second tensor,
    which has no EMA.  With _ops.CHUNK patched, both builders follow the one constant."""
    if chunk is None:
        assert _ops.CHUNK == 8192      # the shipped chunk: the sizes above straddle it
    else:
        monkeypatch.setattr(_ops, "CHUNK", chunk)
    ps, gs, ms, vs, es = ([torch.zeros(n) for n in sizes] for _ in range(5))
    sh = [torch.zeros(n, dtype=torch.bfloat16) for n in sizes]
    es[1] = sh[1] = None
    table, n = _ops.build_chunk_table(list(zip(ps, gs, ms, vs, sh)), "cpu")
    ema, n_ema = _ops.build_ema_pointers(list(zip(ps, es)), "cpu")
    assert n == n_ema == len(want) and ema.dtype == torch.int64 and ema.numel() == n
    owner = [i for i, size in enumerate(sizes) for _ in range(-(-size // _ops.CHUNK))]
    assert [c.n for c in _decode(table, n)] == [size for _, size in want]
    for c, e, i, (off, _) in zip(_decode(table, n), ema.tolist(), owner, want):
        for got, t in ((c.p, ps[i]), (c.g, gs[i]), (c.m, ms[i]), (c.v, vs[i])):
            assert got == t.data_ptr() + 4 * off
        assert (c.shadow or 0) == (sh[i].data_ptr() + 2 * off if sh[i] is not None else 0)
        assert e == (es[i].data_ptr() + 4 * off if es[i] is not None else 0)
    assert [e == 0 for e in ema.tolist()] == [i == 1 for i in owner]


def test_a_table_without_gradients_or_moments_carries_null_there():
    """The form swap_ema() and the engine's pack build: (p, None, None, None, shadow)."""
    p, s = torch.zeros(5), torch.zeros(5)
    table, n = _ops.build_chunk_table([(p, None, None, None, s)], "cpu")
    (c,) = _decode(table, n)
    assert (c.p, c.g, c.m, c.v, c.shadow, c.n) == (p.data_ptr(), None, None, None, s.data_ptr(), 5)


# ---- step tables -----------------------------------------------------------------------------------------------------
def _optimizer(sizes=(5, 9, 3), ema=False, **kwargs):
    """Host fp32 parameters with gradients and the state step() would have made; never stepped."""
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes]
    opt = FusedAdamW(ps, **kwargs)
    for p in ps:
        _give_state(opt, p, ema)
    return opt, ps


def _give_state(opt, p, ema=False):
    p.grad = torch.ones_like(p)
    st = opt.state[p]
    st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
    if ema:
        st["ema"] = p.detach().clone()


def test_step_table_names_what_it_was_built_from():
    opt, ps = _optimizer(ema=True, ema_decay=0.9)
    tab = opt._table(KEY, ps)
    assert type(tab) is _StepTable and tab.version == opt._version and tab.device == ps[0].device
    assert all(a is b for a, b in zip(tab.params, ps)) and all(g is p.grad for g, p in zip(tab.grads, ps))
    assert tab.param_ptrs == [p.data_ptr() for p in ps] and tab.grad_ptrs == [p.grad.data_ptr() for p in ps]
    assert all(m is opt.state[p]["exp_avg"] and v is opt.state[p]["exp_avg_sq"] for (m, v), p in zip(tab.moments, ps))
    assert all(e is opt.state[p]["ema"] for e, p in zip(tab.emas, ps))
    assert tab.nchunks == len(ps) and tab.shadow_dtype == torch.float32 and tab.ema_dev.numel() == tab.nchunks
    assert [c.p for c in _decode(tab.dev_tab, tab.nchunks)] == tab.param_ptrs
    assert len(tab.keep) == len(ps) and not hasattr(tab, "__dict__")


def test_unchanged_parameters_reuse_the_table(monkeypatch):
    opt, ps = _optimizer()
    built = []
    real = _ops.build_chunk_table
    monkeypatch.setattr(_ops, "build_chunk_table", lambda *a: built.append(1) or real(*a))
    monkeypatch.setattr(_ops, "build_ema_pointers", lambda *a: pytest.fail("no parameter has an EMA"))
    tab = opt._table(KEY, ps)
    assert tab.valid(opt, ps) and tab.emas is None and tab.ema_dev is None
    assert opt._table(KEY, ps) is tab and opt._table(KEY, list(ps)) is tab and len(built) == 1
    assert opt._table((0, "t", 1), ps[:1]) is not tab and len(built) == 2      # another key: a table of its own


def _new_grad(opt, ps):
    ps[1].grad = ps[1].grad.clone()


def _grad_data(opt, ps):
    ps[1].grad.data = ps[1].grad.clone()


def _param_data(opt, ps):
    ps[1].data = ps[1].detach().clone()


def _exp_avg(opt, ps):
    opt.state[ps[2]]["exp_avg"] = torch.zeros_like(ps[2])


def _exp_avg_sq(opt, ps):
    opt.state[ps[2]]["exp_avg_sq"] = torch.zeros_like(ps[2])


def _load_state_dict(opt, ps):
    opt.load_state_dict(opt.state_dict())


def _add_param_group(opt, ps):
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})


def _invalidate(opt, ps):
    opt.invalidate()


CHANGES = [_new_grad, _grad_data, _param_data, _exp_avg, _exp_avg_sq, _load_state_dict, _add_param_group,
           _invalidate]


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("change", CHANGES, ids=lambda f: f.__name__.lstrip("_"))
def test_a_change_invalidates_the_step_table(change, ema):
    opt, ps = _optimizer(ema=ema, ema_decay=0.9 if ema else None)
    tab = opt._table(KEY, ps)
    assert tab.valid(opt, ps)
    change(opt, ps)
    assert not tab.valid(opt, ps)
    new = opt._table(KEY, ps)
    assert new is not tab and new.valid(opt, ps) and opt._table(KEY, ps) is new
    assert new.grad_ptrs == [p.grad.data_ptr() for p in ps] and new.param_ptrs == [p.data_ptr() for p in ps]
    assert [c.p for c in _decode(new.dev_tab, new.nchunks)] == new.param_ptrs
    assert [c.m for c in _decode(new.dev_tab, new.nchunks)] == [opt.state[p]["exp_avg"].data_ptr() for p in ps]


def test_a_replaced_ema_invalidates_the_step_table():
    opt, ps = _optimizer(ema=True, ema_decay=0.9)
    tab = opt._table(KEY, ps)
    opt.state[ps[0]]["ema"] = opt.state[ps[0]]["ema"].clone()
    assert not tab.valid(opt, ps)
    new = opt._table(KEY, ps)
    assert new is not tab and new.ema_dev.tolist() == [opt.state[p]["ema"].data_ptr() for p in ps]


def test_a_table_with_ema_pointers_stays_valid_while_ema_decay_is_unchanged():
    opt, ps = _optimizer(ema=True, ema_decay=0.9)
    tab = opt._table(KEY, ps)
    assert tab.emas is not None and tab.valid(opt, ps) and opt._table(KEY, ps) is tab
    opt.ema_decay = 0.99      # the value is a launch argument, not part of the table
    assert tab.valid(opt, ps) and opt._table(KEY, ps) is tab


def test_ema_decay_set_later_invalidates_a_table_built_without_emas():
    opt, ps = _optimizer()
    tab = opt._table(KEY, ps)
    assert tab.emas is None and tab.valid(opt, ps)
    opt.ema_decay = 0.9
    assert not tab.valid(opt, ps)
    for p in ps:      # what step() does next: the missing EMAs, then a table that points at them
        opt.state[p]["ema"] = p.detach().clone()
    new = opt._table(KEY, ps)
    assert new is not tab and new.valid(opt, ps) and new.ema_dev.numel() == new.nchunks


def test_another_parameter_list_of_the_same_length_invalidates_the_step_table():
    opt, ps = _optimizer()
    tab = opt._table(KEY, ps)
    assert not tab.valid(opt, [ps[1], ps[0], ps[2]]) and not tab.valid(opt, ps[:2]) and tab.valid(opt, ps)
    twin = torch.nn.Parameter(ps[2].detach().clone())
    opt.param_groups[0]["params"][2] = twin
    _give_state(opt, twin)
    assert not tab.valid(opt, ps[:2] + [twin])
    assert opt._table(KEY, ps[:2] + [twin]).params[2] is twin


def test_a_non_contiguous_gradient_is_refused_at_the_build():
    opt, ps = _optimizer(sizes=(6,))
    ps[0].grad = torch.ones(12)[::2]
    with pytest.raises(RuntimeError, match="non-contiguous grad/state"):
        opt._table(KEY, ps)
    assert KEY not in opt._tables


# ---- swap tables -----------------------------------------------------------------------------------------------------
def test_looking_for_emas_creates_no_state_entry():
    opt, ps = _optimizer(sizes=(4, 6))
    bare = torch.nn.Parameter(torch.zeros(3))
    opt.add_param_group({"params": [bare]})
    assert opt._ema_params() == [] and opt._ema_swap_tables() == [] and bare not in opt.state
    opt.state[ps[1]]["ema"] = ps[1].detach().clone()
    assert [id(p) for p in opt._ema_params()] == [id(ps[1])] and bare not in opt.state and len(opt.state) == 2
    with pytest.raises(RuntimeError, match="ROCm device"):      # swap_ema() itself is for device parameters
        opt._ema_swap_tables()
    assert bare not in opt.state


def _swap_param_data(opt, ps):
    ps[0].data = ps[0].detach().clone()


def _swap_ema_object(opt, ps):
    opt.state[ps[1]]["ema"] = opt.state[ps[1]]["ema"].clone()


@pytest.mark.parametrize("change", [_swap_param_data, _swap_ema_object, _invalidate, _load_state_dict,
                                    _add_param_group], ids=lambda f: f.__name__.lstrip("_"))
def test_swap_tables_follow_storage_ema_object_and_version(change):
    opt, ps = _optimizer(ema=True, ema_decay=0.9)
    swap = _SwapTables(opt, opt._ema_params())
    assert swap.valid(opt, opt._ema_params()) and swap.version == opt._version
    assert [(k.param is p, k.ptr, k.ema is opt.state[p]["ema"], k.shadow) for k, p in zip(swap.keys, ps)] == \
        [(True, p.data_ptr(), True, None) for p in ps]
    (tab,) = swap.tables      # one device, no shadows: one table, fp32
    assert tab.nchunks == len(ps) and tab.shadow_dtype == torch.float32
    assert [(c.p, c.g, c.shadow) for c in _decode(tab.dev_tab, tab.nchunks)] == [(p.data_ptr(), None, None) for p in ps]
    assert tab.ema_dev.tolist() == [opt.state[p]["ema"].data_ptr() for p in ps]
    change(opt, ps)
    assert not swap.valid(opt, opt._ema_params())
    assert _SwapTables(opt, opt._ema_params()).valid(opt, opt._ema_params())


def test_swap_tables_follow_the_set_of_parameters_with_an_ema():
    opt, ps = _optimizer(ema=True, ema_decay=0.9)
    swap = _SwapTables(opt, opt._ema_params())
    del opt.state[ps[2]]["ema"]
    assert len(opt._ema_params()) == 2 and not swap.valid(opt, opt._ema_params())
    assert not swap.valid(opt, [ps[1], ps[0], ps[2]])
