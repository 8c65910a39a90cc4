"""The transposed bf16 weight copies (runtime.wt_t) as cache entries: the logic around them, on CPU tensors with the
native calls replaced by torch (the kernels themselves: tests/test_gpu_gemm256_dx.py)."""
import gc

import pytest
import torch

BF = torch.bfloat16


@pytest.fixture
def rt(monkeypatch):
    from fddm_hip import ops, optim, runtime

    def transpose_table(pairs):
        return ("table", list(pairs), len(pairs))

    def transpose_bf16_mt(table):
        calls.append(table)
        for src, dst in table[1]:
            dst.copy_(src.t())

    calls = []
    monkeypatch.setattr(ops, "cast", lambda x, dtype: x.to(dtype))
    monkeypatch.setattr(ops, "transpose_table", transpose_table)
    monkeypatch.setattr(ops, "transpose_bf16_mt", transpose_bf16_mt)
    monkeypatch.setattr(ops, "_DX_WT", "1")
    monkeypatch.setattr(optim, "stream", lambda: 0)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    runtime.transpose_calls = calls
    runtime.clear_cache()
    with runtime.use_precision("bf16"):
        yield runtime
    runtime.clear_cache()
    del runtime.transpose_calls


def _param(rows=16, cols=8, seed=0):
    return torch.nn.Parameter(torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)))


def _is_t(t, p):
    return t.dtype == BF and t.is_contiguous() and torch.equal(t, p.detach().to(BF).t())


def test_built_on_a_miss_and_served_again(rt):
    p = _param()
    assert rt.wt_t_entry(p) is None
    t = rt.wt_t(p)
    assert tuple(t.shape) == (8, 16) and _is_t(t, p)
    assert rt.wt_t(p) is t and rt.wt_t_entry(p) is t
    assert rt.bf16_entry(p) is not None and rt.bf16_entry(p) is not t        # its own key, next to the plain copy
    assert len(rt.transpose_calls) == 1


def test_in_place_change_invalidates(rt):
    p = _param()
    t = rt.wt_t(p)
    gen = rt.wcache_generation()
    with torch.no_grad():
        p.add_(1.0)                      # a checkpoint load or a DP broadcast: the version counter moves
    t2 = rt.wt_t(p)
    assert t2 is not t and _is_t(t2, p) and not _is_t(t, p)
    assert rt.wcache_generation() > gen  # the optimizer's tables see the replacement


def test_clear_cache_drops_it(rt):
    p = _param()
    t = rt.wt_t(p)
    epoch = rt.cache_epoch()
    rt.clear_cache()
    assert rt.wt_t_entry(p) is None and rt.cache_epoch() == epoch + 1
    assert rt.wt_t(p) is not t


def test_retained_for_a_captured_graph(rt):
    p = _param()
    with rt.retaining() as kept:
        t = rt.wt_t(p)              # built inside
    assert any(k is t for k in kept)
    with rt.retaining() as kept:
        assert rt.wt_t(p) is t      # served from the cache inside
    assert any(k is t for k in kept)


def test_reused_id_is_not_served_the_old_copy(rt):
    """A freed parameter's id (and address) can be reused: an entry filed under that id belongs to the dead tensor."""
    p = _param(seed=1)
    rt.wt_t(p)
    stale = rt._wcache[(id(p), BF, "T")]
    del p
    gc.collect()
    assert stale.ref() is None
    q = _param(seed=2)
    rt._wcache[(id(q), BF, "T")] = stale            # what id reuse leaves behind
    assert rt.wt_t_entry(q) is None
    t = rt.wt_t(q)
    assert t is not stale.tensor and _is_t(t, q)


def test_none_where_there_is_no_copy(rt, monkeypatch):
    from fddm_hip import ops
    assert rt.wt_t(torch.nn.Parameter(torch.randn(16))) is None          # not 2-D
    assert rt.wt_t(torch.nn.Parameter(torch.randn(12, 8))) is None       # rows % 8
    with rt.use_precision("fp32"):
        assert rt.wt_t(_param()) is None
    monkeypatch.setattr(ops, "_DX_WT", "0")                             # the diagnostic switch
    p = _param()
    assert rt.wt_t(p) is None and rt.wt_t_entry(p) is None


def _optimizer(rt, monkeypatch, params):
    """FusedAdamW whose native launches are replaced: "fddm_adamw" adds 1 to every parameter and rewrites its plain bf16
    copy through the data pointer's tensor, as the kernel does — in place, the version counter does not move."""
    from fddm_hip import optim
    launched = []

    def call(name, *args):
        launched.append(name)
        if name == "fddm_adamw":
            for p in params:
                p.data.add_(1.0)
                if p.dim() >= 2:
                    rt.bf16_entry(p).copy_(p.data.to(BF))
        return 0

    monkeypatch.setattr(optim, "call", call)
    opt = optim.FusedAdamW(params, lr=1e-3)
    for p in params:
        p.grad = torch.zeros_like(p)
    return opt, launched


def test_optimizer_refresh_keeps_it_current(rt, monkeypatch):
    ps = [_param(16, 8, 3), _param(24, 16, 4), torch.nn.Parameter(torch.randn(8))]
    opt, launched = _optimizer(rt, monkeypatch, ps)
    ts = [rt.wt_t(p) for p in ps[:2]]          # the backward asked for them
    n = len(rt.transpose_calls)
    ver = [p._version for p in ps]
    opt.clip_and_step(1.0)
    assert launched.count("fddm_adamw") == 1 and len(rt.transpose_calls) == n + 1     # one launch for all of them
    table = rt.transpose_calls[-1]
    assert [id(d) for _, d in table[1]] == [id(t) for t in ts]
    assert all(s is rt.bf16_entry(p) for (s, _), p in zip(table[1], ps))
    assert [p._version for p in ps] == ver
    for p, t in zip(ps, ts):
        assert rt.wt_t(p) is t and _is_t(t, p)             # same buffer, new contents, no rebuild
    assert len(rt.transpose_calls) == n + 1
    opt.clip_and_step(1.0)                                  # the table is reused
    assert len(rt.transpose_calls) == n + 2 and rt.transpose_calls[-1] is table


def test_optimizer_table_follows_the_cache(rt, monkeypatch):
    """The table's validity check covers the transposed copies: one that appears, is replaced or is dropped after the
    table was built means a new table (and a new table_epoch for captured step graphs)."""
    ps = [_param(16, 8, 5)]
    opt, _ = _optimizer(rt, monkeypatch, ps)
    opt.clip_and_step(1.0)                                  # no transposed copy yet: nothing to transpose
    assert not rt.transpose_calls
    e0 = opt.table_epoch
    t = rt.wt_t(ps[0])
    n = len(rt.transpose_calls)
    opt.clip_and_step(1.0)
    assert opt.table_epoch > e0 and len(rt.transpose_calls) == n + 1 and rt.transpose_calls[-1][1][0][1] is t
    assert _is_t(t, ps[0])
    with torch.no_grad():
        ps[0].mul_(2.0)                                     # changed outside the optimizer
    t2 = rt.wt_t(ps[0])
    e1 = opt.table_epoch
    opt.clip_and_step(1.0)
    assert t2 is not t and opt.table_epoch > e1 and rt.transpose_calls[-1][1][0][1] is t2 and _is_t(t2, ps[0])
    rt.clear_cache()
    e2 = opt.table_epoch
    opt.clip_and_step(1.0)
    assert opt.table_epoch > e2 and rt.wt_t_entry(ps[0]) is None
