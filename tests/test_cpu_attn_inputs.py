"""The inputs of tests/test_gpu_attn7.py::test_fwd8_guard_and_fallback_match_float64, checked without a GPU: a CPU
emulation of the row sum that fwd8's fast path accumulates (helpers.fwd8_fast_path_rowsum, mirroring csrc/attn8.hip's
fixed per-chain reference and its guard 2^-40 <= sum <= 2^64) proves which query rows must send their wave to the
online-softmax fallback and which stay on the fast path, with margins for what the emulation leaves out (the bf16
packing of P, the MFMA summation order)."""
import pytest
import torch

from helpers import FWD8_GUARD_GEOMS, fwd8_fast_path_rowsum, fwd8_guard_cases, fwd8_guard_inputs

bf = torch.bfloat16


def _heads(x, B, H):
    return x.to(bf).view(B, -1, H, 64).transpose(1, 2)


def test_guard_cases_cover_every_class_and_geometry():
    cases = fwd8_guard_cases()
    assert len(cases) == 18 and {g for g, *_ in cases} == set(FWD8_GUARD_GEOMS)
    for g in FWD8_GUARD_GEOMS:
        assert {(k, cls) for gg, k, _, cls in cases if gg == g} == {("rise", "trips"), ("rise", "inside"),
                                                                   ("fall", "trips"), ("fall", "inside")}
    assert sum(1 for g, *_ in cases if g == "a") == 6


def test_emulated_rowsum_of_plain_softmax_inputs():
    """randn inputs: the reference is within the row's spread of its maximum, the sum is a few keys' worth and no row
    trips; a fully masked row sums to 0 and trips; rounding: Q' is bf16, so the scores are those of bf16(q c) k."""
    gen = torch.Generator().manual_seed(1)
    q, k = (torch.randn(L, 64, generator=gen).to(bf) for L in (70, 100))
    tot, trip = fwd8_fast_path_rowsum(q, k)
    assert not trip.any() and (tot >= 1.0).all() and (tot < 2.0 ** 12).all()
    qp = (q.float() * torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32)).to(bf).double()
    s = qp @ k.double().t()
    rf = s[:, :32].max(-1).values.to(bf).double()
    want = torch.exp2(s - rf[:, None]).sum(-1)
    assert torch.allclose(tot.double(), want, rtol=1e-5)
    tot, trip = fwd8_fast_path_rowsum(q, k, torch.zeros(100, dtype=torch.bool))
    assert (tot == 0).all() and trip.all()
    keep = torch.ones(100, dtype=torch.bool)
    keep[:32] = False  # reference 0: the sum is that of exp2(scores)
    tot, _ = fwd8_fast_path_rowsum(q, k, keep)
    assert torch.allclose(tot.double(), torch.exp2(s[:, 32:]).sum(-1), rtol=1e-5)


def test_attn_fwd_rejects_a_bias_table_without_its_gate(monkeypatch):
    """ops.attn_fwd(..., table=t) with no gate: the biased kernel builds read the gate, so the call is refused by the
    Python check, before anything reaches the library (the library's entry point refuses it as well)."""
    from fddm_hip import ops

    def no_call(*a, **k):
        raise AssertionError("attn_fwd reached the library call")
    monkeypatch.setattr(ops, "call", no_call)
    B, H, L = 1, 2, 16
    q, k, v, out = (torch.zeros(B * L, H * 64, dtype=bf) for _ in range(4))
    table = torch.zeros(H, 2 * L - 1)
    with pytest.raises(ValueError, match="gate"):
        ops.attn_fwd(q, k, v, out, None, B, H, L, L, table=table)
    with pytest.raises(ValueError, match="gate"):   # the zero-padded small-head path checks before it recurses
        ops.attn_fwd(q[:, :64], k[:, :64], v[:, :64], out[:, :64], None, B, H, L, L, table=table)


@pytest.mark.parametrize("geom,kind,c,cls", fwd8_guard_cases())
def test_guard_inputs_trip_exactly_the_designated_rows(geom, kind, c, cls):
    B, H, Lq, Lk, _, _, _ = FWD8_GUARD_GEOMS[geom]
    q, k, v, keep, rows = fwd8_guard_inputs(geom, kind, c)
    assert (keep is not None) == (kind == "fall" or geom == "a")
    qh, kh, vh = (_heads(x, B, H) for x in (q, k, v))
    des = torch.zeros(Lq, dtype=torch.bool)
    des[rows] = True
    edge = []
    for b in range(B):
        for h in range(H):
            tot, trip = fwd8_fast_path_rowsum(qh[b, h], kh[b, h], None if keep is None else keep[b])
            lg = torch.log2(tot.double())
            if cls == "trips":
                assert torch.equal(trip, des), (b, h, trip.nonzero().flatten().tolist())
                t = tot[des]
                if c == 12.0:
                    assert torch.isinf(t).all()
                elif c == 25.0:
                    assert (t == 0).all()
                elif kind == "rise":   # representable: at least 2^2 outside the bound
                    assert torch.isfinite(t).all() and (lg[des] >= 66).all(), lg[des]
                else:
                    assert (t > 0).all() and (lg[des] <= -42).all(), lg[des]
            else:
                assert not trip.any(), (b, h, trip.nonzero().flatten().tolist())
                edge.append(lg[des])
            # every row that stays on the fast path: a factor 2^4 inside either bound
            stay = ~des if cls == "trips" else torch.ones_like(des)
            assert (lg[stay] <= 60).all() and (lg[stay] >= -36).all(), (lg[stay].min(), lg[stay].max())
    if cls == "inside":  # some designated row reaches towards its bound: the fast path's range, not its middle
        e = torch.cat(edge)
        assert (e.max() >= 52) if kind == "rise" else (e.min() <= -24), (e.min(), e.max())
    # the float64 reference (softmax, LSE, output) is finite everywhere
    s = (qh.double() @ kh.double().transpose(-1, -2)) / 8.0
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    out = torch.softmax(s, -1) @ vh.double()
    assert torch.isfinite(lse).all() and torch.isfinite(out).all()
