"""The attention backward's reference, per-element bound, inputs and case table (tests/helpers.py), settled on the CPU
from the reference alone before any kernel runs (as tests/test_cpu_gemm_ref.py does for the GEMMs):

  * attn_bwd_ref64 is the operation: with O and LSE from a float64 forward it equals float64 autograd of the suite's
    attention reference, and rows of masked keys and rows past an extent are exact zeros.
  * ATTN_BWD_E: the largest error of the rounding-point emulation (attn_bwd_emulate: fp32 with the kernels' bf16
    roundings) in units of u b after the 2^-8 |ref| term, per family and output; the kernels get C = 2 E.
  * Discrimination: twelve mutated references (never mutated kernels), each of which must leave the bound
    C u b + 2^-8 |ref| on at least half of the elements it touches, per output, on the "edges" input set of every case
    where the mutant applies.
  * The case table reaches every template build of bwdf7, dq7 / dkv7 and dq2 / dkv2, with and without dropout.
"""
import functools

import pytest
import torch

from helpers import (ATTN_BWD_BUILDS, ATTN_BWD_C, ATTN_BWD_E, ATTN_SEED, ATTN_STREAM, attn_bwd_case_inputs,
                     attn_bwd_case_ref, attn_bwd_cases, attn_bwd_emulate, attn_bwd_excess, attn_bwd_ref64,
                     attn_fwd_ref64, attn_heads)

CASES = attn_bwd_cases()
BY_ID = {c["id"]: c for c in CASES}
KINDS = ("flat", "edges")
SCALE = 0.125


def _heads(c, x):
    return tuple(attn_heads(x[n], c["B"], c["H"]) for n in ("q", "k", "v", "do"))


@pytest.mark.parametrize("cid", ["bwdf7-129x200-mask-p0.1-guard", "bwdf7-129x300-300_257_256_70-p0.1-guard",
                                 "pair7-300x200", "pair2-130x70-mask-p0.1-rehash-guard"])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_float64_autograd(cid, kind):
    """O and LSE from the float64 forward, unrounded: the closed form is the gradient of the suite's attention
    reference (test_gpu_attn7._ref, the oracle's dropout mask) to 1e-12 of each gradient's scale."""
    from test_gpu_attn7 import _ref
    c, x = BY_ID[cid], attn_bwd_case_inputs(cid, kind)
    q, k, v, do = (t.double() for t in _heads(c, x))
    o, lse = attn_fwd_ref64(q, k, v, x["keep"], x["drop"], c["p"], SCALE)
    r = attn_bwd_ref64(q, k, v, do, o, lse, x["keep"], x["drop"], c["p"], SCALE)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, rlse = _ref(qr, kr, vr, x["keep"], c["p"], ATTN_SEED, ATTN_STREAM)
    out.backward(do)
    assert (out.detach() - o).abs().max() <= 1e-12 * o.abs().max()
    assert (rlse.detach() - lse).abs().max() <= 1e-12 * lse.abs().max()
    for n, got, ref in (("dq", r.dq, qr.grad), ("dk", r.dk, kr.grad), ("dv", r.dv, vr.grad)):
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max(), n


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["masked"] and c["Lk"] > 1][::3])   # Lk 1: no masked key
def test_reference_and_emulation_give_exact_zeros_for_masked_keys(cid):
    """dK / dV rows of masked keys, rows past an extent among them, are exact zeros in the reference (and in the
    emulation), and their unit is 0: the bound leaves them no room."""
    c, x = BY_ID[cid], attn_bwd_case_inputs(cid, "edges")
    o, lse, _, _, t, (_, b_dk, b_dv) = attn_bwd_case_ref(cid, "edges")
    dead = ~x["keep"]
    assert dead.any()
    if c["ext"] is not None:
        for b, e in enumerate(c["ext"]):
            assert dead[b, e:].all()
    q, k, v, do = _heads(c, x)
    _, edk, edv = attn_bwd_emulate(q, k, v, do, o, lse, x["keep"], x["drop"], c["p"], SCALE, c["family"])
    m = dead[:, None, :, None].expand_as(t.dk)
    for g in (t.dk, t.dv, b_dk, b_dv, edk, edv):
        assert (g[m] == 0).all()
    live = (~dead)[:, None, :, None].expand_as(t.dk)
    assert (b_dk[live] > 0).all() and (b_dv[live] > 0).all()


@functools.lru_cache(maxsize=None)
def _emulation_error():
    """{family: {output: (largest excess, case id, input set)}} of the emulation against the reference."""
    worst = {f: {n: (0.0, None, None) for n in ("dq", "dk", "dv")} for f in ATTN_BWD_E}
    for c in CASES:
        for kind in KINDS:
            x = attn_bwd_case_inputs(c["id"], kind)
            o, lse, _, _, t, units = attn_bwd_case_ref(c["id"], kind)
            q, k, v, do = _heads(c, x)
            got = attn_bwd_emulate(q, k, v, do, o, lse, x["keep"], x["drop"], c["p"], SCALE, c["family"])
            for n, g, r, b in zip(("dq", "dk", "dv"), got, (t.dq, t.dk, t.dv), units):
                e = attn_bwd_excess(g, r, b).max().item()
                if e > worst[c["family"]][n][0]:
                    worst[c["family"]][n] = (e, c["id"], kind)
    return worst


def test_emulation_error_sets_the_constants():
    """E per family and output: the committed constant covers the measured maximum and is not more than a quarter above
    it; the kernels' C is twice E."""
    worst = _emulation_error()
    for f, d in worst.items():
        print(f"family {f}: " + ", ".join(f"E_{n} = {e:.3f} ({cid}, {kind})" for n, (e, cid, kind) in d.items()))
    for f, d in worst.items():
        for n, (e, cid, kind) in d.items():
            assert e <= ATTN_BWD_E[f][n] <= 1.25 * e, (f, n, e, ATTN_BWD_E[f][n], cid, kind)
            assert ATTN_BWD_C[f][n] == 2.0 * ATTN_BWD_E[f][n]


# ------------------------------------------------------------------------------------------------ mutated references
def _grads(c, x, P, D, G, delta, cdrop, *, cg=None):
    q, k, _, do = (t.double() for t in _heads(c, x))
    T = P * ((cdrop if cg is None else cg) * D * G - delta[..., None])
    PD = P * D
    return T, PD, SCALE * (T @ k), SCALE * (T.transpose(-1, -2) @ q), cdrop * (PD.transpose(-1, -2) @ do)


def _probs(t, lse, keep):
    P = torch.exp(t.S - lse.double()[..., None])
    return P if keep is None else P * keep[:, None, None, :].double()


def _last_keys(c, x):
    return [int(x["keep"][b].nonzero().max()) if x["keep"] is not None else c["Lk"] - 1 for b in range(c["B"])]


def _mutate(name, c, x, lse, t):
    """{output: mutated value} of mutant `name` on a case, or None where it does not apply."""
    B, Lq, Lk, p = c["B"], c["Lq"], c["Lk"], c["p"]
    q, k, _, do = (y.double() for y in _heads(c, x))
    keep = x["keep"]
    if name == "last key dropped from dQ":
        T = t.T.clone()
        for b, j in enumerate(_last_keys(c, x)):
            T[b, :, :, j] = 0
        return {"dq": SCALE * (T @ k)}
    if name == "key 256 dropped from dQ":
        if Lk <= 256:
            return None
        T = t.T.clone()
        T[..., 256] = 0
        return {"dq": SCALE * (T @ k)}
    if name in ("last query dropped from dK, dV", "query 64 dropped from dK, dV"):
        i = Lq - 1 if name.startswith("last") else 64
        if i >= Lq:
            return None
        T, PD = t.T.clone(), t.PD.clone()
        T[:, :, i] = 0
        PD[:, :, i] = 0
        return {"dk": SCALE * (T.transpose(-1, -2) @ q), "dv": t.c * (PD.transpose(-1, -2) @ do)}
    if name == "dK without ln 2":
        return {"dk": t.dk * 1.4426950408889634}
    if name == "delta of row i + 1":
        if Lq < 2:
            return None
        _, _, dq, dk, _ = _grads(c, x, t.P, t.D, t.G, torch.roll(t.delta, -1, -1), t.c)
        return {"dq": dq, "dk": dk}
    if name == "LSE of row i + 1":
        if Lq < 2:
            return None
        _, _, dq, dk, dv = _grads(c, x, _probs(t, torch.roll(lse, -1, -1), keep), t.D, t.G, t.delta, t.c)
        return {"dq": dq, "dk": dk, "dv": dv}
    if name == "masked key kept":
        if keep is None:
            return None
        lasts = _last_keys(c, x)
        inside = [(b, j) for b in range(B) for j in (~keep[b]).nonzero().flatten().tolist() if j < lasts[b]]
        if not inside:
            return None
        b, j = inside[len(inside) // 2]
        k2 = keep.clone()
        k2[b, j] = True
        _, _, dq, dk, dv = _grads(c, x, _probs(t, lse, k2), t.D, t.G, t.delta, t.c)
        return {"dq": dq, "dk": dk, "dv": dv}
    if p == 0:
        return None     # the rest are dropout mutants
    if name == "c missing on G":
        _, _, dq, dk, _ = _grads(c, x, t.P, t.D, t.G, t.delta, t.c, cg=1.0)
        return {"dq": dq, "dk": dk}
    if name == "c missing on dV":
        return {"dv": t.dv / t.c}
    if name == "D rolled by one key":
        if Lk < 2:
            return None
        _, _, dq, dk, dv = _grads(c, x, t.P, torch.roll(t.D, 1, -1), t.G, t.delta, t.c)
        return {"dq": dq, "dk": dk, "dv": dv}
    if name == "D rolled by 32 queries":
        if Lq <= 32:
            return None
        _, _, dq, dk, dv = _grads(c, x, t.P, torch.roll(t.D, 32, -2), t.G, t.delta, t.c)
        return {"dq": dq, "dk": dk, "dv": dv}
    raise KeyError(name)


MUTANTS = ["last key dropped from dQ", "key 256 dropped from dQ", "last query dropped from dK, dV",
           "query 64 dropped from dK, dV", "c missing on G", "c missing on dV", "D rolled by one key",
           "D rolled by 32 queries", "delta of row i + 1", "LSE of row i + 1", "masked key kept", "dK without ln 2"]
MIN_SHARE = 0.5


@pytest.mark.parametrize("name", MUTANTS)
def test_mutated_reference_leaves_the_bound(name):
    """On the "edges" inputs of every case where the mutant applies, at least half of the elements of each output it
    changes lie outside C u b + 2^-8 |ref| (C = 2 E of the case's family). A condition on the inputs, not a
    measurement: the edge weights of attn_bwd_case_inputs exist to make it hold."""
    least, where, n = 1.0, None, 0
    for c in CASES:
        x = attn_bwd_case_inputs(c["id"], "edges")
        _, lse, _, _, t, units = attn_bwd_case_ref(c["id"], "edges")
        mut = _mutate(name, c, x, lse, t)
        if mut is None:
            continue
        n += 1
        for out, b in zip(("dq", "dk", "dv"), units):
            if out not in mut:
                continue
            ref = getattr(t, out)
            touched = mut[out] != ref
            if not touched.any():       # one kept key and no dropout: T = 0, nothing of dQ / dK to change
                assert c["Lk"] == 1 and c["p"] == 0 and out != "dv", (name, c["id"], out)
                continue
            share = (attn_bwd_excess(mut[out], ref, b)[touched] > ATTN_BWD_C[c["family"]][out]).double().mean().item()
            if share < least:
                least, where = share, (c["id"], out)
    print(f"mutant '{name}': {n} cases, least share outside the bound {least:.3f} at {where}")
    assert n > 0
    assert least >= MIN_SHARE, (name, least, where)


def test_case_table_reaches_every_build():
    """Every template build of the kernels in scope, as ops.attn_last_path() reads it, is some case's expected path, and
    each (mask, passes, extent) combination with dropout and without."""
    got = {c["expect"] for c in CASES}
    missing = [b for b in ATTN_BWD_BUILDS if b not in got]
    assert not missing, missing
    # bwdf7 12; dq7 8 (dkv7's 6 among them); dq2 6 with dkv2 3; dq2 4 with dkv4 2
    assert len(ATTN_BWD_BUILDS) == 12 + 8 + 6 + 4 and len(set(ATTN_BWD_BUILDS)) == 30
    for b in ATTN_BWD_BUILDS:      # dropout and none: DM 0 next to DM 1 (recorded bits: DM 2 for dq2)
        for dm in ((0, 1, 2) if b[0] == "dq2+dkv2" else (0, 2) if b[0] == "dq2+dkv4" else (0, 1)):
            assert (b[0], dm) + b[2:] in got, (b, dm)
    for fam in ("bwdf7", "pair7"):
        assert any(c["fam"] == fam and c["strided"] for c in CASES)
    for fam in ("bwdf7", "pair7", "pair2"):
        assert any(c["fam"] == fam and c["guard"] for c in CASES)
    assert all(c["B"] * c["H"] <= 8 for c in CASES)
