"""The attention forward's reference, per-element bounds, inputs and case table (tests/helpers.py), settled on the CPU
from the reference alone before any kernel runs (as tests/test_cpu_attn_bwd_ref.py does for the backward):

  * attn_fwd_terms64 / attn_fwd_ref64 is the operation: it equals a float64 restatement by torch.softmax /
    torch.logsumexp over an explicitly materialised bias table[:, rel] to 1e-12, and rows without a kept key are NaN.
  * ATTN_FWD_E: the largest error of the rounding-point emulation (attn_fwd_emulate) in units of u b after the rel and
    lin terms, per family ("7", "8", "16", "f32") and output (O, LSE); the kernels get C = 2 E.
  * Discrimination: sixteen mutated references (never mutated kernels), each of which must leave the bound on at least
    half of the elements it touches, per output, on the "edges" inputs of every case where it applies (one, the P
    rounded before the row sum, on the "faint" inputs that nine fwd7 cases carry: see its entry in MUTANTS).
  * The case table reaches every template build the dispatcher can launch.
"""
import functools

import pytest
import torch

from helpers import (ATTN_FWD_BUILDS, ATTN_FWD_C, ATTN_FWD_E, ATTN_FWD_E_FLOOR, _bf, attn_fwd_case_inputs,
                     attn_fwd_cases, attn_fwd_emulate, attn_fwd_excess, attn_fwd_terms64, attn_fwd_units, attn_heads,
                     attn_p32, attn_rel_index)

CASES = attn_fwd_cases()
BY_ID = {c["id"]: c for c in CASES}
SCALE = 0.125
OUTS = ("o", "lse")

# name -> (input set it is judged on, outputs it changes). Every mutant is a change of the float64 reference.
MUTANTS = {
    "bias index k - i + Lk": ("edges", OUTS),
    "bias index i - k + Lk - 1": ("edges", OUTS),
    "table row of head h + 1": ("edges", OUTS),
    "gate of query i + 1": ("edges", OUTS),
    "gate of head h + 1": ("edges", OUTS),
    "gate without the + 2": ("edges", OUTS),
    "bias added before the scale": ("edges", OUTS),
    "bias zero-filled for |k - i| >= 128": ("edges", OUTS),
    "last kept key dropped": ("edges", OUTS),
    "key past a ragged tile kept": ("edges", OUTS),
    "one masked key kept": ("edges", OUTS),
    "keys at and past key_len kept": ("edges", OUTS),
    # On the "edges" (and "flat") inputs a_ik is about 1, so the rounding of P is the size of the Q' rounding the LSE
    # unit already counts and no bound can tell the two apart; on the "faint" inputs a_ik is 2^-6 of that and the
    # unit shrinks with it, while a P rounded before the row sum moves the LSE by u sqrt(sum P^2 / 3) whatever q is.
    "P rounded to bf16 before the row sum": ("faint", ("lse",)),
    "dropout scale on the LSE": ("edges", ("lse",)),
    "dropout mask transposed": ("edges", ("o",)),
    "1 / (1 - p) left off": ("edges", ("o",)),
}
MIN_SHARE = 0.5


def _groups():
    """Cases that share their inputs (shape, mask, dropout, gate source, dtype): {key: [cases]}."""
    g = {}
    for c in CASES:
        key = (c["Lq"], c["Lk"], c["B"], c["H"], c["masked"], tuple(c["ext"] or ()), c["p"], c["src"], c["f32"],
               c["g8"], c["dead"])
        g.setdefault(key, []).append(c)
    return g


def _fwd(S, Dc, v):
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    return (P if Dc is None else P * Dc) @ v, lse


def _mutants(c, x, r, q, k, v, kind):
    """{name: {output: mutated value}} of every mutant that applies to the case on input set `kind`."""
    B, Lq, Lk, p = c["B"], c["Lq"], c["Lk"], c["p"]
    keep = x["keep"]
    qk = SCALE * (q @ k.transpose(-1, -2))
    vd = v
    out = {}

    def masked(S, kp=keep):
        return S if kp is None else S.masked_fill(~kp[:, None, None, :], float("-inf"))

    def put(name, S, Dc=r.D, vv=vd):
        o, lse = _fwd(S, Dc, vv)
        out[name] = {"o": o, "lse": lse}

    if kind == "faint":
        if c["family"] == "7":
            m = r.m[..., None]
            out["P rounded to bf16 before the row sum"] = {"lse": r.m + torch.log(_bf(torch.exp(r.S - m)).double().sum(-1))}
        return out
    full = r.S if keep is None else None
    if c["rel"]:
        S_ = Lk
        rel, tab, g = attn_rel_index(S_), x["table"].double(), r.g
        T = tab[:, rel]
        bias = lambda gg, TT: masked(qk + gg[..., None] * TT[None])  # noqa: E731
        out_of_row = torch.nn.functional.pad(tab, (0, 1))           # the entry after the row: zero-filled
        put("bias index k - i + Lk", bias(g, out_of_row[:, rel + 1]))
        put("bias index i - k + Lk - 1", bias(g, tab[:, 2 * (S_ - 1) - rel]))
        put("table row of head h + 1", bias(g, torch.roll(tab, -1, 0)[:, rel]))
        if S_ > 1:
            put("gate of query i + 1", bias(torch.roll(g, -1, -1), T))
        put("gate of head h + 1", bias(torch.roll(g, -1, 1), T))
        put("gate without the + 2", bias(g - 2.0, T))
        put("bias added before the scale", masked(qk + SCALE * g[..., None] * T[None]))
        if S_ > 128:
            put("bias zero-filled for |k - i| >= 128", bias(g, T * ((rel - (S_ - 1)).abs() < 128)))
        full = qk + g[..., None] * T[None]
    elif keep is not None:
        full = qk
    alive = [b for b in range(B) if keep is None or keep[b].any()]
    lasts = {b: int(keep[b].nonzero().max()) if keep is not None else Lk - 1 for b in alive}
    if (Lk % 64 != 0 or keep is not None) and all((keep[b].sum() if keep is not None else Lk) > 1 for b in alive):
        S2 = r.S.clone()
        for b, j in lasts.items():
            S2[b, :, :, j] = float("-inf")
        put("last kept key dropped", S2)
    if Lk % 64 != 0 and keep is None:
        # the row read past the end is clamped to Lk - 1 (attn7.hip :249): the last key a second time, with the bias of
        # the offset one further
        col = qk[..., -1:]
        if c["rel"]:
            col = col + r.g[..., None] * out_of_row[:, rel[:, -1] + 1][None, :, :, None]
        put("key past a ragged tile kept", torch.cat([r.S, col], -1),
            None if r.D is None else torch.cat([r.D, r.D[..., -1:]], -1), torch.cat([vd, vd[:, :, -1:]], 2))
    if keep is not None:
        inside = [(b, j) for b in alive for j in (~keep[b]).nonzero().flatten().tolist() if j < lasts[b]]
        if inside:
            b, j = inside[len(inside) // 2]
            S2 = r.S.clone()
            S2[b, :, :, j] = full[b, :, :, j]
            put("one masked key kept", S2)
        if c["ext"] is not None and any(0 < e < Lk for e in c["ext"]):
            k2 = keep.clone()
            for b, e in enumerate(c["ext"]):
                if e > 0:                  # an entry without a key stays without one (no tile runs)
                    k2[b, e:] = True
            put("keys at and past key_len kept", masked(full, k2))
    if p > 0:
        out["dropout scale on the LSE"] = {"lse": r.LSE + torch.log((r.P * r.D).sum(-1))}
        if Lq == Lk and Lk > 1:
            put("dropout mask transposed", r.S, r.D.transpose(-1, -2))
            del out["dropout mask transposed"]["lse"]
        out["1 / (1 - p) left off"] = {"o": r.O / r.c}
    return out


@functools.lru_cache(maxsize=None)
def _survey():
    """One pass over every group of cases and input set: ({family: {output: (largest excess of the emulation, case,
    input set)}}, {mutant: (least share outside the bound, (case, output), cases it applied to)})."""
    worst = {f: {n: (0.0, None, None) for n in OUTS} for f in ATTN_FWD_E}
    shares = {name: [1.0, None, 0] for name in MUTANTS}
    for cs in _groups().values():
        c0 = cs[0]
        for kind in sorted({kd for c in cs for kd in c["kinds"]}):
            x = attn_fwd_case_inputs(c0["id"], kind)
            q, k, v = (attn_heads(x[n], c0["B"], c0["H"]).double() for n in ("q", "k", "v"))
            p = attn_p32(c0["p"])
            g, tb = (x["g64"], x["table"]) if c0["rel"] else (None, None)
            r = attn_fwd_terms64(q, k, v, x["keep"], x["drop"], p, SCALE, g, x.get("dg"), tb)
            muts = None
            for fam in sorted({c["family"] for c in cs if kind in c["kinds"]}):
                c = next(c for c in cs if c["family"] == fam and kind in c["kinds"])
                eo, el, trip = attn_fwd_emulate(fam, q, k, v, x["keep"], x["drop"], p, SCALE, g, tb)
                U = attn_fwd_units(fam, r, q, k, v, SCALE, "either" if c["g8"] else trip)
                bound = {"o": (r.O, U["b_o"], U["rel"], U["lin_o"]), "lse": (r.LSE, U["b_lse"], 0.0, U["lin_lse"])}
                for n, got in (("o", eo), ("lse", el)):
                    ref, b, rel, lin = bound[n]
                    e = attn_fwd_excess(got, ref, b, U["u"], rel, lin).max().item()
                    if e > worst[fam][n][0]:
                        worst[fam][n] = (e, c["id"], kind)
                if kind not in ("edges", "faint"):
                    continue
                if muts is None:
                    muts = _mutants(c, x, r, q, k, v, kind)
                for name, mut in muts.items():
                    if MUTANTS[name][0] != kind or (name.startswith("P rounded") and fam != "7"):
                        continue
                    shares[name][2] += 1
                    for n in MUTANTS[name][1]:
                        ref, b, rel, lin = bound[n]
                        # changed by more than float64 rounding (a second copy of the only key leaves O where it was)
                        touched = ((mut[n] - ref).abs() > 1e-12 * (ref.abs() + 1.0)) & torch.isfinite(ref)
                        if not touched.any():
                            continue
                        ex = attn_fwd_excess(mut[n], ref, b, U["u"], rel, lin)[touched]
                        share = (ex > ATTN_FWD_C[fam][n]).double().mean().item()
                        if share < shares[name][0]:
                            shares[name][0], shares[name][1] = share, (c["id"], n)
    return worst, shares


def test_emulation_error_sets_the_constants():
    """E per family and output: the committed constant covers the measured maximum with at most 10 % headroom (plus
    ATTN_FWD_E_FLOOR); the kernels' C is twice E."""
    worst, _ = _survey()
    for f, d in worst.items():
        print(f"family {f}: " + ", ".join(f"E_{n} = {e:.3f} ({cid}, {kind})" for n, (e, cid, kind) in d.items()))
    for f, d in worst.items():
        for n, (e, cid, kind) in d.items():
            assert e <= ATTN_FWD_E[f][n] <= 1.1 * e + ATTN_FWD_E_FLOOR, (f, n, e, ATTN_FWD_E[f][n], cid, kind)
            assert ATTN_FWD_C[f][n] == 2.0 * ATTN_FWD_E[f][n]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutated_reference_leaves_the_bound(name):
    """At least half of the elements of each output the mutant changes lie outside the bound (C = 2 E of the case's
    family), on every case where it applies. A condition on the inputs, not a measurement: the edge keys and the
    table's spikes of attn_fwd_case_inputs exist to make it hold."""
    least, where, n = _survey()[1][name]
    print(f"mutant '{name}': {n} cases, least share outside the bound {least:.3f} at {where}")
    assert n > 0
    assert least >= MIN_SHARE, (name, least, where)


@pytest.mark.parametrize("kind", ("flat", "edges"))
@pytest.mark.parametrize("cid", ["fwd7-129x200-mask-p0.1-own-guard", "fwd7-129x300-300_257_256_70-p0.1-ready-guard",
                                 "fwd7-257x257-gx-auto", "fwd7-129x129-graw-auto", "fwd5-200x200-mask-gate-relfwd5",
                                 "fwd7-200x200-65_129-gx-auto", "fwd7-129x129-129_0-gx-auto",
                                 "generic-129x129-mask-gate-auto", "fwd8-65x17-mask-dead",
                                 "fwd5-129x129-mask-gate-relfwd5-dead"])
def test_reference_equals_float64_restatement(cid, kind):
    """torch.softmax / torch.logsumexp over scores with an explicitly materialised bias table[:, rel], to 1e-12; rows
    of an entry without a key are NaN in O and LSE, every other element is finite."""
    from oracle import fddm_oracle as O
    c, x = BY_ID[cid], attn_fwd_case_inputs(cid, kind)
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    q, k, v = (attn_heads(x[n], B, H).double() for n in ("q", "k", "v"))
    g, tb = (x["g64"], x["table"]) if c["rel"] else (None, None)
    r = attn_fwd_terms64(q, k, v, x["keep"], x["drop"], attn_p32(c["p"]), SCALE, g, x.get("dg"), tb)
    s = (q @ k.transpose(-1, -2)) / 8.0
    if c["rel"]:
        rel = torch.arange(Lk)[None, :] - torch.arange(Lk)[:, None] + Lk - 1
        bias = torch.stack([tb.double()[h][rel] for h in range(H)])                     # [H, Lq, Lk]
        s = s + g[..., None] * bias[None]
    if x["keep"] is not None:
        s = s.masked_fill(~x["keep"][:, None, None, :], float("-inf"))
    pr, lse = torch.softmax(s, -1), torch.logsumexp(s, -1)
    if c["p"] > 0:
        pr = pr * O.attn_dropout_keep(5, 9, B, H, Lq, Lk, c["p"]).double() / (1.0 - attn_p32(c["p"]))
    out = pr @ v
    dead = torch.zeros(B, dtype=torch.bool) if x["keep"] is None else ~x["keep"].any(-1)
    assert dead.any() == (c["dead"] or (c["ext"] is not None and 0 in c["ext"]))
    assert torch.isnan(r.O[dead]).all() and torch.isnan(r.LSE[dead]).all()
    live = ~dead
    assert torch.isfinite(r.O[live]).all() and torch.isfinite(r.LSE[live]).all()
    assert (r.O[live] - out[live]).abs().max() <= 1e-12 * out[live].abs().max()
    assert (r.LSE[live] - lse[live]).abs().max() <= 1e-12 * lse[live].abs().max()


def test_case_table_reaches_every_build():
    """Every template build the dispatcher can launch, as ops.attn_last_path()["fwd"] reads it, is some case's expected
    path (fwd2_kernel has no relative-position build: helpers.ATTN_FWD_BUILDS)."""
    got = {c["expect"] for c in CASES}
    missing = [b for b in ATTN_FWD_BUILDS if b not in got]
    assert not missing, missing
    # fwd7 6 + 2 KX + 3 REL + 1 REL KX; fwd8 6; fwd6 9; fwd2 4; fwd5 2; the generic kernel's four runtime paths
    assert len(ATTN_FWD_BUILDS) == 12 + 6 + 9 + 4 + 2 + 4 == len(set(ATTN_FWD_BUILDS))
    assert not [e for e in got if e not in ATTN_FWD_BUILDS]
    for kernel in ("fwd7", "fwd8", "fwd6"):
        assert any(c["kernel"] == kernel and c["strided"] for c in CASES)
        assert any(c["kernel"] == kernel and c["guard"] for c in CASES)
        assert {c["bits"] for c in CASES if c["kernel"] == kernel} >= {None, "ready", "own"}
    for src in ("gate", "graw", "gx"):
        for kernel in ("fwd7", "fwd5"):
            assert any(c["kernel"] == kernel and c["src"] == src for c in CASES)
    assert sum(c["g8"] is not None for c in CASES) == 2
    assert all(c["B"] * c["H"] <= 8 for c in CASES)
