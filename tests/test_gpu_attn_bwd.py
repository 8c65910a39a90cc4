"""Every element of dQ, dK and dV of the bf16 attention backward kernels against the float64 reference of the operation
the C ABI defines (helpers.attn_bwd_ref64), within the per-element bound

    |gpu - ref| <= C u b + 2^-8 |ref|,    u = 2^-9, b = helpers.attn_bwd_units (root-sum-square), C = 2 E

whose constants tests/test_cpu_attn_bwd_ref.py settles from the reference alone (E from an emulation of the kernels'
rounding points; twelve mutated references that must leave the bound). Kernels: bwdf7 <DM, MASK, NP, KX>, dq7 + dkv7
(csrc/attn7.hip), dq2 with dkv2 or dkv4 (csrc/attention.hip), every template build, through ops.attn_bwd with and
without key_len. Each test asserts through ops.attn_last_path() the kernels and the builds it meant to reach.

Isolated mode (every case): O = bf16(float64 forward) and LSE = fp32(float64 LSE) go to the kernel and to the
reference alike. Chained mode (about one case in four, and every length-bounded one): O and LSE come from ops.attn_fwd
on the same inputs (fwd7, and fwd8 forced), the reference receives those tensors, and the forward keeps its own
tolerance. Both run on the "flat" and the "edges" inputs of helpers.attn_bwd_case_inputs.

Without exception: outputs are finite; dK / dV rows of masked keys and of keys past an extent are exact zeros (the
outputs are pre-filled with NaN); NaN-filled guard columns around dq / dk / dv keep their bits; the workspace is
pre-filled with NaN (bwdf7's two-pass dQ partials, the pairs' row terms).

Each test prints the kernel's worst error in units of u b per output. Largest seen on an MI355X (dQ / dK / dV, isolated
and chained, both input sets): bwdf7 3.82 / 4.00 / 3.95 and dq7 + dkv7 3.85 / 3.93 / 3.80 against C = 8.4 / 8.8 / 8.6;
dq2 + dkv2 2.27 / 2.36 / 2.60 and dq2 + dkv4 2.14 / 2.10 / 2.59 against C = 5.0 / 5.2 / 5.6.
"""
import pytest
import torch

from helpers import (ATTN_BWD_C, attn_p32, ATTN_SEED, ATTN_STREAM, attn_bwd_case_inputs, attn_bwd_case_ref,
                     attn_bwd_cases, attn_bwd_excess, attn_bwd_ref64, attn_bwd_units, attn_heads, attn_rows, close)

pytestmark = pytest.mark.gpu
LSE_ATOL = 4e-3          # tests/test_gpu_attn7.py's
SCALE = 0.125

dev = torch.device("cuda:0")
bf = torch.bfloat16
CASES = attn_bwd_cases()
BY_ID = {c["id"]: c for c in CASES}
KINDS = ("flat", "edges")
NAN = float("nan")


def ops():
    from fddm_hip import ops as o
    return o


def _nan_bits(t):
    return t.view(torch.int16).clone()


class _Dev:
    """One case's inputs on the device, in the layout the case asks for."""

    def __init__(self, c, x):
        B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
        D = H * 64
        self.D = D
        to = lambda t, L: t.reshape(B * L, D).to(dev, bf)  # noqa: E731
        if c["strided"]:    # the decoder's fused projection: q | k | v side by side, row stride 3 D
            buf = torch.zeros(B * max(Lq, Lk), 3 * D, device=dev, dtype=bf)
            buf[: B * Lq, :D] = to(x["q"], Lq)
            buf[: B * Lk, D: 2 * D] = to(x["k"], Lk)
            buf[: B * Lk, 2 * D:] = to(x["v"], Lk)
            self.q, self.k, self.v = buf[: B * Lq, :D], buf[: B * Lk, D: 2 * D], buf[: B * Lk, 2 * D:]
        else:
            self.q, self.k, self.v = (to(x[n], L).contiguous() for n, L in (("q", Lq), ("k", Lk), ("v", Lk)))
        self.do = to(x["do"], Lq).contiguous()
        self.kk = x["keep"].to(dev).to(torch.uint8).contiguous() if x["keep"] is not None else None


def _bits(c, fam):
    """The recorded keep bits of the case's site, written by the producer under kernel selection `fam` (the layout is
    the selected family's), or None (no dropout, or the backward rehashes)."""
    o = ops()
    if c["p"] == 0 or c["rehash"]:
        return None
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    old = o.attn_force_kernels(fam)
    try:
        db = o.drop_bits(B, H, Lq, Lk, dev).view(1, -1)
        o.attn_drop_bits(db, 1, B, H, Lq, Lk, c["p"], ATTN_SEED, ATTN_STREAM, 0)
    finally:
        o.attn_force_kernels(old)
    return db.view(-1)


def _backward(c, d, od, lse, db):
    """ops.attn_bwd of the case on device tensors; returns (dq, dk, dv) on the CPU as float64 [B, H, L, 64] and asserts
    the path, the guard columns and that every output element was written with a finite value."""
    from fddm_hip._lib import lib
    o = ops()
    B, H, Lq, Lk, D = c["B"], c["H"], c["Lq"], c["Lk"], d.D
    pad = 8 if c["guard"] else 0
    wide = [torch.full((B * L, D + 2 * pad), NAN, device=dev, dtype=bf) for L in (Lq, Lk, Lk)]   # NaN: never-written
    before = [_nan_bits(w) for w in wide]                                                          # elements show
    dq, dk, dv = (w[:, pad: pad + D] for w in wide)
    ws = torch.full((int(lib().fddm_attn_bwd_ws_floats(B, H, Lq, Lk)),), NAN, device=dev)
    kl = o.key_extent(d.kk) if c["ext"] is not None else None
    old = o.attn_force_kernels(c["force"])
    try:
        o.attn_bwd(d.q, d.k, d.v, od, d.do, lse, dq, dk, dv, B, H, Lq, Lk, key_keep=d.kk, drop_p=c["p"],
                   seed=ATTN_SEED, rng_stream=ATTN_STREAM, dbits=db, key_len=kl, ws=ws)
        path = o.attn_last_path()["bwd"]
    finally:
        o.attn_force_kernels(old)
    torch.cuda.synchronize()
    assert path == c["expect"], (path, c["expect"])
    if pad:
        for n, w, b0 in zip(("dq", "dk", "dv"), wide, before):
            now = _nan_bits(w)
            assert torch.equal(now[:, :pad], b0[:, :pad]) and torch.equal(now[:, pad + D:], b0[:, pad + D:]), \
                f"{n}: guard columns changed"
    return tuple(attn_heads(g.float().cpu().double(), B, H) for g in (dq, dk, dv))


def _check(c, kind, mode, got, t, units, keep):
    """The per-element bound, the exact zeros, finiteness; prints the worst error in units of u b."""
    C = ATTN_BWD_C[c["family"]]
    worst, fails = {}, []
    for n, g, b in zip(("dq", "dk", "dv"), got, units):
        ref = getattr(t, n)
        assert torch.isfinite(g).all(), f"{n}: non-finite values ({(~torch.isfinite(g)).sum().item()} elements)"
        ex = attn_bwd_excess(g, ref, b)
        worst[n] = ex.max().item()
        bad = ex > C[n]
        if bad.any():
            idx = bad.nonzero()
            fails.append(f"{n}: {idx.shape[0]} of {bad.numel()} elements outside C = {C[n]:.2f} (worst {worst[n]:.2f} "
                         f"u b); first (b,h,row,col) {idx[:6].tolist()}, rows {sorted(set(idx[:, 2].tolist()))[:12]}")
    print(f"ATTNBWD fam={c['expect'][0]} mode={mode} kind={kind} id={c['id']} " +
          " ".join(f"{n}={worst[n]:.3f}" for n in ("dq", "dk", "dv")))
    if keep is not None:
        dead = (~keep)[:, None, :, None].expand_as(got[1])
        assert (got[1][dead] == 0).all() and (got[2][dead] == 0).all(), "dK / dV rows of masked keys: not exact zeros"
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_attn_bwd_isolated_matches_float64_per_element(cid, kind):
    c, x = BY_ID[cid], attn_bwd_case_inputs(cid, kind)
    o_, lse_, _, _, t, units = attn_bwd_case_ref(cid, kind)
    d = _Dev(c, x)
    od = attn_rows(o_).to(dev, bf).contiguous()
    lse = lse_.reshape(c["B"] * c["H"], c["Lq"]).to(dev).contiguous()
    got = _backward(c, d, od, lse, _bits(c, c["force"]))
    _check(c, kind, "isolated", got, t, units, x["keep"])


CHAINED = [(c["id"], f) for c in CASES if c["chain"]
           for f in (("fwd7",) if c["ext"] is not None else ("fwd7", "fwd8"))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid,fwd", CHAINED)
def test_attn_bwd_chained_behind_the_forward_matches_float64_per_element(cid, fwd, kind):
    """The backward consumes the forward kernel's bf16 O and fp32 LSE, as the train step does; the reference receives
    the same two tensors. A key extent always takes fwd7 (its KX build)."""
    o = ops()
    c, x = BY_ID[cid], attn_bwd_case_inputs(cid, kind)
    _, _, o64, lse64, _, _ = attn_bwd_case_ref(cid, kind)
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    d = _Dev(c, x)
    db = _bits(c, fwd)
    od = torch.full((B * Lq, d.D), NAN, device=dev, dtype=bf)
    lse = torch.full((B * H, Lq), NAN, device=dev)
    kl = o.key_extent(d.kk) if c["ext"] is not None else None
    old = o.attn_force_kernels(fwd)
    try:
        o.attn_fwd(d.q, d.k, d.v, od, lse, B, H, Lq, Lk, key_keep=d.kk, drop_p=c["p"], seed=ATTN_SEED,
                   rng_stream=ATTN_STREAM, dbits=db, bits_ready=db is not None, key_len=kl)
        fpath = o.attn_last_path()["fwd"]
    finally:
        o.attn_force_kernels(old)
    mk = 2 if x["keep"] is not None else 1 if Lk % 64 else 0
    assert fpath == (fwd, int(c["p"] > 0), mk, c["ext"] is not None, False), fpath
    # the forward's own tolerance, as in tests/test_gpu_attn7.py
    q, k, v, do = (attn_heads(x[n], B, H) for n in ("q", "k", "v", "do"))
    smax = (q.double() @ k.double().transpose(-1, -2)).abs().max().item() * SCALE
    close(od.float(), attn_rows(o64), rtol=2e-2, what=f"{fwd} out")
    close(lse.view(B, H, Lq), lse64, rtol=0, atol=max(LSE_ATOL, 2.0 ** -8 * smax), what=f"{fwd} lse")
    got = _backward(c, d, od, lse, db)
    oh, lh = attn_heads(od.float().cpu(), B, H), lse.cpu().view(B, H, Lq)
    t = attn_bwd_ref64(q, k, v, do, oh, lh, x["keep"], x["drop"], attn_p32(c["p"]), SCALE)
    _check(c, kind, f"chained-{fwd}", got, t, attn_bwd_units(t, q, k, v, do, oh, SCALE), x["keep"])
