"""Every element of O and LSE of the attention forward kernels against the float64 reference of the operation the C ABI
defines (helpers.attn_fwd_terms64), within the per-element bounds

    |O_gpu - O_ref|     <= C_O u b_O + rel |O_ref| + lin_O
    |LSE_gpu - LSE_ref| <= C_L u b_LSE + lin_LSE

of helpers.attn_fwd_units (u = 2^-9, rel = 2^-8 for the bf16 families; u = 2^-24, rel = 0 for the f32 kernel; lin = the
gate's own bound and the written-out fp32 floor), whose constants tests/test_cpu_attn_fwd_ref.py settles from the
reference alone (E from an emulation of each family's rounding points, C = 2 E; sixteen mutated references that must
leave the bound). Kernels: fwd7 <DM, MK, REL, KX> (csrc/attn7.hip), fwd8 <DM, MK> with its fallback (csrc/attn8.hip),
fwd6 <DM, MK>, fwd2 <DROP, MASK>, fwd5 <MASK> and the generic f32 kernel (csrc/attention.hip), every build the
dispatcher can launch, through ops.attn_fwd (with and without key_len, gate and table), ops.attn_fwd_relgate and
ops.attn_fwd_relgate_x. Each test asserts through ops.attn_last_path() the kernel and the build it meant to reach.

Without exception: O and LSE are pre-filled with NaN; NaN sits exactly where the reference has it (entries without a
key) and everything else is finite; NaN-filled guard columns around O keep their bits. Where the forward writes the
keep bits itself (an unwritten buffer, and fwd2's / fwd6's own words) they decode to the oracle's bits exactly (under
fwd6 at every kept key: it writes no words for a key tile it skips as fully masked). The LSE is checked wherever the entry point returns one (fddm_attn_fwd_relgate and _relgate_x return none).

Each test prints the kernel's worst error in units of u b per output. Largest seen on an MI355X (O / LSE, every input
set): fwd7 4.07 / 3.29 and its REL builds 3.62 / 3.14 against C = 8.2 / 7.3; fwd8 4.07 / 3.22 (its guard cases 3.63 /
2.41) against C = 8.6 / 6.8; fwd6 3.68, fwd2 3.46 and fwd5 3.16 against C = 7.2, their fp32 LSE never outside the
written-out floor (C = 0.1 on top of it); the generic f32 kernel 2.30, with gate and table 2.91, against C = 5.5 in
units of 2^-24, its LSE likewise inside the floor.
"""
import pytest
import torch

from helpers import (ATTN_FWD_C, ATTN_SEED, ATTN_STREAM, attn_fwd_case_inputs, attn_fwd_case_ref, attn_fwd_cases,
                     attn_fwd_excess, attn_heads)

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
bf = torch.bfloat16
CASES = attn_fwd_cases()
BY_ID = {c["id"]: c for c in CASES}
NAN = float("nan")


def ops():
    from fddm_hip import ops as o
    return o


def _bits_of(t):
    return t.view(torch.int16 if t.dtype == bf else torch.int32).clone()


def _decode_words(c, db, kernel):
    """The keep bits [B H, Lq, Lk] the forward left in `db`: the round-4 words of fwd6 / fwd2 (bit kk of word
    (bh, t, q) = keep(q, key 64 t + kk)) or the 32x32x16 family's lane masks (layout v3) and per-lane dwords (v5)."""
    from test_gpu_kernels import _decode_v3, _decode_v5
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    nt, w = (Lk + 63) // 64, db.cpu()
    if kernel in ("fwd6", "fwd2"):
        words = w[:B * H * nt * Lq].view(B * H, nt, Lq)
        bits = ((words[..., None] >> torch.arange(64, dtype=torch.int64)) & 1).bool()
        return [bits.permute(0, 2, 1, 3).reshape(B * H, Lq, nt * 64)[:, :, :Lk]]
    n3 = B * H * ((Lq + 31) // 32) * nt * 32
    lw = w[n3:2 * n3]
    dw = torch.stack([lw & 0xFFFFFFFF, (lw >> 32) & 0xFFFFFFFF], -1).reshape(-1)
    return [_decode_v3(w[:n3], B * H, Lq, Lk), _decode_v5(dw, B * H, Lq, Lk)]


def _forward(c, x):
    """The case's entry point on device tensors; returns (O float64 [B, H, Lq, 64], LSE float64 [B, H, Lq] or None) on
    the CPU and asserts the path, the guard columns and the keep bits a forward wrote."""
    o = ops()
    B, H, Lq, Lk, p = c["B"], c["H"], c["Lq"], c["Lk"], c["p"]
    D = H * 64
    dt = torch.float32 if c["f32"] else bf
    to = lambda t, L: t.reshape(B * L, D).to(dev, dt)  # noqa: E731
    if c["strided"] or c["rel"]:    # the fused projection's buffer: q | k | v side by side, row stride 3 D
        buf = torch.zeros(B * max(Lq, Lk), 3 * D, device=dev, dtype=dt)
        buf[: B * Lq, :D] = to(x["q"], Lq)
        buf[: B * Lk, D: 2 * D] = to(x["k"], Lk)
        buf[: B * Lk, 2 * D:] = to(x["v"], Lk)
        q, k, v = buf[: B * Lq, :D], buf[: B * Lk, D: 2 * D], buf[: B * Lk, 2 * D:]
    else:
        q, k, v = (to(x[n], L).contiguous() for n, L in (("q", Lq), ("k", Lk), ("v", Lk)))
    pad = 8 if c["guard"] else 0
    wide = torch.full((B * Lq, D + 2 * pad), NAN, device=dev, dtype=dt)     # NaN: never-written elements show
    before = _bits_of(wide)
    out = wide[:, pad: pad + D]
    lse = torch.full((B * H, Lq), NAN, device=dev) if c["has_lse"] else None
    kk = x["keep"].to(dev).to(torch.uint8).contiguous() if x["keep"] is not None else None
    kl = o.key_extent(kk) if c["ext"] is not None else None
    old = o.attn_force_kernels(c["force"])
    try:
        db = None
        if c["bits"] in ("ready", "own"):
            db = torch.zeros(o.drop_words(B, H, Lq, Lk), device=dev, dtype=torch.int64)
            if c["bits"] == "ready":       # the producer writes the selected family's storage layout
                o.attn_drop_bits(db.view(1, -1), 1, B, H, Lq, Lk, p, ATTN_SEED, ATTN_STREAM, 0)
        if c["src"] in (None, "gate"):
            gate = x["gate"].to(dev).contiguous() if c["rel"] else None
            table = x["table"].to(dev).contiguous() if c["rel"] else None
            o.attn_fwd(q, k, v, out, lse, B, H, Lq, Lk, key_keep=kk, gate=gate, table=table, drop_p=p, seed=ATTN_SEED,
                       rng_stream=ATTN_STREAM, dbits=db, bits_ready=c["bits"] == "ready", key_len=kl)
        elif c["src"] == "graw":           # 8 pre-activations per (token, head) with a padded row stride
            gbuf = torch.zeros(B * Lq, 8 * H + 8, device=dev, dtype=bf)
            gbuf[:, :8 * H] = x["graw"].to(dev, bf)
            o.attn_fwd_relgate(q, k, v, out, gbuf, x["gconst"].to(dev), x["table"].to(dev), B, H, Lq)
        else:                              # the attention input with a padded row stride
            xbuf = torch.zeros(B * Lq, D + 64, device=dev, dtype=bf)
            xbuf[:, :D] = x["x"].to(dev, bf)
            o.attn_fwd_relgate_x(q, k, v, out, xbuf[:, :D], x["gw"].to(dev), x["gconst"].to(dev), x["table"].to(dev),
                                 B, H, Lq, key_keep=kk if kl is not None else None, key_len=kl)
        path = o.attn_last_path()["fwd"]
    finally:
        o.attn_force_kernels(old)
    torch.cuda.synchronize()
    assert path == c["expect"], (path, c["expect"])
    if pad:
        now = _bits_of(wide)
        assert torch.equal(now[:, :pad], before[:, :pad]) and torch.equal(now[:, pad + D:], before[:, pad + D:]), \
            "O: guard columns changed"
    if c["bits"] == "own":
        # every key; under fwd6 every kept key: it writes no words for a key tile it skips as fully masked (no kernel
        # reads the bit of a masked key)
        kept = torch.ones(B, Lk, dtype=torch.bool)
        if c["kernel"] == "fwd6" and x["keep"] is not None:
            kept = x["keep"]
        kept = kept[:, None, None, :].expand(B, H, Lq, Lk).reshape(B * H, Lq, Lk)
        ref = x["drop"].reshape(B * H, Lq, Lk)
        for i, got in enumerate(_decode_words(c, db, c["kernel"])):
            diff = (got != ref) & kept
            assert not diff.any(), f"keep bits (layout {i}): {diff.sum().item()} differ from the oracle's"
    return (attn_heads(out.float().cpu().double(), B, H),
            lse.cpu().double().view(B, H, Lq) if lse is not None else None)


@pytest.mark.parametrize("cid,kind", [(c["id"], kd) for c in CASES for kd in c["kinds"]])
def test_attn_fwd_matches_float64_per_element(cid, kind):
    c, x = BY_ID[cid], attn_fwd_case_inputs(cid, kind)
    r, U, _ = attn_fwd_case_ref(cid, kind)
    got_o, got_lse = _forward(c, x)
    C = ATTN_FWD_C[c["family"]]
    checks = [("o", got_o, r.O, U["b_o"], U["rel"], U["lin_o"])]
    if got_lse is not None:
        checks.append(("lse", got_lse, r.LSE, U["b_lse"], 0.0, U["lin_lse"]))
    worst, fails = {"lse": float("nan")}, []
    for n, got, ref, b, rel, lin in checks:
        ex = attn_fwd_excess(got, ref, b, U["u"], rel, lin)
        worst[n] = ex.max().item()
        wrong_nan = torch.isnan(got) != torch.isnan(ref)
        if wrong_nan.any():
            fails.append(f"{n}: {wrong_nan.sum().item()} elements NaN where the reference is not, or the reverse; first "
                         f"{wrong_nan.nonzero()[:4].tolist()}")
        elif not torch.isfinite(got[~torch.isnan(ref)]).all():
            fails.append(f"{n}: infinite values")
        bad = ex > C[n]
        if bad.any():
            idx = bad.nonzero()
            fails.append(f"{n}: {idx.shape[0]} of {bad.numel()} elements outside C = {C[n]:.2f} (worst {worst[n]:.2f} "
                         f"u b); first (b,h,row[,col]) {idx[:6].tolist()}, rows {sorted(set(idx[:, 2].tolist()))[:12]}")
    print(f"ATTNFWD fam={c['expect'][0]} id={cid} kind={kind} o={worst['o']:.3f} lse={worst['lse']:.3f}")
    assert not fails, "; ".join(fails)
