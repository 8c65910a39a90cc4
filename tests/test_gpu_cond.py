"""The decoder's conditioning kernels (linear4_kernel, linrt_kernel, dw_kernel, rows_mean_kernel,
rows_mean_masked_kernel, time_embed_kernel: csrc/small.hip) and RoPE and the token embedding (rope_fwd / rope_bwd, vector
and scalar, embed_fwd, embed_bwd: csrc/misc.hip) per element against float64. They feed every decoder block: t_bias, the
FiLM scale / shift, x = E[tok] + t_bias, RoPE.

Cases (helpers.LIN_CASES, dw_cases(), RM_S x RM_D, TE_D x TE_T, ROPE_CASES, EMBED_CASES): the smallest shapes at which each
mechanism exists. linear4 with one, two (ragged, K % 4 = 3) and four 512-chunks (the prefetch and the second stash), a
second row tile, the smallest shape, input rows off and on a 16-byte boundary; linrt with waves making three trips, a
12-wide last chunk, under one chunk, the transposed build's scalar edge and rows off 16 bytes; 24 weight sets, split by
ops into a linrt and a linear4 launch, and into two linrt launches; every case with both weight layouts and act 0 / 1
/ 2, two of them without a bias. The kernel of every launch is asserted from the tile count (helpers.lin_dispatch).
small_dw with jobs of four shapes in one launch (the grid is sized by the largest, the others return early), at 45, 1
and 64 rows, db given and None, dW and db non-zero, dy a column slice of a wider buffer, and a 17-job call. rows_mean
through its four-fold unrolled loop (S > 96) at the workload's S = 499, d = 72 on the vector path and 130 on the scalar
one, f32 and bf16; the masked kernel bit-equal to it under an all-ones mask, and with holes over NaN rows.
time_embed at d = 2 .. 5, 129, 512 and t = 0 .. 1000. RoPE on the vector kernels, on the scalar ones at d = 2, 6 and at
d = 128 through views one element into a buffer, f32 and bf16 output, the backward onto a non-zero dx. The embedding at d
= 8, 520 (the column loop's third trip), 6 (scalar forward), L = 1, 3, 9, five- and fifty-entry vocabularies, pad_id 0 and
3, a block of eight padding rows, and each optional argument absent.

Inputs carry a power of two per row and per column (2^-2 .. 2^2), so a quiet element meets loud neighbours. Every output
is written into a buffer with guard elements behind it, which must keep their bits.

Bounds, per element, with u = 2^-24 (helpers.lin_out64, dw_ref64, rm_ref64, te_ref64, rope_fwd_ref64, rope_bwd_ref,
embed_bwd_ref64):
    out, pre            C_lin u s                                         s = sum_k |in| |W| + |b|
    silu(pre)           |silu'(y)| C_lin u s + C_silu u |silu(y)| + 2^-121
    act 2               |g| C_lin u s0 + |y0| C_g u (1 + |aux|)           g = silu'(aux), y0 and s0 without the bias
    dW, db              C_dw u s                                          s = |old| + |dy|^T |x|, |old| + sum_r |dy|
    rows_mean           C_rm u s                                          s = the mean of |x| over the (kept) rows
    time_embed          C_te u (|a| (1 + lin_k) + 1)                      a = t f_k, f_k = exp(-lin_k)
    rope_fwd            2 u (|x1 c| + |x2 s'|), then bf16 for a bf16 output
    rope_bwd            3 u (|dx| + |a C| + |b S|)
    embed_fwd           the bits of torch's fp32 E[tok] + tbias[r // L]; out_t its .to(bfloat16)
    embed_bwd           n u (|old| + sum |dx|), n the contributions (n = 0: the old bits); dtb with n = L + 1
C = 8 E, E measured on the CPU from the reference alone (tests/test_cpu_cond_ref.py, which also proves that the listed
mutants of each family leave these bounds on at least half of the elements they change):
    C_lin = 45.6   C_dw = 42.4   C_rm = 26.4   C_te = 9.6   C_silu = 20.4   C_g = 11.6     (hard cap 64)

Measured on an MI355X (the CONDNEED lines this file prints): "units" is the largest |out - ref| over the family's unit
u s (the C it needed; none for silu and act 2, where two units add, and for the bf16 outputs), "share" the largest share of
its bound any element used. A correctly rounded bf16 output next to a rounding boundary uses its whole half ulp.
    path                 units    share of bound
    linear4 pre           4.47    0.098     (of C_lin = 45.6)
    linear4 silu / act 2  -       0.107 / 0.073
    linrt pre             4.68    0.103
    linrt silu / act 2    -       0.107 / 0.081
    dw dW / db            4.83 / 2.90    0.114 / 0.068     (of C_dw = 42.4)
    rows_mean f32 / bf16  3.00 / 1.03    0.114 / 0.039     (of C_rm = 26.4)
    masked f32 / bf16     2.00 / 0.84    0.076 / 0.032
    time_embed            1.11    0.115     (of C_te = 9.6)
    rope fwd f32          1.59 vector, 1.81 scalar (of 2);  bf16 1.000
    rope bwd              1.79 vector, 1.64 scalar (of 3)
    embed_bwd dE / dtb    1.91 of n / 2.73 of L + 1
On the parent commit's kernel the d = 2 and d = 3 time_embed cases leave the bound by a factor 7e5 (sin(1e-4) for sin(1)).
"""
import re

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
F32 = torch.float32
NEED = {}          # row -> [units, share]
assert all(v <= 64.0 for v in H.COND_C.values())


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    for k in sorted(NEED):
        units = f"{NEED[k][0]:6.2f}" if NEED[k][0] >= 0 else "     -"
        print(f"\nCONDNEED {k:<22} units {units}  share {NEED[k][1]:5.3f}", end="")
    print()


def _ops():
    from fddm_hip import ops
    return ops


def _check(row, what, out, ref, bound, unit=None):
    """Every element of out (any device) within bound of ref (CPU float64); a bound of 0 asks for the reference's bits.
    Records the row's largest share of the bound and, with unit (the per-element u s), the C it needed."""
    out = out.detach().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out.double() - ref).abs()
    rel = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    share = rel.max().item() if rel.numel() else 0.0
    units = -1.0
    if unit is not None:
        ok = unit > 0
        units = (err[ok] / unit[ok]).max().item() if ok.any() else 0.0
    n = NEED.setdefault(row, [-1.0, 0.0])
    n[0], n[1] = max(n[0], units), max(n[1], share)
    bad = err > bound
    if bad.any():
        at = np.unravel_index(int(rel.argmax()), tuple(err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements leave their bound, the worst by a "
                             f"factor {share:.2f} at {tuple(int(i) for i in at)}: got {out[at].item()!r}, reference "
                             f"{ref[at].item()!r}")


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


class _Guards:
    """Output buffers with guard elements behind (and optionally before) them; check() after the kernels ran."""

    def __init__(self):
        self.kept = []

    def new(self, shape, dtype=F32, init=None, lead=0):
        n = int(np.prod(shape))
        buf = torch.full((lead + n + 64,), float("nan"), dtype=dtype, device=dev)
        view = buf[lead:lead + n].view(*shape)
        if init is not None:
            view.copy_(init)
        self.kept.append((buf, lead, n, _bits(buf[:lead]), _bits(buf[lead + n:])))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for buf, lead, n, front, back in self.kept:
            assert torch.equal(_bits(buf[:lead]), front) and torch.equal(_bits(buf[lead + n:]), back), \
                f"{what}: wrote outside its output"


def _refused(fn, bad):
    """Every (message, arguments) row raises the ValueError of the precondition it names."""
    for msg, a in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            fn(*a)


# ------------------------------------------------------------------------------------------ the linear family
@pytest.mark.parametrize("case", H.LIN_CASES, ids=[c[0] for c in H.LIN_CASES])
def test_small_linear(case):
    cid, kernels, R, K, N, J, pads, given = case
    o = _ops()
    assert H.lin_dispatch(R, N, J) == kernels, "the case must run the kernels it names"
    x, W, b, aux = H.lin_operands(cid)
    r = H.lin_ref64(cid)
    u_s = H.U24 * r.s
    auxd = aux.to(dev)
    bs = [b[j].to(dev) for j in range(J)] if given else None
    for pad in pads:
        xb = torch.full((R, K + pad), float("nan"), device=dev)
        xb[:, :K] = x.to(dev)
        inp = xb[:, :K]
        assert inp.stride(0) == K + pad
        for tw in (False, True):
            Ws = [(W[j].t() if tw else W[j]).contiguous().to(dev) for j in range(J)]
            for act in (0, 1, 2):
                g = _Guards()
                outs = [g.new((R, N)) for _ in range(J)]
                outs2 = [g.new((R, N)) for _ in range(J)] if act == 1 else None
                o.small_linear(inp, Ws, bs, outs, outs2, act=act, aux=auxd if act == 2 else None, transpose_w=tw)
                what = f"small_linear {cid} pad={pad} tw={int(tw)} act={act}"
                g.check(what)
                got = torch.stack(outs, 1)
                for i, kern in enumerate(kernels):
                    sl = slice(16 * i, 16 * i + 16)
                    if act == 2:
                        _check(f"{kern} act2", what, got[:, sl], r.dx[:, sl], r.b_dx[:, sl])
                    else:
                        _check(f"{kern} pre", what, got[:, sl], r.pre[:, sl], r.b_pre[:, sl], u_s[:, sl])
                    if act == 1:
                        _check(f"{kern} silu", what + " silu", torch.stack(outs2, 1)[:, sl], r.silu[:, sl], r.b_silu[:, sl])


# ------------------------------------------------------------------------------------------ small_dw
@pytest.mark.parametrize("case", H.dw_cases(), ids=[c[0] for c in H.dw_cases()])
def test_small_dw(case):
    cid, R, shapes = case
    o = _ops()
    g = _Guards()
    jobs, refs = [], []
    for (N, K, given), (dyb, x, dW, db) in zip(shapes, H.dw_operands(cid)):
        dy = dyb.to(dev)[:, 1:1 + N]
        assert dy.stride(0) == N + H.DW_PAD and tuple(dy.shape) == (R, N)
        jobs.append((dy, x.to(dev), g.new((N, K), init=dW), g.new((N,), init=db) if given else None))
        refs.append(H.dw_ref64(dyb[:, 1:1 + N], x, dW, db))
    assert len({j[2].shape for j in jobs}) > 1 or len(jobs) > H.LIN_MAXJ
    assert any(j[2].data_ptr() % 16 or j[2].shape[1] % 4 for j in jobs), "a dW row off 16 bytes"
    o.small_dw(jobs)
    g.check(f"small_dw {cid}")
    for j, ((dy, x, dW, db), r) in enumerate(zip(jobs, refs)):
        _check("dw dW", f"small_dw {cid} job {j} dW", dW, r.dW, r.b_dW, H.U24 * r.sW)
        if db is not None:
            _check("dw db", f"small_dw {cid} job {j} db", db, r.db, r.b_db, H.U24 * r.sb)


# ------------------------------------------------------------------------------------------ rows_mean
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("S", H.RM_S)
def test_rows_mean(S, dt):
    o = _ops()
    for d in H.RM_D:
        x = H.rm_operands(S, d, dt)
        r = H.rm_ref64(x)
        xd = x.to(dev)
        out = o.rows_mean(xd)
        assert out.dtype == F32 and out.shape == (H.RM_B, d)
        _check(f"rows_mean {dt}", f"rows_mean S={S} d={d} {dt}", out, r.mean, r.b, H.U24 * r.s)
        if S in H.RM_MASKED_EQ:      # all kept: the unmasked kernel's bits (same slices, same order)
            ones = torch.ones(H.RM_B, S, dtype=torch.uint8, device=dev)
            assert torch.equal(o.rows_mean_masked(xd, ones), out), f"S={S} d={d} {dt}"
            assert torch.equal(o.rows_mean_masked(xd, ones, clamp=True), out), f"S={S} d={d} {dt}"
        if S == H.RM_HOLES_S:
            keep = H.rm_holes(S)
            xh = x.clone()
            xh[keep == 0] = float("nan")          # padded rows are not read
            rh = H.rm_ref64(xh, keep)
            got_u = o.rows_mean_masked(xh.to(dev), keep.to(dev), clamp=False)
            got_c = o.rows_mean_masked(xh.to(dev), keep.to(dev), clamp=True)
            for got in (got_u, got_c):
                _check(f"rows_mean_masked {dt}", f"rows_mean_masked S={S} d={d} {dt}", got[:1], rh.mean[:1], rh.b[:1],
                       H.U24 * rh.s[:1])
            # nothing kept: NaN unclamped (the reference's 0 / 0), 0 under the clamp
            assert torch.isnan(got_u[1]).all() and (got_c[1] == 0).all()


# ------------------------------------------------------------------------------------------ time_embed
@pytest.mark.parametrize("d", H.TE_D)
def test_time_embed(d):
    """d = 2 and 3 (half = 1) fail on a kernel that takes linspace's end point for its only frequency: sin(1e-4 t) for
    sin(t)."""
    o = _ops()
    t = torch.tensor(H.TE_T)
    r = H.te_ref64(t, d)
    out = o.time_embed(t.to(dev), d, H.TE_MAX_STEPS)
    assert out.dtype == F32 and out.shape == (len(H.TE_T), d)
    _check("time_embed", f"time_embed d={d}", out, r.emb, r.b, r.unit)
    if d % 2:
        assert (out[:, -1] == 0).all(), "the padding column of an odd d is exactly 0"


# ------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("case", H.ROPE_CASES, ids=["-".join(map(str, c[:3])) + ("-off" if c[3] else "") for c in H.ROPE_CASES])
def test_rope(case):
    N, L, d, off = case
    o = _ops()
    x, dy, dx0, cos, sin = H.rope_operands(N, L, d)
    f, bk = H.rope_fwd_ref64(x, cos, sin, L), H.rope_bwd_ref(dy, dx0, cos, sin, L)
    cs, sn = cos.to(dev), sin.to(dev)
    lead = 1 if off else 0
    g = _Guards()
    xin, dyin = g.new((N, d), init=x, lead=lead), g.new((N, d), init=dy, lead=lead)
    row = "rope vector" if H.rope_kernel_is_vector(d, off) else "rope scalar"
    for dt in (F32, BF):
        out = g.new((N, d), dtype=dt, lead=lead)
        aligned = all(t.data_ptr() % 16 == 0 for t in (xin, out, cs, sn))
        assert (d % 8 == 0 and aligned) == H.rope_kernel_is_vector(d, off), "the case must run the kernel it names"
        assert o.rope_fwd(xin, cs, sn, out, L) is out
        b = f.b if dt == F32 else H.bf16_round_bound(f.out, f.b)
        _check(f"{row} fwd {'f32' if dt == F32 else 'bf16'}", f"rope_fwd {case} {dt}", out, f.out, b,
               f.b / 2.0 if dt == F32 else None)
    dx = g.new((N, d), init=dx0, lead=lead)
    o.rope_bwd(dyin, cs, sn, dx, L)
    g.check(f"rope {case}")
    _check(f"{row} bwd", f"rope_bwd {case}", dx, bk.dx, bk.b, bk.b / 3.0)
    assert torch.equal(xin.cpu(), x) and torch.equal(dyin.cpu(), dy), "inputs are not written"


# ------------------------------------------------------------------------------------------ token embedding
@pytest.mark.parametrize("case", H.EMBED_CASES, ids=["-".join(map(str, c)) for c in H.EMBED_CASES])
def test_embedding(case):
    d, L, B, V, pad = case
    o = _ops()
    tok, E, tb, dx, dE0, dtb0 = H.embed_operands(*case)
    N = B * L
    tokd, Ed, tbd, dxd = tok.to(dev), E.to(dev), tb.to(dev), dx.to(dev)
    g = _Guards()
    # ---- forward: one IEEE add per element
    for tbias, tbias_d in ((tb, tbd), (None, None)):
        want = H.embed_fwd_exact(tok, E, tbias, L)
        for out_dt in (BF, F32):
            out, out_t = g.new((N, d)), g.new((N, d), dtype=out_dt)
            o.embed_fwd(tokd, Ed, tbias_d, out, out_t, L)
            assert torch.equal(out.cpu(), want), f"embed_fwd {case}: out is E[tok] + tbias bit for bit"
            assert torch.equal(out_t.cpu(), want.to(out_dt)), f"embed_fwd {case}: out_t is that value's {out_dt}"
        only_t = g.new((N, d), dtype=BF)
        o.embed_fwd(tokd, Ed, tbias_d, None, only_t, L)
        assert torch.equal(only_t.cpu(), want.to(BF)), f"embed_fwd {case}: out = None"
        only = g.new((N, d))
        o.embed_fwd(tokd.view(B, L), Ed, tbias_d, only, None, L)
        assert torch.equal(only.cpu(), want), f"embed_fwd {case}: out_t = None"
    # ---- backward onto non-zero dE / dtb
    r = H.embed_bwd_ref64(tok, dx, dE0, dtb0, L, pad)
    for with_dE, with_dtb in ((True, True), (False, True), (True, False)):
        dE = g.new((V, d), init=dE0) if with_dE else None
        dtb = g.new((B, d), init=dtb0) if with_dtb else None
        o.embed_bwd(tokd, dxd, dE, dtb, L, pad)
        what = f"embed_bwd {case} dE={int(with_dE)} dtb={int(with_dtb)}"
        if with_dE:
            _check("embed_bwd dE", what, dE, r.dE, r.b_dE, r.b_dE / r.n.clamp(min=1)[:, None])
            idle = r.n == 0
            assert idle[pad] and torch.equal(_bits(dE.cpu()[idle]), _bits(dE0[idle])), \
                f"{what}: the padding row and unnamed rows keep their bits"
        if with_dtb:
            _check("embed_bwd dtb", what, dtb, r.dtb, r.b_dtb, r.b_dtb / (L + 1))
    g.check(f"embedding {case}")


# ------------------------------------------------------------------------------------------ refusals (no launch)
def _z(*shape, dtype=F32):
    return torch.zeros(*shape, device=dev, dtype=dtype)


def test_rope_refuses_bad_arguments():
    o = _ops()
    N, L, d = 6, 3, 8
    x, cs, sn, out = _z(N, d), _z(L, d), _z(L, d), _z(N, d)
    for name, fn, odt in (("rope_fwd", o.rope_fwd, "float32 or bfloat16"), ("rope_bwd", o.rope_bwd, "float32")):
        IN, OUT, TAB = f"{name}: input is contiguous f32 [N, d]", f"{name}: output is contiguous [N, d], {odt}", \
            f"{name}: cos and sin are contiguous f32 [>= L, d]"
        bad = [
            (IN, (x.view(2, 3, d), cs, sn, out, L)),                          # not 2-D
            (IN, (_z(N, 2 * d)[:, ::2], cs, sn, out, L)),                     # not contiguous
            (IN, (x.double(), cs, sn, out, L)),                               # not f32
            (f"{name}: d is even", (_z(N, 7), _z(L, 7), _z(L, 7), _z(N, 7), L)),
            (f"{name}: L >= 1", (x, cs, sn, out, 0)),
            (OUT, (x, cs, sn, _z(N + 1, d), L)),                              # another shape
            (OUT, (x, cs, sn, _z(d, N).t(), L)),                              # not contiguous
            (OUT, (x, cs, sn, _z(N, d, dtype=torch.float16), L)),             # neither f32 nor bf16
            (TAB, (x, cs.double(), sn, out, L)),                              # cos not f32
            (TAB, (x, cs, _z(L, 2 * d)[:, ::2], out, L)),                     # sin not contiguous
            (TAB, (x, cs, sn[: L - 1], out, L)),                              # fewer than L rows
            (TAB, (x, _z(L, d + 2), sn, out, L)),                             # another d
            (TAB, (x, cs.view(-1), sn, out, L)),                              # not 2-D
            (f"{name}: every tensor on one GPU", (x, cs.cpu(), sn, out, L)),
            (f"{name}: every tensor on one GPU", (x.cpu(), cs.cpu(), sn.cpu(), out.cpu(), L)),
        ]
        if name == "rope_bwd":
            bad.append((OUT, (x, cs, sn, _z(N, d, dtype=BF), L)))             # dx is f32
        _refused(fn, bad)


def test_rope_bwd_entry_point_refuses_an_odd_width():
    """fddm_rope_bwd itself returns hipErrorInvalidValue for an odd d, as fddm_rope_fwd does (no launch)."""
    from fddm_hip._lib import lib
    o = _ops()
    N, L, d = 4, 2, 5
    dy, cs, sn, dx = _z(N, d), _z(L, d), _z(L, d), _z(N, d)
    inval = 1                                                               # hipErrorInvalidValue
    assert lib().fddm_rope_bwd(dy.data_ptr(), cs.data_ptr(), sn.data_ptr(), dx.data_ptr(), N, L, d, o.stream()) == inval
    assert lib().fddm_rope_fwd(o.F32, dy.data_ptr(), cs.data_ptr(), sn.data_ptr(), dx.data_ptr(), N, L, d,
                               o.stream()) == inval


def test_embedding_refuses_bad_arguments():
    o = _ops()
    B, L, V, d = 2, 3, 5, 8
    N = B * L
    tok, E, tb, out, out_t = _z(N, dtype=torch.int64), _z(V, d), _z(B, d), _z(N, d), _z(N, d, dtype=BF)
    TOK, TAB, TB = "embed_fwd: tokens are contiguous int64", "embed_fwd: the table is contiguous f32 [V, d]", \
        "embed_fwd: tbias is contiguous f32 [>= ceil(N / L), d]"
    OUT, OUTT, DEV = "embed_fwd: out is contiguous [N, d], float32", \
        "embed_fwd: out_t is contiguous [N, d], float32 or bfloat16", "embed_fwd: every tensor on one GPU"
    _refused(o.embed_fwd, [
        (TOK, (tok.int(), E, tb, out, out_t, L)),                             # not int64
        (TOK, (_z(2 * N, dtype=torch.int64)[::2], E, tb, out, out_t, L)),     # not contiguous
        ("embed_fwd: L >= 1", (tok, E, tb, out, out_t, 0)),
        (TAB, (tok, None, tb, out, out_t, L)),
        (TAB, (tok, E.double(), tb, out, out_t, L)),                          # not f32
        (TAB, (tok, _z(d, V).t(), tb, out, out_t, L)),                        # not contiguous
        (TAB, (tok, E.view(-1), tb, out, out_t, L)),                          # not 2-D
        (TB, (tok, E, tb.double(), out, out_t, L)),                           # not f32
        (TB, (tok, E, _z(B, 2 * d)[:, ::2], out, out_t, L)),                  # not contiguous
        (TB, (tok, E, tb[:1], out, out_t, L)),                                # fewer than ceil(N / L) rows
        (TB, (tok, E, _z(B, d + 8), out, out_t, L)),                          # another d
        (OUT, (tok, E, tb, _z(N + 1, d), out_t, L)),                          # not [N, d]
        (OUT, (tok, E, tb, _z(d, N).t(), out_t, L)),                          # not contiguous
        (OUT, (tok, E, tb, out.double(), out_t, L)),                          # not f32
        (OUTT, (tok, E, tb, out, _z(N, d, dtype=torch.float16), L)),          # neither f32 nor bf16
        (OUTT, (tok, E, tb, out, _z(N, d + 8, dtype=BF), L)),                 # not [N, d]
        (DEV, (tok, E.cpu(), tb, out, out_t, L)),
        (DEV, (tok.cpu(), E.cpu(), tb.cpu(), out.cpu(), out_t.cpu(), L)),
    ])
    dx, dE, dtb = _z(N, d), _z(V, d), _z(B, d)
    TOK, TAB, TB = "embed_bwd: tokens are contiguous int64", "embed_bwd: the table is contiguous f32 [V, d]", \
        "embed_bwd: dtb is contiguous f32 [>= ceil(N / L), d]"
    DX, DEV = "embed_bwd: dx is contiguous [N, d], float32", "embed_bwd: every tensor on one GPU"
    _refused(o.embed_bwd, [
        (TOK, (tok.int(), dx, dE, dtb, L, 0)),
        (TOK, (_z(2 * N, dtype=torch.int64)[::2], dx, dE, dtb, L, 0)),
        ("embed_bwd: L >= 1", (tok, dx, dE, dtb, 0, 0)),
        (DX, (tok, dx.view(-1), dE, dtb, L, 0)),                              # not 2-D
        (DX, (tok, dx.double(), dE, dtb, L, 0)),                              # not f32
        (DX, (tok, _z(N, 2 * d)[:, ::2], dE, dtb, L, 0)),                     # not contiguous
        (DX, (tok, _z(N + 1, d), dE, dtb, L, 0)),                             # N is not the token count
        (TAB, (tok, dx, dE.double(), dtb, L, 0)),                             # dE not f32
        (TAB, (tok, dx, _z(V, d + 8), dtb, L, 0)),                            # dE of another d
        (TAB, (tok, dx, _z(d, V).t(), dtb, L, 0)),                            # dE not contiguous
        (TB, (tok, dx, dE, dtb[:1], L, 0)),                                   # fewer than ceil(N / L) rows
        (TB, (tok, dx, dE, dtb.double(), L, 0)),                              # not f32
        (TB, (tok, dx, dE, _z(B, 2 * d)[:, ::2], L, 0)),                      # not contiguous
        (DEV, (tok, dx, dE.cpu(), dtb, L, 0)),
        (DEV, (tok.cpu(), dx.cpu(), dE.cpu(), dtb.cpu(), L, 0)),
    ])


def test_small_linear_refuses_bad_arguments():
    o = _ops()
    R, K, N = 3, 8, 5
    x, W, b, out, out2, aux = _z(R, K), _z(N, K), _z(N), _z(R, N), _z(R, N), _z(R, N)
    AUX, O2, BIAS = "small_linear: act 2 reads aux, contiguous f32 [R, N]", "small_linear: outs2 are contiguous f32 [R, N]", \
        "small_linear: biases are contiguous f32 [N]"
    NO2, DEV = "small_linear: act 1 writes silu into outs2, one per output", "small_linear: every tensor on one GPU"

    def call(inp, Ws, bs, outs, outs2, act, aux_):
        o.small_linear(inp, Ws, bs, outs, outs2, act=act, aux=aux_)

    _refused(call, [
        (AUX, (x, [W], [b], [out], None, 2, None)),                           # absent
        (AUX, (x, [W], [b], [out], None, 2, aux.double())),                   # not f32
        (AUX, (x, [W], [b], [out], None, 2, _z(N, R).t())),                   # not contiguous
        (AUX, (x, [W], [b], [out], None, 2, _z(R, N + 1))),                   # not [R, N]
        (NO2, (x, [W], [b], [out], None, 1, None)),                           # absent
        (NO2, (x, [W, W], [b, b], [out, out], [out2], 1, None)),              # one for two outputs
        (O2, (x, [W], [b], [out], [_z(R + 1, N)], 1, None)),                  # not shaped like outs
        (O2, (x, [W], [b], [out], [out2.double()], 1, None)),                 # not f32
        (O2, (x, [W], [b], [out], [_z(N, R).t()], 1, None)),                  # not contiguous
        (BIAS, (x, [W], [b.double()], [out], None, 0, None)),                 # not f32
        (BIAS, (x, [W], [_z(2 * N)[::2]], [out], None, 0, None)),             # not contiguous
        (BIAS, (x, [W], [_z(N + 1)], [out], None, 0, None)),                  # not [N]
        ("small_linear: one bias per weight set", (x, [W, W], [b], [out, out2], None, 0, None)),
        ("small_linear: one output per weight set", (x, [W, W], [b, b], [out], None, 0, None)),
        (DEV, (x, [W], [b.cpu()], [out], None, 0, None)),
        (DEV, (x, [W.cpu()], [b], [out], None, 0, None)),
        (DEV, (x, [W], [b], [out], None, 2, aux.cpu())),
        (DEV, (x, [W], [b], [out], [out2.cpu()], 1, None)),
        (DEV, (x.cpu(), [W.cpu()], [b.cpu()], [out.cpu()], None, 0, None)),
    ])
