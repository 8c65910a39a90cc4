"""Every GEMM kernel family per element against float64: the register-staged 128x128 kernel and its grouped form, the
256x128 "big" LDS-DMA kernel (csrc/gemm.hip), the 128x128 LDS-DMA ring with its split-K, fused colsum, RoPE and grouped
forms (csrc/gemm128.hip), the persistent 256x256 kernel (csrc/gemm256.hip), and the implicit convolutions on each.

Cases (helpers.gemm_cases, helpers.CONV_CASES): the smallest shapes at which each mechanism exists — partial and ragged
K-steps, 1..5 K-tiles against the ring prologues, tiles shifted in one and both dimensions, split-K with a ragged second
slice, a persistent grid with 2 or 3 tiles per workgroup, the scalar store path, batched and f32-stored A operands. Every
test asserts through ops.gemm_last_path() the kernel family (and the split-K slice count) it meant to reach: a forced
family whose preconditions fail falls through to the register-staged kernel without a word. Two fall-throughs are
themselves asserted: alpha != 1 never takes the 256x256 kernel, and a biased call that the ring kernel would accumulate
(EPI_ACC, or an f32 store long enough to split) leaves it, because its accumulate epilogue reads no bias — on the ring
kernel those calls returned the product without the bias.

Inputs are randn times a power of two (2^-6 .. 2^6) per row and per column, so no row or column hides under a larger one.
The reference is torch float64 on the device from the same rounded operands (helpers.gemm_ref64). Bounds, per element
(helpers.gemm_bound), with s = |alpha| |A| |B|^T + |bias| + |c_old| and u = 2^-24:
    f32 store / accumulate   |out - y| <= C u s
    GELU outputs             |gelu'(y)| C u s + a, a = 2e-6 (gelu_f) or 2.6e-5 (the 256x256 GELU-only epilogue, gelu_bf16out)
    dGELU                    |gelu'(pre)| C u s + 2e-6 |y|
    dropout                  dropped elements exactly 0, kept ones the bound times 1 / (1 - p)
    bf16 output              + 2^-8 |ref|
    fused colsum             C u |A|.sum(K)
No element is left out. Output buffers start as NaN; the rows before and after a destination and the columns between N
and ldc must keep their bits.

C = 8 E, E = what fp32 evaluation in the kernels' order costs against float64 on these very cases, measured on the CPU
(tests/test_cpu_gemm_ref.py, which also proves from the reference alone that four mutants — last K element dropped,
bias[n + 1], alpha = 1, a 32-wide K slice dropped — leave these bounds on 0.55 - 1.0 of the elements they touch):
    cases              E      C
    GEMM, f32          3.8    30.4
    GEMM, bf16         3.1    24.8
    conv, f32          7.3    58.4     (hard cap 64)
    conv, bf16         5.9    47.2

Measured on an MI355X: the largest |out - y| / (u s) over the f32 store / accumulate outputs (and fused column sums) of
each family, to compare with C, and the largest share of its bound any output used. The bf16 outputs reach 0.99 of
theirs by construction: a correctly rounded bf16 value just above a power of two is 2^-8 |ref| off, the whole bf16 term.
    family             units    share of bound
    small, f32         3.97     0.130
    small, bf16        4.54     0.993     (the 8-slice K = 4160 cases that a bias moves off the ring kernel)
    128                1.38     0.994
    256                4.71     0.995     (the accumulators start from the bias)
    big                -        0.996
    grouped-128        0.97     0.039
    grouped-small      1.39     0.056
    rope (128)         1.42     0.057
    conv small f32     6.66     0.114     (of C = 58.4)
    conv small bf16    -        0.991
    conv 256           -        0.991
    conv big           -        0.994
The split-K and grouped sums come out of f32 atomics, so these figures move in their last digit from launch to launch.
"""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
TD = {"f32": torch.float32, "bf16": BF}
SEED, STREAM = 7, 3
CASES = H.gemm_cases()
NEED = {}          # row of the table above -> [units, share]
assert all(v <= 64.0 for v in H.GEMM_C.values())


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    for k in sorted(NEED):
        print(f"\nGEMMNEED {k:<16} units {NEED[k][0]:6.2f}  share {NEED[k][1]:5.3f}", end="")
    print()


@pytest.fixture
def o():
    """fddm_hip.ops; the automatic kernel choice and the uncapped persistent grid are restored whatever happens."""
    from fddm_hip import ops
    from fddm_hip._lib import lib
    try:
        yield ops
    finally:
        ops.gemm_force_path("auto")
        lib().fddm_gemm_persistent_cap(0)


def _cap(n):
    from fddm_hip._lib import lib
    lib().fddm_gemm_persistent_cap(n)


_PROD = {}


def _prod(M, N, K, dt, a_f32=False):
    """(A, B, A B^T, |A| |B|^T) in float64 on the device, computed once per shape."""
    key = (M, N, K, dt, a_f32)
    if key not in _PROD:
        A, B = H.gemm_logical64(H.gemm_operands(*key), dt, dev)
        _PROD[key] = (A, B, A @ B.t(), A.abs() @ B.abs().t())
    return _PROD[key]


_CONV = {}


def _conv_ref(name, dt):
    """float64 F.conv1d and its error scale, computed once per geometry on the host and kept on the device."""
    if (name, dt) not in _CONV:
        _CONV[(name, dt)] = tuple(t.to(dev) for t in H.conv_ref(name, *H.conv_operands(name, dt)))
    return _CONV[(name, dt)]


class Guarded:
    """A [rows, cols] destination inside a NaN-filled [rows + 2, ld] buffer: one guard row before and after, guard
    columns cols .. ld."""

    def __init__(self, rows, cols, ld, dtype, init=None):
        self.buf = torch.full((rows + 2, ld), float("nan"), dtype=dtype, device=dev)
        self.view = self.buf[1:rows + 1, :cols]
        if init is not None:
            self.view.copy_(init)
        self.before = self.buf.clone()
        self.inside = torch.zeros(rows + 2, ld, dtype=torch.bool, device=dev)
        self.inside[1:rows + 1, :cols] = True

    def _bits(self, t):
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16)

    def check_guard(self, what, whole=False):
        same = self._bits(self.buf) == self._bits(self.before)
        bad = ~same if whole else ~same & ~self.inside
        assert not bad.any(), f"{what}: {int(bad.sum())} guard elements changed, first at {bad.nonzero()[0].tolist()}"


def _check(what, row, got, ref, bound, units_of=None):
    """|got - ref| <= bound at every element; records the share of the bound used (and, for units_of = u s, the error in
    those units) under table row `row`."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    err = (got - ref).abs()
    share = err / bound.clamp_min(1e-300)        # a zero bound (a dropped element) admits only err == 0
    rec = NEED.setdefault(row, [0.0, 0.0])
    rec[1] = max(rec[1], share.max().item())
    if units_of is not None:
        rec[0] = max(rec[0], (err / units_of).max().item())
    bad = err > bound
    if bad.any():
        idx = tuple(int(v) for v in np.unravel_index(int(share.argmax()), tuple(share.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at {idx}: got "
                             f"{got[idx].item():.9g}, ref {ref[idx].item():.9g}, bound {bound[idx].item():.3g} "
                             f"({share[idx].item():.2f} x)")


def _row(c):
    return f"{c['fam']}, {c['dt']}" if c["fam"] == "small" else c["fam"]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_gemm(o, c):
    M, N, K, dt, epi = c["M"], c["N"], c["K"], c["dt"], c["epi"]
    od = TD[c["out"]]
    ops_ = H.gemm_operands(M, N, K, dt, c["a_f32"])
    A, B = ops_["A"], ops_["B"]
    sAb = 0
    if c["Mi"]:      # batched rows: row m at (m / Mi) sAb + (m % Mi) lda, NaN in every gap
        nb, Mi, lda = M // c["Mi"], c["Mi"], K + 8
        sAb = Mi * lda + 64
        flat = torch.full((nb * sAb,), float("nan"), dtype=A.dtype, device=dev)
        torch.as_strided(flat, (nb, Mi, K), (sAb, lda, 1)).copy_(A.view(nb, Mi, K))
        Ad = flat
    else:
        Ad = (A if c["a_kc"] else A.t()).contiguous().to(dev)
        lda = Ad.shape[1]
    Bd = (B if c["b_kc"] else B.t()).contiguous().to(dev)
    ldc = N + c["pad"]
    bias = ops_["bias"].to(dev) if c["bias"] else None
    c_old = ops_["c_old"].to(dev) if epi == H.EPI_ACC else None
    pre = ops_["pre"].to(od).to(dev) if epi == H.EPI_DGELU else None
    Cg = Guarded(M, N, ldc, od, init=c_old)
    C2g = Guarded(M, N, ldc, od, init=pre) if epi in (H.EPI_GELU, H.EPI_DGELU) else None
    cs_old = ops_["cs_old"].to(dev) if epi == H.EPI_ACC else None
    csg = Guarded(1, M, M, torch.float32, init=cs_old) if c["colsum"] else None

    o.gemm_force_path(c["fam"])
    _cap(c["cap"])
    o.gemm(Ad, Bd, Cg.view, M, N, K, a_kc=bool(c["a_kc"]), b_kc=bool(c["b_kc"]), lda=lda, ldb=Bd.shape[1], ldc=ldc, epi=epi,
           bias=bias, alpha=c["alpha"], C2=C2g.view if C2g else None, Mi=c["Mi"], sAb=sAb, drop_p=c["p"], seed=SEED,
           rng_stream=STREAM, colsum=csg.view[0] if csg else None)
    assert o.gemm_last_path() == (c["expect"], c["splits"]), (o.gemm_last_path(), c["expect"], c["splits"])
    torch.cuda.synchronize()

    A64, B64, P, S = _prod(M, N, K, dt, c["a_f32"])
    keep = O.dropout_keep(SEED, STREAM, M * N, c["p"]).view(M, N).to(dev) if c["p"] else None
    r = H.gemm_ref64(A64, B64, bias=bias, alpha=float(np.float32(c["alpha"])), c_old=c_old, epi=epi, pre=pre, keep=keep,
                     drop_p=c["p"], prod=(P, S))
    Cc, bf = H.GEMM_C[dt], od == BF
    gabs = H.GEMM_GELU_BF16OUT_ABS if (c["expect"] == "256" and epi == H.EPI_GELU_ONLY) else H.GEMM_GELU_ABS
    row = _row(c) if c["expect"] == c["fam"] else "small, bf16"
    if epi in (H.EPI_STORE, H.EPI_ACC, H.EPI_GELU):
        ref, b = H.gemm_bound(r, "y", Cc, bf)
        _check(c["id"] + " C", row, Cg.view, ref, b, units_of=None if bf else H.U24 * r.s)
    else:
        ref, b = H.gemm_bound(r, "act", Cc, bf, gabs)
        _check(c["id"] + " C", row, Cg.view, ref, b)
    Cg.check_guard(c["id"] + " C")
    if epi == H.EPI_GELU:
        ref, b = H.gemm_bound(r, "act", Cc, bf, gabs)
        _check(c["id"] + " C2", row, C2g.view, ref, b)
        C2g.check_guard(c["id"] + " C2")
    elif epi == H.EPI_DGELU:
        C2g.check_guard(c["id"] + " pre-activation (read only)", whole=True)
    if csg:
        old = cs_old.double() if epi == H.EPI_ACC else torch.zeros(M, dtype=torch.float64, device=dev)
        sc = H.U24 * (r.colsum_s + old.abs())
        _check(c["id"] + " colsum", row, csg.view[0], r.colsum + old, Cc * sc, units_of=sc)
        csg.check_guard(c["id"] + " colsum")


@pytest.mark.parametrize("M,N,K", [(200, 128, 64), (392, 256, 192)])
def test_linear_dx_rope(o, M, N, K):
    """fddm_linear_dx_rope (gemm128 EPI_ROPE_ACC): dx += rope_bwd(dy w) on one tile column with a shifted row tile, and on
    4 x 2 tiles with 3 K-tiles, accumulated onto a non-zero dx; L = 100 positions."""
    L = 100
    ops_ = H.gemm_operands(M, N, K, "bf16")
    cos, sin = (t.contiguous().to(dev) for t in O.rope_cos_sin(L, O.rope_inv_freq(N)))
    dy, w = ops_["A"].to(dev), ops_["B"].t().contiguous().to(dev)
    dxg = Guarded(M, N, N, torch.float32, init=ops_["c_old"].to(dev))
    o.gemm_force_path("128")
    assert o.linear_dx_rope(dy, w, dxg.view, cos, sin, L)
    assert o.gemm_last_path() == ("128", 1)
    torch.cuda.synchronize()
    _, _, P, S = _prod(M, N, K, "bf16")
    old = ops_["c_old"].to(dev).double()
    ref = old + H.rope_bwd_ref64(P, cos, sin, L)
    s = H.U24 * (old.abs() + H.rope_bwd_ref64(S, cos.abs(), sin.abs(), L, magnitude=True))
    _check(f"rope {M}x{N}x{K}", "rope (128)", dxg.view, ref, H.GEMM_C["bf16"] * s, units_of=s)
    dxg.check_guard("rope dx")


@pytest.mark.parametrize("kchunk,fam,splits", [(0, "grouped-128", None), (512, "grouped-small", 8)])
def test_linear_dw_grouped(o, kchunk, fam, splits):
    """Grouped weight gradients with the automatic balance (128x128 LDS-DMA kernel) and with kchunk = 512 (register-staged
    grouped kernel: 1, 8 and 2 slices): a ragged token count on shifted tiles, a long reduction on one tile, 1 x 4 tiles
    with the last one shifted; destinations are column slices of larger buffers, one job without a bias gradient."""
    jobs, refs = [], []
    for i, (K, M, N) in enumerate([(203, 136, 264), (4100, 128, 128), (1000, 128, 392)]):
        ops_ = H.gemm_operands(M, N, K, "bf16")
        dy, x = ops_["A"].t().contiguous().to(dev), ops_["B"].t().contiguous().to(dev)
        big = Guarded(M, N + 16, N + 16, torch.float32)
        big.view[:, 8:8 + N] = ops_["c_old"].to(dev)
        big.before = big.buf.clone()
        big.inside[:] = False
        big.inside[1:M + 1, 8:8 + N] = True
        dbg = Guarded(1, M, M, torch.float32, init=ops_["cs_old"].to(dev)) if i != 1 else None
        jobs.append((dy, x, big.view[:, 8:8 + N], dbg.view[0] if dbg else None))
        refs.append((ops_, big, dbg, (M, N, K)))
    o.gemm_force_path("128" if kchunk == 0 else "auto")
    o.linear_dw_grouped(jobs, kchunk=kchunk)
    got_fam, got_nz = o.gemm_last_path()
    assert got_fam == fam and (splits is None or got_nz == splits), (got_fam, got_nz)
    torch.cuda.synchronize()
    Cc = H.GEMM_C["bf16"]
    for (ops_, big, dbg, (M, N, K)), job in zip(refs, jobs):
        A64, B64, P, S = _prod(M, N, K, "bf16")
        r = H.gemm_ref64(A64, B64, c_old=ops_["c_old"].to(dev), prod=(P, S))
        _check(f"{fam} dW {M}x{N}x{K}", fam, job[2], r.y, Cc * H.U24 * r.s, units_of=H.U24 * r.s)
        big.check_guard(f"{fam} dW {M}x{N}x{K}")
        if dbg:
            old = ops_["cs_old"].to(dev).double()
            sc = H.U24 * (r.colsum_s + old.abs())
            _check(f"{fam} db {M}x{N}x{K}", fam, job[3], r.colsum + old, Cc * sc, units_of=sc)
            dbg.check_guard(f"{fam} db")


@pytest.mark.parametrize("name,dt", [("small", "f32"), ("small", "bf16"), ("256", "bf16"), ("big", "bf16")])
@pytest.mark.parametrize("gelu", [False, True])
def test_conv1d_gemm(o, name, dt, gelu):
    """fddm_conv1d_gemm on each family against float64 F.conv1d (geometries: helpers.CONV_CASES)."""
    g = H.CONV_CASES[name]
    x, w, b = (t.to(dev) for t in H.conv_operands(name, dt))
    G, Cg, N, taps, M = g["G"], g["Cg"], g["N"], g["taps"], g["Bn"] * g["Tout"]
    Wp = w.view(G, N, Cg, taps).permute(0, 1, 3, 2).contiguous()
    outg = Guarded(M, G * N, G * N, TD[dt])
    o.gemm_force_path(g["fam"])
    o.conv1d_gemm(x, Wp, outg.view, lda=G * Cg, sAb=g["Tin"] * G * Cg, Tin=g["Tin"], Cg=Cg, cstride=g["stride"],
                  cpad=g["cpad"], Bn=g["Bn"], Tout=g["Tout"], N=N, K=taps * Cg, groups=G, bias=b, gelu=gelu)
    assert o.gemm_last_path() == (g["fam"], 1)
    torch.cuda.synchronize()
    r = H.GemmRef()
    r.y, r.s = _conv_ref(name, dt)
    H.epilogue_ref64(r, H.EPI_GELU_ONLY if gelu else H.EPI_STORE)
    gabs = H.GEMM_GELU_BF16OUT_ABS if name == "256" else H.GEMM_GELU_ABS
    ref, bound = H.gemm_bound(r, "act" if gelu else "y", H.GEMM_C["conv-" + dt], dt == "bf16", gabs)
    row = f"conv {name}" + (f" {dt}" if name == "small" else "")
    _check(f"conv {name} {dt} gelu={gelu}", row, outg.view, ref, bound,
           units_of=H.U24 * r.s if (dt == "f32" and not gelu) else None)
    outg.check_guard(f"conv {name}")
