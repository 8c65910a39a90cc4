"""The decoder's input gradients on the persistent 256x256 kernel: its accumulate (EPI_ACC_F32) and dGELU + dropout
(EPI_DGELU) epilogues, ops.linear_dx through a transposed weight copy, and the multi-tensor transpose that keeps
those copies (csrc/gemm256.hip, csrc/misc.hip fddm_transpose_bf16_mt).

Every GEMM output is checked per element against float64 from the same bf16 operands, with the operands, reference and
bounds of tests/test_gpu_gemm.py (helpers.gemm_operands / gemm_ref64 / gemm_bound, C = GEMM_C["bf16"] = 8 E units of
2^-24 s, s = |A| |B|^T + |c_old|; dGELU |gelu'(pre)| C u s + 2e-6 |y|; dropped elements exactly 0, kept ones times
1 / (1 - p); a bf16 output + 2^-8 |ref|). The accumulate epilogue starts its accumulators from the previous C, as the
other builds start theirs from the bias (the "256" row of that file's table), so the same C covers it.

Shapes, the smallest at which each mechanism exists:
    256 x 256 x 128      one tile, two K-tiles (the kernel needs nk >= 2): prologue loads of C, final epilogue only
    264 x 264 x 128      2 x 2 tiles, three of them shifted: the rows and columns two tiles share must be added once
                         (ldc = N + 8: the columns between N and ldc must keep their bits)
    1024 x 512 x 512     4 x 2 tiles on a grid capped to 8 workgroups, 8 K-tiles: one tile per workgroup, each on its
                         own XCD range of the tile order
    2048 x 520 x 192     8 x 3 = 24 tiles on 8 workgroups, three each: the EP K-tile (a tile's epilogue and the next
                         tile's loads of C inside the next tile's first K-tile), with the shifted last tile column
                         among the tiles that pass through it; ldc = N + 8
    256 x 256 x 2048     32 K-tiles
"""
import pytest
import torch

import helpers as H
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
SEED, STREAM = 7, 3
CC = H.GEMM_C["bf16"]

# (M, N, K, pad, persistent cap)
_CASES = [(256, 256, 128, 0, 0), (264, 264, 128, 8, 0), (1024, 512, 512, 0, 8), (2048, 520, 192, 8, 8),
          (256, 256, 2048, 0, 0)]
_IDS = [f"{m}x{n}x{k}" + (f"-cap{c}" if c else "") for m, n, k, _, c in _CASES]


@pytest.fixture
def o():
    """fddm_hip.ops; the automatic kernel choice and the previous persistent-grid cap are restored whatever happens."""
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    from fddm_hip import ops
    from fddm_hip._lib import lib
    prev = lib().fddm_gemm_persistent_cap(0)
    try:
        yield ops
    finally:
        ops.gemm_force_path("auto")
        lib().fddm_gemm_persistent_cap(prev)


_PROD = {}


def _prod(M, N, K):
    """(operands, A B^T, |A| |B|^T in float64 on the device), once per shape."""
    if (M, N, K) not in _PROD:
        ops_ = H.gemm_operands(M, N, K, "bf16")
        A, B = H.gemm_logical64(ops_, "bf16", dev)
        _PROD[(M, N, K)] = (ops_, A, B, A @ B.t(), A.abs() @ B.abs().t())
    return _PROD[(M, N, K)]


class Guarded:
    """A [rows, cols] destination inside a NaN-filled [rows + 2, ld] buffer; nothing outside it may change."""

    def __init__(self, rows, cols, ld, dtype, init=None):
        self.buf = torch.full((rows + 2, ld), float("nan"), dtype=dtype, device=dev)
        self.view = self.buf[1:rows + 1, :cols]
        if init is not None:
            self.view.copy_(init)
        self.before = self.buf.clone()
        self.inside = torch.zeros(rows + 2, ld, dtype=torch.bool, device=dev)
        self.inside[1:rows + 1, :cols] = True

    def check_guard(self, what, whole=False):
        bits = lambda t: t.view(torch.int32 if t.element_size() == 4 else torch.int16)   # noqa: E731
        bad = bits(self.buf) != bits(self.before)
        if not whole:
            bad &= ~self.inside
        assert not bad.any(), f"{what}: {int(bad.sum())} guard elements changed, first at {bad.nonzero()[0].tolist()}"


def _check(what, got, ref, bound):
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    err = (got - ref).abs()
    share = err / bound.clamp_min(1e-300)
    print(f"\nDX256 {what}: largest share of the bound {share.max().item():.3f}", end="")
    bad = err > bound
    if bad.any():
        i = tuple(int(v) for v in (share == share.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at {i}: got "
                             f"{got[i].item():.9g}, ref {ref[i].item():.9g}, bound {bound[i].item():.3g}")


def _run256(o, M, N, K, pad, cap, epi, p=0.0, fam="256"):
    """One NT fddm_gemm on the forced family; returns (output Guarded, GemmRef)."""
    from fddm_hip._lib import lib
    ops_, A64, B64, P, S = _prod(M, N, K)
    A, B = ops_["A"].to(dev), ops_["B"].to(dev)
    ldc = N + pad
    acc = epi == H.EPI_ACC
    c_old = ops_["c_old"].to(dev) if acc else None
    pre = ops_["pre"].to(BF).to(dev) if epi == H.EPI_DGELU else None
    Cg = Guarded(M, N, ldc, torch.float32 if acc else BF, init=c_old)
    C2g = Guarded(M, N, ldc, BF, init=pre) if pre is not None else None
    o.gemm_force_path(fam)
    prev = lib().fddm_gemm_persistent_cap(cap)
    try:
        o.gemm(A, B, Cg.view, M, N, K, lda=K, ldb=K, ldc=ldc, epi=epi, C2=C2g.view if C2g else None, drop_p=p, seed=SEED,
               rng_stream=STREAM)
        assert o.gemm_last_path() == (fam, 1), o.gemm_last_path()
        torch.cuda.synchronize()
    finally:
        lib().fddm_gemm_persistent_cap(prev)
    keep = O.dropout_keep(SEED, STREAM, M * N, p).view(M, N).to(dev) if p else None
    r = H.gemm_ref64(A64, B64, c_old=c_old, epi=epi, pre=pre, keep=keep, drop_p=p, prod=(P, S))
    if C2g is not None:
        C2g.check_guard("pre-activation (read only)", whole=True)
    return Cg, r


@pytest.mark.parametrize("M,N,K,pad,cap", _CASES, ids=_IDS)
def test_acc_f32_on_256(o, M, N, K, pad, cap):
    """C += A B^T onto a non-zero C (randn times the row and column scales), every element once."""
    Cg, r = _run256(o, M, N, K, pad, cap, H.EPI_ACC)
    assert (Cg.before[1:M + 1, :N] != 0).all()     # the destination was not zero
    ref, b = H.gemm_bound(r, "y", CC, False)
    _check(f"acc {M}x{N}x{K}", Cg.view, ref, b)
    Cg.check_guard("acc C")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M,N,K,pad,cap", _CASES, ids=_IDS)
def test_dgelu_on_256(o, M, N, K, pad, cap, p):
    """C = (A B^T) gelu'(pre) keep / (1 - p) in bf16; with p = 0.1 the zero pattern is the 128x128 kernel's, bit for bit,
    at the same seed and stream (both must drop what the forward's GELU epilogue dropped)."""
    Cg, r = _run256(o, M, N, K, pad, cap, H.EPI_DGELU, p)
    ref, b = H.gemm_bound(r, "act", CC, True)
    _check(f"dgelu {M}x{N}x{K} p={p}", Cg.view, ref, b)
    Cg.check_guard("dgelu C")
    C128, _ = _run256(o, M, N, K, pad, 0, H.EPI_DGELU, p, fam="128")
    z256, z128 = Cg.view == 0, C128.view == 0
    assert torch.equal(z256, z128), f"{int((z256 != z128).sum())} elements dropped by one kernel only"
    if p:
        keep = O.dropout_keep(SEED, STREAM, M * N, p).view(M, N).to(dev)
        assert not (z256 & keep).any() and z256[~keep].all()
        assert 0.05 < z256.float().mean().item() < 0.15


@pytest.mark.parametrize("mode", ["store", "acc", "dgelu"])
def test_linear_dx_with_wt(o, mode):
    """ops.linear_dx through the transposed copy (256x256 kernel, forced: 4 tiles are below its automatic threshold)
    against the same call on W as stored (128x128 ring): both within the float64 bound, so they differ by at most the
    sum of the two."""
    M = N = K = 512            # dy [M, N] @ w [N, K]
    ops_, A64, B64, P, S = _prod(M, K, N)          # the GEMM's (M, N, K) = (M, K, N): B64 [K, N] = w^T
    dy, wt = ops_["A"].to(dev), ops_["B"].to(dev)
    w = wt.t().contiguous()
    kw, p = {}, 0.0
    c_old = pre = keep = None
    if mode == "acc":
        c_old = ops_["c_old"].to(dev)
        kw = dict(accumulate=True)
    elif mode == "dgelu":
        p = 0.1
        pre = ops_["pre"].to(BF).to(dev)
        kw = dict(epi=o.EPI_DGELU, C2=pre, drop_p=p, seed=SEED, rng_stream=STREAM)
        keep = O.dropout_keep(SEED, STREAM, M * K, p).view(M, K).to(dev)
    od = torch.float32 if mode == "acc" else BF
    outs = []
    for fam, t in (("256", wt), ("128", None)):
        g = Guarded(M, K, K, od, init=c_old)
        o.gemm_force_path("256" if fam == "256" else "auto")
        o.linear_dx(dy, w, out=g.view, wt=t, **kw)
        assert o.gemm_last_path() == (fam, 1), (fam, o.gemm_last_path())
        torch.cuda.synchronize()
        g.check_guard(f"linear_dx {mode} {fam}")
        outs.append(g.view.double())
    epi = {"store": H.EPI_STORE, "acc": H.EPI_ACC, "dgelu": H.EPI_DGELU}[mode]
    r = H.gemm_ref64(A64, B64, c_old=c_old, epi=epi, pre=pre, keep=keep, drop_p=p, prod=(P, S))
    ref, b = H.gemm_bound(r, "act" if mode == "dgelu" else "y", CC, od == BF)
    for fam, got in zip(("256", "128"), outs):
        _check(f"linear_dx {mode} on {fam}", got, ref, b)
    assert ((outs[0] - outs[1]).abs() <= 2 * b).all()


_T_SHAPES = [(512, 512), (1536, 512), (2048, 512), (8, 8), (264, 72)]


def _bits(t):
    return t.view(torch.int16)


def _flat_dst(n, gen):
    """n bf16 elements inside a buffer with 64 sentinel elements on either side."""
    buf = torch.randn(n + 128, generator=gen).to(BF).to(dev)
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("shape", _T_SHAPES, ids=[f"{r}x{c}" for r, c in _T_SHAPES])
def test_transpose_one(o, shape):
    gen = torch.Generator().manual_seed(shape[0] * 4099 + shape[1])
    w = torch.randn(*shape, generator=gen).to(BF).to(dev)
    buf, flat = _flat_dst(w.numel(), gen)
    before = buf.clone()
    dst = flat.view(shape[1], shape[0])
    o.transpose_bf16_mt(o.transpose_table([(w, dst)]))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(w.t().contiguous()))
    assert torch.equal(_bits(buf[:64]), _bits(before[:64])) and torch.equal(_bits(buf[-64:]), _bits(before[-64:]))


def test_transpose_table_of_several(o):
    """All five shapes in one launch, each destination between sentinels."""
    gen = torch.Generator().manual_seed(5)
    ws = [torch.randn(*s, generator=gen).to(BF).to(dev) for s in _T_SHAPES]
    ds = [_flat_dst(w.numel(), gen) for w in ws]
    befores = [b.clone() for b, _ in ds]
    pairs = [(w, f.view(w.shape[1], w.shape[0])) for w, (_, f) in zip(ws, ds)]
    tab = o.transpose_table(pairs)
    assert tab[1] == 5 and tab[2] == sum(((r + 63) // 64) * ((c + 63) // 64) for r, c in _T_SHAPES)
    o.transpose_bf16_mt(tab)
    torch.cuda.synchronize()
    for w, (buf, _), (_, dst), before in zip(ws, ds, pairs, befores):
        assert torch.equal(_bits(dst), _bits(w.t().contiguous())), tuple(w.shape)
        assert torch.equal(_bits(buf[:64]), _bits(before[:64])) and torch.equal(_bits(buf[-64:]), _bits(before[-64:]))


def test_transpose_rejects_bad_shapes(o):
    w = torch.zeros(12, 8, dtype=BF, device=dev)
    with pytest.raises(ValueError):
        o.transpose_table([(w, torch.zeros(8, 12, dtype=BF, device=dev))])
