"""The diffusion-loss kernels (csrc/kl.hip, kl_reduce in csrc/small.hip) per element against float64.

Every KL gradient is compared element by element with helpers.kl_term_ref64 under a bound relative to the per-element
error scale s_k (helpers.kl_term_ref64), every per-token KL with its float64 value, masked tokens included; the
cases select each reachable template instantiation of the dispatch in kl.hip (listed at each case table) and place
x_t / x0 at the index edges. The softmax, scale / axpy and kl_reduce kernels follow, each against float64.

How the bounds were set (on the CPU, from the inputs of this file, before any kernel ran):
  * gradient: the fp32 oracle (oracle.fddm_oracle.kl_term) against float64 stays within ORACLE_C = 2.45e-6 s_k over
    every case here (0.13e-6 at B = 3, L = 1 up to 2.45e-6 at V = 32768; 0.6e-6 at V = 36, 1.3e-6 at V = 2052),
    without an absolute floor. The kernels use __expf, v_rcp, v_log, one log per four factors and another summation
    order where the oracle has correctly rounded libm, so they get C_GRAD = 8 x that = 1.96e-5 (hard cap 1e-4:
    beyond it the kernel is wrong, not the tolerance narrow). bf16 outputs add one bf16 rounding, 2^-8 |ref|.
    Measured on an MI355X the kernels need at most 2.9e-6 s_k (kl4 backward, V = 16388).
  * per token: |kl_tok - ref| <= A_TOK + R_TOK |ref|. The fp32 evaluation of the oracle's formula
    (kl_term_ref64(dtype=float32)) has an absolute error of up to ORACLE_A = 2.03e-7 on the tokens with
    |kl_tok| < 0.1 (down to kl_tok ~ 1e-6 at x_t = x0 and small t, where Q ~ 1 rounds: 5 % of the value there) and a
    relative one of up to ORACLE_R = 1.44e-6 on the tokens above; 8 x each. The kernels measure 2.6e-7 and 9.7e-7.
  * the criterion discriminates (asserted per case from the reference alone): on at least half of the generic
    indices (k neither x_t nor x0) of unmasked rows C_GRAD s_k < |ref_k| / 4, and no probability is below 1e-30 (fp32
    exp underflow, where the scale means nothing). Shares: 0.68 - 0.78 at V = 36 / 37 (logits 2 randn), 0.73 at
    V = 1025, 0.83 - 1.00 at the other V (logits 3 randn); each check prints its case's share.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import close, kl_term_ref64
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16

TN = 200                        # diffusion steps; t covers 1 (beta_p = 0), 2, the middle and T
C_GRAD = 1.96e-5                # 8 x ORACLE_C = 8 x 2.45e-6 (see the module docstring)
A_TOK, R_TOK = 1.63e-6, 1.15e-5 # 8 x ORACLE_A = 8 x 2.03e-7, 8 x ORACLE_R = 8 x 1.44e-6
SMALL_TOK = 0.1                 # the split between the absolute and the relative per-token measurement


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()


def ops():
    from fddm_hip import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ KL inputs and checks
def edge_pairs(V):
    """(x_t, x0) at the index edges of a row of V: first / last index, one float4, neighbouring float4s, the last
    (partly filled) chunk, and x_t in the second and the last chunk of a thread of the 512-thread kernels
    (float 2048 i + 1: thread 0, lane 1 of its float4 i), where the row is long enough."""
    p = [(0, 0), (0, V - 1), (V - 1, 0), (5, 4), (4, 8), (V - 1, V - 2), (V - 3, V - 3)]
    for i in sorted({1, (V - 2) // 2048}):
        if i >= 1 and 2048 * i + 1 < V:
            p.append((2048 * i + 1, 2048 * i + 1027 if 2048 * i + 1027 < V else 7))
    return p


class KlCase:
    pass


@functools.lru_cache(maxsize=4)
def kl_case(V, masked, B=4, L=12):
    """Inputs and the float64 reference of one KL case (computed once, shared, never modified). Logits 3 randn
    (2 randn below V = 100: fewer, larger probabilities); x_t = x0 on every third token, then the edge pairs on the
    first tokens of every utterance (rotated by two per utterance, so that L = 1 still sees different pairs).
    masked: utterance 1 all padding (cnt = 0), utterance 2 one valid token, utterance 0 two padded tokens."""
    c = KlCase()
    c.V, c.B, c.L, c.masked = V, B, L, masked
    c.betas, _ = O.sched_tables(TN)
    c.t = torch.tensor({4: [1, 2, 117, TN], 3: [1, 117, TN]}[B])
    c.logits = (2.0 if V < 100 else 3.0) * torch.randn(B, L, V, generator=g(1000 + V))
    c.x0 = torch.randint(0, V, (B, L), generator=g(2000 + V))
    c.xt = torch.randint(0, V, (B, L), generator=g(3000 + V))
    c.xt[:, ::3] = c.x0[:, ::3]
    pairs = edge_pairs(V)
    for b in range(B):
        for l in range(min(L, len(pairs))):
            c.xt[b, l], c.x0[b, l] = pairs[(l + 2 * b) % len(pairs)]
    c.xm = None
    if masked:
        c.xm = torch.ones(B, L, dtype=torch.bool)
        c.xm[1] = False
        c.xm[2] = False
        c.xm[2, min(3, L - 1)] = True
        if L > 2:
            c.xm[0, 1] = False
            c.xm[0, L - 1] = False
    c.kl, c.dz, c.w, c.s = kl_term_ref64(c.logits, c.xt, c.x0, c.t, c.xm, c.betas)
    c.loss = (c.kl * c.w).sum()
    # the criterion must discriminate, from the reference alone
    xhat = torch.softmax(c.logits.double(), -1)
    assert xhat.min().item() >= 1e-30, f"V={V}: probabilities underflow fp32 exp"
    generic = torch.ones(B, L, V, dtype=torch.bool)
    generic.scatter_(-1, c.xt[..., None], False)
    generic.scatter_(-1, c.x0[..., None], False)
    generic &= (c.w > 0)[..., None]
    c.share = ((C_GRAD * c.s < c.dz.abs() / 4) & generic).sum().item() / generic.sum().item()
    assert c.share >= 0.5, f"V={V} masked={masked}: only {c.share:.2f} of the generic elements discriminate"
    return c


def dev_args(c):
    """(logits [N, V], xt, x0, t, betas) on the device."""
    return (c.logits.view(-1, c.V).to(dev), c.xt.reshape(-1).to(dev), c.x0.reshape(-1).to(dev), c.t.to(dev),
            c.betas.to(dev))


def mask_u8(c):
    return c.xm.reshape(-1).to(dev).view(torch.uint8) if c.masked else None


def check_dz(dz, c, what, gs=1.0):
    """|dz - ref| <= C_GRAD s_k (+ 2^-8 |ref| for a bf16 output), every element; s_k = 0 (masked rows) demands
    exactly 0."""
    d = dz.double().view(c.B, c.L, c.V).cpu()
    assert torch.isfinite(d).all(), f"{what}: non-finite gradient"
    ref, s = gs * c.dz, gs * c.s
    err = (d - ref).abs()
    if dz.dtype == BF:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    need = (err[s > 0] / s[s > 0]).max().item() if (s > 0).any() else 0.0
    print(f"{what}: max |dz - ref| / s_k = {need:.3e} (C_GRAD {C_GRAD:.1e}), discriminating share {c.share:.2f}")
    bad = err > C_GRAD * s
    assert not bad.any(), (f"{what}: {bad.sum().item()} elements off, worst ratio {need:.3e}, first at "
                           f"{bad.nonzero()[0].tolist()}")
    if c.masked:
        assert (d[c.w == 0] == 0).all(), f"{what}: masked rows must get an exactly zero gradient"


def check_kl_tok(kl_tok, c, what):
    k = kl_tok.double().view(c.B, c.L).cpu()
    assert torch.isfinite(k).all(), f"{what}: non-finite kl_tok"
    err = (k - c.kl).abs()
    small = c.kl.abs() < SMALL_TOK
    a = err[small].max().item() if small.any() else 0.0
    r = (err[~small] / c.kl[~small].abs()).max().item() if (~small).any() else 0.0
    print(f"{what}: kl_tok max abs err {a:.3e} where |ref| < {SMALL_TOK} (A_TOK {A_TOK:.1e}), "
          f"max rel err {r:.3e} elsewhere (R_TOK {R_TOK:.1e})")
    bad = err > A_TOK + R_TOK * c.kl.abs()
    assert not bad.any(), f"{what}: {bad.sum().item()} tokens off (abs {a:.3e}, rel {r:.3e}), first at {bad.nonzero()[0].tolist()}"


def run_fused(c, what):
    o = ops()
    for dt in (torch.float32, BF):
        kl_tok, dz = o.kl_fused(*dev_args(c), mask_u8(c), c.L, out_dtype=dt)
        check_kl_tok(kl_tok, c, f"{what} {dt}")
        check_dz(dz, c, f"{what} {dt}")


def run_two_pass(c, what, logits_dev=None):
    """kl_fwd, then kl_bwd with the reference's weights: f32 and bf16 dz, gscale None and 2."""
    o = ops()
    a = list(dev_args(c))
    if logits_dev is not None:
        a[0] = logits_dev
    check_kl_tok(o.kl_fwd(*a, c.L), c, what)
    w = c.w.reshape(-1).float().to(dev)
    two = torch.full((1,), 2.0, device=dev)
    for dt in (torch.float32, BF):
        check_dz(o.kl_bwd(*a, w, None, c.L, out_dtype=dt), c, f"{what} bwd {dt}")
        check_dz(o.kl_bwd(*a, w, two, c.L, out_dtype=dt), c, f"{what} bwd {dt} gscale 2", gs=2.0)


# ------------------------------------------------------------------------------------------ KL cases
# fddm_kl_fused (KLF_LAUNCH in kl.hip), f32 and bf16 dz, with the mask and without; oracle ratio / share per V:
#   V = 36     kl4_fused_kernel<2, *, 256>, most lanes padding
#   V = 2048   <2, *, 256> exactly full: the uniform-chunk branch for every chunk
#   V = 2052   <8, *, 256>
#   V = 8196   <16, *, 256>
#   V = 16388  <16, *, 512>
#   V = 32768  <16, *, 512>, the maximum
@pytest.mark.parametrize("V", [36, 2048, 2052, 8196, 16388, 32768])
def test_kl_fused_per_element(V):
    for masked in (True, False):
        run_fused(kl_case(V, masked), f"kl_fused V={V} masked={masked}")


# fddm_kl_fwd / fddm_kl_bwd on the float4 path (KL4_DISPATCH): forward kl4_kernel<2 NV, false, float, 256>, backward
# kl4_kernel<NV, true, float | bf16_t, 512>:
#   V = 36, 2048  NV = 1      V = 2052  NV = 4      V = 8196  NV = 8      V = 16388, 32768  NV = 16
@pytest.mark.parametrize("V", [36, 2048, 2052, 8196, 16388, 32768])
def test_kl_two_pass_vectorised_per_element(V):
    run_two_pass(kl_case(V, True), f"kl4 V={V}")


# V % 4 != 0: the scalar kl_kernel<NPT, false | true, float | bf16_t> (KL_DISPATCH):
#   V = 37    NPT = 4, smallest       V = 1023  NPT = 4, last element in lane 254      V = 1025  NPT = 16
#   V = 4098  NPT = 32                V = 8193  NPT = 64                               V = 16382 NPT = 64, the maximum
@pytest.mark.parametrize("V", [37, 1023, 1025, 4098, 8193, 16382])
def test_kl_two_pass_scalar_per_element(V):
    run_two_pass(kl_case(V, True), f"kl scalar V={V}")


def test_kl_two_pass_unaligned_rows_take_scalar_kernel():
    """V = 2000 (a multiple of 4) on rows that start 4 bytes past a 16-byte boundary: kl_launch's alignment test
    sends them to kl_kernel<16, ...>."""
    c = kl_case(2000, True)
    buf = torch.empty(c.B * c.L * c.V + 1, device=dev)
    shifted = buf[1:].view(c.B * c.L, c.V)
    shifted.copy_(c.logits.view(-1, c.V))
    assert shifted.data_ptr() % 16 == 4
    run_two_pass(c, "kl scalar V=2000 shifted", logits_dev=shifted)


@pytest.mark.parametrize("B,L", [(3, 1), (4, 300)])
def test_kl_row_length_edges(B, L):
    """L = 1 (every token its own utterance) and L = 300 (the 256-thread kernel's mask count loop runs twice; an
    utterance's t is row / L), V = 36, both forms."""
    for masked in (True, False):
        c = kl_case(36, masked, B, L)
        run_fused(c, f"kl_fused B={B} L={L} masked={masked}")
        run_two_pass(c, f"kl4 B={B} L={L} masked={masked}")


def test_kl_fused_and_two_pass_with_kl_reduce_weights_agree():
    """The two forms KLFn chooses between, on one case, both against float64: the one-pass kernel (weights from the
    mask inside the kernel) and kl_fwd -> kl_reduce -> kl_bwd (weights from kl_reduce)."""
    o = ops()
    c = kl_case(2052, True)
    a = dev_args(c)
    kl_tok, dz1 = o.kl_fused(*a, mask_u8(c), c.L)
    check_dz(dz1, c, "one-pass")
    kl2 = o.kl_fwd(*a, c.L)
    check_kl_tok(kl2, c, "two-pass")
    loss, w = o.kl_reduce(kl2, mask_u8(c), c.B, c.L)
    close(loss, c.loss, rtol=1e-6, what="kl_reduce loss")
    close(w.view(c.B, c.L), c.w, rtol=1e-6, atol=0.0, what="kl_reduce w")
    dz2 = o.kl_bwd(*a, w, torch.ones(1, device=dev), c.L)
    check_dz(dz2, c, "two-pass")
    loss1, _ = o.kl_reduce(kl_tok, mask_u8(c), c.B, c.L, want_w=False)
    close(loss1, c.loss, rtol=1e-6, what="one-pass loss")


def test_vocabulary_limits_raise_before_launch():
    """V beyond what a kernel serves is a ValueError naming the range, raised in ops before any launch: the KL pair
    ends at 32768 (V % 4 == 0, aligned rows) or 16384 (otherwise), the softmax pair at 16384."""
    o = ops()
    for V in (32772, 16385):
        z = torch.zeros(2, V, device=dev)
        i = torch.zeros(2, dtype=torch.long, device=dev)
        t = torch.ones(1, dtype=torch.long, device=dev)
        betas = O.sched_tables(TN)[0].to(dev)
        with pytest.raises(ValueError, match="supported range"):
            o.kl_fwd(z, i, i, t, betas, 2)
        with pytest.raises(ValueError, match="supported range"):
            o.kl_bwd(z, i, i, t, betas, torch.zeros(2, device=dev), None, 2)
    z = torch.zeros(2, 16388, device=dev)
    with pytest.raises(ValueError, match="supported range"):
        o.softmax_rows(z, torch.float32)
    with pytest.raises(ValueError, match="supported range"):
        o.softmax_bwd_rows(z, z)


# ------------------------------------------------------------------------------------------ softmax
# softmax_rows_kernel<NPT, float | bf16_t> and softmax_bwd_kernel<NPT, float | bf16_t, float> (SM_ / SMB_DISPATCH):
#   V = 1, 1023  NPT = 4      V = 1025, 4100  NPT = 16 / 32      V = 8000  NPT = 32 (the train step)      V = 16384  NPT = 64
SM_V = [1, 1023, 1025, 4100, 8000, 16384]
FLT_MIN = 2.0 ** -126


@functools.lru_cache(maxsize=2)
def softmax_case(V):
    """x [N, V] (3 randn; row 0 with a +80 outlier, row 1 all equal) and its float64 softmax."""
    N = 3 if V == 1 else 5
    x = 3.0 * torch.randn(N, V, generator=g(4000 + V))
    x[0, V // 3] += 80.0
    x[1] = 0.7
    return x, torch.softmax(x.double(), -1)


@pytest.mark.parametrize("V", SM_V)
def test_softmax_rows_per_element(V):
    """f32: within 1e-5 of the row's largest probability (the existing bound, per row instead of per tensor); bf16:
    one rounding, 2^-8 relative per element; below the smallest normal float the device exp may flush to zero."""
    o = ops()
    x, ref = softmax_case(V)
    y = o.softmax_rows(x.to(dev), torch.float32).double().cpu()
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= 1e-5 * ref.amax(-1, keepdim=True)).all(), \
        f"f32: {((y - ref).abs() / ref.amax(-1, keepdim=True)).max().item():.3e} of the row max"
    yb = o.softmax_rows(x.to(dev), BF)
    assert yb.dtype == BF
    yb = yb.double().cpu()
    assert ((yb - ref).abs() <= 2.0 ** -8 * ref + FLT_MIN).all(), \
        f"bf16: {((yb - ref).abs() / (ref + FLT_MIN)).max().item():.3e} relative"


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("V", SM_V[1:])
def test_softmax_bwd_rows_per_element(V, dt):
    """dz = y (dy - sum y dy) from f32 or bf16 operands (the reference takes the same rounded operands), f32 out:
    within 1e-5 of y_k (|dy_k| + sum_j y_j |dy_j|), the terms whose rounding reaches element k. accumulate adds
    into a prefilled buffer (one more f32 rounding of the sum). The outlier row's probabilities are fp32 denormals:
    results below the smallest normal float carry an absolute error (FLT_MIN covers their spacing or a flush)."""
    o = ops()
    x, sm = softmax_case(V)
    y = sm.to(dt)
    dy = torch.randn(y.shape, generator=g(5000 + V)).to(dt)
    yd, dyd = y.double(), dy.double()
    ref = yd * (dyd - (yd * dyd).sum(-1, keepdim=True))
    tol = 1e-5 * yd * (dyd.abs() + (yd * dyd.abs()).sum(-1, keepdim=True)) + FLT_MIN
    dz = o.softmax_bwd_rows(y.to(dev), dy.to(dev))
    assert dz.dtype == torch.float32
    err = (dz.double().cpu() - ref).abs()
    assert (err <= tol).all(), f"{(err > tol).sum().item()} elements off, worst {(err / (tol + 1e-300)).max().item():.2f} x tol"
    pre = torch.randn(y.shape, generator=g(6000 + V))
    acc = pre.clone().to(dev)
    out = o.softmax_bwd_rows(y.to(dev), dy.to(dev), dz=acc, accumulate=True)
    assert out.data_ptr() == acc.data_ptr()
    want = pre.double() + ref
    err = (acc.double().cpu() - want).abs()
    assert (err <= tol + 2.0 ** -23 * want.abs()).all(), f"accumulate: {(err > tol + 2.0 ** -23 * want.abs()).sum().item()} elements off"


@pytest.mark.parametrize("V", [2056, 8200, 16392])
def test_softmax_bwd_add_bf16_wide_rows(V):
    """softmax_bwd_add_kernel<NV>: V = 2056 NV = 2, 8200 NV = 8, 16392 NV = 16 (NV = 1 and 4 run in
    test_gpu_kernels); the bound of that test; in place over `add` gives the same bits."""
    o = ops()
    N = 5
    x = 3 * torch.randn(N, V, generator=g(7000 + V))
    y = torch.softmax(x, -1).to(BF)
    dy = torch.randn(N, V, generator=g(7100 + V)).to(BF)
    add = (1e-3 * torch.randn(N, V, generator=g(7200 + V))).to(BF)
    yd, dyd = y.double(), dy.double()
    ref = yd * (dyd - (yd * dyd).sum(-1, keepdim=True)) + add.double()
    out = o.softmax_bwd_add_bf16(y.to(dev), dy.to(dev), add.to(dev)).cpu().double()
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().amax(-1, keepdim=True)
    assert ((out - ref).abs() <= tol).all()
    a = add.to(dev)
    o.softmax_bwd_add_bf16(y.to(dev), dy.to(dev), a, out=a)
    assert torch.equal(a.cpu().double(), out)


# ------------------------------------------------------------------------------------------ scale_if / axpy_if
GRID_SPAN = 4096 * 256 * 8      # elements one pass of the capped grid (4096 blocks x 256 threads x 8) covers


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("n", [GRID_SPAN + 8 * 300 + 5, 5])
def test_scale_if_grid_stride_and_tail(n, dt):
    """n past one pass of the capped grid (a second grid-stride iteration) with n % 8 = 5 (the scalar tail), and the
    tail alone: g = 1 touches nothing, g = -3 is exact in f32 and one bf16 rounding (2^-8 relative) in bf16."""
    o = ops()
    x = torch.randn(n, generator=g(80)).to(dt).to(dev)
    before = x.clone()
    o.scale_if(x, torch.ones(1, device=dev))
    assert torch.equal(x, before)
    o.scale_if(x, torch.full((1,), -3.0, device=dev))
    if dt == torch.float32:
        bad = x != before * -3.0
    else:
        ref = before.double() * -3.0
        bad = (x.double() - ref).abs() > 2.0 ** -8 * ref.abs()
    assert not bad.any().item(), f"{bad.sum().item()} elements off, first at {bad.nonzero()[0].item()}"


def test_axpy_if_bf16_grid_stride():
    """n past one pass of the capped grid: g = 1 touches nothing; g = 3 gives x + 2 y within one bf16 rounding
    (2^-8 relative; 2^-23 (|x| + 2 |y|) for the f32 sum before it)."""
    o = ops()
    n = GRID_SPAN + 8 * 77
    x = torch.randn(n, generator=g(81)).to(BF).to(dev)
    y = torch.randn(n, generator=g(82)).to(BF).to(dev)
    before = x.clone()
    o.axpy_if_bf16(x, y, torch.ones(1, device=dev))
    assert torch.equal(x, before)
    o.axpy_if_bf16(x, y, torch.full((1,), 3.0, device=dev))
    ref = before.double() + 2.0 * y.double()
    bad = (x.double() - ref).abs() > 2.0 ** -8 * ref.abs() + 2.0 ** -23 * (before.double().abs() + 2.0 * y.double().abs())
    assert not bad.any().item(), f"{bad.sum().item()} elements off, first at {bad.nonzero()[0].item()}"


# ------------------------------------------------------------------------------------------ kl_reduce / sample_q
@pytest.mark.parametrize("B,L", [(33, 70), (16, 64), (17, 1), (1024, 3)])
def test_kl_reduce_batches_beyond_one_wave_each(B, L):
    """One wave per utterance, 16 waves: B > 16 runs the b += 16 loop again (the benchmark's batch is 32), B = 1024
    fills the per-utterance buffer. With a mask (one all-padding utterance: 0 / (0 + eps)) and without."""
    o = ops()
    gen = g(90 + B)
    kl = torch.rand(B * L, generator=gen)
    m = torch.rand(B, L, generator=gen) > 0.3
    m[B // 2] = False
    m[B - 1] = True
    loss, w = o.kl_reduce(kl.to(dev), m.reshape(-1).to(dev).view(torch.uint8), B, L)
    v = m.double()
    per = (kl.view(B, L).double() * v).sum(1) / (v.sum(1) + 1e-8)
    close(loss, per.mean(), rtol=1e-6, what="kl_reduce loss")
    close(w.view(B, L), v / (v.sum(1, keepdim=True) + 1e-8) / B, rtol=1e-6, what="kl_reduce w")
    loss2, w2 = o.kl_reduce(kl.to(dev), None, B, L)
    close(loss2, kl.double().mean(), rtol=1e-6, what="kl_reduce unmasked")
    close(w2, torch.full((B * L,), 1.0 / (B * L)), rtol=1e-6, what="kl_reduce unmasked w")


def test_kl_reduce_rejects_more_utterances_than_its_buffer():
    o = ops()
    with pytest.raises(RuntimeError):
        o.kl_reduce(torch.zeros(1025 * 2, device=dev), None, 1025, 2)


@pytest.mark.parametrize("K", [2, 37, 8000])
def test_sample_q_bit_exact_small_and_full_vocab(K):
    """sample_q against oracle.sample_xt, bit for bit: B L = 257 (a second, partly filled block), t with 1 and T,
    x0 with 0 and K - 1."""
    o = ops()
    B, L = 257, 1
    _, ab = O.sched_tables(TN)
    x0 = torch.randint(0, K, (B, L), generator=g(95 + K))
    x0[0, 0], x0[1, 0], x0[256, 0] = 0, K - 1, K - 1
    t = torch.randint(1, TN + 1, (B,), generator=g(96 + K))
    t[0], t[1], t[255], t[256] = 1, TN, TN, 1
    thr = torch.from_numpy(O.sample_thresholds(K, ab).astype(np.uint32).view(np.int32)).to(dev)
    xt = o.sample_q(x0.to(dev), t.to(dev), thr, K, 1234)
    ref = O.sample_xt(x0, t, K, ab, seed=1234, stream=1)
    assert torch.equal(xt.cpu(), ref)
    assert int(xt.min()) >= 0 and int(xt.max()) < K
