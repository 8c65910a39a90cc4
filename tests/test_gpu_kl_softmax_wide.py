"""The streamed ("wide") KL and softmax kernels of csrc/kl.hip per element against float64, for vocabularies the
resident kernels cannot hold (and, at V = 36 and 2052, beside them on the same inputs).

Inputs, references, bounds and their derivation: tests/wide_cases.py. Per V the gradient bound is C_GRAD[V] =
min(8 x ORACLE_C[V], 1e-4) in units of the per-element error scale s_k (helpers.kl_term_ref64), the per-token bound
8 x (ORACLE_A[V] + ORACLE_R[V] |ref|); tests/test_cpu_wide_vocab.py re-measures the ORACLE_* on the CPU.

Measured (fp32 oracle on the CPU | the kernels on an MI355X: the largest over f32 / bf16 dz, masked / unmasked, the
fused and the forward-only kernel, aligned and shifted rows), gradient in s_k, per token absolute / relative:
         V    oracle C   kernels C    oracle A / R           kernels A / R
        36    5.99e-7    7.7e-7      1.34e-7 / 3.06e-7      1.9e-7 / 3.9e-7
      2052    1.26e-6    1.04e-6     1.21e-7 / 2.87e-7      1.4e-7 / 2.4e-7
     16383    1.19e-6    1.26e-6     1.16e-7 / 2.96e-7      2.2e-7 / 6.6e-7
     16384    1.98e-6    1.50e-6     7.96e-8 / 6.01e-7      9.0e-8 / 2.7e-7
     16385    1.37e-6    1.31e-6     6.14e-8 / 7.94e-7      2.2e-7 / 2.1e-7
     16388    1.81e-6    1.55e-6     1.11e-7 / 4.62e-7      2.2e-7 / 2.5e-7
     32772    2.74e-6    1.59e-6     1.35e-7 / 1.04e-6      1.6e-7 / 5.2e-7
     50257    3.32e-6    1.73e-6     1.07e-7 / 1.59e-6      1.1e-7 / 5.6e-7
     65536    2.81e-6    1.60e-6     1.87e-7 / 1.12e-6      1.3e-7 / 2.7e-7
    131076    6.00e-6    1.57e-6     1.06e-7 / 5.36e-6      9.3e-8 / 9.3e-7
The kernels' gradient error stays at ~1.6e-6 s_k while the oracle's grows with V: the kernels sum a row as 512 per-
thread partial sums merged in a tree, the oracle in one sequence. The resident kernels on the V = 36 and 2052 inputs:
6.4e-7 and 1.19e-6 s_k. Discriminating shares over every generic element of the unmasked rows (tests/wide_cases.py
check_preconditions, masked / unmasked case): 0.827 / 0.871 at V = 36, 0.906 / 0.871 at 2052 (floor 0.5); 0.99958 /
0.99977, 0.99997 / 0.99987, 0.99781 / 0.99869, 0.99925 / 0.99963 at 16383 - 16388 (floor 0.997); 0.99949 / 0.99975 at
32772, 0.99999 / 0.99998 at 50257, 1.00000 / 0.99995 at 65536, 0.99999 / 0.99999 at 131076 (floor 0.999).

Every case also runs into destination slices of larger buffers filled with a sentinel: the rows before and after dz (the ABI has
no leading dimension, so there are no guard columns) and the elements on either side of kl_tok must keep their bits.
"""
import functools

import pytest
import torch

import wide_cases as W
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
FLT_MIN = 2.0 ** -126
SENTINEL = 0x5A5A5A5B           # every 32-bit word of a guarded buffer before the kernel runs


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()


def ops():
    from fddm_hip import ops as o
    return o


@pytest.fixture(scope="module", params=W.WIDE_V)
def cases(request):
    """(masked case, unmasked case) of one V, preconditions asserted on the CPU side; module scope groups every test
    of one V, so each float64 reference is computed once."""
    V = request.param
    cs = W.kl_case(V, True), W.kl_case(V, False)
    for c in cs:
        print(f"V={V} masked={c.masked}: discriminating share {W.check_preconditions(c):.5f}, p_min {c.pmin:.1e}")
    return cs


def dev_args(c, logits=None):
    """(logits [N, V], xt, x0, t, betas) on the device."""
    return (c.logits.view(-1, c.V).to(dev) if logits is None else logits, c.xt.reshape(-1).to(dev),
            c.x0.reshape(-1).to(dev), c.t.to(dev), c.betas.to(dev))


def mask_u8(c):
    return c.xm.reshape(-1).to(dev).view(torch.uint8) if c.masked else None


GUARD = 2                       # guard rows on either side: 2 V elements keep a V % 4 == 0 slice 16-byte aligned


def guarded(rows, cols, dtype):
    """(raw, inner): a buffer of sentinel words that holds [rows + 2 GUARD, cols] elements of dtype, and its inner
    [rows, cols] slice (contiguous): GUARD guard rows before it and after it."""
    words = (rows + 2 * GUARD) * cols * torch.empty(0, dtype=dtype).element_size() // 4 + 1
    raw = torch.full((words,), SENTINEL, dtype=torch.int32, device=dev)
    return raw, raw.view(dtype)[:(rows + 2 * GUARD) * cols].view(rows + 2 * GUARD, cols)[GUARD:GUARD + rows]


def guards_intact(raw, inner, what):
    """Every bit of the buffer outside the inner slice is still the sentinel's: a fresh sentinel buffer with the
    inner slice copied in equals the buffer word for word."""
    rows, cols = inner.shape
    want, win = guarded(rows, cols, inner.dtype)
    win.copy_(inner)
    assert torch.equal(raw, want), f"{what}: {(raw != want).sum().item()} words outside the destination changed"


def shifted_copy(x2d):
    """The rows of x2d [N, V] from a base one float past a 16-byte boundary."""
    N, V = x2d.shape
    buf = torch.empty(N * V + 1, device=dev)
    s = buf[1:].view(N, V)
    s.copy_(x2d)
    assert s.data_ptr() % 16 == 4
    return s


def run_fused_wide(c, what, dt, logits=None):
    """fddm_kl_fused_wide into guarded destinations: dz and kl_tok against float64, the guards bit-unchanged."""
    o = ops()
    N = c.B * c.L
    raw, dz = guarded(N, c.V, dt)
    kraw, kl2d = guarded(1, N, torch.float32)           # N sentinel elements on either side of kl_tok
    k2, d2 = o.kl_fused_wide(*dev_args(c, logits), mask_u8(c), c.L, kl_tok=kl2d[0], dz=dz)
    assert k2.data_ptr() == kl2d.data_ptr() and d2.data_ptr() == dz.data_ptr()
    a, r = W.check_kl_tok(kl2d[0], c, what)
    need = W.check_dz(dz, c, what)
    guards_intact(raw, dz, f"{what} dz")
    guards_intact(kraw, kl2d, f"{what} kl_tok")
    return need, a, r


# fddm_kl_fused_wide, kl_wide_kernel<VEC, true, float | bf16_t>: VEC = true at V % 4 == 0 (dz's guarded slice starts
# 2 V elements into an aligned buffer, so it stays 16-byte aligned there), false at the odd V; every V of W.WIDE_V,
# masked (one fully masked utterance: dz rows exactly 0, kl_tok finite) and unmasked, dz as f32 and bf16.
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_kl_fused_wide_per_element(cases, dt):
    for c in cases:
        run_fused_wide(c, f"kl_fused_wide V={c.V} masked={c.masked} {dt}", dt)


@pytest.mark.parametrize("V", [2052, 32772])
def test_kl_fused_wide_unaligned_base_takes_scalar_kernel(V):
    """Multiples of 4 on rows that start 4 bytes past a 16-byte boundary: the alignment test of fddm_kl_fused_wide
    sends them to the scalar-access instantiation."""
    c = W.kl_case(V, True)
    s = shifted_copy(c.logits.view(-1, c.V).to(dev))
    for dt in (torch.float32, BF):
        run_fused_wide(c, f"kl_fused_wide V={c.V} shifted {dt}", dt, logits=s)


@pytest.mark.parametrize("V", [36, 2052])
def test_kl_wide_agrees_with_resident_kernels_below_one_chunk(V):
    """The resident one-pass kernel and the resident forward on the same inputs meet the same bounds, and the two
    gradients differ by no more than the two bounds together."""
    o = ops()
    for c in (W.kl_case(V, True), W.kl_case(V, False)):
        a = dev_args(c)
        kr, dr = o.kl_fused(*a, mask_u8(c), c.L)
        kw, dw = o.kl_fused_wide(*a, mask_u8(c), c.L)
        W.check_kl_tok(kr, c, f"resident fused V={c.V}")
        W.check_dz(dr, c, f"resident fused V={c.V}")
        W.check_kl_tok(o.kl_fwd(*a, c.L), c, f"resident fwd V={c.V}")
        diff = (dw.double() - dr.double()).abs().view(c.B, c.L, c.V).cpu()
        assert (diff <= 2 * W.c_grad(c.V) * c.s).all()
        At, Rt = W.tok_bounds(c.V)
        assert ((kw.double() - kr.double()).abs().cpu() <= 2 * (At + Rt * c.kl.abs().view(-1))).all()


# fddm_kl_fwd_wide, kl_wide_kernel<VEC, false, float>, the same V; and on a shifted base where V % 4 == 0
def test_kl_fwd_wide_per_token(cases):
    o = ops()
    for c in cases:
        kraw, kl2d = guarded(1, c.B * c.L, torch.float32)
        o.kl_fwd_wide(*dev_args(c), c.L, kl_tok=kl2d[0])
        W.check_kl_tok(kl2d[0], c, f"kl_fwd_wide V={c.V} masked={c.masked}")
        guards_intact(kraw, kl2d, "kl_fwd_wide kl_tok")
    c = cases[0]
    if c.V % 4 == 0:
        s = shifted_copy(c.logits.view(-1, c.V).to(dev))
        W.check_kl_tok(o.kl_fwd_wide(*dev_args(c, s), c.L), c, f"kl_fwd_wide V={c.V} shifted")


# ------------------------------------------------------------------------------------------ softmax
# softmax_wide_kernel<VEC, float | bf16_t> and softmax_bwd_wide_kernel<VEC, float | bf16_t>: 16385 and 50257 scalar
# (50257: rows 1 and 2 unaligned), 16388 = 2 chunks + one float4, 32768 = whole chunks only, 131076 = 16 chunks + 4
SM_V = [16385, 16388, 32768, 50257, 131076]
SM_N = 3


@functools.lru_cache(maxsize=2)
def softmax_case(V):
    """x [3, V] (3 randn; row 0 with a +80 outlier, row 1 all equal) and its float64 softmax."""
    x = 3.0 * torch.randn(SM_N, V, generator=W.g(4000 + V))
    x[0, V // 3] += 80.0
    x[1] = 0.7
    return x, torch.softmax(x.double(), -1)


@pytest.mark.parametrize("V", SM_V)
def test_softmax_rows_wide_per_element(V):
    """f32: within 1e-5 of the row's largest probability; bf16: one rounding, 2^-8 relative per element; below the
    smallest normal float the device exp may flush to zero. Into a guarded slice."""
    o = ops()
    x, ref = softmax_case(V)
    raw, out = guarded(SM_N, V, torch.float32)
    y = o.softmax_rows_wide(x.to(dev), torch.float32, out=out).double().cpu()
    guards_intact(raw, out, "softmax_rows_wide f32")
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= 1e-5 * ref.amax(-1, keepdim=True)).all(), \
        f"f32: {((y - ref).abs() / ref.amax(-1, keepdim=True)).max().item():.3e} of the row max"
    raw, out = guarded(SM_N, V, BF)
    yb = o.softmax_rows_wide(x.to(dev), BF, out=out)
    guards_intact(raw, out, "softmax_rows_wide bf16")
    assert yb.dtype == BF
    yb = yb.double().cpu()
    assert ((yb - ref).abs() <= 2.0 ** -8 * ref + FLT_MIN).all(), \
        f"bf16: {((yb - ref).abs() / (ref + FLT_MIN)).max().item():.3e} relative"
    y2 = o.softmax_rows_wide(x.to(dev), torch.float32)       # a fresh destination: the same bits
    assert torch.equal(y2.double().cpu(), y)


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("V", SM_V)
def test_softmax_bwd_rows_wide_per_element(V, dt):
    """dz = y (dy - sum y dy) from f32 or bf16 operands (the reference takes the same rounded operands), f32 out:
    within 1e-5 of y_k (|dy_k| + sum_j y_j |dy_j|); accumulate adds into a prefilled buffer (one more f32 rounding of
    the sum). Results below the smallest normal float carry an absolute error (FLT_MIN)."""
    o = ops()
    x, sm = softmax_case(V)
    y = sm.to(dt)
    dy = torch.randn(y.shape, generator=W.g(5000 + V)).to(dt)
    yd, dyd = y.double(), dy.double()
    ref = yd * (dyd - (yd * dyd).sum(-1, keepdim=True))
    tol = 1e-5 * yd * (dyd.abs() + (yd * dyd.abs()).sum(-1, keepdim=True)) + FLT_MIN
    raw, out = guarded(SM_N, V, torch.float32)
    dz = o.softmax_bwd_rows_wide(y.to(dev), dy.to(dev), dz=out)
    guards_intact(raw, out, "softmax_bwd_rows_wide")
    assert dz.dtype == torch.float32
    err = (dz.double().cpu() - ref).abs()
    assert (err <= tol).all(), f"{(err > tol).sum().item()} elements off, worst {(err / (tol + 1e-300)).max().item():.2f} x tol"
    pre = torch.randn(y.shape, generator=W.g(6000 + V))
    acc = pre.clone().to(dev)
    res = o.softmax_bwd_rows_wide(y.to(dev), dy.to(dev), dz=acc, accumulate=True)
    assert res.data_ptr() == acc.data_ptr()
    want = pre.double() + ref
    err = (acc.double().cpu() - want).abs()
    assert (err <= tol + 2.0 ** -23 * want.abs()).all(), f"accumulate: {(err > tol + 2.0 ** -23 * want.abs()).sum().item()} elements off"


@pytest.mark.parametrize("V", [32776, 65536, 131080])
def test_softmax_bwd_add_bf16_wide_per_element(V):
    """softmax_bwd_add_wide_kernel: 32776 = 4 chunks + 8, 65536 = whole chunks, 131080 = 16 chunks + 8; the bound of
    the resident kernel's test; in place over `add` gives the same bits; into a guarded slice."""
    o = ops()
    x = 3 * torch.randn(SM_N, V, generator=W.g(7000 + V))
    y = torch.softmax(x, -1).to(BF)
    dy = torch.randn(SM_N, V, generator=W.g(7100 + V)).to(BF)
    add = (1e-3 * torch.randn(SM_N, V, generator=W.g(7200 + V))).to(BF)
    yd, dyd = y.double(), dy.double()
    ref = yd * (dyd - (yd * dyd).sum(-1, keepdim=True)) + add.double()
    raw, dst = guarded(SM_N, V, BF)
    out = o.softmax_bwd_add_bf16_wide(y.to(dev), dy.to(dev), add.to(dev), out=dst).cpu().double()
    guards_intact(raw, dst, "softmax_bwd_add_bf16_wide")
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().amax(-1, keepdim=True)
    assert ((out - ref).abs() <= tol).all()
    a = add.to(dev)
    o.softmax_bwd_add_bf16_wide(y.to(dev), dy.to(dev), a, out=a)
    assert torch.equal(a.cpu().double(), out)


def test_softmax_bwd_add_bf16_wide_agrees_with_resident_kernel():
    """V = 32768, which both forms serve: the same bound, and results that differ by at most one bf16 rounding of it
    (the row sum is taken in another order)."""
    o = ops()
    V = 32768
    x = 3 * torch.randn(SM_N, V, generator=W.g(7000 + V))
    y = torch.softmax(x, -1).to(BF).to(dev)
    dy = torch.randn(SM_N, V, generator=W.g(7100 + V)).to(BF).to(dev)
    add = (1e-3 * torch.randn(SM_N, V, generator=W.g(7200 + V))).to(BF).to(dev)
    a, b = o.softmax_bwd_add_bf16(y, dy, add).double(), o.softmax_bwd_add_bf16_wide(y, dy, add).double()
    assert ((a - b).abs() <= 2.0 ** -7 * a.abs() + 1e-3 * a.abs().amax(-1, keepdim=True)).all()


# ------------------------------------------------------------------------------------------ range
def test_wide_range_raises_before_launch():
    """V = 2^24 + 4 (and V = 1) is a ValueError naming the range from every wide wrapper, raised in ops before any
    launch (and before the V % 8 test of softmax_bwd_add_bf16_wide, which refuses 32772 by that rule)."""
    o = ops()
    betas = O.sched_tables(W.TN)[0].to(dev)
    i = torch.zeros(2, dtype=torch.long, device=dev)
    t = torch.ones(1, dtype=torch.long, device=dev)
    for V in ((1 << 24) + 4, 1):
        z = torch.zeros(2, V, device=dev)
        zb = torch.zeros(2, V, device=dev, dtype=BF)
        with pytest.raises(ValueError, match="supported range"):
            o.kl_fwd_wide(z, i, i, t, betas, 2)
        with pytest.raises(ValueError, match="supported range"):
            o.kl_fused_wide(z, i, i, t, betas, None, 2)
        with pytest.raises(ValueError, match="supported range"):
            o.softmax_rows_wide(z, torch.float32)
        with pytest.raises(ValueError, match="supported range"):
            o.softmax_bwd_rows_wide(z, z)
        with pytest.raises(ValueError, match="supported range"):
            o.softmax_bwd_add_bf16_wide(zb, zb, zb)
    zb = torch.zeros(2, 32772, device=dev, dtype=BF)
    with pytest.raises(ValueError, match="V % 8"):
        o.softmax_bwd_add_bf16_wide(zb, zb, zb)
