"""The two front-end kernels of the WavLM-Large family per element against float64 (csrc/norm.hip:
conv0_ln_gelu_kernel<float|bf16>, ln_gelu_fwd_kernel<f32|bf16, f32|bf16>), and ln_fwd at d = 1024 in the dtype
combinations the pre-LN residual stream uses.

Cases (wavlm_large_ref): conv0_ln_gelu at C 32 (4 of 64 lanes hold channels) and 512 (every lane), f32 and bf16 output,
T0 1, 67 (a second 64-frame block of three frames) and 4097, three utterances (unit noise; noise on a DC offset of 50;
one whose middle third is exact zeros, so its frames there are the bias vector), nsamp = (T0 - 1) 5 + 13 so that three
tail samples reach no frame; and a constant bias (variance 0 in the silent frames, rstd = eps^-1/2). ln_gelu_fwd at d
32 and 512, N 1, 33, 4099 (a last workgroup of three rows), f32 and bf16 in and out, and in place; row N // 2 is
constant. Every output is written into a slice of a NaN-filled buffer whose row before and row after must keep their
bits.

Bound per element: |gelu'(z)| C u s + the GELU form's absolute error (2e-6 for the erf form of the f32 outputs, 2.6e-5
for gelu_bf16out), then one bf16 rounding for bf16 outputs; u = 2^-24, s the absolute-value evaluation of z including
rstd, C = 8 E with E measured on the CPU from the emulation alone (tests/test_cpu_wavlm_large.py):
    conv0_ln  C = 44.0      ln_gelu  C = 43.6

Measured on an MI355X, the largest share of its bound any element used: conv0_ln f32 0.103, bf16 0.998; ln_gelu f32
0.105, bf16 0.999 (a correctly rounded bf16 value next to a rounding boundary uses the whole half ulp; the f32 share
is mostly gelu_f's own error against its 2e-6 allowance).
"""
import functools

import pytest
import torch

import wavlm_large_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()


def _ops():
    from fddm_hip import ops
    return ops


def _guarded(rows, width, dt):
    """A NaN-filled [rows + 2, width] buffer, its inner rows, and the bits of the two guard rows."""
    buf = torch.full((rows + 2, width), float("nan"), device=dev, dtype=dt)
    bits = torch.int16 if dt == BF else torch.int32
    return buf, buf[1:-1], buf[[0, -1]].view(bits).clone(), bits


def _check(what, out, r, which):
    bf16_out = out.dtype == BF
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    got = out.double().cpu().reshape(r.ref.shape)
    err = (got - r.ref).abs()
    bound = R.row_bound(r, which, bf16_out)
    share = (err / bound).max().item()
    print(f"LARGEK {what}: share of bound {share:.3f}")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements leave their bound, the worst by {share:.2f}"


@functools.lru_cache(maxsize=None)
def _conv0_ref(C, T0, const_bias):
    w, bias, gamma, beta = R.conv0_ln_params(C, const_bias)
    return R.conv0_ln_ref64(R.conv0_ln_wave(T0), w, bias, gamma, beta)


CONV0 = [(C, T0, False) for C in R.CONV0_LN_C for T0 in R.CONV0_LN_T0] + [(32, 67, True), (512, 67, True)]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,T0,const_bias", CONV0, ids=[f"C{c}-T{t}" + ("-constbias" if k else "") for c, t, k in CONV0])
def test_conv0_ln_gelu(C, T0, const_bias, dt):
    o = _ops()
    w, bias, gamma, beta = (t.to(dev) for t in R.conv0_ln_params(C, const_bias))
    wave = R.conv0_ln_wave(T0).to(dev)
    r = _conv0_ref(C, T0, const_bias)
    buf, inner, guard, bits = _guarded(3 * T0, C, dt)
    out = o.conv0_ln_gelu(wave, w, bias, gamma, beta, dt, C, R.K0, R.S0, eps=R.LN_EPS, out=inner.view(3, T0, C))
    torch.cuda.synchronize()
    assert out.dtype == dt and out.shape == (3, T0, C)
    assert torch.equal(buf[[0, -1]].view(bits), guard), "conv0_ln_gelu wrote outside its B*T0 rows"
    _check(f"conv0_ln C={C} T0={T0} {'const bias ' if const_bias else ''}{dt}", out, r, "conv0_ln")


@functools.lru_cache(maxsize=None)
def _ln_gelu_ref(N, d, xdt):
    x, gamma, beta = R.ln_gelu_operands(N, d, xdt)
    return R.ln_gelu_ref64(x, gamma, beta)


LN_GELU = [(d, N) for d in R.LN_GELU_D for N in R.LN_GELU_N]


@pytest.mark.parametrize("xdt,odt,inplace", [(F32, F32, False), (F32, BF, False), (BF, F32, False), (BF, BF, False),
                                             (F32, F32, True), (BF, BF, True)],
                         ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16", "f32-inplace", "bf16-inplace"])
@pytest.mark.parametrize("d,N", LN_GELU, ids=[f"d{d}-N{n}" for d, n in LN_GELU])
def test_ln_gelu_fwd(d, N, xdt, odt, inplace):
    o = _ops()
    x, gamma, beta = R.ln_gelu_operands(N, d, xdt)
    r = _ln_gelu_ref(N, d, xdt)
    buf, inner, guard, bits = _guarded(N, d, odt)
    if inplace:
        inner.copy_(x.to(dev))
        src = inner
    else:
        src = x.to(dev)
    out = o.ln_gelu_fwd(src, gamma.to(dev), beta.to(dev), out=inner, eps=R.LN_EPS)
    torch.cuda.synchronize()
    assert out.data_ptr() == inner.data_ptr() and out.dtype == odt
    assert torch.equal(buf[[0, -1]].view(bits), guard), "ln_gelu_fwd wrote outside its N rows"
    _check(f"ln_gelu d={d} N={N} {xdt}->{odt}{' in place' if inplace else ''}", out, r, "ln_gelu")


def test_new_ops_refuse_bad_arguments():
    o = _ops()
    z = lambda *s, dt=F32: torch.zeros(*s, device=dev, dtype=dt)   # noqa: E731
    wave, w, v = z(2, 33), z(32, 10), z(32)
    assert o.conv0_ln_gelu(wave, w, v, v, v, F32, 32, 10, 5).shape == (2, 5, 32)
    for args in [(wave, z(32, 8), v, v, v, F32, 32, 8, 5), (wave, z(31, 10), z(31), z(31), z(31), F32, 31, 10, 5),
                 (wave, z(36, 10), z(36), z(36), z(36), F32, 36, 10, 5), (wave, w, v, v, z(33), F32, 32, 10, 5),
                 (wave, w, v.double(), v, v, F32, 32, 10, 5), (wave[:, :9].contiguous(), w, v, v, v, F32, 32, 10, 5),
                 (wave, w, v, v, v, torch.float16, 32, 10, 5)]:
        with pytest.raises(ValueError):
            o.conv0_ln_gelu(*args)
    x = z(5, 64)
    assert o.ln_gelu_fwd(x, z(64), z(64)).shape == (5, 64)
    for args, kw in [((z(5, 520), z(520), z(520)), {}), ((z(5, 60), z(60), z(60)), {}), ((x, z(32), z(64)), {}),
                     ((x.t().contiguous().t(), z(5), z(5)), {}), ((x, z(64), z(64)), dict(out=x.view(BF)[:, :64])),
                     ((x, z(64), z(64)), dict(out=z(4, 64)))]:
        with pytest.raises(ValueError):
            o.ln_gelu_fwd(*args, **kw)


# ------------------------------------------------------------------------------------------ ln_fwd at d = 1024
@pytest.mark.parametrize("xdt,ydt,odt,inplace", [(F32, BF, BF, True), (F32, BF, BF, False), (BF, BF, BF, False),
                                                 (F32, F32, F32, True)],
                         ids=["f32+bf16-inplace", "f32+bf16", "bf16+bf16", "f32+f32-inplace"])
def test_ln_fwd_prelen_stream_d1024(xdt, ydt, odt, inplace):
    """ln_fwd as the pre-LN stream launches it at d = 1024 (two chunks per lane), N = 98 (two rows in the last
    workgroup): x + y -> save_s (f32, the new residual; in place over x in the layers) and LN(x + y) -> out_t, no
    mean / rstd. Per element with the bounds of tests/test_gpu_norm_lfd.py: save_s within 1e-6 absolute (|s| < 8,
    asserted), a bf16 out_t within 2^-8 |ref| + 1e-3, an f32 out_t within 1e-5 of the largest reference magnitude. The
    rounding-derived per-element bounds of ln_fwd are in tests/test_gpu_norm_lfd_elem.py."""
    o = _ops()
    N, d = 98, 1024
    gen = torch.Generator().manual_seed(1024)
    x = torch.randn(N, d, generator=gen).to(xdt)
    y = (0.5 * torch.randn(N, d, generator=gen) + 0.3).to(ydt)
    gm, bt = 1 + 0.1 * torch.randn(d, generator=gen), 0.1 * torch.randn(d, generator=gen)
    s = x.double() + y.double()
    assert s.abs().max().item() < 8.0
    ref = torch.nn.functional.layer_norm(s, (d,), gm.double(), bt.double(), 1e-5)
    xd = x.to(dev)
    out = torch.full((N + 2, d), float("nan"), device=dev, dtype=odt)
    sv = xd if inplace else torch.full((N, d), float("nan"), device=dev)
    o.ln_fwd(xd, y.to(dev), gm.to(dev), bt.to(dev), out_t=out[1:-1], save_s=sv, eps=1e-5)
    torch.cuda.synchronize()
    assert torch.isnan(out[[0, -1]]).all(), "ln_fwd wrote outside its N rows"
    got, gs = out[1:-1].double().cpu(), sv.double().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(gs).all()
    es = (gs - s).abs()
    assert (es <= 1e-6).all(), f"save_s: max err {es.max().item():.3e}"
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-3 if odt == BF else torch.full_like(ref, 1e-5 * ref.abs().max().item())
    assert (err <= bound).all(), f"out_t: {int((err > bound).sum())} elements off, max err {err.max().item():.3e}"
