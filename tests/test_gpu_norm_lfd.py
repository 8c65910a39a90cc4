"""LayerNorm / FiLM (csrc/norm.hip) and L_fd (csrc/lfd.hip) kernels at the shapes and dtypes the train step launches.

Every test compares one kernel (or one dispatch branch of it) with a float64 torch reference built from the same
inputs after their rounding to the storage dtype. Shapes are the smallest that reach the branch the docstring names.
Tolerances: f32 outputs within 1e-5 (forward) / 1e-4 (gradients) of the largest reference magnitude, the bars of
test_gpu_kernels.py; a bf16 output within its own rounding (2^-8 relative per element) plus the f32 bar; the file-wide
bf16 bar TOL for a whole bf16 pipeline (L_fd end to end); dropout masks and the bf16 copy of an f32 output bit-exact.
The per-element bars of these kernels (rounding-derived bounds on rows with offsets, outliers and zero variance, every
build) are in tests/test_gpu_norm_lfd_elem.py and DESIGN §4.14; this file keeps the train step's shapes.
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from helpers import close
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
bf, f32 = torch.bfloat16, torch.float32
EPS = 1e-5
SEED, STREAM = 11, 5
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
GUARD = 7.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    from fddm_hip import ops
    assert torch.cuda.is_available()
    return ops


def ops():
    from fddm_hip import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def X(t):
    return None if t is None else t.to(dev).contiguous()


def bf16_close(a, ref, atol, what):
    """Every element within the bf16 output rounding of the float64 reference: |err| <= 2^-8 |ref| + atol."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - ref).abs()
    bad = err > 2.0 ** -8 * ref.abs() + atol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, max err {err.max().item():.3e}"


# ------------------------------------------------------------------------------------- LayerNorm
@functools.lru_cache(maxsize=None)
def ln_case(d, B, L, film, p, xdt=f32, ydt=bf):
    """Seeded inputs of one LayerNorm (rounded to their storage dtypes) and its float64 reference with gradients:
    s = x + y keep / (1 - p), out = layer_norm(s) gamma + beta, then FiLM per batch of L rows. Computed once per
    shape and shared (never modified) by every test of that shape."""
    N = B * L
    x = torch.randn(N, d, generator=g(100)).to(xdt)
    y = None if ydt is None else (0.5 * torch.randn(N, d, generator=g(101)) + 0.3).to(ydt)
    gm = 1 + 0.1 * torch.randn(d, generator=g(102))
    bt = 0.1 * torch.randn(d, generator=g(103))
    fs = 0.2 * torch.randn(B, d, generator=g(104))
    fh = 0.2 * torch.randn(B, d, generator=g(105))
    dout = torch.randn(N, d, generator=g(106))
    keep = O.dropout_keep(SEED, STREAM, N * d, p).view(N, d) if p > 0 else torch.ones(N, d, dtype=torch.bool)
    xr, gr, br, fsr, fhr = (t.double().requires_grad_(True) for t in (x, gm, bt, fs, fh))
    yr = None if y is None else y.double().requires_grad_(True)
    s = xr if y is None else xr + yr * keep.double() / (1 - p)
    out = F.layer_norm(s, (d,), gr, br, EPS)
    if film:
        out = (out.view(B, L, d) * (1 + fsr[:, None]) + fhr[:, None]).view(N, d)
    out.backward(dout.double())
    sd = s.detach()
    return SimpleNamespace(
        d=d, B=B, L=L, N=N, film=film, p=p, x=x, y=y, gm=gm, bt=bt, fs=fs, fh=fh, dout=dout, keep=keep, s=sd,
        out=out.detach(), mean=sd.mean(1), rstd=1 / torch.sqrt(sd.var(1, unbiased=False) + EPS), dx=xr.grad,
        dy=None if y is None else yr.grad, dgm=gr.grad, dbt=br.grad, dfs=fsr.grad if film else None,
        dfh=fhr.grad if film else None)


def run_ln_fwd(c, full):
    """ops.ln_fwd of case c on the GPU: out_t (bf16), mean, rstd and, if full, out_f32 and save_s too."""
    o = ops()
    N, d = c.N, c.d
    r = SimpleNamespace(of=None, sv=None, ot=torch.empty(N, d, device=dev, dtype=bf), mean=torch.empty(N, device=dev),
                        rstd=torch.empty(N, device=dev))
    if full:
        r.of = torch.empty(N, d, device=dev)
        r.sv = torch.empty(N, d, device=dev)
    o.ln_fwd(X(c.x), X(c.y), X(c.gm), X(c.bt), out_f32=r.of, out_t=r.ot, save_s=r.sv, mean=r.mean, rstd=r.rstd,
             film=(X(c.fs), X(c.fh)) if c.film else None, rows_per_batch=c.L, eps=EPS, drop_p=c.p, seed=SEED,
             rng_stream=STREAM)
    torch.cuda.synchronize()
    return r


LN_FWD_CASES = [
    #            x    y     d    B   L     FiLM   p    out_f32 + save_s
    pytest.param(f32, bf, 512, 1, 1101, False, 0.1, True, id="decoder-ln1-N1101"),
    pytest.param(f32, bf, 512, 3, 37, True, 0.1, True, id="decoder-ln2-film-L37"),
    pytest.param(f32, bf, 1024, 2, 64, True, 0.1, True, id="two-chunks-d1024"),
    pytest.param(f32, bf, 520, 2, 64, True, 0.1, True, id="two-chunks-d520"),
    pytest.param(f32, bf, 200, 1, 37, False, 0.1, True, id="d200-fewer-chunks-than-lanes"),
    pytest.param(f32, f32, 512, 37, 1, True, 0.0, False, id="f32-to-bf16-d512"),
    pytest.param(f32, f32, 768, 37, 1, True, 0.0, False, id="f32-to-bf16-d768"),
    pytest.param(bf, None, 512, 1, 1001, False, 0.0, False, id="no-residual-d512"),
    pytest.param(bf, None, 768, 1, 1001, False, 0.0, False, id="no-residual-d768"),
]


@pytest.mark.parametrize("xdt,ydt,d,B,L,film,p,full", LN_FWD_CASES)
def test_ln_fwd_train_step_forms(xdt, ydt, d, B, L, film, p, full):
    """ln_fwd_kernel at the forms the train step launches, none of which the other LayerNorm tests reach:
    - decoder LN1, ln_fwd_kernel<float, bf16_t, bf16_t, true, false, 1> with dropout and all five outputs; N = 1101
      leaves one row in the last 4-row workgroup (three waves exit at row >= N);
    - decoder LN2, <.., true, true, 1>: FiLM with L = 37 rows per batch, so a 4-row workgroup spans two FiLM
      batches (rows 36 | 37) and b = row / rows_per_batch must be per wave;
    - <.., 2> at d = 1024 (every lane has two chunks) and d = 520 (65 chunks: the second chunk is lane 0 alone, all
      other lanes reload the last chunk and must contribute zeros); d = 200: 25 chunks, 39 idle lanes in chunk 0;
    - the (f32, f32 -> bf16) dispatch branch with FiLM at d = 512 (CH 1) and 768 (CH 2), one FiLM batch per row
      (rows_per_batch = 1: the smallest shape in which every row reads another FiLM row);
    - WavLM's feature-projection LayerNorm ln_fwd_kernel<bf16_t, bf16_t, bf16_t, false, false, C> with y = None.
    Reference: float64 layer_norm(x + y keep / (1 - p)) then FiLM, on the inputs as stored. out_f32 within 1e-5;
    save_s within 1e-6 absolute (one rounding of y / (1 - p) and one of the sum: <= 2^-22 + 2^-21 = 7.2e-7 while
    |s| < 8, asserted); mean / rstd within 1e-5 / 1e-4; out_t bit-equal to the bf16 rounding of out_f32 where both
    are written (same registers, round-to-nearest-even), else within 2^-8 |ref| + 1e-3."""
    c = ln_case(d, B, L, film, p, xdt, ydt)
    r = run_ln_fwd(c, full)
    close(r.mean, c.mean, rtol=1e-5, what="mean")
    close(r.rstd, c.rstd, rtol=1e-4, what="rstd")
    if full:
        assert c.s.abs().max().item() < 8.0
        close(r.of, c.out, rtol=1e-5, what="out_f32")
        close(r.sv, c.s, rtol=0.0, atol=1e-6, what="save_s")
        assert torch.equal(r.ot, r.of.to(bf)), "out_t is not the bf16 rounding of out_f32"
    else:
        bf16_close(r.ot, c.out, 1e-3, "out_t")


# id -> (d, B, L, FiLM, how): "fwd" = s / mean / rstd from ops.ln_fwd on the GPU; "torch" = built with torch in f32
# (ln_fwd rejects d % 8 != 0); "offset" = dres starts 4 bytes into its buffer; "noparams" = dgamma = dbeta = None
LN_BWD_CASES = {
    "ch1-ragged-N1100": (512, 1, 1100, False, "fwd"),
    "ch1-film-spb2": (512, 2, 64, True, "fwd"),
    "ch2-film-spb18": (1024, 2, 576, True, "fwd"),
    "d200": (200, 1, 70, False, "fwd"),
    "d520": (520, 1, 70, False, "fwd"),
    "two-pass-film-L20": (512, 3, 20, True, "fwd"),
    "unvectorised-d100": (100, 1, 70, False, "torch"),
    "unvectorised-dres-offset": (512, 1, 70, False, "offset"),
    "no-param-grads": (512, 1, 70, False, "noparams"),
}
P_BWD = 0.1


def ln_bwd_fused(name):
    """Whether fddm_ln_bwd takes the fused single pass for this case (parameter gradients wanted, vector accesses
    possible, FiLM batches in whole 32-row slabs)."""
    d, B, L, film, how = LN_BWD_CASES[name]
    return how == "fwd" and (not film or L % 32 == 0)


@functools.lru_cache(maxsize=None)
def ln_bwd_state(name):
    """The forward state the backward reads (save_s, mean, rstd), on the GPU, shared by the runs of one case."""
    d, B, L, film, how = LN_BWD_CASES[name]
    c = ln_case(d, B, L, film, P_BWD)
    if how == "torch":
        s = c.s.float()
        return c, SimpleNamespace(sv=X(s), mean=X(c.mean.float()), rstd=X(c.rstd.float()))
    return c, run_ln_fwd(c, True)


@functools.lru_cache(maxsize=None)
def ln_bwd_run(name, dt, fold, rep=0):
    """One ops.ln_bwd of the case on non-zero destinations (rep tells repeated identical runs apart); results on
    the CPU, destinations with their bases still added."""
    o = ops()
    d, B, L, film, how = LN_BWD_CASES[name]
    c, st = ln_bwd_state(name)
    N = c.N
    buf = torch.full((N * d + 1,), GUARD, device=dev)
    dres = buf[1:].view(N, d) if how == "offset" else torch.empty(N, d, device=dev)
    dy = torch.empty(N, d, device=dev, dtype=dt)
    base = ln_bases(d, B)
    dg, db, dfs, dfh = (X(t) for t in base)
    params = how != "noparams"
    lnp = o.LnPartials() if fold else None
    o.ln_bwd(X(c.dout), st.sv, st.mean, st.rstd, X(c.gm), X(c.bt), dres=dres, dy_t=dy, dgamma=dg if params else None,
             dbeta=db if params else None, film_scale=X(c.fs) if film else None, dfilm=(dfs, dfh) if film else None,
             rows_per_batch=L, drop_p=P_BWD, seed=SEED, rng_stream=STREAM, partials=lnp)
    if fold:
        lnp.fold()
    torch.cuda.synchronize()
    return SimpleNamespace(dres=dres.cpu(), dy=dy.cpu(), dg=dg.cpu(), db=db.cpu(), dfs=dfs.cpu(), dfh=dfh.cpu(),
                           lead=buf[0].item())


def ln_bases(d, B):
    """Non-zero starting values of dgamma, dbeta, dfilm_scale, dfilm_shift (the kernels accumulate)."""
    a = torch.linspace(-1, 1, d)
    b = torch.linspace(-2, 2, B * d).view(B, d)
    return a.clone(), 2 * a, b.clone(), -0.5 * b


def check_ln_bwd(name, c, r, dt):
    d, B, L, film, how = LN_BWD_CASES[name]
    base = ln_bases(d, B)
    close(r.dres, c.dx, rtol=1e-4, what="dres")
    if dt == f32:
        close(r.dy, c.dy, rtol=1e-4, what="dy_t f32")
    else:
        bf16_close(r.dy, c.dy, 1e-4 * c.dy.abs().max().item(), "dy_t bf16")
    nz = c.dx != 0
    assert torch.equal((r.dy != 0)[nz], c.keep[nz]), "dy_t: dropout mask differs from the oracle's"
    if how == "offset":
        assert r.lead == GUARD, "the element before an offset dres was written"
    if how != "noparams":
        close(r.dg - base[0], c.dgm, rtol=1e-4, what="dgamma")
        close(r.db - base[1], c.dbt, rtol=1e-4, what="dbeta")
    else:
        assert torch.equal(r.dg, base[0]) and torch.equal(r.db, base[1])
    if film:
        close(r.dfs - base[2], c.dfs, rtol=1e-4, what="dfilm_scale")
        close(r.dfh - base[3], c.dfh, rtol=1e-4, what="dfilm_shift")
    else:
        assert torch.equal(r.dfs, base[2]) and torch.equal(r.dfh, base[3])


LN_BWD_PARAMS = [pytest.param(n, fold, id=f"{n}-{'fold' if fold else 'atomics'}") for n in LN_BWD_CASES
                 for fold in (False, True) if not (fold and LN_BWD_CASES[n][4] == "noparams")]


@pytest.mark.parametrize("dt", [f32, bf], ids=["dy_f32", "dy_bf16"])
@pytest.mark.parametrize("name,fold", LN_BWD_PARAMS)
def test_ln_bwd_train_step_forms(name, fold, dt):
    """ops.ln_bwd at the decoder's forms (f32 x + bf16 y forward on the GPU for save_s / mean / rstd, dropout 0.1,
    dy_t f32 or bf16, parameter gradients by atomics or by LnPartials + fold()) against float64 autograd:
    - ch1-ragged: ln_bwd_fused_kernel<1, T>, d = 512, N = 1100 = 34 slabs of 32 rows + one of 12, whose waves 4-7
      break out of the row loop at once and waves 0-3 after one row; 35 slabs also take the fold loop k += 16 round
      three times;
    - ch1-film: FiLM with L = 64 = 2 slabs per batch (b = r0 / rows_per_batch differs between slabs);
    - ch2: ln_bwd_fused_kernel<2, T>, d = 1024, B = 2, L = 576: 18 slabs per batch, 36 in all, so both the FiLM and
      the dgamma fold loops go round more than once (the smallest whole-slab L past 16 slabs per batch);
    - d200 / d520: chunks < lanes, and a second chunk of one lane (N = 70: three slabs, the last of 6 rows);
    - two-pass: FiLM with L = 20, not whole slabs: ln_bwd_kernel<T> + ln_bwd_params_kernel, whose 64-row slabs span
      FiLM batches; with partials the memset-then-atomics form (fold adds zeros);
    - unvectorised: d = 100 (d % 8 != 0; s, mean, rstd from torch since ln_fwd rejects it) and d = 512 with dres
      starting 4 bytes into its buffer (the element before it must stay): vec_ok == false, the two-pass kernels;
      N = 70 gives ln_bwd_params_kernel two row slabs;
    - no-param-grads: dgamma = dbeta = None, no FiLM: ln_bwd_kernel alone (partials need dgamma: atomics form only).
    Destinations start non-zero and must come back as base + gradient; those of absent quantities unchanged.
    dres, parameter and FiLM gradients and f32 dy_t within 1e-4 of the maximum; bf16 dy_t within
    2^-8 |ref| + 1e-4 max|ref|; the dropout mask exact: (dy_t != 0) == keep wherever the reference dres != 0.
    With fold: the folded and the atomic results agree to 1e-5, and two folded runs of the fused pass are
    bit-identical (fixed summation order; the two-pass form adds with atomics, so only dres / dy_t are compared
    bit for bit there)."""
    c, _ = ln_bwd_state(name)
    r = ln_bwd_run(name, dt, fold)
    check_ln_bwd(name, c, r, dt)
    if not fold:
        return
    ra = ln_bwd_run(name, dt, False)
    r2 = ln_bwd_run(name, dt, True, 1)
    for q in ("dg", "db", "dfs", "dfh"):
        close(getattr(r, q), getattr(ra, q), rtol=1e-5, what=f"fold vs atomics {q}")
        if ln_bwd_fused(name):
            assert torch.equal(getattr(r, q), getattr(r2, q)), f"two folded runs differ in {q}"
    assert torch.equal(r.dres, r2.dres) and torch.equal(r.dy, r2.dy)
    assert torch.equal(r.dres, ra.dres) and torch.equal(r.dy, ra.dy)


def test_ln_fold_four_jobs_one_launch():
    """One ln_fold launch for four LayerNorm backwards of different d, as the decoder block folds its three:
    blockIdx.y = 0..3, a grid of dmax / 64 = 16 column blocks, so jobs 1, 2 and 4 must stop at their own d (the
    c < J.d guard; d = 200 ends inside a 64-column block), and z planes 1..2 that only job 3 (FiLM, 18 slabs per
    batch) may use. Jobs of 1, 17, 36 and 35 slabs: the 16-group loop goes round one, two and three times.
    Every destination starts non-zero inside a buffer of guard elements (16 before, 1040 > dmax after) that must
    keep their value; dgamma / dbeta / dfilm_* within 1e-4 of float64."""
    o = ops()
    jobs = [(128, 1, 32, False), (512, 1, 544, False), (1024, 2, 576, True), (200, 1, 1100, False)]
    lnp = o.LnPartials()
    held = []
    for d, B, L, film in jobs:
        c = ln_case(d, B, L, film, P_BWD)
        st = run_ln_fwd(c, True)
        bufs, views = [], []
        for b0 in ln_bases(d, B):
            buf = torch.full((16 + b0.numel() + 1040,), GUARD, device=dev)
            v = buf[16:16 + b0.numel()].view(b0.shape)
            v.copy_(b0)
            bufs.append(buf)
            views.append(v)
        dy = torch.empty(c.N, d, device=dev, dtype=bf)
        o.ln_bwd(X(c.dout), st.sv, st.mean, st.rstd, X(c.gm), X(c.bt), dres=torch.empty(c.N, d, device=dev), dy_t=dy,
                 dgamma=views[0], dbeta=views[1], film_scale=X(c.fs) if film else None,
                 dfilm=(views[2], views[3]) if film else None, rows_per_batch=L, drop_p=P_BWD, seed=SEED,
                 rng_stream=STREAM, partials=lnp)
        held.append((c, bufs, views))
    lnp.fold()
    torch.cuda.synchronize()
    for j, (c, bufs, views) in enumerate(held):
        base = ln_bases(c.d, c.B)
        refs = (c.dgm, c.dbt, c.dfs, c.dfh)
        for q, name in enumerate(("dgamma", "dbeta", "dfilm_scale", "dfilm_shift")):
            n = base[q].numel()
            buf = bufs[q].cpu()
            assert (buf[:16] == GUARD).all() and (buf[16 + n:] == GUARD).all(), f"job {j + 1} {name}: guard overwritten"
            got = views[q].cpu()
            if refs[q] is None:
                assert torch.equal(got, base[q]), f"job {j + 1} {name}: written without FiLM"
            else:
                close(got - base[q], refs[q], rtol=1e-4, what=f"job {j + 1} {name}")


# ------------------------------------------------------------------------------------------ L_fd
def lfd_std_ref(z, eps=EPS):
    z = z.double()
    m = z.mean(0, keepdim=True)
    inv = 1 / torch.sqrt(z.var(0, unbiased=False, keepdim=True) + eps)
    return (z - m) * inv, inv[0]


def lfd_std_bwd_ref(dzt, zt, inv_std):
    """dz = (dz~ - mean_b dz~ - z~ mean_b(dz~ z~)) inv_std in float64, on the z~ the kernel reads."""
    dzt, zt = dzt.double().cpu(), zt.double().cpu()
    m1 = dzt.mean(0, keepdim=True)
    m2 = (dzt * zt).mean(0, keepdim=True)
    return (dzt - m1 - zt * m2) * inv_std.double().cpu()


LFD_STD_SHAPES = [(5, 1000), (32, 257), (1, 300)]


@pytest.mark.parametrize("dt", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C", LFD_STD_SHAPES)
def test_lfd_std_fwd(B, C, dt):
    """lfd_std_fwd_kernel<float> and <bf16_t>: C = 1000 is four 256-thread blocks of which the last is trimmed by
    c >= C (the golden fixture's C = 512 is exactly two), C = 257 leaves one thread in its last block with B = 32
    rows to sum, B = 1 is the degenerate batch (z~ = 0, inv_std = 1 / sqrt(eps)). inv_std within 1e-5, z~ f32
    within 1e-5 of the maximum, z~ bf16 within 2^-8 |ref| + 1e-5."""
    z = torch.randn(B, C, generator=g(200)) + 0.25
    zt_ref, inv_ref = lfd_std_ref(z)
    zt, inv = ops().lfd_std_fwd(X(z), dt, EPS)
    close(inv, inv_ref, rtol=1e-5, what="inv_std")
    if B == 1:
        assert (zt == 0).all()
        close(inv, torch.full((C,), EPS ** -0.5, dtype=torch.float64), rtol=1e-5, what="inv_std B=1")
    if dt == f32:
        close(zt, zt_ref, rtol=1e-5, what="z~ f32")
    else:
        bf16_close(zt, zt_ref, 1e-5, "z~ bf16")


@pytest.mark.parametrize("dt", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C", LFD_STD_SHAPES)
def test_lfd_std_bwd(B, C, dt):
    """lfd_std_bwd_kernel<float> and <bf16_t> at the shapes of test_lfd_std_fwd (trimmed last block, one-thread
    last block, B = 1), reading the z~ and inv_std that lfd_std_fwd just wrote in that dtype; the float64 formula is
    evaluated on the same z~, so the bf16 rounding of z~ is an input, not an error. Within 1e-5 of the maximum."""
    o = ops()
    z = torch.randn(B, C, generator=g(200)) + 0.25
    dzt = torch.randn(B, C, generator=g(201))
    zt, inv = o.lfd_std_fwd(X(z), dt, EPS)
    dz = o.lfd_std_bwd(X(dzt), zt, inv)
    close(dz, lfd_std_bwd_ref(dzt, zt, inv), rtol=1e-5, what="dz")


@pytest.mark.parametrize("dt", [f32, bf], ids=["f32", "bf16"])
def test_lfd_two_ranks_on_one_device(dt):
    """The four data-parallel kernels (lfd_colstat_kernel both passes, lfd_std_apply_kernel<T>,
    lfd_bwd_colstat_kernel<T>, lfd_std_bwd_apply_kernel<T>) without a process group: the (6, 1000) batch split in
    two ranks of 3 rows, the all-reduces replaced by adding the two ranks' partial sums. C = 1000 trims the last
    block. Each rank's z~ equals its rows of the whole-batch lfd_std_fwd (f32: 1e-6 of the maximum; bf16: at most
    one bf16 ulp apart and > 99 % equal); the summed backward column sums match float64 within 1e-5; each rank's
    lfd_std_bwd_apply(inv_n = 1/6, scale = 2) equals twice its rows of the whole-batch lfd_std_bwd run on the same
    z~ (the two ranks' rows concatenated), within 1e-5."""
    o = ops()
    B, C, h = 6, 1000, 3
    z = X(torch.randn(B, C, generator=g(210)) + 0.25)
    dzt = X(torch.randn(B, C, generator=g(211)))
    halves = (z[:h], z[h:])
    s1 = sum(o.lfd_colstat(zh, torch.empty(C, device=dev)) for zh in halves)
    close(s1, z.double().sum(0), rtol=1e-5, what="colstat pass 1")
    s2 = sum(o.lfd_colstat(zh, torch.empty(C, device=dev), s1, 1.0 / B) for zh in halves)
    close(s2, ((z.double() - z.double().mean(0)) ** 2).sum(0), rtol=1e-5, what="colstat pass 2")
    zt_w, inv_w = o.lfd_std_fwd(z, dt, EPS)
    zts = []
    for k, zh in enumerate(halves):
        zt, inv = o.lfd_std_apply(zh, dt, s1, s2, 1.0 / B, EPS)
        ref = zt_w[k * h:(k + 1) * h]
        if dt == f32:
            close(zt, ref, rtol=1e-6, what=f"std_apply rank {k}")
        else:
            rel = (zt.float() - ref.float()).abs() / ref.float().abs().clamp_min(1e-30)
            assert (rel <= 2.0 ** -7).all(), f"std_apply rank {k}: max rel {rel.max().item():.2e}"
            assert (zt == ref).float().mean().item() > 0.99
        close(inv, inv_w, rtol=1e-5, what=f"std_apply inv_std rank {k}")
        zts.append(zt)
    zt_all = torch.cat(zts)
    sums = sum(o.lfd_bwd_colstat(dzt[k * h:(k + 1) * h], zts[k], torch.empty(2 * C, device=dev)) for k in range(2))
    ref_sums = torch.cat([dzt.double().sum(0), (dzt.double() * zt_all.double()).sum(0)])
    close(sums, ref_sums, rtol=1e-5, what="bwd_colstat")
    dz_w = o.lfd_std_bwd(dzt, zt_all, inv_w)
    close(dz_w, lfd_std_bwd_ref(dzt, zt_all, inv_w), rtol=1e-5, what="whole-batch std_bwd")
    for k in range(2):
        dz = o.lfd_std_bwd_apply(dzt[k * h:(k + 1) * h], zts[k], inv_w, sums, 1.0 / B, 2.0)
        close(dz, 2.0 * dz_w[k * h:(k + 1) * h], rtol=1e-5, what=f"std_bwd_apply rank {k}")


LAM = 5e-3
LFD_D = [pytest.param(32, False, id="D32"), pytest.param(33, False, id="D33-scalar-tail"),
         pytest.param(256, False, id="D256-strided"), pytest.param(1030, False, id="D1030-diagonal-loop"),
         pytest.param(256, True, id="D256-offset-4B")]


def lfd_cm(D, offset):
    """Cm = 0.1 randn with a diagonal of 0.7 + 0.1 randn, on the GPU; offset: a view 4 bytes into its buffer."""
    Cm = 0.1 * torch.randn(D, D, generator=g(220))
    Cm.diagonal().copy_(0.7 + 0.1 * torch.randn(D, generator=g(221)))
    if not offset:
        return Cm, Cm.to(dev)
    buf = torch.zeros(D * D + 1, device=dev)
    v = buf[1:1 + D * D].view(D, D)
    v.copy_(Cm)
    assert v.data_ptr() % 16 == 4
    return Cm, v


def lfd_loss_ref(Cm, lam):
    Cm = Cm.double()
    dg = Cm.diagonal()
    return ((1 - dg) ** 2).sum() + lam * ((Cm ** 2).sum() - (dg ** 2).sum())


@pytest.mark.parametrize("D,offset", LFD_D)
def test_lfd_loss_kernel(D, offset):
    """lfd_loss_kernel's loops: D = 32 (n4 = 256: a quarter of the 1024 threads load one float4), D = 33
    (n = 1089 = 4 * 272 + 1: the scalar tail of one element), D = 256 (n4 = 16384: the vector loop strides 16
    times), D = 1030 (the diagonal loop j += 1024 goes round twice for threads 0..5; n % 4 == 0), and D = 256 on a
    view 4 bytes into its buffer (the all-scalar branch, 64 rounds). Against the float64 formula at rtol 1e-5."""
    Cm, Cg = lfd_cm(D, offset)
    close(ops().lfd_loss(Cg, LAM), lfd_loss_ref(Cm, LAM), rtol=1e-5, what=f"lfd_loss D={D}")


@pytest.mark.parametrize("gscale", [None, 2.5])
@pytest.mark.parametrize("dt", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [32, 33, 256, 1030])
def test_lfd_dloss_kernel(D, dt, gscale):
    """lfd_dloss_kernel<float> and <bf16_t> with and without gscale: D = 33 and 1030 end inside a 256-thread block
    (e >= D * D trims; 32 and 256 fill theirs), and at an odd D the diagonal e = j (D + 1) falls on every lane
    residue, so a wrong j / k split of e shows. dC = g (-2 (1 - c) on the diagonal, 2 lam c off it): f32 within
    1e-6 of the maximum, bf16 within 2^-8 relative per element."""
    Cm, Cg = lfd_cm(D, False)
    gs = None if gscale is None else torch.tensor([gscale], device=dev)
    dC = ops().lfd_dloss(Cg, gs, LAM, dt)
    ref = 2 * LAM * Cm.double()
    ref.diagonal().copy_(-2 * (1 - Cm.double().diagonal()))
    ref = ref * (1.0 if gscale is None else gscale)
    if dt == f32:
        close(dC, ref, rtol=1e-6, atol=0.0, what="dC f32")
    else:
        bf16_close(dC, ref, 0.0, "dC bf16")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,D", [(6, 20, 72), (8, 12, 256)])
def test_lfd_loss_end_to_end(B, T, D, prec):
    """losses.fddm_losses.lfd_loss with (3 loss).backward() (the gscale path of lfd_dloss) past the golden
    fixture's (4, 16, 32): (6, 20, 72) has C = T D = 1440 (a trimmed last block) and D = 72 (no multiple of 64, the
    GEMM's ragged tiles), (8, 12, 256) is the production D. zb = 0.6 za + 0.8 randn keeps the diagonal of C near 0.6.
    fp32: loss within 1e-5, gradients within 1e-4 of O.lfd_loss on float64 inputs; bf16 (z~ and dC in bf16): loss and
    gradients within TOL[bf16] = 2e-2 of the maximum (rounding z~ alone costs 1.3e-4 / 2.5e-3 in a CPU emulation)."""
    from fddm_hip import runtime as rt
    from losses.fddm_losses import lfd_loss
    za = torch.randn(B, T, D, generator=g(230))
    zb = 0.6 * za + 0.8 * torch.randn(B, T, D, generator=g(231))
    ar, br = za.double().requires_grad_(True), zb.double().requires_grad_(True)
    ref = O.lfd_loss(ar, br, LAM)
    (3 * ref).backward()
    with rt.use_precision(prec):
        a = za.to(dev).requires_grad_(True)
        b = zb.to(dev).requires_grad_(True)
        loss = lfd_loss(a, b, LAM)
        (3 * loss).backward()
    lt, gt = (1e-5, 1e-4) if prec == "fp32" else (TOL[bf], TOL[bf])
    close(loss, ref.detach(), rtol=lt, what=f"lfd loss {prec}")
    close(a.grad, ar.grad, rtol=gt, what=f"dza {prec}")
    close(b.grad, br.grad, rtol=gt, what=f"dzb {prec}")
