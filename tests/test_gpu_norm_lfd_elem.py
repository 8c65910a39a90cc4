"""The LayerNorm / FiLM kernels (ln_fwd_kernel, ln_bwd_fused_kernel, ln_bwd_kernel, ln_bwd_params_kernel, ln_fold_kernel:
csrc/norm.hip) and the L_fd kernels (csrc/lfd.hip) per element against float64. They run three times per decoder block
forward and backward, at every WavLM layer and on every L_fd step.

Cases (helpers.ln_fwd_cases(), ln_bwd_cases(), LFD_BC, LFD_D x LFD_LAM; tests/test_cpu_norm_lfd_ref.py asserts that they
reach every build ops.ln_fwd / ops.ln_bwd can launch): the four dtype triples x y / no y x FiLM / no FiLM x one / two
chunks per lane and both RoPE builds; d = 8 (63 idle lanes), 200, 512, 520 (a second chunk of one lane), 1024; N = 1, 5,
33, 70, 1100; FiLM batches of L = 1, 20, 32, 37, 576 rows; save_s in place over x; p = 0.1, 0.5, 2^-16 (threshold 1), 1e-6
(threshold 0: nothing dropped, nothing scaled) and 0. The backward in its fused form (with and without
LnPartials + fold, with and without FiLM, f32 and bf16 dy_t, ragged last slabs, 35 slabs, 18 slabs per FiLM batch), in its
two-pass form (d = 100, d = 1, FiLM batches that are no whole slabs, dres 4 bytes into its buffer, with and without
parameter gradients), and four LayerNorms folded by one launch. The backward reads s, mean, rstd made on the CPU: its
reference is the kernel's formula on those stored values. L_fd at B = 1, 2, 3, 32, 33, C = 1, 257, 1000, f32 and bf16 z~;
lfd_loss / lfd_dloss at D = 1, 33, 256, 1030 and a view 4 bytes into its buffer, lam = 0 and 5e-3.

Inputs: randn times a power of two per row and per column (2^-2 .. 2^2); rows with a common offset of 64 standard
deviations, one channel 2^8 above the rest, constant, all-zero and 2^-20-sized rows; gamma with zeros and negative entries;
FiLM scales of exactly -1 and of size 4; y nowhere zero; L_fd columns with an offset of 2^6 spreads and constant columns;
Cm with diagonal entries of exactly 1 and off-diagonals across 2^-8 .. 2^2.

Every kernel output is a slice of a NaN-filled buffer whose other elements must keep their bits (lfd_loss's scalar and
the outputs the lfd_std wrappers allocate are written through ops.call into such buffers as well).

Bounds, per element, u = 2^-24 (helpers.ln_fwd_ref64, ln_bwd_ref64, lfd_std_ref64, lfd_colstat_ref64, lfd_bwd_ref64,
lfd_loss_ref64, lfd_dloss_ref64), v = x + y keep / (1 - p), t = y keep / (1 - p):
    save_s              u (3 |t| + |v|) = sv; u |v| without dropout; the bits of x without y       (derived)
    mean                C_mean u M,  M = mean_j (|v_j| + sv_j)
    rstd                C_rstd u rstd (1 + rstd^2 mean_j (|v_j - m| sv_j))
    out                 C_out u (|gamma| (rstd (|v - m| + M + sv) + |v - m| u_rstd) + |beta|), through FiLM times |1 + fs|
                        plus |fh|; bf16 out_t: plus the exact half ulp, and the bits of out_f32.to(bfloat16)
    rope_out            the out bound through |cos|, |sin| plus rope_fwd's 2 u (|o1 c| + |o2 s'|), then the half ulp
    dres                C_dres u rstd (|gx| + mean |gx| + |xh| mean |gx xh|)
    dy_t                that times 1 / (1 - p) plus 3 u |dy| on kept elements, exactly 0 on dropped ones; bf16: the half ulp
    dgamma, dbeta       C_par u (|old| + sum_r |g'| |xh|), C_par u (|old| + sum_r |g'|)
    dfilm scale, shift  C_par u (|old| + sum_{r in b} |dout| (|xh gamma| + |beta|)), C_par u (|old| + sum |dout|)
    inv_std             C_is u inv_std
    z~                  C_zt u is (|z - m| + mean_b |z|)   (std_apply: |m| for the mean), bf16: the half ulp
    lfd_colstat         C_col u sum |z|;  C_col u sum |t| (|t| + |m|), t = z - m
    lfd_bwd_colstat     C_col u sum |g|, C_col u sum |g z~|
    dz                  C_dz u W is (|g| + mean |g| + |z~| mean |g z~|)
    lfd_loss            C_loss u (lam sum C^2 + sum_j |(1 - c)^2 - lam c^2|)
    lfd_dloss           3 u |dC|, bf16: the half ulp                                                (derived)
C = 8 E, E measured on the CPU (tests/test_cpu_norm_lfd_ref.py, which also proves that the listed mutants leave these
bounds on at least half of the elements they change):
    C_mean 22.4  C_rstd 27.6  C_out 22.4  C_dres 30.8  C_par 30.8  C_is 30.4  C_zt 35.2  C_col 49.2  C_dz 25.6  C_loss 12.4

Measured on an MI355X (the NORMNEED lines this file prints): "units" is the largest |out - ref| over the family's unit
(the C it needed), "share" the largest share of its bound any element used. A correctly rounded bf16 output (and save_s,
whose bound is its own roundings) next to a rounding boundary uses its whole bound.
    path                                  units                       share of bound
    ln_fwd CH 1  mean / rstd / out        2.51 / 2.24 / 2.31          0.112 / 0.081 / 0.103
    ln_fwd CH 2  mean / rstd / out        2.66 / 3.25 / 2.21          0.119 / 0.118 / 0.099
    save_s, bf16 out_t, rope_out          -                           1.000, 1.000, 0.999
    dres  fused CH 1 / CH 2 / rows        3.64 / 3.49 / 3.12          0.118 / 0.113 / 0.101
    dy_t  f32 / bf16                      -                           0.106 / 0.999
    atomics  dgamma / dbeta / dfs / dfh   1.97 / 1.17 / 1.87 / 1.86   0.064 / 0.038 / 0.061 / 0.060   (order-dependent)
    fold     dgamma / dbeta / dfs / dfh   3.03 / 2.18 / 2.38 / 1.56   0.098 / 0.071 / 0.077 / 0.051   (1 and 4 jobs)
    params   dgamma / dbeta / dfs / dfh   3.64 / 2.73 / 2.50 / 2.34   0.118 / 0.089 / 0.081 / 0.076
    lfd inv_std  fwd / apply              3.77 / 1.69                 0.124 / 0.055
    lfd z~       fwd / apply              4.15 / 2.81                 0.118 / 0.080                   (bf16: 0.999)
    lfd colstat 1 / 2 / bwd_colstat       4.08 / 5.05 / 2.94          0.083 / 0.103 / 0.060
    lfd dz / dz apply                     2.95 / 3.02                 0.115 / 0.118
    lfd_loss, lfd_dloss f32               1.47, 1.79 (of 3)           0.119, 0.595                    (dloss bf16: 1.000)
No kernel left its bound. The one disagreement, the scale 1 / (1 - p) at a threshold of 0, was between the oracle and
every kernel with an `if (thr16)` guard; the oracle now follows the kernels, and the p = 1e-6 cases hold it.
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
DT = {"f32": F32, "bf16": BF}
NEED = {}          # row -> [units, share]
assert all(v <= 64.0 for v in H.NORM_C.values())


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    for k in sorted(NEED):
        units = f"{NEED[k][0]:6.2f}" if NEED[k][0] >= 0 else "     -"
        print(f"\nNORMNEED {k:<22} units {units}  share {NEED[k][1]:5.3f}", end="")
    print()


def _ops():
    from fddm_hip import ops
    return ops


def X(t):
    return t.to(dev).contiguous() if t is not None else None


def _check(row, what, out, ref, bound, unit=None):
    """Every element of out (any device) within bound of ref (CPU float64); a bound of 0 asks for the reference's bits.
    Records the row's largest share of the bound and, with unit (the per-element u s), the C it needed."""
    out = out.detach().cpu()
    ref, bound = ref.reshape(out.shape), bound.reshape(out.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out.double() - ref).abs()
    rel = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    share = rel.max().item() if rel.numel() else 0.0
    units = -1.0
    if unit is not None:
        unit = unit.reshape(out.shape)
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


# ------------------------------------------------------------------------------------------ LayerNorm forward
FWD = H.ln_fwd_cases()


@pytest.mark.parametrize("i", range(len(FWD)), ids=[c["id"] for c in FWD])
def test_ln_fwd(i):
    c = FWD[i]
    o = _ops()
    x, y, gamma, beta, film, keep, rope, kind = H.ln_fwd_operands(i)
    N, d, L, p = c["N"], c["d"], c["L"], c["p"]
    r = H.ln_fwd_ref64(x, y, gamma, beta, film, L, p, keep, rope=rope, rope_L=c["rope"])
    g = _Guards()
    xd = g.new((N, d), DT[c["tr"][0]], init=x.to(dev)) if c["alias"] else X(x)
    save_s = xd if c["alias"] else g.new((N, d))
    out_f32, out_t = g.new((N, d)), g.new((N, d), DT[c["tr"][2]])
    mean, rstd = g.new((N,)), g.new((N,))
    ro = g.new((N, d), BF) if rope else None
    o.ln_fwd(xd, X(y), X(gamma), X(beta), out_f32=out_f32, out_t=out_t, save_s=save_s, mean=mean, rstd=rstd,
             film=(X(film[0]), X(film[1])) if film else None, rows_per_batch=L, eps=H.LN_EPS, drop_p=p, seed=H.LN_SEED,
             rng_stream=H.LN_STREAM, rope=(X(rope[0]), X(rope[1]), ro, c["rope"]) if rope else None)
    what = f"ln_fwd {c['id']}"
    g.check(what)
    fam = "ln_fwd" + ("2" if d > 512 else "1")
    _check(f"{fam} save_s", what + " save_s", save_s, r.s, r.b_s)
    _check(f"{fam} mean", what + " mean", mean, r.mean, r.b_mean, H.U24 * r.u_mean)
    _check(f"{fam} rstd", what + " rstd", rstd, r.rstd, r.b_rstd, H.U24 * r.u_rstd)
    _check(f"{fam} out", what + " out_f32", out_f32, r.out, r.b_out, H.U24 * r.u_out)
    if c["tr"][2] == "bf16":
        _check(f"{fam} out bf16", what + " out_t", out_t, r.out, r.b_out_bf)
        assert torch.equal(_bits(out_t), _bits(out_f32.to(BF))), what + ": out_t is not out_f32 rounded to bf16"
    else:
        assert torch.equal(_bits(out_t), _bits(out_f32)), what + ": out_t differs from out_f32"
    if rope:
        _check(f"{fam} rope", what + " rope_out", ro, r.rope, r.b_rope)
    if y is not None and H.ln_thr(p):
        # the mask, exactly: a dropped element is x's bits, a kept one is not (y is nowhere zero); the const and zero
        # rows carry a 2^-30-sized y, which the fp32 sum absorbs
        loud = ((kind != 3) & (kind != 4))[:, None].expand(N, d)
        moved = save_s.cpu() != x.float()
        assert torch.equal(moved[loud], keep[loud]), what + ": the dropout mask differs from the oracle's"
        assert not moved[~keep].any()


def test_ln_fwd_optional_outputs():
    """Each output alone gives the bits of the full call (case 0: f32 + bf16 -> bf16 with FiLM)."""
    o = _ops()
    c = FWD[0]
    x, y, gamma, beta, film, keep, rope, kind = H.ln_fwd_operands(0)
    N, d = c["N"], c["d"]
    args = (X(x), X(y), X(gamma), X(beta))
    kw = dict(film=(X(film[0]), X(film[1])) if film else None, rows_per_batch=c["L"], drop_p=c["p"], seed=H.LN_SEED,
              rng_stream=H.LN_STREAM)
    shapes = dict(out_f32=((N, d), F32), out_t=((N, d), BF), save_s=((N, d), F32), mean=((N,), F32), rstd=((N,), F32))
    g = _Guards()
    full = {k: g.new(*v) for k, v in shapes.items()}
    o.ln_fwd(*args, **full, **kw)
    for k, v in shapes.items():
        one = g.new(*v)
        o.ln_fwd(*args, **{k: one}, **kw)
        g.check(f"ln_fwd with {k} alone")
        assert torch.equal(_bits(one), _bits(full[k])), k


# ------------------------------------------------------------------------------------------ LayerNorm backward
BWD = H.ln_bwd_cases()


def _ln_bwd_launch(o, c, i, g, lnp):
    dout, s, mean, rstd, gamma, beta, fs, keep, old, kind = H.ln_bwd_operands(i)
    N, d, L = c["N"], c["d"], c["L"]
    dres = g.new((N, d), lead=1 if c["off4"] else 0)
    assert (dres.data_ptr() % 16 == 4) == c["off4"]
    dy = g.new((N, d), DT[c["dt"]])
    dst = [g.new(t.shape, init=t.to(dev)) if t is not None else None for t in old]
    par = c["params"]
    o.ln_bwd(X(dout), X(s), X(mean), X(rstd), X(gamma), X(beta), dres=dres, dy_t=dy, dgamma=dst[0] if par else None,
             dbeta=dst[1] if par else None, film_scale=X(fs), dfilm=(dst[2], dst[3]) if (par and L) else None,
             rows_per_batch=L, drop_p=c["p"], seed=H.LN_SEED, rng_stream=H.LN_STREAM, partials=lnp)
    return dres, dy, dst


def _ln_bwd_check(c, i, dres, dy, dst, tag=""):
    dout, s, mean, rstd, gamma, beta, fs, keep, old, kind = H.ln_bwd_operands(i)
    r = H.ln_bwd_ref64(dout, s, mean, rstd, gamma, beta, fs, c["L"], c["p"], keep, old)
    kern = H.ln_bwd_build(c)
    fam = ("ln_bwd fused" + str(kern[0][1]) if kern[0] != "rows" else "ln_bwd rows") + tag
    what = f"ln_bwd {c['id']}{tag}"
    _check(f"{fam} dres", what + " dres", dres, r.dres, r.b_dres, H.U24 * r.u_dres)
    _check(f"{fam} dy {c['dt']}", what + " dy_t", dy, r.dy, r.b_dy[c["dt"]])
    sure = keep & (r.dy.abs() > 2.0 * r.b_dy[c["dt"]])
    got = dy.cpu() != 0
    assert got[sure].all() and not got[~keep].any(), what + ": the dropout mask differs from the oracle's"
    pfam = ("fold" if c["part"] else "atomics") if kern[0] != "rows" else "params"
    for k, name in enumerate(("dgamma", "dbeta", "dfs", "dfh")):
        if dst[k] is None:
            continue
        if c["params"]:
            _check(f"ln_bwd {pfam}{tag} {name}", what + " " + name, dst[k], getattr(r, name), getattr(r, "b_" + name),
                   H.U24 * getattr(r, "u_" + name))
        else:
            assert torch.equal(_bits(dst[k]), _bits(old[k].to(dev))), what + f": {name} written without being asked for"


@pytest.mark.parametrize("i", range(len(BWD)), ids=[c["id"] for c in BWD])
def test_ln_bwd(i):
    c = BWD[i]
    o = _ops()
    g = _Guards()
    lnp = o.LnPartials() if c["part"] else None
    dres, dy, dst = _ln_bwd_launch(o, c, i, g, lnp)
    if lnp is not None:
        lnp.fold()                       # ln_fold_kernel with one job
    g.check(f"ln_bwd {c['id']}")
    _ln_bwd_check(c, i, dres, dy, dst)


def test_ln_fold_four_jobs():
    """Four LayerNorm backwards into one LnPartials, one ln_fold launch: d = 8, 200, 520, 1024-class jobs of different
    slab counts, one with FiLM (z planes that only it may use), every destination guarded."""
    o = _ops()
    part = [i for i, c in enumerate(BWD) if c["part"]]
    film = [i for i in part if BWD[i]["L"]]
    pick = [max(part, key=lambda i: BWD[i]["N"] * (BWD[i]["L"] == 0)), max(film, key=lambda i: BWD[i]["L"]),
            max(part, key=lambda i: BWD[i]["d"]), min(part, key=lambda i: BWD[i]["d"] * 10000 + BWD[i]["N"])]
    assert len(set(pick)) == 4 and len({BWD[i]["d"] for i in pick}) >= 3
    g = _Guards()
    lnp = o.LnPartials()
    held = [(i, _ln_bwd_launch(o, BWD[i], i, g, lnp)) for i in pick]
    lnp.fold()
    g.check("ln_fold with four jobs")
    for i, (dres, dy, dst) in held:
        _ln_bwd_check(BWD[i], i, dres, dy, dst, tag=" x4")


# ------------------------------------------------------------------------------------------ L_fd
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,C", H.LFD_BC, ids=[f"B{b}-C{c}" for b, c in H.LFD_BC])
def test_lfd_standardisation(B, C, dt):
    o = _ops()
    z, dzt, zt, inv, s1, s2, sums = H.lfd_operands(B, C)
    inv_n = 1.0 / (H.LFD_RANKS * B)
    what = f"lfd B={B} C={C} {dt}"
    g = _Guards()
    zd, dztd, s1d, s2d, sumsd, invd = X(z), X(dzt), X(s1), X(s2), X(sums), X(inv)
    ztq = zt.to(DT[dt])
    ztd = X(ztq)
    st, cd = o.stream(), o.code
    # forward
    f = H.lfd_std_ref64(z)
    zt_o, is_o = g.new((B, C), DT[dt]), g.new((C,))
    o.call("fddm_lfd_std_fwd", cd(zt_o), o.ptr(zd), o.ptr(zt_o), o.ptr(is_o), B, C, float(H.LN_EPS), st)
    a = H.lfd_std_ref64(z, s1=s1, s2=s2, inv_n=inv_n)
    zt_a, is_a = g.new((B, C), DT[dt]), g.new((C,))
    o.call("fddm_lfd_std_apply", cd(zt_a), o.ptr(zd), o.ptr(zt_a), o.ptr(is_a), o.ptr(s1d), o.ptr(s2d), float(inv_n),
           float(H.LN_EPS), B, C, st)
    c1, c2 = g.new((C,)), g.new((C,))
    o.lfd_colstat(zd, c1)
    o.lfd_colstat(zd, c2, s1d, inv_n)
    # backward, on the stored z~ and inv_std
    w = H.lfd_bwd_ref64(dzt, ztq.float(), inv)
    wa = H.lfd_bwd_ref64(dzt, ztq.float(), inv, sums=sums, inv_n=inv_n, scale=H.LFD_W)
    dz, dza, cs = g.new((B, C)), g.new((B, C)), g.new((2 * C,))
    o.call("fddm_lfd_std_bwd", cd(ztd), o.ptr(dztd), o.ptr(ztd), o.ptr(invd), o.ptr(dz), B, C, st)
    o.call("fddm_lfd_std_bwd_apply", cd(ztd), o.ptr(dztd), o.ptr(ztd), o.ptr(invd), o.ptr(sumsd), float(inv_n),
           float(H.LFD_W), o.ptr(dza), B, C, st)
    o.lfd_bwd_colstat(dztd, ztd, cs)
    g.check(what)
    r1, r2 = H.lfd_colstat_ref64(z), H.lfd_colstat_ref64(z, s1, inv_n)
    _check("lfd inv_std", what + " inv_std", is_o, f.inv, f.b_inv, H.U24 * f.inv)
    _check("lfd inv_std apply", what + " inv_std (apply)", is_a, a.inv, a.b_inv, H.U24 * a.inv)
    if dt == "f32":
        _check("lfd z~", what + " z~", zt_o, f.zt, f.b_zt, H.U24 * f.u_zt)
        _check("lfd z~ apply", what + " z~ (apply)", zt_a, a.zt, a.b_zt, H.U24 * a.u_zt)
    else:
        _check("lfd z~ bf16", what + " z~", zt_o, f.zt, f.b_zt_bf)
        _check("lfd z~ apply bf16", what + " z~ (apply)", zt_a, a.zt, a.b_zt_bf)
    _check("lfd colstat 1", what + " colstat pass 1", c1, r1.out, r1.b, H.U24 * r1.u)
    _check("lfd colstat 2", what + " colstat pass 2", c2, r2.out, r2.b, H.U24 * r2.u)
    _check("lfd bwd_colstat", what + " bwd_colstat", cs, w.cs, w.b_cs, H.U24 * w.u_cs)
    _check("lfd dz", what + " dz", dz, w.dz, w.b_dz, H.U24 * w.u_dz)
    _check("lfd dz apply", what + " dz (apply)", dza, wa.dz, wa.b_dz, H.U24 * wa.u_dz)
    # the wrappers allocate their outputs: the same bits
    zt_w, is_w = o.lfd_std_fwd(zd, DT[dt], H.LN_EPS)
    assert torch.equal(_bits(zt_w), _bits(zt_o)) and torch.equal(_bits(is_w), _bits(is_o))
    zt_w, is_w = o.lfd_std_apply(zd, DT[dt], s1d, s2d, inv_n, H.LN_EPS)
    assert torch.equal(_bits(zt_w), _bits(zt_a)) and torch.equal(_bits(is_w), _bits(is_a))
    assert torch.equal(_bits(o.lfd_std_bwd(dztd, ztd, invd)), _bits(dz))
    assert torch.equal(_bits(o.lfd_std_bwd_apply(dztd, ztd, invd, sumsd, inv_n, H.LFD_W)), _bits(dza))


@pytest.mark.parametrize("lam", H.LFD_LAM)
@pytest.mark.parametrize("D,off", H.LFD_D, ids=[f"D{d}{'-off4' if f else ''}" for d, f in H.LFD_D])
def test_lfd_loss_and_dloss(D, off, lam):
    o = _ops()
    Cm = H.lfd_cm(D)
    buf = torch.full((D * D + 4,), float("nan"), device=dev)
    Cd = buf[1:1 + D * D].view(D, D) if off else buf[:D * D].view(D, D)
    Cd.copy_(Cm)
    assert (Cd.data_ptr() % 16 == 4) == off
    what = f"lfd_loss D={D} off={off} lam={lam}"
    g = _Guards()
    loss = g.new((1,))
    o.call("fddm_lfd_loss", o.ptr(Cd), o.ptr(loss), D, float(lam), o.stream())
    r = H.lfd_loss_ref64(Cm, lam)
    gs = torch.tensor([0.625], device=dev)
    outs = {dt: g.new((D, D), DT[dt]) for dt in ("f32", "bf16")}
    for dt, dC in outs.items():
        o.call("fddm_lfd_dloss", o.code(dC), o.ptr(Cd), o.ptr(gs), o.ptr(dC), D, float(lam), o.stream())
    g.check(what)
    _check("lfd loss", what, loss, r.loss.reshape(1), r.b.reshape(1), H.U24 * r.u.reshape(1))
    d0 = H.lfd_dloss_ref64(Cm, 0.625, lam)
    _check("lfd dloss f32", what + " dC f32", outs["f32"], d0.dC, d0.b, H.U24 * d0.dC.abs())
    _check("lfd dloss bf16", what + " dC bf16", outs["bf16"], d0.dC, d0.b_bf)
    assert torch.equal(_bits(o.lfd_loss(Cd, lam).reshape(1)), _bits(loss))
    assert torch.equal(_bits(o.lfd_dloss(Cd, gs, lam, BF)), _bits(outs["bf16"]))
    d1 = H.lfd_dloss_ref64(Cm, 1.0, lam)
    _check("lfd dloss f32", what + " dC, no gscale", o.lfd_dloss(Cd, None, lam, F32), d1.dC, d1.b, H.U24 * d1.dC.abs())


# ------------------------------------------------------------------------------------------ refused arguments
def _refused(fn, bad):
    """Every (message, args, kwargs) row raises the ValueError of the precondition it names, before any launch."""
    for msg, a, kw in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            fn(*a, **kw)


def test_ln_arguments_are_checked():
    o = _ops()
    N, d, B = 6, 16, 2
    e = lambda *s, dt=F32: torch.zeros(*s, device=dev, dtype=dt)      # noqa: E731
    x, y, gm, bt = e(N, d), e(N, d, dt=BF), e(d), e(d)
    fs = (e(B, d), e(B, d))
    _refused(o.ln_fwd, [
        ("x is contiguous [N, d]", (e(N, 2 * d)[:, :d], y, gm, bt), {}),
        ("x is contiguous [N, d]", (e(N, d, dt=torch.float16), y, gm, bt), {}),
        ("x is contiguous [N, d]", (e(N, d).cpu(), y, gm, bt), {}),
        ("d is a multiple of 8", (e(N, 12), e(N, 12, dt=BF), e(12), e(12)), {}),
        ("d is a multiple of 8", (e(N, 0), None, e(0), e(0)), {}),
        ("d is a multiple of 8", (e(1, 1032), None, e(1032), e(1032)), {}),
        ("ln_fwd: y is contiguous [N, d]", (x, e(N + 1, d, dt=BF), gm, bt), {}),
        ("ln_fwd: gamma is contiguous float32 with 16 elements", (x, y, e(d + 8), bt), {}),
        ("ln_fwd: beta is contiguous float32 with 16 elements", (x, y, gm, e(d, dt=BF)), {}),
        ("ln_fwd: film is a pair", (x, y, gm, bt), dict(film=(fs[0], e(B, d + 8)), rows_per_batch=3)),
        ("N == B * rows_per_batch for film", (x, y, gm, bt), dict(film=fs, rows_per_batch=4)),
        ("N == B * rows_per_batch for film", (x, y, gm, bt), dict(film=fs)),
        ("ln_fwd: out_f32 is contiguous [N, d], float32", (x, y, gm, bt), dict(out_f32=e(N, d, dt=BF))),
        ("ln_fwd: save_s is contiguous [N, d]", (x, y, gm, bt), dict(save_s=e(N - 1, d))),
        ("ln_fwd: out_t is contiguous [N, d]", (x, y, gm, bt), dict(out_t=e(N, d, dt=torch.float16))),
        ("ln_fwd: mean is contiguous float32 with 6 elements", (x, y, gm, bt), dict(mean=e(N - 1))),
        ("ln_fwd: rstd is contiguous float32 with 6 elements", (x, y, gm, bt), dict(rstd=e(N, dt=BF))),
        ("no build for these dtypes", (x, y, gm, bt), dict(out_t=e(N, d))),
        ("no build for these dtypes", (e(N, d, dt=BF), None, gm, bt), dict(out_t=e(N, d))),
        ("rope needs", (x, e(N, d), gm, bt), dict(out_t=e(N, d), rope=(e(3, d), e(3, d), e(N, d, dt=BF), 3))),
        ("rope cos and sin", (x, y, gm, bt), dict(out_t=e(N, d, dt=BF), rope=(e(2, d), e(3, d), e(N, d, dt=BF), 3))),
    ])
    dout, s, mean, rstd = e(N, d), e(N, d), e(N), e(N)
    dg, db = e(d), e(d)
    _refused(o.ln_bwd, [
        ("dout is contiguous float32 [N, d]", (e(N, d, dt=BF), s, mean, rstd, gm, bt), {}),
        ("d is in [1, 1024]", (e(N, 0), e(N, 0), mean, rstd, e(0), e(0)), {}),
        ("d is in [1, 1024]", (e(1, 1025), e(1, 1025), e(1), e(1), e(1025), e(1025)), {}),
        ("ln_bwd: s is contiguous [N, d]", (dout, e(N, d + 1), mean, rstd, gm, bt), {}),
        ("ln_bwd: mean is contiguous float32 with 6 elements", (dout, s, e(N + 1), rstd, gm, bt), {}),
        ("ln_bwd: gamma is contiguous float32 with 16 elements", (dout, s, mean, rstd, e(d - 1), bt), {}),
        ("ln_bwd: dres is contiguous [N, d]", (dout, s, mean, rstd, gm, bt), dict(dres=e(N, d, dt=BF))),
        ("ln_bwd: dy_t is contiguous [N, d]", (dout, s, mean, rstd, gm, bt), dict(dy_t=e(N, 2 * d)[:, :d])),
        ("dgamma and dbeta come as a pair", (dout, s, mean, rstd, gm, bt), dict(dgamma=dg)),
        ("parameter gradients need beta", (dout, s, mean, rstd, gm, None), dict(dgamma=dg, dbeta=db)),
        ("dfilm needs film_scale", (dout, s, mean, rstd, gm, bt), dict(dfilm=fs, rows_per_batch=3)),
        ("N == B * rows_per_batch for film_scale", (dout, s, mean, rstd, gm, bt), dict(film_scale=fs[0], rows_per_batch=4)),
        ("parameter gradients need dfilm", (dout, s, mean, rstd, gm, bt),
         dict(film_scale=fs[0], rows_per_batch=3, dgamma=dg, dbeta=db)),
        ("ln_bwd: dfilm is a pair", (dout, s, mean, rstd, gm, bt),
         dict(film_scale=fs[0], rows_per_batch=3, dfilm=(fs[0], e(B, d, dt=BF)))),
        ("ln_bwd partials need dgamma and dbeta", (dout, s, mean, rstd, gm, bt), dict(partials=o.LnPartials())),
    ])
    _refused(o.LnPartials().add, [
        ("N > 0 and d in [1, 1024]", (0, d, dg, db), {}),
        ("LnPartials.add: dgamma is contiguous float32 with 16 elements", (N, d, e(d + 1), db), {}),
        ("N == B * rows_per_batch for dfilm", (N, d, dg, db, fs, 4), {}),
    ])
    # the C entry points: d <= 0, and outputs the vector stores cannot take (returned before any launch)
    buf = e(N * d + 4)
    off = buf[1:1 + N * d].view(N, d)

    def fwd(dd=d, **kw):
        a = dict(out_f32=None, out_t=None, save_s=None, mean=None, rstd=None)
        a.update(kw)
        o.call("fddm_ln_fwd", o.F32, o.F32, o.F32, o.ptr(x), None, o.ptr(gm), o.ptr(bt), None, None, o.ptr(a["out_f32"]),
               o.ptr(a["out_t"]), o.ptr(a["save_s"]), o.ptr(a["mean"]), o.ptr(a["rstd"]), N, dd, 0, 1e-5, 0.0, 0, 0, None,
               None, None, 0, o.stream())
    for kw in (dict(dd=0), dict(dd=-8), dict(out_f32=off), dict(out_t=off), dict(save_s=off)):
        with pytest.raises(RuntimeError, match="fddm_ln_fwd failed"):
            fwd(**kw)
    with pytest.raises(RuntimeError, match="fddm_ln_bwd failed"):
        o.call("fddm_ln_bwd", o.F32, o.ptr(dout), o.ptr(s), o.ptr(mean), o.ptr(rstd), o.ptr(gm), o.ptr(bt), None,
               o.ptr(e(N, d)), None, None, None, None, None, N, 0, 0, 0.0, 0, 0, None, o.stream())
    torch.cuda.synchronize()


def test_lfd_arguments_are_checked():
    o = _ops()
    B, C, D = 3, 40, 8
    e = lambda *s, dt=F32: torch.zeros(*s, device=dev, dtype=dt)      # noqa: E731
    z, zt, inv = e(B, C), e(B, C, dt=BF), e(C)
    _refused(o.lfd_std_fwd, [("the input is contiguous float32 [B, C]", (e(B, C, dt=BF), F32), {}),
                             ("the input is contiguous float32 [B, C]", (e(B, 2 * C)[:, :C], F32), {}),
                             ("lfd_std_fwd: B > 0", (e(0, C), F32), {}),
                             ("the output dtype is float32 or bfloat16", (z, torch.float16), {})])
    _refused(o.lfd_std_bwd, [("z~ is contiguous [B, C]", (z, e(B, C + 1), inv), {}),
                             ("z~ is contiguous [B, C]", (z, e(B, C, dt=torch.float16), inv), {}),
                             ("inv_std is contiguous float32 with 40 elements", (z, zt, e(C - 1)), {})])
    _refused(o.lfd_colstat, [("out is contiguous float32 with 40 elements", (z, e(C + 1)), {}),
                             ("mean_sum is contiguous float32 with 40 elements", (z, e(C), e(C, dt=BF), 0.5), {}),
                             ("the input is contiguous float32 [B, C]", (z.cpu(), e(C)), {})])
    _refused(o.lfd_std_apply, [("s1 is contiguous float32 with 40 elements", (z, F32, e(2 * C), e(C), 0.5), {}),
                               ("s2 is contiguous float32 with 40 elements", (z, F32, e(C), e(2 * C)[::2], 0.5), {}),
                               ("the output dtype", (z, torch.int32, e(C), e(C), 0.5), {})])
    _refused(o.lfd_bwd_colstat, [("out is contiguous float32 with 80 elements", (z, zt, e(C)), {}),
                                 ("z~ is contiguous [B, C]", (z, e(B - 1, C), e(2 * C)), {})])
    _refused(o.lfd_std_bwd_apply, [("sums is contiguous float32 with 80 elements", (z, zt, inv, e(C), 0.5), {}),
                                   ("inv_std is contiguous float32 with 40 elements", (z, zt, e(C, dt=BF), e(2 * C), 0.5), {})])
    _refused(o.lfd_loss, [("Cm is contiguous float32 [D, D]", (e(D, D + 1), 0.1), {}),
                          ("Cm is contiguous float32 [D, D]", (e(D, D, dt=BF), 0.1), {}),
                          ("Cm is contiguous float32 [D, D]", (e(0, 0), 0.1), {})])
    _refused(o.lfd_dloss, [("Cm is contiguous float32 [D, D]", (e(D, 2 * D)[:, :D], None, 0.1, F32), {}),
                           ("gscale is contiguous float32 with 1 elements", (e(D, D), e(2), 0.1, F32), {}),
                           ("the output dtype", (e(D, D), None, 0.1, torch.float16), {})])
    torch.cuda.synchronize()
