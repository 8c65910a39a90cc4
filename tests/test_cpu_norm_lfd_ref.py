"""What tests/test_gpu_norm_lfd_elem.py may ask of the LayerNorm / FiLM kernels (csrc/norm.hip) and of the L_fd kernels
(csrc/lfd.hip), settled from the reference alone before any kernel runs.

E: each kernel's arithmetic emulated on the CPU in fp32 in its own order (helpers.ln_fwd_emulate, ln_bwd_emulate,
lfd_emulate, lfd_loss_emulate: 8 elements per lane and chunk, wave_sum_v's tree, the slab's 8-wave / 4-wave combine, the
fold's 16 groups or one atomic per slab, the two-pass form's 64-row chunks, lfd.hip's column loops and lfd_loss's two
accumulators per thread) against float64, in units of u = 2^-24 times the per-element scale of helpers.ln_fwd_ref64,
ln_bwd_ref64, lfd_*_ref64, the maximum over every case of helpers.ln_fwd_cases(), ln_bwd_cases(), LFD_BC, LFD_D x
LFD_LAM. The kernels are allowed NORM_C = 8 E units, hard cap 64. The stored E obey measured <= stored <= 1.1 measured
+ 0.05 (this file prints the measured ones as NORMREF lines).
Derived, not measured: save_s within u (3 |t| + |v|), t = y keep / (1 - p) (the roundings of 1 - p, of the quotient, of
the product and of the add; the FMA form has one fewer), u |v| without dropout, the bits of x without y; lfd_dloss
within 3 u |dC|. Both evaluation orders of save_s are checked against the bound here.

Formula: the backward references take mean / rstd (z~ / inv_std) as inputs; with the exact float64 statistics they
agree with float64 autograd of F.layer_norm (+ FiLM) and of the batch standardisation to 1e-11 of the scale.

Coverage: the case tables reach every build ops.ln_fwd / ops.ln_bwd can launch (helpers.LN_FWD_BUILDS, LN_BWD_BUILDS),
every d, N, L and p of the issue's table.

Discrimination is proven, not measured: each mutant of the reference must leave the per-element bound on at least half
of the elements it changes (NORMREF "least caught share" lines). Skipped, because the mutant is the reference there
or cannot show: unbiased at d = 1 / B = 1; one-pass variance outside the offset rows of the cases without y (with y the
reference does not know the roundings of v, which cost the same cancellation; it shows in rstd, since out carries
the mean's rounding of 64 spreads); eps outside the root on rows of standard deviation >= 1/4 (rstd changes by eps
(1 / sigma - 1 / (2 sigma^2)), nothing at sigma = 1/2 and a few units beyond 4); unbiased and the tail mutants on rows
whose variance is far below eps; the scale and the mask at threshold 0 (nothing is dropped or scaled) and on the const
and zero rows (y is 2^-30-sized there: the fp32 sum is x); the tail chunk at d = 512 and 1024
(no idle lane); RoPE's position at N <= L; s2 of the next row at N = 1; the ragged slab at N % 32 = 0; fold group 15
below 16 slabs; dbeta of column c + 1 at d = 1; local B where the rank is the whole batch; + lam on the diagonal and
the scalar tail at lam = 0; the j, k split at even D and D = 1; the scalar tail where D^2 % 4 = 0 or Cm is unaligned.
"""
import torch
import torch.nn.functional as F

import helpers as H

LEAST = {}
EMAX = {}


def _share(ref, bound, mut, sel=None):
    touched = mut != ref
    if sel is not None:
        touched = touched & sel
    if not touched.any():
        return None
    return ((mut - ref).abs() > bound)[touched].float().mean().item()


def _least(k, v):
    if v is not None:
        LEAST[k] = min(LEAST.get(k, 1.0), v)


def _e(name, got, ref, unit):
    """Record the excess of fp32 `got` over float64 `ref` in units of u `unit`; where the unit is 0 the bits agree."""
    err = (got.double() - ref).abs()
    pos = unit > 0
    assert (err[~pos] == 0).all(), name
    if pos.any():
        EMAX[name] = max(EMAX.get(name, 0.0), (err[pos] / (H.U24 * unit[pos])).max().item())


def _stored(names):
    for n in names:
        e = EMAX[n]
        print(f"\nNORMREF E {n}: measured {e:.4f} stored {H.NORM_E[n]} C {H.NORM_C[n]}", end="")
    print()
    for n in names:
        e = EMAX[n]
        assert e <= H.NORM_E[n] <= 1.1 * e + H.NORM_E_FLOOR, (n, e, H.NORM_E[n])
        assert H.NORM_C[n] <= 64.0


def _caught(prefix, names):
    got = {k for k in LEAST if k.startswith(prefix)}
    assert got == {prefix + n for n in names}, (got, names)
    print(f"\nNORMREF {prefix}least caught share per mutant " + ", ".join(f"{k} {LEAST[k]:.3f}" for k in sorted(got)))
    for k in got:
        assert LEAST[k] >= 0.5, f"mutant {k} leaves the bound on only {LEAST[k]:.3f} of its elements"


# ------------------------------------------------------------------------------------------ coverage
def test_cases_reach_every_build_and_edge():
    fc = H.ln_fwd_cases()
    builds = set()
    for c in fc:
        tr = c["tr"]
        codes = H.ln_fwd_codes(tr[0], tr[1] if c["hy"] else None, tr[2])
        b = H.ln_fwd_dispatch(*codes, c["hy"], c["hf"], c["d"], bool(c["rope"]))
        assert b is not None, c["id"]
        assert not c["hf"] or c["N"] % c["L"] == 0
        assert not c["alias"] or tr[0] == "f32"
        builds.add(b)
    assert builds == set(H.LN_FWD_BUILDS) and len(H.LN_FWD_BUILDS) == 30
    assert {c["d"] for c in fc} >= {8, 200, 512, 520, 1024}
    assert {c["N"] for c in fc} >= {1, 5, 33, 70}
    assert {c["L"] for c in fc if c["hf"]} >= {1, 20, 32, 37, 576}
    assert {c["p"] for c in fc if c["hy"]} == set(H.LN_P)
    assert [H.ln_thr(p) for p in H.LN_P] == [6554, 32768, 1, 0, 0]
    assert any(c["alias"] for c in fc)
    assert len({c["id"] for c in fc}) == len(fc)
    bc = H.ln_bwd_cases()
    assert {H.ln_bwd_build(c) for c in bc} == set(H.LN_BWD_BUILDS) and len(H.LN_BWD_BUILDS) == 20
    assert {c["d"] for c in bc} >= {8, 200, 512, 520, 1024, 100, 1}
    assert {c["N"] for c in bc} >= {1, 5, 33, 70, 1100}
    assert {c["L"] for c in bc if c["L"]} >= {1, 20, 32, 37, 576}
    assert {c["p"] for c in bc} == set(H.LN_P)
    assert any(c["off4"] for c in bc) and sum(c["part"] for c in bc) >= 4
    for c in bc:
        assert not c["part"] or (H.ln_bwd_build(c)[0][0] == "fused" and c["params"]), c["id"]
        assert not c["L"] or c["N"] % c["L"] == 0
    assert {b for b, _ in H.LFD_BC} == {1, 2, 3, 32, 33} and {c for _, c in H.LFD_BC} == {1, 257, 1000}
    assert [d for d, _ in H.LFD_D] == [1, 33, 256, 1030, 256] and H.LFD_LAM == (0.0, 5e-3)


# ------------------------------------------------------------------------------------------ LayerNorm forward
def test_ln_fwd_cost_and_mutants():
    for i, c in enumerate(H.ln_fwd_cases()):
        x, y, gamma, beta, film, keep, rope, kind = H.ln_fwd_operands(i)
        N, d, L, p = c["N"], c["d"], c["L"], c["p"]
        kw = dict(rope=rope, rope_L=c["rope"])
        r = H.ln_fwd_ref64(x, y, gamma, beta, film, L, p, keep, **kw)
        if y is not None:
            assert (y.float() != 0).all()
        for fma in (False, True):
            s, mean, rstd, o = H.ln_fwd_emulate(x, y, gamma, beta, film, L, p, keep, fma=fma)
            assert ((s.double() - r.s).abs() <= r.b_s).all(), c["id"]          # derived: both evaluation orders
            _e("mean", mean, r.mean, r.u_mean)
            _e("rstd", rstd, r.rstd, r.u_rstd)
            _e("out", o, r.out, r.u_out)
            if rope is not None:
                for order in (0, 1, 2):
                    q = H.rope_fwd_eval32(o, rope[0], rope[1], c["rope"], order).to(torch.bfloat16)
                    assert ((q.double() - r.rope).abs() <= r.b_rope).all(), c["id"]
        # ---- mutants
        def m(name):
            return H.ln_fwd_ref64(x, y, gamma, beta, film, L, p, keep, mut=name, **kw)
        live = (r.rstd < 0.5 * H.LN_EPS ** -0.5)                     # rows whose variance is not far below eps
        if d > 1:
            _least("lnf unbiased", _share(r.rstd, r.b_rstd, m("unbiased").rstd, live))
        _least("lnf eps_out", _share(r.rstd, r.b_rstd, m("eps_out").rstd, r.rstd > 4.0))
        if y is None:
            _least("lnf onepass", _share(r.rstd, r.b_rstd, m("onepass").rstd, kind == 1))
        if film is not None:
            _least("lnf fs", _share(r.out, r.b_out, m("fs").out))
            if N > 1:
                _least("lnf film_prev", _share(r.out, r.b_out, m("film_prev").out))
        if y is not None and H.ln_thr(p):
            loud = ((kind != 3) & (kind != 4))[:, None].expand(N, d)      # y is 2^-30-sized on the const and zero rows
            _least("lnf noscale", _share(r.s, r.b_s, m("noscale").s, loud))
            _least("lnf mask_next", _share(r.s, r.b_s, m("mask_next").s, loud))
        if d in (200, 520):
            _least(f"lnf tail{d}", _share(r.out, r.b_out, m("tail").out, live[:, None].expand(N, d)))
        if rope is not None:
            _least("lnf rope_sign", _share(r.rope, r.b_rope, m("rope_sign").rope))
            _least("lnf rope_pos", _share(r.rope, r.b_rope, m("rope_pos").rope))
    _stored(["mean", "rstd", "out"])
    _caught("lnf ", ["unbiased", "eps_out", "onepass", "fs", "film_prev", "noscale", "mask_next", "tail200", "tail520",
                     "rope_sign", "rope_pos"])


def test_ln_fwd_formula_against_layer_norm():
    for i, c in enumerate(H.ln_fwd_cases()):
        x, y, gamma, beta, film, keep, rope, kind = H.ln_fwd_operands(i)
        r = H.ln_fwd_ref64(x, y, gamma, beta, film, c["L"], c["p"], keep)
        ref = F.layer_norm(r.s, (c["d"],), gamma.double(), beta.double(), H.LN_EPS)
        if film is not None:
            B = c["N"] // c["L"]
            ref = (ref.view(B, c["L"], -1) * (1.0 + film[0].double()[:, None]) + film[1].double()[:, None]).view_as(ref)
        assert ((ref - r.out).abs() <= 1e-11 * r.u_out + 1e-300).all(), c["id"]


# ------------------------------------------------------------------------------------------ LayerNorm backward
def test_ln_bwd_cost_and_mutants():
    for i, c in enumerate(H.ln_bwd_cases()):
        dout, s, mean, rstd, gamma, beta, fs, keep, old, kind = H.ln_bwd_operands(i)
        N, d, L, p = c["N"], c["d"], c["L"], c["p"]
        r = H.ln_bwd_ref64(dout, s, mean, rstd, gamma, beta, fs, L, p, keep, old)
        kern = H.ln_bwd_dispatch(d, N, L, L > 0, c["params"], not c["off4"])
        dres, sums = H.ln_bwd_emulate(dout, s, mean, rstd, gamma, beta, fs, L, kern, old, c["part"])
        _e("dres", dres, r.dres, r.u_dres)
        for name, got in zip(("dgamma", "dbeta", "dfs", "dfh"), sums):
            _e("par", got, getattr(r, name), getattr(r, "u_" + name))

        def m(name):
            return H.ln_bwd_ref64(dout, s, mean, rstd, gamma, beta, fs, L, p, keep, old, mut=name)
        _least("lnb no_s1", _share(r.dres, r.b_dres, m("no_s1").dres))
        if N > 1:
            _least("lnb s2_next", _share(r.dres, r.b_dres, m("s2_next").dres))
        if fs is not None:
            _least("lnb dgamma_nofs", _share(r.dgamma, r.b_dgamma, m("dgamma_nofs").dgamma))
            _least("lnb dfs_nobeta", _share(r.dfs, r.b_dfs, m("dfs_nobeta").dfs))
        if N % H.LN_SLAB and kern[0] == "fused":
            _least("lnb ragged", _share(r.dgamma, r.b_dgamma, m("ragged").dgamma))
        if c["part"] and (N + H.LN_SLAB - 1) // H.LN_SLAB > 16:
            q = m("fold15")
            if L == 0:
                _least("lnb fold15", _share(r.dgamma, r.b_dgamma, q.dgamma))
            elif L // H.LN_SLAB > 16:
                _least("lnb fold15", _share(r.dfs, r.b_dfs, q.dfs))
        if d > 1:
            _least("lnb dbeta_next", _share(r.dbeta, r.b_dbeta, m("dbeta_next").dbeta))
        q = m("no_old")
        for name in ("dgamma", "dbeta") + (("dfs", "dfh") if fs is not None else ()):
            _least("lnb no_old", _share(getattr(r, name), getattr(r, "b_" + name), getattr(q, name)))
    _stored(["dres", "par"])
    _caught("lnb ", ["no_s1", "s2_next", "dgamma_nofs", "dfs_nobeta", "ragged", "fold15", "dbeta_next", "no_old"])


def test_ln_bwd_formula_against_autograd():
    for i, c in enumerate(H.ln_bwd_cases()):
        if c["N"] > 100:
            continue
        dout, s, _, _, gamma, beta, fs, keep, old, kind = H.ln_bwd_operands(i)
        N, d, L = c["N"], c["d"], c["L"]
        sd = s.double().requires_grad_(True)
        gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        out = F.layer_norm(sd, (d,), gm, bt, H.LN_EPS)
        leaves = [sd, gm, bt]
        if fs is not None:
            fsd = fs.double().requires_grad_(True)
            fhd = torch.zeros_like(fsd).requires_grad_(True)
            out = (out.view(N // L, L, d) * (1.0 + fsd[:, None]) + fhd[:, None]).view(N, d)
            leaves += [fsd, fhd]
        grads = torch.autograd.grad(out, leaves, dout.double())
        mean = s.double().mean(1)
        rstd = 1.0 / torch.sqrt(s.double().var(1, unbiased=False) + H.LN_EPS)
        zero = [torch.zeros_like(t) if t is not None else None for t in old]
        r = H.ln_bwd_ref64(dout, s, mean, rstd, gamma, beta, fs, L, 0.0, keep, zero)
        # at d = 1 and on constant rows autograd's dres is 0 up to rounding: the scale decides
        for name, gv in zip(("dres", "dgamma", "dbeta", "dfs", "dfh"), grads):
            assert ((getattr(r, name) - gv).abs() <= 1e-9 * getattr(r, "u_" + name) + 1e-11).all(), (c["id"], name)


# ------------------------------------------------------------------------------------------ L_fd
def test_lfd_cost_and_mutants():
    for B, C in H.LFD_BC:
        z, dzt, zt, inv, s1, s2, sums = H.lfd_operands(B, C)
        inv_n = 1.0 / (H.LFD_RANKS * B)
        f = H.lfd_std_ref64(z)
        a = H.lfd_std_ref64(z, s1=s1, s2=s2, inv_n=inv_n)
        c1, c2 = H.lfd_colstat_ref64(z), H.lfd_colstat_ref64(z, s1, inv_n)
        for zdt in (torch.float32, torch.bfloat16):
            ztq = zt.to(zdt).float()
            w = H.lfd_bwd_ref64(dzt, ztq, inv)
            wa = H.lfd_bwd_ref64(dzt, ztq, inv, sums=sums, inv_n=inv_n, scale=H.LFD_W)
            e = H.lfd_emulate(z, dzt, ztq, inv, s1, s2, sums, inv_n, H.LFD_W)
            _e("lfd_is", e["inv"], f.inv, f.inv)
            _e("lfd_is", e["inv_a"], a.inv, a.inv)
            _e("lfd_zt", e["zt"], f.zt, f.u_zt)
            _e("lfd_zt", e["zt_a"], a.zt, a.u_zt)
            _e("lfd_col", e["c1"], c1.out, c1.u)
            _e("lfd_col", e["c2"], c2.out, c2.u)
            _e("lfd_col", e["cs"], w.cs, w.u_cs)
            _e("lfd_dz", e["dz"], w.dz, w.u_dz)
            _e("lfd_dz", e["dz_a"], wa.dz, wa.u_dz)
            _least("lfd no_m2", _share(w.dz, w.b_dz, H.lfd_bwd_ref64(dzt, ztq, inv, mut="no_m2").dz))
            _least("lfd localB", _share(wa.dz, wa.b_dz, H.lfd_bwd_ref64(dzt, ztq, inv, sums=sums, inv_n=inv_n, scale=H.LFD_W,
                                                                         mut="localB").dz))
            _least("lfd noW", _share(wa.dz, wa.b_dz, H.lfd_bwd_ref64(dzt, ztq, inv, sums=sums, inv_n=inv_n, scale=H.LFD_W,
                                                                     mut="noW").dz))
        if B > 1:
            _least("lfd unbiased", _share(f.inv, f.b_inv, H.lfd_std_ref64(z, mut="unbiased").inv, f.inv < 100.0))
        _least("lfd localB", _share(a.zt, a.b_zt, H.lfd_std_ref64(z, s1=s1, s2=s2, inv_n=inv_n, mut="localB").zt))
    for D, off in H.LFD_D:
        Cm = H.lfd_cm(D)
        assert (Cm.diagonal() == 1.0).any()
        for lam in H.LFD_LAM:
            r = H.lfd_loss_ref64(Cm, lam)
            got = H.lfd_loss_emulate(Cm, lam, aligned=not off)
            _e("lfd_loss", got.reshape(1), r.loss.reshape(1), r.u.reshape(1))
            d0 = H.lfd_dloss_ref64(Cm, 0.625, lam)
            l32 = torch.tensor(lam, dtype=torch.float32)
            g32 = torch.tensor(0.625, dtype=torch.float32)
            eye = torch.eye(D, dtype=torch.bool)
            for ev in (g32 * torch.where(eye, -2.0 * (1.0 - Cm), 2.0 * l32 * Cm),
                       torch.where(eye, (g32 * -2.0) * (1.0 - Cm), (g32 * 2.0 * l32) * Cm)):
                assert ((ev.double() - d0.dC).abs() <= d0.b).all()
                assert ((ev.to(torch.bfloat16).double() - d0.dC).abs() <= d0.b_bf).all()
            if lam > 0:
                _least("lfd diag_lam", _share(r.loss.reshape(1), r.b.reshape(1), H.lfd_loss_ref64(Cm, lam, mut="diag_lam").loss.reshape(1)))
                if (D * D) % 4 and not off:
                    _least("lfd tail", _share(r.loss.reshape(1), r.b.reshape(1), H.lfd_loss_ref64(Cm, lam, mut="tail").loss.reshape(1)))
            if D % 2 and D > 1:
                _least("lfd jk", _share(d0.dC, d0.b_bf, H.lfd_dloss_ref64(Cm, 0.625, lam, mut="jk").dC))
    _stored(["lfd_is", "lfd_zt", "lfd_col", "lfd_dz", "lfd_loss"])
    _caught("lfd ", ["unbiased", "no_m2", "localB", "noW", "diag_lam", "jk", "tail"])


def test_lfd_formula_against_autograd():
    for B, C in H.LFD_BC:
        z, dzt, _, _, _, _, _ = H.lfd_operands(B, C)
        zd = z.double().requires_grad_(True)
        m = zd.mean(0, keepdim=True)
        is_ = 1.0 / torch.sqrt(((zd - m) ** 2).mean(0, keepdim=True) + H.LN_EPS)
        zt = (zd - m) * is_
        f = H.lfd_std_ref64(z)
        assert ((f.zt - zt.detach()).abs() <= 1e-12 * f.u_zt + 1e-300).all()
        (gz,) = torch.autograd.grad(zt, zd, dzt.double())
        w = H.lfd_bwd_ref64(dzt, zt.detach(), is_.detach()[0])
        assert ((w.dz - gz).abs() <= 1e-9 * w.u_dz + 1e-300).all(), (B, C)
    for D, _ in H.LFD_D[:3]:
        Cm = H.lfd_cm(D)
        for lam in H.LFD_LAM:
            l = float(torch.tensor(lam, dtype=torch.float32))
            Cd = Cm.double().requires_grad_(True)
            off = Cd - torch.diag(Cd.diagonal())
            loss = ((1.0 - Cd.diagonal()) ** 2).sum() + l * (off ** 2).sum()
            r = H.lfd_loss_ref64(Cm, lam)
            assert abs(r.loss.item() - loss.item()) <= 1e-11 * r.u.item()
            (g,) = torch.autograd.grad(loss, Cd)
            d0 = H.lfd_dloss_ref64(Cm, 1.0, lam)
            assert ((d0.dC - g).abs() <= 1e-12 * d0.dC.abs() + 1e-300).all()
