"""What tests/test_gpu_cond.py may ask of the decoder's conditioning kernels (the linear family, small_dw, rows_mean,
time_embed: csrc/small.hip) and of RoPE and the token embedding (csrc/misc.hip), settled from the reference alone
before any kernel runs.

E: each kernel's arithmetic emulated on the CPU in its own order (helpers.lin_emulate: linear4's four K-quarter FMA chains
and linrt's eight wave chains; dw_emulate: one FMA chain over the rows, then the old value; rows_mean_emulate: 32 row
slices, added in order, divided by (float) the count; the oracle's fp32 time_embedding; silu32 / dsilu32 on
helpers.silu_grid()) against float64, in units of 2^-24 times the per-element scale, the maximum over every case of
helpers.LIN_CASES, dw_cases(), RM_S x RM_D x {f32, bf16} (and the masked kernel's holes case), TE_D x TE_T. The kernels are
allowed COND_C = 8 E units, hard cap 64.
    family   scale                                    measured E    stored E    C = 8 E
    lin      sum_k |in| |W| + |b|                     5.19          5.7         45.6
    dw       |old| + |dy|^T |x|  (db: sum_r |dy|)     4.83          5.3         42.4
    rm       mean |x|                                 3.00          3.3         26.4
    te       |a| (1 + lin_k) + 1                      1.06          1.2          9.6
    silu     |silu(v)|  (+ 2^-121: expf overflow)     2.31          2.55        20.4
    g        1 + |x|                                  1.30          1.45        11.6
RoPE's constants are derived, not measured: the forward is two roundings (2 u (|x1 c| + |x2 s'|)), the backward three
(3 u (|dx| + |a C| + |b S|)); every evaluation order a compiler may choose (either product through the FMA, neither,
two chained FMAs) is checked against them here, with an f32 and a bf16 result. embed_fwd is one IEEE add (bit equality),
embed_bwd n roundings for n contributions in any order.

Discrimination is proven, not measured: each mutant of the reference must leave the per-element bound on at least half
of the elements it changes. Measured shares (the least over the cases a mutant is asserted on):
    linear  the last k dropped (every case)                                   0.994
            one 512-chunk dropped (linear4 launches)                          1.000
            one K-quarter dropped (linear4 launches with K > 128)             1.000
            wave 7's chunks dropped (linrt launches with K > 448)             1.000
            bias[n + 1] (cases with a bias and N > 1)                         1.000
            job j + 1's weights (J > 1)                                       1.000
            W read in the other layout (N K > 1)                              1.000
            act 2 with the bias added in (cases with a bias)                  1.000
            silu' without the x (1 - sigma) term (every case)                 0.998
            row 32 taken from row 0 (R > 32)                                  1.000
    dw      the last row dropped (every job)                                  0.997
            the old value not added (every job)                               1.000
            job j + 1's dy (the 17-job call: equal shapes)                    1.000
            db summed over N instead of R (jobs with N > 1 or R > 1)          1.000
    rm      row S - 1 dropped (S > 1)                                         0.996
            rows >= 128 dropped (S > 128)                                     0.996
            divided by S + 1 (every case)                                     0.984
    te      step log_max / half (d >= 4)                                      0.920
            the half = 1 bug itself (d = 2, 3)                                1.000
            sin and cos swapped (every d)                                     1.000
            f from k + 1 (d >= 4)                                             0.875
    rope    sin's sign (L > 1)                                                1.000
            position r instead of r % L (N > L)                               0.994
            pairs (i, i + h) in place of (2 i, 2 i + 1) (d > 2)               1.000
    embed   a padding row counted                                             1.000
            dtb of entry b + 1                                                1.000
Skipped, because the mutant is the reference there: the layout mutant at N = K = 1; job j + 1's dy in the launches whose
jobs differ in shape (that dy has another N); db over N at N = R = 1; step and k + 1 at half = 1 (there is no step);
sin's sign at L = 1 (every position is 0: sin = 0); position r at L = N; the pair mutant at d = 2 (one pair either way).
The time-embedding mutants that move f change cos a by a^2 / 2 times the relative change: for t = 1 and small a that is
below one rounding of cos a ~ 1, so those elements cannot show and the share is what the sines and the larger t give.
"""
import pytest
import torch

import helpers as H
from oracle import fddm_oracle as O

LEAST = {}


def _share(ref, bound, mut, sel=None):
    """Share of the elements mutant output `mut` changes (within sel) at which it leaves `bound` around `ref`."""
    touched = mut != ref
    if sel is not None:
        touched = touched & sel
    assert touched.any()
    return ((mut - ref).abs() > bound)[touched].float().mean().item()


def _least(k, v):
    LEAST[k] = min(LEAST.get(k, 1.0), v)


def _stored(name, e):
    assert e <= H.COND_E[name] <= 1.1 * e + H.COND_E_FLOOR, (name, e, H.COND_E[name])


def _caught(prefix, names):
    got = {k for k in LEAST if k.startswith(prefix)}
    assert got == {prefix + n for n in names}, got
    print(f"\nCONDREF {prefix} least caught share per mutant " + ", ".join(f"{k} {LEAST[k]:.3f}" for k in sorted(got)))
    for k in got:
        assert LEAST[k] >= 0.5, f"mutant {k} leaves the bound on only {LEAST[k]:.3f} of its elements"


def test_linear_cost_and_mutants():
    E = 0.0
    for cid, kernels, R, K, N, J, pads, given in H.LIN_CASES:
        assert H.lin_dispatch(R, N, J) == kernels, cid
        x, W, b, aux = H.lin_operands(cid)
        r = H.lin_ref64(cid)
        assert r.pre.shape == (R, J, N) and (r.s0 > 0).all()
        bb = b if given else None
        run = torch.zeros(J, dtype=torch.bool), torch.zeros(J, dtype=torch.bool)      # jobs on linear4, on linrt
        # ---- E: each launch's kernel in its own order; the whole fp32 evaluation stays inside every bound
        for i, kern in enumerate(kernels):
            sl = slice(16 * i, 16 * i + 16)
            run[kern == "linrt"][sl] = True
            y0, y = H.lin_emulate(x, W[sl], bb[sl] if given else None, kern)
            E = max(E, ((y.double() - r.pre[:, sl]).abs() / (H.U24 * r.s[:, sl])).max().item(),
                    ((y0.double() - r.y0[:, sl]).abs() / (H.U24 * r.s0[:, sl])).max().item())
            assert ((H.silu32(y).double() - r.silu[:, sl]).abs() <= r.b_silu[:, sl]).all(), cid
            dx = y0 * H.dsilu32(aux)[:, None, :]
            assert ((dx.double() - r.dx[:, sl]).abs() <= r.b_dx[:, sl]).all(), cid
        assert (run[0] ^ run[1]).all()
        # ---- mutants
        xd, Wd = x.double(), W.double()

        def part(ks, jobs=None):
            """pre without the k of `ks` (in the jobs of `jobs`)"""
            d = torch.einsum("rk,jnk->rjn", xd[:, ks], Wd[:, :, ks])
            if jobs is not None:
                d = d * jobs.double()[None, :, None]
            return H.lin_out64(r.y0 - d, r.s0, bb, aux)

        ks = torch.arange(K)
        _least("lin last_k", _share(r.pre, r.b_pre, part(ks[-1:]).pre))
        if run[0].any():
            ch = 1 if K > 512 else 0
            _least("lin chunk", _share(r.pre, r.b_pre, part(ks[(ks // 512) == ch], run[0]).pre))
            if K > 128:
                _least("lin quarter", _share(r.pre, r.b_pre, part(ks[(ks % 512) // 128 == 1], run[0]).pre))
        if run[1].any() and K > 448:
            _least("lin wave7", _share(r.pre, r.b_pre, part(ks[(ks // 64) % 8 == 7], run[1]).pre))
        if given and N > 1:
            _least("lin bias_next", _share(r.pre, r.b_pre, H.lin_out64(r.y0, r.s0, b.roll(-1, 1), aux).pre))
        if J > 1:
            _least("lin job_next", _share(r.pre, r.b_pre, H.lin_out64(r.y0.roll(-1, 1), r.s0, bb, aux).pre))
        if N * K > 1:
            Wo = Wd.reshape(J, K, N).transpose(1, 2)
            _least("lin layout", _share(r.pre, r.b_pre, H.lin_out64(torch.einsum("rk,jnk->rjn", xd, Wo), r.s0, bb, aux).pre))
        if given:
            _least("lin act2_bias", _share(r.dx, r.b_dx, r.pre * r.g))
        _least("lin g_sigma", _share(r.dx, r.b_dx, r.y0 * H.sigmoid64(aux)[:, None, :]))
        if R > 32:
            y0m = r.y0.clone()
            y0m[32:] = r.y0[: R - 32]
            _least("lin row32", _share(r.pre, r.b_pre, H.lin_out64(y0m, r.s0, bb, aux).pre))
    print(f"\nCONDREF lin: E {E:.2f}")
    _stored("lin", E)
    _caught("lin ", ["last_k", "chunk", "quarter", "wave7", "bias_next", "job_next", "layout", "act2_bias", "g_sigma",
                     "row32"])


def test_silu_and_its_derivative_on_the_grid():
    """C_silu and C_g: the two fp32 expressions of small.hip's epilogues on about 4000 points, the zero of silu', +-0 and
    overflowing expf included."""
    v = H.silu_grid()
    assert 4000 <= v.numel() <= 4100 and (v == 0).sum() >= 2 and torch.isinf(torch.exp(-v)).any()
    vd = v.double()
    silu = vd * torch.sigmoid(vd)
    es = (((H.silu32(v).double() - silu).abs() - H.SILU_FLUSH).clamp_min(0.0) / (H.U24 * silu.abs()).clamp_min(1e-300))
    eg = (H.dsilu32(v).double() - H.dsilu64(v)).abs() / (H.U24 * (1.0 + vd.abs()))
    assert torch.isfinite(H.silu32(v)).all() and torch.isfinite(H.dsilu32(v)).all()
    print(f"\nCONDREF silu: E {es.max().item():.2f}; g: E {eg.max().item():.2f}")
    _stored("silu", es.max().item())
    _stored("g", eg.max().item())
    # a relative bound on g cannot hold: at its zero the fp32 value is wrong by far more than C u |g|
    z = torch.tensor([H.SILU_G_ZERO])
    assert H.dsilu64(z).abs().item() < 1e-7


def test_dw_cost_and_mutants():
    E = 0.0
    for cid, R, jobs in H.dw_cases():
        ops_ = H.dw_operands(cid)
        refs = []
        for (N, K, given), (dyb, x, dW, db) in zip(jobs, ops_):
            dy = dyb[:, 1:1 + N]
            assert dy.stride(0) == N + H.DW_PAD > N
            refs.append(H.dw_ref64(dy, x, dW, db))
        for j, ((N, K, given), (dyb, x, dW, db), r) in enumerate(zip(jobs, ops_, refs)):
            dy = dyb[:, 1:1 + N]
            eW, eb = H.dw_emulate(dy, x, dW, db)
            E = max(E, ((eW.double() - r.dW).abs() / (H.U24 * r.sW)).max().item(),
                    ((eb.double() - r.db).abs() / (H.U24 * r.sb)).max().item())
            m = H.dw_ref64(dy[:-1], x[:-1], dW, db)
            _least("dw last_row", _share(r.dW, r.b_dW, m.dW))
            _least("dw last_row", _share(r.db, r.b_db, m.db))
            _least("dw no_old", _share(r.dW, r.b_dW, r.dW - dW.double()))
            _least("dw no_old", _share(r.db, r.b_db, r.db - db.double()))
            if cid == "many":
                nxt = ops_[(j + 1) % len(jobs)][0][:, 1:1 + N]
                m = H.dw_ref64(nxt, x, dW, db)
                _least("dw dy_next", _share(r.dW, r.b_dW, m.dW))
                _least("dw dy_next", _share(r.db, r.b_db, m.db))
            if N > 1 or R > 1:
                over_n = db.double() + dy.double().sum(1)[torch.arange(N) % R]
                _least("dw db_over_n", _share(r.db, r.b_db, over_n))
    print(f"\nCONDREF dw: E {E:.2f}")
    _stored("dw", E)
    _caught("dw ", ["last_row", "no_old", "dy_next", "db_over_n"])


def test_rows_mean_cost_and_mutants():
    E = 0.0
    for S in H.RM_S:
        for d in H.RM_D:
            for dt in ("f32", "bf16"):
                x = H.rm_operands(S, d, dt)
                assert x.dtype == (torch.bfloat16 if dt == "bf16" else torch.float32)
                r = H.rm_ref64(x)
                E = max(E, ((H.rows_mean_emulate(x).double() - r.mean).abs() / (H.U24 * r.s)).max().item())
                xd = x.double()
                if S > 1:
                    _least("rm last_row", _share(r.mean, r.b, xd[:, :-1].sum(1) / S))
                if S > 128:
                    _least("rm first_128", _share(r.mean, r.b, xd[:, :128].sum(1) / S))
                _least("rm s_plus_1", _share(r.mean, r.b, xd.sum(1) / (S + 1)))
    # the masked kernel: the same order over the kept rows, the padded rows never read
    S = H.RM_HOLES_S
    keep = H.rm_holes(S)
    assert 0 < keep[0].sum() < S and keep[1].sum() == 0
    for d in H.RM_D:
        for dt in ("f32", "bf16"):
            x = H.rm_operands(S, d, dt).clone()
            x[keep == 0] = float("nan")
            r = H.rm_ref64(x, keep)
            em = H.rows_mean_emulate(x, keep)
            E = max(E, ((em[0].double() - r.mean[0]).abs() / (H.U24 * r.s[0])).max().item())
            assert (em[1] == 0).all() and (r.mean[1] == 0).all()
    print(f"\nCONDREF rm: E {E:.2f}")
    _stored("rm", E)
    _caught("rm ", ["last_row", "first_128", "s_plus_1"])


def test_time_embed_cost_and_mutants():
    E = 0.0
    t = torch.tensor(H.TE_T)
    for d in H.TE_D:
        r = H.te_ref64(t, d)
        assert r.emb.shape == (len(H.TE_T), d)
        emu = O.time_embedding(t, d, H.TE_MAX_STEPS)
        E = max(E, ((emu.double() - r.emb).abs() / r.unit).max().item())
        if d % 2:
            assert (r.emb[:, -1] == 0).all() and (emu[:, -1] == 0).all()
        half = d // 2
        if half > 1:
            _least("te step", _share(r.emb, r.b, H.te_ref64(t, d, step_div=half).emb))
            _least("te k_plus_1", _share(r.emb, r.b, H.te_ref64(t, d, kshift=1).emb))
        else:
            m = H.te_ref64(t, d, half1_bug=True).emb
            _least("te half1_bug", _share(r.emb, r.b, m))
            # the finding: t = 1 gives sin(1), the parent's kernel gave sin(1 / max_steps)
            assert abs(r.emb[1, 0].item() - 0.8414709848) < 1e-9 and abs(m[1, 0].item() - 1e-4) < 1e-9
        _least("te swap", _share(r.emb, r.b, H.te_ref64(t, d, swap=True).emb))
    print(f"\nCONDREF te: E {E:.2f}")
    _stored("te", E)
    _caught("te ", ["step", "k_plus_1", "half1_bug", "swap"])


def test_rope_orders_and_mutants():
    seen = set()
    for N, L, d, _ in H.ROPE_CASES:
        if (N, L, d) in seen:
            continue
        seen.add((N, L, d))
        x, dy, dx, cos, sin = H.rope_operands(N, L, d)
        assert cos.shape == (N, d) and N >= L
        f, bk = H.rope_fwd_ref64(x, cos, sin, L), H.rope_bwd_ref(dy, dx, cos, sin, L)
        # oracle's formula and its autograd transpose are what the references compute
        xr, p = x.double().requires_grad_(True), torch.arange(N) % L
        o = O.rope_apply(xr, cos.double()[p], sin.double()[p])
        assert torch.equal(o.detach(), f.out)
        o.backward(dy.double())
        assert ((dx.double() + xr.grad - bk.dx).abs() <= 1e-15 * bk.b / H.U24).all()
        for order in (0, 1, 2):
            e = H.rope_fwd_eval32(x, cos, sin, L, order)
            assert ((e.double() - f.out).abs() <= f.b).all(), (N, L, d, order)
            eb = e.to(torch.bfloat16)
            assert ((eb.double() - f.out).abs() <= H.bf16_round_bound(f.out, f.b)).all(), (N, L, d, order)
        for order in (0, 1, 2, 3):
            e = H.rope_bwd_eval32(dy, dx, cos, sin, L, order)
            assert ((e.double() - bk.dx).abs() <= bk.b).all(), (N, L, d, order)
        muts = []
        if L > 1:
            muts.append(("sin_sign", dict(sin_sign=-1.0)))
        if N > L:
            muts.append(("pos", dict(pos=torch.arange(N))))
        if d > 2:
            muts.append(("halves", dict(halves=True)))
        for name, kw in muts:
            _least("rope " + name, _share(f.out, f.b, H.rope_fwd_ref64(x, cos, sin, L, **kw).out))
            _least("rope " + name, _share(bk.dx, bk.b, H.rope_bwd_ref(dy, dx, cos, sin, L, **kw).dx))
    _caught("rope ", ["sin_sign", "pos", "halves"])


def test_embed_reference_and_mutants():
    for case in H.EMBED_CASES:
        d, L, B, V, pad = case
        tok, E, tb, dx, dE, dtb = H.embed_operands(*case)
        N = B * L
        assert N % 8 and (tok[8:16] == pad).all() and tok.min() >= 0 and tok.max() < V
        x = H.embed_fwd_exact(tok, E, tb, L)
        assert ((x.double() - (E.double()[tok] + tb.double().repeat_interleave(L, 0))).abs()
                <= H.U24 * x.double().abs()).all()
        r = H.embed_bwd_ref64(tok, dx, dE, dtb, L, pad)
        assert r.n[pad] == 0 and (r.b_dE[pad] == 0).all() and torch.equal(r.dE[pad], dE[pad].double())
        if V == 50:
            assert (r.n == 0).sum() > 1, "a row no token names"
        # fp32 accumulation in two orders stays inside the bounds
        live = tok != pad
        for order in (torch.arange(N), torch.arange(N).flip(0)):
            o = order[live[order]]
            e = dE.clone().index_add_(0, tok[o], dx[o])
            assert ((e.double() - r.dE).abs() <= r.b_dE).all()
        e = dtb + dx.view(B, L, d).sum(1)
        assert ((e.double() - r.dtb).abs() <= r.b_dtb).all()
        m = H.embed_bwd_ref64(tok, dx, dE, dtb, L, pad, count_pad=True)
        _least("embed count_pad", _share(r.dE, r.b_dE, m.dE))
        if B > 1:
            _least("embed dtb_next", _share(r.dtb, r.b_dtb, H.embed_bwd_ref64(tok, dx, dE, dtb, L, pad, dtb_shift=1).dtb))
    _caught("embed ", ["count_pad", "dtb_next"])


def test_constants_and_tables():
    assert set(H.COND_E) == {"lin", "dw", "rm", "te", "silu", "g"}
    for k, e in H.COND_E.items():
        assert H.COND_C[k] == 8.0 * e and H.COND_C[k] <= 64.0
    by = {c[0]: c for c in H.LIN_CASES}
    assert len(by) == len(H.LIN_CASES)
    # every mechanism the table is there for
    assert by["l4-prefetch"][3] > 3 * 512 and by["l4-ragged"][3] % 4 == 3 and by["l4-ragged"][2] == 33
    assert by["l4-strided"][6] == (1, 4) and not by["l4-strided"][7] and not by["rt-short"][7]
    assert -(-by["rt-trips"][3] // 64) == 18 and by["rt-trips"][3] % 64 == 12
    assert by["rt-tail"][4] % 4 and by["rt-short"][3] < 64
    assert by["split"][1] == ("linrt", "linear4") and by["rt-24"][1] == ("linrt", "linrt")
    assert any(c[2] > 32 and c[1] == ("linear4",) for c in H.LIN_CASES), "blockIdx.z > 0 on linear4"
    shapes = {j[:2] for _, _, jobs in H.dw_cases() for j in jobs}
    assert shapes >= set(H.DW_SHAPES) and any(k % 4 for _, k in shapes)
    assert {len(c[2]) for c in H.dw_cases()} == {4, 17} and {c[1] for c in H.dw_cases()} >= {45, 1, 64}
    assert any(not g for c in H.dw_cases() for _, _, g in c[2]) and any(g for c in H.dw_cases() for _, _, g in c[2])
    assert max(H.RM_S) > 96 + 31 and any(d % 8 == 0 and d % 64 for d in H.RM_D) and any(d % 8 for d in H.RM_D)
    assert {2, 3} <= set(H.TE_D) and 0 in H.TE_T
    vec = [c for c in H.ROPE_CASES if H.rope_kernel_is_vector(c[2], c[3])]
    assert len(vec) == 4 and {c[2] for c in H.ROPE_CASES if c not in vec} == {2, 6, 128}
    assert {c[0] for c in H.EMBED_CASES} == {8, 520, 6} and {c[1] for c in H.EMBED_CASES} == {1, 3, 9}
    assert {c[3] for c in H.EMBED_CASES} == {5, 50} and {c[4] for c in H.EMBED_CASES} == {0, 3}


@pytest.mark.parametrize("d", [2, 3])
def test_time_embedding_of_one_frequency_is_the_linspace_start(d):
    """torch.linspace(0, log max_steps, 1) is [0]: the oracle, and so the reference model, uses f = 1 at d = 2, 3."""
    t = torch.tensor([1, 7])
    want = torch.stack([torch.sin(t.double()), torch.cos(t.double())], 1)
    got = O.time_embedding(t, d, H.TE_MAX_STEPS)
    assert ((got[:, :2].double() - want).abs() <= 4 * H.U24).all()
