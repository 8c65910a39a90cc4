"""What tests/test_gpu_wavlm_front.py may ask of the WavLM front-end kernels (conv layer 0 + GroupNorm + GELU, the
positional conv, the relative-position gate), settled from the reference alone before any kernel runs.

E: each kernel's arithmetic emulated on the CPU in its own order (helpers.conv0_emulate_apply: ten fp32 FMAs in tap order,
then fma(y, sc, sh) with f32 sc / sh made from float64 statistics; helpers.conv0_emulate_mfma: the hi/lo bf16 split, 32
exact products added in fp32; helpers.posconv_emulate: 32-wide K chunks of exact bf16 products added in fp32, tap-major;
helpers.gate_emulate: fp32 FMAs in channel order from the bias, two sums of four, fp32 exp) against float64, in units of
the family's unit times the per-element error scale s, the maximum over every case of helpers.CONV0_CASES (both
emulations on every case), POSCONV_CASES, GATE_CASES. The kernels are allowed FRONT_C = 8 E units, hard cap 64.
    family         unit     measured E    stored E    C = 8 E
    conv0_f32      2^-24    4.65           5.1          40.8
    conv0_split    2^-18    4.26           4.65         37.2
    posconv        2^-24    1.36           1.49         11.92
    gate           2^-24    2.18           2.39         19.12

Discrimination is proven, not measured: each mutant of the reference must leave the per-element bound on at least half
of the elements it touches (elements whose float64 output it changes). Measured shares (the least over the cases / T0
values a mutant is asserted on):
    conv0   x_lo part dropped (mfma-exposed, the dc utterance)               0.562
            scsh of utterance b + 1 (every case and T0)                      0.874
            statistics without the last frame (mfma-tile, T0 = 17)           0.941
            unbiased variance (mfma-tile, T0 = 9)                            0.953
            eps omitted (mfma-exposed and f32-exposed, the quiet utterance)  0.999
            frames >= 4096 left out of the statistics (stats, T0 = 8193)     0.996
    posconv last tap dropped (every case)                                    0.876
            one (tap, channel) term dropped (every case)                     0.522
            window shifted by one frame (every case)                         0.976
            bias[n + 1] (every case)                                         0.959
            group g + 1's weights (every case with G > 1)                    0.975
    gate    bias[2] omitted (every case)                                     0.822
            cst[h + 1] (every case with H > 1)                               0.853
            the two sums swapped (every case)                                1.000
            head h + 1's slice of x (every case with H > 1)                  0.998
            output written [B S][H] (every case with H > 1)                  0.995
The last-tap mutant is skipped where S < kp / 2 (that tap then meets only padding), scsh of the next utterance where
T0 = 1 (one frame: z is beta for every utterance). One dropped term, the centre tap's channel 5, per case (Cg x kp):
16x8 0.945, 16x16 0.815, 32x12 0.739, 48x8 0.913, 48x128 0.522, 64x2 0.848, 64x128 0.559. The 64 x 128 case draws its
frame scales from 2^-1 .. 2^1 (helpers.POSCONV_FS_MAX): over 2^-2 .. 2^2 one term of K = 8192 from a quiet frame in a
window that always holds loud ones is below the bf16 output's half ulp, and the share was 0.47 - 0.50 whichever term
was dropped.
"""
import torch

import helpers as H

F = torch.nn.functional


def _share(ref, bound, mut, sel=None):
    """Share of the elements mutant output `mut` changes (within sel) at which it leaves `bound` around `ref`."""
    touched = mut != ref
    if sel is not None:
        touched = touched & sel
    assert touched.any()
    return ((mut - ref).abs() > bound)[touched].float().mean().item(), touched.float().mean().item()


def _least(d, k, v):
    d[k] = min(d.get(k, 1.0), v)


def _conv0_mutant(r, path, sc, sh, sel=None):
    m = H.conv0_out64(r.y, r.ya, sc, sh)
    return _share(r.ref, H.conv0_bound(r, path), m.ref, sel)[0]


def test_conv0_cost_and_mutants():
    E = {"conv0_f32": 0.0, "conv0_split": 0.0}
    least = {}
    for cid, path, C, T0s, kinds in H.CONV0_CASES:
        w, gamma, beta = H.conv0_params(C)
        for T0 in T0s:
            wave = H.conv0_wave(kinds, T0)
            assert wave.shape == (len(kinds), (T0 - 1) * 5 + 13)
            r = H.conv0_ref64(wave, w, gamma, beta)
            assert r.ref.shape == (len(kinds), T0, C) and (r.s > 0).all()
            # ---- E: both kernels' arithmetic against float64
            sc32, sh32 = H.conv0_scsh32(r.y, gamma, beta)
            e32 = ((H.conv0_emulate_apply(wave, w, sc32, sh32).double() - r.z).abs() / (H.U24 * r.s)).max().item()
            esp = ((H.conv0_emulate_mfma(wave, w, sc32, sh32).double() - r.z).abs() / (H.U18 * r.s)).max().item()
            E["conv0_f32"], E["conv0_split"] = max(E["conv0_f32"], e32), max(E["conv0_split"], esp)
            # ---- mutants
            if T0 > 1:      # one frame: var = 0 and y = mean, so every utterance's z is beta
                _least(least, "scsh_next", _conv0_mutant(r, path, r.sc.roll(-1, 0), r.sh.roll(-1, 0)))
            if cid == "mfma-tile" and T0 == 17:
                _, _, sc, sh = H.conv0_affine64(r.y[:, :-1], gamma, beta)
                _least(least, "stats_last_frame", _conv0_mutant(r, path, sc, sh))
            if cid == "mfma-tile" and T0 == 9:
                _, _, sc, sh = H.conv0_affine64(r.y, gamma, beta, unbiased=True)
                _least(least, "unbiased_var", _conv0_mutant(r, path, sc, sh))
            if cid == "stats" and T0 == 8193:
                _, _, sc, sh = H.conv0_affine64(r.y[:, :4096], gamma, beta)
                _least(least, "stats_first_block", _conv0_mutant(r, path, sc, sh))
            if kinds == H.CONV0_EXPOSED:
                quiet = torch.zeros_like(r.ref, dtype=torch.bool)
                quiet[kinds.index("quiet")] = True
                _, _, sc, sh = H.conv0_affine64(r.y, gamma, beta, eps=1e-30)   # 0 would divide the silent one by 0
                _least(least, "eps_omitted", _conv0_mutant(r, path, sc, sh, quiet))
            if cid == "mfma-exposed":
                b = kinds.index("dc")
                lo = wave.double() - wave.to(torch.bfloat16).double()
                ylo, _ = H.conv0_terms64(lo, w)
                m = H.conv0_out64(r.y - ylo, r.ya, r.sc, r.sh)
                dc = torch.zeros_like(r.ref, dtype=torch.bool)
                dc[b] = True
                _least(least, "xlo_dropped", _share(r.ref, H.conv0_bound(r, path), m.ref, dc)[0])
                # and the emulation itself without that part misses the bound there, with it it holds everywhere
                bound = H.conv0_bound(r, path)
                full = F.gelu(H.conv0_emulate_mfma(wave, w, sc32, sh32).double())
                part = F.gelu(H.conv0_emulate_mfma(wave, w, sc32, sh32, drop_xlo=True).double())
                assert ((full - r.ref).abs() <= bound).all()
                assert ((part - r.ref).abs() > bound)[b].float().mean().item() >= 0.5
    print(f"\nFRONTREF conv0: E f32 {E['conv0_f32']:.2f} split {E['conv0_split']:.2f}; least caught share per mutant "
          + ", ".join(f"{k} {v:.3f}" for k, v in least.items()))
    assert set(least) == {"scsh_next", "stats_last_frame", "unbiased_var", "stats_first_block", "eps_omitted",
                          "xlo_dropped"}
    for k, e in E.items():
        assert e <= H.FRONT_E[k] <= 1.1 * e + H.FRONT_E_FLOOR, (k, e)
    for k, v in least.items():
        assert v >= 0.5, f"conv0 mutant {k} leaves the bound on only {v:.3f} of its elements"


def test_posconv_cost_and_mutants():
    Emax, least, term = 0.0, {}, {}
    for case in H.POSCONV_CASES:
        Cg, kp, G, B, S = case
        x, w, bias = H.posconv_operands(*case)
        E_, K = G * Cg, kp * Cg
        r = H.posconv_ref64(x, w, bias, G)
        assert r.ref.shape == (B, S, E_) and r.full.shape == (B, S + 1, E_) and (r.s > 0).all()
        cols = H.posconv_im2col(x.double(), w.double(), G)
        y64 = torch.cat([A @ Wg.t() for A, Wg in cols], 1) + bias.double()
        assert ((y64.view(B, S, E_) - r.y).abs() <= 1e-12 * r.s).all(), "the im2col operands are the convolution's"
        e = ((H.posconv_emulate(x, w, bias, G).double() - r.y).abs() / (H.U24 * r.s)).max().item()
        Emax = max(Emax, e)
        bound = H.posconv_bound(r)

        def share(dy=None, y=None):
            m = H.posconv_out64(r.y + dy.view(B, S, E_) if y is None else y, r.s)
            return _share(r.ref, bound, m.ref)[0]

        k1 = K // 2 + 5
        if S >= kp // 2:    # in a shorter utterance the last tap meets only padding
            _least(least, "last_tap", share(-torch.cat([A[:, -Cg:] @ Wg[:, -Cg:].t() for A, Wg in cols], 1)))
        term[case] = share(-torch.cat([torch.outer(A[:, k1], Wg[:, k1]) for A, Wg in cols], 1))
        _least(least, "shift", share(y=r.full[:, 1:]))
        bd = bias.double()
        _least(least, "bias_next", share((bd.roll(-1) - bd)[None, :].expand(B * S, E_)))
        if G > 1:
            nxt = torch.cat([A @ cols[(g + 1) % G][1].t() for g, (A, _) in enumerate(cols)], 1) + bd
            _least(least, "group_next", share(y=nxt.view(B, S, E_)))
    print(f"\nFRONTREF posconv: E {Emax:.2f}; least caught share per mutant "
          + ", ".join(f"{k} {v:.3f}" for k, v in least.items()) + "; one term dropped, per case: "
          + ", ".join(f"{c[0]}x{c[1]} {v:.3f}" for c, v in term.items()))
    assert Emax <= H.FRONT_E["posconv"] <= 1.1 * Emax + H.FRONT_E_FLOOR, Emax
    for k, v in least.items():
        assert v >= 0.5, f"posconv mutant {k} leaves the bound on only {v:.3f} of its elements"
    assert all(v >= 0.5 for v in term.values()), term


def test_gate_cost_and_mutants():
    Emax, least = 0.0, {}
    for case in H.GATE_CASES:
        dt, B, S, Hh, dh = case
        x, W, bias, cst = H.gate_operands(*case)
        r = H.gate_ref64(x, W, bias, cst, B, S, Hh)
        assert r.ref.shape == (B, Hh, S)
        pa, pb, g32 = H.gate_emulate(x, W, bias, cst, B, S, Hh)
        e = max(((pa.double() - r.pa).abs() / (H.U24 * r.sa)).max().item(),
                ((pb.double() - r.pb).abs() / (H.U24 * r.sb)).max().item())
        Emax = max(Emax, e)
        bound = H.gate_bound(r)
        assert ((g32.double() - r.ref).abs() <= bound).all(), "the fp32 evaluation itself stays inside the bound"
        xh, Wd, bd = x.double().view(B, S, Hh, dh), W.double(), bias.double()
        p = xh @ Wd.t() + bd
        sp = xh.abs() @ Wd.abs().t() + bd.abs()

        def share(m):
            return _share(r.ref, bound, m)[0]

        b2 = bd.clone()
        b2[2] = 0.0
        _least(least, "bias_omitted", share(H.gate_out64(xh @ Wd.t() + b2, sp, cst).ref))
        _least(least, "sums_swapped", share(H.gate_out64(p.roll(4, -1), sp, cst).ref))
        if Hh > 1:
            _least(least, "cst_next", share(H.gate_out64(p, sp, cst.roll(-1)).ref))
            _least(least, "head_next", share(H.gate_out64(p.roll(-1, 2), sp, cst).ref))
            _least(least, "token_major", share(r.ref.transpose(1, 2).reshape(B, Hh, S)))
    print(f"\nFRONTREF gate: E {Emax:.2f}; least caught share per mutant "
          + ", ".join(f"{k} {v:.3f}" for k, v in least.items()))
    assert len(least) == 5
    assert Emax <= H.FRONT_E["gate"] <= 1.1 * Emax + H.FRONT_E_FLOOR, Emax
    for k, v in least.items():
        assert v >= 0.5, f"gate mutant {k} leaves the bound on only {v:.3f} of its elements"


def test_constants_and_tables():
    for k, e in H.FRONT_E.items():
        assert H.FRONT_C[k] == 8.0 * e and H.FRONT_C[k] <= 64.0
    # the exact half ulp: 1.0 rounds within 2^-8 of a value in [1, 2), 0.99 within 2^-9; nothing is added at 0
    t = torch.tensor([1.0, 0.99, 0.0, -3.0], dtype=torch.float64)
    assert H.bf16_round_bound(t, torch.zeros_like(t)).tolist() == [2.0 ** -8, 2.0 ** -9, 0.0, 2.0 ** -7]
    v = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3
    assert ((v.to(torch.bfloat16).double() - v).abs() <= H.bf16_round_bound(v, torch.zeros_like(v))).all()
    # every mechanism the tables are there for
    by = {c[0]: c for c in H.CONV0_CASES}
    assert all(c[2] % 512 == 0 for c in H.CONV0_CASES if c[1] == "mfma")
    assert all(c[2] % 512 for c in H.CONV0_CASES if c[1] == "bf16")
    assert by["mfma-z1"][2] == 1024 and by["f32-loop"][2] == 1024 and by["stats"][3] == (4096, 4097, 8193)
    assert all(len(set(c[4])) == len(c[4]) > 1 for c in H.CONV0_CASES)
    assert {c[0] // 16 for c in H.POSCONV_CASES} == {1, 2, 3, 4}
    assert all((c[0] * c[1]) % 128 == 0 and c[1] % 2 == 0 for c in H.POSCONV_CASES)
    assert {c[4] for c in H.POSCONV_CASES} >= {1, 255, 256, 257}
    assert {(c[0] * c[1]) // 128 for c in H.POSCONV_CASES} >= {1, 2, 3, 48, 64}
    assert all(c[4] % 8 == 0 and c[4] <= 64 for c in H.GATE_CASES)
