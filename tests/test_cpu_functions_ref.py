"""What tests/test_gpu_functions.py may ask of the autograd Functions (fddm_hip/functions.py), settled from the float64
restatements of tests/helpers.py alone, before any Function runs on a device.

References: helpers.head_ref64 / linear_fn_ref64 / lfd_fn_ref64 / cond_fn_ref64 are plain torch graphs; their KL term is
the oracle's (O.kl_term, an fp32 evaluation: loss within 1e-5, its closed-form gradient within the KL's own error scale),
their L_fd is O.lfd_loss itself on float64 leaves, their text embedding and decoder conditioning are the oracle's
expressions (softmax @ W^T; O.decoder_forward's first lines).

Bounds: |got - ref| <= C u companion per element. The same graphs evaluated in fp32 stay inside the bound at C = 64
(what fp32 arithmetic costs, FNREF "fp32 eval" lines), and every wiring mutant leaves it at C = 64 on at least half of
the elements of at least one checked gradient (FNREF "caught" lines):
  u = 2^-24: all seven mutants, on the composite with all four consumers of the logits (helpers.HEAD_ALL).
  u = 2^-9 (bf16 mode, where the logits gradient itself is not observable): the three dropped consumers on the head's
  bias gradient of the same composite; the two KL-scale mutants on the head's input gradient of the KL-alone case
  (next to other consumers 64 x 2^-9 = 1/8 of the whole companion hides a 0.625 share of the smallest part: there they
  are caught on 40 - 50 % of x only; the device test allows min(64, 8 E) units, which is tighter wherever E < 8).
The loss coefficients are balanced (every consumer's median share of the logits gradient's companion within 4x of every
other's, in every case), and the L_fd inputs keep every column's batch standard deviation within 0.25 of the median's.
"""
import pytest
import torch

import helpers as H
from oracle import fddm_oracle as O

C64 = 64.0


def _caught(ref, mut, u):
    """{gradient: share of its elements on which the mutant leaves the C = 64 bound}"""
    out = {}
    for k, g in ref.g.items():
        if g is None:
            continue
        gm = mut.g[k] if mut.g[k] is not None else torch.zeros_like(g)
        out[k] = ((gm - g).abs() > C64 * u * ref.m[k]).float().mean().item()
    return out


@pytest.mark.parametrize("V", H.HEAD_V)
@pytest.mark.parametrize("masked", [True, False])
def test_kl_restatement_is_the_oracles(V, masked):
    i = H.head_inputs(V, masked)
    r = H.head_ref64(V, masked, (("kl", 1.0),))
    logits = (i.x.double() @ i.hw.double().t() + i.hb.double()).view(H.HEAD_B, H.HEAD_L, V)
    loss, dz = O.kl_term(logits.float(), i.xt, i.x0, i.t, i.mask, i.betas)
    assert abs(float(loss) - r.loss) <= 1e-5 * abs(r.loss)
    e = H.fn_excess(dz.view(-1, V), r.g["dl"], r.m["dl"], H.U24)
    print(f"\nFNREF oracle kl dz V={V} masked={masked}: {e:.2f} units of 2^-24 s")
    assert e <= C64


def test_text_and_lfd_restatements_are_the_oracles():
    V = H.HEAD_V[0]
    i = H.head_inputs(V, False)
    r = H.head_ref64(V, False, (("text", 1.0),))
    logits = i.x.double() @ i.hw.double().t() + i.hb.double()
    z = torch.nn.functional.linear(torch.softmax(logits, -1), i.tw.double())       # models/projection.py:41-47
    assert abs(float((z * i.Rz.double()).sum()) - r.loss) <= 1e-12 * abs(r.loss)
    za, zb = H.lfd_fn_inputs()
    r = H.lfd_fn_ref64(1.0)
    assert abs(float(O.lfd_loss(za.double(), zb.double(), H.LFD_FN_LAM, H.LN_EPS)) - r.loss) <= 1e-12 * abs(r.loss)
    assert abs(float(O.lfd_loss(za, zb, H.LFD_FN_LAM, H.LN_EPS)) - r.loss) <= 1e-4 * abs(r.loss)
    r37 = H.lfd_fn_ref64(H.LFD_FN_G[1])
    for k in r.g:
        assert torch.allclose(r37.g[k], H.LFD_FN_G[1] * r.g[k], rtol=1e-12, atol=0.0)


def test_cond_restatement_is_the_oracles_conditioning():
    """x of cond_fn_ref64 against the first lines of O.decoder_forward (fp32: embedding, time MLP, time_proj)."""
    NL, d = 0, 128
    i = H.cond_fn_inputs(NL, d)
    r = H.cond_fn_ref64(NL, d, "gbuf")
    p = i.params
    te = O.time_embedding(i.t, d)
    te = torch.nn.functional.linear(torch.nn.functional.silu(torch.nn.functional.linear(te, p[0], p[1])), p[2], p[3])
    x = torch.nn.functional.embedding(i.xt, i.E, padding_idx=0) + torch.nn.functional.linear(te, p[4], p[5])[:, None]
    H.close(x.reshape(-1, d), r.x, rtol=1e-5, what="conditioning x")


@pytest.mark.parametrize("V", H.HEAD_V)
def test_head_fp32_evaluation_stays_inside_the_bound(V):
    worst = {}
    for name in H.HEAD_CASES:
        for masked in (True, False):
            r = H.head_case_ref(name, V, masked)
            r32 = H.head_ref64(V, masked, H.HEAD_CASES[name], dtype=torch.float32)
            for k, g in r.g.items():
                if g is not None:
                    worst[k] = max(worst.get(k, 0.0), H.fn_excess(r32.g[k], g, r.m[k], H.U24))
    print(f"\nFNREF fp32 eval head V={V}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= C64, worst


@pytest.mark.parametrize("V", H.HEAD_V)
@pytest.mark.parametrize("masked", [True, False])
def test_head_mutants_leave_the_bound(V, masked):
    ref = H.head_ref64(V, masked, H.HEAD_ALL)
    for mut in H.HEAD_MUTANTS:
        c = _caught(ref, H.head_ref64(V, masked, H.HEAD_ALL, mut=mut), H.U24)
        print(f"\nFNREF caught u=2^-24 V={V} masked={masked} {mut}: " + ", ".join(f"{k} {v:.2f}" for k, v in c.items()), end="")
        assert max(c.values()) >= 0.5, (mut, c)
    for mut in ("no_expand", "no_dense", "no_text"):
        c = _caught(ref, H.head_ref64(V, masked, H.HEAD_ALL, mut=mut), H.U9)
        print(f"\nFNREF caught u=2^-9 V={V} masked={masked} {mut}: " + ", ".join(f"{k} {v:.2f}" for k, v in c.items()), end="")
        assert c["hb"] >= 0.5, (mut, c)
    alone = H.head_case_ref("kl_g", V, masked)
    for mut in ("kl_unscaled", "kl_twice"):
        c = _caught(alone, H.head_ref64(V, masked, H.HEAD_CASES["kl_g"], mut=mut), H.U9)
        print(f"\nFNREF caught u=2^-9 V={V} masked={masked} kl_g {mut}: " + ", ".join(f"{k} {v:.2f}" for k, v in c.items()), end="")
        assert c["x"] >= 0.5, (mut, c)


@pytest.mark.parametrize("V", H.HEAD_V)
@pytest.mark.parametrize("masked", [True, False])
def test_head_loss_coefficients_are_balanced(V, masked):
    """Every consumer's share of m_dl has its median within 4x of every other's, in the composite and in every case
    (over the rows the consumer reaches: the masked rows of the KL and the rows past a slice carry none of it)."""
    for name, cons in list(H.HEAD_CASES.items()) + [("all", H.HEAD_ALL)]:
        r = H.head_ref64(V, masked, cons) if name == "all" else H.head_case_ref(name, V, masked)
        med = {k: v[v.sum(1) > 0].median().item() for k, v in r.shares.items()}
        assert max(med.values()) <= 4.0 * min(med.values()), (name, med)


def test_linear_fp32_evaluation_and_mutant():
    for si in range(len(H.LINEAR_SHAPES)):
        for bias in (False, True):
            r = H.linear_fn_ref64(si, bias)
            r32 = H.linear_fn_ref64(si, bias, dtype=torch.float32)
            e = {k: H.fn_excess(r32.g[k], g, r.m[k], H.U24) for k, g in r.g.items() if g is not None}
            print(f"\nFNREF fp32 eval linear {si} bias={bias}: " + ", ".join(f"{k} {v:.2f}" for k, v in e.items()), end="")
            assert max(e.values()) <= C64, e
        r = H.linear_fn_ref64(si, True)
        c = _caught(r, H.linear_fn_ref64(si, True, mut="b_overwrite"), H.U24)
        assert c["b"] >= 0.5, c
        # 2^-9: the overwritten sum differs by the first pass's column sum, 45 randn against 64 / 512 of 90 |randn|:
        # caught on the columns where the first pass's sum is not small, reported, not asserted
        print(f"\nFNREF caught linear {si} b_overwrite: u=2^-24 {c['b']:.2f}, u=2^-9 "
              f"{_caught(r, H.linear_fn_ref64(si, True, mut='b_overwrite'), H.U9)['b']:.2f}")


def test_lfd_inputs_fp32_evaluation_and_mutant():
    for z in H.lfd_fn_inputs():
        sd = z.double().std(0, unbiased=False)
        assert sd.min() >= 0.25 * sd.median(), (sd.min().item(), sd.median().item())
    for g in H.LFD_FN_G:
        r = H.lfd_fn_ref64(g)
        r32 = H.lfd_fn_ref64(g, dtype=torch.float32)
        e = {k: H.fn_excess(r32.g[k], v, r.m[k], H.U24) for k, v in r.g.items()}
        print(f"\nFNREF fp32 eval lfd g={g}: " + ", ".join(f"{k} {v:.2f}" for k, v in e.items()), end="")
        assert max(e.values()) <= C64, e
        for u in (H.U24, H.U9):
            c = _caught(r, H.lfd_fn_ref64(g, mut="nt_once"), u)
            assert min(c.values()) >= 0.5, c


def test_cond_fp32_evaluation_stays_inside_the_bound():
    for NL in H.COND_FN_NL:
        for d in H.COND_FN_D:
            for mode in H.COND_FN_MODES:
                if NL == 0 and mode != "gbuf":
                    continue
                r = H.cond_fn_ref64(NL, d, mode)
                r32 = H.cond_fn_ref64(NL, d, mode, dtype=torch.float32)
                assert {k for k, v in r.g.items() if v is None} == {k for k, v in r.m.items() if v is None}
                e = {k: H.fn_excess(r32.g[k], g, r.m[k], H.U24) for k, g in r.g.items() if g is not None}
                print(f"\nFNREF fp32 eval cond NL={NL} d={d} {mode}: worst {max(e.values()):.2f}", end="")
                assert max(e.values()) <= C64, e


def test_stored_constants():
    for k, e in H.FN_E.items():
        assert e >= H.FN_E_FLOOR and H.fn_c(*k) == min(64.0, 8.0 * e), k
    assert len(H.linear_fn_cases()) == len(set(H.linear_fn_cases()))
