"""What tests/test_gpu_gemm.py may ask of the GEMM kernels, settled from the reference alone before any kernel runs.

For every case of helpers.gemm_cases() and helpers.CONV_CASES the product is evaluated in fp32 the way the kernels
order it (helpers.gemm_eval_fp32: 64-wide K tiles added in order, split-K slices added in order, then alpha, bias, the
previous C) and compared with float64 in units of 2^-24 s, s = |alpha| |A| |B|^T + |bias| + |c_old|. The maximum E per
compute dtype (the GEMM cases and the convolutions apart) must stay below helpers.GEMM_E, and the kernels' allowance
GEMM_C = 8 E below the hard cap of 64 units.

Discrimination is proven, not measured: in every case each mutant of the reference — the last K element dropped, bias[n + 1]
read for bias[n], alpha = 1 where alpha != 1, one 32-wide K slice dropped — must leave the per-element bound on at least
half of the elements it touches. An element counts as caught when any output the GPU test compares (the stored y, the
GELU / dGELU output) leaves its bound there."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import fddm_oracle as O

CASES = H.gemm_cases()
FAMS = ("small", "128", "256", "big")
SEED, STREAM = 7, 3


def _prod(c, cache):
    key = (c["M"], c["N"], c["K"], c["dt"], c["a_f32"])
    if key not in cache:
        cache.clear()            # cases of one shape are consecutive enough; keep one product in memory
        A, B = H.gemm_logical64(H.gemm_operands(*key), c["dt"])
        cache[key] = (A, B, A @ B.t(), A.abs() @ B.abs().t())
    return cache[key]


def _ref(c, A, B, P, S, ops_, alpha=None, bias=None, dP=None):
    """Reference of case c, optionally mutated: another alpha, another bias vector, P + dP."""
    al = float(np.float32(c["alpha"] if alpha is None else alpha))
    b = (ops_["bias"] if c["bias"] else None) if bias is None else bias
    keep = None
    if c["p"]:
        keep = O.dropout_keep(SEED, STREAM, c["M"] * c["N"], c["p"]).view(c["M"], c["N"])
    pre = ops_["pre"].to(torch.bfloat16 if c["out"] == "bf16" else torch.float32) if c["epi"] == H.EPI_DGELU else None
    return H.gemm_ref64(A, B, bias=b, alpha=al, c_old=ops_["c_old"] if c["epi"] == H.EPI_ACC else None, epi=c["epi"],
                        pre=pre, keep=keep, drop_p=c["p"], prod=(P if dP is None else P + dP, S))


def _caught(c, r, m, C):
    """Elements at which the mutated reference m leaves the bounds around r on an output the GPU test compares."""
    bf = c["out"] == "bf16"
    gabs = H.GEMM_GELU_BF16OUT_ABS if (c["expect"] == "256" and c["epi"] == H.EPI_GELU_ONLY) else H.GEMM_GELU_ABS
    hit = torch.zeros_like(r.y, dtype=torch.bool)
    if c["epi"] in (H.EPI_STORE, H.EPI_ACC, H.EPI_GELU):
        ref, b = H.gemm_bound(r, "y", C, bf)
        hit |= (m.y - ref).abs() > b
    if r.act is not None:
        ref, b = H.gemm_bound(r, "act", C, bf, gabs)
        hit |= (m.act - ref).abs() > b
    return hit


@pytest.mark.parametrize("fam", FAMS)
def test_fp32_cost_and_mutants(fam):
    cache, Emax, seen = {}, {"f32": 0.0, "bf16": 0.0}, set()
    worst = {}
    for c in (x for x in CASES if x["fam"] == fam):
        ops_ = H.gemm_operands(c["M"], c["N"], c["K"], c["dt"], c["a_f32"])
        A, B, P, S = _prod(c, cache)
        C = H.GEMM_C[c["dt"]]
        r = _ref(c, A, B, P, S, ops_)
        # ---- E: fp32 in the kernels' order against float64
        key = (c["M"], c["N"], c["K"], c["dt"], c["a_f32"], c["alpha"], c["bias"], c["epi"] == H.EPI_ACC, c["ksplit"])
        if key not in seen:
            seen.add(key)
            y32 = H.gemm_eval_fp32(A.float(), B.float(), bias=ops_["bias"] if c["bias"] else None, alpha=c["alpha"],
                                   c_old=ops_["c_old"] if c["epi"] == H.EPI_ACC else None, ksplit=c["ksplit"])
            yy = H.gemm_ref64(A, B, bias=ops_["bias"] if c["bias"] else None, alpha=float(np.float32(c["alpha"])),
                              c_old=ops_["c_old"] if c["epi"] == H.EPI_ACC else None, prod=(P, S))
            e = ((y32.double() - yy.y).abs() / (H.U24 * yy.s)).max().item()
            Emax[c["dt"]] = max(Emax[c["dt"]], e)
        # ---- mutants
        al = float(np.float32(c["alpha"]))
        K = c["K"]
        k0 = 32 if K >= 96 else 0
        muts = {"last_k": _ref(c, A, B, P, S, ops_, dP=-torch.outer(A[:, -1], B[:, -1])),
                "k_slice": _ref(c, A, B, P, S, ops_, dP=-(A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].t()))}
        if c["bias"]:
            muts["bias_next"] = _ref(c, A, B, P, S, ops_, bias=torch.roll(ops_["bias"], -1))
        if c["alpha"] != 1.0:
            muts["alpha_one"] = _ref(c, A, B, P, S, ops_, alpha=1.0)
        for name, m in muts.items():
            touched = m.y != r.y
            assert touched.float().mean().item() > 0.9, (c["id"], name)
            frac = _caught(c, r, m, C)[touched].float().mean().item()
            worst[name] = min(worst.get(name, 1.0), frac)
            assert frac >= 0.5, f"{c['id']}: mutant {name} leaves the bound on only {frac:.3f} of its elements"
    print(f"\nGEMMREF family {fam}: E f32 {Emax['f32']:.2f} bf16 {Emax['bf16']:.2f}; least caught fraction per mutant "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for dt in Emax:
        assert Emax[dt] <= H.GEMM_E[dt], (fam, dt, Emax[dt])


@pytest.mark.parametrize("name,dt", [("small", "f32"), ("small", "bf16"), ("256", "bf16"), ("big", "bf16")])
def test_conv_fp32_cost(name, dt):
    x, w, b = H.conv_operands(name, dt)
    y, s = H.conv_ref(name, x, w, b)
    g = H.CONV_CASES[name]
    cols = [H.gemm_eval_fp32(A.float(), B.float(), bias=b[z * g["N"]:(z + 1) * g["N"]])
            for z, (A, B) in enumerate(H.conv_im2col(name, x, w))]
    y32 = torch.cat(cols, dim=1)
    y64 = torch.cat([A.double() @ B.double().t() for A, B in H.conv_im2col(name, x, w)], dim=1) + b.double()
    assert ((y64 - y).abs() <= 1e-12 * s).all(), "the im2col operands are the convolution's"
    e = ((y32.double() - y).abs() / (H.U24 * s)).max().item()
    print(f"\nGEMMREF conv {name} {dt}: E {e:.2f}")
    assert e <= H.GEMM_E["conv-" + dt]
    last = (g["Tout"] - 1) * g["stride"] - g["cpad"] + g["taps"] - 1
    assert (g["cpad"] > 0) == (last >= g["Tin"]), "padded cases reach past both ends, unpadded ones end inside"


def test_constants_and_split_plans():
    for k in H.GEMM_E:
        assert H.GEMM_C[k] == 8.0 * H.GEMM_E[k] and H.GEMM_C[k] <= 64.0
    for dt in ("f32", "bf16"):   # 1096 = 576 + 520, the second slice ends on a partial K-step of both dtypes
        assert H.small_splits(136, 72, 1096, dt) == (2, 576) and (1096 - 576) % 64 == 8
    assert H.g128_splits(200, 136, 4160) == (2, 2112) and H.g128_splits(200, 136, 4100) == (2, 2112)
    assert (4100 - 2112) % 64 == 4
    split = [c for c in CASES if c["splits"] > 1]
    assert {c["expect"] for c in split} == {"small", "128"}
    assert all(c["splits"] == 2 for c in split if c["expect"] == c["fam"])
    # biased calls that the ring kernel would accumulate must leave it: 8 slices of 576 on the register-staged kernel
    moved = [c for c in CASES if c["fam"] == "128" and c["expect"] == "small"]
    assert moved and all(c["bias"] and (c["epi"] == H.EPI_ACC or c["K"] >= 4096) for c in moved)
    assert all(c["splits"] == (8 if c["K"] >= 4096 else 1) for c in moved)
    assert not any(c["bias"] and c["epi"] == H.EPI_ACC for c in CASES if c["expect"] == "128")
    # every (family, layout, epilogue) meets both a bias and none; the families that take alpha meet all three
    # (the small family per epilogue, the 128 family per layout and epilogue)
    groups = {}
    for c in CASES:
        if c["fam"] == "128":
            groups.setdefault(("128", c["a_kc"], c["b_kc"], c["epi"]), []).append(c)
        elif c["fam"] == "small" and not c["a_f32"]:
            groups.setdefault(("small", "epi", c["epi"]), []).append(c)
    for k, v in groups.items():
        assert {c["alpha"] for c in v} == set(H.GEMM_ALPHAS), k
        if not (k[0] == "128" and k[3] == H.EPI_ACC):      # the ring kernel's accumulate epilogue takes no bias
            assert {c["bias"] for c in v} == {True, False}, k


def test_rope_bwd_ref_is_the_oracles_transpose():
    L, d, M = 100, 128, 200
    cos, sin = O.rope_cos_sin(L, O.rope_inv_freq(d))
    P = torch.randn(M, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    xr = torch.zeros(M // L, L, d, dtype=torch.float64, requires_grad=True)
    O.rope_apply(xr, cos.double(), sin.double()).backward(P.view(M // L, L, d))
    assert torch.equal(H.rope_bwd_ref64(P, cos, sin, L), xr.grad.view(M, d))
