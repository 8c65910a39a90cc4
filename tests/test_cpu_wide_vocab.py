"""The CPU side of the streamed ("wide") row kernels: their declarations in include/fddm_hip.h as the wrappers of
fddm_hip/ops.py pass them, and the fp32-oracle-against-float64 constants the GPU test's bounds are built from
(tests/wide_cases.py), re-measured on that test's inputs so that a changed input set cannot outrun its bound."""
import ctypes

import pytest

import wide_cases as W

P, L_, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
WIDE_DECLS = {
    # logits, xt, x0, t, betas, kl_tok, N, L, V, stream
    "fddm_kl_fwd_wide": [P, P, P, P, P, P, L_, L_, L_, P],
    # logits, xt, x0, t, betas, mask, kl_tok, dz, dz_dtype, N, L, V, stream
    "fddm_kl_fused_wide": [P, P, P, P, P, P, P, P, I, L_, L_, L_, P],
    # x, y, out_dtype, N, V, stream
    "fddm_softmax_rows_wide": [P, P, I, L_, L_, P],
    # y, dy, dz, dtype, N, V, accumulate, stream
    "fddm_softmax_bwd_rows_wide": [P, P, P, I, L_, L_, I, P],
    # y, dy, add, out, N, V, stream
    "fddm_softmax_bwd_add_bf16_wide": [P, P, P, P, L_, L_, P],
}
RESIDENT = {"fddm_kl_fwd_wide": "fddm_kl_fwd", "fddm_kl_fused_wide": "fddm_kl_fused",
            "fddm_softmax_rows_wide": "fddm_softmax_rows", "fddm_softmax_bwd_rows_wide": "fddm_softmax_bwd_rows",
            "fddm_softmax_bwd_add_bf16_wide": "fddm_softmax_bwd_add_bf16"}


def test_wide_symbols_are_declared_with_the_wrappers_argument_types():
    from fddm_hip._lib import parse_header
    decls = parse_header()
    for name, args in WIDE_DECLS.items():
        assert name in decls, f"{name} is not declared in include/fddm_hip.h"
        res, got = decls[name]
        assert res is ctypes.c_int and got == args, f"{name}: {got}"
        assert got == decls[RESIDENT[name]][1], f"{name} takes the arguments of {RESIDENT[name]}"


def test_wide_limit_sits_beside_the_resident_limits():
    """ops.WIDE_MAX_V = 2^24, the last V at which float(V) is exact, above every resident limit."""
    import numpy as np
    from fddm_hip import ops
    assert ops.WIDE_MAX_V == 1 << 24
    assert float(np.float32(ops.WIDE_MAX_V)) == ops.WIDE_MAX_V and float(np.float32(ops.WIDE_MAX_V + 1)) != ops.WIDE_MAX_V + 1
    assert ops.WIDE_MAX_V > max(ops.KL_VEC_MAX_V, ops.KL_FUSED_MAX_V, ops.SOFTMAX_MAX_V, ops.SOFTMAX_ADD_MAX_V)


def test_bounds_stay_under_the_hard_cap_and_cover_every_tested_vocabulary():
    for V in W.WIDE_V:
        assert 8.0 * W.ORACLE_C[V] <= W.CAP_GRAD, f"V={V}: 8 x the oracle's error passes the hard cap"
        assert V in W.ORACLE_A and V in W.ORACLE_R
    assert {2 * W.WIDE_C - 1, 2 * W.WIDE_C, 2 * W.WIDE_C + 4} <= set(W.WIDE_V)
    from fddm_hip import _lib
    assert _lib.lib().fddm_wide_chunk() == W.WIDE_C, "the tests' chunk size is the kernels' (a host call, no GPU)"


@pytest.mark.parametrize("V", W.WIDE_V)
def test_oracle_constants_are_reproduced_on_the_gpu_tests_inputs(V):
    """max |oracle32 - ref64| / s_k and the fp32 formula's per-token errors over the masked and the unmasked case of V:
    within 10 % of the constants in tests/wide_cases.py; the cases' preconditions hold."""
    got = [W.oracle_errors(W.kl_case(V, masked)) for masked in (True, False)]
    for masked in (True, False):
        W.check_preconditions(W.kl_case(V, masked))
    for i, (name, table) in enumerate((("ORACLE_C", W.ORACLE_C), ("ORACLE_A", W.ORACLE_A), ("ORACLE_R", W.ORACLE_R))):
        m = max(g_[i] for g_ in got)
        print(f"V={V} {name}: measured {m:.4e}, stored {table[V]:.4e}")
        assert abs(m - table[V]) <= 0.1 * table[V], f"V={V} {name}: measured {m:.4e}, stored {table[V]:.4e}"
