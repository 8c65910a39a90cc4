"""Inputs, float64 references and bounds of the streamed ("wide") KL kernels' tests, shared by
tests/test_gpu_kl_softmax_wide.py (the kernels), tests/test_gpu_wide_vocab_step.py (the no-grad route) and
tests/test_cpu_wide_vocab.py (which re-measures, on the CPU, the fp32 oracle's own error the bounds are built from).
Nothing here touches a GPU.

The bounds, per V (how they were set: on the CPU, from these inputs, before any kernel ran):
  * gradient: |dz - ref| <= C_GRAD[V] s_k with C_GRAD[V] = min(8 x ORACLE_C[V], 1e-4); ORACLE_C[V] is the largest
    |oracle32 - ref64| / s_k of the fp32 oracle (oracle.fddm_oracle.kl_term) over the masked and the unmasked case of
    that V. It grows with V (the row sums collect V roundings), which is why the constant of
    tests/test_gpu_kl_softmax.py (measured up to V = 32768) is not reused. The hard cap of that file stays: beyond
    1e-4 the kernel is wrong, not the tolerance narrow; every V of the list stays under it (largest: 4.8e-5).
  * per token: |kl_tok - ref| <= 8 (ORACLE_A[V] + ORACLE_R[V] |ref|): the fp32 evaluation of the oracle's formula
    (helpers.kl_term_ref64(dtype=float32)) against float64, absolute on the tokens with |ref| < 0.1 and relative on
    the others, as in that file.
"""
import functools

import torch

from helpers import kl_term_ref64
from oracle import fddm_oracle as O

TN = 200                        # diffusion steps; t covers 1 (beta_p = 0), 2, the middle and T
WIDE_C = 8192                   # elements per workgroup iteration of the streamed kernels (csrc/kl.hip WIDE_C)
SMALL_TOK = 0.1                 # the split between the absolute and the relative per-token measurement
CAP_GRAD = 1e-4

# 36, 2052: less than one chunk (also run against the resident kernels); 2 WIDE_C - 1, 2 WIDE_C, 2 WIDE_C + 4: the
# chunk edges (the last chunk one short of full, no partial chunk, one float4 in it); 16385: odd, the first V past the
# resident scalar limit; 32772: the first aligned V past the resident limit; 50257: odd, every second row unaligned;
# 65536: whole chunks only; 131076: sixteen chunks and one float4
WIDE_V = (36, 2052, 2 * WIDE_C - 1, 2 * WIDE_C, 16385, 2 * WIDE_C + 4, 32772, 50257, 65536, 131076)

# The draw of each V (logits, x0, x_t: generator seeds 1000 / 2000 / 3000 + V + SEED_STEP * SEED[V]). Whether a token's
# generic gradient discriminates depends on the drawn logits: where a token's KL is all but zero (x_t = x0 with P ~ Q, or
# t = 1 with the two special terms cancelling) the whole row's gradient cancels to ~1e-5 of its scale and cannot tell a
# wrong kernel from a right one. SEED[V] is the first draw, counted from 0, on which check_preconditions holds for the
# masked and the unmasked case; it was chosen from the float64 reference alone, before any kernel ran on the inputs.
SEED_STEP = 200000
SEED = {36: 0, 2052: 0, 16383: 3, 16384: 7, 16385: 3, 16388: 4, 32772: 0, 50257: 4, 65536: 0, 131076: 1}

# max |oracle32 - ref64| / s_k, and the fp32 formula's per-token absolute / relative error, measured on the CPU over
# kl_case(V, True) and kl_case(V, False) (tests/test_cpu_wide_vocab.py reproduces each within 10 %)
ORACLE_C = {36: 5.993e-7, 2052: 1.264e-6, 16383: 1.189e-6, 16384: 1.983e-6, 16385: 1.367e-6, 16388: 1.814e-6,
            32772: 2.740e-6, 50257: 3.320e-6, 65536: 2.814e-6, 131076: 6.003e-6}
ORACLE_A = {36: 1.342e-7, 2052: 1.207e-7, 16383: 1.160e-7, 16384: 7.963e-8, 16385: 6.136e-8, 16388: 1.114e-7,
            32772: 1.347e-7, 50257: 1.065e-7, 65536: 1.872e-7, 131076: 1.064e-7}
ORACLE_R = {36: 3.057e-7, 2052: 2.873e-7, 16383: 2.956e-7, 16384: 6.013e-7, 16385: 7.944e-7, 16388: 4.624e-7,
            32772: 1.035e-6, 50257: 1.594e-6, 65536: 1.118e-6, 131076: 5.363e-6}


def share_floor(V):
    """The least share of the generic elements of unmasked rows on which the criterion must discriminate: the bar of
    tests/test_gpu_kl_softmax.py below one chunk (measured 0.83 - 0.91 at V = 36 and 2052, whose few, large
    probabilities leave more elements near their own scale), 0.997 around two chunks (measured 0.9978 - 0.99997),
    0.999 from V = 32772 (measured 0.99949 - 1.00000)."""
    return 0.999 if V >= 32772 else 0.997 if V >= 2 * WIDE_C - 1 else 0.5


def c_grad(V):
    return min(8.0 * ORACLE_C[V], CAP_GRAD)


def tok_bounds(V):
    return 8.0 * ORACLE_A[V], 8.0 * ORACLE_R[V]


def g(seed):
    return torch.Generator().manual_seed(seed)


def edge_pairs(V):
    """(x_t, x0) at the index edges of a row of V: first / last index, one float4, neighbouring float4s, the last
    (partly filled) chunk, both sides of every kind of chunk boundary (first chunk | second, last full chunk | the
    partly filled one), and a thread's second float4 of a chunk."""
    p = [(0, 0), (0, V - 1), (V - 1, 0), (5, 4), (4, 8), (V - 1, V - 2), (V - 3, V - 3)]
    if V > WIDE_C:
        last = (V - 1) // WIDE_C * WIDE_C           # first index of the last chunk
        p += [(WIDE_C - 1, WIDE_C), (last, last - 1), (last - 1, last - 1), (2049, last + 1 if last + 1 < V else 7)]
    return p


class KlCase:
    pass


@functools.lru_cache(maxsize=2)
def kl_case(V, masked, B=4, L=12):
    """Inputs and the float64 reference of one KL case (computed once, shared, never modified). Logits 3 randn
    (2 randn below V = 100); x_t = x0 on every third token, then the edge pairs on the first tokens of every
    utterance (rotated by two per utterance). masked: utterance 1 all padding (cnt = 0), utterance 2 one valid token,
    utterance 0 two padded tokens."""
    c = KlCase()
    c.V, c.B, c.L, c.masked = V, B, L, masked
    c.betas, _ = O.sched_tables(TN)
    c.t = torch.tensor([1, 2, 117, TN])
    sd = V + SEED_STEP * SEED[V]
    c.logits = (2.0 if V < 100 else 3.0) * torch.randn(B, L, V, generator=g(1000 + sd))
    c.x0 = torch.randint(0, V, (B, L), generator=g(2000 + sd))
    c.xt = torch.randint(0, V, (B, L), generator=g(3000 + sd))
    c.xt[:, ::3] = c.x0[:, ::3]
    pairs = edge_pairs(V)
    for b in range(B):
        for l in range(min(L, len(pairs))):
            c.xt[b, l], c.x0[b, l] = pairs[(l + 2 * b) % len(pairs)]
    c.xm = None
    if masked:
        c.xm = torch.ones(B, L, dtype=torch.bool)
        c.xm[1] = False
        c.xm[2] = False
        c.xm[2, 3] = True
        c.xm[0, 1] = False
        c.xm[0, L - 1] = False
    c.kl, c.dz, c.w, c.s = kl_term_ref64(c.logits, c.xt, c.x0, c.t, c.xm, c.betas)
    c.loss = (c.kl * c.w).sum()
    c.generic = torch.ones(B, L, V, dtype=torch.bool)
    c.generic.scatter_(-1, c.xt[..., None], False)
    c.generic.scatter_(-1, c.x0[..., None], False)
    c.generic &= (c.w > 0)[..., None]
    c.pmin = torch.softmax(c.logits.double(), -1).min().item()
    return c


def check_preconditions(c):
    """The criterion must discriminate, from the reference alone: no probability below 1e-30 (fp32 exp underflow,
    where the scale means nothing), and C_GRAD s_k < |ref_k| / 4 on at least share_floor(V) of the generic indices
    (k neither x_t nor x0) of unmasked rows, every row counted: at V >= 32772 at most 0.1 % of them lie too close to
    their own scale to tell a wrong kernel from a right one. Returns the share."""
    assert c.pmin >= 1e-30, f"V={c.V}: probabilities underflow fp32 exp"
    ok = (c_grad(c.V) * c.s < c.dz.abs() / 4) & c.generic
    share = ok.sum().item() / c.generic.sum().item()
    assert share >= share_floor(c.V), (f"V={c.V} masked={c.masked}: only {share:.5f} of the generic elements "
                                       f"discriminate (floor {share_floor(c.V)})")
    return share


def oracle_errors(c):
    """(max |oracle32 - ref64| / s_k, max abs per-token error where |ref| < SMALL_TOK, max relative one elsewhere)
    of fp32 arithmetic on this case: the gradient from the fp32 oracle, the per-token KL from the fp32 evaluation of
    the reference's formula."""
    _, dz32 = O.kl_term(c.logits, c.xt, c.x0, c.t, c.xm, c.betas)
    live = c.s > 0
    cg = ((dz32.double() - c.dz).abs()[live] / c.s[live]).max().item()
    kl32 = kl_term_ref64(c.logits, c.xt, c.x0, c.t, c.xm, c.betas, dtype=torch.float32)[0].double()
    err = (kl32 - c.kl).abs()
    small = c.kl.abs() < SMALL_TOK
    a = err[small].max().item() if small.any() else 0.0
    r = (err[~small] / c.kl[~small].abs()).max().item() if (~small).any() else 0.0
    return cg, a, r


def grad_excess(dz, c, gs=1.0):
    """(max |dz - ref| / s_k over the elements with s_k > 0, the elements beyond C_GRAD s_k) of a kernel's gradient
    [B L, V] (f32 or bf16: a bf16 output gets one bf16 rounding, 2^-8 |ref|, on top)."""
    d = dz.double().view(c.B, c.L, c.V).cpu()
    assert torch.isfinite(d).all(), "non-finite gradient"
    ref, s = gs * c.dz, gs * c.s
    err = (d - ref).abs()
    if dz.dtype == torch.bfloat16:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    need = (err[s > 0] / s[s > 0]).max().item() if (s > 0).any() else 0.0
    return need, err > c_grad(c.V) * s, d


def check_dz(dz, c, what):
    """|dz - ref| <= C_GRAD[V] s_k (+ 2^-8 |ref| for a bf16 output), every element; s_k = 0 (masked rows) demands
    exactly 0. Returns the measured ratio."""
    need, bad, d = grad_excess(dz, c)
    print(f"{what}: max |dz - ref| / s_k = {need:.3e} (C_GRAD {c_grad(c.V):.2e})")
    assert not bad.any(), (f"{what}: {bad.sum().item()} elements off, worst ratio {need:.3e}, first at "
                           f"{bad.nonzero()[0].tolist()}")
    if c.masked:
        assert (d[c.w == 0] == 0).all(), f"{what}: masked rows must get an exactly zero gradient"
    return need


def check_kl_tok(kl_tok, c, what):
    A, R = tok_bounds(c.V)
    k = kl_tok.double().view(c.B, c.L).cpu()
    assert torch.isfinite(k).all(), f"{what}: non-finite kl_tok"
    err = (k - c.kl).abs()
    small = c.kl.abs() < SMALL_TOK
    a = err[small].max().item() if small.any() else 0.0
    r = (err[~small] / c.kl[~small].abs()).max().item() if (~small).any() else 0.0
    print(f"{what}: kl_tok max abs err {a:.3e} where |ref| < {SMALL_TOK} (A_TOK {A:.2e}), max rel err {r:.3e} "
          f"elsewhere (R_TOK {R:.2e})")
    bad = err > A + R * c.kl.abs()
    assert not bad.any(), (f"{what}: {bad.sum().item()} tokens off (abs {a:.3e}, rel {r:.3e}), first at "
                           f"{bad.nonzero()[0].tolist()}")
    return a, r
