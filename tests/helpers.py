"""Shared test helpers: PCG parameter dicts with reference names, fixture loading, comparisons."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle.weights import pcg_array


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol=1e-5, atol=1e-6, what=""):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.tensor(a, dtype=torch.float64)
    b = T(b).double() if not torch.is_tensor(b) else b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item() if a.numel() else 0.0
    tol = atol + rtol * b.abs().max().item() if b.numel() else atol
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e} (ref max {b.abs().max().item():.3e})"


def _dec_sd(V, d, H, NL, FF, prefix="dec."):
    from oracle.weights import pcg_array as P

    shapes = {"tok_emb.weight": (V, d), "time_emb.mlp.0.weight": (4 * d, d), "time_emb.mlp.0.bias": (4 * d,),
              "time_emb.mlp.2.weight": (d, 4 * d), "time_emb.mlp.2.bias": (d,), "time_proj.weight": (d, d),
              "time_proj.bias": (d,), "head.weight": (V, d), "head.bias": (V,)}
    for i in range(NL):
        b = f"blocks.{i}."
        for a in ("self_attn.", "cross_attn."):
            shapes[b + a + "in_proj_weight"] = (3 * d, d)
            shapes[b + a + "in_proj_bias"] = (3 * d,)
            shapes[b + a + "out_proj.weight"] = (d, d)
            shapes[b + a + "out_proj.bias"] = (d,)
        for f in ("scale_proj.", "shift_proj."):
            shapes[b + "film_layer." + f + "weight"] = (d, d)
            shapes[b + "film_layer." + f + "bias"] = (d,)
        shapes[b + "ff.0.weight"] = (FF, d)
        shapes[b + "ff.0.bias"] = (FF,)
        shapes[b + "ff.3.weight"] = (d, FF)
        shapes[b + "ff.3.bias"] = (d,)
        for n in ("norm1.", "norm2.", "norm3."):
            shapes[b + n + "weight"] = (d,)
            shapes[b + n + "bias"] = (d,)
    sd = {n: T(P(prefix + n, s)) for n, s in shapes.items()}
    sd["tok_emb.weight"][0] = 0.0
    return sd


SMALL_WAVLM = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                   conv_dim=(32,) * 7, num_conv_pos_embedding_groups=4)


def wavlm_sd(geom, d_model, with_proj=True):
    E = geom["hidden_size"]
    C = geom["conv_dim"]
    H = geom["num_attention_heads"]
    shapes = {}
    cin = 1
    for i, (c, k) in enumerate(zip(C, geom["conv_kernel"])):
        shapes[f"backbone.feature_extractor.conv_layers.{i}.conv.weight"] = (c, cin, k)
        cin = c
    shapes["backbone.feature_extractor.conv_layers.0.layer_norm.weight"] = (C[0],)
    shapes["backbone.feature_extractor.conv_layers.0.layer_norm.bias"] = (C[0],)
    shapes["backbone.feature_projection.layer_norm.weight"] = (C[-1],)
    shapes["backbone.feature_projection.layer_norm.bias"] = (C[-1],)
    shapes["backbone.feature_projection.projection.weight"] = (E, C[-1])
    shapes["backbone.feature_projection.projection.bias"] = (E,)
    kp, gp = geom["num_conv_pos_embeddings"], geom["num_conv_pos_embedding_groups"]
    shapes["backbone.encoder.pos_conv_embed.conv.bias"] = (E,)
    shapes["backbone.encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, kp)
    shapes["backbone.encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (E, E // gp, kp)
    shapes["backbone.encoder.layer_norm.weight"] = (E,)
    shapes["backbone.encoder.layer_norm.bias"] = (E,)
    for i in range(geom["num_hidden_layers"]):
        p = f"backbone.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            shapes[p + f"attention.{n}.weight"] = (E, E)
            shapes[p + f"attention.{n}.bias"] = (E,)
        shapes[p + "attention.gru_rel_pos_const"] = (1, H, 1, 1)
        shapes[p + "attention.gru_rel_pos_linear.weight"] = (8, E // H)
        shapes[p + "attention.gru_rel_pos_linear.bias"] = (8,)
        if i == 0:
            shapes[p + "attention.rel_attn_embed.weight"] = (geom["num_buckets"], H)
        shapes[p + "layer_norm.weight"] = (E,)
        shapes[p + "layer_norm.bias"] = (E,)
        shapes[p + "feed_forward.intermediate_dense.weight"] = (geom["intermediate_size"], E)
        shapes[p + "feed_forward.intermediate_dense.bias"] = (geom["intermediate_size"],)
        shapes[p + "feed_forward.output_dense.weight"] = (E, geom["intermediate_size"])
        shapes[p + "feed_forward.output_dense.bias"] = (E,)
        shapes[p + "final_layer_norm.weight"] = (E,)
        shapes[p + "final_layer_norm.bias"] = (E,)
    if with_proj and E != d_model:
        shapes["proj.weight"] = (d_model, E)
        shapes["proj.bias"] = (d_model,)
    return {n: T(pcg_array(n, s)) for n, s in shapes.items()}


def _step_params(V, d, NL, FF, H):
    sd = _dec_sd(V, d, H, NL, FF)
    params = {"decoder." + n: p for n, p in sd.items()}
    params["s_proj.proj.net.0.weight"] = T(pcg_array("s_proj.proj.net.0.weight", (256, d)))
    params["s_proj.proj.net.0.bias"] = T(pcg_array("s_proj.proj.net.0.bias", (256,)))
    params["t_embed.proj.weight"] = T(pcg_array("t_embed.proj.weight", (256, V)))
    params["t_proj.proj.net.0.weight"] = T(pcg_array("t_proj.proj.net.0.weight", (256, 256)))
    params["t_proj.proj.net.0.bias"] = T(pcg_array("t_proj.proj.net.0.bias", (256,)))
    return params




def jumpy_case_inputs(i, B, L, K):
    """Seeded inputs of jumpy posterior case i — the same numpy-PCG64 draws as
    tests/golden/make_golden.py:jumpy_case_inputs (the fixture stores only the outputs)."""
    r = np.random.Generator(np.random.PCG64(300 + i))
    logits = torch.from_numpy(3.0 * r.standard_normal((B, L, K), dtype=np.float32))
    xt = torch.from_numpy(r.integers(0, K, size=(B, L))).long()
    boost = torch.from_numpy(r.uniform(-10.0, 6.0, size=(B, L)).astype(np.float32))
    logits.scatter_add_(-1, xt[..., None], boost[..., None])
    return logits, xt


def kl_term_ref64(logits, xt, x0, t, x_mask, betas, dtype=torch.float64):
    """SchedulerAdapter.kl_term (train.py:190-255) per token and per element in float64: the formulas of
    oracle.fddm_oracle.kl_term with every tensor (the fp32 logits and the fp32 betas) promoted first. Returns
      kl_tok [B, L]     the per-token KL, masked tokens included,
      dz     [B, L, V]  d loss / d logits = w xhat (g - sum_j g_j xhat_j), g = g0 + g1,
      w      [B, L]     the masked-mean weights d loss / d kl_tok (mask / (count + eps) / B, or 1 / (L B)),
      s      [B, L, V]  the per-element error scale w xhat_k (|g0_k| + |g1_k| + sum_j xhat_j (|g0_j| + |g1_j|)) with
                        g0 = -Q M a_p / ((P + eps)(d_p + eps)) and g1 = [k = x_t] a_t S1 / (d_p + eps): the size of
                        the terms whose rounding errors reach element k (|dz_k| itself is no usable scale where
                        g_k is close to sum_j g_j xhat_j).
    dtype=torch.float32 evaluates the same expressions in fp32 (what fp32 arithmetic costs per token, which the
    oracle, returning only the loss, does not show); the reference is the float64 default."""
    B, L, V = logits.shape
    eps = 1e-8
    K = float(V)
    z = logits.to(dtype)
    xhat = torch.softmax(z, dim=-1)
    bt = betas[t - 1].to(dtype).view(B, 1)
    bp = torch.where(t.eq(1), torch.zeros((), dtype=betas.dtype), betas[(t - 2).clamp(min=0)]).to(dtype).view(B, 1)
    a_t, b_t = 1.0 - bt, bt / K
    a_p, b_p = 1.0 - bp, bp / K
    is_xt = torch.nn.functional.one_hot(xt, V).to(dtype)
    is_x0 = torch.nn.functional.one_hot(x0, V).to(dtype)
    M = b_t[..., None] + a_t[..., None] * is_xt
    d_q = b_t + a_t * (x0 == xt).to(dtype)
    d_p = b_t + a_t * torch.gather(xhat, -1, xt[..., None])[..., 0]
    Q = M * (a_p[..., None] * is_x0 + b_p[..., None]) / (d_q[..., None] + eps)
    P = M * (a_p[..., None] * xhat + b_p[..., None]) / (d_p[..., None] + eps)
    kl_tok = (Q * (torch.log(Q + eps) - torch.log(P + eps))).sum(-1)
    if x_mask is not None:
        valid = x_mask.to(dtype)
        w = valid / (valid.sum(1, keepdim=True) + eps) / B
    else:
        w = torch.full((B, L), 1.0 / (L * B), dtype=dtype)
    S1 = (Q * P / (P + eps)).sum(-1)
    g0 = -Q * M * a_p[..., None] / ((P + eps) * (d_p[..., None] + eps))
    g1 = is_xt * (a_t * S1 / (d_p + eps))[..., None]
    g = g0 + g1
    dz = w[..., None] * xhat * (g - (g * xhat).sum(-1, keepdim=True))
    ga = g0.abs() + g1.abs()
    s = w[..., None] * xhat * (ga + (ga * xhat).sum(-1, keepdim=True))
    return kl_tok, dz, w, s


# ------------------------------------------------------------------ fused AdamW (csrc/optim.hip) reference and inputs
def _f32(x):
    return float(np.float32(x))


class AdamwScales:
    """Per-element quantities of one adamw_step_ref step (float64): the update term u and the error scales."""
    __slots__ = ("u", "s_m", "s_v", "s_u", "s_p", "coef")


def adamw_step_ref(p, g, m, v, step, total_sq, *, lr, wd, b1, b2, eps, max_norm, grad_scale, dtype=torch.float64,
                   torch_form=False):
    """One fused clip + AdamW step (the order at the top of csrc/optim.hip) from a given state. `step` is the tensor's
    step counter before the step (the bias corrections use t = step + 1), total_sq the sum of squares of the raw
    gradients of the whole step. With s = grad_scale:
        coef = s min(1, max_norm / (s sqrt(total_sq) + 1e-6))   (coef = s when max_norm is None or 0)
        g' = coef g;  p1 = p (1 - lr wd);  m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2
        ss = lr / (1 - b1^t);  bc = sqrt(1 - b2^t);  u = ss m' / (sqrt(v') / bc + eps);  p' = p1 - u
    Default form: the operation as the C ABI receives it — lr, lr wd, b1, b2, eps, max_norm, grad_scale (and the 1e-6
    of the clip, a float literal in the kernel) are rounded to float32 first, everything after that is float64, the
    bias corrections included. torch_form=True keeps the Python doubles (1 - b2 = 0.001 as in torch.optim.AdamW).
    dtype=torch.float32 evaluates the same expressions in fp32 in the kernel's order (ss and bc in double, then
    rounded, as the kernel does), without FMA contraction.
    Returns p', m', v' (in dtype) and an AdamwScales of float64 tensors:
        u    the update term
        s_m  = |m| + |g'|
        s_v  = v + g'^2
        s_u  = ss (b1 |m| + (1 - b1) |g'|) / (sqrt(v') / bc + eps)   the cancellation-free size of u (|u| itself is no
               usable scale where b1 m is close to -(1 - b1) g')
        s_p  = |p| + |p'| + |u|"""
    import math
    if torch_form:
        lr_, lrwd, b1_, b2_, eps_, tiny = float(lr), float(lr) * float(wd), float(b1), float(b2), float(eps), 1e-6
        mn, s = float(max_norm or 0.0), float(grad_scale)
    else:
        lr_, lrwd, b1_, b2_, eps_, tiny = _f32(lr), _f32(float(lr) * float(wd)), _f32(b1), _f32(b2), _f32(eps), _f32(1e-6)
        mn, s = _f32(max_norm or 0.0), _f32(grad_scale)
    R = _f32 if dtype == torch.float32 else float       # the rounding of every scalar intermediate
    coef = s
    if mn > 0.0:
        coef = R(s * min(1.0, R(mn / R(R(s * R(math.sqrt(float(total_sq)))) + tiny))))
    t = float(step) + 1.0
    ss = R(lr_ / (1.0 - b1_ ** t))
    bc = R(math.sqrt(1.0 - b2_ ** t))
    keep, omb1, omb2 = R(1.0 - lrwd), R(1.0 - b1_), R(1.0 - b2_)
    P, G, M, V = (x.detach().to(dtype) for x in (p, g, m, v))
    g1 = G * coef
    p1 = P * keep
    m1 = M + omb1 * (g1 - M)
    v1 = V * b2_ + (omb2 * g1) * g1
    den = v1.sqrt() / bc + eps_
    u = ss * (m1 / den)
    p2 = p1 - u
    sc = AdamwScales()
    Pd, Md, Vd, g1d, dend = P.double(), M.double(), V.double(), g1.double(), den.double()
    sc.coef = coef
    sc.u = u.double()
    sc.s_m = Md.abs() + g1d.abs()
    sc.s_v = Vd + g1d * g1d
    sc.s_u = ss * (b1_ * Md.abs() + (1.0 - b1_) * g1d.abs()) / dend
    sc.s_p = Pd.abs() + p2.double().abs() + sc.u.abs()
    return p2, m1, v1, sc


# fp32 evaluation of the step against float64, in units of 2^-24 x the scales, measured on the CPU over every scenario of
# adamw_scenarios() on the tensors of adamw_tensors() (tests/test_cpu_optim_ref.py asserts them with 10 % headroom;
# tests/test_gpu_optim.py allows the kernel ADAMW_C x these):
#   |dp + du| <= E_P 2^-24 s_p (the decay and the final subtraction), |du| <= E_U 2^-24 s_u,
#   |dm| <= E_M 2^-24 s_m, |dv| <= E_V 2^-24 s_v
ADAMW_E = dict(P=1.19, U=6.17, M=1.03, V=1.98)
ADAMW_C = 4.0              # the kernel differs from that evaluation only by FMA contraction
ADAMW_HP = dict(lr=2e-4, wd=0.01, b1=0.9, b2=0.999, eps=1e-8)           # FusedAdamW's defaults
ADAMW_HP2 = dict(lr=1e-3, wd=0.1, b1=0.8, b2=0.95, eps=1e-6)            # the second parameter group
MT_CHUNK = 65536           # elements per block of the multi-tensor kernels (csrc/optim.hip)

# (name, shape, parameter kind, gradient kind, unaligned, parameter group). Parameter kinds: unit = randn, small =
# 1e-3 randn, zero. Gradient kinds: randn7 = randn with every 7th element exactly 0, logu = magnitudes log-uniform in
# 1e-10 .. 1 with a random sign (reaches sqrt(v) / bc ~ eps). Every shape has a unit parameter and a logu gradient
# somewhere in the set; 475 408 elements, 13 chunks.
ADAMW_TENSORS = [
    ("a", (257, 255), "unit", "logu", False, 0),    # one chunk, n % 4 = 3: vector loop + scalar tail (bf16: both copies)
    ("b", (256, 256), "unit", "randn7", False, 0),  # exactly one chunk
    ("c", (3, 43691), "unit", "logu", False, 1),    # three chunks, the last holds one element
    ("d", (40963,), "unit", "randn7", False, 0),    # 1-D; n / 4 = 10240: one 8-deep sumsq pass + ragged single loads
    ("e", (70,), "unit", "randn7", False, 1),
    ("f", (1,), "unit", "logu", False, 0),
    ("g", (65661,), "unit", "logu", True, 1),       # element offset 1 of a larger buffer: scalar paths, two chunks
    ("h", (256, 256), "zero", "logu", False, 0),
    ("i", (40963,), "small", "logu", False, 1),
    ("j", (70,), "zero", "logu", False, 1),
]


def adamw_params(seed=11):
    """{name: initial fp32 parameter} of ADAMW_TENSORS."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape, pk, _, _, _ in ADAMW_TENSORS:
        x = torch.randn(*shape, generator=gen)
        out[name] = x if pk == "unit" else 1e-3 * x if pk == "small" else torch.zeros(*shape)
    return out


def adamw_grads(k, mult=1.0, seed=23):
    """{name: fp32 gradient} of draw k (one per step), scaled by mult."""
    gen = torch.Generator().manual_seed(seed + 1000 * k)
    out = {}
    for name, shape, _, gk, _, _ in ADAMW_TENSORS:
        x = torch.randn(*shape, generator=gen)
        if gk == "randn7":
            x.view(-1)[::7] = 0.0
        else:
            mag = torch.pow(10.0, -10.0 * torch.rand(*shape, generator=gen, dtype=torch.float64)).float()
            x = torch.where(x < 0, -mag, mag)
        out[name] = x * mult
    return out


def adamw_scenarios():
    """name -> dict(mult = gradient multiplier, max_norm, grad_scale, groups = use both hyperparameter sets). Each runs
    steps 1, 2, 3 and then one step with every step counter set to 999."""
    return {
        "clipped": dict(mult=10.0, max_norm=5.0, grad_scale=1.0, groups=False),
        "not_clipped": dict(mult=1e-4, max_norm=5.0, grad_scale=1.0, groups=False),   # coef == grad_scale exactly
        "no_clip": dict(mult=1.0, max_norm=None, grad_scale=1.0, groups=False),
        "scaled_clipped": dict(mult=10.0, max_norm=5.0, grad_scale=0.125, groups=False),
        "scaled_not_clipped": dict(mult=1e-4, max_norm=5.0, grad_scale=0.125, groups=False),
        "groups": dict(mult=10.0, max_norm=5.0, grad_scale=1.0, groups=True),
    }


ADAMW_COUNTERS = (0.0, 1.0, 2.0, 999.0)     # the step counter before each of a scenario's four steps
ADAMW_SKIP = {"b": 1, "i": 1}               # groups scenario: tensor -> index of the step at which its grad is None


def adamw_scenario_grads(cfg, k):
    """Gradients of step index k of a scenario (the groups scenario drops ADAMW_SKIP's tensors at their step)."""
    G = adamw_grads(k, cfg["mult"])
    if cfg["groups"]:
        for n, ks in ADAMW_SKIP.items():
            if ks == k:
                del G[n]
    return G


def adamw_hp(name, groups):
    """Hyperparameters of tensor `name`: the second set for group 1 of the groups scenario, else the defaults."""
    grp = {n: gr for n, _, _, _, _, gr in ADAMW_TENSORS}[name]
    return ADAMW_HP2 if groups and grp == 1 else ADAMW_HP


def adamw_bounds(sc):
    """The per-element bounds of tests/test_gpu_optim.py on |p - p_ref|, |m - m_ref|, |v - v_ref|."""
    c = ADAMW_C * 2.0 ** -24
    return (c * (ADAMW_E["P"] * sc.s_p + ADAMW_E["U"] * sc.s_u), c * ADAMW_E["M"] * sc.s_m, c * ADAMW_E["V"] * sc.s_v)


def sumsq64(grads):
    """Sum of squares of a {name: gradient} dict in float64."""
    return sum(float((x.double() ** 2).sum()) for x in grads.values())


class CollectiveLog:
    """Records every torch.distributed collective issued inside the context (name, shape, dtype, reduce op), in
    issue order: DP ranks must issue the identical sequence (fddm_hip.dist, train.train_one_epoch)."""

    NAMES = ("all_reduce", "broadcast", "all_gather", "all_gather_into_tensor", "reduce_scatter_tensor",
             "all_gather_object", "barrier")

    def __init__(self):
        self.log = []
        self._orig = {}

    def __enter__(self):
        import torch.distributed as dist
        for n in self.NAMES:
            f = getattr(dist, n, None)
            if f is None:
                continue
            self._orig[n] = f

            def wrap(*a, _n=n, _f=f, **k):
                t = a[0] if a and hasattr(a[0], "shape") else None
                op = k.get("op", a[1] if _n == "all_reduce" and len(a) > 1 else None)
                self.log.append((_n, tuple(t.shape) if t is not None else None, str(t.dtype) if t is not None
                                 else None, str(op) if op is not None else None))
                return _f(*a, **k)
            setattr(dist, n, wrap)
        return self

    def __exit__(self, *exc):
        import torch.distributed as dist
        for n, f in self._orig.items():
            setattr(dist, n, f)
        return False


# ------------------------------------------------------------------ fwd8 (csrc/attn8.hip) guard inputs
def fwd8_fast_path_rowsum(q, k, keep=None):
    """What fwd8's fast path accumulates as one head's row sums, emulated on the CPU (csrc/attn8.hip: first_ref, the
    chain-state comment and the guard before the fallback): q [Lq, 64], k [Lk, 64] already rounded to bf16, keep [Lk]
    bool or None. Q' = bf16(q scale log2 e) at scale 1/8; scores Q' k^T in log2 units, masked keys -inf; the
    reference is the bf16 rounding of the row's maximum over keys 0..31 (0 where that is -inf), fixed for the whole
    row; the sum of exp2(score - reference) in float32. Returns (sum [Lq] float32, tripped [Lq] bool): tripped = the
    guard's predicate, not (2^-40 <= sum <= 2^64), NaN included. It proves statements about test inputs (which rows
    must take the fallback); it does not model the bf16 packing of P or the MFMA summation order and is no oracle for
    the kernel's outputs."""
    sl2 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    qp = (q.float() * sl2).to(torch.bfloat16)
    s = (qp.double() @ k.double().t()).float()
    if keep is not None:
        s = s.masked_fill(~keep[None, :], float("-inf"))
    m0 = s[:, :32].max(-1).values
    rf = torch.where(torch.isinf(m0) & (m0 < 0), torch.zeros_like(m0), m0.to(torch.bfloat16).float())
    tot = torch.exp2(s - rf[:, None]).sum(-1, dtype=torch.float32)
    return tot, ~((tot >= 2.0 ** -40) & (tot <= 2.0 ** 64))


# (kind, c, class, geometries) of fwd8_guard_inputs: what the fast path's row sum of a designated row does. The
# constants hold for fwd8_guard_inputs' seed and these geometries (tests/test_cpu_attn_inputs.py asserts the margins); the
# designated rows' sums spread over ~2^16 between rows and heads (the randn part of their scores), which is why the
# inside constants sit further from the bounds than a single row would need.
FWD8_GUARD_KINDS = [
    ("rise", 12.0, "trips", "abcd"),   # the sum overflows float32: only the fallback can be right
    ("rise", 4.7, "trips", "a"),       # above 2^64 but finite
    ("rise", 3.3, "inside", "abcd"),   # the fast path at the top of its range
    ("fall", 25.0, "trips", "abcd"),   # every exponential underflows, the sum is 0: only the fallback can be right
    ("fall", 10.0, "trips", "a"),      # below 2^-40 but nonzero
    ("fall", 6.8, "inside", "abcd"),   # the fast path at the bottom of its range
]
# name -> (B, H, Lq, Lk, dropout p, keys padded at the end of the last batch, designated query rows (None = all))
FWD8_GUARD_GEOMS = {
    "a": (1, 2, 256, 256, 0.1, 9, (37, 200)),
    "b": (1, 2, 130, 200, 0.1, 0, (129,)),
    "c": (1, 2, 600, 512, 0.0, 0, (5, 599)),
    "d": (2, 3, 64, 96, 0.1, 0, None),
}


def fwd8_guard_inputs(geom, kind, c, seed=29):
    """Inputs whose designated query rows drive fwd8's fixed-reference row sum to the edges of its guard (or past
    them). Per head q, k, v ~ randn; one unit vector u shared by every head; the designated rows of q are
    40 u + 0.05 randn, so their scaled score against a key shifted by s u is 5 s (7.2 s in log2 units) plus the randn
    part. kind "rise": keys 0..31 get -c u and keys 32.. get +c u (the later keys exceed the first half-tile's
    reference by ~14.4 c in log2 units); kind "fall": keys 0..31 are padding (the reference stays 0) and every key gets
    -c u (every valid score sits ~7.2 c below it). Returns q [B, Lq, H*64], k, v [B, Lk, H*64] (float32), keep
    [B, Lk] bool or None, and the designated rows as a list."""
    B, H, Lq, Lk, _, tail, rows = FWD8_GUARD_GEOMS[geom]
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(64, generator=gen)
    u = u / u.norm()
    q, k, v = (torch.randn(B, L, H, 64, generator=gen) for L in (Lq, Lk, Lk))
    rows = list(range(Lq)) if rows is None else list(rows)
    q[:, rows] = 40.0 * u + 0.05 * torch.randn(B, len(rows), H, 64, generator=gen)
    keep = None
    if tail or kind == "fall":
        keep = torch.ones(B, Lk, dtype=torch.bool)
        if tail:
            keep[B - 1, Lk - tail:] = False
    if kind == "rise":
        k[:, :32] -= c * u
        k[:, 32:] += c * u
    else:
        keep[:, :32] = False
        k -= c * u
    return q.reshape(B, Lq, H * 64), k.reshape(B, Lk, H * 64), v.reshape(B, Lk, H * 64), keep, rows


def fwd8_guard_cases():
    """(geometry, kind, c, class) of every guard case: the representable-but-tripping constants on geometry a only."""
    return [(g, kind, c, cls) for g in FWD8_GUARD_GEOMS for kind, c, cls, where in FWD8_GUARD_KINDS if g in where]


# ------------------------------------------------------------------ GEMM families (csrc/gemm.hip, gemm128.hip, gemm256.hip)
# Reference, per-element bounds, inputs and the case table shared by tests/test_cpu_gemm_ref.py (which sets the
# constants below from the reference alone) and tests/test_gpu_gemm.py (which runs the kernels).
U24 = 2.0 ** -24
EPI_STORE, EPI_GELU, EPI_ACC, EPI_GELU_ONLY, EPI_DGELU = 0, 1, 2, 3, 4
EPI_NAMES = {EPI_STORE: "store", EPI_GELU: "gelu+c2", EPI_ACC: "acc", EPI_GELU_ONLY: "gelu", EPI_DGELU: "dgelu"}
GEMM_ALPHAS = (1.0, -0.375, 1.0 / 1536.0)
GEMM_GELU_ABS = 2e-6           # gelu_f against the erf GELU (test_gelu_fast_erf_accuracy's bar)
GEMM_GELU_BF16OUT_ABS = 2.6e-5  # gelu_bf16out, the 256x256 kernel's GELU-only epilogue (csrc/common.h)
GEMM_DGELU_REL = 2e-6          # gelu_grad: |err| <= 2e-6 |y| (common.h documents 1e-7 for Phi)
# fp32 evaluation (64-wide K tiles added in order, split-K slices added in order, then alpha, bias, c_old) against
# float64 in units of 2^-24 s, the maximum over every case of gemm_cases() (3.43, 2.82) and of CONV_CASES as im2col
# GEMMs (6.66, 5.34) per compute dtype (f32, bf16), measured on the CPU
# (tests/test_cpu_gemm_ref.py asserts them; the constants keep 10 % headroom). The kernels are allowed GEMM_C = 8 E units:
# the margin covers the MFMA-internal summation order, gemm128's k-half split, the order of the split-K atomics and the
# epilogue's roundings. Hard cap 64.
GEMM_E = {"f32": 3.8, "bf16": 3.1, "conv-f32": 7.3, "conv-bf16": 5.9}
GEMM_C = {k: 8.0 * v for k, v in GEMM_E.items()}
# The WavLM front end (csrc/wavlm.hip, csrc/posconv.hip; the section at the end of this file), in the same way:
U18 = 2.0 ** -18               # conv0_mfma: v = hi + lo leaves <= 2^-18 |v|, the dropped lo * lo term is of that order
# fp32 (resp. hi/lo bf16 split) evaluation in each kernel's order against float64, in units of 2^-24 s (conv0_split:
# 2^-18 s), the maximum over every case of the tables below, measured on the CPU: 4.65, 4.26, 1.36, 2.18
# (tests/test_cpu_wavlm_front_ref.py asserts them; the constants keep 10 % headroom). The kernels are allowed
# FRONT_C = 8 E units: the margin covers the MFMA-internal summation order, packed-FMA contraction, the roundings of sc
# and sh and the fast exp / rcp. Hard cap 64.
FRONT_E = {"conv0_f32": 5.1, "conv0_split": 4.65, "posconv": 1.49, "gate": 2.39}
FRONT_C = {k: 8.0 * v for k, v in FRONT_E.items()}
FRONT_E_FLOOR = 0.05           # stored <= 1.1 measured + this


class GemmRef:
    __slots__ = ("y", "s", "act", "lin", "add", "scale", "epi", "colsum", "colsum_s")


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def gemm_ref64(A, B, *, bias=None, alpha=1.0, c_old=None, epi=EPI_STORE, pre=None, keep=None, drop_p=0.0, prod=None):
    """Float64 reference of one fddm_gemm call. A [M, K], B [N, K]: the logical operands, already rounded to the
    compute dtype and promoted to float64 (any device). alpha as the C ABI receives it (a float32 value).
      y        alpha A B^T + bias (+ c_old)
      s        |alpha| (|A| |B|^T) + |bias| + |c_old|: the size of the terms whose roundings reach each element
      act      the epilogue's second value: gelu(y) (EPI_GELU, EPI_GELU_ONLY) or y (Phi(pre) + pre phi(pre)) (EPI_DGELU),
               times the dropout mask keep / (1 - p) when keep (bool [M, N], oracle dropout_keep) is given; else None
      lin      |d act / d y| without the dropout factor: |gelu'(y)| or |gelu'(pre)|
      add      the absolute slack of act that scales with the data: 2e-6 |y| for EPI_DGELU, else 0
      scale    keep / (1 - p) (1 without dropout): dropped elements get bound 0, i.e. must be exactly 0
      colsum   A.sum(K) and colsum_s = |A|.sum(K), the fused bias gradient of an M/N-contiguous A
    prod = (A B^T, |A| |B|^T) computed earlier from the same operands (cases that share a shape share the products)."""
    r = GemmRef()
    a = float(alpha)
    P, S = prod if prod is not None else (A @ B.t(), A.abs() @ B.abs().t())
    r.y = a * P
    r.s = abs(a) * S
    if bias is not None:
        r.y = r.y + bias.double()[None, :]
        r.s = r.s + bias.double().abs()[None, :]
    if c_old is not None:
        r.y = r.y + c_old.double()
        r.s = r.s + c_old.double().abs()
    r.colsum, r.colsum_s = A.sum(1), A.abs().sum(1)
    return epilogue_ref64(r, epi, pre=pre, keep=keep, drop_p=drop_p)


def epilogue_ref64(r, epi, *, pre=None, keep=None, drop_p=0.0):
    """Fill act / lin / add / scale of a GemmRef whose y and s are set (gemm_ref64's second half; the implicit
    convolutions enter here with F.conv1d's y)."""
    r.epi = epi
    r.scale = torch.ones_like(r.y)
    if keep is not None:
        r.scale = keep.to(r.y.dtype) / (1.0 - float(np.float32(drop_p)))
    r.act = r.lin = r.add = None
    if epi in (EPI_GELU, EPI_GELU_ONLY):
        r.act = torch.nn.functional.gelu(r.y) * r.scale
        r.lin = gelu_grad64(r.y).abs()
        r.add = torch.zeros_like(r.y)
    elif epi == EPI_DGELU:
        g = gelu_grad64(pre.double())
        r.act = r.y * g * r.scale
        r.lin = g.abs()
        r.add = GEMM_DGELU_REL * r.y.abs()
    return r


def gemm_bound(r, which, C, bf16_out, gelu_abs=GEMM_GELU_ABS):
    """(reference, per-element bound) of output `which` of a GemmRef: "y" (store / accumulate / the pre-activation
    of EPI_GELU): C 2^-24 s; "act": (lin C 2^-24 s + a) scale with a = gelu_abs for the GELU outputs and 2e-6 |y| for
    dGELU. A bf16 output adds one rounding with a factor 2, 2^-8 |ref|."""
    if which == "y":
        ref, b = r.y, C * U24 * r.s
    else:
        ref = r.act
        b = (r.lin * (C * U24) * r.s + (r.add if r.epi == EPI_DGELU else gelu_abs)) * r.scale
    if bf16_out:
        b = b + 2.0 ** -8 * ref.abs()
    return ref, b


def gemm_eval_fp32(A, B, *, bias=None, alpha=1.0, c_old=None, ksplit=0):
    """The same value in fp32 arithmetic: A [M, K], B [N, K] float32 (the rounded operands; products of two bf16 are
    exact in fp32). Each split-K slice of ksplit (0: one slice) accumulates its 64-wide K tiles in order; the slices are
    added in order; then alpha, the bias and c_old."""
    M, K = A.shape
    ks = ksplit or K
    tot = torch.zeros(M, B.shape[0], dtype=torch.float32)
    for k0 in range(0, K, ks):
        acc = torch.zeros_like(tot)
        for k in range(k0, min(K, k0 + ks), 64):
            k1 = min(K, k0 + ks, k + 64)
            acc = acc + A[:, k:k1] @ B[:, k:k1].t()
        tot = tot + acc
    y = tot * np.float32(alpha)
    if bias is not None:
        y = y + bias.float()[None, :]
    if c_old is not None:
        y = y + c_old.float()
    return y


_GEMM_OPERANDS = {}


def gemm_operands(M, N, K, dt, a_f32=False):
    """Seeded operands of one (M, N, K): A [M, K] and B [N, K] = randn times a per-row (A) and a per-column (B, the
    output's columns) power of two from 2^-6 .. 2^6, rounded to the compute dtype dt ("f32" / "bf16"; a_f32: A stays
    float32, the kernel rounds it to bf16 while staging), so that small rows and columns cannot hide under large ones.
    bias = randn times the column scale (f32). c_old (the accumulate epilogue's previous C) = randn times both scales,
    pre (the dGELU epilogue's saved pre-activation) = 2 randn, cs_old = randn times the row scale. CPU tensors, cached."""
    key = (M, N, K, dt, a_f32)
    if key not in _GEMM_OPERANDS:
        gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        r = torch.pow(2.0, torch.randint(-6, 7, (M,), generator=gen).float())
        c = torch.pow(2.0, torch.randint(-6, 7, (N,), generator=gen).float())
        td = torch.float32 if dt == "f32" else torch.bfloat16
        A = torch.randn(M, K, generator=gen) * r[:, None]
        B = (torch.randn(N, K, generator=gen) * c[:, None]).to(td)
        A = A if a_f32 else A.to(td)
        bias = torch.randn(N, generator=gen) * c
        c_old = torch.randn(M, N, generator=gen) * r[:, None] * c[None, :]
        pre = 2.0 * torch.randn(M, N, generator=gen)
        cs_old = torch.randn(M, generator=gen) * r
        _GEMM_OPERANDS[key] = dict(A=A, B=B, bias=bias, c_old=c_old, pre=pre, cs_old=cs_old)
    return _GEMM_OPERANDS[key]


def gemm_logical64(ops_, dt, device=None):
    """The logical float64 operands of a gemm_operands() entry: an f32-stored A of a bf16 GEMM rounds to bf16 first."""
    A, B = ops_["A"], ops_["B"]
    if dt == "bf16":
        A = A.to(torch.bfloat16)
    if device is not None:
        A, B = A.to(device), B.to(device)
    return A.double(), B.double()


def small_splits(M, N, K, dt):
    """(slices, K per slice) of fddm_gemm's register-staged kernel for an f32 store / accumulate (csrc/gemm.hip)."""
    kstep = 64 if dt == "bf16" else 32
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 512 or K < 8 * kstep:
        return 1, 0
    nz = max(1, min((512 + tiles - 1) // tiles, K // max(kstep, 512), 64))
    if nz == 1:
        return 1, 0
    ks = ((K + nz - 1) // nz + kstep - 1) // kstep * kstep
    return (K + ks - 1) // ks, ks


def g128_splits(M, N, K):
    """(slices, K per slice) of the 128x128 LDS-DMA kernel for an f32 store / accumulate (fddm_gemm's dispatch)."""
    t = ((M + 127) // 128) * ((N + 127) // 128)
    if t >= 192 or K < 4096:
        return 1, 0
    nz = max(1, min((256 + t - 1) // t, K // 2048))
    if nz == 1:
        return 1, 0
    ks = ((K + nz - 1) // nz + 63) // 64 * 64
    return (K + ks - 1) // ks, ks


def _case(fam, dt, M, N, K, epi, out, *, a_kc=1, b_kc=1, bias=True, alpha=1.0, p=0.0, pad=0, colsum=False, Mi=0,
          a_f32=False, cap=0, expect=None):
    nz, ks = 1, 0
    if out == "f32" and epi in (EPI_STORE, EPI_ACC) and not Mi:
        if fam == "small":
            nz, ks = small_splits(M, N, K, dt)
        elif fam == "128":
            nz, ks = g128_splits(M, N, K)
    if fam == "128" and bias and (epi == EPI_ACC or nz > 1):
        # the ring kernel's accumulate epilogue takes no bias: fddm_gemm must send these to the register-staged kernel
        expect = "small"
        nz, ks = small_splits(M, N, K, dt)
    c = dict(fam=fam, dt=dt, M=M, N=N, K=K, epi=epi, out=out, a_kc=a_kc, b_kc=b_kc, bias=bias, alpha=alpha, p=p, pad=pad,
             colsum=colsum, Mi=Mi, a_f32=a_f32, cap=cap, splits=nz, ksplit=ks, expect=expect or fam)
    c["id"] = (f"{fam}-{dt}{'-af32' if a_f32 else ''}-{M}x{N}x{K}-{'k' if a_kc else 'm'}{'k' if b_kc else 'm'}-"
               f"{EPI_NAMES[epi]}-{out}" + ("-bias" if bias else "") + (f"-a{GEMM_ALPHAS.index(alpha)}" if alpha != 1.0 else "")
               + (f"-p{p}" if p else "") + (f"-pad{pad}" if pad else "") + ("-colsum" if colsum else "")
               + (f"-Mi{Mi}" if Mi else "") + (f"-cap{cap}" if cap else "") + (f"-z{nz}" if nz > 1 else "")
               + (f"-not{fam}" if expect else ""))
    return c


LAYOUTS = ((1, 1), (1, 0), (0, 0), (0, 1))


def _epis(dt, which):
    """(epi, out, p) of every epilogue in `which` for compute dtype dt; the GELU family writes the compute dtype."""
    o = []
    for e in which:
        if e == "store_f32":
            o.append((EPI_STORE, "f32", 0.0))
        elif e == "store_bf16":
            if dt == "bf16":
                o.append((EPI_STORE, "bf16", 0.0))
        elif e == "acc":
            o.append((EPI_ACC, "f32", 0.0))
        elif e == "gelu_only":
            o.append((EPI_GELU_ONLY, dt, 0.0))
        elif e == "gelu":
            o += [(EPI_GELU, dt, 0.0), (EPI_GELU, dt, 0.1)]
        elif e == "dgelu":
            o += [(EPI_DGELU, dt, 0.0), (EPI_DGELU, dt, 0.1)]
    return o


ALL_EPIS = ("store_f32", "store_bf16", "gelu", "gelu_only", "dgelu", "acc")


def gemm_cases():
    """Every fddm_gemm case of tests/test_gpu_gemm.py: the smallest shapes at which each mechanism of each kernel family
    exists (the reasons stand next to the shapes). alpha and bias cycle so that every (family, layout, epilogue) meets
    all three alphas and both a bias and none."""
    cs = []
    count = {}

    def cyc(out, *key):
        # alpha = 1/1536 meets a bias only where the output is f32: under a bf16 output's rounding of a bias-sized
        # value no reference could tell what happened to a product 1536 times smaller
        n = count[key] = count.get(key, -1) + 1       # one cycle of 6 per (family, layout / epilogue)
        al = GEMM_ALPHAS[n % 3]
        return dict(alpha=al, bias=n % 2 == 0 and not (out == "bf16" and al == GEMM_ALPHAS[2]))

    # ---- small: the register-staged 128x128 kernel (gemm_kernel), forced
    for dt in ("f32", "bf16"):
        for a_kc, b_kc in LAYOUTS:
            # one partial K-step, N < 128 | 3 x 2 tiles, ragged last K-step (bf16 64-wide, f32 32-wide)
            for M, N, K in ((136, 72, 40), (264, 136, 200)):
                cs.append(_case("small", dt, M, N, K, EPI_STORE, dt, a_kc=a_kc, b_kc=b_kc, **cyc(dt, "s", EPI_STORE)))
        # N % 8 != 0, ldc = 77: the scalar store path of every epilogue, rows unaligned
        for epi, out, p in _epis(dt, ALL_EPIS):
            cs.append(_case("small", dt, 136, 75, 200, epi, out, p=p, pad=2, **cyc(out, "s", epi)))
        # ... and zero2d's unaligned-row and tail branches under a 2-slice split-K store
        cs.append(_case("small", dt, 136, 75, 1096, EPI_STORE, "f32", pad=2, **cyc("f32", "s", EPI_STORE)))
        # split-K, K = 1096 = 576 + 520: 2 slices, the second ragged; bias on slice 0 only; ldc > N
        for epi in (EPI_STORE, EPI_ACC):
            for al in GEMM_ALPHAS[:2]:
                cs.append(_case("small", dt, 136, 72, 1096, epi, "f32", bias=True, alpha=al, pad=8))
            cs.append(_case("small", dt, 136, 72, 1096, epi, "f32", a_kc=0, b_kc=0, colsum=True, **cyc("f32", "s", epi)))
        cs.append(_case("small", dt, 136, 72, 200, EPI_STORE, "f32", a_kc=0, b_kc=0, colsum=True, bias=False))
        cs.append(_case("small", dt, 136, 72, 200, EPI_ACC, "f32", a_kc=0, b_kc=0, colsum=True, bias=True))
        # batched A rows: Mi = 50, batch stride > Mi * lda
        cs.append(_case("small", dt, 150, 72, 200, EPI_STORE, dt, Mi=50, **cyc(dt, "s", EPI_STORE)))
        cs.append(_case("small", dt, 150, 72, 1096, EPI_STORE, "f32", Mi=50, **cyc("f32", "s", EPI_STORE)))   # batched: never split
        # every epilogue on 3 x 2 tiles
        for epi, out, p in _epis(dt, ALL_EPIS):
            cs.append(_case("small", dt, 264, 136, 200, epi, out, p=p, **cyc(out, "s", epi)))
    for a_kc, b_kc in LAYOUTS:   # f32-stored A, bf16 MFMA
        cs.append(_case("small", "bf16", 136, 72, 200, EPI_STORE, "bf16", a_kc=a_kc, b_kc=b_kc, a_f32=True, **cyc("bf16", "s", "af32")))

    # ---- 128: the 4-stage LDS-DMA ring (gemm128_kernel), forced, bf16
    # one tile | 1..5 K-tiles against the 3-ahead ring prologue, tiles shifted in both dimensions | 4 x 3 tiles
    shapes = [(128, 128, 64)] + [(200, 136, K) for K in (64, 128, 192, 256, 320)] + [(392, 264, 128)]
    per_layout = {(1, 1): ALL_EPIS, (1, 0): ("store_f32", "store_bf16", "dgelu", "acc"), (0, 0): ("store_f32", "acc")}
    for (a_kc, b_kc), which in per_layout.items():
        for M, N, K in shapes:
            for epi, out, p in _epis("bf16", which):
                kw = cyc(out, a_kc, b_kc, epi, p)
                kw["bias"] = kw["bias"] and epi != EPI_ACC      # the ring's accumulate epilogue takes no bias (below)
                cs.append(_case("128", "bf16", M, N, K, epi, out, a_kc=a_kc, b_kc=b_kc, p=p, pad=8 if M == 392 else 0,
                                colsum=(a_kc == 0 and K in (64, 192)), **kw))
    # ragged token count: mask_set and the buffer range check, fused colsum; one ragged K-tile alone
    for epi in (EPI_STORE, EPI_ACC):
        for M, N, K in ((200, 136, 203), (128, 128, 8)):
            kw = cyc("f32", 0, 0, epi, 0.0)
            kw["bias"] = kw["bias"] and epi != EPI_ACC
            cs.append(_case("128", "bf16", M, N, K, epi, "f32", a_kc=0, b_kc=0, colsum=True, **kw))
    # split-K: 2 slices (KC: 2112 + 2048; MC: 2112 + 1988, ragged), overlap added once. With a bias the call must
    # leave this family for the register-staged kernel (8 slices there), which adds the bias on slice 0 only
    for (a_kc, b_kc), K in (((1, 1), 4160), ((0, 0), 4100)):
        for epi in (EPI_STORE, EPI_ACC):
            for bias in (True, False):
                cs.append(_case("128", "bf16", 200, 136, K, epi, "f32", a_kc=a_kc, b_kc=b_kc, bias=bias, pad=8,
                                alpha=GEMM_ALPHAS[len(cs) % 3], colsum=a_kc == 0))
    # accumulate with bias, one slice, all three alphas: off this family as well
    for al in GEMM_ALPHAS:
        cs.append(_case("128", "bf16", 200, 136, 192, EPI_ACC, "f32", bias=True, alpha=al))

    # ---- 256: the persistent 256x256 kernel (gemm256_kernel), forced, bf16 KC/KC, alpha = 1
    e256 = [(EPI_STORE, "bf16", 0.0), (EPI_STORE, "f32", 0.0), (EPI_GELU, "bf16", 0.0), (EPI_GELU, "bf16", 0.1),
            (EPI_GELU_ONLY, "bf16", 0.0)]
    i = 0
    # one tile, 2 / 3 / 4 / 9 K-tiles | 2 x 3 tiles shifted in both dimensions | 5 x 4 = 20 tiles: on 8 workgroups 2 or 3
    # tiles each and a last tile-row group of 1 < GM rows; uncapped one tile per workgroup
    for M, N, K, cap in [(256, 256, K, 0) for K in (128, 192, 256, 576)] + [(264, 520, 192, 0), (1100, 776, 128, 8),
                                                                            (1100, 776, 128, 0)]:
        for epi, out, p in e256:
            i += 1
            cs.append(_case("256", "bf16", M, N, K, epi, out, p=p, bias=i % 2 == 0, pad=8 if (i // 2) % 2 else 0, cap=cap))
    cs.append(_case("256", "bf16", 256, 256, 128, EPI_STORE, "bf16", alpha=-0.375, expect="small"))

    # ---- big: the 256x128 LDS-DMA kernel (gemm_big_kernel), forced, bf16 output
    # 15 x 17 = 255 tiles ragged in both dimensions, XCD remap remainder 7, 1..4 K-steps against the 3-slot ring
    for K in (64, 128, 192, 256):
        for epi, out, p in ((EPI_STORE, "bf16", 0.0), (EPI_GELU, "bf16", 0.1), (EPI_GELU_ONLY, "bf16", 0.0)):
            cs.append(_case("big", "bf16", 3592, 2056, K, epi, out, p=p, bias=True, alpha=GEMM_ALPHAS[len(cs) % 2]))
    seen, out = set(), []
    for c in cs:       # the explicit cases may repeat one the cycle produced
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def rope_bwd_ref64(P, cos, sin, L, magnitude=False):
    """The decoder's RoPE backward (oracle rope_apply's transpose) of P [M, d] (float64), row m at position m % L:
    with a = P[:, :d/2], b = P[:, d/2:]: out[:, 0::2] = a cos[:, 0::2] + b sin[:, 0::2],
    out[:, 1::2] = -a sin[:, 1::2] + b cos[:, 1::2]. magnitude=True adds every term (P, cos, sin given as magnitudes):
    the error scale of the same sum."""
    M, d = P.shape
    pos = torch.arange(M, device=P.device) % L
    c, s = cos.double()[pos], sin.double()[pos]
    a, b = P[:, : d // 2], P[:, d // 2:]
    out = torch.empty_like(P)
    out[:, 0::2] = a * c[:, 0::2] + b * s[:, 0::2]
    out[:, 1::2] = (a if magnitude else -a) * s[:, 1::2] + b * c[:, 1::2]
    return out


# implicit conv (fddm_conv1d_gemm): name -> geometry. x [Bn, Tin, G Cg] channels-last, w [G N, Cg, taps] as F.conv1d takes it
CONV_CASES = {
    # taps outside the input at both ends (cpad 2; the last frame's last tap is at Tin), 2 groups, 396 rows = 3 tiles + 12
    "small": dict(fam="small", G=2, Cg=16, N=24, taps=5, stride=2, cpad=2, Bn=3, Tin=263, Tout=132),
    # 260 rows x 264 columns: 2 x 2 shifted 256x256 tiles, 6 K-tiles over 3 taps, frames of both utterances in one tile
    "256": dict(fam="256", G=1, Cg=128, N=264, taps=3, stride=2, cpad=0, Bn=2, Tin=261, Tout=130),
    # 3848 x 1928: 16 x 16 = 256 tiles of 256x128 (ragged in both), one K-step per tap
    "big": dict(fam="big", G=1, Cg=64, N=1928, taps=3, stride=2, cpad=0, Bn=4, Tin=1925, Tout=962),
}


def conv_operands(name, dt):
    """x [Bn, Tin, G Cg] = randn times a power of two per frame, w [G N, Cg, taps] = randn times a power of two per
    output channel, both rounded to dt; bias = randn times the channel scale."""
    g = CONV_CASES[name]
    gen = torch.Generator().manual_seed(77 + g["Tin"])
    td = torch.float32 if dt == "f32" else torch.bfloat16
    r = torch.pow(2.0, torch.randint(-6, 7, (g["Bn"], g["Tin"], 1), generator=gen).float())
    c = torch.pow(2.0, torch.randint(-6, 7, (g["G"] * g["N"],), generator=gen).float())
    x = (torch.randn(g["Bn"], g["Tin"], g["G"] * g["Cg"], generator=gen) * r).to(td)
    w = (torch.randn(g["G"] * g["N"], g["Cg"], g["taps"], generator=gen) * c[:, None, None]).to(td)
    bias = torch.randn(g["G"] * g["N"], generator=gen) * c
    return x, w, bias


def conv_im2col(name, x, w):
    """The implicit GEMM's logical operands per group: A_z [Bn Tout, taps Cg] (row = frame, k = tap * Cg + c, zeros for
    taps outside the input) and B_z [N, taps Cg], in the dtype of x / w."""
    g = CONV_CASES[name]
    xp = torch.nn.functional.pad(x, (0, 0, g["cpad"], g["cpad"]))
    win = xp.unfold(1, g["taps"], g["stride"])[:, : g["Tout"]]               # [Bn, Tout, G Cg, taps]
    out = []
    for z in range(g["G"]):
        A = win[:, :, z * g["Cg"]:(z + 1) * g["Cg"], :].permute(0, 1, 3, 2).reshape(g["Bn"] * g["Tout"], -1)
        B = w[z * g["N"]:(z + 1) * g["N"]].permute(0, 2, 1).reshape(g["N"], -1)
        out.append((A, B))
    return out


def conv_ref(name, x, w, bias, dtype=torch.float64):
    """F.conv1d of the case in dtype and its error scale |x| * |w| + |bias|, both [Bn * Tout, G N] (rows = frames);
    x, w, bias on any device."""
    g = CONV_CASES[name]
    F = torch.nn.functional
    xt = x.to(dtype).transpose(1, 2)
    y = F.conv1d(xt, w.to(dtype), bias.to(dtype), stride=g["stride"], padding=g["cpad"], groups=g["G"])
    s = F.conv1d(xt.abs(), w.to(dtype).abs(), bias.to(dtype).abs(), stride=g["stride"], padding=g["cpad"], groups=g["G"])
    assert y.shape[-1] == g["Tout"], (y.shape, g["Tout"])
    return (y.transpose(1, 2).reshape(g["Bn"] * g["Tout"], -1), s.transpose(1, 2).reshape(g["Bn"] * g["Tout"], -1))


# ------------------------------------------------------------------ attention backward (csrc/attn7.hip, csrc/attention.hip)
# Reference, per-element units, rounding-point emulation, inputs and the case table shared by
# tests/test_cpu_attn_bwd_ref.py (which sets the constants below from the reference alone and proves with mutated
# references that the bound tells real bugs apart) and tests/test_gpu_attn_bwd.py (which runs the kernels).
U9 = 2.0 ** -9                 # half an ulp of bf16, relative
LOG2E_F32 = float(np.float32(1.4426950408889634))
LN2_F32 = float(np.float32(0.6931471805599453))
ATTN_SEED, ATTN_STREAM = 5, 9  # the dropout site of every attention-backward case


def attn_p32(p):
    """The dropout probability as the C ABI receives it."""
    return float(np.float32(p))


class AttnBwdTerms:
    """Float64 pieces of one attention backward: S, P, G, delta, T, PD (= P o D), D (float), c, and dq / dk / dv."""
    __slots__ = ("S", "P", "G", "delta", "T", "PD", "D", "c", "dq", "dk", "dv")


def attn_fwd_ref64(q, k, v, keep, drop_keep, p, scale, bias=None):
    """Float64 forward: q [B, H, Lq, 64], k, v [B, H, Lk, 64] (any float dtype), keep [B, Lk] bool or None, drop_keep
    [B, H, Lq, Lk] bool or None (oracle.attn_dropout_keep), bias [B, H, Lq, Lk] float64 or None (added to the scaled
    scores: WavLM's gate times its relative-position table). Returns O [B, H, Lq, 64] and LSE [B, H, Lq] (natural log
    of the scaled scores), both float64. A row without a kept key is NaN in both (softmax of all -inf), as in every
    kernel."""
    s = float(scale) * (q.double() @ k.double().transpose(-1, -2))
    if bias is not None:
        s = s + bias
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    lse = torch.where(torch.isinf(lse) & (lse < 0), torch.full_like(lse, float("nan")), lse)
    pr = torch.exp(s - lse[..., None])
    if drop_keep is not None:
        pr = pr * drop_keep.double() / (1.0 - float(p))
    return pr @ v.double(), lse


def attn_bwd_terms64(q, k, v, do, o, lse, keep, drop_keep, p, scale, *, c_on_g=True):
    """S, P, G, delta, T, PD of attn_bwd_ref64 (below), without the three products. c_on_g=False leaves the dropout
    scale off G (a mutant of tests/test_cpu_attn_bwd_ref.py)."""
    t = AttnBwdTerms()
    q, k, v, do, o, lse = (x.double() for x in (q, k, v, do, o, lse))
    t.c = 1.0 / (1.0 - float(p)) if drop_keep is not None else 1.0
    t.S = float(scale) * (q @ k.transpose(-1, -2))
    t.P = torch.exp(t.S - lse[..., None])
    if keep is not None:
        t.P = t.P * keep[:, None, None, :].double()
    t.D = drop_keep.double() if drop_keep is not None else torch.ones_like(t.P)
    t.G = do @ v.transpose(-1, -2)
    t.delta = (do * o).sum(-1)
    t.T = t.P * ((t.c if c_on_g else 1.0) * t.D * t.G - t.delta[..., None])
    t.PD = t.P * t.D
    return t


def attn_bwd_products64(t, q, k, do, scale):
    """dQ = s T K, dK = s T^T Q, dV = c (P o D)^T dO into t.dq / t.dk / t.dv; returns t."""
    t.dq = float(scale) * (t.T @ k.double())
    t.dk = float(scale) * (t.T.transpose(-1, -2) @ q.double())
    t.dv = t.c * (t.PD.transpose(-1, -2) @ do.double())
    return t


def attn_bwd_ref64(q, k, v, do, o, lse, keep, drop_keep, p, scale):
    """The operation fddm_attn_bwd defines, in float64 on the values the kernel receives: bf16 Q, K, V, dO, O as
    [B, H, L, 64] and the fp32 LSE [B, H, Lq] (O and LSE are inputs of the backward, not recomputed: the reference is
    exact for whatever forward produced them). keep [B, Lk] bool or None is the key mask M (keys past an extent are
    masked keys), drop_keep [B, H, Lq, Lk] bool or None the keep bits D of oracle.attn_dropout_keep, c = 1 / (1 - p)
    with p as given (attn_p32(p) is what the C ABI receives, a float32), s = scale:
        S = s Q K^T      P = exp(S - LSE), 0 where M is false      G = dO V^T
        delta_i = sum_d dO_id O_id      T = P o (c D o G - delta)
        dQ = s T K       dK = s T^T Q       dV = c (P o D)^T dO
    Returns an AttnBwdTerms. dK / dV rows of masked keys are exact zeros (their P column is)."""
    return attn_bwd_products64(attn_bwd_terms64(q, k, v, do, o, lse, keep, drop_keep, p, scale), q, k, do, scale)


def attn_bwd_units(t, q, k, v, do, o, scale):
    """Root-sum-square error units (b_dQ, b_dK, b_dV) of an AttnBwdTerms, for the check
        |gpu - ref| <= C u b + 2^-8 |ref|,   u = 2^-9.
    The bf16 rounding points of the kernels, each a relative error of at most u on the value it rounds:
      (1) Q' = bf16(Q s log2 e), the score operand (attn7.hip scale_frag: dq7 :588, bwdf7 :1035; dkv7 streams the Q'
          dq7 wrote, :725-729 / :790). It moves S_ik by sum_d dQ'_id K_kd, of root-sum-square size u a_ik with
          a_ik = s sqrt(sum_d Q_id^2 K_kd^2), and with it P_ik, T_ik and (P D)_ik by the factor a_ik u.
      (2) T packed to bf16 before the second MFMAs (dq7 :695, dkv7 :903-904, bwdf7 :1161-1165).
      (3) P o D packed to bf16 before the dV MFMA (dkv7 :901-902, bwdf7 :1159-1160); dq7 never rounds P itself.
      (4) dK formed from Q' (the ring's image, dkv7 :916-919, bwdf7 :1177-1180) and multiplied by ln 2 = s / (s log2 e)
          (:939, :1241): the rounding (1) enters dK a second time, as T_ik dQ'_id.
      (5) -LSE log2 e as a bf16 pair hi + lo (neg_split, dq7 :602; dkv7 :866-869; bwdf7 :1125-1128): 2^-18 |LSE| on the
          exponent, fp32-sized, not counted.
      (6) dQ, dK, dV rounded to bf16 (dq7 :739, dkv7 :949, bwdf7 :1218 / :1252): the 2^-8 |ref| term.
      (7) G_ik = sum_d dO_id V_kd (the dP MFMAs, dq7 :676, dkv7 :875, bwdf7 :1134) and delta_i = sum_d dO_id O_id (dq7
          :592-595, bwdf7 :1029-1033) are fp32 sums of 64 products each, subtracted from one another (:687-693, :894-897,
          :1152-1155). The fp32 rounding of a sum of n products is taken as sqrt(n) 2^-24 of the root-sum-square of
          the products (each of the n partial sums rounds once, and a partial sum grows like the root-sum-square), here
          2^-21 h_ik = 2^-12 u h_ik with h_ik^2 = sum_d dO_id^2 ((c D_ik V_kd)^2 + O_id^2). Next to (1) and (2) it is
          2^-12 of nothing in general; it is the whole error where c D G - delta cancels: an entry with one kept key
          and no dropout has O = V, T = 0 and dQ = dK = 0 in the reference, and the kernels' T is the difference of two
          fp32 sums taken in different orders.
    Everything else is fp32 and not counted: the score MFMA accumulators, exp2, the final scalings, the f32 dQ partial
    bwdf7 keeps in the workspace between its two key passes. dq2 / dkv2 (attention.hip :1099-1459) round at (2), (3),
    (6) and (7) only: the score operand is Q itself, S s log2 e - LSE log2 e is fp32 (:1490, :1668), dK = s T^T Q
    (:1711). With e_ik^2 = T_ik^2 (1 + a_ik^2) + (2^-12 P_ik h_ik)^2:
        b_dQ[i, d] = s sqrt(sum_k e_ik^2 K_kd^2)
        b_dK[k, d] = s sqrt(sum_i (e_ik^2 + T_ik^2) Q_id^2)
        b_dV[k, d] = c sqrt(sum_i (P D)_ik^2 (1 + a_ik^2) dO_id^2)"""
    q2, k2, v2, do2, o2 = (x.double() ** 2 for x in (q, k, v, do, o))
    s = float(scale)
    a2 = s * s * (q2 @ k2.transpose(-1, -2))
    T2 = t.T ** 2
    h2 = (t.c * t.D) ** 2 * (do2 @ v2.transpose(-1, -2)) + (do2 * o2).sum(-1)[..., None]
    e2 = T2 * (1.0 + a2) + 2.0 ** -24 * t.P ** 2 * h2
    b_dq = s * torch.sqrt(e2 @ k2)
    b_dk = s * torch.sqrt((e2 + T2).transpose(-1, -2) @ q2)
    b_dv = t.c * torch.sqrt((t.PD ** 2 * (1.0 + a2)).transpose(-1, -2) @ do2)
    return b_dq, b_dk, b_dv


def _bf(x):
    return x.to(torch.bfloat16).float()


def attn_bwd_emulate(q, k, v, do, o, lse, keep, drop_keep, p, scale, family="7"):
    """The kernels' rounding points in plain torch: fp32 where the kernel holds fp32, .to(bfloat16) at the points (1)-(6)
    of attn_bwd_units. family "7": bwdf7 / dq7 / dkv7; family "2": dq2 / dkv2 (no Q' rounding, fp32 LSE, dK from Q with
    the scale). Not modelled: the MFMA summation order, the hardware exp2, FMA contraction other than c D G - delta.
    It sets the constants ATTN_BWD_E and proves statements about inputs; it is no oracle for the kernels. Returns
    (dq, dk, dv) float32 holding bf16 values."""
    f32 = torch.float32
    q, k, v, do, o = (x.to(f32) for x in (q, k, v, do, o))
    sc = float(np.float32(scale))
    sl2 = float(np.float32(sc * LOG2E_F32))
    lse2 = lse.to(f32) * LOG2E_F32
    if family == "7":
        qp = _bf(q * sl2)
        hi = _bf(-lse2)
        lo = _bf(-lse2 - hi)
        arg = (hi + lo)[..., None] + qp @ k.transpose(-1, -2)
    else:
        qp = q
        arg = (q @ k.transpose(-1, -2)) * sl2 - lse2[..., None]
    P = torch.exp2(arg)
    if keep is not None:
        P = P * keep[:, None, None, :].to(f32)
    G = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1)
    if drop_keep is not None:
        c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        D = drop_keep.to(f32)
        X = (G.double() * D.double() * c - delta.double()[..., None]).to(f32)      # one fmaf
    else:
        c, D = 1.0, torch.ones_like(P)
        X = G - delta[..., None]
    T = _bf(P * X)
    PD = _bf(P * D)
    dq = _bf((T @ k) * sc)
    dk = _bf((T.transpose(-1, -2) @ qp) * (LN2_F32 if family == "7" else sc))
    dv = _bf((PD.transpose(-1, -2) @ do) * c)
    if keep is not None:       # masked keys: the kernels store zeros whatever the accumulators hold
        z = keep[:, None, :, None].to(f32)
        dk, dv = dk * z, dv * z
    return dq, dk, dv


def attn_bwd_excess(got, ref, b):
    """(|got - ref| - 2^-8 |ref|)+ in units of u b, per element; 0 where b == 0 and got == ref, inf where b == 0 and
    they differ. The check |got - ref| <= C u b + 2^-8 |ref| is attn_bwd_excess <= C."""
    x = ((got.double() - ref).abs() - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    out = x / (U9 * b)
    out = torch.where(b == 0, torch.where(x == 0, torch.zeros_like(x), torch.full_like(x, float("inf"))), out)
    return out


# The largest error of attn_bwd_emulate against attn_bwd_ref64 in units of u b (after the 2^-8 |ref| term), over every
# case of attn_bwd_cases() and every input set, per kernel family and output, measured on the CPU
# (tests/test_cpu_attn_bwd_ref.py asserts the measured values stay at or below these). The kernels are allowed
# ATTN_BWD_C = 2 E units: what the emulation leaves out is fp32-sized (about 2^-15 of the counted terms), and a flipped
# bf16 tie of T is a counted term, so the factor covers only the tail between one sample of roundings and another.
# Measured: family 7 (bwdf7, dq7 / dkv7) dq 3.85, dk 4.00, dv 3.95; family 2 (dq2 with dkv2 or dkv4) dq 2.27, dk 2.36,
# dv 2.60; the constants keep about 10 % headroom.
ATTN_BWD_E = {"7": dict(dq=4.2, dk=4.4, dv=4.3), "2": dict(dq=2.5, dk=2.6, dv=2.8)}
ATTN_BWD_C = {f: {n: 2.0 * e for n, e in d.items()} for f, d in ATTN_BWD_E.items()}

ATTN_EDGE_KEYS = (0, 31, 32, 63, 64, 127, 128, 255, 256)
ATTN_EDGE_QUERIES = (0, 31, 32, 63, 64, 127, 128)
ATTN_EDGE_DO = 32.0            # dO rows of edge queries, a power of two
ATTN_EDGE_QSTD = 0.5           # the random part of every query
ATTN_EDGE_QW = 4.0             # every query's component along w
ATTN_EDGE_MASS = 1.0           # edge keys : other keys, the ratio of probability mass the edge keys are sized for


def attn_bwd_mask(B, Lk, ext=None):
    """The key masks of the cases (tests/test_gpu_lengths.py's): keep [B, Lk] bool.
    ext given (length-bounded cases): keys below each entry's extent, with a hole of three keys (10..12) and a whole
    masked 64-key tile (64..127) in entry 0 and the key before the last masked in the last entry.
    ext None: entry 0 gets the same holes, the last entry a padded tail of 9 keys and the key before its last masked.
    Every hole stays inside the kept range; an entry never loses its last key (or its only one)."""
    e = torch.tensor(ext if ext is not None else [Lk] * (B - 1) + [max(1, Lk - 9)])
    keep = torch.arange(Lk)[None, :] < e[:, None]
    e0, el = int(e[0]), int(e[B - 1])
    if e0 > 13:
        keep[0, 10:13] = False
    if e0 > 128:
        keep[0, 64:128] = False
    if el >= 3:
        keep[B - 1, el - 2] = False
    return keep


def _attn_edge_keys(keep_b, Lk):
    """Edge keys of one entry: ATTN_EDGE_KEYS, Lk - 1, extent - 1 and the key after each hole, where kept."""
    kept = keep_b.nonzero().flatten().tolist()
    last = kept[-1]
    edges = set(ATTN_EDGE_KEYS) | {Lk - 1, last}
    edges |= {j for j in kept if j > 0 and not keep_b[j - 1]}
    return sorted(j for j in edges if j <= last and keep_b[j])


def _c(fam, Lq, Lk, masked, p, *, ext=None, force="auto", rehash=False, strided=False, guard=False, peaked=False,
       B=2, H=2, chain=False):
    """One case. fam: "bwdf7" | "pair7" | "pair2"; expect: what ops.attn_last_path()["bwd"] must read."""
    kx = ext is not None
    if kx:
        B, masked = len(ext), True
    dm = 0 if p == 0 else 1
    if fam == "bwdf7":
        expect = ("bwdf7", dm, int(masked), 0, 1 if Lk <= 256 else 2, kx)
    elif fam == "pair7":
        mk = 2 if masked else 1 if Lk % 64 else 0
        expect = ("dq7+dkv7", dm, mk, int(masked), 0, kx)
    else:
        # the dK / dV launch is chosen on its own (attention.hip run<>, which == 2): dkv2 when it rehashes or Lq > 1024,
        # else the round-4 dkv4, which is therefore what the default dispatch runs beside dq2 at Lk > 1024
        dm = 0 if p == 0 else 1 if rehash else 2
        expect = ("dq2+dkv2" if rehash or Lq > 1024 else "dq2+dkv4", dm, int(masked or Lk % 64 != 0), 0, 0, False)
    cid = (f"{fam}-{Lq}x{Lk}" + ("-" + "_".join(map(str, ext)) if kx else "") + ("-mask" if masked and not kx else "")
           + (f"-p{p}" if p else "") + ("-rehash" if rehash else "") + (f"-{force}" if force != "auto" else "")
           + ("-strided" if strided else "") + ("-guard" if guard else "") + ("-peaked" if peaked else ""))
    return dict(id=cid, fam=fam, family="2" if fam == "pair2" else "7", B=B, H=H, Lq=Lq, Lk=Lk, masked=masked, p=p,
                ext=ext, force=force, rehash=rehash, strided=strided, guard=guard, peaked=peaked, expect=expect,
                chain=chain or kx)


ATTN_KX = {200: [200, 1, 63, 64, 65, 129], 300: [300, 257, 256, 70]}   # one, then two, live key passes of bwdf7


def attn_bwd_cases():
    """Every case of tests/test_gpu_attn_bwd.py: the smallest shapes at which each mechanism of each backward kernel
    exists (B H <= 8). guard: dq / dk / dv are column slices of wider NaN-filled buffers; strided: q, k, v are column
    slices of one [rows, 3 H 64] buffer; chain: the case also runs behind ops.attn_fwd (fwd7 and forced fwd8)."""
    cs = []
    n = 0
    for fam, force, shapes in (
            # one key pass: one query and key | a partial 32-query group, five keys | two query tiles, 17 keys | exactly
            # one tile | three query tiles, ragged fourth key tile | four full tiles of each
            ("bwdf7", "auto", ((1, 1), (33, 5), (65, 17), (64, 64), (129, 200), (256, 256))),
            # two key passes: one key in the second | a ragged second pass | both full
            ("bwdf7", "auto", ((40, 257), (129, 300), (256, 512))),
            # the split pair by default: Lq > 256 (MK 0 and MK 1) | 512 < Lk <= 1024 (MK 1 and MK 0)
            ("pair7", "auto", ((257, 64), (300, 200), (40, 513), (96, 1024))),
            # ... and forced at the fused launch's shapes
            ("pair7", "nofused", ((65, 17), (129, 200), (129, 300)))):
        for Lq, Lk in shapes:
            for masked in (False, True):
                for p in (0.0, 0.1):
                    cs.append(_c(fam, Lq, Lk, masked, p, force=force, guard=p > 0 and masked,
                                 chain=n % 4 == (n // 4) % 4))     # one of a shape's four variants, in rotation
                    n += 1
    for fam, force in (("bwdf7", "auto"), ("pair7", "nofused")):
        for Lk, ext in ATTN_KX.items():
            for p in (0.0, 0.1):
                cs.append(_c(fam, 129, Lk, True, p, ext=ext, force=force, H=1 if Lk == 200 else 2, guard=p > 0))
        # q, k, v from one fused-projection buffer; a peaked softmax (flat inputs with q x 3)
        cs.append(_c(fam, 129, 200, True, 0.1, force=force, strided=True, chain=True))
        cs.append(_c(fam, 129, 200, True, 0.1, force=force, peaked=True))
    # dq2 (+ dkv4 up to Lq 1024, dkv2 beyond): Lk > 1024 with recorded bits (DM 2) and without dropout (DM 0): one key in
    # the 17th tile | two query blocks, 18 tiles | Lk a multiple of 64 (the unmasked builds); dq2 + dkv2 at any Lk when
    # the kernels rehash (DM 1)
    for Lq, Lk in ((40, 1025), (130, 1100)):
        for masked in (False, True):
            for p in (0.0, 0.1):
                cs.append(_c("pair2", Lq, Lk, masked, p, guard=p > 0 and masked))
    for p in (0.0, 0.1):
        cs.append(_c("pair2", 40, 1088, False, p, B=1))
        # Lq > 1024 as well: dkv2 without dropout and with recorded bits (17 query tiles, one query in the last)
        cs.append(_c("pair2", 1025, 1088, False, p, B=1, H=1))
        cs.append(_c("pair2", 1025, 1030, p > 0, p, B=1, H=1, guard=p > 0))
    for Lq, Lk in ((130, 70), (64, 128)):
        for masked in (False, True):
            cs.append(_c("pair2", Lq, Lk, masked, 0.1, rehash=True, guard=masked))
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


# the template builds the case table must reach (attention.hip run<>, attn7.hip attn7_bwdf / attn7_dq / attn7_dkv), as
# ops.attn_last_path()["bwd"] reads them: every (MASK / MK, NP, KX) combination with and without dropout
ATTN_BWD_BUILDS = (
    [("bwdf7", dm, mask, 0, np_, False) for dm in (0, 1) for mask in (0, 1) for np_ in (1, 2)] +
    [("bwdf7", dm, 1, 0, np_, True) for dm in (0, 1) for np_ in (1, 2)] +
    # dq7 <DM, MK, KX> with dkv7 <DM, MASK, KX>: MASK = a mask was passed, which is MK == 2
    [("dq7+dkv7", dm, mk, int(mk == 2), 0, False) for dm in (0, 1) for mk in (0, 1, 2)] +
    [("dq7+dkv7", dm, 2, 1, 0, True) for dm in (0, 1)] +
    [("dq2+dkv2", dm, mask, 0, 0, False) for dm in (0, 1, 2) for mask in (0, 1)] +
    # dq2 <DM, MASK> beside dkv4 <DM>: Lk > 1024 with Lq <= 1024
    [("dq2+dkv4", dm, mask, 0, 0, False) for dm in (0, 2) for mask in (0, 1)])


@functools.lru_cache(maxsize=None)
def attn_bwd_case_inputs(cid, kind):
    """Inputs of case `cid` for input set `kind`, built once and never modified: a dict of
      q, do [B, Lq, H 64], k, v [B, Lk, H 64] float32 holding bf16 values; keep [B, Lk] bool or None; drop [B, H, Lq, Lk]
      bool or None (the oracle's keep bits at ATTN_SEED / ATTN_STREAM); edge_keys (per entry), edge_queries.
    "flat": randn q, k, v, dO (q x 3 in a peaked case).
    "edges": q = 0.5 randn + 4 w for one unit vector w (64 entries of +-1/8), every edge key of an entry (ATTN_EDGE_KEYS,
      Lk - 1, each extent - 1, the key after each hole) gets + beta w with beta = 2 ln(kept keys / edge keys), so that
      the edge keys together hold about half of each row's probability mass (the extra scaled score of an edge key is
      beta / 2); masked keys get the same + beta w (no effect on the reference; a kernel that keeps one shows it);
      dO rows of the edge queries (ATTN_EDGE_QUERIES, Lq - 1) are multiplied by ATTN_EDGE_DO = 32. The halved random
      part of q keeps the edge keys' probabilities within a factor of about two of one another (at full size the
      scores' randn part spreads them over e^+-1.1 and a single edge key often carries too little of its row), the
      factor 32 lets the at most 8 edge queries outweigh up to 248 others in dK and dV: with 4 w on a full-size q and a
      factor 8 the mutants of tests/test_cpu_attn_bwd_ref.py left the bound on 0.47-0.56 of their elements at
      Lk >= 300, with these on 0.64 or more."""
    import math
    from oracle import fddm_oracle as O
    c = {x["id"]: x for x in attn_bwd_cases()}[cid]
    B, H, Lq, Lk, p = c["B"], c["H"], c["Lq"], c["Lk"], c["p"]
    gen = torch.Generator().manual_seed(7919 * Lq + 31 * Lk + (1 if kind == "edges" else 0))
    q, k, v, do = (torch.randn(B, L, H, 64, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = attn_bwd_mask(B, Lk, c["ext"]) if c["masked"] else None
    full = torch.ones(B, Lk, dtype=torch.bool) if keep is None else keep
    ek = [_attn_edge_keys(full[b], Lk) for b in range(B)]
    eq = sorted({j for j in ATTN_EDGE_QUERIES + (Lq - 1,) if j < Lq})
    if kind == "edges":
        w = (torch.randint(0, 2, (64,), generator=gen).float() * 2.0 - 1.0) / 8.0
        q = ATTN_EDGE_QSTD * q + ATTN_EDGE_QW * w
        for b in range(B):
            nk = int(full[b].sum())
            beta = max(0.0, 8.0 / ATTN_EDGE_QW * math.log(ATTN_EDGE_MASS * nk / len(ek[b])))
            k[b, ek[b]] += beta * w
            k[b, (~full[b]).nonzero().flatten()] += beta * w
        do[:, eq] *= ATTN_EDGE_DO
    elif c["peaked"]:
        q = q * 3.0
    rnd = lambda x, L: x.to(torch.bfloat16).float().reshape(B, L, H * 64)  # noqa: E731
    drop = O.attn_dropout_keep(ATTN_SEED, ATTN_STREAM, B, H, Lq, Lk, p) if p > 0 else None
    return dict(q=rnd(q, Lq), k=rnd(k, Lk), v=rnd(v, Lk), do=rnd(do, Lq), keep=keep, drop=drop, edge_keys=ek,
                edge_queries=eq)


def attn_heads(x, B, H):
    """[B, L, H 64] or [B L, H 64] -> [B, H, L, 64]."""
    return x.reshape(B, -1, H, 64).transpose(1, 2)


def attn_rows(t):
    """[B, H, L, 64] -> [B L, H 64]."""
    B, H, L, _ = t.shape
    return t.transpose(1, 2).reshape(B * L, H * 64)


@functools.lru_cache(maxsize=None)
def attn_bwd_case_ref(cid, kind):
    """The isolated mode's O = bf16(float64 forward) and LSE = fp32(float64 LSE) of a case, with the float64 reference
    of the backward that receives them and its units: (o [B, H, Lq, 64] float32 holding bf16 values, lse [B, H, Lq]
    float32, out64 [B, H, Lq, 64], lse64, AttnBwdTerms, (b_dQ, b_dK, b_dV)). Built once, never modified."""
    c = {x["id"]: x for x in attn_bwd_cases()}[cid]
    x = attn_bwd_case_inputs(cid, kind)
    B, H = c["B"], c["H"]
    q, k, v, do = (attn_heads(x[n], B, H) for n in ("q", "k", "v", "do"))
    o64, lse64 = attn_fwd_ref64(q, k, v, x["keep"], x["drop"], attn_p32(c["p"]), 0.125)
    o, lse = o64.to(torch.bfloat16).float(), lse64.float()
    t = attn_bwd_ref64(q, k, v, do, o, lse, x["keep"], x["drop"], attn_p32(c["p"]), 0.125)
    return o, lse, o64, lse64, t, attn_bwd_units(t, q, k, v, do, o, 0.125)


# ------------------------------------------------------------ WavLM front end (csrc/wavlm.hip, csrc/posconv.hip)
# Reference, per-element bounds, inputs and case tables shared by tests/test_cpu_wavlm_front_ref.py (which sets the
# constants below from the reference alone) and tests/test_gpu_wavlm_front.py (which runs the kernels).
def bf16_round_bound(ref, b):
    """b plus one rounding to nearest bf16 of a value within b of ref: b + 2^(floor(log2(|ref| + b)) - 8), the exact
    half ulp (0 where |ref| + b is 0)."""
    m = ref.abs() + b
    _, e = torch.frexp(m)                      # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    half = torch.ldexp(torch.ones_like(m), e - 9)
    return b + torch.where(m > 0, half, torch.zeros_like(m))


def _bf32(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


class Conv0Ref:
    """y, ya = |x| * |w| [B, T0, C]; sc, sh [B, C]; z = sc y + sh with error scale s; ref = gelu(z); lin = |gelu'(z)|."""
    __slots__ = ("y", "ya", "sc", "sh", "z", "s", "ref", "lin")


class PosconvRef:
    """y [B, S, E] with error scale s; ref = gelu(y); lin = |gelu'(y)|; full: the S + 1 frames of the padded conv."""
    __slots__ = ("y", "s", "ref", "lin", "full")


class GateRef:
    """pa, pb [B, S, H] with error scales sa, sb; ref [B, H, S]; da, db = |d gate / d pa|, |d gate / d pb|; A: the
    absolute allowance."""
    __slots__ = ("pa", "pb", "sa", "sb", "ref", "da", "db", "A")


# ---- conv layer 0 + GroupNorm + GELU
CONV0_K, CONV0_S, CONV0_EPS, CONV0_TAIL = 10, 5, 1e-5, 3
CONV0_KINDS = {"loud": (3.0, 0.0), "plain": (0.1, 0.0), "dc": (0.05, 0.4), "quiet": (1e-4, 0.0), "silent": (0.0, 0.0)}
CONV0_MIX = ("loud", "plain", "dc")
CONV0_EXPOSED = ("dc", "quiet", "silent")
# (id, path, C, T0s, utterance kinds): path "mfma" (bf16 out, C % 512 == 0), "f32" (conv0_apply<float>), "bf16"
# (conv0_apply<bf16_t>)
CONV0_CASES = [
    ("mfma-tile", "mfma", 512, (1, 8, 9, 16, 17), CONV0_MIX),       # both store halves empty, full, and the tile edge
    ("mfma-block", "mfma", 512, (512, 513), CONV0_MIX),             # second frame block holds one frame
    ("mfma-exposed", "mfma", 512, (600,), CONV0_EXPOSED),           # exposed regimes of the split and the variance
    ("mfma-z1", "mfma", 1024, (40,), CONV0_MIX),                    # blockIdx.z = 1
    ("f32-block", "f32", 512, (63, 64, 65), CONV0_MIX),             # 64-frame apply block edge
    ("f32-loop", "f32", 1024, (20,), CONV0_MIX),                    # second trip of the channel loop
    ("f32-idle", "f32", 6, (20,), CONV0_MIX),                       # most threads idle
    ("f32-exposed", "f32", 512, (600,), CONV0_EXPOSED),
    ("bf16-apply", "bf16", 64, (65,), ("loud", "dc")),            # bf16 apply path
    ("stats", "f32", 64, (4096, 4097, 8193), ("plain", "dc")),    # one full statistics block; + one frame; three blocks
]


@functools.lru_cache(maxsize=None)
def conv0_params(C):
    """w [C, 10] = 0.3 randn times a power of two per channel (2^-3 .. 2^3), gamma = 1 + 0.1 randn, beta = 0.1 randn."""
    gen = torch.Generator().manual_seed(4000 + C)
    w = 0.3 * torch.randn(C, CONV0_K, generator=gen) * torch.pow(2.0, torch.randint(-3, 4, (C, 1), generator=gen).float())
    return w, 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)


@functools.lru_cache(maxsize=None)
def conv0_wave(kinds, T0):
    """[B, nsamp] f32, one utterance per kind; nsamp = (T0 - 1) 5 + 10 + 3: the last three samples reach no frame."""
    nsamp = (T0 - 1) * CONV0_S + CONV0_K + CONV0_TAIL
    gen = torch.Generator().manual_seed(77 * T0 + len(kinds))
    return torch.stack([CONV0_KINDS[k][0] * torch.randn(nsamp, generator=gen) + CONV0_KINDS[k][1] for k in kinds])


def conv0_terms64(wave, w):
    """(y, |x| * |w|) [B, T0, C] float64 on wave's device."""
    conv = torch.nn.functional.conv1d
    x, wd = wave.double()[:, None], w.double().to(wave.device)[:, None]
    return conv(x, wd, stride=CONV0_S).transpose(1, 2), conv(x.abs(), wd.abs(), stride=CONV0_S).transpose(1, 2)


def conv0_affine64(y, gamma, beta, eps=CONV0_EPS, unbiased=False):
    """(mean, var, sc, sh) [B, C] of y [B, T, C]: the GroupNorm with one channel per group, folded."""
    mean = y.mean(1)
    var = y.var(1, unbiased=unbiased) if y.shape[1] > 1 else torch.zeros_like(mean)
    sc = gamma.double().to(y.device) / torch.sqrt(var + eps)
    return mean, var, sc, beta.double().to(y.device) - mean * sc


def conv0_out64(y, ya, sc, sh):
    r = Conv0Ref()
    r.y, r.ya, r.sc, r.sh = y, ya, sc, sh
    r.z = sc[:, None, :] * y + sh[:, None, :]
    r.s = sc.abs()[:, None, :] * ya + sh.abs()[:, None, :]
    r.ref = torch.nn.functional.gelu(r.z)
    r.lin = gelu_grad64(r.z).abs()
    return r


def conv0_ref64(wave, w, gamma, beta):
    y, ya = conv0_terms64(wave, w)
    _, _, sc, sh = conv0_affine64(y, gamma, beta)
    return conv0_out64(y, ya, sc, sh)


def conv0_bound(r, path):
    """Per-element bound of conv0_gn_gelu's output on kernel path "f32" / "bf16" / "mfma"."""
    if path == "mfma":
        b = r.lin * (FRONT_C["conv0_split"] * U18) * r.s + GEMM_GELU_BF16OUT_ABS
    else:
        b = r.lin * (FRONT_C["conv0_f32"] * U24) * r.s + (GEMM_GELU_ABS if path == "f32" else GEMM_GELU_BF16OUT_ABS)
    return b if path == "f32" else bf16_round_bound(r.ref, b)


def conv0_scsh32(y, gamma, beta):
    """f32 (sc, sh) as conv0_gn_affine makes them from float64 statistics."""
    mean, var, _, _ = conv0_affine64(y, gamma, beta)
    rstd = (1.0 / torch.sqrt(var + float(np.float32(CONV0_EPS)))).float()
    sc = rstd * gamma.float()
    return sc, beta.float() - mean.float() * sc


def _conv0_frames(wave):
    T0 = (wave.shape[1] - CONV0_K) // CONV0_S + 1
    return wave.float().unfold(1, CONV0_K, CONV0_S)[:, :T0]            # [B, T0, K]


def conv0_emulate_apply(wave, w, sc, sh):
    """z as conv0_apply forms it: ten fp32 FMAs in tap order, then fma(y, sc, sh)."""
    X, wf = _conv0_frames(wave), w.float()
    y = torch.zeros(X.shape[0], X.shape[1], wf.shape[0])
    for k in range(CONV0_K):
        y = _fma32(wf[None, None, :, k], X[:, :, k, None], y)
    return _fma32(y, sc[:, None, :], sh[:, None, :])


def conv0_emulate_mfma(wave, w, sc, sh, drop_xlo=False):
    """z as conv0_mfma forms it: v = f32(sc w); x, v and sh split into bf16 hi + lo; the 32 products (exact in fp32) of
    the row [x_hi x_lo x_hi 1 1] . [v_hi v_hi v_lo sh_hi sh_lo] added in order in fp32."""
    X = _conv0_frames(wave)
    xh = _bf32(X)
    xl = _bf32(X - xh)
    v = sc[:, :, None] * w.float()[None]                               # [B, C, K]
    vh = _bf32(v)
    vl = _bf32(v - vh)
    shh = _bf32(sh)
    shl = _bf32(sh - shh)
    acc = torch.zeros(X.shape[0], X.shape[1], v.shape[1])
    for xa, va in ((xh, vh), (xl, vh), (xh, vl)):
        if drop_xlo and xa is xl:
            continue
        for k in range(CONV0_K):
            acc = acc + xa[:, :, k, None] * va[:, None, :, k]
    return (acc + shh[:, None, :]) + shl[:, None, :]


# ---- positional conv + GELU
# (Cg, kp, G, B, S)
POSCONV_CASES = [
    (16, 8, 3, 2, 3),       # <1>, single weight stage, S shorter than the padding
    (16, 16, 2, 2, 257),    # two stages; second block holds one frame
    (32, 12, 2, 2, 256),    # <2>, three stages, exactly one block
    (48, 8, 1, 3, 1),       # <3>, S = 1
    (48, 128, 2, 2, 499),   # the model's group geometry and length, 48 stages, taps straddling stages
    (64, 2, 2, 2, 255),     # <4>, single stage, kp = 2
    (64, 128, 2, 2, 300),   # <4>, WavLM-Large group geometry, two blocks
]
# Frame scales are 2^-2 .. 2^2 except here. With 128 taps every output has some 2^2 frames in its window, and of
# K = 8192 one term of a quieter frame is then worth less than the bf16 output's half ulp: over 2^-2 .. 2^2 a dropped
# (tap, channel) term left the bound on 0.47 - 0.50 of its elements whichever term it was, over 2^-1 .. 2^1 on
# 0.54 - 0.56 (tests/test_cpu_wavlm_front_ref.py asserts it).
POSCONV_FS_MAX = {(64, 128, 2, 2, 300): 1}


@functools.lru_cache(maxsize=None)
def posconv_operands(Cg, kp, G, B, S):
    """x [B, S, E] bf16 = randn times a power of two per frame (2^-2 .. 2^2, POSCONV_FS_MAX); w [E, Cg, kp] bf16 (Conv1d
    layout) = randn / sqrt(Cg kp) times a power of two per output channel (2^-6 .. 2^6); bias [E] f32 = randn times that scale."""
    E = G * Cg
    gen = torch.Generator().manual_seed(100003 * Cg + 1009 * kp + 97 * G + S)
    fm = POSCONV_FS_MAX.get((Cg, kp, G, B, S), 2)
    fs = torch.pow(2.0, torch.randint(-fm, fm + 1, (B, S, 1), generator=gen).float())
    cs = torch.pow(2.0, torch.randint(-6, 7, (E,), generator=gen).float())
    x = (torch.randn(B, S, E, generator=gen) * fs).to(torch.bfloat16)
    w = (torch.randn(E, Cg, kp, generator=gen) / (Cg * kp) ** 0.5 * cs[:, None, None]).to(torch.bfloat16)
    return x, w, torch.randn(E, generator=gen) * cs


def posconv_pack(w, G):
    """Conv1d weight [E, Cg, kp] -> the kernel's [G, Cg, kp * Cg] (tap-major K)."""
    E, Cg, kp = w.shape
    return w.view(G, Cg, Cg, kp).permute(0, 1, 3, 2).reshape(G, Cg, kp * Cg).contiguous()


def posconv_out64(y, s):
    r = PosconvRef()
    r.y, r.s = y, s
    r.ref = torch.nn.functional.gelu(y)
    r.lin = gelu_grad64(y).abs()
    return r


def posconv_ref64(x, w, bias, G, device=None):
    """Float64 reference [B, S, E] on `device`; r.full keeps the S + 1 frames of the padded conv (SamePad drops the last)."""
    conv = torch.nn.functional.conv1d
    kp = w.shape[2]
    xd, wd, bd = (t.to(device).double() for t in (x, w, bias))
    full = conv(xd.transpose(1, 2), wd, bd, padding=kp // 2, groups=G).transpose(1, 2)
    s = conv(xd.abs().transpose(1, 2), wd.abs(), bd.abs(), padding=kp // 2, groups=G).transpose(1, 2)[:, :-1]
    r = posconv_out64(full[:, :-1], s)
    r.full = full
    return r


def posconv_bound(r):
    return bf16_round_bound(r.ref, r.lin * (FRONT_C["posconv"] * U24) * r.s + GEMM_GELU_ABS)


def posconv_im2col(x, w, G):
    """Per group (A [B * S, kp * Cg], W [Cg, kp * Cg]) in the operands' dtype, K tap-major as the kernel walks it."""
    E, Cg, kp = w.shape
    B, S, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, kp // 2, kp // 2))
    win = xp.unfold(1, kp, 1)[:, :S]                                   # [B, S, E, kp]
    Wp = posconv_pack(w, G)
    return [(win[:, :, g * Cg:(g + 1) * Cg].permute(0, 1, 3, 2).reshape(B * S, kp * Cg), Wp[g]) for g in range(G)]


def posconv_emulate(x, w, bias, G):
    """fp32 in the kernel's order: 32-wide K chunks (one MFMA each, products of two bf16 exact) added in order, then the
    bias. [B, S, E] float32."""
    B, S, E = x.shape
    cols = []
    for A, Wg in posconv_im2col(x, w, G):
        A, Wg = A.float(), Wg.float()
        acc = torch.zeros(A.shape[0], Wg.shape[0])
        for k in range(0, A.shape[1], 32):
            acc = acc + A[:, k:k + 32] @ Wg[:, k:k + 32].t()
        cols.append(acc)
    return (torch.cat(cols, 1) + bias.float()[None, :]).view(B, S, E)


# ---- gated relative-position gate
# (dtype, B, S, H, dh)
GATE_CASES = [
    ("f32", 2, 100, 3, 64),     # 600 entries, three blocks, the last ragged
    ("bf16", 2, 100, 3, 64),    # H not a power of two: e / H and e % H matter
    ("bf16", 3, 43, 5, 32),     # narrower head
    ("f32", 1, 7, 2, 8),        # one partial block, the narrowest head
    ("bf16", 2, 128, 1, 64),    # exactly one full block
]


@functools.lru_cache(maxsize=None)
def gate_operands(dt, B, S, H, dh):
    """x [B * S, H dh] randn (rounded to bf16 for "bf16"), W [8, dh] = 0.2 randn times a power of two per row
    (2^-2 .. 2^2), bias = 0.5 randn, cst = 0.5 + rand, distinct per head."""
    gen = torch.Generator().manual_seed(7919 * B + 131 * S + 17 * H + dh + (dt == "bf16"))
    x = torch.randn(B * S, H * dh, generator=gen).to(torch.bfloat16 if dt == "bf16" else torch.float32)
    W = 0.2 * torch.randn(8, dh, generator=gen) * torch.pow(2.0, torch.randint(-2, 3, (8, 1), generator=gen).float())
    return x, W, 0.5 * torch.randn(8, generator=gen), 0.5 + torch.rand(H, generator=gen)


def gate_out64(p, sp, cst):
    """p, sp [B, S, H, 8] float64 (pre-activations and their error scales), cst [H] -> GateRef with ref [B, H, S]."""
    r = GateRef()
    c = cst.double().to(p.device)[None, None, :]
    r.pa, r.pb = p[..., :4].sum(-1), p[..., 4:].sum(-1)
    r.sa, r.sb = sp[..., :4].sum(-1), sp[..., 4:].sum(-1)
    ga, gb = torch.sigmoid(r.pa), torch.sigmoid(r.pb)
    r.ref = (ga * (gb * c - 1.0) + 2.0).transpose(1, 2)
    r.da = (ga * (1 - ga) * (gb * c - 1.0)).abs()
    r.db = (ga * c * gb * (1 - gb)).abs()
    # fast exp: (|p| + 4) u relative on e^-p through sigma (1 - sigma); then the closing arithmetic
    r.A = U24 * ((r.pa.abs() + 4) * r.da + (r.pb.abs() + 4) * r.db + 4 * ((ga * gb * c).abs() + ga.abs() + 2.0))
    return r


def gate_ref64(x, W, bias, cst, B, S, H):
    xh = x.double().view(B, S, H, -1)
    Wd, bd = W.double().to(x.device), bias.double().to(x.device)
    return gate_out64(xh @ Wd.t() + bd, xh.abs() @ Wd.abs().t() + bd.abs(), cst)


def gate_bound(r, C=None):
    """[B, H, S], laid out as the output."""
    C = FRONT_C["gate"] if C is None else C
    return ((r.da * r.sa + r.db * r.sb) * (C * U24) + r.A).transpose(1, 2)


def gate_emulate(x, W, bias, cst, B, S, H):
    """fp32 in the kernel's order: per output, fma over the head's channels in order starting from the bias; the two
    sums of four; torch.exp in fp32. Returns (pa, pb [B, S, H], gate [B, H, S]) float32."""
    xh, Wf = x.float().view(B, S, H, -1), W.float()
    r = bias.float().expand(B, S, H, 8).contiguous()
    for d in range(xh.shape[-1]):
        r = _fma32(Wf[:, d], xh[..., d, None], r)
    pa = ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]
    pb = ((r[..., 4] + r[..., 5]) + r[..., 6]) + r[..., 7]
    ga, gb = 1.0 / (1.0 + torch.exp(-pa)), 1.0 / (1.0 + torch.exp(-pb))
    return pa, pb, (ga * (gb * cst.float()[None, None, :] - 1.0) + 2.0).transpose(1, 2)


# ------------------------------------------------- attention forward (csrc/attn7.hip, csrc/attn8.hip, csrc/attention.hip)
# Reference, per-element units per kernel family, rounding-point emulation, inputs and the case table shared by
# tests/test_cpu_attn_fwd_ref.py (which sets ATTN_FWD_E from the reference alone and proves with mutated references that
# the bound tells real bugs apart) and tests/test_gpu_attn_fwd.py (which runs the kernels). DESIGN.md 4.10.
class AttnFwdRef:
    """Float64 pieces of one attention forward: S (scores with the bias, -inf at masked keys), P, D (c times the keep
    bits, or None), c, O, LSE, m (row maximum of S), g / dg (the gate [B, H, L] and its own bound, or None), T (the
    table gathered to [H, L, L], or None)."""
    __slots__ = ("S", "P", "D", "c", "O", "LSE", "m", "g", "dg", "T")


def attn_rel_index(L):
    """[L, L]: the table column of (query i, key k), k - i + L - 1 (HF modeling_wavlm.py:474-513 through
    models/wavlm.py's table layout; csrc/attn7.hip :176)."""
    return torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1


def attn_fwd_gate64(src, B, H, L, *, gate=None, graw=None, x=None, gw=None, gconst=None):
    """The query gate of WavLM's biased attention in float64 on the kernel's own inputs, and the bound dg of the
    kernel's gate against it (gate_bound: the form and the constant pinned for fddm_wavlm_gate; the in-kernel forms
    compute the same expression with the same __expf). Both [B, H, L].
      "gate": the precomputed fp32 row [B H, L] as given, dg = 0;
      "graw": the 4 + 4 bf16 pre-activations [B L, >= 8 H] summed, two sigmoids, ga (gb gconst[h] - 1) + 2
              (attn7.hip :280-288, attention.hip :586-594);
      "gx":   x [B L, >= 64 H] (bf16) against models.wavlm._fold_gate's 130 floats (attn7.hip :289-311,
              attention.hip :597-624)."""
    if src == "gate":
        g = gate.double().reshape(B, H, L)
        return g, torch.zeros_like(g)
    if src == "graw":
        p = graw.double()[:, :H * 8].reshape(B, L, H, 8)
        sp = p.abs()
    else:
        xh, w = x.double()[:, :H * 64].reshape(B, L, H, 64), gw.double()
        p = torch.zeros(B, L, H, 8, dtype=torch.float64)
        sp = torch.zeros_like(p)
        for j, (lo, bi) in enumerate(((0, 128), (64, 129))):
            p[..., 4 * j] = xh @ w[lo:lo + 64] + w[bi]
            sp[..., 4 * j] = xh.abs() @ w[lo:lo + 64].abs() + w[bi].abs()
    r = gate_out64(p, sp, gconst)
    return r.ref, gate_bound(r)


def attn_fwd_terms64(q, k, v, keep, drop_keep, p, scale, gate=None, dg=None, table=None):
    """The operation every forward entry point defines, in float64 on the values the C ABI receives (bf16 or f32 Q, K, V
    as [B, H, L, 64]; keep [B, Lk] bool or None with the keys at and past key_len[b] already false; the oracle's keep
    bits; p = attn_p32(p); the fp32 table [H, 2 L - 1] with the float64 gate of attn_fwd_gate64):
        S_ik = s Q_i.K_k + g_i T[h][k - i + Lk - 1]      P = softmax over kept keys      LSE_i = logsumexp_k S_ik
        O_id = c sum_k P_ik D_ik V_kd,  c = 1 / (1 - p)
    O and LSE come from attn_fwd_ref64. A row without a kept key is NaN in O and LSE. Returns an AttnFwdRef."""
    r = AttnFwdRef()
    r.g, r.dg = gate, dg
    r.T = table.double()[:, attn_rel_index(k.shape[2])] if table is not None else None
    bias = gate[..., None] * r.T[None] if table is not None else None
    r.O, r.LSE = attn_fwd_ref64(q, k, v, keep, drop_keep, p, scale, bias)
    s = float(scale) * (q.double() @ k.double().transpose(-1, -2))
    if bias is not None:
        s = s + bias
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    r.S, r.m = s, s.max(-1).values
    r.P = torch.exp(s - r.LSE[..., None])
    r.c = 1.0 / (1.0 - float(p)) if drop_keep is not None else 1.0
    r.D = drop_keep.double() * r.c if drop_keep is not None else None
    return r


ATTN_FWD_FAMILY = {"fwd7": "7", "fwd8": "8", "fwd6": "16", "fwd2": "16", "fwd5": "16", "generic": "f32"}


def attn_fwd_units(family, r, q, k, v, scale, tripped=None):
    """Per-element units of an AttnFwdRef for the checks
        |O_gpu - O_ref|     <= C_O u b_O + rel |O_ref| + lin_O
        |LSE_gpu - LSE_ref| <= C_L u b_LSE + lin_LSE
    as a dict (u, rel, b_o, b_lse, lin_o, lin_lse). u = 2^-9 and rel = 2^-8 (O is stored as bf16) for the bf16
    families, u = 2^-24 and rel = 0 for "f32". With a_ik = s sqrt(sum_d Q_id^2 K_kd^2), e_ikd = c D_ik V_kd and every
    sum over the kept keys k, the rounding points, each a relative error of at most u on the value it rounds, and the
    root-sum-square size they give an output:

    family "7" (fwd7_kernel, every build, attn7.hip :214-525; also the rows fwd8's fallback recomputes, attn8.hip
    :608-663, which is fwd7's algorithm with f32 row sums, :303-314):
      (1) Q' = bf16(Q s log2 e) (scale_frag, :269): one rounding eps_id' per query element, shared by every key of the
          row. It moves S_ik by s sum_d' eps_id' Q_id' K_kd', hence LSE_i by s sum_d' eps_id' Q_id' Kbar_id' with
          Kbar_i = sum_k P_ik K_k, and O_id by s sum_d' eps_id' Q_id' M_id'd with M_i = sum_k P_ik K_k (e_ik - O_i)^T
          (64 x 64 per row). Taking the keys' errors as independent (u a_ik per score) underrates both by the factor
          by which P and K are correlated along Q, about 4 at Lk 1024 on random inputs: the first emulation run showed
          it, the LSE of fwd7 at (96, 1024) sat at 10.5 of those units;
      (2) P o D packed to bf16 for the PV MFMA (:438); the row sum takes the fp32, undropped P (:432-433, :470): a
          relative u on every term P_ik e_ikd of O, nothing on LSE;
      (3) O rounded to bf16 (:511): the rel term.
      The softmax reference rf is bf16-exact inside the score MFMA (:376, :460, :468), the mask is an exact 0 / -inf
      (:338), the bias FMA (:415), exp2 (:430) and __log2f (:517) are fp32.
          b_O^2 = s^2 sum_d' Q_id'^2 M_id'd^2 + sum_k P_ik^2 e_ikd^2     b_LSE^2 = s^2 sum_d' Q_id'^2 Kbar_id'^2
    family "8" (fwd8_kernel's fast path, attn8.hip): (1) (:225-226) and (3) (:687-688) as above; the row sums come from
      row-selector MFMAs on the packed, undropped bf16 P (:6-9, :33-37, :589, :597) and the PV operand is that same
      packed value under the keep mask (:373-389), so one rounding of P_ik enters the numerator and the denominator
      together and moves O by P_ik (e_ikd - O_id), not by P_ik e_ikd, and LSE by P_ik:
          b_O^2 = s^2 sum_d' Q_id'^2 M_id'd^2 + sum_k P_ik^2 (e_ikd - O_id)^2
          b_LSE^2 = s^2 sum_d' Q_id'^2 Kbar_id'^2 + sum_k P_ik^2
      `tripped` [B, H, Lq] marks the rows whose wave took the fallback (attn_fwd_emulate returns it): family "7" units.
      tripped = "either" (the fwd8 guard cases) takes the larger of the two units per element instead: there the rows
      that fall back are the kernel's to decide, and tests/test_gpu_attn7.py's guard test pins which ones must.
    family "16" (fwd6 / fwd2 / fwd5, attention.hip; the three share one tile body): Q is not pre-scaled, scores,
      bias and mask are fp32 (softmax_tile :305-310, :336), so (1) does not exist; P o D is packed to bf16 (pv2
      :376-379), the row sum is fp32 (:338, :351), O is bf16 (finish_group :408-409), the LSE is fp32 (:412):
          b_O^2 = sum_k P_ik^2 e_ikd^2                                      b_LSE = the fp32 terms below
    family "f32" (fwd_kernel<float>, attention.hip :166-245): nothing rounds to bf16. u = 2^-24; the fast __expf of
      every probability (:221) is taken as gate_out64 takes it, (|S_ik - m_i| + 4) u relative on P_ik, in numerator and
      denominator alike; __logf (:244) is in the floor.
    fp32 terms, every family (sqrt(n) 2^-24 of the root-sum-square of the n products, as attn_bwd_units (7)): the
      64-term score sums move S_ik by 8 a_ik 2^-24; the bias FMA by 2 |g_i T_ik| 2^-24 (the product and the sum); the
      Lk-term PV and row sums give sqrt(Lk) 2^-24 sqrt(sum_k P_ik^2 (e_ikd^2 + O_id^2)) on O and sqrt(Lk) 2^-24
      sqrt(sum_k P_ik^2) on LSE. All enter b in quadrature (they are 2^-15 of a unit for the bf16 families).
    lin_LSE starts from the floor, written out: 2^-24 (8 + 4 |m_i| + 4 |LSE_i| + nt (R_i + 4)), m_i the row's largest
      score, R_i = m_i - its smallest kept score, nt = ceil(Lk / 64): the exponent's argument is an fp32 difference of
      two terms of size up to |m| log2 e (4 |m|), the LSE is an fp32 sum and product of terms of size |LSE| log2 e
      (4 |LSE|), exp2 / log2 / __logf are good to an ulp (8), and each of the nt rescalings of the online softmax
      multiplies the sum by an exponential of an argument of at most R_i (the f32 family's __expf: (R_i + 4) each).
    Gate term (a table was given): the kernel's gate differs from float64 by at most dg_i (attn_fwd_gate64) plus
      2 2^-24 |g_i| for its fp32 rescaling (g log2 e, attn7.hip :313; g / s, attention.hip :650). It moves every
      score of row i together, so it is added linearly:
          lin_O += dg_i |sum_k P_ik T_ik (e_ikd - O_id)|                   lin_LSE += dg_i |sum_k P_ik T_ik|"""
    f32 = family == "f32"
    u = U24 if f32 else U9
    s, Lk = float(scale), k.shape[2]
    v2 = v.double()
    a2 = s * s * ((q.double() ** 2) @ (k.double() ** 2).transpose(-1, -2))
    W = r.P ** 2
    Dc = r.D if r.D is not None else 1.0

    def sums(Wt):       # sum_k Wt (e - O)^2 and sum_k Wt e^2, [B, H, Lq, 64]
        WD = Wt * Dc
        A2 = (WD * Dc) @ v2 ** 2
        return (A2 - 2.0 * r.O * (WD @ v2) + r.O ** 2 * Wt.sum(-1, keepdim=True)).clamp_min(0.0), A2

    gT = r.g[..., None] * r.T[None] if r.T is not None else None
    fs2 = 64.0 * a2 + (4.0 * gT ** 2 if gT is not None else 0.0)
    if f32:
        arg = (r.S - r.m[..., None]).abs()
        fs2 = fs2 + (torch.where(torch.isfinite(arg), arg, torch.zeros_like(arg)) + 4.0) ** 2
    sig2 = U24 ** 2 * fs2
    devW, A2W = sums(W)
    dev_s, _ = sums(W * sig2)
    Wsum = W.sum(-1)
    fo2 = U24 ** 2 * Lk * (A2W + r.O ** 2 * Wsum[..., None])
    var_o = dev_s + (0.0 if f32 else u * u * A2W) + fo2
    var_l = (W * sig2).sum(-1) + U24 ** 2 * Lk * Wsum
    vq_o = 0.0
    if family in ("7", "8"):        # point (1), per (b, h) and in chunks of rows: M is [rows, 64, 64]
        kd, q2 = k.double(), q.double() ** 2
        Kbar = r.P @ kd
        var_l = var_l + u * u * s * s * (q2 * Kbar ** 2).sum(-1)
        PD = r.P * Dc
        vq = torch.empty_like(r.O)
        step = max(1, (1 << 22) // (Lk * 64))
        for b in range(q.shape[0]):
            for h in range(q.shape[1]):
                for i0 in range(0, q.shape[2], step):
                    i = slice(i0, i0 + step)
                    M = (PD[b, h, i, :, None] * kd[b, h][None]).transpose(1, 2) @ v2[b, h]
                    M = M - Kbar[b, h, i, :, None] * r.O[b, h, i, None, :]
                    vq[b, h, i] = torch.einsum("rd,rde->re", q2[b, h, i], M ** 2)
        vq_o = u * u * s * s * vq
        var_o = var_o + vq_o
    if family == "8":
        var_o8, var_l8 = dev_s + vq_o + u * u * devW + fo2, var_l + u * u * Wsum
        if isinstance(tripped, str):     # the guard cases: which waves fell back is the kernel's business, so the larger unit
            var_o, var_l = torch.maximum(var_o, var_o8), var_l8
        else:
            t = tripped if tripped is not None else torch.zeros_like(Wsum, dtype=torch.bool)
            var_o, var_l = torch.where(t[..., None], var_o, var_o8), torch.where(t, var_l, var_l8)
    smin = torch.where(torch.isinf(r.S), torch.full_like(r.S, float("inf")), r.S).min(-1).values
    lin_l = U24 * (8.0 + 4.0 * r.m.abs() + 4.0 * r.LSE.abs() + ((Lk + 63) // 64) * (r.m - smin + 4.0))
    lin_o = torch.zeros_like(r.O)
    if gT is not None:
        dgt = r.dg + 2.0 * U24 * r.g.abs()
        PT = r.P * r.T[None]
        lin_l = lin_l + dgt * PT.sum(-1).abs()
        lin_o = dgt[..., None] * ((PT * Dc) @ v2 - r.O * PT.sum(-1, keepdim=True)).abs()
    return dict(u=u, rel=0.0 if f32 else 2.0 ** -8, b_o=var_o.sqrt() / u, b_lse=var_l.sqrt() / u, lin_o=lin_o,
                lin_lse=lin_l)


def attn_fwd_excess(got, ref, b, u, rel=0.0, lin=0.0):
    """(|got - ref| - rel |ref| - lin)+ in units of u b, per element, in the shape of attn_bwd_excess: 0 where b == 0
    and nothing is left, inf where b == 0 and something is. Where the reference is NaN (a row without a kept key) the
    kernel's value must be NaN too: 0 if it is, inf if not, and inf where got is NaN and the reference is not."""
    got = got.double()
    x = ((got - ref).abs() - rel * ref.abs() - lin).clamp_min(0.0)
    out = x / (u * b)
    inf = torch.full_like(x, float("inf"))
    out = torch.where(b == 0, torch.where(x == 0, torch.zeros_like(x), inf), out)
    rn, gn = torch.isnan(ref), torch.isnan(got)
    return torch.where(rn | gn, torch.where(rn & gn, torch.zeros_like(x), inf), out)


def attn_fwd_emulate(family, q, k, v, keep, drop_keep, p, scale, gate=None, table=None):
    """The kernels' rounding points in plain torch: fp32 where the kernel holds fp32, .to(bfloat16) at the points of
    attn_fwd_units. Not modelled: the MFMA summation order, the hardware exp2, FMA contraction, the tile-by-tile
    rescaling of the online softmax (the reference is the row's final one; fwd8's is that of its first 32 keys, as in
    the kernel), the gate's own arithmetic (the float64 gate rounded to fp32 goes in). It sets ATTN_FWD_E and proves
    statements about inputs; it is no oracle for the kernels. Returns (O float32 [B, H, Lq, 64], holding bf16 values
    for the bf16 families; LSE float32 [B, H, Lq]; tripped [B, H, Lq] bool for family "8", else None)."""
    f = torch.float32
    q, k, v = (x.to(f) for x in (q, k, v))
    sc = float(np.float32(scale))
    sl2 = float(np.float32(sc * LOG2E_F32))
    Lq, Lk = q.shape[2], k.shape[2]
    Tm = table.to(f)[:, attn_rel_index(Lk)][None] if table is not None else None
    g = gate.to(f) if gate is not None else None
    D = drop_keep.to(f) if drop_keep is not None else None
    c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if D is not None else 1.0
    kT = k.transpose(-1, -2)
    nan = torch.tensor(float("nan"))

    def mask(s):
        return s if keep is None else s.masked_fill(~keep[:, None, None, :], float("-inf"))

    def ref_of(mx, rnd):
        return torch.where(torch.isinf(mx), torch.zeros_like(mx), rnd(mx))

    tripped = None
    if family in ("7", "8"):
        s2 = _bf(q * sl2) @ kT
        if Tm is not None:
            s2 = s2 + (g * LOG2E_F32)[..., None] * Tm
        s2 = mask(s2)
        rf = ref_of(s2.max(-1).values, _bf)
        P = torch.exp2(s2 - rf[..., None])
        l = P.sum(-1)
        PD = _bf(P if D is None else P * D)
        if family == "8":
            rf8 = ref_of(s2[..., :32].max(-1).values, _bf)
            P8 = _bf(torch.exp2(s2 - rf8[..., None]))
            l8 = P8.sum(-1)
            trip = ~((l8 >= 2.0 ** -40) & (l8 <= 2.0 ** 64)) & (l > 0)
            pad = (-Lq) % 64        # the guard is per wave: 64 consecutive queries fall back together
            tw = torch.nn.functional.pad(trip, (0, pad)).unflatten(-1, (-1, 64)).any(-1, keepdim=True)
            tripped = tw.expand(*tw.shape[:-1], 64).flatten(-2)[..., :Lq]
            PD = torch.where(tripped[..., None], PD, P8 if D is None else P8 * D)
            l, rf = torch.where(tripped, l, l8), torch.where(tripped, rf, rf8)
        o = _bf((PD @ v) * (c / l)[..., None])
        lse = (rf + torch.log2(l)) * LN2_F32
    elif family == "16":
        x = q @ kT
        if Tm is not None:
            x = x + (g / sc)[..., None] * Tm
        x = mask(x)
        m = ref_of(x.max(-1).values, lambda t: t)
        P = torch.exp2(x * sl2 - (m * sl2)[..., None])
        l = P.sum(-1)
        o = _bf((_bf(P if D is None else P * D) @ v) * (c / l)[..., None])
        lse = (m * sl2 + torch.log2(l)) * LN2_F32
    else:
        nthr = torch.get_num_threads()      # here the fp32 sums are the whole error: one thread, so that the summation
        torch.set_num_threads(1)            # order, and with it the measured E, does not depend on the thread count
        try:
            x = (q @ kT) * sc
            if Tm is not None:
                x = x + g[..., None] * Tm
            x = mask(x)
            m = ref_of(x.max(-1).values, lambda t: t)
            P = torch.exp(x - m[..., None])
            l = P.sum(-1)
            o = ((P if D is None else P * D * c) @ v) / l[..., None]
        finally:
            torch.set_num_threads(nthr)
        lse = m + torch.log(l)
    dead = ~(l > 0)
    return torch.where(dead[..., None], nan, o), torch.where(dead, nan, lse), tripped


# The largest error of attn_fwd_emulate against the float64 reference in units of u b (after the rel and lin terms),
# over every case of attn_fwd_cases() and every input set, per kernel family and output, measured on the CPU
# (tests/test_cpu_attn_fwd_ref.py asserts stored <= 1.1 measured + ATTN_FWD_E_FLOOR and measured <= stored). The kernels
# are allowed ATTN_FWD_C = 2 E units, the backward's factor and reason: what the emulation leaves out is fp32-sized and
# inside the units, so the factor covers only the tail between one sample of roundings and another.
# Measured (O / LSE): family 7 3.88 / 3.47, family 8 4.07 / 3.22, family 16 3.44 / 0 and f32 2.61 / 0: the LSE of the
# families that keep it in fp32 never leaves the written-out floor, their E is the floor of the rule.
ATTN_FWD_E = {"7": dict(o=4.1, lse=3.65), "8": dict(o=4.3, lse=3.4), "16": dict(o=3.6, lse=0.05),
              "f32": dict(o=2.75, lse=0.05)}
ATTN_FWD_E_FLOOR = 0.05
ATTN_FWD_C = {f: {n: 2.0 * e for n, e in d.items()} for f, d in ATTN_FWD_E.items()}

ATTN_REL_SPIKES = (129, 128, 127, 65, 64, 63, 33, 32, 31, 1)     # and their negatives, 0 and +-(S - 1)
ATTN_FWD_SHAPES = ((1, 1), (33, 5), (65, 17), (64, 64), (129, 200), (256, 256), (40, 257), (129, 300), (257, 64),
                   (40, 513), (96, 1024))
ATTN_FWD_FAINT = 2.0 ** -6      # the "faint" input set: the flat q times this
ATTN_REL_SPIKE_MASS = 2.0 / 3.0  # of the median row before the last key's weight: half of the row after it
ATTN_REL_LAST_MASS = 0.25       # the last kept key's share of every row, WavLM "edges"
ATTN_REL_QW_MIN, ATTN_REL_QW_MAX = 4.0, 32.0    # the range of a query's component along w


def _fc(kernel, Lq, Lk, masked=False, p=0.0, *, force, ext=None, bits=None, strided=False, guard=False, B=2, H=2,
        src=None, g8=None, faint=False, dead=False, tag=""):
    """One forward case. kernel: what ops.attn_last_path()["fwd"][0] must read; expect: the whole tuple (kernel, DM, MK,
    KX, REL). bits: None (no dropout), "ready" (the producer wrote the keep bits, the forward reads them), "own" (the
    forward gets an unwritten buffer and it, or the launch wrapper for it, writes the words), "rehash" (no buffer).
    src: the gate source of a WavLM case ("gate" | "graw" | "gx"), None for the decoder's. g8: (geometry, kind, c) of
    fwd8_guard_inputs. dead: the last entry's mask keeps no key. The f32 family runs fp32 tensors."""
    rel, kx = src is not None, ext is not None
    if kx:
        B, masked = len(ext), True
    mk = 2 if masked else 1 if Lk % 64 else 0
    m01 = int(masked or Lk % 64 != 0)
    expect = {"fwd7": ("fwd7", int(p > 0), mk, kx, rel),
              "fwd8": ("fwd8", int(p > 0), mk, False, False),
              "fwd6": ("fwd6", 0 if p == 0 else 1 if bits == "ready" else 2, mk, False, False),
              "fwd2": ("fwd2", int(p > 0), m01, False, False),
              "fwd5": ("fwd5", 0, m01, False, True),
              "generic": ("generic", int(p > 0), int(masked), False, False)}[kernel]
    cid = (f"{kernel}-{Lq}x{Lk}" + ("-" + "_".join(map(str, ext)) if kx else "") + ("-mask" if masked and not kx else "")
           + (f"-p{p}-{bits}" if p else "") + (f"-{src}" if rel else "") + ("-strided" if strided else "")
           + ("-guard" if guard else "") + (f"-{force}" if force not in ("fwd7", "fwd8", "v6") else "")
           + ("-dead" if dead else "") + tag)
    kinds = ("guard",) if g8 else ("flat", "edges", "faint") if faint else ("flat", "edges")
    return dict(id=cid, kernel=kernel, family=ATTN_FWD_FAMILY[kernel], B=B, H=H, Lq=Lq, Lk=Lk, masked=masked, p=p,
                ext=ext, force=force, bits=bits, strided=strided, guard=guard, src=src, rel=rel, g8=g8, kinds=kinds, dead=dead,
                f32=kernel == "generic", expect=expect, has_lse=src in (None, "gate"))


@functools.lru_cache(maxsize=None)
def attn_fwd_cases():
    """Every case of tests/test_gpu_attn_fwd.py: the smallest shapes at which each mechanism of each forward kernel
    exists (B H <= 8). guard: O is a column slice of a wider NaN-filled buffer; strided: q, k, v are column slices of
    one [rows, 3 H 64] buffer."""
    cs = []
    # the decoder's kernels (no table): one query and key | a partial 32-query group, five keys | two query groups, 17
    # keys | exactly one tile | ragged fourth key tile | four full tiles | one key in the fifth tile | ragged fifth |
    # three query blocks of fwd7, two of fwd8 | one key in the ninth tile | sixteen full tiles
    for kernel, force in (("fwd7", "fwd7"), ("fwd8", "fwd8"), ("fwd6", "v6")):
        for si, (Lq, Lk) in enumerate(ATTN_FWD_SHAPES):
            for masked in (False, True):
                for p in (0.0, 0.1):
                    # both ways of getting the keep bits under every mask build: alternate over shapes and masks
                    bits = None if p == 0 else ("ready", "own")[(si + masked) % 2]
                    cs.append(_fc(kernel, Lq, Lk, masked, p, force=force, bits=bits, guard=p > 0 and masked,
                                  faint=kernel == "fwd7" and (Lq, Lk) in ((129, 200), (96, 1024))))
        # more than eight query blocks of 128 (fwd7 / fwd6), five of 256 (fwd8), the last with one query
        cs.append(_fc(kernel, 1025, 64, False, 0.0, force=force, B=1))
        cs.append(_fc(kernel, 1025, 64, True, 0.1, force=force, B=1, bits="ready", guard=True))
        # q | k | v from one fused-projection buffer
        cs.append(_fc(kernel, 129, 200, True, 0.1, force=force, bits="ready", strided=True))
    # the default dispatch at these small grids is fwd7 (attention.hip run<>: load8 > load7)
    cs.append(_fc("fwd7", 129, 200, True, 0.1, force="auto", bits="ready"))
    cs.append(_fc("fwd7", 65, 17, False, 0.0, force="auto"))
    # key extents (fddm_attn_fwd_kx): always fwd7's KX builds
    for Lk, ext in ATTN_KX.items():
        for p in (0.0, 0.1):
            cs.append(_fc("fwd7", 129, Lk, True, p, force="fwd7", ext=ext, H=1 if Lk == 200 else 2,
                          bits="ready" if p else None, guard=p > 0))
    # ... and an entry without a key: NaN rows in O and LSE
    cs.append(_fc("fwd7", 129, 200, True, 0.0, force="fwd7", ext=[200, 0]))
    # fwd8 alone: three workgroups, the last partial | exactly one half-tile | one key in the second half
    cs.append(_fc("fwd8", 600, 300, True, 0.1, force="fwd8", bits="ready"))
    cs.append(_fc("fwd8", 32, 32, False, 0.1, force="fwd8", B=1, H=1, bits="own"))
    cs.append(_fc("fwd8", 64, 33, False, 0.0, force="fwd8", B=1))
    # ... and two of its guard cases, whose designated rows' waves take the fallback
    for geom, kind, cc in (("a", "rise", 4.7), ("b", "fall", 25.0)):
        B, H, Lq, Lk, p, tail, _ = FWD8_GUARD_GEOMS[geom]
        cs.append(_fc("fwd8", Lq, Lk, bool(tail) or kind == "fall", p, force="fwd8", B=B, H=H, bits="ready",
                      g8=(geom, kind, cc), tag=f"-{kind}{cc}"))
    # Lk > 1024: fwd2 whatever is forced; it draws its own keep bits and records them when it has a buffer
    for Lq, Lk in ((40, 1025), (130, 1100)):
        for masked in (False, True):
            for p, bits in ((0.0, None), (0.1, "own"), (0.1, "rehash")):
                cs.append(_fc("fwd2", Lq, Lk, masked, p, force="fwd7", bits=bits, guard=masked and bits == "own",
                              tag="-long"))
    # ... and its unmasked builds: Lk a multiple of 64
    cs.append(_fc("fwd2", 40, 1088, False, 0.0, force="fwd7", B=1, tag="-long"))
    cs.append(_fc("fwd2", 40, 1088, False, 0.1, force="fwd7", B=1, bits="own", tag="-long"))
    # the generic f32 kernel
    cs.append(_fc("generic", 65, 17, False, 0.0, force="auto"))
    cs.append(_fc("generic", 129, 200, True, 0.1, force="auto", bits="rehash", guard=True))
    cs.append(_fc("generic", 40, 257, False, 0.1, force="auto", bits="rehash"))
    # WavLM's gated relative-position bias (a table; Lq = Lk = S, no dropout, H = 3 so that h (2 S - 1) is no multiple
    # of anything convenient): fwd7's REL builds, and fwd5 forced (S > 1024 takes fwd5 whatever is forced)
    for kernel, force, more in (("fwd7", "auto", ()), ("fwd5", "relfwd5", (1030, 1100))):
        for S in (1, 33, 64, 127, 128, 129, 200, 257, 513, 1024) + more:
            for src in ("gx", "gate", "graw") if S in (129, 257) else ("gx",):
                cs.append(_fc(kernel, S, S, force=force, src=src, B=2 if S <= 257 else 1, H=3,
                              faint=kernel == "fwd7" and S == 200))
        # a key-padding mask without an extent (attn_fwd with gate + table + key_keep)
        cs.append(_fc(kernel, 200, 200, True, force=force, src="gate", H=3))
        # ... and with one (attn_fwd_relgate_x with key_keep and key_len): the ATTN_KX extents two entries at a time,
        # and an entry without a key
        for S, exts in ((200, ([200, 1], [63, 64], [65, 129])), (300, ([300, 257], [256, 70])), (129, ([129, 0],))):
            for ext in exts:
                cs.append(_fc(kernel, S, S, force=force, src="gx", ext=ext, H=3))
    cs.append(_fc("generic", 129, 129, True, force="auto", src="gate", H=3))
    # an entry whose mask keeps no key (no extent): NaN rows in O and LSE from every kernel
    for kernel, force in (("fwd7", "fwd7"), ("fwd8", "fwd8"), ("fwd6", "v6"), ("generic", "auto")):
        cs.append(_fc(kernel, 65, 17, True, 0.0, force=force, dead=True))
    cs.append(_fc("fwd2", 40, 1025, True, 0.0, force="fwd7", dead=True, tag="-long"))
    for kernel, force in (("fwd7", "auto"), ("fwd5", "relfwd5")):
        cs.append(_fc(kernel, 129, 129, True, force=force, src="gate", H=3, dead=True))
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


# the template builds the case table must reach, as ops.attn_last_path()["fwd"] reads them (attention.hip run<>,
# attn7.hip attn7_fwd, attn8.hip attn8_fwd). fwd2_kernel has no relative-position build: a table with Lk > 1024 takes
# fwd5.
ATTN_FWD_BUILDS = (
    [("fwd7", dm, mk, False, False) for dm in (0, 1) for mk in (0, 1, 2)] +
    [("fwd7", dm, 2, True, False) for dm in (0, 1)] +
    [("fwd7", 0, mk, False, True) for mk in (0, 1, 2)] + [("fwd7", 0, 2, True, True)] +
    [("fwd8", dm, mk, False, False) for dm in (0, 1) for mk in (0, 1, 2)] +
    [("fwd6", dm, mk, False, False) for dm in (0, 1, 2) for mk in (0, 1, 2)] +
    [("fwd2", dm, mask, False, False) for dm in (0, 1) for mask in (0, 1)] +
    [("fwd5", 0, mask, False, True) for mask in (0, 1)] +
    [("generic", dm, mask, False, False) for dm, mask in ((0, 0), (1, 1), (1, 0), (0, 1))])


def _bisect(f, hi, target=0.5, steps=14):
    """The x in [0, hi] at which the increasing f reaches target (hi if it never does)."""
    lo = 0.0
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


def _median_mass(s, sel):
    """Median over the rows with a kept key of the probability mass softmax(s) puts on the keys `sel` selects."""
    pr = torch.softmax(s, -1)
    m = (pr * sel).sum(-1)
    return m[torch.isfinite(m)].median().item()


@functools.lru_cache(maxsize=6)
def attn_fwd_case_inputs(cid, kind):
    """Inputs of case `cid` for input set `kind`, built once and never modified: a dict of q [B, Lq, H 64], k, v
    [B, Lk, H 64] float32 (holding bf16 values unless the case runs the f32 kernel); keep [B, Lk] bool or None (keys at
    and past an extent are false); drop [B, H, Lq, Lk] bool or None; for a WavLM case also table [H, 2 S - 1], gconst
    [H], gw [130] float32, x [B S, H 64] and graw [B S, 8 H] float32 holding bf16 values, gate [B H, S] float32, and
    g64 / dg [B, H, S] (attn_fwd_gate64 of the case's source).
    "flat": randn q, k, v; table = 2 randn. "faint": the flat q times 2^-6 (a_ik of attn_fwd_units shrinks to
      2^-6 of its flat size while P stays a bf16-sized rounding away from its row sum: the input set on which a P
      rounded before the row sum shows in the LSE).
    "edges", decoder: attn_bwd_case_inputs' recipe (q = 0.5 randn + 4 w, every edge key + beta w with beta from
      ATTN_EDGE_MASS, masked keys the same + beta w).
    "edges", WavLM: q = 0.5 randn (so that a single spike is not drowned); table = 2 randn plus a spike h at each
      offset k - i in +-ATTN_REL_SPIKES, 0 and +-(S - 1) that exists, h solved (bisection on the reference's softmax) so
      that at the case's gates the spiked keys hold ATTN_REL_SPIKE_MASS = 2/3 of the median row, which is half of it
      once the last key has its quarter. As i runs over a query block every spike lands on every lane position, tile
      edge and shifted-copy parity. The mask and tile-edge mutants need a key every row sees, and a table entry is seen
      by one row per key while the 2 randn table moves a key's share by e^(+-g 2) from row to row: so the last kept key
      of every entry gets + 8 w and query i gets + alpha_i w (w: 64 entries of +-1/8), alpha_i in [4, 32] solved per row
      so that this key holds ATTN_REL_LAST_MASS = 1/4 of row i (more where 4 w already gives it more); the w component
      adds N(0, (alpha_i / 8)^2) to every other score of the row. Masked keys get + 16 w: a kernel that keeps one shows
      it in every row.
    "guard": fwd8_guard_inputs of the case's g8."""
    import math
    from oracle import fddm_oracle as O
    c = {x["id"]: x for x in attn_fwd_cases()}[cid]
    B, H, Lq, Lk, p = c["B"], c["H"], c["Lq"], c["Lk"], c["p"]
    drop = O.attn_dropout_keep(ATTN_SEED, ATTN_STREAM, B, H, Lq, Lk, p) if p > 0 else None
    rnd = (lambda t: t.float()) if c["f32"] else (lambda t: t.to(torch.bfloat16).float())
    if c["g8"]:
        q, k, v, keep, _ = fwd8_guard_inputs(*c["g8"])
        return dict(q=rnd(q), k=rnd(k), v=rnd(v), keep=keep, drop=drop)
    gen = torch.Generator().manual_seed(104729 * Lq + 31 * Lk + 7 * c["masked"] + (1 if kind == "edges" else 0))
    q, k, v = (torch.randn(B, L, H, 64, generator=gen) for L in (Lq, Lk, Lk))
    keep = attn_bwd_mask(B, Lk, c["ext"]) if c["masked"] else None
    if c["dead"]:
        keep[B - 1] = False
    full = torch.ones(B, Lk, dtype=torch.bool) if keep is None else keep
    out = {}
    if c["rel"]:
        S = Lk
        x = torch.randn(B * S, H * 64, generator=gen).to(torch.bfloat16).float()
        lin = torch.nn.Linear(64, 8)
        with torch.no_grad():
            lin.weight.copy_(0.2 * torch.randn(8, 64, generator=gen))
            lin.bias.copy_(0.1 * torch.randn(8, generator=gen))
        gconst = 0.5 + torch.rand(H, generator=gen)
        table = 2.0 * torch.randn(H, 2 * S - 1, generator=gen)
        # models.wavlm._fold_gate's 130 floats, restated so that the reference needs no built library: the sums of
        # weight rows 0-3 and 4-7, then the two bias sums (tests/test_cpu_host.py pins _fold_gate itself)
        Wl, bl = lin.weight.detach().float(), lin.bias.detach().float()
        gw = torch.cat([Wl[:4].sum(0), Wl[4:].sum(0), bl[:4].sum().reshape(1), bl[4:].sum().reshape(1)]).contiguous()
        graw = (torch.einsum("nhd,od->nho", x.view(B * S, H, 64), lin.weight.detach()) + lin.bias.detach())
        graw = graw.reshape(B * S, H * 8).to(torch.bfloat16).float()
        gate = attn_fwd_gate64("gx", B, H, S, x=x, gw=gw, gconst=gconst)[0].float().reshape(B * H, S)
        g64, dg = attn_fwd_gate64(c["src"], B, H, S, gate=gate, graw=graw, x=x, gw=gw, gconst=gconst)
        out = dict(table=table, gconst=gconst, gw=gw, x=x, graw=graw, gate=gate, g64=g64, dg=dg)
    if kind == "faint":
        q = q * ATTN_FWD_FAINT
    if kind == "edges":
        w = (torch.randint(0, 2, (64,), generator=gen).float() * 2.0 - 1.0) / 8.0
        live = [b for b in range(B) if full[b].any()]
        if not c["rel"]:
            q = ATTN_EDGE_QSTD * q + ATTN_EDGE_QW * w
            for b in live:
                ek = _attn_edge_keys(full[b], Lk)
                beta = max(0.0, 8.0 / ATTN_EDGE_QW * math.log(ATTN_EDGE_MASS * int(full[b].sum()) / len(ek)))
                k[b, ek] += beta * w
                k[b, (~full[b]).nonzero().flatten()] += beta * w
        else:
            q = ATTN_EDGE_QSTD * q
        if c["rel"] and Lk >= 4:
            S = Lk
            rel = attn_rel_index(S)
            g64 = out["g64"]
            base = 0.125 * torch.einsum("bihd,bkhd->bhik", q.double(), k.double())
            base = (base + g64[..., None] * table.double()[:, rel][None]).masked_fill(~full[:, None, None, :],
                                                                                    float("-inf"))
            offs = sorted({o for a in ATTN_REL_SPIKES + (S - 1,) for o in (a, -a) if a <= S - 1} | {0})
            spike = torch.zeros(2 * S - 1)
            spike[[o + S - 1 for o in offs]] = 1.0
            M = spike[rel][None, None].double()
            h = _bisect(lambda t: _median_mass(base + t * g64[..., None] * M, M), 32.0, ATTN_REL_SPIKE_MASS)
            base = base + h * g64[..., None] * M
            # the last kept key of every entry: + 8 w on the key and alpha_i w on query i, alpha_i >= ATTN_REL_QW_MIN
            # solved per row so that the key holds ATTN_REL_LAST_MASS of the row (more where 4 w already gives more)
            E = torch.zeros(B, S, dtype=torch.float64)
            for b in live:
                E[b, int(full[b].nonzero().max())] = 1.0
            E = E[:, None, None, :]
            cw = 0.125 * torch.einsum("bkhd,d->bhk", k.double(), w.double())[:, :, None, :] + E
            lo = torch.full(base.shape[:3], ATTN_REL_QW_MIN, dtype=torch.float64)
            hi = torch.full_like(lo, ATTN_REL_QW_MAX)
            for _ in range(14):
                mid = 0.5 * (lo + hi)
                low = (torch.softmax(base + mid[..., None] * cw, -1) * E).sum(-1) < ATTN_REL_LAST_MASS
                lo, hi = torch.where(low, mid, lo), torch.where(low, hi, mid)
            q = q + hi.float().transpose(1, 2)[..., None] * w
            for b in live:
                k[b, int(full[b].nonzero().max())] += 8.0 * w
            for b in range(B):      # a masked key, were it kept, would outweigh the last key e^alpha times before the bias
                k[b, (~full[b]).nonzero().flatten()] += 16.0 * w
            out["table"] = table + h * spike
    flat = lambda t, L: rnd(t).reshape(B, L, H * 64)  # noqa: E731
    out.update(q=flat(q, Lq), k=flat(k, Lk), v=flat(v, Lk), keep=keep, drop=drop)
    return out


@functools.lru_cache(maxsize=6)
def attn_fwd_case_ref(cid, kind):
    """(AttnFwdRef, units, (O, LSE) of the emulation) of a case's family on its inputs. Built once, never modified."""
    c = {x["id"]: x for x in attn_fwd_cases()}[cid]
    x = attn_fwd_case_inputs(cid, kind)
    q, k, v = (attn_heads(x[n], c["B"], c["H"]) for n in ("q", "k", "v"))
    p = attn_p32(c["p"])
    g, tb = (x["g64"], x["table"]) if c["rel"] else (None, None)
    r = attn_fwd_terms64(q, k, v, x["keep"], x["drop"], p, 0.125, g, x.get("dg"), tb)
    eo, el, trip = attn_fwd_emulate(c["family"], q, k, v, x["keep"], x["drop"], p, 0.125, g, tb)
    return r, attn_fwd_units(c["family"], r, q, k, v, 0.125, "either" if c["g8"] else trip), (eo, el)


# --------------------------------- conditioning, RoPE and embedding kernels (csrc/small.hip, csrc/misc.hip)
# References, per-element bounds, inputs, emulations and case tables shared by tests/test_cpu_cond_ref.py (which sets
# the constants below from the reference alone) and tests/test_gpu_cond.py (which runs the kernels).
# fp32 evaluation in each kernel's own summation order (lin_emulate, dw_emulate, rows_mean_emulate, the oracle's
# time_embedding, silu32 / dsilu32) against float64 in units of 2^-24 times the per-element scale, the maximum over
# every case of the tables below, measured on the CPU: 5.19, 4.83, 3.00, 1.06, 2.31, 1.30 (tests/test_cpu_cond_ref.py
# asserts them; the constants keep 10 % headroom). The kernels are allowed COND_C = 8 E units: the margin covers
# contraction, the device's expf / sinf / cosf against the CPU's and the division. Hard cap 64.
COND_E = {"lin": 5.7, "dw": 5.3, "rm": 3.3, "te": 1.2, "silu": 2.55, "g": 1.45}
COND_C = {k: 8.0 * v for k, v in COND_E.items()}
COND_E_FLOOR = 0.05            # stored <= 1.1 measured + this
SILU_FLUSH = 2.0 ** -121       # expf(-v) is inf beyond -v = ln FLT_MAX = 88.72: silu32 gives 0 where |silu| < 88.73 / FLT_MAX < 2^-121
SILU_G_ZERO = -1.2784645       # silu'(x) = 0: why act 2's second term is absolute


class Ref:
    """A float64 value and its per-element bound or error scale, by attribute."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


def _pow2(gen, n, lo=-2, hi=2):
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=gen).float())


def sigmoid64(x):
    return torch.sigmoid(x.double())


def dsilu64(x):
    """silu'(x) = sigma (1 + x (1 - sigma))"""
    sg = sigmoid64(x)
    return sg * (1.0 + x.double() * (1.0 - sg))


def silu32(v):
    """small.hip's fp32 expression v / (1 + expf(-v))"""
    v = v.float()
    return v / (1.0 + torch.exp(-v))


def dsilu32(x):
    """small.hip's fp32 expression sg (1 + x (1 - sg)), sg = 1 / (1 + expf(-x))"""
    x = x.float()
    sg = 1.0 / (1.0 + torch.exp(-x))
    return sg * (1.0 + x * (1.0 - sg))


def silu_grid():
    """About 4000 points over [-20, 20] with +-0, the zero of silu' +- 2^-10, and arguments at which expf overflows to
    inf (|v| > 88.7) or its result leaves the normal range."""
    g = torch.linspace(-20.0, 20.0, 4001, dtype=torch.float64).float()
    extra = torch.tensor([0.0, -0.0, SILU_G_ZERO, SILU_G_ZERO - 2.0 ** -10, SILU_G_ZERO + 2.0 ** -10, -88.0, -89.0, -100.0,
                          -1000.0, 88.0, 89.0, 100.0, 1000.0], dtype=torch.float32)
    return torch.cat([g, extra])


# ---- the linear family (linear4_kernel, linrt_kernel through ops.small_linear)
LIN_MAXJ = 16                  # jobs per launch (small.hip MAXJ; ops.small_linear splits longer lists)
# (id, kernels per launch of <= 16 jobs, R, K, N, jobs, input row strides beyond K, bias given)
LIN_CASES = [
    ("l4-chunk", ("linear4",), 5, 512, 40, 1, (0,), True),          # one full 512-chunk
    ("l4-prefetch", ("linear4",), 32, 2048, 24, 1, (0,), True),     # four chunks: fetch(k0 + 512), the second stash()
    ("l4-ragged", ("linear4",), 33, 515, 13, 1, (0,), True),        # row tile 2 holds one row; K % 4 = 3; 13 columns
    ("l4-one", ("linear4",), 1, 1, 1, 1, (0,), True),               # the smallest shape
    ("l4-strided", ("linear4",), 7, 100, 20, 3, (1, 4), False),     # rows off 16 bytes (scalar loads), then on; no bias
    ("rt-trips", ("linrt",), 45, 1100, 400, 12, (0,), True),        # 18 chunks: waves 0, 1 make three trips; last 12 wide
    ("rt-tail", ("linrt",), 45, 579, 130, 16, (0,), True),          # odd K; ragged n + 3 < N; ldw = 130 off 16 bytes
    ("rt-short", ("linrt",), 33, 40, 130, 16, (0,), False),         # under one chunk: seven waves add zeros; no bias
    ("l4-exact", ("linear4",), 64, 64, 64, 16, (0,), True),         # exact multiples; 64 tiles: linear4, blockIdx.z = 1
    ("rt-exact", ("linrt",), 64, 64, 128, 16, (0,), True),          # exact multiples at 128 tiles
    ("split", ("linrt", "linear4"), 32, 64, 256, 24, (0,), True),   # 16 jobs of 128 tiles, then 8 of 64
    ("rt-24", ("linrt", "linrt"), 16, 96, 768, 24, (0,), True),     # both launches on linrt
]


def lin_dispatch(R, N, J):
    """The kernel of every launch ops.small_linear makes for J weight sets (fddm_small_linear: linrt where the
    32-column tiles of one launch make at least 128 blocks)."""
    out = []
    for j0 in range(0, J, LIN_MAXJ):
        tiles = ((N + 31) // 32) * min(LIN_MAXJ, J - j0) * ((R + 31) // 32)
        out.append("linrt" if tiles >= 128 else "linear4")
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lin_operands(cid):
    """x [R, K] = randn times a power of two per row, W [J, N, K] (the logical weights: out = x W_j^T) = randn / sqrt(K)
    times a power of two per output column, b [J, N] = randn times the column's, aux [R, N] = 1.5 randn; powers from
    2^-2 .. 2^2. f32 CPU tensors, never modified."""
    _, _, R, K, N, J, _, _ = {c[0]: c for c in LIN_CASES}[cid]
    gen = _gen(R, K, N, J)
    rs, cs = _pow2(gen, R), _pow2(gen, N)
    x = torch.randn(R, K, generator=gen) * rs[:, None]
    W = torch.randn(J, N, K, generator=gen) * (cs[None, :, None] / K ** 0.5)
    b = torch.randn(J, N, generator=gen) * cs[None, :]
    return x, W, b, 1.5 * torch.randn(R, N, generator=gen)


def lin_out64(y0, s0, b, aux):
    """The three outputs of the family from y0 = sum_k x W (float64 [R, J, N]) with scale s0 = sum_k |x| |W|, the bias
    b [J, N] or None, aux [R, N]: Ref with
      pre, b_pre      y = y0 + b within C_lin u s, s = s0 + |b|                            (act 0's out, act 1's out)
      silu, b_silu    silu(y) within |silu'(y)| C_lin u s + C_silu u |silu(y)| + SILU_FLUSH  (act 1's out2)
      dx, b_dx        y0 silu'(aux) within |g| C_lin u s0 + |y0| C_g u (1 + |aux|)         (act 2: no bias)"""
    cl = COND_C["lin"] * U24
    y, s = y0, s0
    if b is not None:
        y, s = y0 + b.double()[None], s0 + b.double().abs()[None]
    silu = y * torch.sigmoid(y)
    a = aux.double()[:, None, :]
    g = dsilu64(a)
    return Ref(y0=y0, s0=s0, pre=y, s=s, b_pre=cl * s, silu=silu,
               b_silu=dsilu64(y).abs() * cl * s + COND_C["silu"] * U24 * silu.abs() + SILU_FLUSH,
               g=g, dx=y0 * g, b_dx=g.abs() * cl * s0 + y0.abs() * (COND_C["g"] * U24) * (1.0 + a.abs()))


@functools.lru_cache(maxsize=None)
def lin_ref64(cid):
    x, W, b, aux = lin_operands(cid)
    xd, Wd = x.double(), W.double()
    given = {c[0]: c for c in LIN_CASES}[cid][7]
    return lin_out64(torch.einsum("rk,jnk->rjn", xd, Wd), torch.einsum("rk,jnk->rjn", xd.abs(), Wd.abs()),
                     b if given else None, aux)


def lin_emulate(x, W, b, kernel):
    """y0 and y [R, J, N] in fp32 in the kernel's order. linear4: thread quarter q owns k in [128 q, 128 q + 128) of every
    512-chunk, one FMA chain across all chunks in k order, then ((q0 + q1) + q2) + q3 (small.hip linear4_kernel, the kk
    loop and the `red` line). linrt: wave w owns the 64-chunks w, w + 8, ..., one FMA chain in k order, the 8 partials
    added from 0 in wave order (linrt_kernel, the c loop and the ww loop). Then + bias."""
    R, K = x.shape
    J, N, _ = W.shape
    xd, Wd = x.double(), W.double()
    ng = 4 if kernel == "linear4" else 8
    acc = torch.zeros(ng, R, J, N, dtype=torch.float64)       # f32 values held in float64
    for k in range(K):
        q = (k % 512) // 128 if kernel == "linear4" else (k // 64) % 8
        acc[q] = (xd[:, k, None, None] * Wd[None, :, :, k] + acc[q]).float().double()
    a = acc.float()
    if kernel == "linear4":
        y0 = ((a[0] + a[1]) + a[2]) + a[3]
    else:
        y0 = torch.zeros(R, J, N)
        for w in range(8):
            y0 = y0 + a[w]
    return y0, (y0 + b.float()[None] if b is not None else y0)


# ---- small_dw (dw_kernel)
# one launch holds jobs of these (N, K); the last list is the 17-job call (ops.small_dw splits it 16 + 1)
DW_SHAPES = ((40, 200), (200, 40), (33, 65), (1, 1))
DW_DB = (True, False, True, False)                 # db given / None
DW_ROWS = (45, 1, 64)
DW_MANY = (17, 6, 10, 7)                           # jobs, N, K, R: equal shapes, K % 4 != 0, db on even jobs
DW_PAD = 3                                         # dy is dybuf[:, 1 : 1 + N] of an [R, N + DW_PAD] buffer: lddy > N


def dw_cases():
    """(id, R, ((N, K, db given), ...))"""
    cs = [(f"R{R}", R, tuple((n, k, g) for (n, k), g in zip(DW_SHAPES, DW_DB))) for R in DW_ROWS]
    J, N, K, R = DW_MANY
    return cs + [("many", R, tuple((N, K, j % 2 == 0) for j in range(J)))]


@functools.lru_cache(maxsize=None)
def dw_operands(cid):
    """Per job (dybuf [R, N + DW_PAD], x [R, K], dW_old [N, K], db_old [N]): randn times a power of two per row and per
    column of dy, per column of x (2^-2 .. 2^2); the old values carry both column scales."""
    _, R, jobs = {c[0]: c for c in dw_cases()}[cid]
    out = []
    for j, (N, K, _) in enumerate(jobs):
        gen = _gen(R, N, K, j)
        rs, ns, ks = _pow2(gen, R), _pow2(gen, N + DW_PAD), _pow2(gen, K)
        dyb = torch.randn(R, N + DW_PAD, generator=gen) * rs[:, None] * ns[None, :]
        x = torch.randn(R, K, generator=gen) * ks[None, :]
        dW = torch.randn(N, K, generator=gen) * ns[1:1 + N, None] * ks[None, :]
        out.append((dyb, x, dW, torch.randn(N, generator=gen) * ns[1:1 + N]))
    return out


def dw_ref64(dy, x, dW_old, db_old):
    """dW_new = dW_old + dy^T x with s = |dW_old| + |dy|^T |x|; db_new = db_old + sum_r dy with s = |db_old| + sum_r |dy|;
    both within C_dw u s."""
    dy, x, w0, b0 = dy.double(), x.double(), dW_old.double(), db_old.double()
    c = COND_C["dw"] * U24
    sW, sb = w0.abs() + dy.abs().t() @ x.abs(), b0.abs() + dy.abs().sum(0)
    return Ref(dW=w0 + dy.t() @ x, sW=sW, b_dW=c * sW, db=b0 + dy.sum(0), sb=sb, b_db=c * sb)


def dw_emulate(dy, x, dW_old, db_old):
    """fp32 in dw_kernel's order: one FMA chain over the rows in order, then one add onto the old value; db is plain
    adds over the rows, then one add."""
    dyd, xd = dy.double(), x.double()
    acc = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float64)
    bacc = torch.zeros(dy.shape[1])
    for r in range(dy.shape[0]):
        acc = (dyd[r, :, None] * xd[r, None, :] + acc).float().double()
        bacc = bacc + dy[r].float()
    return dW_old.float() + acc.float(), db_old.float() + bacc


# ---- rows_mean, rows_mean_masked
RM_B = 2
RM_S = (1, 31, 33, 128, 131, 499)
RM_D = (8, 64, 72, 130, 512)
RM_MASKED_EQ = (131, 499)      # all-ones mask: rows_mean's bits
RM_HOLES_S = 131


@functools.lru_cache(maxsize=None)
def rm_operands(S, d, dt):
    """x [2, S, d] = randn times a power of two per row and per column (2^-2 .. 2^2), rounded to bf16 for "bf16"."""
    gen = _gen(S, d, dt == "bf16")
    x = torch.randn(RM_B, S, d, generator=gen) * _pow2(gen, S)[None, :, None] * _pow2(gen, d)[None, None, :]
    return x.to(torch.bfloat16 if dt == "bf16" else torch.float32)


def rm_holes(S):
    """keep [2, S] uint8: entry 0 keeps about two rows in three, never the last; entry 1 keeps nothing."""
    keep = (torch.rand(RM_B, S, generator=_gen(S, 77)) < 0.66).to(torch.uint8)
    keep[0, 0], keep[0, -1], keep[1] = 1, 0, 0
    return keep


def rm_ref64(x, keep=None):
    """The float64 mean over the (kept) rows with s = the mean of |x| over them, within C_rm u s. Entries that keep
    nothing: mean and s are 0 here; what the kernel writes there is asserted apart."""
    xd = x.double()
    if keep is None:
        m, s = xd.mean(1), xd.abs().mean(1)
    else:
        k = keep.double()[..., None]
        cnt = k.sum(1).clamp(min=1)
        xz = torch.where(k > 0, xd, torch.zeros_like(xd))
        m, s = xz.sum(1) / cnt, xz.abs().sum(1) / cnt
    return Ref(mean=m, s=s, b=COND_C["rm"] * U24 * s)


def rows_mean_emulate(x, keep=None):
    """fp32 in the kernels' order: slice sl sums its (kept) rows sl, sl + 32, ... in order; the 32 slice sums are added
    from 0 in order and divided by (float) the row count."""
    B, S, d = x.shape
    xf = x.float()
    tot = torch.zeros(B, d)
    for sl in range(32):
        acc = torch.zeros(B, d)
        for s in range(sl, S, 32):
            row = xf[:, s]
            acc = acc + (row if keep is None else torch.where(keep[:, s, None] > 0, row, torch.zeros_like(row)))
        tot = tot + acc
    n = torch.full((B, 1), float(S)) if keep is None else keep.float().sum(1, keepdim=True).clamp(min=1)
    return tot / n


# ---- time_embed
TE_D = (2, 3, 4, 5, 129, 512)
TE_T = (0, 1, 7, 200, 1000)
TE_MAX_STEPS = 10000


def te_ref64(t, d, max_steps=TE_MAX_STEPS, *, step_div=None, half1_bug=False, swap=False, kshift=0):
    """[sin a, cos a, 0 if d is odd], a = t f_k, f_k = exp(-lin_k), lin_k = k ln(max_steps) / (half - 1) (0 when half
    is 1: torch.linspace(.., steps=1) is its start), in float64, within C_te units of u (|a| (1 + lin_k) + 1): the fp32
    roundings of lin_k and of expf reach the argument scaled by |a|, the + 1 is the sine's own. The keyword arguments
    build the mutants of tests/test_cpu_cond_ref.py."""
    half = d // 2
    k = torch.arange(half, dtype=torch.float64) + kshift
    lm = float(np.log(float(max_steps)))
    div = (half - 1) if step_div is None else step_div
    lin = k * (lm / div) if half > 1 else torch.full((1,), lm if half1_bug else 0.0, dtype=torch.float64)
    a = t.double()[:, None] * torch.exp(-lin)[None, :]
    parts = [torch.cos(a), torch.sin(a)] if swap else [torch.sin(a), torch.cos(a)]
    unit = U24 * (a.abs() * (1.0 + lin)[None, :] + 1.0)
    pad = [torch.zeros(t.numel(), 1, dtype=torch.float64)] * (d % 2)
    unit = torch.cat([unit, unit] + pad, 1)
    return Ref(emb=torch.cat(parts + pad, 1), unit=unit, b=COND_C["te"] * unit)


# ---- RoPE (rope_fwd_kernel / rope_fwd_scalar, rope_bwd_kernel / rope_bwd_scalar); positions are r % L
# (N, L, d, one element into a buffer)
ROPE_CASES = [(18, 9, 128, False), (7, 7, 8, False), (12, 1, 16, False), (20, 5, 520, False),      # the vector kernels
              (18, 9, 2, False), (7, 3, 6, False), (18, 9, 128, True)]                             # the scalar ones


def rope_kernel_is_vector(d, off):
    """misc.hip vec_ok: d % 8 == 0 and every tensor on a 16-byte boundary (N d < 2^31 holds in every case)."""
    return d % 8 == 0 and not off


@functools.lru_cache(maxsize=None)
def rope_operands(N, L, d):
    """x, dy, dx_old [N, d] = randn times a power of two per row and per column (2^-2 .. 2^2); cos, sin [N, d]: the
    oracle's f32 tables for N >= L positions (the kernels read the first L rows)."""
    from oracle import fddm_oracle as O
    gen = _gen(N, L, d)
    sc = _pow2(gen, N)[:, None] * _pow2(gen, d)[None, :]
    x, dy, dx = (torch.randn(N, d, generator=gen) * sc for _ in range(3))
    cos, sin = O.rope_cos_sin(N, O.rope_inv_freq(d))
    return x, dy, dx, cos.contiguous(), sin.contiguous()


def _rope_pos(N, L, pos):
    return (torch.arange(N) % L) if pos is None else pos


def rope_fwd_ref64(x, cos, sin, L, *, pos=None, sin_sign=1.0, halves=False):
    """out[:, i] = x1 c - x2 s', out[:, h + i] = x1 s + x2 c' with x1 = x[:, 2i], x2 = x[:, 2i + 1], c, s the tables at
    column 2i and c', s' at 2i + 1, within 2 u (|x1 c| + |x2 s'|): two roundings, with or without contraction. The
    keyword arguments build the mutants (pos: positions; sin_sign; halves: pairs (i, i + h))."""
    N, d = x.shape
    h = d // 2
    p = _rope_pos(N, L, pos)
    xd, c, s = x.double(), cos.double()[p], sin.double()[p] * sin_sign
    x1, x2 = (xd[:, :h], xd[:, h:]) if halves else (xd[:, 0::2], xd[:, 1::2])
    t = [(x1 * c[:, 0::2], x2 * s[:, 1::2]), (x1 * s[:, 0::2], x2 * c[:, 1::2])]
    ref = torch.cat([t[0][0] - t[0][1], t[1][0] + t[1][1]], 1)
    return Ref(out=ref, b=2.0 * U24 * torch.cat([t[0][0].abs() + t[0][1].abs(), t[1][0].abs() + t[1][1].abs()], 1))


def rope_bwd_ref(dy, dx_old, cos, sin, L, *, pos=None, sin_sign=1.0, halves=False):
    """dx_new = dx_old + a C + b S at even columns, dx_old - a S + b C at odd ones (a = dy[:, i], b = dy[:, h + i];
    rope_bwd_ref64 above), within 3 u (|dx_old| + |a C| + |b S|): three roundings."""
    N, d = dy.shape
    p = _rope_pos(N, L, pos)
    c, s = cos.double()[p], sin.double()[p] * sin_sign      # gathered per row: rope_bwd_ref64 below takes them with L = N
    if halves:
        h = d // 2
        a, b = dy.double()[:, :h], dy.double()[:, h:]
        t = torch.cat([a * c[:, 0::2] + b * s[:, 0::2], -a * s[:, 1::2] + b * c[:, 1::2]], 1)
        m = torch.cat([(a * c[:, 0::2]).abs() + (b * s[:, 0::2]).abs(), (a * s[:, 1::2]).abs() + (b * c[:, 1::2]).abs()], 1)
    else:
        t = rope_bwd_ref64(dy.double(), c, s, N)
        m = rope_bwd_ref64(dy.double().abs(), c.abs(), s.abs(), N, magnitude=True)
    return Ref(dx=dx_old.double() + t, b=3.0 * U24 * (dx_old.double().abs() + m))


def rope_fwd_eval32(x, cos, sin, L, order):
    """The forward in fp32: order 0 rounds the second product and feeds the first through an FMA, order 1 the other
    way round, order 2 rounds both products (no contraction)."""
    N, d = x.shape
    p = torch.arange(N) % L
    c, s = cos[p], sin[p]
    x1, x2 = x[:, 0::2], x[:, 1::2]

    def comb(u, cu, v, cv):
        if order == 0:
            return _fma32(u, cu, v * cv)
        if order == 1:
            return _fma32(v, cv, u * cu)
        return u * cu + v * cv
    return torch.cat([comb(x1, c[:, 0::2], -x2, s[:, 1::2]), comb(x1, s[:, 0::2], x2, c[:, 1::2])], 1)


def rope_bwd_eval32(dy, dx_old, cos, sin, L, order):
    """The backward in fp32: t = a C + b S as in rope_fwd_eval32 (orders 0 - 2), then dx_old + t; order 3 is two chained
    FMAs onto dx_old."""
    N, d = dy.shape
    h = d // 2
    p = torch.arange(N) % L
    c, s = cos[p], sin[p]
    a, b = dy[:, :h], dy[:, h:]

    def comb(u, cu, v, cv, old):
        if order == 0:
            return old + _fma32(u, cu, v * cv)
        if order == 1:
            return old + _fma32(v, cv, u * cu)
        if order == 2:
            return old + (u * cu + v * cv)
        return _fma32(u, cu, _fma32(v, cv, old))
    out = torch.empty_like(dx_old)
    out[:, 0::2] = comb(a, c[:, 0::2], b, s[:, 0::2], dx_old[:, 0::2])
    out[:, 1::2] = comb(-a, s[:, 1::2], b, c[:, 1::2], dx_old[:, 1::2])
    return out


# ---- token embedding (embed_fwd_kernel / embed_fwd_scalar, embed_bwd_kernel)
# (d, L, B, V, pad_id): B L is no multiple of 8; rows 8 .. 15 (one whole block of embed_bwd) are padding
EMBED_CASES = [(8, 1, 21, 5, 0), (520, 3, 7, 50, 3), (6, 9, 3, 5, 3), (520, 9, 3, 5, 0), (8, 3, 7, 50, 0), (6, 1, 21, 50, 3)]


@functools.lru_cache(maxsize=None)
def embed_operands(d, L, B, V, pad_id):
    """tok [B L] int64 in [0, V) with rows 8 .. 15 and one more set to pad_id; E, dE_old [V, d], tbias, dtb_old [B, d],
    dx [B L, d]: randn times powers of two per row and column (2^-2 .. 2^2)."""
    gen = _gen(d, L, B, V, pad_id)
    N = B * L
    tok = torch.randint(0, V, (N,), generator=gen)
    tok[8:16] = pad_id
    tok[N - 2] = pad_id
    cs = _pow2(gen, d)[None, :]
    E, dE = (torch.randn(V, d, generator=gen) * _pow2(gen, V)[:, None] * cs for _ in range(2))
    tb, dtb = (torch.randn(B, d, generator=gen) * _pow2(gen, B)[:, None] * cs for _ in range(2))
    return tok, E, tb, torch.randn(N, d, generator=gen) * _pow2(gen, N)[:, None] * cs, dE, dtb


def embed_fwd_exact(tok, E, tbias, L):
    """E[tok] + tbias[r // L] in fp32 by torch: one IEEE add per element, so the kernel's bits."""
    x = E[tok]
    return x if tbias is None else x + tbias[torch.arange(tok.numel()) // L]


def embed_bwd_ref64(tok, dx, dE_old, dtb_old, L, pad_id, *, count_pad=False, dtb_shift=0):
    """dE_new[v] = dE_old[v] + the sum of dx over the rows naming v (none for pad_id), within n u (|old| + sum |dx|),
    n the number of such rows (n = 0: the old bits); dtb_new[b] = dtb_old[b] + sum_l dx[b, l] within (L + 1) u (..):
    L - k adds inside the blocks and k atomics for an entry spread over k blocks. The keyword arguments build the
    mutants."""
    V, d = dE_old.shape
    B = dtb_old.shape[0]
    dxd = dx.double()
    live = torch.ones_like(tok, dtype=torch.bool) if count_pad else tok != pad_id
    add = torch.zeros(V, d, dtype=torch.float64).index_add_(0, tok[live], dxd[live])
    mag = torch.zeros(V, d, dtype=torch.float64).index_add_(0, tok[live], dxd[live].abs())
    n = torch.zeros(V, dtype=torch.float64).index_add_(0, tok[live], torch.ones(int(live.sum()), dtype=torch.float64))
    tb = dxd.view(B, L, d).sum(1).roll(-dtb_shift, 0)
    tbm = dxd.abs().view(B, L, d).sum(1).roll(-dtb_shift, 0)
    return Ref(dE=dE_old.double() + add, b_dE=n[:, None] * U24 * (dE_old.double().abs() + mag), n=n,
               dtb=dtb_old.double() + tb, b_dtb=(L + 1) * U24 * (dtb_old.double().abs() + tbm))


# --------------------------------- the jumpy-sampler step (csrc/jumpy.hip: jump_kernel, ops.jump)
# The float64 reference of one jump, an fp32 emulation in the kernel's own evaluation order, the per-row bounds and
# the case table, shared by tests/test_cpu_jump_ref.py (which sets the constants from the reference and the
# emulation alone) and tests/test_gpu_jump.py (which runs the kernel).
#
# What the kernel rounds. The row max m and both argmax searches compare fp32 values: exact. The softmax normaliser
# s = sum_k expf(z_k - m) is an fp32 sum of fp32 terms, each with the rounding of z_k - m (which moves the term by
# u |d_k|, d_k = z_k - m) and of expf; 1 / s, x^_{x_t}, x^_o and both greedy scores are double. So a greedy decision
# carries one error, the relative error delta of s, common to p_x and p_o:
#     |margin - margin64| <= delta W,   W = ((a_cum + b_cum) a_tg p_x + b_cum a_tg p_o) / max(s_x, s_o)
#     delta <= (C_g + K_exp) u S,       S = sum_k e_k (1 + |d_k|) / sum_k e_k   (the absolute-value evaluation of s)
# A sampled score log(max(P_k, 1e-12)) / temp + g_k adds fp32 x^_k = expf(d_k) (float)(1 / s), P_k (delta once more
# through the normaliser Z of the exact posterior), logf, the product with 1 / temp, the Gumbel term and the last add:
#     |score_k - score64_k| <= (C_s + K_dev) u U_k
#     U_k = (2 S + (1 + |d_k|) + (1 + |lp_k|) + |lp_k|) / temp + (1 + |g_k|) + |score_k|,   lp_k = log max(P_k, 1e-12)
# E: the emulation's largest excess over every case in those units, measured on the CPU (numpy's correctly rounded
# fp32 exp / log): greedy 1.014, sample 0.711 (tests/test_cpu_jump_ref.py asserts measured <= stored <= 1.1 measured +
# 0.05). C = 8 E, hard cap 64. The device's __expf / __logf are not numpy's: their error has its own term K, from one
# grid on an MI355X against float64 (not from jump_kernel), in the units above:
#     __expf on [-87, 0], 2^22 points:                |err| / (u (1 + |x|) exp x)     <= JUMP_K["exp"]
#     __logf on [1e-12, 1], 2^22 + 2^16 points:       |err| / (u (1 + |log x|))       <= JUMP_K["log"]
#     -__logf(-__logf(u)) for all 2^23 draws u:       |err| / (u (1 + |g|))           <= JUMP_K["gum"]
# Below -87.3 expf's result is denormal and the device writes 0: an absolute 2^-126 per term, V 2^-126 relative to s >= 1.
JUMP_FAST, JUMP_SAMPLE = 1, 2
JUMP_E = {"greedy": 1.1, "sample": 0.75}
JUMP_E_FLOOR = 0.05
JUMP_C = {k: min(64.0, 8.0 * v) for k, v in JUMP_E.items()}
JUMP_K = {"exp": 1.5, "log": 3.5, "gum": 3.3}      # measured 1.204, 2.966, 2.977 (the last over every draw)
JUMP_K_DEV = max(JUMP_K.values())
JUMP_V = (2, 3, 63, 64, 65, 255, 256, 257, 260, 2003)
JUMP_SAMPLE_V = JUMP_V[:-1]                          # the draw is checked up to V = 260
JUMP_LAYOUTS = ("contig", "pad4", "pad1", "off1")    # ldz = V, V + 4, V + 1; the base one float past 16 bytes
JUMP_NL = tuple((N, L) for N in (1, 5, 64) for L in (1, 5, 16))
JUMP_SAMPLE_NL = ((64, 5), (64, 16), (5, 1), (1, 16))
JUMP_TEMPS = (0.7, 1.0, 2.0)
JUMP_T, JUMP_BETA_MAX, JUMP_DELTA = 200, 0.2, 5
JUMP_PAD = 1e30                                      # padding columns: an over-read changes the argmax
JUMP_SENTINEL = -0x5A5A5A5A5A5A5A5B                  # output buffers around the slice the kernel writes
JUMP_KINDS = ("rand", "tie4", "ninf", "bis+", "bis-", "tie64", "tie256", "tie2", "ru4", "ru64", "ru256", "ru2",
              "const", "rand", "ninf_x", "peaked")
JUMP_PEAK = 40.0                                     # logit spread of the peaked rows: most P on the 1e-12 clamp
JUMP_BISECT_AT = 4.0                                 # constructed rows sit at margin = +-4 bounds
# seeds whose draw of (row, class) is extreme for N = 64, V = 256, stream 7: every bit of h >> 41 set (and of h >> 40,
# contract v1's 24 bits), resp. clear (found by a CPU search; tests/test_cpu_jump_ref.py re-derives them)
JUMP_ONES = ((2678, 5, 144), (3227, 49, 149), (3651, 41, 176))
JUMP_ZERO = (200, 28, 109)
JUMP_STREAM = 7


def jump_is_vector(V, layout):
    """jump_kernel's float4 path: V and ldz multiples of 4 and a 16-byte aligned base."""
    return V % 4 == 0 and layout in ("contig", "pad4")


def jump_ldz(V, layout):
    return V + {"contig": 0, "pad4": 4, "pad1": 1, "off1": 0}[layout]


def _jump_rows(logits, xt, coef, L):
    z = np.asarray(logits, dtype=np.float64)
    N, V = z.shape
    x = np.clip(np.asarray(xt, dtype=np.int64), 0, V - 1)
    cf = np.asarray(coef, dtype=np.float32).reshape(-1, 4).astype(np.float64)[np.arange(N) // L]
    return z, N, V, x, cf


def jump_ref64(logits, xt, coef, L, mode=0, temperature=1.0, seed=0, stream=0):
    """One jump in float64, per row: `am` the first argmax (0 for a row without an orderable entry, NaN counting as
    -inf: torch.argmax's answer for an all -inf row), `o` the first argmax over k != x_t (x_t clamped into [0, V)),
    `sx`, `so` and `margin` = (sx - so) / max(sx, so), `choice` the greedy x_{t-delta} (fast mode: am), `munit` = S W,
    the margin's error scale (the comment above), `ok` False for a row without an orderable entry; with JUMP_SAMPLE
    also `score` [N, V] = log(max(P_k, 1e-12)) / temp + g_k with P from the float64 softmax and g from the contract's
    u in float64 (oracle.jump_uniform), `P`, `g`, and `unit` = U_k."""
    from oracle import fddm_oracle as O
    z, N, V, x, cf = _jump_rows(logits, xt, coef, L)
    r = np.arange(N)
    zc = np.where(np.isnan(z), -np.inf, z)
    m = zc.max(1)
    ok = np.isfinite(m)
    am = zc.argmax(1)
    zo = zc.copy()
    zo[r, x] = -np.inf
    o = np.where(np.isfinite(zo.max(1)), zo.argmax(1), np.where(x == 0, 1, 0))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = zc - m[:, None]
        e = np.exp(d)
        s = e.sum(1)
        xh = e / s[:, None]
        ad = np.where(e > 0, np.abs(d), 0.0)
        S = (e * (1.0 + ad)).sum(1) / s
        ac, bc, atg, btg = cf.T
        px, po = xh[r, x], xh[r, o]
        sx = (ac + bc) * (atg * px + btg)
        so = bc * (atg * po + btg)
        top = np.maximum(np.maximum(sx, so), 1e-300)
        margin = (sx - so) / top
        W = ((ac + bc) * atg * px + bc * atg * po) / top
    choice = am if mode & JUMP_FAST else np.where((sx > so) | ((sx == so) & (x < o)), x, o)
    out = Ref(am=am, o=o, x=x, sx=sx, so=so, margin=margin, choice=choice, S=S, munit=S * W, ok=ok, xh=xh)
    if mode & JUMP_SAMPLE:
        temp = float(np.float32(temperature))
        with np.errstate(invalid="ignore", divide="ignore"):
            if mode & JUMP_FAST:
                P = ac[:, None] * xh + (1.0 - ac[:, None]) / V
            else:
                A = np.broadcast_to(bc[:, None], (N, V)).copy()
                A[r, x] += ac
                un = A * (atg[:, None] * xh + btg[:, None])
                P = un / un.sum(1, keepdims=True)
            lp = np.log(np.maximum(P, 1e-12))
            h = O.mix64(seed, stream, r[:, None].astype(np.uint64) * np.uint64(V) + np.arange(V, dtype=np.uint64)[None])
            g = -np.log(-np.log(O.jump_uniform(h)))
            score = lp / temp + g
            unit = (2.0 * S[:, None] + (1.0 + ad) + (1.0 + np.abs(lp)) + np.abs(lp)) / temp + (1.0 + np.abs(g)) + \
                np.abs(score)
        out.__dict__.update(P=P, g=g, score=score, unit=unit, lp=lp)
    return out


def jump_greedy_bound(ref, V, C=None):
    """Per row: how far the kernel's margin may lie from ref.margin."""
    C = JUMP_C["greedy"] if C is None else C
    return (C + JUMP_K["exp"]) * U24 * ref.munit + V * 2.0 ** -126 + 2.0 ** -48


def jump_sample_bound(ref, C=None):
    """Per row: a class whose float64 score lies further than this under the row's best cannot win on the kernel
    (twice the largest per-class score error)."""
    C = JUMP_C["sample"] if C is None else C
    return 2.0 * ((C + JUMP_K_DEV) * U24 * ref.unit).max(1)


def jump_candidates(ref):
    """[N, V] bool: the classes the kernel may draw."""
    return ref.score >= (ref.score.max(1) - jump_sample_bound(ref))[:, None]


def jump_emulate(logits, xt, coef, L, mode=0, temperature=1.0, seed=0, stream=0, vector=False):
    """The kernel's own evaluation in numpy: fp32 expf terms summed per lane in the kernel's order (float4 path: lane l
    takes k = 4 l + 256 p .. + 3, `sum += ((e0 + e1) + e2) + e3`; scalar path: k = l + 64 p), the xor tree of wave_sum,
    then the double-precision tail for p_x, p_o, s_x, s_o; with JUMP_SAMPLE the fp32 x^, P, logf and Gumbel term.
    Returns (margin [N], score [N, V] or None). Rows need an orderable entry."""
    from oracle import fddm_oracle as O
    f = np.float32
    z64, N, V, x, cf = _jump_rows(logits, xt, coef, L)
    z = np.asarray(logits, dtype=f)
    r = np.arange(N)
    m = z.max(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.exp((z - m[:, None]).astype(f)).astype(f)
        span = 256 if vector else 64
        Wd = -(-V // span) * span
        ep = np.zeros((N, Wd), dtype=f)
        ep[:, :V] = e
        lanes = np.zeros((N, 64), dtype=f)
        if vector:
            q = ep.reshape(N, Wd // 256, 64, 4)
            for p in range(Wd // 256):
                lanes = lanes + (((q[:, p, :, 0] + q[:, p, :, 1]) + q[:, p, :, 2]) + q[:, p, :, 3])
        else:
            q = ep.reshape(N, Wd // 64, 64)
            for p in range(Wd // 64):
                lanes = lanes + q[:, p]
        idx = np.arange(64)
        for sft in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ sft]
        assert lanes.dtype == f
        s = lanes[:, 0]
        inv_s = 1.0 / s.astype(np.float64)
        zo = z64.copy()
        zo[r, x] = -np.inf
        oval = zo.max(1)
        ac, bc, atg, btg = cf.T
        px = np.exp(z64[r, x] - m.astype(np.float64)) * inv_s
        po = np.exp(oval - m.astype(np.float64)) * inv_s
        sx = (ac + bc) * (atg * px + btg)
        so = bc * (atg * po + btg)
        margin = (sx - so) / np.maximum(np.maximum(sx, so), 1e-300)
        if not mode & JUMP_SAMPLE:
            return margin, None
        inv_sf = inv_s.astype(f)
        xh = e * inv_sf[:, None]
        assert xh.dtype == f
        if mode & JUMP_FAST:
            ab = ac.astype(f)[:, None]
            P = ab * xh + ((f(1.0) - ab) / f(V))
        else:
            Zn = bc * (atg + V * btg) + ac * (atg * px + btg)
            A = np.broadcast_to(bc[:, None], (N, V)).copy()
            A[r, x] += ac
            P = (A * (atg[:, None] * xh.astype(np.float64) + btg[:, None]) / Zn[:, None]).astype(f)
        assert P.dtype == f
        h = O.mix64(seed, stream, r[:, None].astype(np.uint64) * np.uint64(V) + np.arange(V, dtype=np.uint64)[None])
        u = O.jump_uniform(h, f)
        g = -np.log(-np.log(u))
        inv_temp = f(1.0) / f(temperature)
        score = np.log(np.maximum(P, f(1e-12))) * inv_temp + g
        assert u.dtype == f and g.dtype == f and score.dtype == f
    return margin, score


def jump_coefs(V, B, fast):
    """[B, 4] f32 step coefficients, different per batch element: exact {a_cum, b_cum, a_tg, b_tg} of a jump of
    JUMP_DELTA from t_b (oracle.jump_coeffs), fast {abar_{t_b - delta}, 0, 0, 0}. Element B // 2 has t - delta = 0:
    a_tg = 1, b_tg = 0, abar = 1."""
    from oracle import fddm_oracle as O
    betas, abar = (np.asarray(v, dtype=np.float32) for v in O.sched_tables(JUMP_T, JUMP_BETA_MAX))
    ts = [JUMP_DELTA + (53 * b + 17) % (JUMP_T - JUMP_DELTA + 1) for b in range(B)]
    ts[B // 2] = JUMP_DELTA
    c = np.zeros((B, 4), dtype=np.float32)
    for b, t in enumerate(ts):
        if fast:
            c[b, 0] = abar[t - JUMP_DELTA - 1] if t > JUMP_DELTA else 1.0
        else:
            c[b] = O.jump_coeffs(betas, V, JUMP_T, t, JUMP_DELTA)
    return c


def _jump_pair(kind, V, gen):
    """Two classes that share a float4 ("4"), a lane on consecutive passes of the scalar ("64") or the float4 path
    ("256"), or neither ("2"); the nearest placement that fits V otherwise."""
    ri = lambda n: int(torch.randint(0, max(1, n), (1,), generator=gen))
    if kind == "4":
        if V >= 4:
            k = 4 * ri((V - 3) // 4 + 1) + 1
            return k, k + 1
        return V - 2, V - 1
    if kind == "256" and V > 256:
        k = ri(V - 256)
        return k, k + 256
    if kind in ("64", "256") and V > 64:
        k = ri(V - 64)
        return k, k + 64
    if V > 9:
        k = ri(V - 9)
        return k, k + 9
    return 0, V - 1


@functools.lru_cache(maxsize=None)
def jump_case(V, N, L):
    """Inputs of case (V, N, L), the same for every layout: `logits` [N, V] f32, `xt` [N] (0, V - 1, the argmax, a
    non-argmax, -1, V + 5 in turn), `coef` / `coef_fast` [B, 4], `kinds` per row (JUMP_KINDS, rotated per case so that N
    = 1 and 5 meet different ones) and `built` [N]: +-1 on the rows whose logit at x_t was bisected until the exact
    greedy margin sits at +-JUMP_BISECT_AT bounds, 0 elsewhere (a "bis" row on which no logit reaches that margin stays
    an ordinary row)."""
    gen = _gen(7001, V, N, L)
    B = (N + L - 1) // L
    coef, coef_fast = jump_coefs(V, B, False), jump_coefs(V, B, True)
    z = (3.0 * torch.randn(N, V, generator=gen)).numpy().astype(np.float32)
    rot = (V + 3 * N + 5 * L) % 16
    kinds = [JUMP_KINDS[(r + rot) % 16] for r in range(N)]
    xt = np.zeros(N, dtype=np.int64)
    for r, kind in enumerate(kinds):
        top = float(np.abs(z[r]).max())
        if kind == "peaked":
            z[r] = (JUMP_PEAK * torch.rand(V, generator=gen) ** 3).numpy()       # two thirds more than 27.6 under the top
            z[r, int(torch.randint(0, V, (1,), generator=gen))] = JUMP_PEAK
            z[r, int(torch.randint(0, V, (1,), generator=gen))] = 0.0
        elif kind == "const":
            z[r] = z[r, 0]
        elif kind.startswith("tie"):
            k1, k2 = _jump_pair(kind[3:], V, gen)
            z[r, k1] = z[r, k2] = top + 1.5
        elif kind.startswith("ru") and V > 2:
            k1, k2 = _jump_pair(kind[2:], V, gen)
            p = (k2 + 3) % V
            while p in (k1, k2):
                p = (p + 1) % V
            z[r, k1] = z[r, k2] = top + 1.5
            z[r, p] = top + 3.0
        am = int(z[r].argmax())
        xk = (r + rot // 2) % 6
        xt[r] = (0, V - 1, am, (am + 1 + int(torch.randint(0, V - 1, (1,), generator=gen))) % V, -1, V + 5)[xk]
        if kind.startswith("ru") and V > 2:
            xt[r] = am
        x = min(max(int(xt[r]), 0), V - 1)
        if kind in ("ninf", "ninf_x"):
            hole = (torch.rand(V, generator=gen) < 0.3).numpy()
            keep = (x + 1 + r % (V - 1)) % V            # a finite class other than x_t
            hole[keep] = False
            hole[x] = kind == "ninf_x"
            z[r, hole] = -np.inf
    built = np.zeros(N, dtype=np.int64)
    for r, kind in enumerate(kinds):
        if kind in ("bis+", "bis-"):
            built[r] = _jump_bisect_row(z, xt, coef, L, r, 1 if kind == "bis+" else -1)
    for a in (z, xt, coef, coef_fast, built):
        a.setflags(write=False)
    return dict(logits=z, xt=xt, coef=coef, coef_fast=coef_fast, kinds=kinds, built=built, V=V, N=N, L=L)


def _jump_bisect_row(z, xt, coef, L, r, sign):
    """Move z[r, x_t] until the row's exact greedy margin is sign * JUMP_BISECT_AT bounds; the best other class gets
    most of the mass first, so that the margin changes sign over the range. Returns sign, or 0 with the row restored."""
    V = z.shape[1]
    x = min(max(int(xt[r]), 0), V - 1)
    saved = z[r].copy()
    o = (x + 1 + r % (V - 1)) % V
    z[r, o] = np.abs(saved).max() + 4.0
    lo, hi = float(z[r, o]) - 40.0, 48.0
    cf = coef[r // L][None]

    def ref_at(v):
        row = z[r:r + 1].copy()
        row[0, x] = np.float32(lo + v)
        return jump_ref64(row, [x], cf, 1)

    def f(v, k):
        q = ref_at(v)
        return float(q.margin[0] - sign * k * jump_greedy_bound(q, V)[0])

    if not (f(0.0, JUMP_BISECT_AT) < 0.0 < f(hi, JUMP_BISECT_AT)):
        z[r] = saved
        return 0
    v = _bisect(lambda t: f(t, JUMP_BISECT_AT), hi, target=0.0, steps=60)
    z[r, x] = np.float32(lo + v)
    q = jump_ref64(z[r:r + 1], [x], cf, 1)
    k = float(q.margin[0] / jump_greedy_bound(q, V)[0]) * sign
    if not JUMP_BISECT_AT - 1.0 <= k <= JUMP_BISECT_AT + 1.0:      # fp32 steps of the logit too coarse for this row
        z[r] = saved
        return 0
    return sign


@functools.lru_cache(maxsize=None)
def jump_case_ref(V, N, L, mode, temperature=1.0):
    """(reference, seed) of case (V, N, L) under `mode`, computed once."""
    c = jump_case(V, N, L)
    seed = 1000 + 7 * V + 3 * N + L
    return jump_ref64(c["logits"], c["xt"], c["coef_fast"] if mode & JUMP_FAST else c["coef"], L, mode, temperature,
                      seed, JUMP_STREAM), seed


def jump_extreme_case(which):
    """N = 64, V = 256 rows whose draw of one (row, class) is extreme. which = 0, 1, 2: the JUMP_ONES seeds, every bit of
    the draw set; that class gets a probability under the 1e-12 clamp and class 3 nearly all the mass, so the reference
    picks class 3 by a wide margin (u = 1 and a Gumbel term of +inf pick the clamped class instead). which = "zero": the
    draw with every bit clear (JUMP_ZERO); its class gets nearly all the mass and still loses only if its Gumbel term is
    far below -log(-log 2^-24) = -2.81."""
    seed, row, k = JUMP_ONES[which] if which != "zero" else JUMP_ZERO
    N, V, L = 64, 256, 64          # one batch element, t - delta = 0: b_tg = 0 and abar = 1, so P can reach the clamp
    z = (1.0 * torch.randn(N, V, generator=_gen(7002, seed))).numpy().astype(np.float32)
    if which == "zero":
        z[row, k] = 14.0
    else:
        z[row, k] = -36.0
        z[row, 3] = 14.0
    xt = np.full(N, k if which == "zero" else 3, dtype=np.int64)      # x_t on the favoured class: a_cum is on its side
    return dict(logits=z, xt=xt, coef=jump_coefs(V, N // L, False), coef_fast=jump_coefs(V, N // L, True), V=V, N=N,
                L=L, seed=seed, row=row, k=k)


@functools.lru_cache(maxsize=None)
def jump_peaked_case():
    """N = 64, V = 260, every row with a logit spread of JUMP_PEAK and one batch element with t - delta = 0 (b_tg = 0, abar
    = 1: nothing but x^ keeps P off the floor), so that most P sit on the 1e-12 clamp."""
    N, V, L = 64, 260, 64
    gen = _gen(7004)
    z = (JUMP_PEAK * torch.rand(N, V, generator=gen) ** 3).numpy().astype(np.float32)
    r = np.arange(N)
    z[r, (7 * r) % V] = JUMP_PEAK
    z[r, (7 * r + 1) % V] = 0.0
    xt = torch.randint(0, V, (N,), generator=gen).numpy()
    return dict(logits=z, xt=xt, coef=jump_coefs(V, 1, False), coef_fast=jump_coefs(V, 1, True), V=V, N=N, L=L, seed=4242)


# ----------------------------------------------- LayerNorm / FiLM (csrc/norm.hip) and L_fd (csrc/lfd.hip)
# References, per-element error scales, inputs, emulations and case tables shared by tests/test_cpu_norm_lfd_ref.py
# (which sets the constants below from the reference alone) and tests/test_gpu_norm_lfd_elem.py (which runs the kernels).
# E: the fp32 evaluation in each kernel's own summation order (ln_fwd_emulate, ln_bwd_emulate, lfd_emulate: 8 elements
# per lane, wave_sum_v's tree, the slab's 8-wave / 4-wave LDS combine, the fold's 16 groups, the column loops of
# lfd.hip) against float64 in units of 2^-24 times the per-element scale, the maximum over every case below, measured
# on the CPU (tests/test_cpu_norm_lfd_ref.py asserts measured <= stored <= 1.1 measured + NORM_E_FLOOR). The kernels are
# allowed NORM_C = 8 E units (contraction, the device's sqrtf and division), hard cap 64.
NORM_E = {"mean": 2.8, "rstd": 3.45, "out": 2.8, "dres": 3.85, "par": 3.85,
          "lfd_is": 3.8, "lfd_zt": 4.4, "lfd_col": 6.15, "lfd_dz": 3.2, "lfd_loss": 1.55}
NORM_C = {k: min(64.0, 8.0 * v) for k, v in NORM_E.items()}
NORM_E_FLOOR = 0.05
LN_EPS = 1e-5
LN_SLAB = 32                   # rows per workgroup of ln_bwd_fused_kernel (norm.hip LNB_ROWS)
LN_PROWS = 64                  # rows per workgroup of ln_bwd_params_kernel (norm.hip LNP_ROWS)
LN_SEED, LN_STREAM = 20240611, 5
LN_P = (0.1, 0.5, 2.0 ** -16, 1e-6, 0.0)       # thresholds 6554, 32768, 1, 0 (p > 0) and no dropout
LN_TRIPLES = (("f32", "bf16", "bf16"), ("f32", "f32", "f32"), ("bf16", "bf16", "bf16"), ("f32", "f32", "bf16"))
_TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def ln_thr(p):
    """norm.hip's thr16 = llrintf(p 65536) for p > 0 (round to nearest even of the fp32 product), else 0."""
    return int(np.rint(np.float32(p) * np.float32(65536.0))) if p > 0 else 0


def ln_drop_scale(p):
    """The exact 1 / (1 - p) of the fp32 p where a threshold exists; 1 where thr16 = 0 (p = 0 and 0 < p < 2^-17: DESIGN
    §2 — nothing is dropped, nothing is scaled). The kernel's fp32 1.f / (1.f - p) is within two roundings of it."""
    return 1.0 / (1.0 - float(np.float32(p))) if ln_thr(p) else 1.0


def ln_keep(N, d, p):
    from oracle import fddm_oracle as O
    if not ln_thr(p):
        return torch.ones(N, d, dtype=torch.bool)
    return O.dropout_keep(LN_SEED, LN_STREAM, N * d, p).view(N, d)


def ln_fwd_dispatch(xdt, ydt, odt, hy, hf, d, rope=False):
    """fddm_ln_fwd's choice of build (norm.hip): (x, y, out dtype, HY, HF, CH, RP), or None where it refuses."""
    if d <= 0 or d > 1024 or d % 8:
        return None
    ch = 1 if d <= 512 else 2
    if rope:
        if (xdt, ydt, odt) != LN_TRIPLES[0] or not hy or hf or d % 16:
            return None
        return (xdt, ydt, odt, True, False, ch, True)
    return (xdt, ydt, odt, hy, hf, ch, False) if (xdt, ydt, odt) in LN_TRIPLES else None


def ln_fwd_codes(xdt, ydt, odt):
    """The dtype triple ops.ln_fwd passes for x, y (None: absent) and out_t (always given here)."""
    return (xdt, ydt if ydt is not None else xdt, odt)


# every build ops.ln_fwd can launch: without y the y code is x's, so (f32, bf16, bf16) exists only with HY
LN_FWD_BUILDS = tuple((*tr, hy, hf, ch, False) for tr in LN_TRIPLES for hy in (True, False) for hf in (True, False)
                      for ch in (1, 2) if hy or tr[0] == tr[1]) + tuple((*LN_TRIPLES[0], True, False, ch, True) for ch in (1, 2))


def ln_fwd_cases():
    """dicts: id, tr (dtype triple), hy, hf, N, d, L (rows per FiLM batch, 0: none), p, rope (L of the tables, 0: none),
    alias (save_s in place over x), k0 (the first row's kind, ln_rows)."""
    out = []
    D1, D2, NS, BL = (8, 200, 512), (520, 1024), (1, 5, 33, 70), ((5, 1), (2, 20), (2, 32), (2, 37))

    def add(tr, hy, hf, N, d, L, p, rope=0, alias=False):
        i = len(out)
        out.append(dict(id=f"{i:02d}-{'-'.join(tr)}-{'y' if hy else 'n'}{'f' if hf else 'n'}-N{N}-d{d}-L{L}-p{p:.2g}"
                        + ("-rope" if rope else "") + ("-alias" if alias else ""),
                        tr=tr, hy=hy, hf=hf, N=N, d=d, L=L, p=p, rope=rope, alias=alias, k0=i))
    for tr in LN_TRIPLES:
        for hy in (True, False):
            for hf in (True, False):
                for ch in (1, 2):
                    if not hy and tr[0] != tr[1]:
                        continue
                    i = len(out)
                    d = D1[i % 3] if ch == 1 else D2[i % 2]
                    B, L = BL[i % 4] if hf else (NS[i % 4], 0)
                    add(tr, hy, hf, B * L if hf else B, d, L, LN_P[i % 5] if hy else 0.0, alias=tr[0] == "f32" and i % 3 == 0)
    add(LN_TRIPLES[0], True, False, 18, 128, 0, 0.1, rope=9)
    add(LN_TRIPLES[0], True, False, 10, 528, 0, 0.5, rope=5)
    for j, p in enumerate(LN_P):                       # every p with every row kind, at the tail shapes
        add(LN_TRIPLES[j % 4], True, j % 2 == 0, 14 if j % 2 else 74, (200, 520)[j % 2], 0 if j % 2 else 37, p)
    add(LN_TRIPLES[1], True, True, 2 * 576, 8, 576, 0.1)
    add(LN_TRIPLES[2], True, True, 64, 512, 32, 0.5)
    add(LN_TRIPLES[0], True, False, 1, 512, 0, 0.1)
    add(LN_TRIPLES[3], False, False, 1, 1024, 0, 0.0)
    add(LN_TRIPLES[1], False, False, 70, 8, 0, 0.0)
    add(LN_TRIPLES[2], False, False, 33, 520, 0, 0.0)
    add(LN_TRIPLES[1], False, False, 14, 200, 0, 0.0)
    return out


LN_KINDS = ("flat", "offset", "outlier", "const", "zero", "tiny", "flat")


def ln_rows(gen, N, d, k0, hy):
    """x, y [N, d] f32: randn times a power of two per row and per column; row r is of kind LN_KINDS[(r + k0) % 7]:
    offset = a common offset of 64 row standard deviations, outlier = one channel 2^8 above the loudest, const, zero,
    tiny = 2^-20-sized values. y is nowhere zero (|y| >= 0.05 of its scale); on const and zero rows it is 2^-30-sized, so
    that the row's fp32 sum x + y is x (variance 0 in the kernel, < 2^-58 in the reference: rstd = eps^-1/2 either way)."""
    rp, cp = _pow2(gen, N), _pow2(gen, d)
    sc = rp[:, None] * cp[None, :]
    x = torch.randn(N, d, generator=gen) * sc
    y = (torch.randn(N, d, generator=gen).abs() + 0.05) * (torch.randint(0, 2, (N, d), generator=gen) * 2.0 - 1.0) * sc
    kind = (torch.arange(N) + k0) % 7
    xo = x[kind == 1]
    x[kind == 1] += 64.0 * (xo - xo.mean(1, keepdim=True)).pow(2).mean(1, keepdim=True).sqrt().clamp_min(rp[kind == 1, None])
    r = torch.nonzero(kind == 2)[:, 0]
    x[r, (7 * r) % d] = 2.0 ** 8 * 4.0 * rp[r]
    x[kind == 3] = (1.5 * rp[kind == 3])[:, None].expand(-1, d)
    x[kind == 4] = 0.0
    x[kind == 5] *= 2.0 ** -20
    y[(kind == 3) | (kind == 4)] *= 2.0 ** -30
    y[kind == 5] *= 2.0 ** -20
    return x, (y if hy else None), kind


def ln_affine(gen, d, B=0):
    """gamma (zeros at c % 5 = 2, negative entries), beta; with B: FiLM scale [B, d] (exactly -1 at c % 7 = 1, +-4 at
    c % 11 = 3) and shift."""
    gamma, beta = torch.randn(d, generator=gen), 0.5 * torch.randn(d, generator=gen)
    gamma[2::5] = 0.0
    if d > 1:
        gamma[1::4] = -gamma[1::4].abs()
    if not B:
        return gamma, beta, None
    fs, fh = 0.5 * torch.randn(B, d, generator=gen), torch.randn(B, d, generator=gen)
    fs[:, 1::7] = -1.0
    fs[:, 3::11] = 4.0 * torch.sign(fs[:, 3::11] + 1e-9)
    return gamma, beta, (fs.contiguous(), fh.contiguous())


@functools.lru_cache(maxsize=None)
def ln_fwd_operands(i):
    """x, y in their storage dtypes (y None without HY), gamma, beta, film or None, keep [N, d], (cos, sin) or None."""
    from oracle import fddm_oracle as O
    c = ln_fwd_cases()[i]
    gen = _gen(8100, i)
    x, y, kind = ln_rows(gen, c["N"], c["d"], c["k0"], c["hy"])
    gamma, beta, film = ln_affine(gen, c["d"], c["N"] // c["L"] if c["hf"] else 0)
    x = x.to(_TDT[c["tr"][0]])
    y = y.to(_TDT[c["tr"][1]]) if y is not None else None
    rope = None
    if c["rope"]:
        cos, sin = O.rope_cos_sin(c["N"], O.rope_inv_freq(c["d"]))      # the kernel reads the first c["rope"] rows
        rope = (cos.contiguous(), sin.contiguous())
    return x, y, gamma, beta, film, ln_keep(c["N"], c["d"], c["p"]), rope, kind


def ln_fwd_ref64(x, y, gamma, beta, film, L, p, keep, *, eps=LN_EPS, rope=None, rope_L=0, mut=None):
    """float64 on the operands as stored. v = x + y keep / (1 - p), m, rstd = (var + eps)^-1/2, out = (v - m) rstd gamma
    + beta (then (1 + fs[b]) . + fh[b], b = row // L), and per element the scale each may be wrong by, in units of u:
      s     sv = 3 |t| + |v|  (t = y keep / (1 - p): 1 - p, the quotient, the product; then the add; with or without
            contraction); |v| without dropout; 0 without y (a copy)
      mean  M = mean_j (|v_j| + sv_j)
      rstd  rstd (1 + rstd^2 mean_j (|v_j - m| sv_j)): its own roundings, and d var = 2 mean (v - m) dv
      out   |gamma| (rstd (|v - m| + M + sv) + |v - m| u_rstd) + |beta|, through FiLM times |1 + fs|, plus |fh|
    `mut` builds the mutants of tests/test_cpu_norm_lfd_ref.py."""
    N, d = x.shape
    xd = x.double()
    thr = ln_thr(p)
    if y is None:
        v, sv = xd, torch.zeros_like(xd)
    elif thr == 0:
        v = xd + y.double()
        sv = v.abs()
    else:
        k = keep.reshape(-1).roll(-1).view(N, d) if mut == "mask_next" else keep
        t = y.double() * k.double() * (1.0 if mut == "noscale" else ln_drop_scale(p))
        v = xd + t
        sv = 3.0 * t.abs() + v.abs()
    m = v.mean(1, keepdim=True)
    c = v - m
    var = (c * c).mean(1, keepdim=True)
    if mut == "unbiased":
        var = var * d / max(d - 1, 1)
    elif mut == "onepass":                              # fp32 E[v^2] - m^2
        v32 = v.float()
        m32 = v32.mean(1, keepdim=True)
        m, var = m32.double(), ((v32 * v32).mean(1, keepdim=True) - m32 * m32).double().clamp_min(0.0)
        c = v - m
    elif mut == "tail":                                 # the lanes past the row end count the chunk they re-loaded
        n = 64 * (1 if d <= 512 else 2) - d // 8
        m = (v.sum(1, keepdim=True) + n * v[:, -8:].sum(1, keepdim=True)) / d
        c = v - m
        var = ((c * c).sum(1, keepdim=True) + n * (c[:, -8:] ** 2).sum(1, keepdim=True)) / d
    rstd = 1.0 / (var.sqrt() + eps) if mut == "eps_out" else 1.0 / torch.sqrt(var + eps)
    M = (v.abs() + sv).mean(1, keepdim=True)
    u_rstd = rstd * (1.0 + rstd ** 2 * (c.abs() * sv).mean(1, keepdim=True))
    g, b = gamma.double()[None, :], beta.double()[None, :]
    out = c * rstd * g + b
    u_out = g.abs() * (rstd * (c.abs() + M + sv) + c.abs() * u_rstd) + b.abs()
    if film is not None:
        row = torch.arange(N)
        bi = ((row - 1).clamp_min(0) if mut == "film_prev" else row) // L
        fs, fh = film[0].double()[bi], film[1].double()[bi]
        f1 = fs if mut == "fs" else 1.0 + fs
        out = out * f1 + fh
        u_out = u_out * f1.abs() + fh.abs()
    r = Ref(s=v, u_s=sv, mean=m[:, 0], u_mean=M[:, 0], rstd=rstd[:, 0], u_rstd=u_rstd[:, 0], out=out, u_out=u_out)
    r.b_s = U24 * sv * (1.0 + 2.0 ** -20)
    r.b_mean, r.b_rstd, r.b_out = NORM_C["mean"] * U24 * r.u_mean, NORM_C["rstd"] * U24 * r.u_rstd, NORM_C["out"] * U24 * u_out
    r.b_out_bf = bf16_round_bound(out, r.b_out)
    if rope is not None:
        pos = torch.arange(N) if mut == "rope_pos" else None
        q = rope_fwd_ref64(out, rope[0], rope[1], rope_L, pos=pos, sin_sign=-1.0 if mut == "rope_sign" else 1.0)
        pm = _rope_pos(N, rope_L, None)
        ca, sa = rope[0].double()[pm].abs(), rope[1].double()[pm].abs()
        b1, b2 = r.b_out[:, 0::2], r.b_out[:, 1::2]
        carried = torch.cat([b1 * ca[:, 0::2] + b2 * sa[:, 1::2], b1 * sa[:, 0::2] + b2 * ca[:, 1::2]], 1)
        r.rope, r.b_rope = q.out, bf16_round_bound(q.out, q.b + carried)
    return r


def _tree64(t):
    """wave_sum_v (norm.hip): lanes l and l ^ 1, ^ 2, ^ 4 (row_half_mirror of equal quads), ^ 8 (row_mirror), ^ 16, ^ 32
    (the permlane swaps), every addend pair the same on both lanes: six rounds of adjacent pairs. t [..., 64] fp32."""
    for _ in range(6):
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _seq(t):
    """Sum over the last axis, one fp32 accumulator from 0 in index order."""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def ln_rowsum32(t, vec):
    """A row sum of t [N, d] fp32 as the kernels take it. vec: a lane adds the 8 elements of chunk lane, then of chunk
    lane + 64 (ln_fwd_kernel, ln_bwd_fused_kernel); else elements lane, lane + 64, ... (ln_bwd_kernel); then the tree."""
    N, d = t.shape
    if vec:
        ch = 1 if d <= 512 else 2
        p = torch.zeros(N, ch * 512)
        p[:, :d] = t
        lanes = p.view(N, ch, 64, 8).permute(0, 2, 1, 3).reshape(N, 64, ch * 8)
    else:
        p = torch.zeros(N, 1024)
        p[:, :d] = t
        lanes = p.view(N, 16, 64).permute(0, 2, 1)
    return _tree64(_seq(lanes))


def ln_fwd_emulate(x, y, gamma, beta, film, L, p, keep, eps=LN_EPS, fma=False):
    """ln_fwd_kernel in fp32 on the CPU: s, mean, rstd, out. fma: the dropout product through an FMA."""
    N, d = x.shape
    v = x.float()
    if y is not None:
        if ln_thr(p):
            ds = (np.float32(1.0) / (np.float32(1.0) - np.float32(p))).item()
            ds = torch.tensor(ds, dtype=torch.float32)
            kf = keep.float()
            v = _fma32(y.float() * kf, ds.expand(N, d), v) if fma else v + y.float() * kf * ds
        else:
            v = v + y.float()
    fd = torch.tensor(float(d), dtype=torch.float32)
    mean = (ln_rowsum32(v, True) / fd)[:, None]
    t = v - mean
    var = ln_rowsum32(t * t, True) / fd
    rstd = (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))[:, None]
    o = (v - mean) * rstd * gamma[None, :] + beta[None, :]
    if film is not None:
        bi = torch.arange(N) // L
        o = o * (1.0 + film[0][bi]) + film[1][bi]
    return v, mean[:, 0], rstd[:, 0], o


# ---- LayerNorm backward
def ln_bwd_dispatch(d, N, L, film, params, aligned=True, beta=True):
    """fddm_ln_bwd's choice (norm.hip): ("fused", CH) or ("rows",) / ("rows", "params")."""
    vec_ok = d % 8 == 0 and d <= 1024 and aligned
    rpb = L if L > 0 else N
    if params and (not film or rpb % LN_SLAB == 0) and beta and vec_ok:
        return ("fused", 1 if d <= 512 else 2)
    return ("rows", "params") if params else ("rows",)


# (kernel, dy dtype, partials, FiLM): the fused builds; ("rows", dy dtype, with ln_bwd_params_kernel): the two-pass form
LN_BWD_BUILDS = tuple((("fused", ch), dt, part, film) for ch in (1, 2) for dt in ("f32", "bf16") for part in (False, True)
                      for film in (False, True)) + tuple(("rows", dt, par) for dt in ("f32", "bf16") for par in (False, True))


def ln_bwd_cases():
    """dicts: id, d, N, L (0: no FiLM), dt (dy_t's dtype), p, part (LnPartials), params (parameter gradients wanted),
    off4 (dres one float into its buffer: the unvectorised path)."""
    out = []

    def add(d, N, L, dt, p, part=False, params=True, off4=False):
        i = len(out)
        out.append(dict(id=f"{i:02d}-d{d}-N{N}-L{L}-{dt}-p{p:.2g}" + ("-part" if part else "") + ("" if params else "-nopar")
                        + ("-off4" if off4 else ""), d=d, N=N, L=L, dt=dt, p=p, part=part, params=params, off4=off4, k0=i))
    D1, D2, NS, BL = (8, 200, 512), (520, 1024), (1, 5, 33, 70), ((2, 32), (3, 32))
    for ch in (1, 2):
        for dt in ("f32", "bf16"):
            for part in (False, True):
                for film in (False, True):
                    i = len(out)
                    d = D1[i % 3] if ch == 1 else D2[i % 2]
                    B, L = BL[i % 2] if film else (NS[i % 4], 0)
                    add(d, B * L if film else B, L, dt, LN_P[i % 5], part)
    add(200, 1100, 0, "bf16", 0.1, True)               # 35 slabs: three fold rounds, a ragged last slab
    add(200, 1100, 0, "f32", 0.5, False)
    add(8, 2 * 576, 576, "bf16", 0.1, True)            # 18 slabs per FiLM batch: fold group 15 exists
    add(8, 70, 0, "f32", 2.0 ** -16, True)
    add(520, 70, 0, "bf16", 1e-6, False)
    add(100, 70, 0, "f32", 0.1)                        # the two-pass form: d % 8 != 0
    add(100, 33, 0, "bf16", 0.5, params=False)
    add(1, 5, 0, "f32", 0.0)
    add(1, 70, 1, "bf16", 0.1)
    add(200, 5, 1, "f32", 0.1)                         # FiLM, a batch per row
    add(512, 40, 20, "bf16", 0.5)                      # FiLM, batches inside a slab
    add(8, 74, 37, "f32", 1e-6)                        # FiLM, a 64-row params workgroup over two batches
    add(200, 33, 0, "f32", 0.1, off4=True)
    add(200, 5, 0, "bf16", 0.0, params=False, off4=True)
    add(100, 5, 0, "f32", 0.1, params=False)
    return out


def ln_bwd_build(c):
    k = ln_bwd_dispatch(c["d"], c["N"], c["L"], c["L"] > 0, c["params"], not c["off4"])
    return (k, c["dt"], c["part"], c["L"] > 0) if k[0] == "fused" else ("rows", c["dt"], len(k) == 2)


@functools.lru_cache(maxsize=None)
def ln_bwd_operands(i):
    """dout, s, mean, rstd (f32: the float64 statistics of s, rounded), gamma, beta, fs or None, keep, old (dgamma, dbeta,
    dfs, dfh: non-zero)."""
    c = ln_bwd_cases()[i]
    N, d, L = c["N"], c["d"], c["L"]
    gen = _gen(8200, i)
    s, _, kind = ln_rows(gen, N, d, c["k0"], False)
    B = N // L if L else 0
    gamma, beta, film = ln_affine(gen, d, B)
    dout = torch.randn(N, d, generator=gen) * _pow2(gen, N)[:, None] * _pow2(gen, d)[None, :]
    sd = s.double()
    mean = sd.mean(1)
    rstd = 1.0 / torch.sqrt(sd.var(1, unbiased=False) + LN_EPS)
    old = [torch.randn(d, generator=gen), torch.randn(d, generator=gen)]
    old += [torch.randn(B, d, generator=gen), torch.randn(B, d, generator=gen)] if L else [None, None]
    return dout, s, mean.float(), rstd.float(), gamma, beta, film[0] if film else None, ln_keep(N, d, c["p"]), old, kind


def ln_bwd_ref64(dout, s, mean, rstd, gamma, beta, fs, L, p, keep, old, *, mut=None):
    """The kernels' formula in float64 on the stored s, mean, rstd: xh = (s - mean) rstd, g' = dout (1 + fs[b]),
    gx = g' gamma, dres = rstd (gx - mean_j gx - xh mean_j (gx xh)), dy = dres keep / (1 - p); dgamma = old + sum_r g' xh,
    dbeta = old + sum_r g', dfs[b] = old + sum_{r in b} dout (xh gamma + beta), dfh[b] = old + sum_{r in b} dout. Scales:
    rstd (|gx| + mean |gx| + |xh| mean |gx xh|) and the absolute sums."""
    N, d = dout.shape
    xh = (s.double() - mean.double()[:, None]) * rstd.double()[:, None]
    g0 = dout.double()
    gm, bt = gamma.double()[None, :], beta.double()[None, :]
    bi = torch.arange(N) // L if fs is not None else None
    g = g0 * (1.0 + fs.double()[bi]) if fs is not None else g0
    gx = g * gm
    s1 = gx.mean(1, keepdim=True)
    s2 = (gx * xh).mean(1, keepdim=True)
    rs = rstd.double()[:, None]
    dres = rs * (gx - (0.0 if mut == "no_s1" else s1) - xh * (s2.roll(-1, 0) if mut == "s2_next" else s2))
    u_dres = rs * (gx.abs() + gx.abs().mean(1, keepdim=True) + xh.abs() * (gx * xh).abs().mean(1, keepdim=True))
    ds = ln_drop_scale(p)
    r = Ref(dres=dres, u_dres=u_dres, b_dres=NORM_C["dres"] * U24 * u_dres)
    r.dy = dres * keep.double() * ds
    b_dy = (r.b_dres * ds + 3.0 * U24 * r.dy.abs()) * keep.double()
    r.b_dy = {"f32": b_dy, "bf16": torch.where(keep, bf16_round_bound(r.dy, b_dy), torch.zeros_like(b_dy))}
    rows = torch.ones(N, 1, dtype=torch.float64)
    if mut == "ragged":
        rows[(N // LN_SLAB) * LN_SLAB:] = 0.0
    elif mut == "fold15":                               # the fold's sixteenth group: slabs 15, 31, ... (of the batch)
        slab = torch.arange(N) // LN_SLAB
        rows[(slab % 16) == 15] = 0.0
    o = [torch.zeros_like(t) if mut == "no_old" else t.double() for t in old if t is not None]
    gg = g0 if mut == "dgamma_nofs" else g
    r.dgamma, r.u_dgamma = o[0] + (gg * xh * rows).sum(0), o[0].abs() + (g * xh).abs().sum(0)
    db = (g * rows).sum(0)
    r.dbeta, r.u_dbeta = o[1] + (db.roll(-1) if mut == "dbeta_next" else db), o[1].abs() + g.abs().sum(0)
    if fs is not None:
        B = fs.shape[0]
        if mut == "fold15":
            rows = torch.ones(N, 1, dtype=torch.float64)
            rows[((torch.arange(N) % L) // LN_SLAB) % 16 == 15] = 0.0
        lin = xh * gm + (0.0 if mut == "dfs_nobeta" else bt)
        r.dfs = o[2] + (g0 * lin * rows).view(B, L, d).sum(1)
        r.u_dfs = o[2].abs() + (g0.abs() * ((xh * gm).abs() + bt.abs())).view(B, L, d).sum(1)
        r.dfh = o[3] + (g0 * rows).view(B, L, d).sum(1)
        r.u_dfh = o[3].abs() + g0.abs().view(B, L, d).sum(1)
    for n in ("dgamma", "dbeta", "dfs", "dfh"):
        if hasattr(r, n):
            setattr(r, "b_" + n, NORM_C["par"] * U24 * getattr(r, "u_" + n))
    return r


def _slab_sums32(t, L):
    """ln_bwd_fused_kernel's per-slab column sums of t [N, d] fp32: wave w adds rows w, w + 8, w + 16, w + 24 in order,
    waves w and w + 4 are added, then the four in order. [nslab, d]."""
    N, d = t.shape
    ns = (N + LN_SLAB - 1) // LN_SLAB
    p = torch.zeros(ns * LN_SLAB, d)
    p[:N] = t
    w = _seq(p.view(ns, 4, 8, d).permute(0, 2, 3, 1))                   # [ns, 8, d]
    w = w[:, :4] + w[:, 4:]
    return _seq(w.permute(0, 2, 1))


def _fold32(part, old):
    """ln_fold_kernel: group g adds slabs g, g + 16, ... in order, the 16 groups are added in order, then onto old."""
    ns, d = part.shape
    p = torch.zeros(((ns + 15) // 16) * 16, d)
    p[:ns] = part
    return old + _seq(_seq(p.view(-1, 16, d).permute(1, 2, 0)).permute(1, 0))


def ln_bwd_emulate(dout, s, mean, rstd, gamma, beta, fs, L, kernel, old, part):
    """The backward in fp32: dres, and the four parameter sums added to old. kernel: ln_bwd_dispatch's answer. Fused: slab
    sums, then the fold (part) or one atomic per slab in slab order; two-pass: 64-row chunks (cut at FiLM batches for
    the FiLM sums), one atomic each, in order."""
    N, d = dout.shape
    x = (s - mean[:, None]) * rstd[:, None]
    g0 = dout
    bi = torch.arange(N) // L if fs is not None else None
    g = g0 * (1.0 + fs[bi]) if fs is not None else g0
    gx = g * gamma[None, :]
    vec = kernel[0] == "fused"
    fd = torch.tensor(float(d), dtype=torch.float32)
    s1 = (ln_rowsum32(gx, vec) / fd)[:, None]
    s2 = (ln_rowsum32(gx * x, vec) / fd)[:, None]
    dres = rstd[:, None] * (gx - s1 - x * s2)
    terms = [g * x, g] + ([g0 * (x * gamma[None, :] + beta[None, :]), g0] if fs is not None else [])
    outs = []
    for q, t in enumerate(terms):
        groups = [(0, N)] if q < 2 else [(b * L, (b + 1) * L) for b in range(N // L)]
        res = []
        for lo, hi in groups:
            o = old[q] if q < 2 else old[q][lo // L]
            if vec:
                ps = _slab_sums32(t[lo:hi], L)
                o = _fold32(ps, o) if part else _seq(torch.cat([o[None], ps]).permute(1, 0))
            else:
                cuts = sorted(set(range(lo, hi, 1)) & (set(range(0, N, LN_PROWS)) | {lo}))
                for a in cuts:
                    e = min(hi, (a // LN_PROWS + 1) * LN_PROWS)
                    o = o + _seq(t[a:e].permute(1, 0))
            res.append(o)
        outs.append(res[0] if q < 2 else torch.stack(res))
    return dres, outs


# ---- L_fd
LFD_BC = ((1, 257), (2, 1000), (3, 1), (32, 257), (33, 1000), (3, 257))
LFD_D = ((1, False), (33, False), (256, False), (1030, False), (256, True))          # (D, a view 4 bytes into its buffer)
LFD_LAM = (0.0, 5e-3)
LFD_W = 0.375                  # lfd_std_bwd_apply's scale (1 / world size times the loss weight: any value)
LFD_RANKS = 3                  # the data-parallel kernels see one rank's rows of a batch LFD_RANKS times as large


@functools.lru_cache(maxsize=None)
def lfd_operands(B, C):
    """z, dz~ [B, C] f32, z~ [B, C] (f32; the bf16 case rounds it), inv_std [C], and for the data-parallel kernels the
    global sums s1, s2 [C] and backward sums [2 C] of a batch of LFD_RANKS B rows. Columns: a power of two per row and
    per column; column c of kind c % 5: 1 = an offset of 2^6 spreads, 2 = constant."""
    gen = _gen(8300, B, C)
    sc = _pow2(gen, B)[:, None] * _pow2(gen, C)[None, :]
    z = torch.randn(B, C, generator=gen) * sc
    kind = torch.arange(C) % 5
    z[:, kind == 1] += 64.0 * _pow2(gen, C)[None, kind == 1] * 4.0
    z[:, kind == 2] = (1.5 * _pow2(gen, C))[None, kind == 2].expand(B, -1)
    dzt = torch.randn(B, C, generator=gen) * sc
    zt = torch.randn(B, C, generator=gen)
    zt[:, kind == 2] = 0.0
    inv = 1.0 / (torch.rand(C, generator=gen) * 4.0 + 0.01)
    n = LFD_RANKS * B
    rest = torch.randn(n - B, C, generator=gen) * _pow2(gen, C)[None, :] + z.mean(0, keepdim=True)
    allz = torch.cat([z, rest]).double()
    s1 = allz.sum(0).float()
    s2 = ((allz - allz.mean(0, keepdim=True)) ** 2).sum(0).float()
    sums = torch.cat([dzt.double().sum(0) * LFD_RANKS, (dzt.double() * zt.double()).sum(0) * LFD_RANKS]).float()
    return z, dzt, zt, inv, s1, s2, sums


def lfd_std_ref64(z, eps=LN_EPS, *, s1=None, s2=None, inv_n=None, mut=None):
    """z~ = (z - m) is, is = (var + eps)^-1/2 over the batch (lfd_std_fwd), or from the stored global sums m = s1 inv_n,
    var = s2 inv_n (lfd_std_apply). Scales: is (relative); is (|z - m| + mean_b |z|), with |m| for the mean of |z| in the
    apply form (m is read, not summed)."""
    zd = z.double()
    B = z.shape[0]
    if s1 is None:
        m = zd.mean(0, keepdim=True)
        var = ((zd - m) ** 2).sum(0, keepdim=True) / (max(B - 1, 1) if mut == "unbiased" else B)
        ma = zd.abs().mean(0, keepdim=True)
    else:
        n = float(np.float32(1.0 / B if mut == "localB" else inv_n))
        m, var = s1.double()[None, :] * n, s2.double()[None, :] * n
        ma = m.abs()
    is_ = 1.0 / torch.sqrt(var + eps)
    zt = (zd - m) * is_
    u_zt = is_ * ((zd - m).abs() + ma)
    r = Ref(inv=is_[0], b_inv=NORM_C["lfd_is"] * U24 * is_[0], zt=zt, u_zt=u_zt, b_zt=NORM_C["lfd_zt"] * U24 * u_zt)
    r.b_zt_bf = bf16_round_bound(zt, r.b_zt)
    return r


def lfd_colstat_ref64(z, s1=None, inv_n=None):
    """pass 1: sum_b z, scale sum |z|; pass 2: sum_b t^2, t = z - s1 inv_n on the stored s1, scale sum |t| (|t| + |m|)."""
    zd = z.double()
    if s1 is None:
        return Ref(out=zd.sum(0), u=zd.abs().sum(0), b=NORM_C["lfd_col"] * U24 * zd.abs().sum(0))
    m = s1.double()[None, :] * float(np.float32(inv_n))
    t = zd - m
    u = (t.abs() * (t.abs() + m.abs())).sum(0)
    return Ref(out=(t * t).sum(0), u=u, b=NORM_C["lfd_col"] * U24 * u)


def lfd_bwd_ref64(dzt, zt, inv, *, sums=None, inv_n=None, scale=1.0, mut=None):
    """dz = W is (g - m1 - z~ m2) on the stored z~ and inv_std: m1, m2 the batch means of g and g z~ (lfd_std_bwd, W = 1)
    or sums inv_n (lfd_std_bwd_apply). Also the column sums of lfd_bwd_colstat. Scales: the absolute evaluation."""
    g, z = dzt.double(), zt.double()
    B, C = g.shape
    if sums is None:
        m1, m2 = g.mean(0, keepdim=True), (g * z).mean(0, keepdim=True)
        a1, a2 = g.abs().mean(0, keepdim=True), (g * z).abs().mean(0, keepdim=True)
    else:
        n = float(np.float32(1.0 / B if mut == "localB" else inv_n))
        m1, m2 = sums.double()[None, :C] * n, sums.double()[None, C:] * n
        a1, a2 = m1.abs(), m2.abs()
    W = 1.0 if mut == "noW" else float(np.float32(scale))
    is_ = inv.double()[None, :]
    dz = W * is_ * (g - m1 - z * (0.0 if mut == "no_m2" else m2))
    u = abs(W) * is_ * (g.abs() + a1 + z.abs() * a2)
    cs = torch.cat([g.sum(0), (g * z).sum(0)])
    u_cs = torch.cat([g.abs().sum(0), (g * z).abs().sum(0)])
    return Ref(dz=dz, u_dz=u, b_dz=NORM_C["lfd_dz"] * U24 * u, cs=cs, u_cs=u_cs, b_cs=NORM_C["lfd_col"] * U24 * u_cs)


def lfd_emulate(z, dzt, zt, inv, s1, s2, sums, inv_n, scale, eps=LN_EPS):
    """lfd.hip's column loops in fp32: a dict of every kernel's outputs."""
    B = z.shape[0]
    fB = torch.tensor(float(B), dtype=torch.float32)
    n = torch.tensor(inv_n, dtype=torch.float32)
    e = torch.tensor(eps, dtype=torch.float32)
    col = lambda t: _seq(t.permute(1, 0))
    m = col(z) / fB
    var = col((z - m) ** 2) / fB
    is_ = 1.0 / torch.sqrt(var + e)
    o = dict(inv=is_, zt=(z - m) * is_, c1=col(z))
    ma = s1 * n
    o["c2"] = col((z - ma) ** 2)
    o["inv_a"] = 1.0 / torch.sqrt(s2 * n + e)
    o["zt_a"] = (z - ma) * o["inv_a"]
    g1, g2 = col(dzt), col(dzt * zt)
    o["cs"] = torch.cat([g1, g2])
    o["dz"] = (dzt - g1 / fB - zt * (g2 / fB)) * inv
    C = z.shape[1]
    o["dz_a"] = (dzt - sums[:C] * n - zt * (sums[C:] * n)) * (inv * torch.tensor(scale, dtype=torch.float32))
    return o


@functools.lru_cache(maxsize=None)
def lfd_cm(D):
    """Cm [D, D] f32: off-diagonals randn times 2^-8 .. 2^2 per element, the diagonal 0.7 + 0.1 randn with every third
    entry exactly 1."""
    gen = _gen(8400, D)
    Cm = torch.randn(D, D, generator=gen) * torch.pow(2.0, torch.randint(-8, 3, (D, D), generator=gen).float())
    dg = 0.7 + 0.1 * torch.randn(D, generator=gen)
    dg[0::3] = 1.0
    Cm.diagonal().copy_(dg)
    return Cm


def lfd_loss_ref64(Cm, lam, *, mut=None, aligned=True):
    """loss = lam sum_all C^2 + sum_j ((1 - c_jj)^2 - lam c_jj^2) on the fp32 lam; scale lam sum C^2 + sum_j |(1 - c)^2 -
    lam c^2|."""
    l = float(np.float32(lam))
    Cd = Cm.double()
    c = Cd.diagonal()
    sq = (Cd * Cd).sum()
    if mut == "tail" and aligned:
        n = Cd.numel()
        sq = (Cd.reshape(-1)[:(n >> 2) << 2] ** 2).sum()
    dterm = (1.0 - c) ** 2 - (0.0 if mut == "diag_lam" else l * c * c)
    u = l * (Cd * Cd).sum() + dterm.abs().sum()
    return Ref(loss=l * sq + dterm.sum(), u=u, b=NORM_C["lfd_loss"] * U24 * u)


def lfd_dloss_ref64(Cm, g, lam, *, mut=None):
    """dC = g (-2 (1 - c)) on the diagonal, g 2 lam c off it, within 3 u |dC| (1 - c, the product with c or with g, the
    other product), then the bf16 rounding."""
    l = float(np.float32(lam))
    D = Cm.shape[0]
    Cd = Cm.double()
    e = torch.arange(D * D)
    Dm = (D & ~1) if mut == "jk" and D > 1 else D
    j = e // Dm
    diag = ((e - j * Dm) == j).view(D, D)
    dC = float(g) * torch.where(diag, -2.0 * (1.0 - Cd), 2.0 * l * Cd)
    b = 3.0 * U24 * dC.abs()
    return Ref(dC=dC, b=b, b_bf=bf16_round_bound(dC, b))


def lfd_loss_emulate(Cm, lam, aligned=True):
    """lfd_loss_kernel in fp32: thread t's float4s t, t + 1024, ... into two accumulators, the scalar tail, its diagonal
    terms, lam sq + dg; the 16 waves' trees, then the waves in order."""
    D = Cm.shape[0]
    n = D * D
    flat = Cm.reshape(-1)
    l = torch.tensor(lam, dtype=torch.float32)
    sq = torch.zeros(1024)
    i0 = 0
    if aligned:
        n4 = n >> 2
        K = (n4 + 1023) // 1024
        p = torch.zeros(K * 1024, 4)
        p[:n4] = flat[:n4 * 4].view(n4, 4)
        p = p.view(K, 1024, 4)
        a0 = _seq((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]).permute(1, 0))
        a1 = _seq((p[..., 2] * p[..., 2] + p[..., 3] * p[..., 3]).permute(1, 0))
        sq = a0 + a1
        i0 = n4 << 2
    tail = flat[i0:]
    K = (tail.numel() + 1023) // 1024
    if K:
        p = torch.zeros(K * 1024)
        p[:tail.numel()] = tail
        for k in range(K):
            sq = sq + p[k * 1024:(k + 1) * 1024] ** 2
    c = Cm.diagonal()
    K = (D + 1023) // 1024
    p = torch.zeros(K * 1024)
    p[:D] = (1.0 - c) * (1.0 - c) - l * c * c
    dg = _seq(p.view(K, 1024).permute(1, 0))
    return _seq(_tree64((l * sq + dg).view(16, 64)))


# ------------------------------------------------ the autograd Functions (fddm_hip/functions.py)
# Float64 restatements of what each torch.autograd.Function claims to be, as plain differentiable torch graphs, shared by
# tests/test_cpu_functions_ref.py (references against the oracle, mutants against the bounds, balance of the loss
# coefficients) and tests/test_gpu_functions.py (the Functions on the device). Every operand sits on the bf16 grid, so
# the fp32 and the bf16 mode read the values the reference reads. Gradients are float64 autograd of the composite loss.
# Each gradient comes with a magnitude companion: the same linear maps on absolute operands (as gemm_bound's s). The
# bound per element is |got - ref| <= C u companion, u = 2^-24 (fp32 mode) or 2^-9 (bf16 mode), C = min(64, 8 E), E the
# worst ratio |got - ref| / (u companion) measured on the MI355X over every case of the tables below, one per (Function,
# output, precision), stored with measured <= stored <= 1.1 measured + FN_E_FLOOR. The wiring errors in question (a share
# of the logits gradient lost, a scale ignored, overwrite for accumulate) are of the companion's own size: the CPU file
# proves that they leave the bound at C = 64.
# EmbedFn and CondFn compute in fp32 in both modes (csrc/small.hip, the f32 embedding): their u is 2^-24 in both.
U9 = 2.0 ** -9
FN_U = {"fp32": U24, "bf16": U9}
FN_E_FLOOR = 0.05
FN_E = {
    # (function, gradient, precision): E, measured on an MI355X (tests/test_gpu_functions.py prints them as FNE lines);
    # the worst case of each stands behind it.
    # head: the HeadFn / KLFn / TextEmbedFn hand-over matrix; hw, hb = the head's weight and bias, x = its input, tw = the
    # text weight, dl = the logits gradient (observable in fp32 mode only). The fp32 figures are what the logits' own
    # rounding (u times ~10 |logit|-sized terms) costs through the softmax: the fp32 evaluation on the CPU shows 8 .. 21
    ("head", "hw", "fp32"): 20.3,     # 18.46  kl_g V=301 no mask
    ("head", "hb", "fp32"): 11.8,     # 10.76  kl_slice V=301 no mask
    ("head", "x", "fp32"): 18.6,      # 16.92  kl_g V=301 masked
    ("head", "tw", "fp32"): 25.9,     # 23.55  text V=301 no mask
    ("head", "dl", "fp32"): 36.6,     # 33.26  text V=304 no mask
    ("head", "hw", "bf16"): 5.15,     # 4.66   kl_g_text V=304 no mask
    ("head", "hb", "bf16"): 3.78,     # 3.41   kl_g_text V=304 masked
    ("head", "x", "bf16"): 2.75,      # 2.47   kl_g_text V=304 no mask
    ("head", "tw", "bf16"): 1.7,      # 1.52   text V=300 no mask
    ("linear", "x", "fp32"): 3.08,    # 2.77   out 100, weight frozen, arena
    ("linear", "w", "fp32"): 1.7,     # 1.51   out 256, x detached, weight in the arena
    ("linear", "b", "fp32"): 0.11,    # 0.056  out 256, weight frozen, arena
    # bf16 mode: operands and cotangents on the bf16 grid, fp32 accumulation: nothing is rounded at 2^-9 (< 0.0005)
    ("linear", "x", "bf16"): 0.05, ("linear", "w", "bf16"): 0.05, ("linear", "b", "bf16"): 0.05,
    ("lfd", "za", "fp32"): 14.6,      # 13.26  g = 1
    ("lfd", "zb", "fp32"): 10.15,     # 9.22   g = 0.37
    ("lfd", "za", "bf16"): 5.15,      # 4.66   g = 0.37
    ("lfd", "zb", "bf16"): 4.8,       # 4.35   g = 0.37
    # EmbedFn / CondFn: fp32 arithmetic in both modes, the same figures in both
    ("cond", "time", "fp32"): 6.6,    # 5.98   NL 2, d 200, mlp.2.weight
    ("cond", "film", "fp32"): 1.55,   # 1.38   NL 2, d 200, scale_proj.weight of block 0
    ("cond", "emb", "fp32"): 0.05,    # 0: at most three bf16-grid rows meet in one embedding row, their fp32 sum is exact
    ("cond", "time", "bf16"): 6.6, ("cond", "film", "bf16"): 1.55, ("cond", "emb", "bf16"): 0.05,
}


def fn_c(fn, out, prec):
    return min(64.0, 8.0 * FN_E[(fn, out, prec)])


def _grid(x):
    """x rounded onto the bf16 grid, as float32."""
    return x.to(torch.bfloat16).float()


def fn_excess(got, ref, comp, u):
    """max |got - ref| / (u companion) (elements whose companion is 0 must agree exactly: inf otherwise)."""
    err = (got.detach().double().cpu() - ref).abs()
    assert err.shape == comp.shape, (err.shape, comp.shape)
    pos = comp > 0
    if (err[~pos] != 0).any():
        return float("inf")
    return (err[pos] / (u * comp[pos])).max().item() if pos.any() else 0.0


# ---- HeadFn / KLFn / TextEmbedFn: the logits gradient's way from its consumers to the head
HEAD_B, HEAD_L, HEAD_D, HEAD_T, HEAD_TW = 3, 20, 128, 10, 64     # 60 rows: no multiple of 8, 32 or 64
HEAD_V = (304, 300, 301)       # V % 8 == 0 (the combined bf16 buffer) | V % 4 == 0 only (one-pass KL, f32 text part) |
#                                the two-pass KL and the zero-padded GEMMs
HEAD_G = 0.375                 # the KL's weight where it is not 1 (a GradScaler, a weighted KL)
# loss coefficients of the text, dense and expanded consumers, balanced so that every consumer's share of the logits
# gradient's companion has its median within 4x of the KL's (tests/test_cpu_functions_ref.py asserts it)
HEAD_CT, HEAD_CD, HEAD_CE = 2.0 ** -13, 2.0 ** -15, 2.0 ** -15
# name -> the consumers of the logits in the order the graph is built (autograd runs their backwards in the reverse):
# (kind, coefficient). kl: KLFn on the whole logits; klslice: KLFn on logits[:1]; text: (TextEmbedFn(logits) * Rz).sum();
# dense: (logits * R).sum(); expand: logits.sum(), whose gradient arrives as an expanded (zero-stride) scalar
HEAD_CASES = {
    "kl": (("kl", 1.0),),
    "kl_g": (("kl", HEAD_G),),
    "kl_text": (("kl", 1.0), ("text", HEAD_CT)),
    "kl_g_text": (("kl", HEAD_G), ("text", HEAD_CT)),
    "text_kl": (("text", HEAD_CT), ("kl", 1.0)),
    "text": (("text", HEAD_CT),),
    "kl_dense": (("kl", 1.0), ("dense", HEAD_CD)),
    "kl_expand": (("kl", 1.0), ("expand", HEAD_CE)),
    "kl_kl": (("kl", 1.0), ("kl", HEAD_G)),
    "kl_slice": (("klslice", 1.0),),
}
HEAD_ALL = (("kl", HEAD_G), ("text", HEAD_CT), ("dense", HEAD_CD), ("expand", HEAD_CE))   # the mutants' composite
HEAD_MUTANTS = ("no_expand", "no_dense", "kl_unscaled", "kl_twice", "no_text")


@functools.lru_cache(maxsize=None)
def head_inputs(V, masked):
    """Operands of the hand-over matrix on the bf16 grid (f32 tensors): x [N, d] the head's input (randn times a power
    of two per row), hw [V, d] and hb [V] (logits of spread ~1.5), tw [64, V] the text weight with one sign per column
    (so that the text share of a logits column keeps its sign over the rows and shows in the bias gradient), Rz
    [N, 64] > 0 and R [N, V] > 0 the cotangents of the text and the dense consumer; xt, x0 [B, L] (every third token
    x0 == xt), t = (1, T, 5), x_mask [B, L] with the tail of row 1 padded (or None), the scheduler's betas."""
    from oracle import fddm_oracle as O
    B, L, d, Tn, TW = HEAD_B, HEAD_L, HEAD_D, HEAD_T, HEAD_TW
    gen = _gen(9100, V)
    N = B * L
    x = _grid(torch.randn(N, d, generator=gen) * _pow2(gen, N, -1, 1)[:, None])
    hw = _grid(0.11 * torch.randn(V, d, generator=gen))
    hb = _grid(0.5 * torch.randn(V, generator=gen))
    sign = torch.where(torch.rand(V, generator=gen) < 0.5, -1.0, 1.0)
    tw = _grid((0.25 + torch.randn(TW, V, generator=gen).abs()) * sign[None, :] * _pow2(gen, TW, -1, 1)[:, None])
    Rz = _grid(0.25 + torch.randn(N, TW, generator=gen).abs())
    R = _grid(0.25 + torch.randn(N, V, generator=gen).abs())
    x0 = torch.randint(0, V, (B, L), generator=gen)
    xt = torch.randint(0, V, (B, L), generator=gen)
    xt.view(-1)[::3] = x0.view(-1)[::3]
    t = torch.tensor([1, Tn, 5])
    mask = None
    if masked:
        mask = torch.ones(B, L, dtype=torch.bool)
        mask[1, 14:] = False
    betas, _ = O.sched_tables(Tn)
    return Ref(x=x, hw=hw, hb=hb, tw=tw, Rz=Rz, R=R, xt=xt, x0=x0, t=t, mask=mask, betas=betas.float())


def head_ref64(V, masked, consumers, dtype=torch.float64, mut=None):
    """The composite loss sum_i c_i consumer_i(logits), logits = x hw^T + hb, as a plain torch graph in `dtype`, and its
    autograd gradients: g = {x, hw, hb, tw (None without a text consumer), dl = d loss / d logits}, all float64.
    Companions m (same keys): m_dl = the sum of the consumers' shares, KL: |c| s (kl_term_ref64's scale), text:
    |c| xhat (a + sum_j xhat_j a_j) with a = |Rz| |tw|, dense |c R|, expand |c|; hw: m_dl^T |x|; hb: the column sums of
    m_dl; x: m_dl |hw|; tw: |c Rz|^T xhat. shares = {kind: its part of m_dl}, terms = {kind: c_i consumer_i}.
    mut (tests/test_cpu_functions_ref.py): no_expand / no_dense / no_text drop that consumer, kl_unscaled takes every
    KL with weight 1, kl_twice with weight 1 + c (the unscaled share left in the buffer and the scaled one added)."""
    i = head_inputs(V, masked)
    B, L = HEAD_B, HEAD_L
    x, hw, hb, tw = (v.clone().to(dtype).requires_grad_(True) for v in (i.x, i.hw, i.hb, i.tw))
    logits = x @ hw.t() + hb
    logits.retain_grad()
    lg = logits.view(B, L, V)
    loss = torch.zeros((), dtype=dtype)
    m_dl = torch.zeros(B * L, V, dtype=torch.float64)
    m_tw = None
    shares, terms = {}, {}
    for kind, c in consumers:
        if mut == "no_" + kind:
            continue
        if kind in ("kl", "klslice"):
            r = B if kind == "kl" else 1
            cm = 1.0 if mut == "kl_unscaled" else (1.0 + c) if mut == "kl_twice" else c
            kl_tok, _, w, s = kl_term_ref64(lg[:r], i.xt[:r], i.x0[:r], i.t[:r], None if i.mask is None else i.mask[:r],
                                            i.betas, dtype=dtype)
            term = cm * (w.detach() * kl_tok).sum()
            sh = torch.zeros(B, L, V, dtype=torch.float64)
            sh[:r] = abs(c) * s.detach().double()
            sh = sh.view(B * L, V)
        elif kind == "text":
            xhat = torch.softmax(logits, -1)
            term = c * ((xhat @ tw.t()) * i.Rz.to(dtype)).sum()
            xh = xhat.detach().double()
            a = (abs(c) * i.Rz.double()) @ i.tw.double().abs()
            sh = xh * (a + (xh * a).sum(-1, keepdim=True))
            mt = (abs(c) * i.Rz.double()).t() @ xh
            m_tw = mt if m_tw is None else m_tw + mt
        elif kind == "dense":
            term = c * (logits * i.R.to(dtype)).sum()
            sh = abs(c) * i.R.double()
        elif kind == "expand":
            term = c * logits.sum()
            sh = torch.full((B * L, V), abs(c), dtype=torch.float64)
        else:
            raise ValueError(kind)
        loss = loss + term
        m_dl = m_dl + sh
        shares[kind] = shares.get(kind, 0) + sh
        terms[kind] = terms.get(kind, 0.0) + float(term.detach())
    loss.backward()
    g = {"x": x.grad, "hw": hw.grad, "hb": hb.grad, "tw": tw.grad if m_tw is not None else None, "dl": logits.grad}
    g = {k: (None if v is None else v.detach().double()) for k, v in g.items()}
    m = {"dl": m_dl, "hw": m_dl.t() @ i.x.double().abs(), "hb": m_dl.sum(0), "x": m_dl @ i.hw.double().abs(), "tw": m_tw}
    return Ref(loss=float(loss.detach()), g=g, m=m, shares=shares, terms=terms)


@functools.lru_cache(maxsize=None)
def head_case_ref(name, V, masked):
    return head_ref64(V, masked, HEAD_CASES[name])


# ---- LinearFn
# (rows shape, in, out): 45 rows as [3, 15, 128] -> 256 | out = 100 (100 % 8 = 4: the zero-padded GEMMs)
LINEAR_SHAPES = (((3, 15), 128, 256), ((3, 15), 128, 100))
LINEAR_NEEDS = ("all", "x_detached", "w_frozen")      # w_frozen: the bias alone trains (the colsum branch)
LINEAR_DEST = ("fresh", "arena", "w_arena")           # w_arena: the weight in a GradArena, the bias fresh (ab != aw)


def linear_fn_cases():
    """(shape index, bias, needs, dest) of every LinearFn case that is not another one in disguise: no frozen weight
    without a bias (nothing trains), no w_arena without a trainable weight and a bias."""
    out = []
    for si in range(len(LINEAR_SHAPES)):
        for bias in (False, True):
            for needs in LINEAR_NEEDS:
                for dest in LINEAR_DEST:
                    if needs == "w_frozen" and (not bias or dest == "w_arena"):
                        continue
                    if dest == "w_arena" and not bias:
                        continue
                    out.append((si, bias, needs, dest))
    return out


@functools.lru_cache(maxsize=None)
def linear_fn_inputs(si):
    """x [3, 15, in], w [out, in], b [out] and the cotangents Ry of the two passes [2, 3, 15, out], on the bf16 grid."""
    lead, K, N = LINEAR_SHAPES[si]
    gen = _gen(9200, si)
    M = lead[0] * lead[1]
    x = _grid(torch.randn(M, K, generator=gen) * _pow2(gen, M)[:, None]).view(*lead, K)
    w = _grid(torch.randn(N, K, generator=gen) * _pow2(gen, N)[:, None] * 0.1)
    b = _grid(torch.randn(N, generator=gen))
    Ry = _grid(torch.randn(2, M, N, generator=gen) * _pow2(gen, N)[None, None, :]).view(2, *lead, N)
    return Ref(x=x, w=w, b=b, Ry=Ry)


@functools.lru_cache(maxsize=None)
def linear_fn_ref64(si, bias, dtype=torch.float64, mut=None):
    """y = x w^T + b and the gradients of two forward / backward passes, loss_p = (y Ry_p).sum(), summed as .grad or a
    grad-arena slot sums them: g = {x, w, b}, companions m = sum_p (|Ry_p| |w|, |Ry_p|^T |x|, the column sums of
    |Ry_p|). y is returned too. mut = "b_overwrite": the second pass overwrites the bias gradient."""
    i = linear_fn_inputs(si)
    x, w, b = (v.clone().to(dtype).requires_grad_(True) for v in (i.x, i.w, i.b))
    y = x @ w.t() + (b if bias else 0.0)
    ((y * i.Ry[0].to(dtype)).sum() + (y * i.Ry[1].to(dtype)).sum()).backward()
    g = {"x": x.grad.double(), "w": w.grad.double(), "b": b.grad.double() if bias else None}
    if mut == "b_overwrite" and bias:
        g["b"] = i.Ry[1].double().reshape(-1, w.shape[0]).sum(0)
    Ra = (i.Ry[0].double().abs() + i.Ry[1].double().abs()).reshape(-1, w.shape[0])
    xa = i.x.double().abs().reshape(-1, w.shape[1])
    m = {"x": (Ra @ i.w.double().abs()).view(i.x.shape), "w": Ra.t() @ xa, "b": Ra.sum(0)}
    return Ref(y=y.detach().double(), g=g, m=m)


# ---- LfdFn
LFD_FN = (4, 6, 64)            # B, T, D
LFD_FN_G = (1.0, 0.37)         # the upstream scalar
LFD_FN_LAM = 5e-3


@functools.lru_cache(maxsize=None)
def lfd_fn_inputs():
    """z_a, z_b [B, T, D] on the bf16 grid. Each (t, d) column is standardised over the batch exactly and given a scale
    0.75 .. 1.25 times a power of two and an offset, so that every column's batch standard deviation is within 0.25 of
    the median column's (at B = 4 a raw randn column can be 100 times flatter: the standardisation would amplify its
    rounding by that factor); z_b = 0.6 z_a's standardised column + 0.8 another, so the correlation's diagonal is ~0.6."""
    B, Tn, D = LFD_FN
    gen = _gen(9300, B, Tn, D)

    def std(v):
        v = v - v.mean(0, keepdim=True)
        return v / v.pow(2).mean(0, keepdim=True).sqrt()

    a = std(torch.randn(B, Tn, D, generator=gen, dtype=torch.float64))
    n = std(torch.randn(B, Tn, D, generator=gen, dtype=torch.float64))
    b = std(0.6 * a + 0.8 * n)
    out = []
    for v in (a, b):
        sc = (0.75 + 0.5 * torch.rand(Tn, D, generator=gen, dtype=torch.float64))
        off = torch.randn(Tn, D, generator=gen, dtype=torch.float64)
        out.append(_grid((v * sc + off).float()))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def lfd_fn_ref64(g, dtype=torch.float64, mut=None):
    """g * oracle.lfd_loss(z_a, z_b) in `dtype` and its autograd gradients {za, zb} (float64). No magnitude can be
    carried through the batch standardisation (its backward subtracts two batch means): the companion of an element is
    max |ref| over its column d (all b, t), m = {za, zb} [1, 1, D]. mut = "nt_once": 1 / (B T) applied once instead of
    twice (the backward GEMMs' alpha left out): the gradients times B T."""
    from oracle import fddm_oracle as O
    B, Tn, D = LFD_FN
    za, zb = (v.clone().to(dtype).requires_grad_(True) for v in lfd_fn_inputs())
    loss = O.lfd_loss(za, zb, LFD_FN_LAM, LN_EPS)
    (g * loss).backward()
    k = float(B * Tn) if mut == "nt_once" else 1.0
    gr = {"za": k * za.grad.double(), "zb": k * zb.grad.double()}
    ref = gr if mut is None and dtype == torch.float64 else lfd_fn_ref64(g).g
    m = {n: v.abs().amax((0, 1), keepdim=True).expand_as(v).contiguous() for n, v in ref.items()}
    return Ref(loss=float(loss.detach()), g=gr, m=m)


# ---- EmbedFn + CondFn: t_bias = time_proj(mlp(sinusoid(t))), FiLM projections of the pooled condition, x = E[xt] + t_bias
COND_FN_B, COND_FN_L, COND_FN_V = 3, 7, 11
COND_FN_NL = (0, 2)
COND_FN_D = (128, 200)
COND_FN_MODES = ("gbuf", "foreign", "film_only")   # FiLM gradients as gbuf slices | foreign tensors, one None (the
#                                                    stacked branch) | no gradient for t_bias (dtb = None)


@functools.lru_cache(maxsize=None)
def cond_fn_inputs(NL, d):
    """The conditioning path's operands on the bf16 grid: t = (1, 10, 3), pooled [B, d], the six time-path parameters,
    2 NL FiLM (weight, bias) pairs, E [V, d] with the pad row 0 zero, xt [B, L] with pad tokens, cotangents Rx [B L, d] of
    the embedding output and Rf [2 NL, B, d] of the FiLM outputs."""
    B, L, V = COND_FN_B, COND_FN_L, COND_FN_V
    gen = _gen(9400, NL, d)
    rn = lambda *s, k=1.0: _grid(k * torch.randn(*s, generator=gen))     # noqa: E731
    p = [rn(4 * d, d, k=0.1), rn(4 * d, k=0.5), rn(d, 4 * d, k=0.05), rn(d, k=0.5), rn(d, d, k=0.1), rn(d, k=0.5)]
    for _ in range(2 * NL):
        p += [rn(d, d, k=0.1), rn(d, k=0.5)]
    E = rn(V, d)
    E[0] = 0.0
    xt = torch.randint(1, V, (B, L), generator=gen)
    xt[1, 4:] = 0
    xt[2, 2] = 0
    return Ref(t=torch.tensor([1, 10, 3]), pooled=rn(B, d), params=tuple(p), E=E, xt=xt, Rx=rn(B * L, d),
               Rf=rn(max(2 * NL, 1), B, d)[:2 * NL])


@functools.lru_cache(maxsize=None)
def cond_fn_ref64(NL, d, mode, dtype=torch.float64):
    """loss = (x Rx).sum() + sum_i (film_i Rf_i).sum() (mode film_only: the FiLM part alone; mode foreign: FiLM output
    1 unused), x = E[xt] + t_bias[b], t_bias = Wp (W2 silu(W1 emb + b1) + b2) + bp on the float64 time embedding
    (te_ref64), film_i = pooled Wf_i^T + bf_i. g = {E, p0 .. p(5 + 4 NL)} (None where the loss does not reach), m the
    companions: the backward with every operand and every intermediate cotangent replaced by its magnitude
    (|silu'(pre)| for the activation; the embedding's magnitude is |emb| + its argument's, te_ref64's unit)."""
    i = cond_fn_inputs(NL, d)
    B, L = COND_FN_B, COND_FN_L
    te = te_ref64(i.t, d)
    emb = te.emb.to(dtype)
    P = [v.clone().to(dtype).requires_grad_(True) for v in i.params]
    E = i.E.clone().to(dtype).requires_grad_(True)
    W1, b1, W2, b2, Wp, bp = P[:6]
    pre = emb @ W1.t() + b1
    h = torch.nn.functional.silu(pre)
    tev = h @ W2.t() + b2
    tb = tev @ Wp.t() + bp
    x = torch.nn.functional.embedding(i.xt, E, padding_idx=0) + tb[:, None]
    loss = torch.zeros((), dtype=dtype)
    time_used = mode != "film_only"
    if time_used:
        loss = loss + (x.reshape(B * L, d) * i.Rx.to(dtype)).sum()
    pooled = i.pooled.to(dtype)
    used = [not (mode == "foreign" and k == 1) for k in range(2 * NL)]
    for k in range(2 * NL):
        if used[k]:
            loss = loss + ((pooled @ P[6 + 2 * k].t() + P[7 + 2 * k]) * i.Rf[k].to(dtype)).sum()
    if loss.requires_grad:
        loss.backward()
    g = {"E": E.grad}
    for k, v in enumerate(P):
        g[f"p{k}"] = v.grad
    g = {k: (None if v is None else v.double()) for k, v in g.items()}
    m = {k: None for k in g}
    if time_used:
        Rx = i.Rx.double().abs()
        live = (i.xt.view(-1) != 0)
        m["E"] = torch.zeros(COND_FN_V, d, dtype=torch.float64).index_add_(0, i.xt.view(-1)[live], Rx[live])
        dtb = Rx.view(B, L, d).sum(1)
        a = lambda v: v.detach().double().abs()     # noqa: E731
        dte = dtb @ a(Wp)
        dh = dte @ a(W2)
        dpre = dh * dsilu64(pre.detach().double()).abs()
        m_emb = te.emb.abs() + te.unit / U24
        m_tev = a(h) @ a(W2).t() + a(b2)            # te's terms, not |te|: the roundings of its sum reach dWp
        m.update(p5=dtb.sum(0), p4=dtb.t() @ m_tev, p3=dte.sum(0), p2=dte.t() @ a(h), p1=dpre.sum(0),
                 p0=dpre.t() @ m_emb)
    for k in range(2 * NL):
        if used[k]:
            Rf = i.Rf[k].double().abs()
            m[f"p{6 + 2 * k}"] = Rf.t() @ i.pooled.double().abs()
            m[f"p{7 + 2 * k}"] = Rf.sum(0)
    return Ref(g=g, m=m, tb=tb.detach().double(), x=x.detach().double().reshape(B * L, d), used=used)
