"""Shared test helpers: PCG parameter dicts with reference names, fixture loading, comparisons."""
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
