"""WavLM-Large family: geometries, name-generated weights and inputs, and the per-element references, fp32 emulations
and bounds of its two front-end kernels (csrc/norm.hip: conv0_ln_gelu_kernel, ln_gelu_fwd_kernel). Shared by
tests/golden/make_golden_wavlm_large.py, tests/test_cpu_wavlm_large.py (which measures the constants below from the
emulation alone), tests/test_gpu_wavlm_large_kernels.py and tests/test_gpu_wavlm_large.py.

Both kernels evaluate, per row (a frame's C channels / a row of d),
    y_c    = bias_c + sum_k w_ck x_k                 conv0 only: ten fp32 FMAs in tap order starting from the bias
    mean   = (sum_c y_c) / C                         8 consecutive channels per lane in order, then a 64-lane tree
    var    = (sum_c (y_c - mean)^2) / C              the same order
    z_c    = (y_c - mean) rstd gamma_c + beta_c      rstd = 1 / sqrt(var + eps)
    out_c  = gelu(z_c)
The error scale of z_c, "the absolute-value evaluation of the same expression including the rstd factor", is
    s_c    = (ya_c + mean_a) rstd |gamma_c| + |beta_c|,    ya_c = |bias_c| + sum_k |w_ck| |x_k|  (|y_c| for ln_gelu),
             mean_a = (sum_c ya_c) / C
with rstd the float64 reference's. An error of the variance reaches z through (y - mean) rstd, which s bounds.
"""
import functools
import math

import numpy as np
import torch

from oracle.weights import pcg_array

# ------------------------------------------------------------------------------------------ geometries and weights
SWITCHES = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
SMALL_LARGE = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                   conv_dim=(32,) * 7, num_conv_pos_embedding_groups=4, **SWITCHES)
WIDE_LARGE = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096,
                  conv_dim=(512,) * 7, num_conv_pos_embedding_groups=16, **SWITCHES)
FULL_LARGE = dict(WIDE_LARGE, num_hidden_layers=24)
# tag -> (geometry, d_model, B, lengths of the masked variant or None)
GEOMS = {"small": (SMALL_LARGE, 64, 3, (16000, 9000, 500)),
         "wide": (WIDE_LARGE, 128, 2, (16000, 9000)),
         "full": (FULL_LARGE, 128, 1, None)}
CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
NSAMP = 16000


def large_wave(B):
    """[B, 16000] ~ 0.1 N(0, 1) f32 from a name alone."""
    w = 0.1 * math.sqrt(float(NSAMP)) * pcg_array("wavlm_large.wave", (B, NSAMP))
    return torch.from_numpy(w.astype(np.float32))


def large_shapes(geom, d_model):
    """name -> shape of AcousticEncoder's state_dict for a WavLM-Large-family geometry (transformers' names under
    backbone., masked_spec_embed left out, plus proj.*)."""
    E, C, H = geom["hidden_size"], geom["conv_dim"], geom["num_attention_heads"]
    I = geom["intermediate_size"]
    sh = {}
    cin = 1
    for i, (c, k) in enumerate(zip(C, CONV_KERNEL)):
        p = f"backbone.feature_extractor.conv_layers.{i}."
        sh[p + "conv.weight"] = (c, cin, k)
        sh[p + "conv.bias"] = (c,)
        sh[p + "layer_norm.weight"] = (c,)
        sh[p + "layer_norm.bias"] = (c,)
        cin = c
    sh["backbone.feature_projection.layer_norm.weight"] = (C[-1],)
    sh["backbone.feature_projection.layer_norm.bias"] = (C[-1],)
    sh["backbone.feature_projection.projection.weight"] = (E, C[-1])
    sh["backbone.feature_projection.projection.bias"] = (E,)
    kp, gp = 128, geom["num_conv_pos_embedding_groups"]
    sh["backbone.encoder.pos_conv_embed.conv.bias"] = (E,)
    sh["backbone.encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, kp)
    sh["backbone.encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (E, E // gp, kp)
    sh["backbone.encoder.layer_norm.weight"] = (E,)
    sh["backbone.encoder.layer_norm.bias"] = (E,)
    for i in range(geom["num_hidden_layers"]):
        p = f"backbone.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sh[p + f"attention.{n}.weight"] = (E, E)
            sh[p + f"attention.{n}.bias"] = (E,)
        sh[p + "attention.gru_rel_pos_const"] = (1, H, 1, 1)
        sh[p + "attention.gru_rel_pos_linear.weight"] = (8, E // H)
        sh[p + "attention.gru_rel_pos_linear.bias"] = (8,)
        if i == 0:
            sh[p + "attention.rel_attn_embed.weight"] = (320, H)
        sh[p + "layer_norm.weight"] = (E,)
        sh[p + "layer_norm.bias"] = (E,)
        sh[p + "feed_forward.intermediate_dense.weight"] = (I, E)
        sh[p + "feed_forward.intermediate_dense.bias"] = (I,)
        sh[p + "feed_forward.output_dense.weight"] = (E, I)
        sh[p + "feed_forward.output_dense.bias"] = (E,)
        sh[p + "final_layer_norm.weight"] = (E,)
        sh[p + "final_layer_norm.bias"] = (E,)
    if E != d_model:
        sh["proj.weight"] = (d_model, E)
        sh["proj.bias"] = (d_model,)
    return sh


def large_sd(geom, d_model):
    """The PCG64 weights oracle.weights.load_pcg gives a module with these names."""
    return {n: torch.from_numpy(pcg_array(n, s)) for n, s in large_shapes(geom, d_model).items()}


def hf_encoder64(geom, d_model, dtype=torch.float64):
    """(transformers WavLMModel, proj Linear) in `dtype` on the CPU with the name-generated weights: the reference."""
    from transformers import WavLMConfig, WavLMModel
    from oracle.weights import load_pcg
    m = WavLMModel(WavLMConfig(**geom))
    load_pcg(m, prefix="backbone.")
    proj = torch.nn.Linear(geom["hidden_size"], d_model)
    load_pcg(proj, prefix="proj.")
    return m.to(dtype).eval(), proj.to(dtype).eval()


def hf_forward(m, proj, wave, lengths=None):
    """What the reference AcousticEncoder(wave, lengths) with pooling="mean" returns, restated on transformers' model:
    (feats, feat_mask or None, pooled, extract_features): attention_mask = ids < lengths; feat_mask keeps
    min(ceil(len / 320), S) frames; pooled the masked mean with the count clamped to >= 1."""
    dt = next(m.parameters()).dtype
    with torch.no_grad():
        am = None
        if lengths is not None:
            am = torch.arange(wave.shape[1])[None, :] < lengths[:, None]
        out = m(wave.to(dt), attention_mask=am)
        feats = proj(out.last_hidden_state)
        if lengths is None:
            return feats, None, feats.mean(1), out.extract_features
        S = feats.shape[1]
        fl = torch.clamp((lengths + 319) // 320, max=S)
        mask = torch.arange(S)[None, :] < fl[:, None]
        pooled = (feats * mask[..., None]).sum(1) / mask.sum(1).clamp(min=1)[..., None]
        return feats, mask, pooled, out.extract_features


# ------------------------------------------------------------------------------------------ kernel references
U24 = 2.0 ** -24
LN_EPS = 1e-5
K0, S0, TAIL0 = 10, 5, 3
# Largest |z_emulated - z_float64| / (u s) over every case of the two families below, measured on the CPU by
# tests/test_cpu_wavlm_large.py::test_front_error_constants (python -m pytest tests/test_cpu_wavlm_large.py -k
# error_constants -s prints "LARGE_E measured ..."); stored <= 1.1 x measured + 0.05. The GPU bound uses 8 x these.
LARGE_E = {"conv0_ln": 5.5, "ln_gelu": 5.45}       # measured 5.214, 5.176 (the inputs are numpy PCG64 draws: the same
#                                                    figures under every torch CPU capability and thread count)
LARGE_E_FLOOR = 0.05
LARGE_C = {k: 8.0 * v for k, v in LARGE_E.items()}
GELU_ABS = 2e-6             # gelu_f against the erf GELU (helpers.GEMM_GELU_ABS)
GELU_BF16OUT_ABS = 2.6e-5   # gelu_bf16out (helpers.GEMM_GELU_BF16OUT_ABS)

CONV0_LN_C = (32, 512)
CONV0_LN_T0 = (1, 67, 4097)
CONV0_LN_KINDS = ("noise", "dc", "gap")     # unit noise; noise on a DC offset of 50; middle third exact zeros
LN_GELU_D = (32, 512)
LN_GELU_N = (1, 33, 4099)


class RowRef:
    """z [.., C] float64 with error scale s; ref = gelu(z); lin = |gelu'(z)|; y the rows that were normalised, var
    [.., 1] their variance."""
    __slots__ = ("y", "var", "z", "s", "ref", "lin")


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def row_ln64(y, ya, gamma, beta, eps=LN_EPS, *, unbiased=False, no_eps=False):
    """The float64 reference of LayerNorm + GELU over the last axis of y with the error scale above."""
    y, ya, g, b = y.double(), ya.double(), gamma.double(), beta.double()
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).sum(-1, keepdim=True) / (y.shape[-1] - (1 if unbiased else 0))
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else eps))
    r = RowRef()
    r.y, r.var = y, var
    r.z = (y - mean) * rstd * g + b
    r.s = (ya + ya.mean(-1, keepdim=True)) * rstd * g.abs() + b.abs()
    r.ref = torch.nn.functional.gelu(r.z)
    r.lin = gelu_grad64(r.z).abs()
    return r


def _f(x):
    return x.float()


def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _row_sum32(v):
    """The kernels' row sum in fp32: 8 consecutive elements per lane added in order, then a pairwise tree over the 64
    lanes (idle lanes hold zeros). v [R, d], d % 8 == 0, d <= 512."""
    R, d = v.shape
    lanes = torch.zeros(R, 64, dtype=torch.float32)
    p = v.float().reshape(R, d // 8, 8)
    acc = torch.zeros(R, d // 8, dtype=torch.float32)
    for e in range(8):
        acc = acc + p[:, :, e]
    lanes[:, : d // 8] = acc
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return lanes                                                        # [R, 1]


def row_ln_emulate(y, gamma, beta, eps=LN_EPS, *, mul_inv=False):
    """z as the kernels form it in fp32 from the fp32 rows y [R, d]. mul_inv: the mean and variance are sum * (1/d)
    (conv0_ln_gelu) instead of sum / d (ln_gelu_fwd)."""
    y = y.float()
    d = y.shape[-1]
    inv = torch.tensor(1.0 / d, dtype=torch.float32)
    dv = (lambda t: t * inv) if mul_inv else (lambda t: t / torch.tensor(float(d), dtype=torch.float32))
    mean = dv(_row_sum32(y))
    t = y - mean
    var = dv(_row_sum32(t * t))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return _fma32((y - mean) * rstd, gamma.float(), beta.float())


class _Rng:
    """Normal draws and integer exponents from numpy's PCG64: bit-identical on every machine (torch.randn's CPU kernels
    differ in the last bits between instruction sets, and the constants above are maxima of rounding errors, which a
    last-bit change of an input moves)."""

    def __init__(self, seed):
        self.g = np.random.Generator(np.random.PCG64(seed))

    def randn(self, *shape):
        return torch.from_numpy(self.g.standard_normal(shape).astype(np.float32))

    def pow2(self, lo, hi, *shape):
        """2^k, k uniform in lo .. hi inclusive."""
        return torch.from_numpy(np.ldexp(1.0, self.g.integers(lo, hi + 1, size=shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def conv0_ln_params(C, const_bias=False):
    """w [C, 10] = 0.3 randn times a power of two per channel (2^-3 .. 2^3), bias 0.2 randn (or the constant 0.3),
    gamma = 1 + 0.1 randn, beta = 0.1 randn."""
    gen = _Rng(5000 + C)
    w = 0.3 * gen.randn(C, K0) * gen.pow2(-3, 3, C, 1)
    bias = 0.2 * gen.randn(C)
    if const_bias:
        bias = torch.full((C,), 0.3)
    return w, bias, 1.0 + 0.1 * gen.randn(C), 0.1 * gen.randn(C)


@functools.lru_cache(maxsize=None)
def conv0_ln_wave(T0):
    """[3, nsamp] f32, one utterance per kind of CONV0_LN_KINDS; nsamp = (T0 - 1) 5 + 10 + 3: the last three samples
    reach no frame. The gap utterance's middle third of samples is exact zeros (digital silence)."""
    nsamp = (T0 - 1) * S0 + K0 + TAIL0
    x = _Rng(91 * T0 + 3).randn(3, nsamp)
    x[1] += 50.0
    x[2, nsamp // 3: max(2 * nsamp // 3, nsamp // 3 + K0)] = 0.0
    return x


def conv0_frames(wave):
    T0 = (wave.shape[1] - K0) // S0 + 1
    return wave.unfold(1, K0, S0)[:, :T0]                               # [B, T0, K]


def conv0_ln_ref64(wave, w, bias, gamma, beta, **mut):
    """Float64 reference of conv0_ln_gelu on [B, nsamp]; mut: unbiased / no_eps / no_bias mutants."""
    no_bias = mut.pop("no_bias", False)
    X = conv0_frames(wave.double().cpu())
    wd, bd = w.double().cpu(), bias.double().cpu()
    y = X @ wd.t() + (0.0 if no_bias else bd)
    ya = X.abs() @ wd.abs().t() + bd.abs()
    return row_ln64(y, ya, gamma.cpu(), beta.cpu(), **mut)


def conv0_ln_emulate(wave, w, bias, gamma, beta):
    """z as conv0_ln_gelu_kernel forms it."""
    X = conv0_frames(wave.float())
    B, T0, _ = X.shape
    y = bias.float()[None, None, :].expand(B, T0, -1)
    for k in range(K0):
        y = _fma32(w.float()[None, None, :, k], X[:, :, k, None], y)
    C = y.shape[-1]
    return row_ln_emulate(y.reshape(B * T0, C), gamma, beta, mul_inv=True).reshape(B, T0, C)


@functools.lru_cache(maxsize=None)
def ln_gelu_operands(N, d, dt):
    """x [N, d] (randn times a power of two per row 2^-6 .. 2^2, plus a per-row offset; row N // 2 is constant where N > 1) in
    dtype dt, gamma = 1 + 0.1 randn, beta = 0.1 randn."""
    gen = _Rng(7000 + 13 * N + d)
    x = gen.randn(N, d) * gen.pow2(-6, 2, N, 1)
    x = x + gen.randn(N, 1)
    if N > 1:
        x[N // 2] = 0.75
    return x.to(dt), 1.0 + 0.1 * gen.randn(d), 0.1 * gen.randn(d)


def ln_gelu_ref64(x, gamma, beta, **mut):
    xd = x.double().cpu()
    return row_ln64(xd, xd.abs(), gamma.cpu(), beta.cpu(), **mut)


def bf16_round_bound(ref, b):
    """b plus one rounding to nearest bf16 of a value within b of ref (helpers.bf16_round_bound)."""
    m = ref.abs() + b
    _, e = torch.frexp(m)
    half = torch.ldexp(torch.ones_like(m), e - 9)
    return b + torch.where(m > 0, half, torch.zeros_like(m))


def row_bound(r, which, bf16_out):
    """Per-element bound of a kernel output: |gelu'| C u s + the GELU form's absolute error (+ the bf16 rounding)."""
    b = r.lin * (LARGE_C[which] * U24) * r.s + (GELU_BF16OUT_ABS if bf16_out else GELU_ABS)
    return bf16_round_bound(r.ref, b) if bf16_out else b


def pre_bound(r, which):
    """The bound of the pre-activation z alone (the mutant checks and the constants use it)."""
    return (LARGE_C[which] * U24) * r.s
