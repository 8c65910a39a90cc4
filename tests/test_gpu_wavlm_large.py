"""The WavLM-Large family end to end on the GPU against transformers' float64 model (tests/golden/wavlm_large.npz,
made by tests/golden/make_golden_wavlm_large.py; pinned on the CPU by tests/test_cpu_wavlm_large.py). The weights and
the waveform are rebuilt from names (wavlm_large_ref.large_sd / large_wave); transformers is not imported here.

Budgets: helpers.close (largest error relative to the reference's largest magnitude) with the whole-encoder budgets of
tests/test_gpu_models.py: 1e-4 in fp32 mode, 5e-2 in bf16 mode, at 2 and at 24 layers alike.
"""
import functools

import pytest
import torch

import wavlm_large_ref as R
from helpers import T, close, load

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
PRECS = [("fp32", 1e-4), ("bf16", 5e-2)]


def _rt():
    from fddm_hip import runtime as rt
    return rt


@functools.lru_cache(maxsize=None)
def _sd(tag):
    geom, d_model, _, _ = R.GEOMS[tag]
    return R.large_sd(geom, d_model)


def _encoder(tag, pooling="none"):
    from models.acoustic_encoder import AcousticEncoder
    geom, d_model, _, _ = R.GEOMS[tag]
    enc = AcousticEncoder(wavlm_name=dict(geom), d_model=d_model, pooling=pooling)
    assert enc.backbone.stable_ln
    sd = enc.state_dict()
    for n, v in _sd(tag).items():
        assert n in sd and sd[n].shape == v.shape, n
        sd[n] = v
    enc.load_state_dict(sd)
    return enc.to(dev).eval()


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("tag", ["small", "wide", "full"])
def test_large_encoder_matches_transformers_float64(tag, prec, tol):
    g = load("wavlm_large")
    B = R.GEOMS[tag][2]
    with _rt().use_precision(prec):
        enc = _encoder(tag)
        feats, m, pooled = enc(R.large_wave(B).to(dev))
        assert m is None and pooled is None
        if tag != "full":       # the conv feature extractor alone (7 conv layers, their LayerNorms and GELUs), seen
            from fddm_hip import ops        # as HF's extract_features: through the feature projection's LayerNorm
            bb = enc.backbone
            h = bb.stage_conv1(bb.stage_conv0(R.large_wave(B).to(dev)))
            for i in range(2, 7):
                h = bb._conv(h, i)
            fp = bb.feature_projection.layer_norm
            hn = torch.empty_like(h)
            ops.ln_fwd(h.view(-1, h.shape[-1]), None, fp.weight.float(), fp.bias.float(),
                       out_t=hn.view(-1, h.shape[-1]), eps=bb.config.layer_norm_eps)
            close(hn.float(), g[tag + "_conv"], rtol=tol, what=f"{prec} {tag} conv stack")
    close(feats.float(), g[tag + "_feats"], rtol=tol, what=f"{prec} {tag} feats")


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("tag", ["small", "wide"])
def test_large_encoder_with_lengths_matches_transformers_float64(tag, prec, tol):
    """AcousticEncoder(wave, lengths), pooling="mean": the features on the kept frames, the returned mask (equal, not
    close) and the pooled mean, as tests/test_gpu_lengths.py compares them for the base family."""
    g = load("wavlm_large")
    B = R.GEOMS[tag][2]
    with _rt().use_precision(prec):
        enc = _encoder(tag, pooling="mean")
        feats, mask, pooled = enc(R.large_wave(B).to(dev), T(g[tag + "_lengths"]).to(dev))
    want = T(g[tag + "_m_mask"])
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), want)
    close(feats.float().cpu()[want], T(g[tag + "_m_feats"])[want], rtol=tol, what=f"{prec} {tag} kept feats")
    close(pooled, g[tag + "_m_pooled"], rtol=tol, what=f"{prec} {tag} pooled")


def test_graphed_large_encoder_matches_eager_bf16():
    """fddm_hip.graphs.GraphedEncoder captures the large encoder through the unchanged stage_conv0 / stage_conv1 /
    stage_rest split; both slots replay the eager result bit for bit in bf16."""
    from fddm_hip.graphs import GraphedEncoder
    gen = torch.Generator().manual_seed(5)
    waves = [(0.1 * torch.randn(3, 16000, generator=gen)).to(dev) for _ in range(4)]
    with _rt().use_precision("bf16"):
        enc = _encoder("small")
        ge = GraphedEncoder(enc)
        assert GraphedEncoder.supported(enc)
        got = [ge.run(w, i % 2).float().clone() for i, w in enumerate(waves)]
        torch.cuda.synchronize()
        refs = [enc(w)[0].float() for w in waves]
    for i, (a, r) in enumerate(zip(got, refs)):
        assert torch.isfinite(r).all() and torch.equal(a, r), f"batch {i}: graph replay differs from eager"
    assert not torch.equal(refs[0], refs[1])


def test_large_encoder_runs_on_the_mfma_families_bf16():
    """wide-large, unmasked, bf16: the layers' attention is the 32x32x16 family's forward in its WavLM bias build
    (fwd7, REL), not the register-staged fallbacks; conv layer 1 (bias + plain store) meets the 256x256 kernel's
    preconditions: forced to that family it runs there (a forced family whose preconditions fail falls through to
    the register-staged kernel without a word) and gives the default kernel's result. The dispatcher's own choice
    goes by the tile count: 2 x 1 s is 26 tiles of 256 x 256, below the 64 from which it prefers that kernel (and
    below the 128-row ring's 240), so the fixture's batch runs register-staged by the shape rule, as the base family
    does at that size; 6 x 1 s (76 tiles) takes the 256x256 kernel unforced."""
    from fddm_hip import ops
    B = R.GEOMS["wide"][2]
    wave = R.large_wave(B).to(dev)
    with _rt().use_precision("bf16"):
        enc = _encoder("wide")
        bb = enc.backbone
        bb.stage_conv1(bb.stage_conv0(R.large_wave(6).to(dev)))
        assert ops.gemm_last_path() == ("256", 1), ops.gemm_last_path()
        h0 = bb.stage_conv0(wave)
        h1 = bb.stage_conv1(h0)
        assert ops.gemm_last_path() == ("small", 1), ops.gemm_last_path()
        old = ops.gemm_force_path("256")
        try:
            h1f = bb.stage_conv1(h0)
            assert ops.gemm_last_path() == ("256", 1), ops.gemm_last_path()
        finally:
            ops.gemm_force_path(old)
        close(h1f.float(), h1.float(), rtol=2e-2, what="conv layer 1 on the 256x256 kernel vs the default family")
        bb.stage_rest(h1)
        kernel, _, _, kx, rel = ops.attn_last_path()["fwd"]
        torch.cuda.synchronize()
    assert (kernel, kx, rel) == ("fwd7", False, True), ops.attn_last_path()
