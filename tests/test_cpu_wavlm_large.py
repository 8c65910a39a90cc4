"""The WavLM-Large family (feat_extract_norm="layer", conv_bias, do_stable_layer_norm) without a device: the
parameter tree against transformers', loading a local checkpoint directory, the fixture's pin, the argument checks of
the two new C entries, and what tests/test_gpu_wavlm_large_kernels.py may ask of conv0_ln_gelu and ln_gelu_fwd.

E: each kernel's arithmetic emulated on the CPU in its own order (wavlm_large_ref.conv0_ln_emulate: bias, ten fp32 FMAs
in tap order, row sums as 8 per lane in order then a 64-lane tree, centred second pass, fma with the affine;
row_ln_emulate the same from given rows) against float64, in units of u s (u = 2^-24, s in wavlm_large_ref's
docstring), the maximum over every case the GPU test runs:
    family      measured E    stored E    C = 8 E
    conv0_ln    5.21          5.5         44.0
    ln_gelu     5.18          5.45        43.6
The inputs are drawn with numpy's PCG64 (wavlm_large_ref._Rng), not torch.randn, whose CPU kernels differ in the last
bits between instruction sets: E is a maximum of rounding errors and must come out the same on every machine.
Mutants of the reference (each must leave the f32-output bound on at least half of the elements it changes; the
least share over the cases it is asserted on):
    conv0_ln    unbiased variance (every case) 0.957, eps dropped (the silent frames) 0.938, bias omitted (every
                case) 0.984
    ln_gelu     unbiased variance (every case with N > 1) 0.946, eps dropped (rows of variance < 1e-2) 0.975
"""
import ctypes
import json
import os

import pytest
import torch

import wavlm_large_ref as R
from helpers import load

F = torch.nn.functional
INVALID = 1     # hipErrorInvalidValue


def _hf(geom):
    from transformers import WavLMConfig, WavLMModel
    return WavLMModel(WavLMConfig(**geom))


# ------------------------------------------------------------------------------------------ parameter tree, loading
def test_state_dict_matches_transformers():
    from models.acoustic_encoder import AcousticEncoder
    enc = AcousticEncoder(wavlm_name=dict(R.SMALL_LARGE), d_model=64)
    assert enc.backbone.random_init and enc.backbone.stable_ln
    ours = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    hf = {"backbone." + k: tuple(v.shape) for k, v in _hf(R.SMALL_LARGE).state_dict().items()}
    hf["proj.weight"], hf["proj.bias"] = (64, 128), (64,)
    assert ours == hf
    # and the names the tests generate weights from are exactly these (masked_spec_embed is unused in eval)
    assert set(R.large_shapes(R.SMALL_LARGE, 64)) | {"backbone.masked_spec_embed"} == set(ours)
    assert all(ours[k] == s for k, s in R.large_shapes(R.SMALL_LARGE, 64).items())


def test_large_geometry_is_the_published_one():
    from models.wavlm import WAVLM_LARGE, wavlm_config
    c = wavlm_config(**WAVLM_LARGE)
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size) == (1024, 24, 16, 4096)
    assert tuple(c.conv_dim) == (512,) * 7 and tuple(c.conv_kernel) == (10, 3, 3, 3, 3, 2, 2)
    assert tuple(c.conv_stride) == (5, 2, 2, 2, 2, 2, 2)
    assert (c.feat_extract_norm, c.conv_bias, c.do_stable_layer_norm) == ("layer", True, True)
    assert (c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, c.num_buckets, c.max_bucket_distance) == \
        (128, 16, 320, 800)
    assert c.hidden_size // c.num_attention_heads == 64 and c.hidden_size // c.num_conv_pos_embedding_groups == 64


def _write_dir(path, hf_model, legacy):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        f.write(hf_model.config.to_json_string())
    sd = {}
    for k, v in hf_model.state_dict().items():
        if legacy:
            k = k.replace("parametrizations.weight.original0", "weight_g").replace(
                "parametrizations.weight.original1", "weight_v")
        sd[k] = v.detach().clone().contiguous()
    save_file(sd, os.path.join(path, "model.safetensors"))
    return sd


@pytest.mark.parametrize("legacy", [False, True], ids=["parametrizations", "weight_g_v"])
def test_from_pretrained_loads_a_large_family_directory_strictly(tmp_path, legacy):
    from models.acoustic_encoder import AcousticEncoder
    from safetensors.torch import save_file
    hf = _hf(R.SMALL_LARGE)
    sd = _write_dir(str(tmp_path / "ok"), hf, legacy)
    assert json.load(open(tmp_path / "ok" / "config.json"))["do_stable_layer_norm"] is True
    enc = AcousticEncoder(wavlm_name=str(tmp_path / "ok"), d_model=64)
    assert not enc.backbone.random_init and enc.backbone.stable_ln
    got = enc.backbone.state_dict()
    want = hf.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    # a deleted key raises
    bad = str(tmp_path / "bad")
    _write_dir(bad, hf, legacy)
    sd.pop("feature_extractor.conv_layers.3.conv.bias")
    save_file(sd, os.path.join(bad, "model.safetensors"))
    with pytest.raises(RuntimeError, match="conv_layers.3.conv.bias"):
        AcousticEncoder(wavlm_name=bad, d_model=64)


@pytest.mark.parametrize("sw", [dict(feat_extract_norm="layer"), dict(conv_bias=True), dict(do_stable_layer_norm=True),
                                dict(feat_extract_norm="layer", conv_bias=True),
                                dict(feat_extract_norm="layer", do_stable_layer_norm=True),
                                dict(conv_bias=True, do_stable_layer_norm=True)],
                         ids=lambda d: "+".join(sorted(d)))
def test_mixed_switches_are_refused(sw):
    from models.wavlm import WavLMModel, wavlm_config
    geom = {k: v for k, v in R.SMALL_LARGE.items() if k not in R.SWITCHES}
    with pytest.raises(NotImplementedError, match="only the two WavLM families transformers ships are built"):
        WavLMModel(wavlm_config(**geom, **sw))


def test_fixture_is_transformers_float64_on_small_large():
    g = load("wavlm_large")
    geom, d_model, B, lengths = R.GEOMS["small"]
    m, proj = R.hf_encoder64(geom, d_model)
    assert type(m.encoder).__name__ == "WavLMEncoderStableLayerNorm"
    assert type(m.feature_extractor.conv_layers[0]).__name__ == "WavLMLayerNormConvLayer"
    wave = R.large_wave(B)
    feats, _, _, conv = R.hf_forward(m, proj, wave)
    assert (feats - torch.from_numpy(g["small_feats"])).abs().max().item() <= 1e-12
    assert (conv - torch.from_numpy(g["small_conv"])).abs().max().item() <= 1e-12
    assert tuple(g["small_lengths"]) == lengths
    f, mask, pooled, _ = R.hf_forward(m, proj, wave, torch.tensor(lengths))
    assert (f - torch.from_numpy(g["small_m_feats"])).abs().max().item() <= 1e-12
    assert (pooled - torch.from_numpy(g["small_m_pooled"])).abs().max().item() <= 1e-12
    assert torch.equal(mask, torch.from_numpy(g["small_m_mask"])) and mask.sum(1).tolist() == [49, 29, 2]
    for tag, (_, dm, b, ln) in R.GEOMS.items():
        assert g[tag + "_feats"].shape == (b, 49, dm)


# ------------------------------------------------------------------------------------------ argument checks
def test_new_entries_refuse_bad_arguments_without_a_device():
    """Every rejected call returns hipErrorInvalidValue before anything is launched: no device is needed (the pointers
    are never dereferenced)."""
    from fddm_hip._lib import lib
    L = lib()
    p = 0x10000          # a 16-B aligned non-null address
    ok0 = dict(out_dtype=0, x=p, w=p, bias=p, gamma=p, beta=p, out=p, B=2, nsamp=33, T0=5, C=32, K=10, S=5)

    def conv0(**over):
        a = dict(ok0, **over)
        return L.fddm_conv0_ln_gelu(a["out_dtype"], a["x"], a["w"], a["bias"], a["gamma"], a["beta"], a["out"], a["B"],
                                    a["nsamp"], a["T0"], a["C"], a["K"], a["S"], ctypes.c_float(1e-5), None)

    bad0 = [dict(K=8), dict(K=16), dict(C=31), dict(C=33), dict(C=36), dict(C=520), dict(C=0), dict(S=0), dict(S=17),
            dict(out_dtype=2), dict(x=0), dict(w=0), dict(bias=0), dict(gamma=0), dict(beta=0), dict(out=0),
            dict(w=p + 4), dict(bias=p + 8), dict(gamma=p + 4), dict(beta=p + 12), dict(out=p + 2), dict(x=p + 2),
            dict(T0=6), dict(nsamp=29), dict(B=-1), dict(B=70000)]
    for over in bad0:
        assert conv0(**over) == INVALID, over
    assert conv0(B=0) == 0 and conv0(T0=0) == 0           # nothing to do: no launch, no error

    ok1 = dict(xd=0, od=1, x=p, gamma=p, beta=p, out=p + 0x1000, N=3, d=64)

    def lng(**over):
        a = dict(ok1, **over)
        return L.fddm_ln_gelu_fwd(a["xd"], a["od"], a["x"], a["gamma"], a["beta"], a["out"], a["N"], a["d"],
                                  ctypes.c_float(1e-5), None)

    bad1 = [dict(d=520), dict(d=1024), dict(d=60), dict(d=7), dict(d=0), dict(xd=2), dict(od=-1), dict(x=0),
            dict(gamma=0), dict(beta=0), dict(out=0), dict(x=p + 8), dict(gamma=p + 4), dict(beta=p + 4),
            dict(out=p + 2), dict(out=p), dict(N=-1)]            # out == x with different dtypes
    for over in bad1:
        assert lng(**over) == INVALID, over
    assert lng(N=0) == 0


# ------------------------------------------------------------------------------------------ error constants, mutants
def _share(r, which, mut):
    """Share of the elements the mutant reference changes at which it leaves the f32-output bound."""
    touched = mut.ref != r.ref
    assert touched.any()
    return ((mut.ref - r.ref).abs() > R.row_bound(r, which, False))[touched].float().mean().item()


def _sel(r, mut, rows):
    """mut restricted to `rows` (a bool mask over r.ref's leading axes): elsewhere the reference itself."""
    m = R.RowRef()
    m.ref = torch.where(rows[..., None], mut.ref, r.ref)
    return m


def test_front_error_constants():
    E = {"conv0_ln": 0.0, "ln_gelu": 0.0}
    least = {}

    def low(k, v):
        least[k] = min(least.get(k, 1.0), v)

    for C in R.CONV0_LN_C:
        for const_bias in (False, True):
            w, bias, gamma, beta = R.conv0_ln_params(C, const_bias)
            for T0 in R.CONV0_LN_T0:
                if const_bias and T0 != 67:
                    continue
                wave = R.conv0_ln_wave(T0)
                assert wave.shape == (3, (T0 - 1) * 5 + 13)
                r = R.conv0_ln_ref64(wave, w, bias, gamma, beta)
                assert r.ref.shape == (3, T0, C) and (r.s > 0).all()
                z = R.conv0_ln_emulate(wave, w, bias, gamma, beta)
                assert torch.isfinite(z).all()
                E["conv0_ln"] = max(E["conv0_ln"], ((z.double() - r.z).abs() / (R.U24 * r.s)).max().item())
                # silent frames: the conv output is the bias vector
                silent = (R.conv0_frames(wave) == 0).all(-1)
                assert T0 == 1 or silent[2].any()
                if silent.any():
                    bd, gd, be = bias.double(), gamma.double(), beta.double()
                    zb = (bd - bd.mean()) / torch.sqrt(bd.var(unbiased=False) + R.LN_EPS) * gd + be
                    assert (r.z[silent] - zb).abs().max().item() <= 1e-12
                if const_bias:
                    continue
                low("conv0 unbiased", _share(r, "conv0_ln", R.conv0_ln_ref64(wave, w, bias, gamma, beta, unbiased=True)))
                low("conv0 no_bias", _share(r, "conv0_ln", R.conv0_ln_ref64(wave, w, bias, gamma, beta, no_bias=True)))
                if silent.any():
                    m = R.conv0_ln_ref64(wave, w, bias, gamma, beta, no_eps=True)
                    low("conv0 no_eps", _share(r, "conv0_ln", _sel(r, m, silent)))
    for d in R.LN_GELU_D:
        for N in R.LN_GELU_N:
            for dt in (torch.float32, torch.bfloat16):
                x, gamma, beta = R.ln_gelu_operands(N, d, dt)
                r = R.ln_gelu_ref64(x, gamma, beta)
                assert N == 1 or ((x[N // 2] == 0.75).all() and r.var[N // 2].item() == 0.0)
                z = R.row_ln_emulate(x.float(), gamma, beta)
                assert torch.isfinite(z).all()
                E["ln_gelu"] = max(E["ln_gelu"], ((z.double() - r.z).abs() / (R.U24 * r.s)).max().item())
                if N > 1:
                    low("ln_gelu unbiased", _share(r, "ln_gelu", R.ln_gelu_ref64(x, gamma, beta, unbiased=True)))
                quiet = (r.var[:, 0] < 1e-2) & (r.var[:, 0] > 0)
                if quiet.any():
                    m = R.ln_gelu_ref64(x, gamma, beta, no_eps=True)
                    m.ref = torch.where(torch.isfinite(m.ref), m.ref, r.ref)        # the constant row: 0 / 0
                    low("ln_gelu no_eps", _share(r, "ln_gelu", _sel(r, m, quiet)))
    print("\nLARGE_E measured " + ", ".join(f"{k} {v:.3f}" for k, v in E.items()) + "; least caught share per mutant "
          + ", ".join(f"{k} {v:.3f}" for k, v in least.items()))
    assert set(least) == {"conv0 unbiased", "conv0 no_bias", "conv0 no_eps", "ln_gelu unbiased", "ln_gelu no_eps"}
    for k, e in E.items():
        assert e <= R.LARGE_E[k] <= 1.1 * e + R.LARGE_E_FLOOR, (k, e)
        assert R.LARGE_C[k] <= 64.0
    for k, v in least.items():
        assert v >= 0.5, f"mutant {k} leaves the bound on only {v:.3f} of its elements"
