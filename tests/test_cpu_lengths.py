"""Variable-length audio on the CPU: a torch restatement of the reference's masked paths, pinned to the fixture the
reference itself produced (tests/golden/lengths.npz, tests/golden/make_golden_lengths.py), the new C-ABI symbols, and
the key-extent definition.

The restatement (fp32 torch, built from the oracle's pieces) covers what oracle/fddm_oracle.py lacks:
  masked_wavlm_forward     HF WavLMModel.forward with attention_mask (modeling_wavlm.py:1053-1073, 654-672, 399-402, 198)
  masked_acoustic_encoder  reference models/acoustic_encoder.py:92-128 (lengths -> feats, feat_mask, pooled)
  masked_decoder_forward   reference models/denoise_decoder.py:147-192, 242-287 with c_mask (cross-attention
                           key_padding_mask and the masked FiLM pooled mean)
tests/test_gpu_lengths.py imports them as the reference at the shapes the fixture does not cover.
Bound: the project's fp32 parity bound, 1e-4 of the reference's maximum (tests/test_oracle_golden.py).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import SMALL_WAVLM, T, _dec_sd, close, load, wavlm_sd
from oracle import fddm_oracle as O
from oracle.weights import pcg_array

LENGTHS_DEC = dict(V=96, d=128, H=2, NL=2, FF=256, L=32)


def load_lengths():
    """The lengths fixture: lengths.npz plus the decoder gradients kept in files of their own (no committed file may
    pass 1 MiB; make_golden_lengths.py grad_file)."""
    g = {}
    for f in ("lengths", "lengths_grads_b0", "lengths_grads_b1", "lengths_grads_time"):
        g.update(load(f))
    return g


def lengths_inputs():
    """The fixture's inputs that are functions of a name alone (make_golden_lengths.py lengths_inputs): the waveform
    [3, 16000] ~ 0.1 N(0, 1) and the loss weights R [3, L, V] ~ N(0, 1)."""
    wave = 0.1 * math.sqrt(16000.0) * pcg_array("lengths.wave", (3, 16000))
    R = math.sqrt(LENGTHS_DEC["L"] * LENGTHS_DEC["V"]) * pcg_array("lengths.R", (3, LENGTHS_DEC["L"], LENGTHS_DEC["V"]))
    return torch.from_numpy(wave.astype(np.float32)), torch.from_numpy(R.astype(np.float32))


# ------------------------------------------------------------------------------------------- restatement
def key_extent_ref(keep: torch.Tensor) -> torch.Tensor:
    """1 + the largest k with keep[b][k] != 0, 0 if there is none (fddm_key_extent's definition)."""
    k = torch.arange(1, keep.shape[1] + 1, device=keep.device)
    return ((keep != 0).long() * k).amax(1).to(torch.int32)


def feature_mask(attention_mask: torch.Tensor, S: int, g: dict) -> torch.Tensor:
    """HF _get_feature_vector_attention_mask (modeling_wavlm.py:654-672)."""
    n = attention_mask.long().sum(-1)
    for k, s in zip(g["conv_kernel"], g["conv_stride"]):
        n = torch.div(n - k, s, rounding_mode="floor") + 1                  # HF:640-646
    m = torch.zeros(attention_mask.shape[0], S, dtype=torch.long)
    m[torch.arange(m.shape[0]), n - 1] = 1                                   # HF:670
    return m.flip([-1]).cumsum(-1).flip([-1]).bool()                         # HF:671


def masked_wavlm_forward(sd, wave, attention_mask, g, pre=""):
    """O.wavlm_forward with HF's attention_mask path: the conv feature extractor sees the whole padded waveform
    (HF:1053); padded frames are zeroed after the feature projection (HF:399-402) and are no keys in any layer
    (HF:198); the output rows at padded positions are whatever the layers leave there."""
    eps = g["layer_norm_eps"]
    E, H = g["hidden_size"], g["num_attention_heads"]
    dh = E // H
    fe = O.wavlm_feature_extractor(sd, pre, wave, g).transpose(1, 2)
    keep = feature_mask(attention_mask, fe.shape[1], g)
    x = F.layer_norm(fe, (fe.shape[-1],), sd[pre + "feature_projection.layer_norm.weight"],
                     sd[pre + "feature_projection.layer_norm.bias"], eps)
    x = F.linear(x, sd[pre + "feature_projection.projection.weight"], sd[pre + "feature_projection.projection.bias"])
    x = x * keep[..., None].to(x.dtype)                                      # HF:399-402
    gw = sd[pre + "encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
    vw = sd[pre + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
    w = gw * vw / vw.norm(dim=(0, 1), keepdim=True)
    kpos = g["num_conv_pos_embeddings"]
    pos = F.conv1d(x.transpose(1, 2), w, sd[pre + "encoder.pos_conv_embed.conv.bias"], padding=kpos // 2,
                   groups=g["num_conv_pos_embedding_groups"])
    if kpos % 2 == 0:
        pos = pos[:, :, :-1]
    x = x + F.gelu(pos).transpose(1, 2)
    x = F.layer_norm(x, (E,), sd[pre + "encoder.layer_norm.weight"], sd[pre + "encoder.layer_norm.bias"], eps)
    B, S, _ = x.shape
    rel = torch.arange(S)[None, :] - torch.arange(S)[:, None]
    bucket = O.rel_position_bucket(rel, g["num_buckets"], g["max_bucket_distance"])
    bias = sd[pre + "encoder.layers.0.attention.rel_attn_embed.weight"][bucket].permute(2, 0, 1)
    for i in range(g["num_hidden_layers"]):
        lp = f"{pre}encoder.layers.{i}."
        a = lp + "attention."
        gh = x.view(B, S, H, dh).permute(0, 2, 1, 3)
        rp = F.linear(gh, sd[a + "gru_rel_pos_linear.weight"], sd[a + "gru_rel_pos_linear.bias"])
        rp = rp.view(B, H, S, 2, 4).sum(-1)
        ga, gb = torch.sigmoid(rp).chunk(2, dim=-1)
        gate = ga * (gb * sd[a + "gru_rel_pos_const"].view(1, H, 1, 1) - 1.0) + 2.0
        q = F.linear(x, sd[a + "q_proj.weight"], sd[a + "q_proj.bias"]).view(B, S, H, dh).transpose(1, 2)
        k = F.linear(x, sd[a + "k_proj.weight"], sd[a + "k_proj.bias"]).view(B, S, H, dh).transpose(1, 2)
        v = F.linear(x, sd[a + "v_proj.weight"], sd[a + "v_proj.bias"]).view(B, S, H, dh).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dh) + gate * bias[None]
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))           # HF:198 key_padding_mask
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, E)
        o = F.linear(o, sd[a + "out_proj.weight"], sd[a + "out_proj.bias"])
        x = F.layer_norm(x + o, (E,), sd[lp + "layer_norm.weight"], sd[lp + "layer_norm.bias"], eps)
        ffh = F.gelu(F.linear(x, sd[lp + "feed_forward.intermediate_dense.weight"],
                              sd[lp + "feed_forward.intermediate_dense.bias"]))
        ff = F.linear(ffh, sd[lp + "feed_forward.output_dense.weight"], sd[lp + "feed_forward.output_dense.bias"])
        x = F.layer_norm(x + ff, (E,), sd[lp + "final_layer_norm.weight"], sd[lp + "final_layer_norm.bias"], eps)
    return x, keep


def masked_acoustic_encoder(sd, wave, lengths, g, d_model, pooling="mean"):
    """Reference acoustic_encoder.py:92-128: (feats, feat_mask, pooled). The returned mask uses the reference's own
    ceil(len / 320) frame count (clamped to S), not the backbone's."""
    T_ = wave.shape[1]
    attention_mask = torch.arange(T_)[None, :] < lengths[:, None]             # :96
    h, _ = masked_wavlm_forward(sd, wave, attention_mask, g, pre="backbone.")
    if g["hidden_size"] != d_model:
        h = F.linear(h, sd["proj.weight"], sd["proj.bias"])                  # :107
    S = h.shape[1]
    fl = torch.clamp((lengths + 319) // 320, max=S)                          # :73-82, :114-116
    feat_mask = torch.arange(S)[None, :] < fl[:, None]                       # :117
    pooled = None
    if pooling == "mean":
        denom = feat_mask.sum(1).clamp(min=1).unsqueeze(-1)                  # :125
        pooled = (h * feat_mask.unsqueeze(-1)).sum(1) / denom                # :126
    return h, feat_mask, pooled


def masked_decoder_block(sd, pre, x, cond, x_mask, c_mask, cos, sin, H, drop=None):
    """O.decoder_block with c_mask: the cross-attention's key_padding_mask (:173) and the masked pooled mean
    (:181-183, count not clamped)."""
    p = drop.p if drop is not None else 0.0
    D = (lambda z: drop(z)) if drop is not None else (lambda z: z)
    d = x.shape[-1]
    qk = O.rope_apply(x, cos, sin)
    a = pre + "self_attn."
    x2 = O.mha(qk, qk, x, sd[a + "in_proj_weight"], sd[a + "in_proj_bias"], sd[a + "out_proj.weight"],
               sd[a + "out_proj.bias"], H, key_keep=x_mask, drop_p=p, drop=drop)
    x = F.layer_norm(x + D(x2), (d,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5)
    a = pre + "cross_attn."
    x2 = O.mha(x, cond, cond, sd[a + "in_proj_weight"], sd[a + "in_proj_bias"], sd[a + "out_proj.weight"],
               sd[a + "out_proj.bias"], H, key_keep=c_mask, drop_p=p, drop=drop)
    x = F.layer_norm(x + D(x2), (d,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-5)
    if c_mask is not None:
        pooled = (cond * c_mask.unsqueeze(-1).float()).sum(1) / c_mask.sum(1, keepdim=True).float()   # :183
    else:
        pooled = cond.mean(dim=1)
    scale = F.linear(pooled, sd[pre + "film_layer.scale_proj.weight"], sd[pre + "film_layer.scale_proj.bias"])
    shift = F.linear(pooled, sd[pre + "film_layer.shift_proj.weight"], sd[pre + "film_layer.shift_proj.bias"])
    x = x * (1 + scale[:, None]) + shift[:, None]
    h = F.gelu(F.linear(x, sd[pre + "ff.0.weight"], sd[pre + "ff.0.bias"]))
    h = D(h)
    x2 = F.linear(h, sd[pre + "ff.3.weight"], sd[pre + "ff.3.bias"])
    return F.layer_norm(x + D(x2), (d,), sd[pre + "norm3.weight"], sd[pre + "norm3.bias"], 1e-5)


def masked_decoder_forward(sd, xt, t, cond, x_mask, c_mask, H, num_layers, pad_id=0, dropout=0.0, seed=0):
    """O.decoder_forward with c_mask (the same dropout sites in the same order: the oracle's _Dropper)."""
    d = sd["tok_emb.weight"].shape[1]
    L = xt.shape[1]
    x = F.embedding(xt, sd["tok_emb.weight"], padding_idx=pad_id)
    cos, sin = O.rope_cos_sin(L, O.rope_inv_freq(d))
    te = O.time_embedding(t, d)
    te = F.linear(F.silu(F.linear(te, sd["time_emb.mlp.0.weight"], sd["time_emb.mlp.0.bias"])),
                  sd["time_emb.mlp.2.weight"], sd["time_emb.mlp.2.bias"])
    x = x + F.linear(te, sd["time_proj.weight"], sd["time_proj.bias"])[:, None]
    if x_mask is None:
        x_mask = xt != pad_id
    drop = O._Dropper(dropout, seed) if dropout > 0 else None
    for i in range(num_layers):
        x = masked_decoder_block(sd, f"blocks.{i}.", x, cond, x_mask, c_mask, cos, sin, H, drop)
    return F.linear(x, sd["head.weight"], sd["head.bias"])


# ------------------------------------------------------------------------------------------------- tests
HAND_MASKS = {  # name -> (mask rows, expected extents)
    "all kept": ([[1, 1, 1, 1, 1]], [5]),
    "none kept": ([[0, 0, 0, 0, 0]], [0]),
    "hole in the middle": ([[1, 1, 0, 0, 1, 1, 0, 0]], [6]),
    "single trailing key": ([[0, 0, 0, 0, 0, 0, 1]], [7]),
    "single leading key": ([[1, 0, 0, 0]], [1]),
    "non-0/1 bytes keep": ([[0, 7, 255, 0]], [3]),
}


@pytest.mark.parametrize("name", list(HAND_MASKS))
def test_key_extent_definition_on_hand_made_masks(name):
    rows, want = HAND_MASKS[name]
    keep = torch.tensor(rows, dtype=torch.uint8)
    assert key_extent_ref(keep).tolist() == want
    # the bound keeps every kept key inside it and ends on one (or is 0)
    e = want[0]
    assert not keep[0, e:].any() and (e == 0 or keep[0, e - 1] != 0)


def test_new_symbols_are_declared_and_exported():
    from fddm_hip import _lib
    names = set(_lib.declared_symbols())
    L = _lib.lib()
    for n in ("fddm_key_extent", "fddm_attn_fwd_kx", "fddm_attn_bwd_kx", "fddm_attn_fwd_relgate_x_kx",
              "fddm_rows_mean_masked", "fddm_rows_zero_masked"):
        assert n in names, f"{n} is not declared in include/fddm_hip.h"
        assert hasattr(L, n), f"{n} is not exported"
    assert L.fddm_abi_version() == 6


def test_feature_mask_matches_hf_frame_counts():
    """500 samples keep a single frame, a full second all 49; the package's device-side restatement
    (WavLMModel.feature_mask) equals the CPU one."""
    from models.wavlm import WavLMModel, wavlm_config
    g = O.wavlm_geometry(**SMALL_WAVLM)
    lengths = torch.tensor([16000, 9000, 500, 400])
    am = torch.arange(16000)[None, :] < lengths[:, None]
    keep = feature_mask(am, 49, g)
    assert keep.sum(1).tolist() == [49, 27, 1, 1]
    m = WavLMModel(wavlm_config(**SMALL_WAVLM))
    assert torch.equal(m.feature_mask(am, 49), keep)


@pytest.mark.parametrize("tag,geom,d_model", [("tiny", SMALL_WAVLM, 64), ("base", {}, 128)])
def test_masked_encoder_restatement_matches_reference_fixture(tag, geom, d_model):
    g = load("lengths")
    wave, _ = lengths_inputs()
    geo = O.wavlm_geometry(**geom)
    sd = wavlm_sd(geo, d_model)
    with torch.no_grad():
        feats, mask, pooled = masked_acoustic_encoder(sd, wave, T(g["lengths"]), geo, d_model)
    assert torch.equal(mask, T(g[tag + "_mask"]))
    close(feats, g[tag + "_feats"], rtol=1e-4, what=f"{tag} feats")
    close(pooled, g[tag + "_pooled"], rtol=1e-4, what=f"{tag} pooled")


def test_masked_decoder_restatement_matches_reference_fixture():
    g = load_lengths()
    _, R = lengths_inputs()
    V, d, H, NL, FF = (LENGTHS_DEC[k] for k in ("V", "d", "H", "NL", "FF"))
    sd = {n: p.clone().requires_grad_(True) for n, p in _dec_sd(V, d, H, NL, FF).items()}
    logits = masked_decoder_forward(sd, T(g["dec_xt"]), T(g["dec_t"]), T(g["base_feats"]), None, T(g["base_mask"]),
                                    H, NL)
    close(logits, g["dec_logits"], rtol=1e-4, what="decoder logits")
    (logits * R).sum().backward()
    for n, p in sd.items():
        gr = p.grad if p.grad is not None else torch.zeros_like(p)
        assert "g." + n in g, f"the fixture holds no full gradient of {n}"
        close(gr, g["g." + n], rtol=1e-4, atol=1e-6, what="grad " + n)
        close((gr.double() ** 2).sum(), g["g_sq." + n], rtol=2e-4, atol=1e-12, what="grad sq " + n)
