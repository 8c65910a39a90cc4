"""Generate tests/golden/wavlm_large.npz: the WavLM-Large family (feat_extract_norm="layer", conv_bias,
do_stable_layer_norm) of transformers' own WavLMModel on the CPU, with oracle.weights.load_pcg weights (names -> PCG64)
and the projection / masks / pooling of the reference AcousticEncoder restated (tests/wavlm_large_ref.py hf_forward).

Run from the repo root:  python tests/golden/make_golden_wavlm_large.py
Only arrays are saved. The waveform and the weights are pure functions of names (wavlm_large_ref.large_wave,
large_sd): tests rebuild them and never import transformers on the GPU.

Dtypes: `small` and `wide` are computed in float64; `full` (24 layers, 1.3 GB of fp32 weights) is computed in float64
as well (a few seconds on 8 cores). Arrays are stored as float64 except the 512-wide conv checkpoint (float32).

Contents (tag in small / wide / full; geometries, d_model, batch and lengths in wavlm_large_ref.GEOMS)
  {tag}_feats                 proj(last_hidden_state) [B, 49, d_model], no attention_mask
  {tag}_conv                  small, wide: HF's extract_features (the conv feature extractor's output through the
                              feature projection's LayerNorm) [B, 49, C] of the unmasked run; wide as float32
  {tag}_m_feats / _m_mask / _m_pooled / _lengths
                              small, wide: the masked run (lengths, pooling="mean")
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
import wavlm_large_ref as R  # noqa: E402


def arrays(tag):
    geom, d_model, B, lengths = R.GEOMS[tag]
    m, proj = R.hf_encoder64(geom, d_model, torch.float64)
    wave = R.large_wave(B)
    out = {}
    feats, _, _, conv = R.hf_forward(m, proj, wave)
    out[tag + "_feats"] = feats.numpy()
    if tag != "full":
        out[tag + "_conv"] = conv.numpy() if tag == "small" else conv.float().numpy()
    if lengths is not None:
        ln = torch.tensor(lengths)
        f, mask, pooled, _ = R.hf_forward(m, proj, wave, ln)
        out.update({tag + "_m_feats": f.numpy(), tag + "_m_mask": mask.numpy(), tag + "_m_pooled": pooled.numpy(),
                    tag + "_lengths": ln.numpy()})
    return out


def main():
    out = {}
    for tag in R.GEOMS:
        out.update(arrays(tag))
        print(tag, "done")
    path = os.path.join(HERE, "wavlm_large.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
