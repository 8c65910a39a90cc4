"""Generate tests/golden/lengths.npz: the REFERENCE's variable-length path (AcousticEncoder(waveforms, lengths) and
the decoder with c_mask), the way make_golden.py produces its fixtures.

Run from the repo root:  python tests/golden/make_golden_lengths.py
The reference is imported read-only (bytecode writing disabled); `WavLMModel.from_pretrained` is replaced by the local
PCG-weights constructor (oracle/weights.py). Only arrays are saved. Inputs that are pure functions of a name (the
waveform, the loss weights R) are NOT saved: tests rebuild them with lengths_inputs() below's recipe
(oracle.weights.pcg_array), restated in tests/test_cpu_lengths.py.

Contents
  lengths                      [3] sample counts 16000 (full), 9000, 500 (a single HF frame) of 3 x 1 s
  {tiny,base}_feats            AcousticEncoder(...)[0], pooling="mean": tiny = 2-layer geometry (d_model 64),
  {tiny,base}_mask / _pooled   base = WavLM-base geometry with d_model 128 (C1)
  dec_xt, dec_t                decoder inputs: d 128, H 2, 2 layers, L 32, V 96, dropout 0; cond = base_feats (S 49),
                               c_mask = base_mask, x_mask = None (xt != pad)
  dec_logits, g_sum.* g_sq.*   logits; per-parameter gradient sum and sum of squares (float64) of (logits * R).sum()
  g.*                          full gradients: make_golden.py's _dec_grads_subset (every parameter of at most 70000
                               elements, which at these sizes is every parameter). No committed file may pass 1 MiB,
                               so they are spread over four files (grad_file below): lengths_grads_b0.npz and
                               lengths_grads_b1.npz hold block 0's and block 1's self_attn, cross_attn and ff weight
                               gradients, lengths_grads_time.npz the time embedding's and time projection's,
                               lengths.npz the rest.
"""
from __future__ import annotations

import math
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("FDDM_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
from oracle.weights import load_pcg, pcg_array  # noqa: E402

SMALL_WAVLM = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                   conv_dim=(32,) * 7, num_conv_pos_embedding_groups=4)
LENGTHS = (16000, 9000, 500)
DEC = dict(V=96, d=128, H=2, NL=2, FF=256, L=32)
BLOCK_FILE_LEAVES = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "cross_attn.in_proj_weight",
                     "cross_attn.out_proj.weight", "ff.0.weight", "ff.3.weight")


def grad_file(name: str) -> str:
    """The fixture file that holds parameter `name`'s full gradient."""
    for i in range(DEC["NL"]):
        if any(name == f"blocks.{i}.{leaf}" for leaf in BLOCK_FILE_LEAVES):
            return f"lengths_grads_b{i}"
    return "lengths_grads_time" if name.startswith("time_") else "lengths"


def lengths_inputs():
    """(wave [3, 16000] ~ 0.1 N(0, 1), R [3, L, V] ~ N(0, 1)) from names alone."""
    wave = 0.1 * math.sqrt(16000.0) * pcg_array("lengths.wave", (3, 16000))
    R = math.sqrt(DEC["L"] * DEC["V"]) * pcg_array("lengths.R", (3, DEC["L"], DEC["V"]))
    return torch.from_numpy(wave.astype(np.float32)), torch.from_numpy(R.astype(np.float32))


def _patch_from_pretrained(geometry: dict, prefix: str):
    from transformers import WavLMConfig, WavLMModel
    import models.acoustic_encoder as ae

    def fake_from_pretrained(name, *a, **k):
        m = WavLMModel(WavLMConfig(**geometry))
        load_pcg(m, prefix=prefix)
        return m

    ae.WavLMModel.from_pretrained = staticmethod(fake_from_pretrained)


def main():
    from models.acoustic_encoder import AcousticEncoder
    from models.denoise_decoder import DenoisingTransformerDecoder

    wave, R = lengths_inputs()
    lengths = torch.tensor(LENGTHS)
    out = dict(lengths=lengths)
    for tag, geom, d_model in (("tiny", SMALL_WAVLM, 64), ("base", {}, 128)):
        _patch_from_pretrained(geom, "backbone.")
        enc = AcousticEncoder(wavlm_name="local-" + tag, d_model=d_model, pooling="mean")
        load_pcg(enc, prefix="")
        enc.eval()
        with torch.no_grad():
            feats, mask, pooled = enc(wave, lengths)
        out[tag + "_feats"], out[tag + "_mask"], out[tag + "_pooled"] = feats, mask, pooled

    V, d, H, NL, FF, L = (DEC[k] for k in ("V", "d", "H", "NL", "FF", "L"))
    dec = DenoisingTransformerDecoder(vocab_size=V, d_model=d, nhead=H, num_layers=NL, dim_ff=FF, dropout=0.0,
                                      max_len=1024, pad_id=0)
    load_pcg(dec, prefix="dec.", pad_row=("tok_emb.weight", 0))
    dec.train()
    r = np.random.Generator(np.random.PCG64(21))
    xt = torch.from_numpy(r.integers(1, V, size=(3, L))).long()
    xt[1, 25:] = 0
    xt[2, 9:] = 0
    t = torch.tensor([3, 170, 42])
    cond = out["base_feats"].clone()
    c_mask = out["base_mask"].clone()
    logits = dec(xt, t, cond, x_mask=None, c_mask=c_mask)
    (logits * R).sum().backward()
    out.update(dec_xt=xt, dec_t=t, dec_logits=logits.detach())
    files = {"lengths": {}}
    for n, p in dec.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out["g_sum." + n] = g.sum()
        out["g_sq." + n] = (g.double() ** 2).sum()
        if g.numel() <= 70000:
            files.setdefault(grad_file(n), {})["g." + n] = g
    files["lengths"].update(out)
    for fname, d_ in files.items():
        arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d_.items()}
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **arrs)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)
    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    print({k: v.shape for k, v in arrs.items() if not k.startswith("g")})
    print("masks kept:", {k: arrs[k].sum(1).tolist() for k in ("tiny_mask", "base_mask")})


if __name__ == "__main__":
    main()
