"""DenoisingTransformerDecoder on MI355X (drop-in for models/denoise_decoder.py of the reference).

Same constructor signature, forward signature, submodule names and state_dict keys as the reference
(models/denoise_decoder.py:25-295), so reference checkpoints load unchanged. The compute is one fused
autograd Function per DecoderBlock (fddm_hip.functions.DecoderBlockFn) over libfddm_hip kernels.

Deviations (documented in DESIGN.md): only pos_emb_type="rope" is built (the only type the reference's
train.py constructs, train.py:517-526); head_dim <= 64 (the attention kernels are built for 64-wide heads;
smaller heads run on zero-padded slots, fddm_hip.ops.attn_fwd); the gradient w.r.t. `cond` is not
produced (the encoder is frozen and its projection is never optimised, train.py:543).
"""
from __future__ import annotations

import math
from typing import Literal, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from fddm_hip import functions as FN
from fddm_hip import runtime as rt
from fddm_hip.ops import attn_drop_bits as ops_attn_drop_bits
from fddm_hip.ops import drop_words
from fddm_hip.ops import linear as ops_linear
from fddm_hip.ops import key_extent as ops_key_extent
from fddm_hip.ops import rows_mean as ops_rows_mean
from fddm_hip.ops import rows_mean_masked as ops_rows_mean_masked


class RoPEEmbedding(nn.Module):
    """models/denoise_decoder.py:25-53 — keeps the `inv_freq` buffer; tables are cached per length."""

    def __init__(self, d_model: int, base: float = 10000.0):
        super().__init__()
        self.d_model = d_model
        self.base = base
        self.register_buffer("inv_freq", 1.0 / (base ** (torch.arange(0, d_model, 2).float() / d_model)))

    def forward(self, seq_len: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        return rt.rope_tables(seq_len, self.inv_freq, device)

    @staticmethod
    def apply_rotary_pos_emb(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
        """Reference formula (denoise_decoder.py:42-53), kept for API compatibility."""
        x1, x2 = x[..., ::2], x[..., 1::2]
        return torch.cat([x1 * cos[..., ::2] - x2 * sin[..., 1::2], x1 * sin[..., ::2] + x2 * cos[..., 1::2]], -1)


class FiLMLayer(nn.Module):
    """models/denoise_decoder.py:74-89; the affine itself is fused into the LN2 kernel."""

    def __init__(self, d_model: int, cond_dim: int):
        super().__init__()
        self.scale_proj = nn.Linear(cond_dim, d_model)
        self.shift_proj = nn.Linear(cond_dim, d_model)

    def params(self, cond_pooled: torch.Tensor):
        return self.scale_proj(cond_pooled), self.shift_proj(cond_pooled)

    def forward(self, x: torch.Tensor, cond: torch.Tensor) -> torch.Tensor:
        scale, shift = self.params(cond)
        return x * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)


class SinusoidalTimeEmbedding(nn.Module):
    """models/denoise_decoder.py:92-119 (tiny [B, d] MLP; torch ops)."""

    def __init__(self, d_model: int, max_steps: int = 10000):
        super().__init__()
        self.d_model = d_model
        self.max_steps = max_steps
        self.mlp = nn.Sequential(nn.Linear(d_model, d_model * 4), nn.SiLU(), nn.Linear(d_model * 4, d_model))

    def forward(self, t: torch.Tensor) -> torch.Tensor:
        if t.dim() == 0:
            t = t[None]
        half = self.d_model // 2
        freqs = torch.exp(torch.linspace(math.log(1.0), math.log(self.max_steps), half, device=t.device) * (-1))
        args = t.float().unsqueeze(1) * freqs.unsqueeze(0)
        emb = torch.cat([torch.sin(args), torch.cos(args)], dim=1)
        if self.d_model % 2 == 1:
            emb = F.pad(emb, (0, 1))
        return self.mlp(emb)


class _MHAParams(nn.Module):
    """Parameter holder with nn.MultiheadAttention's state_dict names (in_proj_weight, in_proj_bias,
    out_proj.weight, out_proj.bias) and its default initialisation."""

    def __init__(self, d_model: int, nhead: int, dropout: float):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = d_model, nhead, dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class DecoderBlock(nn.Module):
    """models/denoise_decoder.py:122-192."""

    def __init__(self, d_model: int, nhead: int, dim_ff: int, dropout: float = 0.1, use_film: bool = True,
                 pos_emb_type: str = "rope"):
        super().__init__()
        if pos_emb_type != "rope" or not use_film:
            raise NotImplementedError("only the reference's default block (rope + FiLM) is built")
        if d_model % nhead or d_model // nhead > 64:
            raise NotImplementedError("head_dim = d_model / nhead must divide d_model and be <= 64 on this build")
        self.use_film, self.pos_emb_type = use_film, pos_emb_type
        self.nhead, self.p = nhead, dropout
        self.self_attn = _MHAParams(d_model, nhead, dropout)
        self.cross_attn = _MHAParams(d_model, nhead, dropout)
        self.film_layer = FiLMLayer(d_model, d_model)
        self.ff = nn.Sequential(nn.Linear(d_model, dim_ff), nn.GELU(), nn.Dropout(dropout), nn.Linear(dim_ff, d_model))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.drop = nn.Dropout(dropout)

    def block_params(self):
        return (self.self_attn.in_proj_weight, self.self_attn.in_proj_bias, self.self_attn.out_proj.weight,
                self.self_attn.out_proj.bias, self.cross_attn.in_proj_weight, self.cross_attn.in_proj_bias,
                self.cross_attn.out_proj.weight, self.cross_attn.out_proj.bias, self.ff[0].weight, self.ff[0].bias,
                self.ff[3].weight, self.ff[3].bias, self.norm1.weight, self.norm1.bias, self.norm2.weight,
                self.norm2.bias, self.norm3.weight, self.norm3.bias)

    def run(self, x, xT, cT, key_keep, film, B, L, S, layer, seed, cos, sin, kv=None, bits=None, xr=None,
            handoff=None, c_keep=None, c_len=None):
        """film = (scale, shift, (dscale, dshift) accumulators or None) from DenoisingTransformerDecoder's
        conditioning Function; kv = this block's precomputed cross-attention K|V [B*S, 2d] (strided view) or None;
        bits = (self, cross) attention-dropout keep-bit words already written for this block, or None;
        xr = rope(x) already written by the previous block's LN3, or None; handoff = a dict in which this block's LN3
        leaves rope(its output) under "xr" for the next block (bf16), or None; c_keep / c_len = the condition's
        key-padding mask (u8 [B, S]) and its key extents for the cross-attention (:169-174), or None."""
        fscale, fshift, gfilm = film
        p = self.p if self.training else 0.0
        meta = (B, L, S, self.nhead, layer, p, seed, cos, sin, gfilm, kv, bits, xr, handoff, c_keep, c_len)
        return FN.DecoderBlockFn.apply(x, xT, cT, key_keep, fscale, fshift, meta, *self.block_params())


class DenoisingTransformerDecoder(nn.Module):
    """models/denoise_decoder.py:194-295."""

    def __init__(self, vocab_size: int, d_model: int = 768, nhead: int = 12, num_layers: int = 6, dim_ff: int = 2048,
                 dropout: float = 0.1, max_len: int = 2048, pad_id: int = 0,
                 pos_emb_type: Literal["rope", "sinusoidal", "learned"] = "rope", use_film: bool = True,
                 rope_base: float = 10000.0) -> None:
        super().__init__()
        if pos_emb_type != "rope":
            raise NotImplementedError("pos_emb_type != 'rope' is out of scope (train.py always uses rope)")
        self.pos_emb_type, self.use_film = pos_emb_type, use_film
        self.tok_emb = nn.Embedding(vocab_size, d_model, padding_idx=pad_id)
        self.pos_emb = RoPEEmbedding(d_model, base=rope_base)
        self.time_emb = SinusoidalTimeEmbedding(d_model)
        self.time_proj = nn.Linear(d_model, d_model)
        self.blocks = nn.ModuleList([DecoderBlock(d_model, nhead, dim_ff, dropout, use_film, pos_emb_type)
                                     for _ in range(num_layers)])
        self.head = nn.Linear(d_model, vocab_size)
        self.pad_id = pad_id
        self.d_model, self.nhead = d_model, nhead

    def forward(self, xt: torch.Tensor, t: torch.Tensor, cond: torch.Tensor, x_mask: Optional[torch.Tensor] = None,
                c_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, L = xt.shape
        S = cond.shape[1]
        dev = xt.device
        cd = rt.compute_dtype()
        # conditioning (:272-274 time bias, :185 pooled condition -> FiLM of every block) in one Function
        c_keep = c_len = None
        with torch.no_grad():
            cc = cond.detach()
            cc = cc if cc.is_contiguous() else cc.contiguous()
            if c_mask is None:
                pooled = ops_rows_mean(cc)                                          # (:185) mean over S, f32
            else:
                # (:173, :181-183) the condition's key-padding mask for every block's cross-attention, its key extents
                # (once per forward, no host sync) and the masked pooled mean (count not clamped, as the reference)
                c_keep = c_mask.to(dev)
                c_keep = c_keep.contiguous().view(torch.uint8) if c_keep.dtype == torch.bool else \
                    (c_keep != 0).contiguous().view(torch.uint8)
                c_len = ops_key_extent(c_keep)
                pooled = ops_rows_mean_masked(cc, c_keep, clamp=False)
        nb = len(self.blocks)
        gbuf = torch.zeros(2 * nb, B, self.d_model, device=dev, dtype=torch.float32)
        te = self.time_emb
        film_params = [q for blk in self.blocks for lin in (blk.film_layer.scale_proj, blk.film_layer.shift_proj)
                       for q in (lin.weight, lin.bias)]
        outs = FN.CondFn.apply(t, pooled, gbuf, self.d_model, te.max_steps, te.mlp[0].weight, te.mlp[0].bias,
                               te.mlp[2].weight, te.mlp[2].bias, self.time_proj.weight, self.time_proj.bias,
                               *film_params)
        t_bias, films = outs[0], outs[1:]
        if t_bias.shape[0] != B:
            t_bias = t_bias.expand(B, -1)
        x, xT = FN.EmbedFn.apply(xt, self.tok_emb.weight, t_bias, self.pad_id)      # (:254)
        if x_mask is None:
            x_mask = xt != self.pad_id                                             # (:277-278)
        key_keep = x_mask.contiguous().view(torch.uint8) if x_mask.dtype == torch.bool else \
            x_mask.to(torch.uint8).contiguous()
        with torch.no_grad():
            c = cond.detach()
            cT = (c if c.dtype == cd else c.to(cd)).reshape(B * S, -1).contiguous()
        cos, sin = self.pos_emb(L, dev)
        seed = rt.next_seed()
        kv_all = self._cross_kv(cT)
        bits = self._drop_bits(B, L, S, seed, dev)
        xr = None
        for i, blk in enumerate(self.blocks):
            film = (films[2 * i], films[2 * i + 1], (gbuf[2 * i], gbuf[2 * i + 1]))
            kv = None if kv_all is None else kv_all[:, 2 * self.d_model * i: 2 * self.d_model * (i + 1)]
            bi = None if bits is None else (bits[0][i], bits[1][i])
            handoff = {} if i + 1 < len(self.blocks) else None
            x, xT = blk.run(x, xT, cT, key_keep, film, B, L, S, i, seed, cos, sin, kv, bi, xr, handoff, c_keep,
                            c_len)
            xr = None if handoff is None else handoff.get("xr")
        logits = FN.HeadFn.apply(x, xT, self.head.weight, self.head.bias)           # (:286)
        return logits.view(B, L, -1)

    @torch.no_grad()
    def _drop_bits(self, B, L, S, seed, dev):
        """The attention-probability dropout keep bits of every block's two attention sites (rng streams 6i+1 self,
        6i+3 cross; RNG contract v2, oracle.attn_dropout_keep), written by two launches ahead of the blocks in the
        storage layout the attention kernels read (fddm_attn_drop_words: layout v3, one lane mask per score-MFMA
        register), so the forward and backward read them instead of drawing them. bf16 training only (the fp32 parity kernels draw their own)."""
        p = self.blocks[0].p if (self.training and len(self.blocks)) else 0.0
        if p <= 0 or rt.compute_dtype() != torch.bfloat16:
            return None
        H, nb = self.nhead, len(self.blocks)
        ws = drop_words(B, H, L, L)
        wc = drop_words(B, H, L, S)
        bs = torch.empty(nb, ws, device=dev, dtype=torch.int64)
        bc = torch.empty(nb, wc, device=dev, dtype=torch.int64)
        ops_attn_drop_bits(bs, nb, B, H, L, L, p, seed, 1, 6)
        ops_attn_drop_bits(bc, nb, B, H, L, S, p, seed, 3, 6)
        return bs, bc

    @torch.no_grad()
    def _cross_kv(self, cT):
        """The cross-attention K|V projections of the acoustic condition for ALL blocks as one GEMM
        ([B*S, d] x [NL*2d, d]^T): they depend only on the condition and the blocks' weights, not on the decoder
        state, so NL launches of [B*S, 2d] (one 256^2-tile round each at C2) become one launch of NL x the work.
        Block i attends to columns [2d*i, 2d*(i+1)) (row stride NL*2d); the K|V weight gradients stay in each
        block's backward (cond carries no gradient)."""
        if len(self.blocks) < 2:
            return None
        d = self.d_model
        w = torch.cat([rt.wt(blk.cross_attn.in_proj_weight)[d:] for blk in self.blocks])
        b = torch.cat([blk.cross_attn.in_proj_bias.detach()[d:] for blk in self.blocks])
        return ops_linear(cT, w, b, out_dtype=rt.compute_dtype())

    def grad_ready_order(self):
        """Parameters in the order backward finalises their gradients: head, the blocks from last to first (their
        own weights; FiLM projections are reduced by the conditioning Function at the very end), then the rest.
        The grad arena is laid out in this order so the DP all-reduce overlaps backward (fddm_hip.dist)."""
        out = [self.head.weight, self.head.bias]
        for blk in reversed(self.blocks):
            out += [p for n, p in blk.named_parameters() if not n.startswith("film_layer.")]
        seen = set(id(p) for p in out)
        return out + [p for p in self.parameters() if id(p) not in seen]

    @torch.no_grad()
    def predict_x0(self, xt, t, cond, x_mask=None, c_mask=None) -> torch.Tensor:
        return self.forward(xt, t, cond, x_mask, c_mask).softmax(dim=-1)
