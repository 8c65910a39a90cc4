"""GPU parity of the 32x32x16-MFMA decoder attention kernels (csrc/attn7.hip) against float64 references with the
oracle's dropout mask (contract v2), at the shapes the decoder runs (keep bits written ahead by
fddm_attn_drop_bits, as models/denoise_decoder.py does) and at ragged / masked / extreme-score edge cases.

Tolerance: bf16 inputs and outputs, fp32 softmax statistics -> 2e-2 of the reference's max magnitude (tests/
test_gpu_kernels.py TOL for bf16); the LSE within LSE_ATOL absolute (natural-log units) where the row is finite.
fwd7 multiplies Q by scale*log2(e) once and rounds that to bf16 (one rounding of 2^-9 relative per element instead
of rounding the scores), so a score of magnitude |s| carries up to ~|s|*2^-9 of extra error; over randn inputs at
d=64 the LSE moves by up to ~2e-3, hence 4e-3 (the outputs stay within the bf16 2e-2 bar).
Reference: models/denoise_decoder.py:129-130,164,169-176 (nn.MultiheadAttention, key_padding_mask, dropout on
the probabilities).
"""
import functools

import pytest
import torch

from helpers import FWD8_GUARD_GEOMS, close, fwd8_fast_path_rowsum, fwd8_guard_cases, fwd8_guard_inputs
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu
LSE_ATOL = 4e-3

dev = torch.device("cuda:0")
bf = torch.bfloat16


def ops():
    from fddm_hip import ops as o
    return o


def _ref(q, k, v, keep, p, seed, stream):
    """q [B,H,Lq,64] float64 ... -> O [B,H,Lq,64], lse [B,H,Lq] (natural log, of the scaled scores)."""
    B, H, Lq, _ = q.shape
    Lk = k.shape[2]
    s = (q @ k.transpose(-1, -2)) / 8.0
    if keep is not None:
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if p > 0:
        m = O.attn_dropout_keep(seed, stream, B, H, Lq, Lk, p).double()
        pr = pr * m / (1 - p)
    return pr @ v, lse


def _run(B, H, Lq, Lk, keep, p, q, k, v, do=None, seed=5, stream=9, family="auto"):
    o = ops()
    D = H * 64
    to = lambda x: x.to(dev, bf).reshape(-1, D).contiguous()  # noqa: E731
    qd, kd, vd = to(q), to(k), to(v)
    od = torch.empty(B * Lq, D, device=dev, dtype=bf)
    lse = torch.empty(B * H, Lq, device=dev)
    kk = keep.to(dev).to(torch.uint8) if keep is not None else None
    db = None
    old = o.attn_force_kernels(family)    # the producer writes the selected family's storage layout
    try:
        if p > 0:
            db = o.drop_bits(B, H, Lq, Lk, dev).view(1, -1)
            o.attn_drop_bits(db, 1, B, H, Lq, Lk, p, seed, stream, 0)
            db = db.view(-1)
        o.attn_fwd(qd, kd, vd, od, lse, B, H, Lq, Lk, key_keep=kk, drop_p=p, seed=seed, rng_stream=stream, dbits=db,
                   bits_ready=db is not None)
        grads = None
        if do is not None:
            dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
            o.attn_bwd(qd, kd, vd, od, to(do), lse, dq, dk, dv, B, H, Lq, Lk, key_keep=kk, drop_p=p, seed=seed,
                       rng_stream=stream, dbits=db)
            grads = (dq, dk, dv)
    finally:
        o.attn_force_kernels(old)
    torch.cuda.synchronize()
    return od, lse, grads


def _heads(x, B, H):
    return x.to(bf).double().view(B, -1, H, 64).transpose(1, 2)


def _back(t):
    B, H, L, _ = t.shape
    return t.transpose(1, 2).reshape(B * L, H * 64)


SHAPES = [  # (B, H, Lq, Lk, key-padding mask, dropout p)
    (2, 3, 256, 256, True, 0.1),     # decoder self-attention (C2 geometry per head)
    (2, 3, 256, 499, False, 0.1),    # cross-attention, 10 s of audio (ragged last key tile)
    (2, 2, 512, 512, True, 0.1),     # C4 self
    (2, 2, 512, 499, False, 0.1),    # C4 cross
    (2, 3, 130, 70, True, 0.0),      # ragged queries and keys, no dropout
    (1, 2, 40, 1000, False, 0.1),    # long key range, a partial query block
    (2, 3, 129, 257, True, 0.1),
    (3, 1, 64, 64, False, 0.0),
    (2, 2, 200, 200, True, 0.1),
    (1, 1, 1, 1, False, 0.1),        # one query, one key
    (2, 2, 33, 5, True, 0.1),        # a partial 32-query group, five keys
    (1, 2, 96, 1024, True, 0.1),     # the longest key range of the 32x32x16 family (16 tiles, mask on every one)
    (1, 2, 96, 1025, False, 0.1),    # one key past it: the round-4 family takes the launch
]


FWD8_EXTRA = [  # forced fwd8 only
    (2, 2, 600, 300, True, 0.1),     # three workgroups per (b, h), the last one partial
    (1, 1, 32, 32, False, 0.1),      # exactly one half-tile: the pipeline-end row-sum MFMA carries the whole sum
    (1, 2, 64, 33, False, 0.0),      # one key in the second half
]


def _families(shapes, extra8=()):
    """Each shape under the default dispatch ("auto": fwd7 at these small B*H; it keeps the shape-only test id) and
    with fwd8 forced (attn8.hip; not past Lk 1024, where the launch leaves the 32x32x16 family whatever is forced),
    plus the fwd8-only shapes."""
    name = lambda s: "-".join(str(x) for x in s)  # noqa: E731
    return ([pytest.param("auto", *s, id=name(s)) for s in shapes] +
            [pytest.param("fwd8", *s, id="fwd8-" + name(s)) for s in list(shapes) + list(extra8) if s[3] <= 1024])


@pytest.mark.parametrize("family,B,H,Lq,Lk,masked,p", _families(SHAPES, FWD8_EXTRA))
def test_attn7_forward_matches_float64(family, B, H, Lq, Lk, masked, p):
    D = H * 64
    gen = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q, k, v = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk))
    keep = None
    if masked:
        keep = torch.ones(B, Lk, dtype=torch.bool)
        keep[B - 1, max(1, Lk - 9):] = False
        if Lk > 3:
            keep[0, 3] = False
        if Lk > 130:
            keep[B - 1, 64:128] = False  # a whole 64-key tile of padding inside the range (skipped tile)
    od, lse, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family=family)
    ref, rlse = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, p, 5, 9)
    close(od.float(), _back(ref), rtol=2e-2, what="attn7 out")
    # with few keys the LSE is close to one score, whose error is the bf16 rounding of Q' (|s| 2^-9), not averaged
    smax = (_heads(q, B, H) @ _heads(k, B, H).transpose(-1, -2)).abs().max().item() / 8.0
    close(lse.view(B, H, Lq), rlse, rtol=0, atol=max(LSE_ATOL, 2.0 ** -8 * smax), what="attn7 lse")


@pytest.mark.parametrize("family,B,H,Lq,Lk,masked,p",
                         _families([SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[6], SHAPES[9], SHAPES[10], SHAPES[11],
                                    SHAPES[12]], FWD8_EXTRA))
def test_attn7_forward_then_backward_matches_float64(family, B, H, Lq, Lk, masked, p):
    """The backward kernels read the forward's LSE and the same keep words: gradients vs float64 autograd. Under
    "fwd8" the backward consumes fwd8's LSE and bf16 output, as the training step does."""
    D = H * 64
    gen = torch.Generator().manual_seed(7 + Lq + Lk)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = None
    if masked:
        keep = torch.ones(B, Lk, dtype=torch.bool)
        keep[B - 1, max(1, Lk - 9):] = False
    od, lse, (dq, dk, dv) = _run(B, H, Lq, Lk, keep, p, q, k, v, do, family=family)
    qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
    ref, _ = _ref(qr, kr, vr, keep, p, 5, 9)
    ref.backward(_heads(do, B, H))
    close(od.float(), _back(ref.detach()), rtol=2e-2, what="out")
    # delta = rowsum(dO O) comes from the stored bf16 O: dS carries ~2^-9 |dO| |O| absolute error even where the
    # exact gradient vanishes (one key: softmax = 1, dQ = dK = 0 exactly), hence an absolute floor of 1e-2
    close(dq.float(), _back(qr.grad), rtol=6e-2, atol=1e-2, what="dq")
    close(dk.float(), _back(kr.grad), rtol=6e-2, atol=1e-2, what="dk")
    close(dv.float(), _back(vr.grad), rtol=6e-2, atol=1e-2, what="dv")


@pytest.mark.parametrize("B,H,Lq,Lk,masked,p", [(2, 3, 256, 256, True, 0.1), (2, 2, 300, 200, True, 0.1),
                                                (1, 2, 1, 256, False, 0.0), (2, 1, 65, 17, True, 0.1),
                                                (1, 1, 200, 240, False, 0.1), (2, 3, 256, 499, False, 0.1),
                                                (2, 2, 100, 300, True, 0.1), (1, 2, 256, 512, True, 0.0),
                                                (2, 1, 64, 257, False, 0.1), (2, 2, 200, 512, True, 0.1),
                                                (2, 2, 300, 400, True, 0.1)])  # the last: Lq > 256 -> the pair
def test_attn7_fused_backward_matches_float64_and_split_pair(B, H, Lq, Lk, masked, p):
    """Lk <= 256, or Lq <= 256 and Lk <= 512 (two key passes, the dQ partial kept in the workspace between them): the
    fused backward (bwdf7, one launch per (b, h) computing P and dP once, dQ from the dS^T image in LDS; the default)
    against float64 autograd, and against the split pair (dq7 + dkv7, family "nofused") on the same forward — two
    bf16 roundings of one float64 result (P, dS rounded to bf16 in both, sums in other orders)."""
    D = H * 64
    gen = torch.Generator().manual_seed(17 + Lq + Lk)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = None
    if masked:
        keep = torch.ones(B, Lk, dtype=torch.bool)
        keep[B - 1, max(1, Lk - 9):] = False
        if Lk > 130:
            keep[0, 64:128] = False  # a padded 64-key tile inside the range: two waves with no valid key
    _, _, gf = _run(B, H, Lq, Lk, keep, p, q, k, v, do, family="auto")
    _, _, gs = _run(B, H, Lq, Lk, keep, p, q, k, v, do, family="nofused")
    qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
    ref, _ = _ref(qr, kr, vr, keep, p, 5, 9)
    ref.backward(_heads(do, B, H))
    for n, a_, b_, r in zip(("dq", "dk", "dv"), gf, gs, (qr.grad, kr.grad, vr.grad)):
        close(a_.float(), _back(r), rtol=6e-2, atol=1e-2, what=f"fused {n}")
        close(a_.float(), b_.float(), rtol=2e-2, atol=1e-2, what=f"fused vs split {n}")


@pytest.mark.parametrize("family,Lk", [pytest.param("auto", 256, id="256"), pytest.param("auto", 499, id="499"),
                                       pytest.param("fwd8", 256, id="fwd8-256"),
                                       pytest.param("fwd8", 499, id="fwd8-499")])
def test_attn7_rescale_path_with_growing_scores(family, Lk):
    """Scores that grow along the keys (every 32-key half-tile exceeds the running maximum by far more than the
    2^8 rescale threshold) exercise the slow path on every half-tile; scores that fall along the keys keep the first
    half's reference. Forward against float64. The gradients at these scores (up to ~100, |K| up to ~25 per element)
    are bf16-limited in any kernel (dQ = scale sum_k dS K amplifies the bf16 rounding of P and dS by |K|): measured
    ~0.2-0.36 of max|dQ| for both families, so the backward is held to the round-4 family's error on the same inputs
    (within 1.5x) instead of to float64.
    Under "fwd8" (fixed reference per chain, no rescale branch) the rising ramp ends ~2^130 above the first half-tile's
    reference: the fast path's row sums overflow and every wave goes through the guard to the online-softmax fallback;
    the falling ramp stays on the fast path (the first half-tile holds the maximum). Same checks, same bounds."""
    B, H, Lq = 2, 2, 128
    D = H * 64
    gen = torch.Generator().manual_seed(11)
    u = torch.randn(64, generator=gen)
    u = u / u.norm()
    q = (u * 4.0).repeat(B, Lq, H) + 0.05 * torch.randn(B, Lq, D, generator=gen)
    ramp = torch.linspace(0.0, 200.0, Lk)   # +6 to +13 scaled score units per 32-key half-tile
    for sign in (1.0, -1.0):
        k = (sign * ramp[None, :, None] * u.repeat(H)[None, None, :]).expand(B, Lk, D).contiguous()
        k = k + 0.05 * torch.randn(B, Lk, D, generator=gen)
        v = torch.randn(B, Lk, D, generator=gen)
        do = torch.randn(B, Lq, D, generator=gen)
        qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
        ref, rlse = _ref(qr, kr, vr, None, 0.1, 5, 9)
        ref.backward(_heads(do, B, H))
        rg = [_back(x.grad) for x in (qr, kr, vr)]
        err = {}
        for fam in (family, "v6"):
            od, lse, grads = _run(B, H, Lq, Lk, None, 0.1, q, k, v, do, family=fam)
            if fam == family:
                close(od.float(), _back(ref.detach()), rtol=2e-2, what=f"out (sign {sign})")
                # the bf16 rounding of the pre-scaled Q moves scores by up to ~|s| 2^-9, as a bf16 rounding of the
                # scores themselves would (torch's bf16 bmm): a tolerance relative to the LSE
                close(lse.view(B, H, Lq), rlse.detach(), rtol=2.0 ** -9, atol=LSE_ATOL, what=f"lse (sign {sign})")
            err[fam] = [(g.float().cpu().double() - r).abs().max().item() / r.abs().max().item()
                        for g, r in zip(grads, rg)]
        for n, a_, b_ in zip(("dq", "dk", "dv"), err[family], err["v6"]):
            assert a_ <= 1.5 * b_ + 2e-2, f"{n} (sign {sign}): attn7 rel err {a_:.3g} vs round-4 family {b_:.3g}"


@pytest.mark.parametrize("family", ["auto", "fwd8"])
def test_attn7_fully_masked_rows_give_nan_like_softmax(family):
    """A batch whose keys are all padding: softmax over all -inf is NaN in the reference (torch), and so is every
    output and LSE of that batch here; the other batch is unaffected. In fwd8 such a batch entry still walks its
    tiles (nact > 0) and ends with row sums of 0: the guard trips, the fallback's sums are 0 again -> NaN rows."""
    B, H, Lq, Lk = 2, 2, 96, 140
    D = H * 64
    gen = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk))
    keep = torch.ones(B, Lk, dtype=torch.bool)
    keep[1] = False
    od, lse, _ = _run(B, H, Lq, Lk, keep, 0.1, q, k, v, family=family)
    o = od.float().view(B, Lq, D)
    assert torch.isnan(o[1]).all() and torch.isnan(lse.view(B, H, Lq)[1]).all()
    ref, _ = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, 0.1, 5, 9)
    close(o[0], _back(ref)[: Lq].view(Lq, D), rtol=2e-2, what="unmasked batch")


@pytest.mark.parametrize("B,H,Lq,Lk,masked,p", [SHAPES[0], SHAPES[2], SHAPES[5]])
def test_attn7_agrees_with_round4_kernel(B, H, Lq, Lk, masked, p):
    """The 32x32x16 forward and the round-4 16x16x32 forward (fwd6, keep words read the same way) on the same
    inputs: both bf16 roundings of one float64 result, so within twice the per-kernel tolerance of each other."""
    D = H * 64
    gen = torch.Generator().manual_seed(99)
    q, k, v = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk))
    keep = None
    if masked:
        keep = torch.ones(B, Lk, dtype=torch.bool)
        keep[0, Lk - 30:] = False
    o7, l7, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="auto")
    o6, l6, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="v6")
    close(o7.float(), o6.float(), rtol=2e-2, what="fwd7 vs fwd6")
    close(l7, l6, rtol=0, atol=LSE_ATOL, what="lse fwd7 vs fwd6")


def test_attn7_forward_records_bits_when_not_ready():
    """attn_fwd with a keep-bit buffer that the producer has not filled (a standalone call, not the decoder's path):
    the 32x32x16 family writes the site's masks itself first, and the backward reads them."""
    o = ops()
    B, H, Lq, Lk, p = 2, 2, 96, 140, 0.1
    D = H * 64
    gen = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    to = lambda x: x.to(dev, bf).reshape(-1, D).contiguous()  # noqa: E731
    od = torch.empty(B * Lq, D, device=dev, dtype=bf)
    lse = torch.empty(B * H, Lq, device=dev)
    db = o.drop_bits(B, H, Lq, Lk, dev)
    o.attn_fwd(to(q), to(k), to(v), od, lse, B, H, Lq, Lk, drop_p=p, seed=5, rng_stream=9, dbits=db)
    dq, dk, dv = (torch.empty(B * L, D, device=dev, dtype=bf) for L in (Lq, Lk, Lk))
    o.attn_bwd(to(q), to(k), to(v), od, to(do), lse, dq, dk, dv, B, H, Lq, Lk, drop_p=p, seed=5, rng_stream=9,
               dbits=db)
    torch.cuda.synchronize()
    qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
    ref, _ = _ref(qr, kr, vr, None, p, 5, 9)
    ref.backward(_heads(do, B, H))
    close(od.float(), _back(ref.detach()), rtol=2e-2, what="out")
    close(dk.float(), _back(kr.grad), rtol=6e-2, what="dk")


def test_decoder_long_audio_families_agree():
    """The whole bf16 decoder (training mode, dropout 0.1, keep bits written ahead by the producer for every block's
    two attention sites) with a condition longer than the 32x32x16 family takes (S = 1100 frames: the cross sites run
    on the round-4 kernels and read the round-4 words, the self sites on attn7 with layout v3): logits and every
    parameter gradient agree with the all-round-4 run on the same inputs and seeds (bf16 roundings of one result)."""
    from fddm_hip import runtime as rt
    from test_gpu_models import make_decoder
    o = ops()
    B, L, S, V, d, H, NL, FF = 2, 64, 1100, 300, 128, 2, 2, 256
    gen = torch.Generator().manual_seed(41)
    xt = torch.randint(1, V, (B, L), generator=gen)
    xt[1, 50:] = 0
    t = torch.tensor([3, 17])
    cond = torch.randn(B, S, d, generator=gen)
    R = torch.randn(B, L, V, generator=gen)
    res = {}
    for fam in ("auto", "v6"):
        old = o.attn_force_kernels(fam)
        try:
            with rt.use_precision("bf16"):
                torch.manual_seed(3)
                dec = make_decoder(V, d, H, NL, FF, dropout=0.1)
                dec.train()
                rt.reseed(11)
                logits = dec(xt.to(dev), t.to(dev), cond.to(dev), x_mask=(xt != 0).to(dev))
                (logits.float() * R.to(dev)).sum().backward()
                torch.cuda.synchronize()
                res[fam] = (logits.float().cpu(), {n: p.grad.float().cpu() for n, p in dec.named_parameters()
                                                   if p.grad is not None})
        finally:
            o.attn_force_kernels(old)
    close(res["auto"][0], res["v6"][0], rtol=3e-2, what="logits auto vs round-4")
    assert res["auto"][1].keys() == res["v6"][1].keys()
    for n in res["auto"][1]:
        close(res["auto"][1][n], res["v6"][1][n], rtol=6e-2, atol=1e-3, what=f"grad {n}")


@pytest.mark.parametrize("family,p", [pytest.param("auto", 0.0, id="0.0"), pytest.param("auto", 0.1, id="0.1"),
                                      pytest.param("fwd8", 0.0, id="fwd8-0.0"),
                                      pytest.param("fwd8", 0.1, id="fwd8-0.1")])
def test_attn7_first_half_tile_masked_with_very_negative_scores(family, p):
    """a query whose first 32 keys are all padding keeps m = -inf after its first half-tile; with every
    valid score far below the running reference (here ~ -130 in log2 units) the fast path's exponentials underflow
    to 0 and the row sum stays 0 unless the slow path runs while no finite reference exists. Output and LSE must be
    finite and match float64 (torch's softmax is finite there). Under "fwd8" the chains' reference stays 0, every
    exponential underflows, the row sums are 0 and the guard sends every wave to the fallback."""
    B, H, Lq, Lk = 1, 2, 64, 160
    D = H * 64
    gen = torch.Generator().manual_seed(13)
    u = torch.randn(64, generator=gen)
    u = u / u.norm()
    q = (u * 30.0).repeat(B, Lq, H) + 0.05 * torch.randn(B, Lq, D, generator=gen)
    k = (-u * 30.0).repeat(B, Lk, H) + 0.05 * torch.randn(B, Lk, D, generator=gen)   # q.k / 8 ~ -112
    v = torch.randn(B, Lk, D, generator=gen)
    keep = torch.ones(B, Lk, dtype=torch.bool)
    keep[:, :32] = False
    od, lse, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family=family)
    assert torch.isfinite(od.float()).all() and torch.isfinite(lse).all()
    ref, rlse = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, p, 5, 9)
    close(od.float(), _back(ref), rtol=2e-2, what="out")
    close(lse.view(B, H, Lq), rlse, rtol=2.0 ** -8, atol=LSE_ATOL, what="lse")


@pytest.mark.parametrize("B,H,Lq,Lk,masked,p", [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4], SHAPES[6], SHAPES[9],
                                                SHAPES[10], SHAPES[11], (2, 2, 600, 300, True, 0.1)])
def test_fwd8_agrees_with_fwd7(B, H, Lq, Lk, masked, p):
    """The two-chain forward (attn8.hip fwd8, forced; the default where its grid loads no CU more than fwd7's) against
    the one-chain fwd7 on the same inputs and keep bits:
    same score operands (pre-scaled Q'), different reference handling (fwd8 fixes each chain's reference at its first
    half-tile), so both are bf16 roundings of one float64 result."""
    D = H * 64
    gen = torch.Generator().manual_seed(123 + Lq + Lk)
    q, k, v = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk))
    keep = None
    if masked:
        keep = torch.ones(B, Lk, dtype=torch.bool)
        keep[B - 1, max(1, Lk - 9):] = False
        if Lk > 130:
            keep[0, 64:128] = False
    o8, l8, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="fwd8")
    o7, l7, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="fwd7")
    close(o8.float(), o7.float(), rtol=2e-2, what="fwd8 vs fwd7")
    close(l8, l7, rtol=0, atol=LSE_ATOL, what="lse fwd8 vs fwd7")


@functools.lru_cache(maxsize=None)
def _guard_case(geom, kind, c):
    """One guard case's inputs, the emulated fast-path verdict per (b, h) and the float64 reference: built once,
    shared by the families, never modified."""
    B, H, Lq, Lk, p, _, _ = FWD8_GUARD_GEOMS[geom]
    q, k, v, keep, rows = fwd8_guard_inputs(geom, kind, c)
    qh, kh = (x.to(bf).view(B, -1, H, 64).transpose(1, 2) for x in (q, k))
    trips = [[fwd8_fast_path_rowsum(qh[b, h], kh[b, h], None if keep is None else keep[b])[1].nonzero().flatten()
              .tolist() for h in range(H)] for b in range(B)]
    ref, rlse = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, p, 5, 9)
    return q, k, v, keep, rows, trips, ref, rlse


@pytest.mark.parametrize("family", ["fwd8", "fwd7"])
@pytest.mark.parametrize("geom,kind,c,cls", fwd8_guard_cases())
def test_fwd8_guard_and_fallback_match_float64(geom, kind, c, cls, family):
    """fwd8's guard on the final row sums and the online-softmax fallback behind it (attn8.hip, `redo`), forward
    only, output and LSE of every row against float64 with the oracle's dropout mask. The inputs
    (helpers.fwd8_guard_inputs) put designated query rows at, or past, the edges of what the fixed per-chain
    reference can represent; the CPU emulation of the fast path's row sum proves first which rows trip the guard:
    exactly the designated ones ("trips") or none ("inside": the fast path at the top / bottom of its range, 2^4
    inside the bound by tests/test_cpu_attn_inputs.py). One tripped row sends its whole wave (64 queries, both
    chains) through the fallback, so the other rows of those waves are recomputed there as well, while waves
    without a designated row stay on the fast path in the same workgroup.
    Proof that the fallback ran, for "rise" 12 and "fall" 25: the fast path's float32 sum of a designated row is
    +inf, respectively exactly 0 (every exponential underflows), so its output would be 0 / NaN and its LSE inf /
    NaN; a finite output and LSE matching float64 at those rows cannot have come from it.
    Geometries and the template builds (DM = dropout, MK = key mask: 0 none, 1 ragged Lk, 2 mask bytes) they reach:
    a: Lq 256 Lk 256 p 0.1, last 9 keys padded, rows 37 (wave 0, chain B) and 200 (wave 3, chain A): DM 1 MK 2,
       waves 1 and 2 on the fast path; b: Lq 130 Lk 200 p 0.1, row 129 (wave 2, chain A; chain B lies past Lq, its
       query group is clamped in the fallback's keep-dword read; ragged last key tile clamped in its staging): DM 1
       MK 1 (rise) / MK 2 (fall); c: Lq 600 Lk 512 p 0, rows 5 and 599 (first and last workgroup, eight tiles): DM 0
       MK 0 (rise) / MK 2 (fall); d: B 2 H 3 Lq 64 Lk 96 p 0.1, every row designated (no fast-path wave left): DM 1
       MK 1 (rise) / MK 2 (fall).
    fwd7 runs the same inputs as the control (its online softmax is the algorithm the fallback claims to be); it is
    not an oracle. Tolerances are the file's: 2e-2 of the reference maximum, LSE rtol 2^-8 / LSE_ATOL (scores up to
    ~130: the bf16 rounding of Q' moves them by ~|s| 2^-9)."""
    B, H, Lq, Lk, p, _, _ = FWD8_GUARD_GEOMS[geom]
    q, k, v, keep, rows, trips, ref, rlse = _guard_case(geom, kind, c)
    want = sorted(rows) if cls == "trips" else []
    assert all(t == want for tb in trips for t in tb), (want, trips)
    assert torch.isfinite(ref).all() and torch.isfinite(rlse).all()
    od, lse, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family=family)
    assert torch.isfinite(od.float()).all() and torch.isfinite(lse).all()
    close(od.float(), _back(ref), rtol=2e-2, what=f"{family} out")
    close(lse.view(B, H, Lq), rlse, rtol=2.0 ** -8, atol=LSE_ATOL, what=f"{family} lse")


def _per_head_close(od, lse, ref, rlse, B, H, Lq, what):
    """Every (b, h) on its own: output within 2e-2 of that head's reference maximum, LSE within LSE_ATOL (a block
    remap that swaps heads passes no per-tensor bound by luck of equal magnitudes, but fails these)."""
    o = od.float().cpu().double().view(B, Lq, H, 64).transpose(1, 2)
    ls = lse.cpu().double().view(B, H, Lq)
    assert torch.isfinite(o).all() and torch.isfinite(ls).all(), f"{what}: non-finite values"
    err, tol = (o - ref).abs().amax((-1, -2)), 2e-2 * ref.abs().amax((-1, -2))
    bad = (err > tol).nonzero().tolist()
    assert not bad, (f"{what}: out of tolerance at (b, h) {bad[:8]}: err {err.max().item():.3e}, "
                     f"tol {tol.min().item():.3e}")
    lerr = (ls - rlse).abs().amax(-1)
    bad = (lerr > LSE_ATOL).nonzero().tolist()
    assert not bad, f"{what}: lse out of tolerance at (b, h) {bad[:8]}: err {lerr.max().item():.3e}"


def _grid_inputs(B, H, Lq, Lk, seed):
    """randn k, v and 0.5 randn q, a key mask on the last batch. The half-scale queries keep the worst of ~65 000 rows
    inside LSE_ATOL by the number formats alone: with 96 keys a row's LSE follows its few largest scores, and at unit
    scale the bf16 rounding of Q' (shared by fwd7 and fwd8) moves the worst row's LSE by 3.7e-3 on the CPU, 4.5e-3
    with a bf16 rounding of P before the row sum — no room under 4e-3 for any kernel; at half scale those figures are
    0.7e-3 and 1.1e-3."""
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, L, H * 64, generator=gen) for L in (Lq, Lk, Lk))
    q = 0.5 * q
    keep = torch.ones(B, Lk, dtype=torch.bool)
    keep[B - 1, Lk - 9:] = False
    return q, k, v, keep


def test_auto_takes_fwd8_at_one_workgroup_per_cu():
    """The benchmark-like grid: B * H = the device's CU count at Lq 256 (one fwd8 workgroup per (b, h) and CU; fwd7
    would need two per CU), keep bits from the producer, a key mask on the last batch. The default dispatch must pick
    fwd8 (bit-identical to the forced fwd8 run, not to the forced fwd7 run), and every (b, h) must match float64:
    xcd_tile's block remap at a grid of that many blocks would show as whole heads swapped."""
    nh = torch.cuda.get_device_properties(0).multi_processor_count
    B, H = (nh // 8, 8) if nh % 8 == 0 else (nh, 1)
    Lq, Lk, p = 256, 96, 0.1
    q, k, v, keep = _grid_inputs(B, H, Lq, Lk, 77)
    oa, la, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="auto")
    o8, l8, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="fwd8")
    o7, l7, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="fwd7")
    assert torch.equal(oa, o8) and torch.equal(la, l8), "auto is not fwd8 at one workgroup per CU"
    assert not torch.equal(oa, o7), "auto is bit-identical to fwd7"
    ref, rlse = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, p, 5, 9)
    _per_head_close(oa, la, ref, rlse, B, H, Lq, "auto")


def test_fwd8_block_remap_remainder_grid():
    """Seven blocks (B * H = 7, one workgroup each): xcd_tile's remainder branch r = n & 7 with q = n >> 3 = 0. Forced
    fwd8 against float64, per head."""
    B, H, Lq, Lk, p = 1, 7, 200, 96, 0.1
    q, k, v, keep = _grid_inputs(B, H, Lq, Lk, 78)
    od, lse, _ = _run(B, H, Lq, Lk, keep, p, q, k, v, family="fwd8")
    ref, rlse = _ref(_heads(q, B, H), _heads(k, B, H), _heads(v, B, H), keep, p, 5, 9)
    _per_head_close(od, lse, ref, rlse, B, H, Lq, "fwd8")
