"""GPU parity of the variable-length path: key extents, the length-bounded attention builds (csrc/attn7.hip KX),
the masked pooled mean and row zeroing, and the modules that use them (AcousticEncoder lengths, WavLM attention_mask,
decoder c_mask, train._encoded, the sampler).

References: float64 softmax attention over the same bf16 inputs with the oracle's dropout mask (as
tests/test_gpu_attn7.py, whose error measure and bounds for masked cases are used: outputs 2e-2 of the reference
maximum, LSE 4e-3 absolute, gradients 6e-2 with an absolute floor of 1e-2); the reference's own fixture
(tests/golden/lengths.npz) at 1e-4 in the fp32 parity mode; the torch restatement of tests/test_cpu_lengths.py (pinned
to that fixture) at other shapes, with the bf16 bounds tests/test_gpu_models.py uses for the unmasked modules
(encoder 5e-2, decoder 3e-2, gradients three times that).
"""
import functools

import pytest
import torch

from helpers import SMALL_WAVLM, T, close, load, wavlm_sd
from oracle import fddm_oracle as O
from test_cpu_lengths import (LENGTHS_DEC, key_extent_ref, lengths_inputs, load_lengths, masked_acoustic_encoder,
                              masked_decoder_forward)

pytestmark = pytest.mark.gpu
LSE_ATOL = 4e-3

dev = torch.device("cuda:0")
bf = torch.bfloat16


def ops():
    from fddm_hip import ops as o
    return o


def _rt():
    from fddm_hip import runtime as rt
    return rt


# ------------------------------------------------------------------------------------------------ key extent
def _extent_masks(Lk):
    """B = 5: all kept, none kept, a hole in the middle, a single trailing key, right-padded at half."""
    keep = torch.zeros(5, Lk, dtype=torch.uint8)
    keep[0] = 1
    keep[2, : max(1, (3 * Lk) // 4)] = 1
    keep[2, Lk // 4: Lk // 2] = 0
    keep[3, Lk - 1] = 1
    keep[4, : max(1, Lk // 2)] = 3          # any non-zero byte keeps
    return keep


@pytest.mark.parametrize("Lk", [1, 63, 64, 65, 499])
def test_key_extent_equals_torch_expression(Lk):
    keep = _extent_masks(Lk)
    got = ops().key_extent(keep.to(dev))
    assert got.dtype == torch.int32 and got.shape == (5,)
    assert torch.equal(got.cpu(), key_extent_ref(keep))
    # a row start that is not 4-byte aligned (the byte path) and one that is (Lk 64: the dword path) both occur
    # above; a view at an odd offset exercises the byte path at every Lk
    buf = torch.zeros(5 * Lk + 1, dtype=torch.uint8, device=dev)
    buf[1:] = keep.reshape(-1).to(dev)
    assert torch.equal(ops().key_extent(buf[1:].view(5, Lk)).cpu(), key_extent_ref(keep))


# ------------------------------------------------------------------------------- length-bounded attention
def _ref(q, k, v, keep, p, seed, stream):
    """q [B,H,Lq,64] float64 ... -> O, lse (as tests/test_gpu_attn7.py _ref)."""
    B, H, Lq, _ = q.shape
    Lk = k.shape[2]
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * O.attn_dropout_keep(seed, stream, B, H, Lq, Lk, p).double() / (1 - p)
    return pr @ v, lse


def _heads(x, B, H):
    return x.to(bf).double().view(B, -1, H, 64).transpose(1, 2)


def _back(t):
    B, H, L, _ = t.shape
    return t.transpose(1, 2).reshape(B * L, H * 64)


def _run(B, H, Lq, Lk, keep, p, q, k, v, do, *, kx, family="auto", dtype=bf, seed=5, stream=9):
    """Forward + backward through ops.attn_fwd / attn_bwd with the key_keep mask, and with key_len when kx."""
    o = ops()
    D = q.shape[-1]
    to = lambda x: x.to(dev, dtype).reshape(-1, D).contiguous()  # noqa: E731
    qd, kd, vd = to(q), to(k), to(v)
    od = torch.empty(B * Lq, D, device=dev, dtype=dtype)
    lse = torch.empty(B * H, Lq, device=dev)
    kk = keep.to(dev).to(torch.uint8).contiguous()
    kl = o.key_extent(kk) if kx else None
    db = None
    old = o.attn_force_kernels(family)
    try:
        if p > 0 and dtype == bf:
            db = o.drop_bits(B, H, Lq, Lk, dev).view(1, -1)
            o.attn_drop_bits(db, 1, B, H, Lq, Lk, p, seed, stream, 0)
            db = db.view(-1)
        o.attn_fwd(qd, kd, vd, od, lse, B, H, Lq, Lk, key_keep=kk, drop_p=p, seed=seed, rng_stream=stream, dbits=db,
                   bits_ready=db is not None, key_len=kl)
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        dk.fill_(7.0)      # rows past an extent must be written (zeros), not left
        dv.fill_(7.0)
        o.attn_bwd(qd, kd, vd, od, to(do), lse, dq, dk, dv, B, H, Lq, Lk, key_keep=kk, drop_p=p, seed=seed,
                   rng_stream=stream, dbits=db, key_len=kl)
    finally:
        o.attn_force_kernels(old)
    torch.cuda.synchronize()
    return od, lse, dq, dk, dv


KX_CASES = {  # name -> (B, H, Lk, extents): an entry on each side of each 64-key tile boundary, a single key
    "lk200": (6, 2, 200, [200, 1, 63, 64, 65, 129]),
    "lk300": (4, 2, 300, [300, 257, 256, 70]),      # bwdf7 with two, two, one and one live key passes
}


@functools.lru_cache(maxsize=None)
def _kx_case(name, Lq, p, hole):
    """Inputs and the float64 reference of one case: built once, shared by the kernel families, never modified."""
    B, H, Lk, ext = KX_CASES[name]
    D = H * 64
    gen = torch.Generator().manual_seed(1000 * Lq + Lk + int(p * 100))
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = torch.arange(Lk)[None, :] < torch.tensor(ext)[:, None]
    if hole:      # holes inside the extents: part of a tile, a whole 64-key tile, and the key before the last
        keep[0, 10:13] = False
        keep[0, 64:128] = False
        keep[B - 1, ext[B - 1] - 2] = False
    qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
    ref, rlse = _ref(qr, kr, vr, keep, p, 5, 9)
    ref.backward(_heads(do, B, H))
    smax = (qr.detach() @ kr.detach().transpose(-1, -2)).abs().max().item() / 8.0
    return (q, k, v, do, keep, _back(ref.detach()), rlse.detach(), _back(qr.grad), _back(kr.grad), _back(vr.grad),
            smax)


def _check_kx(name, Lq, p, family, hole):
    B, H, Lk, ext = KX_CASES[name]
    q, k, v, do, keep, ref, rlse, rdq, rdk, rdv, smax = _kx_case(name, Lq, p, hole)
    od, lse, dq, dk, dv = _run(B, H, Lq, Lk, keep, p, q, k, v, do, kx=True, family=family)
    close(od.float(), ref, rtol=2e-2, what="kx out")
    close(lse.view(B, H, Lq), rlse, rtol=0, atol=max(LSE_ATOL, 2.0 ** -8 * smax), what="kx lse")
    close(dq.float(), rdq, rtol=6e-2, atol=1e-2, what="kx dq")
    close(dk.float(), rdk, rtol=6e-2, atol=1e-2, what="kx dk")
    close(dv.float(), rdv, rtol=6e-2, atol=1e-2, what="kx dv")
    dkb, dvb = dk.float().view(B, Lk, -1), dv.float().view(B, Lk, -1)
    for b, e in enumerate(ext):
        assert (dkb[b, e:] == 0).all() and (dvb[b, e:] == 0).all(), f"dK / dV rows past extent {e} of entry {b}"
    # the key_keep-only path on the same inputs: the skipped tiles contribute exact zeros
    po, pl, pdq, pdk, pdv = _run(B, H, Lq, Lk, keep, p, q, k, v, do, kx=False, family=family)
    for n, a_, b_ in (("out", od, po), ("lse", lse, pl), ("dq", dq, pdq), ("dk", dk, pdk), ("dv", dv, pdv)):
        assert torch.equal(a_, b_), (f"{n}: key_len path differs from the key_keep path, max "
                                     f"{(a_.float() - b_.float()).abs().max().item():.3e}")


@pytest.mark.parametrize("family", ["auto", "nofused"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Lq", [40, 129])
@pytest.mark.parametrize("name", list(KX_CASES))
def test_kx_attention_matches_float64_and_key_keep_path(name, Lq, p, family):
    """fwd7 + bwdf7 ("auto": Lq <= 256 and Lk <= 512 take the fused backward, one or two key passes) and fwd7 + dq7 +
    dkv7 ("nofused") with key extents, right-padded masks."""
    _check_kx(name, Lq, p, family, hole=False)


@pytest.mark.parametrize("family", ["auto", "nofused"])
@pytest.mark.parametrize("name", list(KX_CASES))
def test_kx_attention_mask_with_holes_inside_the_extent(name, family):
    """The byte mask still applies inside the bound: holes (three keys, a whole tile, the key before the last)."""
    _check_kx(name, 129, 0.1, family, hole=True)


def test_kx_long_queries_take_the_split_pair():
    """Lq > 256: the default backward is dq7 + dkv7 (three query workgroups per head, two key workgroups of which
    one lies past most extents)."""
    B, H, Lq, Lk, ext = 3, 2, 300, 200, [200, 100, 3]
    D = H * 64
    gen = torch.Generator().manual_seed(77)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = torch.arange(Lk)[None, :] < torch.tensor(ext)[:, None]
    od, lse, dq, dk, dv = _run(B, H, Lq, Lk, keep, 0.1, q, k, v, do, kx=True)
    qr, kr, vr = (_heads(x, B, H).requires_grad_(True) for x in (q, k, v))
    ref, rlse = _ref(qr, kr, vr, keep, 0.1, 5, 9)
    ref.backward(_heads(do, B, H))
    close(od.float(), _back(ref.detach()), rtol=2e-2, what="out")
    for n, a_, r in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        close(a_.float(), _back(r), rtol=6e-2, atol=1e-2, what=n)
    for b, e in enumerate(ext):
        assert (dk.float().view(B, Lk, -1)[b, e:] == 0).all() and (dv.float().view(B, Lk, -1)[b, e:] == 0).all()


@pytest.mark.parametrize("family", ["auto", "nofused"])
def test_kx_fully_masked_entry(family):
    """An entry with no kept key (extent 0) between two ordinary ones: its output and LSE rows are NaN, as on the
    key_keep path and in torch's softmax over all -inf; its dK / dV rows past the first 128 keys (the key-owned
    workgroup of dkv7 that holds the one live tile; bwdf7: past the first 64) are zeros (the key_keep path leaves NaN
    there: the one case in which the two paths differ); the other entries get the bits of
    the key_keep path and match float64."""
    B, H, Lq, Lk, ext = 3, 2, 70, 200, [150, 0, 200]
    D = H * 64
    gen = torch.Generator().manual_seed(91)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = torch.arange(Lk)[None, :] < torch.tensor(ext)[:, None]
    od, lse, dq, dk, dv = _run(B, H, Lq, Lk, keep, 0.1, q, k, v, do, kx=True, family=family)
    po, pl, pdq, pdk, pdv = _run(B, H, Lq, Lk, keep, 0.1, q, k, v, do, kx=False, family=family)
    rows = lambda x, L: x.float().view(B, L, D)  # noqa: E731
    assert torch.isnan(rows(od, Lq)[1]).all() and torch.isnan(lse.view(B, H, Lq)[1]).all()
    assert torch.isnan(rows(po, Lq)[1]).all() and torch.isnan(pl.view(B, H, Lq)[1]).all()
    assert (rows(dk, Lk)[1, 128:] == 0).all() and (rows(dv, Lk)[1, 128:] == 0).all()
    for b in (0, 2):
        for n, a_, b_, L in (("out", od, po, Lq), ("dq", dq, pdq, Lq), ("dk", dk, pdk, Lk), ("dv", dv, pdv, Lk)):
            assert torch.equal(rows(a_, L)[b], rows(b_, L)[b]), f"{n} of entry {b}"
        assert torch.equal(lse.view(B, H, Lq)[b], pl.view(B, H, Lq)[b])
    live = torch.tensor([0, 2])
    sub = lambda x: x.view(B, -1, D)[live]  # noqa: E731
    qr, kr, vr = (_heads(sub(x), 2, H).requires_grad_(True) for x in (q, k, v))
    ref, _ = _ref(qr, kr, vr, keep[live], 0.0, 5, 9)
    od0, _, dq0, dk0, dv0 = _run(B, H, Lq, Lk, keep, 0.0, q, k, v, do, kx=True, family=family)
    ref.backward(_heads(sub(do), 2, H))
    close(rows(od0, Lq)[live].reshape(-1, D), _back(ref.detach()), rtol=2e-2, what="out of the live entries")
    close(rows(dk0, Lk)[live].reshape(-1, D), _back(kr.grad), rtol=6e-2, atol=1e-2, what="dk of the live entries")
    close(rows(dv0, Lk)[live].reshape(-1, D), _back(vr.grad), rtol=6e-2, atol=1e-2, what="dv of the live entries")
    close(rows(dq0, Lq)[live].reshape(-1, D), _back(qr.grad), rtol=6e-2, atol=1e-2, what="dq of the live entries")


@pytest.mark.parametrize("arm", ["fp32", "v6", "head_dim32", "lk1100"])
def test_key_len_is_ignored_where_no_bounded_kernel_runs(arm):
    """fp32 parity mode, the 16x16x32 family, zero-padded small heads and Lk > 1024: the bound is ignored and the
    key_keep path runs — the same kernels on the same inputs, so the same bits."""
    B, H, Lq, Lk, ext = 2, 2, 40, (1100 if arm == "lk1100" else 150), [150, 66]
    dh = 32 if arm == "head_dim32" else 64
    D = H * dh
    gen = torch.Generator().manual_seed(31)
    q, k, v, do = (torch.randn(B, L, D, generator=gen) for L in (Lq, Lk, Lk, Lq))
    keep = torch.arange(Lk)[None, :] < torch.tensor(ext)[:, None]
    kw = dict(dtype=torch.float32 if arm == "fp32" else bf, family="v6" if arm == "v6" else "auto")
    a = _run(B, H, Lq, Lk, keep, 0.0, q, k, v, do, kx=True, **kw)
    b = _run(B, H, Lq, Lk, keep, 0.0, q, k, v, do, kx=False, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_kx_entries_require_mask_and_extent_together():
    o = ops()
    q = torch.zeros(64, 64, device=dev, dtype=bf)
    out, lse = torch.empty_like(q), torch.empty(1, 64, device=dev)
    keep = torch.ones(1, 64, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        o.attn_fwd(q, q, q, out, lse, 1, 1, 64, 64, key_len=o.key_extent(keep))
    with pytest.raises(ValueError):
        o.attn_fwd(q, q, q, out, lse, 1, 1, 64, 64, key_keep=keep, key_len=torch.ones(1, device=dev))   # not int32


# ------------------------------------------------------------------------------- WavLM REL attention
def test_wavlm_rel_attention_with_mask_and_extent_matches_float64():
    """The `x` gate mode of the gated relative-position attention (fwd7's REL build) with a key-padding mask and
    extents on both sides of a tile boundary and a 7-key entry: S 149 (3 s), three key tiles of which two, one, one
    are live. float64: score = q.k / 8 + gate(x) * table[h][k - q + S - 1], gate as HF modeling_wavlm.py:171-176."""
    o = ops()
    B, H, S, ext = 3, 2, 149, [149, 64, 7]
    E = H * 64
    gen = torch.Generator().manual_seed(40)
    x = torch.randn(B * S, E, generator=gen).to(bf)
    qkv = torch.randn(B * S, 3 * E, generator=gen).to(bf)
    W = torch.randn(8, 64, generator=gen) * 0.2
    bias = torch.randn(8, generator=gen) * 0.1
    cst = torch.rand(H, generator=gen) + 0.5
    table = torch.randn(H, 2 * S - 1, generator=gen)
    gw = torch.cat([W[:4].sum(0), W[4:].sum(0), bias[:4].sum().reshape(1), bias[4:].sum().reshape(1)]).contiguous()
    keep = torch.arange(S)[None, :] < torch.tensor(ext)[:, None]
    kk = keep.to(dev).to(torch.uint8).contiguous()
    qd = qkv.to(dev)
    out = torch.empty(B * S, E, device=dev, dtype=bf)
    o.attn_fwd_relgate_x(qd, qd[:, E:], qd[:, 2 * E:], out, x.to(dev), gw.to(dev), cst.to(dev), table.to(dev), B, H, S,
                         key_keep=kk, key_len=o.key_extent(kk))
    plain = torch.empty_like(out)
    gate_d = o.wavlm_gate(x.to(dev), W.to(dev), bias.to(dev), cst.to(dev), B, S, H)
    o.attn_fwd(qd, qd[:, E:], qd[:, 2 * E:], plain, None, B, H, S, S, gate=gate_d, table=table.to(dev), key_keep=kk)
    torch.cuda.synchronize()
    xh = x.double().view(B, S, H, 64).transpose(1, 2)
    pre = xh @ W.double().T + bias.double()                                   # [B,H,S,8]
    ga, gb = torch.sigmoid(pre[..., :4].sum(-1)), torch.sigmoid(pre[..., 4:].sum(-1))
    gate = ga * (gb * cst.double().view(1, H, 1) - 1.0) + 2.0                  # [B,H,S]
    idx = torch.arange(S)[None, :] - torch.arange(S)[:, None] + S - 1          # [q, k]
    rb = table.double()[:, idx]                                               # [H,S,S]
    qh, kh, vh = (qkv[:, i * E:(i + 1) * E].double().view(B, S, H, 64).transpose(1, 2) for i in range(3))
    s = qh @ kh.transpose(-1, -2) / 8.0 + gate[..., None] * rb[None]
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    ref = _back(torch.softmax(s, -1) @ vh)
    close(out.float(), ref, rtol=2e-2, what="masked REL attention")
    close(plain.float(), ref, rtol=2e-2, what="general entry with key_keep")


# ------------------------------------------------------------------------------- masked mean / row zeroing
def _row_masks(B, S):
    keep = torch.zeros(B, S, dtype=torch.uint8)
    keep[0] = 1
    keep[1, : S // 2] = 1
    keep[2, 0] = 1
    keep[3, 5:9] = 1
    keep[3, S - 1] = 1          # row 4 (if any) keeps nothing
    return keep


@pytest.mark.parametrize("d", [128, 512, 768])
@pytest.mark.parametrize("dt", [torch.float32, bf])
def test_rows_mean_masked_matches_float64(dt, d):
    """f32 sums of at most 49 rows: within 1e-6 relative of float64 (the bound of the unmasked rows_mean test); bf16
    inputs are promoted exactly, so the same bound holds against the float64 mean of the bf16 values. A zero-count row
    is 0 under the clamp flag and NaN without it (the reference's unclamped 0 / 0)."""
    B, S = 5, 49
    gen = torch.Generator().manual_seed(d)
    x = torch.randn(B, S, d, generator=gen).to(dt)
    x[1, S // 2:] = float("nan")        # padded rows are not read
    keep = _row_masks(B, S)
    xd = x.double().nan_to_num(0.0)
    cnt = keep.double().sum(1, keepdim=True)
    want = (xd * keep.double()[..., None]).sum(1) / cnt.clamp(min=1)
    got_c = ops().rows_mean_masked(x.to(dev), keep.to(dev), clamp=True)
    got_u = ops().rows_mean_masked(x.to(dev), keep.to(dev), clamp=False)
    assert got_c.dtype == torch.float32 and got_c.shape == (B, d)
    close(got_c, want, rtol=1e-6, what="clamped masked mean")
    close(got_u[:4], want[:4], rtol=1e-6, what="unclamped masked mean")
    assert torch.isnan(got_u[4]).all() and (got_c[4] == 0).all()
    # all kept: the unmasked kernel's result, bit for bit (same slices, same order)
    assert torch.equal(ops().rows_mean_masked(x[:1].to(dev), keep[:1].to(dev)), ops().rows_mean(x[:1].to(dev)))


@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("dt", [torch.float32, bf])
def test_rows_zero_masked_is_exact(dt, E):
    B, S = 5, 49
    gen = torch.Generator().manual_seed(E + 1)
    x = torch.randn(B * S, E, generator=gen).to(dt)
    keep = _row_masks(B, S).reshape(-1)
    x[keep == 0, 3] = float("nan")      # whatever the padded rows held
    xd = x.to(dev).clone()
    ops().rows_zero_masked(xd, keep.to(dev))
    got = xd.cpu()
    assert torch.equal(got[keep != 0], x[keep != 0]) and (got[keep == 0] == 0).all()


# ------------------------------------------------------------------------------------------ module level
def _encoder(geom, d_model, pooling="mean"):
    from models.acoustic_encoder import AcousticEncoder
    enc = AcousticEncoder(wavlm_name=dict(geom), d_model=d_model, pooling=pooling)
    sd = enc.state_dict()
    for n, v in wavlm_sd(O.wavlm_geometry(**geom), d_model).items():
        assert n in sd, n
        sd[n] = v
    enc.load_state_dict(sd)
    return enc.to(dev).eval()


def _decoder(dropout=0.0, V=None):
    from test_gpu_models import make_decoder
    V = V or LENGTHS_DEC["V"]
    return make_decoder(V, LENGTHS_DEC["d"], LENGTHS_DEC["H"], LENGTHS_DEC["NL"], LENGTHS_DEC["FF"], dropout=dropout)


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 5e-2)])
@pytest.mark.parametrize("tag,geom,d_model", [("tiny", SMALL_WAVLM, 64), ("base", {}, 128)])
def test_encoder_with_lengths_matches_reference_fixture(tag, geom, d_model, prec, tol):
    """AcousticEncoder(wave, lengths), pooling="mean": lengths 16000 / 9000 / 500 of 3 x 1 s (a full entry, 27 HF
    frames, a single HF frame). fp32 parity mode within 1e-4 of the reference, bf16 within the unmasked encoder's
    5e-2; the returned mask (the reference's ceil(len / 320) count) is equal, not close."""
    g = load("lengths")
    wave, _ = lengths_inputs()
    with _rt().use_precision(prec):
        enc = _encoder(geom, d_model)
        feats, mask, pooled = enc(wave.to(dev), T(g["lengths"]).to(dev))
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), T(g[tag + "_mask"]))
    close(feats.float(), g[tag + "_feats"], rtol=tol, what=f"{prec} {tag} feats")
    close(pooled, g[tag + "_pooled"], rtol=tol, what=f"{prec} {tag} pooled")


def test_wavlm_attention_mask_matches_restatement_at_two_tiles_bf16():
    """2 s (S = 99: two key tiles) with lengths on both sides of the tile boundary of the HF frame count (64 frames
    <-> 20560 samples): the bf16 backbone through WavLMModel.forward(input_values, attention_mask) against the fp32
    restatement, the unmasked encoder's bf16 bound."""
    geo = O.wavlm_geometry(**SMALL_WAVLM)
    gen = torch.Generator().manual_seed(19)
    wave = 0.1 * torch.randn(3, 32000, generator=gen)
    lengths = torch.tensor([32000, 20559, 20560])
    sd = wavlm_sd(geo, 64)
    with torch.no_grad():
        ref, mask, pooled = masked_acoustic_encoder(sd, wave, lengths, geo, 64)
    with _rt().use_precision("bf16"):
        enc = _encoder(SMALL_WAVLM, 64)
        am = torch.arange(32000)[None, :] < lengths[:, None]
        assert enc.backbone.feature_mask(am.to(dev), 99).sum(1).tolist() == [99, 63, 64]
        feats, fm, pl = enc(wave.to(dev), lengths.to(dev))
        hid = enc.backbone(wave.to(dev), attention_mask=am.to(dev)).last_hidden_state
        assert torch.equal(enc.project(hid), feats)
    assert torch.equal(fm.cpu(), mask)
    close(feats.float(), ref, rtol=5e-2, what="bf16 masked encoder, 2 tiles")
    close(pl, pooled, rtol=5e-2, what="bf16 masked pooled")


# bf16: the parameters tests/test_gpu_models.py checks in its bf16 decoder test (at three times the logits bound), and
# the cross-attention and feed-forward weights of both blocks, which the mask reaches first
BF16_GRADS = ("blocks.0.self_attn.in_proj_weight", "blocks.1.ff.0.weight", "head.weight", "tok_emb.weight",
              "blocks.0.norm2.weight", "blocks.1.film_layer.scale_proj.weight", "time_proj.weight",
              "blocks.0.cross_attn.in_proj_weight", "blocks.0.cross_attn.out_proj.weight",
              "blocks.1.cross_attn.in_proj_weight", "blocks.1.cross_attn.out_proj.weight", "blocks.0.ff.0.weight",
              "blocks.0.ff.3.weight", "blocks.1.ff.3.weight")


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_decoder_with_c_mask_matches_reference_fixture(prec, tol):
    """Logits and gradients against the reference's fixture: fp32 parity mode every parameter at 1e-4, bf16 the
    BF16_GRADS subset at three times the logits bound."""
    g = load_lengths()
    _, R = lengths_inputs()
    with _rt().use_precision(prec):
        dec = _decoder()
        dec.train()
        logits = dec(T(g["dec_xt"]).to(dev), T(g["dec_t"]).to(dev), T(g["base_feats"]).to(dev),
                     c_mask=T(g["base_mask"]).to(dev))
        close(logits.float(), g["dec_logits"], rtol=tol, what=f"{prec} logits")
        (logits.float() * R.to(dev)).sum().backward()
    for n, p in dec.named_parameters():
        if prec == "fp32":
            close(p.grad, g["g." + n], rtol=tol, atol=1e-6, what=f"fp32 grad {n}")
            close((p.grad.double() ** 2).sum(), g["g_sq." + n], rtol=2e-4, atol=1e-12, what="grad sq " + n)
        elif n in BF16_GRADS:
            close(p.grad, g["g." + n], rtol=3 * tol, atol=1e-6, what=f"bf16 grad {n}")


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_decoder_c_mask_with_dropout_matches_restatement(prec, tol, monkeypatch):
    """Dropout 0.1 at every site (the oracle's _Dropper under the shared RNG contract), S = 70 (two key tiles) with
    extents 70, 64 and 5; bounds of test_gpu_models.test_decoder_dropout_matches_oracle."""
    rt = _rt()
    V, H, NL, B, L, S, d = 304, LENGTHS_DEC["H"], LENGTHS_DEC["NL"], 3, 24, 70, LENGTHS_DEC["d"]
    gen = torch.Generator().manual_seed(3)
    xt = torch.randint(1, V, (B, L), generator=gen)
    xt[1, 20:] = 0
    t = torch.tensor([5, 150, 77])
    cond = torch.randn(B, S, d, generator=gen)
    R = torch.randn(B, L, V, generator=gen)
    c_mask = torch.arange(S)[None, :] < torch.tensor([70, 64, 5])[:, None]
    monkeypatch.setattr(rt, "next_seed", lambda: 777)
    with rt.use_precision(prec):
        dec = _decoder(dropout=0.1, V=V)
        dec.train()
        logits = dec(xt.to(dev), t.to(dev), cond.to(dev), c_mask=c_mask.to(dev))
        (logits * R.to(dev)).sum().backward()
    sd = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in dec.named_parameters()}
    ref = masked_decoder_forward(sd, xt, t, cond, None, c_mask, H, NL, dropout=0.1, seed=777)
    (ref * R).sum().backward()
    close(logits, ref.detach(), rtol=tol, what=f"{prec} logits")
    for n in ("blocks.0.self_attn.in_proj_weight", "blocks.0.cross_attn.in_proj_weight", "blocks.1.ff.0.weight",
              "head.weight", "tok_emb.weight", "blocks.0.norm2.weight", "blocks.1.film_layer.scale_proj.weight",
              "time_proj.weight"):
        close(dict(dec.named_parameters())[n].grad, sd[n].grad, rtol=3 * tol, atol=1e-6, what=f"{prec} grad {n}")


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-6), ("bf16", 2e-2)])
def test_all_true_c_mask_equals_no_mask(prec, tol):
    """fp32: the same kernels with an all-true mask, within 1e-6. bf16: the mask selects fwd7's bounded build where
    c_mask=None may take fwd8 — the fwd7-vs-fwd8 bound of tests/test_gpu_attn7.py (2e-2)."""
    g = load("lengths")
    xt, t, cond = T(g["dec_xt"]).to(dev), T(g["dec_t"]).to(dev), T(g["base_feats"]).to(dev)
    with _rt().use_precision(prec):
        dec = _decoder()
        dec.eval()
        with torch.no_grad():
            a = dec(xt, t, cond, c_mask=torch.ones(3, cond.shape[1], dtype=torch.bool, device=dev))
            b = dec(xt, t, cond)
    close(a.float(), b.float(), rtol=tol, atol=1e-6, what=f"{prec} all-true c_mask vs None")


def test_encoded_passes_lengths_and_keeps_the_graph_for_plain_batches(monkeypatch):
    """train._encoded: a batch's third element reaches the encoder as `lengths` (c_mask = its frame mask, features of
    the eager masked forward); batches without one still go through the graph-replayed encoder (c_mask None): the
    graph runner is called for exactly the plain batch, the module's forward for exactly the two with lengths."""
    import train as T_
    from fddm_hip.graphs import GraphedEncoder
    calls = {"graph": 0, "eager": []}
    graph_run = GraphedEncoder.run

    def counted_run(self, *a, **k):
        calls["graph"] += 1
        return graph_run(self, *a, **k)

    monkeypatch.setattr(GraphedEncoder, "run", counted_run)

    class Opt:
        param_groups = [{"params": []}]

    gen = torch.Generator().manual_seed(4)
    waves = [0.1 * torch.randn(2, 16000, generator=gen) for _ in range(3)]
    x0 = torch.zeros(2, 8, dtype=torch.long)
    lens = torch.tensor([16000, 7000])
    loader = [(waves[0], x0, lens), (waves[1], x0), (waves[2], x0, lens)]
    with _rt().use_precision("bf16"):
        enc = _encoder(SMALL_WAVLM, 64, pooling="none")
        assert GraphedEncoder.supported(enc)
        hook = enc.register_forward_pre_hook(lambda mod, args: calls["eager"].append(len(args) > 1 and args[1] is not None))
        got = [(c.float().clone(), None if m is None else m.clone()) for c, m, _ in T_._encoded(enc, loader, dev, Opt())]
        torch.cuda.synchronize()
        hook.remove()
        assert calls["graph"] == 1 and calls["eager"] == [True, True], calls
        want = [enc(waves[0].to(dev), lens.to(dev)), enc(waves[1].to(dev)), enc(waves[2].to(dev), lens.to(dev))]
    for (c, m), (rc, rm, _) in zip(got, want):
        assert (m is None) == (rm is None) and (m is None or torch.equal(m, rm))
        assert torch.equal(c, rc.float())
    assert got[0][1].sum(1).tolist() == [49, 22]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sampler_threads_c_mask_eager_and_graph(prec):
    """sample(..., c_mask=...) reaches the decoder: the eager loop and the HIP-graph replay agree for two different
    masks through one captured graph (the mask is a static buffer), and differ from the unmasked run.
    Between the capture and the later replays the test allocates and fills many small tensors: the captured launches
    read the jump plan's coefficient tensors by address, and a graph entry that did not keep them alive would replay
    with whatever the allocator put into their blocks (the decoder forward itself is deterministic here in both
    precisions, no atomics at these shapes: eager and replay give the same tokens, logits within 1e-5)."""
    from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
    from sampler import jumpy_sampler as JS
    rt = _rt()
    V = LENGTHS_DEC["V"]
    g = load("lengths")
    cond = T(g["base_feats"]).to(dev)
    masks = [T(g["base_mask"]).to(dev), (torch.arange(49)[None, :] < torch.tensor([5, 49, 33])[:, None]).to(dev)]
    with rt.use_precision(prec):
        dec = _decoder()
        dec.eval()
        smp = JS.DiffusionJumpySampler(DiscreteDiffusionScheduler(K=V, T=200, device=dev, beta_max=0.2), dec, K=V,
                                       T_train=200, T_infer=6, r=2, greedy=True, posterior_mode="map",
                                       sampling_mode="exact", device=dev)
        xT = torch.randint(0, V, (3, 16), generator=torch.Generator().manual_seed(2)).to(dev)
        eager = []
        for m in masks:
            _, e0, el = smp._run(xT, cond, smp._plan(3), m)
            eager.append((e0.clone(), el.float().clone()))
        _, _, plain = smp._run(xT, cond, smp._plan(3))
        plain = plain.float().clone()
        junk = []
        for rnd in range(3):          # capture on the first pass, replays on the later ones
            for m, (e0, el) in zip(masks, eager):
                g0, gl = smp._sample_graph(xT, cond, m)
                assert torch.equal(e0, g0), f"pass {rnd}: tokens of the graph replay differ from the eager loop"
                close(gl.float(), el, rtol=1e-5, what=f"pass {rnd}: graph vs eager logits")
            junk += [torch.full((n,), 1e30, device=dev) for n in (3, 12, 12, 48, 100) for _ in range(40)]
        assert len(smp._graphs) == 1
        gp, glp = smp._sample_graph(xT, cond)
        close(glp.float(), plain, rtol=1e-5, what="unmasked graph vs eager logits")
        assert len(smp._graphs) == 2          # keyed on whether a mask is present
        del junk
    assert (eager[0][1] - plain).abs().max().item() > 1e-3
    assert (eager[0][1] - eager[1][1]).abs().max().item() > 1e-3
