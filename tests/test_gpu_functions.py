"""The torch.autograd.Functions of the train step (fddm_hip/functions.py) against float64 autograd of the operation each
claims to be. The kernels they launch are pinned one by one elsewhere; this file pins the wiring between them: which
buffer a launch reads, accumulate against overwrite, the upstream scalar, gradient destinations (fresh tensors against
GradArena slots) and, in bf16 mode, the logits gradient's way from KLFn / TextEmbedFn to HeadFn through the module-level
hand-over dicts.

References, inputs, companions and case tables: tests/helpers.py ("the autograd Functions"); what the bounds can tell
apart: tests/test_cpu_functions_ref.py. Per element |got - ref| <= C u companion, u = 2^-24 in fp32 mode and 2^-9 in
bf16 mode (EmbedFn / CondFn: 2^-24 in both, they compute in fp32 in both), C = min(64, 8 E), E = helpers.FN_E, the
worst ratio measured on an MI355X over every case of this file (the FNE lines it prints).

What turned out of the branches nobody had run:
  HeadFn.backward with a zero-stride dlogits (loss = KL + c logits.sum(), case kl_expand, bf16): real. The branch took
    the handed-over KL gradient alone and lost c from every element. Fixed: a gradient that is not None is always added.
  KLFn.forward on logits[:1] (case kl_slice, bf16): real. The slice shares the owner's address, took the bf16 hand-over
    and left a [L, V] gradient for a HeadFn whose xT has B L rows (a ValueError from linear_dw after the first GEMM had
    run). Fixed: the owner's shape must match; the slice then takes the fp32 path and autograd pads its gradient.
  Not on the list: only bf16-mode forwards swept the dicts for outputs that were freed without a backward, so the
    entries (and the KL gradient buffer) of an abandoned bf16 forward outlived every fp32-mode step that followed.
    Fixed: HeadFn.forward sweeps in both modes (test_head_handover_survives_an_abandoned_forward).
  CondFn.backward's `dtb is None` and `g is None` branches: unreachable from autograd. CondFn leaves
    materialize_grads on, so an unused t_bias or FiLM output arrives as a zero tensor (modes film_only and foreign below
    run exactly that: the stacked branch with a zero in place of the missing gradient). nf == 0 is reachable (NL = 0).
  Order independence (text_kl), V % 8 != 0, two KL terms, the KL's upstream scalar in both hand-over forms, LinearFn's
    ab != aw and colsum branches, a second backward into arena slots, LfdFn's alpha and upstream scalar: all correct.
"""
import gc

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _mods():
    from fddm_hip import functions as FN
    from fddm_hip import ops
    from fddm_hip import runtime as rt
    return FN, ops, rt


def _check(fn, out, prec, got, ref, comp, what, u=None):
    e = H.fn_excess(got, ref, comp, H.FN_U[prec] if u is None else u)
    print(f"FNE {fn} {out} {prec} {what}: {e:.3f} (allowed {H.fn_c(fn, out, prec):.1f})")
    return e <= H.fn_c(fn, out, prec), f"{fn} {out} {prec} {what}: {e:.3f} units > C {H.fn_c(fn, out, prec):.1f}"


def _all(results):
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "; ".join(bad)


def _dicts_empty(FN):
    return not (FN._head_outputs or FN._dlogits_bf16 or FN._kl_dz or FN._combined)


# ------------------------------------------------------------------ HeadFn / KLFn / TextEmbedFn
def _head_graph(FN, rt, V, masked, consumers, prec):
    """The composite of helpers.head_ref64 on the device: (loss, leaves, logits2d)."""
    i = H.head_inputs(V, masked)
    B, L = H.HEAD_B, H.HEAD_L
    x = i.x.to(dev).requires_grad_(True)
    xT = x.detach().to(rt.compute_dtype()).contiguous()
    hw, hb, tw = (torch.nn.Parameter(v.to(dev)) for v in (i.hw, i.hb, i.tw))
    logits2d = FN.HeadFn.apply(x, xT, hw, hb)
    if prec == "fp32":
        logits2d.retain_grad()
    logits = logits2d.view(B, L, V)
    xt, x0, t, betas = i.xt.to(dev), i.x0.to(dev), i.t.to(dev), i.betas.to(dev)
    mask = None if i.mask is None else i.mask.to(dev).view(torch.uint8)
    loss = None
    for kind, c in consumers:
        if kind in ("kl", "klslice"):
            r = B if kind == "kl" else 1
            term = c * FN.KLFn.apply(logits[:r] if r < B else logits, xt[:r], x0[:r], t[:r],
                                     None if mask is None else mask[:r].reshape(-1), betas)
        elif kind == "text":
            term = c * (FN.TextEmbedFn.apply(logits, tw) * i.Rz.to(dev).view(B, L, -1)).sum()
        elif kind == "dense":
            term = c * (logits * i.R.to(dev).view(B, L, V)).sum()
        else:
            term = c * logits.sum()
        loss = term if loss is None else loss + term
    return loss, dict(x=x, hw=hw, hb=hb, tw=tw), logits2d


def _head_case(prec, name, V, masked):
    FN, ops, rt = _mods()
    ref = H.head_case_ref(name, V, masked)
    with rt.use_precision(prec):
        loss, leaves, logits2d = _head_graph(FN, rt, V, masked, H.HEAD_CASES[name], prec)
        loss.backward()
        torch.cuda.synchronize()
    assert _dicts_empty(FN), "hand-over dicts not empty after a completed backward"
    what = f"{name} V={V} masked={masked}"
    scale = sum(abs(v) for v in ref.terms.values())
    err = abs(float(loss.detach()) - ref.loss)
    print(f"FNE head loss {prec} {what}: {err / scale:.3e} of sum |terms|")
    res = [(err <= 64.0 * H.FN_U[prec] * scale, f"loss {float(loss.detach())} vs {ref.loss}")]
    got = {k: v.grad for k, v in leaves.items()}
    got["dl"] = logits2d.grad if prec == "fp32" else None
    for k, g in ref.g.items():
        if k == "dl" and prec != "fp32":
            continue                      # bf16 mode: the logits gradient never passes through autograd
        if g is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None, f"{what}: no gradient for {k}"
        res.append(_check("head", k, prec, got[k], g, ref.m[k], what))
    _all(res)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("V", H.HEAD_V)
@pytest.mark.parametrize("name", list(H.HEAD_CASES))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_head_kl_text_handover_matrix(prec, name, V, masked):
    """Every case of helpers.HEAD_CASES at 60 rows, V = 304 / 300 / 301, with a padded x_mask and with None: the
    gradients of head.weight, head.bias, the head's input, the text weight and (fp32 mode) the logits against float64
    autograd of the same composite, and the four hand-over dicts empty afterwards. kl_expand and kl_slice are the two
    cases that were wrong before (module docstring)."""
    _head_case(prec, name, V, masked)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_head_handover_survives_an_abandoned_forward(prec):
    """A bf16 forward with the KL built and no backward leaves its entries in the dicts; once its tensors are dropped,
    the next step, in either precision, must clean them up (dead weak references, or the reused address), compute the
    float64 gradients and leave the dicts empty. (fp32-mode forwards did not sweep before: the abandoned step's KL
    gradient buffer stayed alive until the next bf16 forward.)"""
    FN, ops, rt = _mods()
    with rt.use_precision("bf16"):
        loss, leaves, logits2d = _head_graph(FN, rt, 304, True, H.HEAD_CASES["kl_text"], "bf16")
        torch.cuda.synchronize()
        assert FN._head_outputs and FN._kl_dz, "the abandoned forward registered nothing: the case tests nothing"
        del loss, leaves, logits2d
        gc.collect()
    _head_case(prec, "kl_text", 304, True)
    _head_case(prec, "kl", 300, False)


# ------------------------------------------------------------------ LinearFn
@pytest.mark.parametrize("si,bias,needs,dest", H.linear_fn_cases())
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_linear_fn(prec, si, bias, needs, dest):
    """Two forward / backward passes with different cotangents and no zeroing between them: .grad (fresh destinations,
    summed by autograd) or the GradArena slot (accumulated by the kernels) must hold the float64 sum. 3-D input, 45
    rows; out = 100 takes the zero-padded GEMMs; w_arena = weight in the arena, bias fresh (ab != aw); w_frozen = the
    bias-only colsum branch."""
    FN, ops, rt = _mods()
    i = H.linear_fn_inputs(si)
    ref = H.linear_fn_ref64(si, bias)
    with rt.use_precision(prec):
        x = i.x.to(dev).requires_grad_(needs != "x_detached")
        w = torch.nn.Parameter(i.w.to(dev), requires_grad=needs != "w_frozen")
        b = torch.nn.Parameter(i.b.to(dev)) if bias else None
        inside = [p for p in ((w, b) if dest == "arena" else (w,) if dest == "w_arena" else ()) if p is not None
                  and p.requires_grad]
        arena = rt.GradArena(inside) if inside else None
        for p in range(2):
            y = FN.linear(x, w, b)
            (y * i.Ry[p].to(dev)).sum().backward()
        torch.cuda.synchronize()
    H.close(y, ref.y, rtol=1e-5, what="y")
    if arena is not None:
        for p, v in zip(arena.params, arena.views):
            assert p.grad.data_ptr() == v.data_ptr(), "the gradient left its arena slot"
    what = f"{H.LINEAR_SHAPES[si]} bias={bias} {needs} {dest}"
    res = []
    for k, t in (("x", x), ("w", w), ("b", b)):
        want = ref.g[k] is not None and t is not None and t.requires_grad
        if not want:
            assert t is None or t.grad is None, f"{what}: unexpected gradient for {k}"
            continue
        assert t.grad is not None, f"{what}: no gradient for {k}"
        res.append(_check("linear", k, prec, t.grad, ref.g[k], ref.m[k], what))
    _all(res)


# ------------------------------------------------------------------ LfdFn
@pytest.mark.parametrize("g", H.LFD_FN_G)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_lfd_fn(prec, g):
    """B = 4, T = 6, D = 64, group = None: both inputs' gradients (the two alpha = 1 / (N T) GEMMs, the upstream scalar)
    against float64 autograd of g * oracle.lfd_loss. Companion: max |ref| of the element's column d (helpers.lfd_fn_ref64
    says why no finer one exists)."""
    FN, ops, rt = _mods()
    ref = H.lfd_fn_ref64(g)
    za, zb = (v.to(dev).requires_grad_(True) for v in H.lfd_fn_inputs())
    with rt.use_precision(prec):
        loss = FN.LfdFn.apply(za, zb, H.LFD_FN_LAM, H.LN_EPS, None)
        (loss if g == 1.0 else g * loss).backward()
        torch.cuda.synchronize()
    err = abs(float(loss.detach()) - ref.loss) / abs(ref.loss)
    print(f"FNE lfd loss {prec} g={g}: rel {err:.3e}")
    res = [(err <= (1e-4 if prec == "fp32" else 2e-2), f"loss {float(loss.detach())} vs {ref.loss}")]
    res += [_check("lfd", k, prec, t.grad, ref.g[k], ref.m[k], f"g={g}") for k, t in (("za", za), ("zb", zb))]
    _all(res)


# ------------------------------------------------------------------ EmbedFn + CondFn
class _FilmUse(torch.autograd.Function):
    """Stands in for a decoder block's use of its FiLM pair: (scale * R0).sum() + (shift * R1).sum(), whose backward
    accumulates into the two gbuf slices it was given and hands those slices back, as DecoderBlockFn does."""

    @staticmethod
    def forward(ctx, fs, fh, gs, gh, R0, R1):
        ctx.save_for_backward(gs, gh, R0, R1)
        return (fs * R0).sum() + (fh * R1).sum()

    @staticmethod
    def backward(ctx, g):
        gs, gh, R0, R1 = ctx.saved_tensors
        gs.data.add_(g * R0)        # through .data, as a kernel writes: CondFn saved gbuf, whose version must not move
        gh.data.add_(g * R1)
        return gs, gh, None, None, None, None


COND_CASES = [(NL, d, mode, dest) for NL in H.COND_FN_NL for d in H.COND_FN_D for mode in H.COND_FN_MODES
              for dest in ("fresh", "arena") if NL > 0 or mode == "gbuf"]


@pytest.mark.parametrize("NL,d,mode,dest", COND_CASES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_embed_cond_fn(prec, NL, d, mode, dest):
    """x = E[xt] + t_bias with pad tokens and the FiLM projections, B = 3: mode gbuf = the FiLM gradients come back as
    the gbuf slices the blocks accumulated into; foreign = as other tensors, FiLM output 1 unused (the stacked branch;
    autograd materialises the missing one as zeros, see the module docstring); film_only = t_bias unused (zeros for dtb).
    NL = 0: no FiLM at all. A parameter the loss does not reach has no gradient or an all-zero one."""
    FN, ops, rt = _mods()
    i = H.cond_fn_inputs(NL, d)
    ref = H.cond_fn_ref64(NL, d, mode)
    B, L = H.COND_FN_B, H.COND_FN_L
    with rt.use_precision(prec):
        P = [torch.nn.Parameter(v.to(dev)) for v in i.params]
        E = torch.nn.Parameter(i.E.to(dev))
        arena = rt.GradArena(P + [E]) if dest == "arena" else None
        gbuf = torch.zeros(2 * NL, B, d, device=dev)
        outs = FN.CondFn.apply(i.t.to(dev), i.pooled.to(dev), gbuf, d, H.TE_MAX_STEPS, *P)
        tb, films = outs[0], outs[1:]
        assert len(films) == 2 * NL
        x, xT = FN.EmbedFn.apply(i.xt.to(dev), E, tb, 0)
        H.close(x, ref.x, rtol=1e-5, what="x")
        Rf = i.Rf.to(dev)
        loss = torch.zeros((), device=dev)
        if mode != "film_only":
            loss = loss + (x * i.Rx.to(dev)).sum()
        for blk in range(NL):
            if mode == "gbuf":
                loss = loss + _FilmUse.apply(films[2 * blk], films[2 * blk + 1], gbuf[2 * blk], gbuf[2 * blk + 1],
                                             Rf[2 * blk], Rf[2 * blk + 1])
            else:
                for k in (2 * blk, 2 * blk + 1):
                    if ref.used[k]:
                        loss = loss + (films[k] * Rf[k]).sum()
        loss.backward()
        torch.cuda.synchronize()
    if arena is not None:
        for p, v in zip(arena.params, arena.views):
            assert p.grad.data_ptr() == v.data_ptr(), "the gradient left its arena slot"
    what = f"NL={NL} d={d} {mode} {dest}"
    res = []
    for k, g in ref.g.items():
        p = E if k == "E" else P[int(k[1:])]
        if g is None:
            assert p.grad is None or not p.grad.any(), f"{what}: {k} has a gradient the loss does not give it"
            continue
        assert p.grad is not None, f"{what}: no gradient for {k}"
        out = "emb" if k == "E" else "time" if int(k[1:]) < 6 else "film"
        res.append(_check("cond", out, prec, p.grad, g, ref.m[k], f"{what} {k}", u=H.U24))
    _all(res)


# ------------------------------------------------------------------ ops.linear_dx_rope: where it applies
def test_linear_dx_rope_applicability_and_fallback():
    """linear_dx_rope must answer False, launching nothing, for RoPE tables its kernel cannot read (it takes raw
    pointers and reads both tables with 16-byte loads at positions 0 .. L - 1): a bf16 sin table, tables shorter than L,
    a non-contiguous sin table, a sin table that is not 16-byte aligned. dx keeps its bits in each case. The caller's fallback (linear_dx + rope_bwd,
    DecoderBlockFn.backward) and the fused launch on the valid tables both give dx_old + RoPE^T(dy W) in float64."""
    FN, ops, rt = _mods()
    L, d, M = H.HEAD_L, 128, 7 * H.HEAD_L        # 140 rows: the fused kernel needs 128, the second tile is ragged
    gen = H._gen(9500)
    dy = H._grid(torch.randn(M, 2 * d, generator=gen)).to(dev).to(torch.bfloat16)
    w = H._grid(0.1 * torch.randn(2 * d, d, generator=gen)).to(dev).to(torch.bfloat16)
    dx0 = torch.randn(M, d, generator=gen).to(dev)
    from oracle import fddm_oracle as O
    cos, sin = (v.to(dev).contiguous() for v in O.rope_cos_sin(L, O.rope_inv_freq(d)))
    wide = torch.zeros(L, 2 * d, device=dev)
    wide[:, ::2] = sin
    off = torch.zeros(L * d + 4, device=dev)
    off[1: 1 + L * d] = sin.reshape(-1)
    bad = {"bf16 sin": (cos, sin.to(torch.bfloat16)), "short tables": (cos[: L - 1], sin[: L - 1]),
           "strided sin": (cos, wide[:, ::2]), "short sin": (cos, sin[: L - 1]),
           "sin 4 bytes past a 16-byte boundary": (cos, off[1: 1 + L * d].view(L, d))}
    for name, (cs, sn) in bad.items():
        dx = dx0.clone()
        assert ops.linear_dx_rope(dy, w, dx, cs, sn, L) is False, name
        torch.cuda.synchronize()
        assert torch.equal(dx, dx0), f"{name}: dx changed"
    P = dy.double().cpu() @ w.double().cpu()
    Pm = dy.double().cpu().abs() @ w.double().cpu().abs()
    want = dx0.double().cpu() + H.rope_bwd_ref64(P, cos.cpu(), sin.cpu(), L)
    comp = dx0.double().cpu().abs() + H.rope_bwd_ref64(Pm, cos.cpu().abs(), sin.cpu().abs(), L, magnitude=True)
    dx = dx0.clone()
    dxr = ops.linear_dx(dy, w)
    ops.rope_bwd(dxr, cos, sin, dx, L)
    e_fb = H.fn_excess(dx, want, comp, H.U24)
    dx2 = dx0.clone()
    fused = ops.linear_dx_rope(dy, w, dx2, cos, sin, L)
    assert fused is True, "the check refuses tables the fused kernel can read"
    e_fu = H.fn_excess(dx2, want, comp, H.U24)
    print(f"FNE dx_rope fallback {e_fb:.3f} fused({fused}) {e_fu:.3f} units of 2^-24")
    assert e_fb <= H.GEMM_C["bf16"] and e_fu <= H.GEMM_C["bf16"], (e_fb, e_fu)
