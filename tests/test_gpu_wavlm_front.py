"""The encoder-only kernels per element against float64: conv layer 0 + GroupNorm + GELU (conv0_gram, conv0_gn_affine,
conv0_apply<float|bf16>, conv0_mfma), the relative-position gate (wavlm_gate<float|bf16>) (csrc/wavlm.hip) and the
positional conv (posconv_kernel<1..4>, csrc/posconv.hip). The encoder is frozen: no loss curve would show a wrong frame
or channel here.

Cases (helpers.CONV0_CASES, POSCONV_CASES, GATE_CASES): the smallest shapes at which each mechanism exists — both halves
of the MFMA kernel's 16-frame store split empty and full, its 512-frame block, a second channel block (blockIdx.z = 1),
the apply kernel's 64-frame block, the second trip of its channel loop, its bf16 form, a mostly idle block, the
4096-frame statistics block with one frame and with two blocks after it; every posconv instantiation with 1, 2, 3, 48
and 64 weight stages, S = 1, S shorter than the padding, S on the 256-frame block edge; gate heads of 8, 32 and 64
channels with H = 1, 2, 3, 5 and a ragged last block.

Inputs: each conv0 case takes its utterances from different kinds (loud 3 randn, plain 0.1 randn, dc 0.05 randn + 0.4,
quiet 1e-4 randn, silent zeros), so every utterance has its own GroupNorm affine, with three tail samples that reach no
frame; weights 0.3 randn times a power of two per channel. The positional conv's x carries a power of two per frame
(2^-2 .. 2^2; 2^-1 .. 2^1 in the 64 x 128 case, helpers.POSCONV_FS_MAX), its weights and bias one per output channel
(2^-6 .. 2^6). The gate's W rows carry 2^-2 .. 2^2 and cst differs per head. The reference is torch float64 on the
device from the same operands.

Bounds, per element, with u = 2^-24 and s the size of the terms whose roundings reach the pre-activation:
    conv0, f32 out (conv0_apply<float>)     |gelu'(z)| C32 u s + 2e-6                 s = |sc| (|x| * |w|) + |sh|
    conv0, bf16 out, C % 512 != 0           |gelu'(z)| C32 u s + 2.6e-5, then bf16
    conv0, bf16 out, C % 512 == 0 (MFMA)    |gelu'(z)| Csplit 2^-18 s + 2.6e-5, then bf16
    posconv                                 |gelu'(y)| Cpos u s + 2e-6, then bf16     s = |x| * |w| + |bias|
    gate                                    |dgate/dpa| Cg8 u s_a + |dgate/dpb| Cg8 u s_b + A   (helpers.gate_out64)
    "then bf16": b + 2^(floor(log2(|ref| + b)) - 8), one rounding to nearest, the exact half ulp
No element is left out. The positional conv writes into a slice of a NaN-filled buffer; the row of E before it and the
row after it must keep their bits.

C = 8 E, E measured on the CPU from the reference alone (tests/test_cpu_wavlm_front_ref.py, which also proves that the
listed mutants of each family leave these bounds on at least half of the elements they touch):
    C32 = 40.8    Csplit = 37.2    Cpos = 11.92    Cg8 = 19.12     (hard cap 64)

Measured on an MI355X: "units" is the C an f32 output would have needed: for conv0 the largest
(|out - ref| - 2e-6) / (|gelu'(z)| u s) over its elements with |gelu'(z)| >= 0.1 (a GELU output shows its
pre-activation's error only through gelu', and the 2e-6 of the GELU itself would read as hundreds of units of a
near-silent utterance's s), for the gate the plain |out - ref| / (u (|dgate/dpa| s_a + |dgate/dpb| s_b)), A left in, over
its elements where that denominator is at least u (where both derivatives vanish the gate is a constant and only its
own rounding is left); "share" is the largest share of its bound any output used. The bf16 outputs reach 0.99 of
theirs by construction: a correctly rounded value next to a rounding boundary uses the whole half ulp.
    path               units    share of bound
    conv0 apply f32    1.21     0.113     (of C32 = 40.8)
    conv0 apply bf16   -        0.995
    conv0 mfma         -        0.984
    posconv <1>        -        0.999
    posconv <2>        -        0.998
    posconv <3>        -        0.996
    posconv <4>        -        0.999
    gate f32           1.46     0.194     (of Cg8 = 19.12, A left in)
    gate bf16          2.72     0.247
"""
import re

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
NEED = {}          # row of the table above -> [units, share]
assert all(v <= 64.0 for v in H.FRONT_C.values())


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    for k in sorted(NEED):
        units = f"{NEED[k][0]:6.2f}" if NEED[k][0] >= 0 else "     -"
        print(f"\nFRONTNEED {k:<16} units {units}  share {NEED[k][1]:5.3f}", end="")
    print()


def _ops():
    from fddm_hip import ops
    return ops


def _check(row, what, out, ref, bound, need=None):
    """Every element of out within bound of ref; record the row's share of the bound (and, for an f32 output, need =
    (absolute term, |lin| unit s): the C it would have needed)."""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out.double() - ref).abs()
    share = (err / bound).max().item()
    units = -1.0
    if need is not None:
        a, d = need
        ok = d[1]
        units = ((err - a).clamp_min(0.0)[ok] / d[0][ok]).max().item() if ok.any() else 0.0
    print(f"FRONT {what}: share {share:.3f}" + (f" units {units:.2f}" if need is not None else ""))
    n = NEED.setdefault(row, [-1.0, 0.0])
    n[0], n[1] = max(n[0], units), max(n[1], share)
    bad = err > bound
    at = np.unravel_index(int((err / bound).argmax()), tuple(err.shape))
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements leave their bound, the worst by a factor "
                           f"{share:.2f} at {tuple(int(i) for i in at)}")


def _refused(fn, bad):
    """Every (message, arguments) row raises the ValueError of the precondition it names."""
    for msg, a in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            fn(*a)


@pytest.mark.parametrize("case", H.CONV0_CASES, ids=[c[0] for c in H.CONV0_CASES])
def test_conv0_gn_gelu(case):
    cid, path, C, T0s, kinds = case
    o = _ops()
    w, gamma, beta = (t.to(dev) for t in H.conv0_params(C))
    dt = torch.float32 if path == "f32" else BF
    for T0 in T0s:
        wave = H.conv0_wave(kinds, T0).to(dev)
        r = H.conv0_ref64(wave, w, gamma, beta)
        out = o.conv0_gn_gelu(wave, w, gamma, beta, dt, C, H.CONV0_K, H.CONV0_S, eps=H.CONV0_EPS)
        assert out.dtype == dt and out.shape == (len(kinds), T0, C)
        need = None
        if path == "f32":
            need = (H.GEMM_GELU_ABS, (r.lin * H.U24 * r.s, r.lin >= 0.1))
        row = {"mfma": "conv0 mfma", "bf16": "conv0 apply bf16", "f32": "conv0 apply f32"}[path]
        _check(row, f"conv0 {cid} T0={T0}", out, r.ref, H.conv0_bound(r, path), need)


@pytest.mark.parametrize("case", H.POSCONV_CASES, ids=["x".join(map(str, c)) for c in H.POSCONV_CASES])
def test_posconv_gelu(case):
    Cg, kp, G, B, S = case
    o = _ops()
    E = G * Cg
    x, w, bias = H.posconv_operands(*case)
    r = H.posconv_ref64(x, w, bias, G, device=dev)
    buf = torch.full((B * S + 2, E), float("nan"), device=dev, dtype=BF)
    guard = buf[[0, -1]].view(torch.int16).clone()
    out = buf[1:-1]
    o.posconv_gelu(x.to(dev).view(B * S, E), H.posconv_pack(w, G).to(dev), bias.to(dev), out, B, S, E, G, kp)
    torch.cuda.synchronize()
    assert torch.equal(buf[[0, -1]].view(torch.int16), guard), "posconv wrote outside its B*S rows"
    _check(f"posconv <{Cg // 16}>", f"posconv Cg={Cg} kp={kp} G={G} B={B} S={S}", out.view(B, S, E), r.ref,
           H.posconv_bound(r))


@pytest.mark.parametrize("case", H.GATE_CASES, ids=["-".join(map(str, c)) for c in H.GATE_CASES])
def test_wavlm_gate(case):
    dt, B, S, Hh, dh = case
    o = _ops()
    x, W, bias, cst = (t.to(dev) for t in H.gate_operands(*case))
    r = H.gate_ref64(x, W, bias, cst, B, S, Hh)
    out = o.wavlm_gate(x, W, bias, cst, B, S, Hh)
    assert out.dtype == torch.float32 and out.shape == (B * Hh, S)
    d = ((r.da * r.sa + r.db * r.sb) * H.U24).transpose(1, 2)
    _check(f"gate {dt}", f"gate {dt} B={B} S={S} H={Hh} dh={dh}", out.view(B, Hh, S), r.ref, H.gate_bound(r),
           (0.0, (d, d >= H.U24)))


def test_wavlm_gate_refuses_bad_arguments():
    o = _ops()
    B, S, Hh, dh = 2, 5, 3, 16
    x = torch.zeros(B * S, Hh * dh, device=dev)
    W, bias, cst = torch.zeros(8, dh, device=dev), torch.zeros(8, device=dev), torch.ones(Hh, device=dev)
    assert o.wavlm_gate(x, W, bias, cst, B, S, Hh).shape == (B * Hh, S)
    X, ROWS, EH, DH = "x is contiguous f32 / bf16 [B*S, E]", "x has B*S rows, H > 0", "E is a multiple of H", "head width"
    WM, BM, CM = "W is contiguous f32 [8, dh]", "bias is f32 [8]", "cst is f32 [H]"
    z = lambda *shape: torch.zeros(*shape, device=dev)   # noqa: E731
    bad = [
        (X, (x.view(B, S, -1), W, bias, cst, B, S, Hh)),                    # not 2-D
        (X, (x.t().contiguous().t(), W, bias, cst, B, S, Hh)),              # not contiguous
        (X, (x.half(), W, bias, cst, B, S, Hh)),                            # neither f32 nor bf16
        (ROWS, (x, W, bias, cst, B, S + 1, Hh)),                            # not B*S rows
        (ROWS, (x, W, bias, z(0), B, S, 0)),                                # no head
        (EH, (x, W, bias, z(5), B, S, 5)),                                  # E % H
        (DH, (x, z(8, 12), bias, z(4), B, S, 4)),                           # dh % 8
        (DH, (z(B * S, 72), z(8, 72), bias, z(1), B, S, 1)),                # dh > 64
        (WM, (x, W.bfloat16(), bias, cst, B, S, Hh)),                       # W not f32
        (WM, (x, z(dh, 8).t(), bias, cst, B, S, Hh)),                       # W not contiguous
        (WM, (x, z(8, 2 * dh), bias, cst, B, S, Hh)),                       # W not [8, dh]
        (BM, (x, W, z(4), cst, B, S, Hh)),                                  # bias not [8]
        (BM, (x, W, bias.double(), cst, B, S, Hh)),                         # bias not f32
        (BM, (x, W, z(16)[::2], cst, B, S, Hh)),                            # bias not contiguous
        (CM, (x, W, bias, z(Hh + 1), B, S, Hh)),                            # cst not [H]
        (CM, (x, W, bias, cst.double(), B, S, Hh)),                         # cst not f32
        (CM, (x, W, bias, z(2 * Hh)[::2], B, S, Hh)),                       # cst not contiguous
    ]
    _refused(o.wavlm_gate, bad)


def test_conv0_gn_gelu_refuses_bad_arguments():
    o = _ops()
    C, K, S = 6, 10, 5
    wave = torch.zeros(2, 33, device=dev)
    w, gamma, beta = torch.zeros(C, K, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    assert o.conv0_gn_gelu(wave, w, gamma, beta, torch.float32, C, K, S).shape == (2, 5, C)
    f32 = torch.float32
    WV, KC = "wave is contiguous f32 [B, nsamp]", "kernel width 10, an even"
    WM, GB = "w is contiguous f32 [C, K]", "gamma and beta"
    z = lambda *shape: torch.zeros(*shape, device=dev)   # noqa: E731
    bad = [
        (WV, (wave[0], w, gamma, beta, f32, C, K, S)),                      # not 2-D
        (WV, (wave[:, ::2], w, gamma, beta, f32, C, K, S)),                 # not contiguous
        (WV, (wave.double(), w, gamma, beta, f32, C, K, S)),                # not f32
        ("shorter than the kernel", (wave[:, :9].contiguous(), w, gamma, beta, f32, C, K, S)),   # nsamp < K
        (WM, (wave, w.bfloat16(), gamma, beta, f32, C, K, S)),              # w not f32
        (WM, (wave, z(K, C).t(), gamma, beta, f32, C, K, S)),               # w not contiguous
        (WM, (wave, z(C + 2, K), gamma, beta, f32, C, K, S)),               # w not [C, K]
        (KC, (wave, z(C, 8), gamma, beta, f32, C, 8, S)),                   # K != 10
        (KC, (wave, z(5, K), gamma[:5], beta[:5], f32, 5, K, S)),           # C odd
        (GB, (wave, w, gamma.double(), beta, f32, C, K, S)),                # gamma not f32
        (GB, (wave, w, gamma, beta.bfloat16(), f32, C, K, S)),              # beta not f32
        (GB, (wave, w, gamma[:4], beta, f32, C, K, S)),                     # gamma not [C]
        (GB, (wave, w, gamma, z(C + 1), f32, C, K, S)),                     # beta not [C]
        (GB, (wave, w, z(2 * C)[::2], beta, f32, C, K, S)),                 # gamma not contiguous
        (GB, (wave, w, gamma, z(2 * C)[::2], f32, C, K, S)),                # beta not contiguous
        ("f32 or bf16 output", (wave, w, gamma, beta, torch.float16, C, K, S)),
    ]
    _refused(o.conv0_gn_gelu, bad)
