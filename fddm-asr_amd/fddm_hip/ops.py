"""Thin torch-tensor wrappers over libfddm_hip (one function per C entry point, plus shape helpers).

Every wrapper launches on torch's current HIP stream and checks the hipError_t. Tensors must be
contiguous where the kernel assumes it; shapes are validated here before any launch so a kernel
never sees operands that disagree with its grid.
"""
from __future__ import annotations

import math
import os

import torch

from ._lib import call, lib

F32, BF16 = 0, 1
EPI_STORE, EPI_GELU, EPI_ACC, EPI_GELU_ONLY, EPI_DGELU = 0, 1, 2, 3, 4


def code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def tdtype(c: int):
    return torch.float32 if c == F32 else torch.bfloat16


def ptr(t):
    return 0 if t is None else t.data_ptr()


_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_device = torch._C._cuda_getDevice


def stream():
    """The current HIP stream of the current device as a raw handle (the launch path's hottest host call:
    torch.cuda.current_stream() builds a Stream object and resolves the device index through Python)."""
    return _raw_stream(_cur_device())


def _chk(cond, msg):
    if not cond:
        raise ValueError(msg)


# ------------------------------------------------------------------------------------------ GEMM
def _layout_ok(A, B, M, N, K, a_kc, b_kc, lda, ldb):
    """fddm_gemm's layout preconditions (csrc/gemm.hip): 16-B chunks of every operand row never straddle a row end
    (the contiguous dimension of each operand and its leading dimension are multiples of 8 bf16 / 4 f32 elements)
    and both operand base addresses are 16-B aligned."""
    ech = 8 if B.dtype == torch.bfloat16 else 4
    ok = (K % ech == 0 if a_kc else M % ech == 0) and lda % ech == 0
    ok = ok and (K % ech == 0 if b_kc else N % ech == 0) and ldb % ech == 0
    return ok and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0


def _gemm_padded(A, B, C, M, N, K, a_kc, b_kc, lda, ldb, ldc, epi, bias, alpha, colsum):
    """A GEMM whose operands miss the kernels' layout preconditions (a vocabulary or width that is not a multiple of
    8, e.g. the head / TextEmbedding GEMMs at V % 8 != 0): the operands are copied into zero-padded buffers (M, N,
    K rounded up to 8; the zero tail adds nothing to any dot product), the padded GEMM runs, and the M x N block is
    copied back. STORE / ACCUMULATE epilogues with bias and the fused column sum only."""
    _chk(epi in (EPI_STORE, EPI_ACC), "ragged GEMM: only store / accumulate epilogues have a padded form")
    p8 = lambda n: (n + 7) // 8 * 8   # noqa: E731
    Mp, Np, Kp = p8(M), p8(N), p8(K)
    a = torch.as_strided(A, (M, K) if a_kc else (K, M), (lda, 1))
    b = torch.as_strided(B, (N, K) if b_kc else (K, N), (ldb, 1))
    Ap = torch.zeros((Mp, Kp) if a_kc else (Kp, Mp), device=A.device, dtype=A.dtype)
    Bp = torch.zeros((Np, Kp) if b_kc else (Kp, Np), device=B.device, dtype=B.dtype)
    Ap[: a.shape[0], : a.shape[1]] = a
    Bp[: b.shape[0], : b.shape[1]] = b
    c = torch.as_strided(C, (M, N), (ldc, 1))
    Cp = torch.zeros(Mp, Np, device=C.device, dtype=C.dtype)
    if epi == EPI_ACC:
        Cp[:M, :N] = c
    bp = None
    if bias is not None:
        bp = torch.zeros(Np, device=bias.device, dtype=bias.dtype)
        bp[:N] = bias[:N]
    cs = None
    if colsum is not None:
        cs = torch.zeros(Mp, device=colsum.device, dtype=colsum.dtype)
        if epi == EPI_ACC:
            cs[:M] = colsum[:M]
    gemm(Ap, Bp, Cp, Mp, Np, Kp, a_kc=a_kc, b_kc=b_kc, lda=Ap.shape[1], ldb=Bp.shape[1], ldc=Np, epi=epi, bias=bp,
         alpha=alpha, colsum=cs)
    c.copy_(Cp[:M, :N])
    if colsum is not None:
        colsum[:M].copy_(cs[:M])
    return C


GEMM_PATHS = {"auto": 0, "big": 1, "small": 2, "256": 3, "128": 4}


def gemm_force_path(name: str) -> str:
    """Force a GEMM kernel family for every following fddm_gemm / conv GEMM launch (tests and diagnostics; "auto"
    restores the shape-based choice). Returns the previous setting's name."""
    from ._lib import lib
    old = lib().fddm_gemm_force_path(GEMM_PATHS[name])     # returns the previous path, not an error code
    return {v: k for k, v in GEMM_PATHS.items()}[old]


GEMM_FAMILIES = ("none", "small", "big", "256", "128", "grouped-small", "grouped-128")


def gemm_last_path():
    """(family, split-K slices) of the kernel the most recent gemm / conv1d_gemm / linear_dw_grouped / linear_dx_rope
    call launched (fddm_gemm_last_path): family is one of GEMM_FAMILIES, "none" when the call launched nothing. A
    host-side record for tests, which must know the kernel they measured: gemm_force_path only enables a family, and a
    shape outside its preconditions falls through to the register-staged kernel."""
    from ._lib import lib
    v = lib().fddm_gemm_last_path()
    return GEMM_FAMILIES[v & 0xFF], v >> 8


ATTN_KERNELS = {"auto": 0, "v6": 1, "nofused": 2, "fwd7": 3, "fwd8": 4, "relfwd5": 5}


def attn_force_kernels(name: str) -> str:
    """Select the attention kernel family for every following launch (tests and diagnostics): "v6" = the
    16x16x32-MFMA kernels of attention.hip where the 32x32x16 family (attn7.hip) would run, "nofused" = the 32x32x16
    family without its fused backward (dq7 + dkv7 at every key length), "fwd7" = the default with the one-chain forward
    fwd7 everywhere, "fwd8" = the default with the two-chain fwd8 (attn8.hip) everywhere, "relfwd5" = the default with
    WavLM's biased attention on the round-2 fwd5 instead of fwd7's REL build, "auto" = the default choice (fwd8 unless
    its 256-query workgroups load the busiest CU with more queries than fwd7's). Returns the previous setting's name."""
    from ._lib import lib
    old = lib().fddm_attn_set_kernels(ATTN_KERNELS[name])
    return {v: k for k, v in ATTN_KERNELS.items()}[old]


ATTN_FWD_KERNELS = ("none", "fwd7", "fwd8", "fwd6", "fwd2", "fwd5", "generic")
ATTN_DQ_KERNELS = {0: "none", 1: "bwdf7", 2: "dq7", 3: "dq2", 4: "bwd3s", 5: "dq4", 6: "dq"}
ATTN_DKV_KERNELS = {0: "", 2: "+dkv7", 3: "+dkv2", 5: "+dkv4", 6: "+dkv", 15: "+disagree"}


def attn_last_path():
    """The kernels the most recent attention forward call and the most recent attention backward call launched
    (fddm_attn_last_path), as a dict:
      fwd  (kernel, DM, MK, KX, REL): kernel one of ATTN_FWD_KERNELS and its template build
      bwd  (kernels, DM, MK, dkv MASK, NP, KX): kernels "bwdf7", "bwd3s" or a pair such as "dq7+dkv7", "dq2+dkv2",
           "dq2+dkv4" (ATTN_DQ_KERNELS + ATTN_DKV_KERNELS; the two launches are chosen separately); MK is dq7's MK or
           the MASK build of bwdf7 / dq2 (0 / 1); dkv MASK is dkv7's; NP bwdf7's key passes (0 for the pairs)
    A host-side record for tests, which must know the kernel they measured: attn_force_kernels only enables a family,
    and a shape outside its preconditions takes another kernel."""
    from ._lib import lib
    v = lib().fddm_attn_last_path()
    f, b = v & 0xFFFF, (v >> 16) & 0xFFFF
    return {"fwd": (ATTN_FWD_KERNELS[f & 15], (f >> 4) & 3, (f >> 6) & 3, bool((f >> 8) & 1), bool((f >> 9) & 1)),
            "bwd": (ATTN_DQ_KERNELS[b & 15] + ATTN_DKV_KERNELS[(b >> 12) & 15], (b >> 4) & 3, (b >> 6) & 3, (b >> 8) & 1,
                    (b >> 9) & 3, bool((b >> 11) & 1))}


def gemm(A, B, C, M, N, K, *, a_kc=True, b_kc=True, lda, ldb, ldc, epi=EPI_STORE, bias=None, alpha=1.0,
         C2=None, Mi=0, sAb=0, drop_p=0.0, seed=0, rng_stream=0, colsum=None):
    """C[m][n] = alpha * sum_k A(m,k) B(n,k) (+bias, epilogue). Compute dtype = B.dtype.
    bias (f32 [N]) is added once whatever kernel runs: epi=EPI_ACC gives C += alpha A B^T + bias, and an f32 store or
    accumulate that the library splits along K adds it on the first slice only (such biased calls run on the
    register-staged kernel, never on the 128x128 LDS-DMA ring). alpha != 1 is supported by every family but the
    persistent 256x256 kernel, which such calls never reach.
    Operands that miss the kernels' layout preconditions (a dimension or leading dimension not a multiple of 8, e.g.
    a ragged vocabulary) run zero-padded copies (_gemm_padded) — unbatched calls only: a batched / strided call
    (Mi or sAb set) with such operands raises."""
    _chk(B.dtype in (torch.float32, torch.bfloat16), "B dtype")
    if M == 0 or N == 0:
        return C
    if not _layout_ok(A, B, M, N, K, a_kc, b_kc, lda, ldb):
        _chk(Mi == 0 and sAb == 0, "batched / strided GEMM operands must meet the 8-element layout preconditions "
                                   "(the zero-padded fallback covers unbatched calls only)")
        return _gemm_padded(A, B, C, M, N, K, a_kc, b_kc, lda, ldb, ldc, epi, bias, alpha, colsum)
    call("fddm_gemm", code(B), code(A), int(a_kc), int(b_kc), epi, code(C), ptr(A), lda, Mi, sAb, ptr(B), ldb,
         ptr(C), ldc, ptr(C2), ptr(bias), float(alpha), M, N, K, seed, rng_stream, float(drop_p), ptr(colsum),
         stream())
    return C


def linear(x2d, w, bias=None, out_dtype=None, out=None, epi=EPI_STORE, C2=None, drop_p=0.0, seed=0, rng_stream=0):
    """y[M,N] = x[M,K] @ w[N,K]^T + bias.  x, w: compute dtype (x may be f32 when w is bf16)."""
    M, K = x2d.shape
    N = w.shape[0]
    _chk(w.shape[1] == K and x2d.stride(1) == 1 and w.is_contiguous(), "linear shapes")
    if out is None:
        out = torch.empty(M, N, device=x2d.device, dtype=out_dtype or w.dtype)
    return gemm(x2d, w, out, M, N, K, lda=x2d.stride(0), ldb=K, ldc=out.stride(0), epi=epi, bias=bias, C2=C2,
                drop_p=drop_p, seed=seed, rng_stream=rng_stream)


# diagnostic A/B knob (tools/ab.sh): FDDM_DX_WT=0 runs every dX on W as stored and keeps no transposed copies (the
# routing before they existed); a string of the letters s, a, d lets only the plain-store, the f32-accumulate and the
# dGELU-fused dX use their copies (FDDM_DX_WT=sa is stage A of profiles/dx_gemm256.md); 1 = all three
_DX_WT = os.environ.get("FDDM_DX_WT", "1")
_DX_WT_CLASS = {EPI_STORE: "s", EPI_ACC: "a", EPI_DGELU: "d"}


def dx_wt_enabled() -> bool:
    return _DX_WT != "0"


def linear_dx(dy2d, w, out=None, accumulate=False, out_dtype=torch.float32, epi=None, C2=None, drop_p=0.0, seed=0,
              rng_stream=0, wt=None):
    """dx[M,K] = dy[M,N] @ w[N,K]  (w M/N-contiguous operand). accumulate -> out (f32) += .
    wt (optional, bf16): w^T as a [K, N'] tensor whose rows hold w's columns (a column slice of a transposed weight
    copy: stride(1) == 1, any row stride). The product then runs as an ordinary NT GEMM on the K-contiguous copy,
    which lets fddm_gemm take the 256x256 kernel where its rule does (gemm_last_path tells); without wt, and with
    FDDM_DX_WT=0, w is read as stored."""
    M, N = dy2d.shape
    K = w.shape[1]
    _chk(w.shape[0] == N and w.is_contiguous() and dy2d.stride(1) == 1, "linear_dx shapes")
    if out is None:
        out = torch.empty(M, K, device=dy2d.device, dtype=out_dtype)
    e = EPI_ACC if accumulate else (EPI_STORE if epi is None else epi)
    if wt is not None and dy2d.dtype == torch.bfloat16 and (_DX_WT == "1" or _DX_WT_CLASS.get(e, "-") in _DX_WT):
        _chk(tuple(wt.shape) == (K, N) and wt.stride(1) == 1 and wt.dtype == w.dtype, "linear_dx: wt is not w^T")
        return gemm(dy2d, wt, out, M, K, N, a_kc=True, b_kc=True, lda=dy2d.stride(0), ldb=wt.stride(0),
                    ldc=out.stride(0), epi=e, C2=C2, drop_p=drop_p, seed=seed, rng_stream=rng_stream)
    return gemm(dy2d, w, out, M, K, N, a_kc=True, b_kc=False, lda=dy2d.stride(0), ldb=K, ldc=out.stride(0), epi=e,
                C2=C2, drop_p=drop_p, seed=seed, rng_stream=rng_stream)


def transpose_table(pairs):
    """Device table for transpose_bf16_mt over (src [rows, cols], dst [cols, rows]) pairs of contiguous bf16 tensors
    (rows and cols multiples of 8): (table, tensors, workgroups). Built on the host; not inside a graph capture."""
    rows_, nb = [], 0
    for src, dst in pairs:
        _chk(src.dim() == 2 and dst.dim() == 2 and src.dtype == torch.bfloat16 and dst.dtype == torch.bfloat16,
             "transpose: 2-D bf16 tensors")
        r, c = src.shape
        _chk(tuple(dst.shape) == (c, r) and src.is_contiguous() and dst.is_contiguous(), "transpose: dst is not src^T")
        _chk(r % 8 == 0 and c % 8 == 0 and r > 0 and c > 0, "transpose: rows and cols must be multiples of 8")
        _chk(src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.data_ptr() != dst.data_ptr(),
             "transpose: 16-B aligned, distinct buffers")
        rows_ += [src.data_ptr(), dst.data_ptr(), r, c, nb]
        nb += ((r + 63) // 64) * ((c + 63) // 64)
    dev = pairs[0][0].device
    tab = torch.tensor(rows_, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    return tab, len(pairs), nb


def transpose_bf16_mt(table):
    """dst = src^T for every pair of a transpose_table(), one launch."""
    tab, nt, nb = table
    call("fddm_transpose_bf16_mt", tab.data_ptr(), nt, nb, stream())


_NO_ROPE_FUSE = os.environ.get("FDDM_ROPE_FUSE", "1") == "0"     # diagnostic A/B knob (tools/ab.sh)


def linear_dx_rope(dy2d, w, dx, cs, sn, L) -> bool:
    """dx[M,d] += rope_bwd(dy[M,n] @ w[n,d]) in one launch (fddm_linear_dx_rope: the self-attention input gradient
    through RoPE). Returns False, launching nothing, where the fused kernel does not apply (not bf16, d % 128 != 0,
    a GEMM-family override, or RoPE tables the kernel cannot read: cs and sn must be contiguous f32 [rows >= L, d]
    tables of one shape on 16-byte boundaries, which the kernel reads with 16-byte loads at positions 0 .. L - 1): the
    caller then runs linear_dx into a temporary + rope_bwd."""
    M, N = dy2d.shape
    d = w.shape[1]
    if _NO_ROPE_FUSE:
        return False
    if not (dy2d.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and dx.dtype == torch.float32 and d % 128 == 0
            and w.shape[0] == N and w.is_contiguous() and dy2d.stride(1) == 1 and dx.is_contiguous()
            and tuple(dx.shape) == (M, d) and L > 0
            and cs.is_contiguous() and sn.is_contiguous() and cs.dtype == torch.float32 and sn.dtype == torch.float32
            and cs.dim() == 2 and cs.shape == sn.shape and cs.shape[-1] == d and cs.shape[0] >= L
            and cs.data_ptr() % 16 == 0 and sn.data_ptr() % 16 == 0):
        return False
    rc = lib().fddm_linear_dx_rope(ptr(dy2d), dy2d.stride(0), ptr(w), d, ptr(dx), d, ptr(cs), ptr(sn), M, d, N, L,
                                   stream())
    if rc == 1:      # hipErrorInvalidValue: not applicable, nothing launched
        return False
    if rc != 0:
        msg = lib().fddm_error_string(rc)
        raise RuntimeError(f"fddm_linear_dx_rope failed: hipError {rc} ({msg.decode() if msg else '?'})")
    return True


def linear_dw(dy2d, x2d, out=None, accumulate=False, db=None):
    """dW[N,K] = dy[M,N]^T @ x[M,K]  (both M/N-contiguous operands, K-reduction over tokens);
    db (optional, f32 [N]) receives sum_m dy[m] — the bias gradient, fused into the same launch.
    accumulate: out += and db += (grad-arena slots); otherwise both are overwritten."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    _chk(x2d.shape[0] == M and dy2d.stride(1) == 1 and x2d.stride(1) == 1, "linear_dw shapes")
    if out is None:
        out = torch.empty(N, K, device=dy2d.device, dtype=torch.float32)
    if db is not None and dy2d.dtype != x2d.dtype:
        gemm(dy2d, x2d, out, N, K, M, a_kc=False, b_kc=False, lda=dy2d.stride(0), ldb=x2d.stride(0),
             ldc=out.stride(0), epi=EPI_ACC if accumulate else EPI_STORE)
        colsum(dy2d, out=db, accumulate=accumulate)
        return out
    return gemm(dy2d, x2d, out, N, K, M, a_kc=False, b_kc=False, lda=dy2d.stride(0), ldb=x2d.stride(0),
                ldc=out.stride(0), epi=EPI_ACC if accumulate else EPI_STORE, colsum=db)


def linear_dw_grouped(jobs, kchunk=0):
    """One launch for several weight-gradient GEMMs, all accumulating: for each (dy [K,M], x [K,N], dW [M,N] f32,
    db [M] f32 or None): dW += dy^T x, db += sum_k dy. dy/x bf16 with unit inner stride.
    kchunk 0: the library balances split-K over the CUs (128x128 LDS-DMA kernel); kchunk > 0: every workgroup
    of the 128x128 register-staged kernel reduces about kchunk tokens."""
    import ctypes
    jobs = [j for j in jobs if j[0].shape[0] > 0]
    for i in range(0, len(jobs), 12):
        chunk = jobs[i:i + 12]
        n = len(chunk)
        for dy, x, dW, db in chunk:
            _chk(dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dW.dtype == torch.float32, "dw dtypes")
            _chk(dy.shape[0] == x.shape[0] and dW.shape == (dy.shape[1], x.shape[1]), "dw shapes")
            _chk(dy.stride(1) == 1 and x.stride(1) == 1 and dW.stride(1) == 1, "dw strides")
            _chk(db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == dy.shape[1]),
                 "db")
        P = ctypes.c_void_p * n
        L = ctypes.c_long * n
        call("fddm_gemm_dw_grouped", n, P(*[j[0].data_ptr() for j in chunk]), L(*[j[0].stride(0) for j in chunk]),
             P(*[j[1].data_ptr() for j in chunk]), L(*[j[1].stride(0) for j in chunk]),
             P(*[j[2].data_ptr() for j in chunk]), L(*[j[2].stride(0) for j in chunk]),
             P(*[ptr(j[3]) for j in chunk]), L(*[j[0].shape[1] for j in chunk]), L(*[j[1].shape[1] for j in chunk]),
             L(*[j[0].shape[0] for j in chunk]), kchunk, stream())


def colsum(X2d, out=None, accumulate=False):
    M, N = X2d.shape
    if out is None:
        out = torch.zeros(N, device=X2d.device, dtype=torch.float32)
    elif not accumulate:
        out.zero_()
    call("fddm_colsum", code(X2d), ptr(X2d), ptr(out), M, N, X2d.stride(0), stream())
    return out


def conv1d_gemm(x, W, out, *, lda, sAb, Tin, Cg, cstride, cpad, Bn, Tout, N, K, groups=1, bias=None, gelu=False):
    call("fddm_conv1d_gemm", code(W), EPI_GELU_ONLY if gelu else EPI_STORE, ptr(x), lda, sAb, Tin, Cg, cstride,
         cpad, ptr(W), ptr(out), out.shape[-1], ptr(bias), Bn, Tout, N, K, groups, stream())
    return out


def posconv_gelu(x, W, bias, out, B, S, E, G, kp):
    """WavLM positional conv + GELU (bf16): x/out [B*S, E], W [G, Cg, kp*Cg], bias [E] f32."""
    _chk(x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and out.dtype == torch.bfloat16, "posconv dtypes")
    _chk(x.is_contiguous() and W.is_contiguous() and out.is_contiguous() and bias.is_contiguous(), "posconv layout")
    _chk(x.numel() == B * S * E and out.numel() == B * S * E and W.numel() == E * kp * (E // G), "posconv shapes")
    call("fddm_posconv_gelu", ptr(x), ptr(W), ptr(bias), ptr(out), B, S, E, G, kp, stream())
    return out


def conv0_gn_gelu(wave, w, gamma, beta, out_dtype, C, K, S, eps=1e-5):
    """WavLM conv layer 0 + GroupNorm(C groups) + GELU: wave [B, nsamp] f32, w [C, K] f32 -> [B, T0, C] (f32 / bf16)."""
    _chk(wave.dim() == 2 and wave.is_contiguous() and wave.dtype == torch.float32,
         "conv0: wave is contiguous f32 [B, nsamp]")
    _chk(K == 10 and C % 2 == 0, "conv0: kernel width 10, an even channel count")
    _chk(w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (C, K), "conv0: w is contiguous f32 [C, K]")
    _chk(gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
         and gamma.is_contiguous() and beta.is_contiguous(), "conv0: gamma and beta are f32 [C]")
    _chk(out_dtype in (torch.float32, torch.bfloat16), "conv0: f32 or bf16 output")
    B, nsamp = wave.shape
    _chk(nsamp >= K, "conv0: an utterance shorter than the kernel")
    T0 = (nsamp - K) // S + 1
    nb = (T0 + 4095) // 4096  # statistics blocks per utterance (wavlm.hip C0_GRAM_FRAMES)
    ws = torch.empty(B * nb * (K + K * (K + 1) // 2) + B * C, device=wave.device, dtype=torch.float64)
    out = torch.empty(B, T0, C, device=wave.device, dtype=out_dtype)
    call("fddm_conv0_gn_gelu", code(out), ptr(wave), ptr(w), ptr(gamma), ptr(beta), ptr(ws), ptr(out), B, nsamp, T0,
         C, K, S, float(eps), stream())
    return out


def conv0_ln_gelu(wave, w, bias, gamma, beta, out_dtype, C, K, S, eps=1e-5, out=None):
    """Conv layer 0 of the WavLM-Large family: conv (w [C, K], bias) + LayerNorm over the C channels of every frame +
    GELU: wave [B, nsamp] f32 -> [B, T0, C] (f32 / bf16; written into `out`, contiguous, if given)."""
    _chk(wave.dim() == 2 and wave.is_contiguous() and wave.dtype == torch.float32,
         "conv0: wave is contiguous f32 [B, nsamp]")
    _chk(K == 10 and C % 8 == 0 and 0 < C <= 512, "conv0_ln: kernel width 10, C a multiple of 8 up to 512")
    _chk(w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (C, K), "conv0: w is contiguous f32 [C, K]")
    for t in (bias, gamma, beta):
        _chk(t.dtype == torch.float32 and t.numel() == C and t.is_contiguous(), "conv0_ln: bias, gamma and beta are f32 [C]")
    _chk(out_dtype in (torch.float32, torch.bfloat16), "conv0: f32 or bf16 output")
    B, nsamp = wave.shape
    _chk(nsamp >= K, "conv0: an utterance shorter than the kernel")
    T0 = (nsamp - K) // S + 1
    if out is None:
        out = torch.empty(B, T0, C, device=wave.device, dtype=out_dtype)
    _chk(out.is_contiguous() and tuple(out.shape) == (B, T0, C) and out.dtype == out_dtype,
         "conv0_ln: out is contiguous [B, T0, C] of out_dtype")
    call("fddm_conv0_ln_gelu", code(out), ptr(wave), ptr(w), ptr(bias), ptr(gamma), ptr(beta), ptr(out), B, nsamp, T0,
         C, K, S, float(eps), stream())
    return out


def ln_gelu_fwd(x2d, gamma, beta, out=None, out_dtype=None, eps=1e-5):
    """gelu(LayerNorm(x) gamma + beta) over the rows of x2d [N, d] (f32 / bf16; d % 8 == 0, d <= 512). out: a
    contiguous [N, d] tensor (x2d itself for in place), or None for a new one of out_dtype (default x2d's)."""
    _chk(x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype in (torch.float32, torch.bfloat16),
         "ln_gelu: x is contiguous f32 / bf16 [N, d]")
    N, d = x2d.shape
    _chk(d % 8 == 0 and 0 < d <= 512, "ln_gelu: d a multiple of 8 up to 512")
    for t in (gamma, beta):
        _chk(t.dtype == torch.float32 and t.numel() == d and t.is_contiguous(), "ln_gelu: gamma and beta are f32 [d]")
    if out is None:
        out = torch.empty(N, d, device=x2d.device, dtype=out_dtype or x2d.dtype)
    _chk(out.is_contiguous() and tuple(out.shape) == (N, d) and out.dtype in (torch.float32, torch.bfloat16),
         "ln_gelu: out is contiguous f32 / bf16 [N, d]")
    _chk(out.data_ptr() != x2d.data_ptr() or out.dtype == x2d.dtype, "ln_gelu: in place needs equal dtypes")
    call("fddm_ln_gelu_fwd", code(x2d), code(out), ptr(x2d), ptr(gamma), ptr(beta), ptr(out), N, d, float(eps),
         stream())
    return out


def wavlm_gate(x2d, W, bias, cst, B, S, H):
    """Gated relative-position gate: x2d [B*S, E] (f32 / bf16), W [8, E/H] f32, bias [8], cst [H] -> [B*H, S] f32."""
    _chk(x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype in (torch.float32, torch.bfloat16),
         "wavlm_gate: x is contiguous f32 / bf16 [B*S, E]")
    _chk(H > 0 and x2d.shape[0] == B * S, "wavlm_gate: x has B*S rows, H > 0")
    E = x2d.shape[1]
    _chk(E % H == 0, "wavlm_gate: E is a multiple of H")
    dh = E // H
    _chk(dh % 8 == 0 and 0 < dh <= 64, "wavlm_gate: head width a multiple of 8, at most 64")
    _chk(W.dtype == torch.float32 and W.is_contiguous() and tuple(W.shape) == (8, dh),
         "wavlm_gate: W is contiguous f32 [8, dh]")
    _chk(bias.dtype == torch.float32 and tuple(bias.shape) == (8,) and bias.is_contiguous(), "wavlm_gate: bias is f32 [8]")
    _chk(cst.dtype == torch.float32 and tuple(cst.shape) == (H,) and cst.is_contiguous(), "wavlm_gate: cst is f32 [H]")
    gate = torch.empty(B * H, S, device=x2d.device, dtype=torch.float32)
    call("fddm_wavlm_gate", code(x2d), ptr(x2d), ptr(W), ptr(bias), ptr(cst), ptr(gate), B, S, H, E, stream())
    return gate


# ------------------------------------------------------------------------------------- attention
def drop_words(B, H, Lq, Lk):
    """u64 words per site of a keep-bit buffer (fddm_attn_drop_words: room for either storage layout)."""
    from ._lib import lib
    return int(lib().fddm_attn_drop_words(B, H, Lq, Lk))


def drop_bits(B, H, Lq, Lk, device):
    """Buffer for one attention site's dropout keep bits (written by attn_drop_bits or by the forward, read by the
    backward; the layout is the selected kernel family's: csrc/attn7.hip layout v3 by default)."""
    return torch.empty(drop_words(B, H, Lq, Lk), device=device, dtype=torch.int64)


def _heads(x, rows, H, dh):
    """[rows, H*dh] view (any row stride) as [rows, H, dh]."""
    return x[:rows, : H * dh].unflatten(1, (H, dh))


def _pad64(x, rows, H, dh):
    """Head slots widened to the kernels' 64 lanes with zeros: [rows, H*64]. Zero q/k columns add nothing to
    Q K^T and zero v columns give zero output columns, so the attention of the first dh columns is unchanged."""
    xp = torch.zeros(rows, H, 64, device=x.device, dtype=x.dtype)
    xp[:, :, :dh] = _heads(x, rows, H, dh)
    return xp.view(rows, H * 64)


def attn_drop_bits(out, nsites, B, H, Lq, Lk, drop_p, seed, stream0, stream_step):
    """The dropout keep-bit words of `nsites` attention sites of one shape (rng streams stream0 + s * stream_step)
    into out [nsites, words] (int64): what attn_fwd(..., dbits=out[s], bits_ready=True) and attn_bwd read."""
    _chk(out.dtype == torch.int64 and out.is_contiguous() and out.dim() == 2 and out.shape[0] >= nsites,
         "drop-bit buffer layout")
    call("fddm_attn_drop_bits", ptr(out), out.shape[1], nsites, B, H, Lq, Lk, float(drop_p), seed, stream0,
         stream_step, stream())
    return out


def _chk_key_len(key_len, key_keep, B, Lk):
    _chk(key_keep is not None, "key_len comes with its key_keep mask")
    _chk(key_keep.dtype == torch.uint8 and key_keep.is_contiguous() and key_keep.numel() == B * Lk,
         "key_keep: contiguous uint8 [B, Lk]")
    _chk(key_len.dtype == torch.int32 and key_len.is_contiguous() and key_len.numel() == B
         and key_len.device == key_keep.device and key_len.is_cuda, "key_len: int32 [B] on the device")


def key_extent(key_keep):
    """key_keep [B, Lk] (uint8, contiguous; != 0 keeps) -> int32 [B]: 1 + the last kept key of each entry, 0 if none
    (fddm_key_extent; one launch, no host sync). The key_len of attn_fwd / attn_bwd / attn_fwd_relgate_x."""
    _chk(key_keep.dtype == torch.uint8 and key_keep.is_contiguous() and key_keep.dim() == 2 and key_keep.is_cuda,
         "key_extent: contiguous uint8 [B, Lk] on the device")
    B, Lk = key_keep.shape
    _chk(Lk >= 1, "key_extent: at least one key")
    out = torch.empty(B, device=key_keep.device, dtype=torch.int32)
    call("fddm_key_extent", ptr(key_keep), B, Lk, ptr(out), stream())
    return out


def attn_fwd(q, k, v, out, lse, B, H, Lq, Lk, *, key_keep=None, gate=None, table=None, drop_p=0.0, seed=0,
             rng_stream=0, scale=None, dbits=None, bits_ready=False, key_len=None):
    """q: [B*Lq, >=H*dh] row stride q.stride(0); k/v: [B*Lk, ...]; out [B*Lq, H*dh]; lse [B*H, Lq], dh =
    out.shape[1] // H. dbits (optional, drop_bits()): the dropout keep bits the backward reads; bits_ready: they
    were already written by attn_drop_bits (the forward only reads them), else the forward writes them.
    The kernels are built for head_dim 64; a smaller head_dim (the reference's nn.MultiheadAttention takes any
    d_model / nhead) runs them on zero-padded 64-wide head slots — the scores, the softmax, the dropout
    element indices (b, h, query, key) and hence the RNG stream are those of the unpadded heads.
    key_len (optional, key_extent(key_keep)): selects fddm_attn_fwd_kx, whose bf16 kernels stop each entry's key
    tiles at its extent (same result as key_keep alone; fp32, Lk > 1024 and the padded small heads ignore it)."""
    _chk(q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "attention inputs need unit inner stride")
    _chk(q.dtype == k.dtype == v.dtype == out.dtype, "attention dtype mismatch")
    _chk(out.shape[1] % H == 0, "attention output width must be H * head_dim")
    _chk(table is None or gate is not None, "a relative-position bias table needs its gate")
    dh = out.shape[1] // H
    _chk(1 <= dh <= 64, f"head_dim {dh} > 64 is not built")
    if key_len is not None:
        _chk_key_len(key_len, key_keep, B, Lk)
    sc = 1.0 / math.sqrt(dh) if scale is None else scale
    if dh != 64:
        op = torch.empty(B * Lq, H * 64, device=out.device, dtype=out.dtype)
        attn_fwd(_pad64(q, B * Lq, H, dh), _pad64(k, B * Lk, H, dh), _pad64(v, B * Lk, H, dh), op, lse, B, H, Lq,
                 Lk, key_keep=key_keep, gate=gate, table=table, drop_p=drop_p, seed=seed, rng_stream=rng_stream,
                 scale=sc, dbits=dbits, bits_ready=bits_ready)
        _heads(out, B * Lq, H, dh).copy_(op.view(B * Lq, H, 64)[:, :, :dh])
        return out
    if key_len is not None:
        call("fddm_attn_fwd_kx", code(q), ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
             out.stride(0), ptr(lse), ptr(key_keep), ptr(key_len), ptr(gate), ptr(table), B, H, Lq, Lk, float(sc),
             float(drop_p), seed, rng_stream, ptr(dbits), int(bool(bits_ready) and dbits is not None), stream())
        return out
    call("fddm_attn_fwd", code(q), ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
         out.stride(0), ptr(lse), ptr(key_keep), ptr(gate), ptr(table), B, H, Lq, Lk, float(sc), float(drop_p), seed,
         rng_stream, ptr(dbits), int(bool(bits_ready) and dbits is not None), stream())
    return out


def attn_fwd_relgate_x(q, k, v, out, x, gw, gconst, table, B, H, L, scale=None, key_keep=None, key_len=None):
    """WavLM attention (bf16) with the gate computed in the kernel from the attention input x [B*L, H*64] (bf16, row
    stride x.stride(0)) and the folded gru_rel_pos_linear weights gw (130 floats: sum of weight rows 0-3, rows 4-7,
    the two bias sums; models/wavlm.py). key_keep [B, L] (uint8) with key_len = key_extent(key_keep): the key-padding
    mask of a padded batch (fddm_attn_fwd_relgate_x_kx); both or neither."""
    _chk((key_keep is None) == (key_len is None), "relgate attention: key_keep and key_len come together")
    _chk(q.dtype == k.dtype == v.dtype == out.dtype == x.dtype == torch.bfloat16, "relgate attention is bf16")
    _chk(x.stride(-1) == 1 and x.shape[1] >= H * 64 and x.data_ptr() % 16 == 0, "gate input layout")
    _chk(gw.dtype == torch.float32 and gw.numel() >= 130 and gw.is_contiguous() and gw.data_ptr() % 16 == 0,
         "folded gate weights")
    sc = 1.0 / math.sqrt(64) if scale is None else scale
    if key_len is not None:
        _chk_key_len(key_len, key_keep, B, L)
        call("fddm_attn_fwd_relgate_x_kx", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
             out.stride(0), ptr(x), x.stride(0), ptr(gw), ptr(gconst), ptr(table), ptr(key_keep), ptr(key_len), B, H,
             L, L, float(sc), stream())
        return out
    call("fddm_attn_fwd_relgate_x", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
         out.stride(0), ptr(x), x.stride(0), ptr(gw), ptr(gconst), ptr(table), B, H, L, L, float(sc), stream())
    return out


def attn_fwd_relgate(q, k, v, out, graw, gconst, table, B, H, L, scale=None):
    """WavLM attention (bf16) with the gate computed in the kernel from graw [B*L, >= H*8] (row stride
    graw.stride(0)): 8 gru_rel_pos_linear pre-activations per (token, head)."""
    _chk(q.dtype == k.dtype == v.dtype == out.dtype == graw.dtype == torch.bfloat16, "relgate attention is bf16")
    _chk(graw.stride(-1) == 1 and graw.shape[1] >= H * 8 and graw.data_ptr() % 16 == 0, "graw layout")
    sc = 1.0 / math.sqrt(64) if scale is None else scale
    call("fddm_attn_fwd_relgate", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
         out.stride(0), ptr(graw), graw.stride(0), ptr(gconst), ptr(table), B, H, L, L, float(sc), stream())
    return out


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Lq, Lk, *, key_keep=None, drop_p=0.0, seed=0, rng_stream=0,
             dbits=None, scale=None, key_len=None, ws=None):
    """Gradients of attn_fwd (same layouts; head_dim = o.shape[1] // H, padded to 64 as in attn_fwd). key_len as in
    attn_fwd (fddm_attn_bwd_kx: dk / dv rows at or past an entry's extent are exact zeros). ws (optional): the
    workspace to use instead of a fresh one, f32 with at least fddm_attn_bwd_ws_floats elements (the kernels write
    every float they read back, so its contents do not matter; tests pass a NaN-filled one)."""
    _chk(o.shape[1] % H == 0, "attention output width must be H * head_dim")
    dh = o.shape[1] // H
    _chk(1 <= dh <= 64, f"head_dim {dh} > 64 is not built")
    if key_len is not None:
        _chk_key_len(key_len, key_keep, B, Lk)
    sc = 1.0 / math.sqrt(dh) if scale is None else scale
    if dh != 64:
        rq, rk = B * Lq, B * Lk
        dqp = torch.empty(rq, H * 64, device=dq.device, dtype=dq.dtype)
        dkp = torch.empty(rk, H * 64, device=dk.device, dtype=dk.dtype)
        dvp = torch.empty(rk, H * 64, device=dv.device, dtype=dv.dtype)
        attn_bwd(_pad64(q, rq, H, dh), _pad64(k, rk, H, dh), _pad64(v, rk, H, dh), _pad64(o, rq, H, dh),
                 _pad64(do, rq, H, dh), lse, dqp, dkp, dvp, B, H, Lq, Lk, key_keep=key_keep, drop_p=drop_p, seed=seed,
                 rng_stream=rng_stream, dbits=dbits, scale=sc)
        for g, gp, r in ((dq, dqp, rq), (dk, dkp, rk), (dv, dvp, rk)):
            _heads(g, r, H, dh).copy_(gp.view(r, H, 64)[:, :, :dh])
        return
    # row-term workspace: delta = rowsum(dO O) and -LSE log2(e) per query, [2][B*H][Lq rounded up to 64] (the
    # 32x32x16 backward's layout; the other kernels use the first B*H*Lq floats)
    nws = int(lib().fddm_attn_bwd_ws_floats(B, H, Lq, Lk))
    if ws is not None:
        _chk(ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= nws and ws.device == q.device,
             "attention backward workspace: contiguous f32, fddm_attn_bwd_ws_floats elements")
    delta = ws if ws is not None else torch.empty(nws, device=q.device, dtype=torch.float32)
    if key_len is not None:
        call("fddm_attn_bwd_kx", code(q), ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(o),
             o.stride(0), ptr(do), do.stride(0), ptr(lse), ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv),
             dv.stride(0), ptr(delta), ptr(key_keep), ptr(key_len), B, H, Lq, Lk, float(sc), float(drop_p), seed,
             rng_stream, ptr(dbits), stream())
        return
    call("fddm_attn_bwd", code(q), ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(o),
         o.stride(0), ptr(do), do.stride(0), ptr(lse), ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv),
         dv.stride(0), ptr(delta), ptr(key_keep), B, H, Lq, Lk, float(sc), float(drop_p), seed, rng_stream,
         ptr(dbits), stream())


# ----------------------------------------------------------------------------------- layernorm
_LN_FWD_BUILDS = ((torch.float32, torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32, torch.float32),
                  (torch.bfloat16, torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32, torch.bfloat16))
_FLOATS = (torch.float32, torch.bfloat16)


def _chk_rows(name, what, t, N, d, dtypes, dev):
    """t is None or a contiguous [N, d] tensor of one of dtypes on dev (the kernels index it from a raw pointer)."""
    _chk(t is None or (t.dim() == 2 and t.shape[0] == N and t.shape[1] == d and t.is_contiguous() and t.dtype in dtypes
                       and t.device == dev),
         f"{name}: {what} is contiguous [N, d], " + " or ".join(str(x)[6:] for x in dtypes) + ", on the input's GPU")


def _chk_vec(name, what, t, n, dev, at_least=False):
    """t is None or a contiguous f32 tensor of n elements (at_least: n or more) on dev."""
    _chk(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                       and (t.numel() >= n if at_least else t.numel() == n)),
         f"{name}: {what} is contiguous float32 with {'>= ' if at_least else ''}{n} elements, on the input's GPU")


def _chk_film(name, what, pair, N, d, rows_per_batch, dev):
    """pair is None or two contiguous f32 [B, d] tensors with N == B rows_per_batch."""
    if pair is None:
        return
    _chk(len(pair) == 2 and all(t is not None and t.dim() == 2 and t.shape[1] == d and t.dtype == torch.float32
                                and t.is_contiguous() and t.device == dev for t in pair)
         and pair[0].shape[0] == pair[1].shape[0], f"{name}: {what} is a pair of contiguous float32 [B, d], on the input's GPU")
    _chk(rows_per_batch > 0 and pair[0].shape[0] * rows_per_batch == N, f"{name}: N == B * rows_per_batch for {what}")


def ln_fwd(x, y, gamma, beta, *, out_f32=None, out_t=None, save_s=None, mean=None, rstd=None, film=None,
           rows_per_batch=0, eps=1e-5, drop_p=0.0, seed=0, rng_stream=0, rope=None):
    """x [N, d] f32 / bf16, y None or [N, d], gamma / beta f32 [d], film = (scale, shift) f32 [B, d] with N == B
    rows_per_batch; out_f32 / save_s f32 [N, d], out_t [N, d] in a dtype a build exists for ((x, y, out_t) = (f32, bf16,
    bf16), (f32, f32, f32), (bf16, bf16, bf16), (f32, f32, bf16); without y its dtype counts as x's), mean / rstd f32, N
    elements; d a multiple of 8 up to 1024; every tensor contiguous and on one GPU.
    rope = (cos [>= L, d], sin [>= L, d], out bf16 [N, d], L): also write RoPE(output) — rope_fwd of the output — for the
    decoder's next block (f32 x, bf16 y and out_t, no FiLM)."""
    _chk(x.dim() == 2 and x.is_contiguous() and x.dtype in _FLOATS and x.is_cuda, "ln_fwd: x is contiguous [N, d], float32 or bfloat16, on a GPU")
    N, d = x.shape
    dev = x.device
    _chk(d > 0 and d % 8 == 0 and d <= 1024, "ln_fwd: d is a multiple of 8 in [8, 1024]")
    _chk_rows("ln_fwd", "y", y, N, d, _FLOATS, dev)
    _chk_vec("ln_fwd", "gamma", gamma, d, dev)
    _chk_vec("ln_fwd", "beta", beta, d, dev)
    _chk(gamma is not None and beta is not None, "ln_fwd: gamma and beta are given")
    _chk_film("ln_fwd", "film", film, N, d, rows_per_batch, dev)
    _chk_rows("ln_fwd", "out_f32", out_f32, N, d, (torch.float32,), dev)
    _chk_rows("ln_fwd", "save_s", save_s, N, d, (torch.float32,), dev)
    _chk_rows("ln_fwd", "out_t", out_t, N, d, _FLOATS, dev)
    _chk_vec("ln_fwd", "mean", mean, N, dev)
    _chk_vec("ln_fwd", "rstd", rstd, N, dev)
    ydt = y.dtype if y is not None else x.dtype
    odt = out_t.dtype if out_t is not None else ydt
    _chk((x.dtype, ydt, odt) in _LN_FWD_BUILDS, "ln_fwd: no build for these dtypes of x, y and out_t")
    fs, fh = film if film is not None else (None, None)
    rc, rs, ro, rl = rope if rope is not None else (None, None, None, 0)
    if rope is not None:
        _chk(rl >= 1 and d % 16 == 0 and y is not None and film is None and
             (x.dtype, ydt, odt) == _LN_FWD_BUILDS[0], "ln_fwd: rope needs f32 x, bf16 y and out_t, no film, d % 16 == 0, L >= 1")
        _chk_rows("ln_fwd", "rope out", ro, N, d, (torch.bfloat16,), dev)
        for t in (rc, rs):
            _chk(t is not None and t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == d
                 and t.shape[0] >= rl and t.device == dev, "ln_fwd: rope cos and sin are contiguous float32 [>= L, d]")
    call("fddm_ln_fwd", code(x), code(y) if y is not None else code(x), code(out_t) if out_t is not None else
         (code(y) if y is not None else code(x)), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(fs), ptr(fh),
         ptr(out_f32), ptr(out_t), ptr(save_s), ptr(mean), ptr(rstd), N, d, rows_per_batch, float(eps), float(drop_p),
         seed, rng_stream, ptr(rc), ptr(rs), ptr(ro), rl, stream())


def ln_bwd(dout, s, mean, rstd, gamma, beta, *, dres=None, dy_t=None, dgamma=None, dbeta=None, film_scale=None,
           dfilm=None, rows_per_batch=0, drop_p=0.0, seed=0, rng_stream=0, partials=None):
    """dout, s f32 [N, d] (d <= 1024), mean / rstd f32 with N elements, gamma / beta f32 [d]; dres f32 [N, d], dy_t
    [N, d] f32 / bf16, dgamma / dbeta f32 [d] (added to), film_scale f32 [B, d] and dfilm = (dscale, dshift) f32 [B, d]
    with N == B rows_per_batch; every tensor contiguous and on one GPU.
    partials: a LnPartials (ln_partials) collecting this LayerNorm's dgamma / dbeta slab sums for one ln_fold launch
    (the fused pass only), or None: the sums are added to dgamma / dbeta with atomics."""
    _chk(dout.dim() == 2 and dout.is_contiguous() and dout.dtype == torch.float32 and dout.is_cuda,
         "ln_bwd: dout is contiguous float32 [N, d], on a GPU")
    N, d = dout.shape
    dev = dout.device
    _chk(0 < d <= 1024, "ln_bwd: d is in [1, 1024]")
    _chk(s is not None and mean is not None and rstd is not None and gamma is not None, "ln_bwd: s, mean, rstd and gamma are given")
    _chk_rows("ln_bwd", "s", s, N, d, (torch.float32,), dev)
    _chk_vec("ln_bwd", "mean", mean, N, dev)
    _chk_vec("ln_bwd", "rstd", rstd, N, dev)
    _chk_vec("ln_bwd", "gamma", gamma, d, dev)
    _chk_vec("ln_bwd", "beta", beta, d, dev)
    _chk_rows("ln_bwd", "dres", dres, N, d, (torch.float32,), dev)
    _chk_rows("ln_bwd", "dy_t", dy_t, N, d, _FLOATS, dev)
    _chk_vec("ln_bwd", "dgamma", dgamma, d, dev)
    _chk_vec("ln_bwd", "dbeta", dbeta, d, dev)
    _chk((dgamma is None) == (dbeta is None), "ln_bwd: dgamma and dbeta come as a pair")
    wants = dgamma is not None or dfilm is not None
    _chk(not wants or beta is not None, "ln_bwd: parameter gradients need beta")
    _chk(film_scale is not None or dfilm is None, "ln_bwd: dfilm needs film_scale")
    if film_scale is not None:
        _chk_film("ln_bwd", "film_scale", (film_scale, film_scale), N, d, rows_per_batch, dev)
        _chk(not wants or dfilm is not None, "ln_bwd: with film_scale, parameter gradients need dfilm")
        _chk_film("ln_bwd", "dfilm", dfilm, N, d, rows_per_batch, dev)
        _chk(dfilm is None or dfilm[0].shape == film_scale.shape, "ln_bwd: dfilm has film_scale's shape")
    dfs, dfh = dfilm if dfilm is not None else (None, None)
    part = None
    if partials is not None:
        _chk(dgamma is not None and dbeta is not None, "ln_bwd partials need dgamma and dbeta")
        part = partials.add(N, d, dgamma, dbeta, (dfs, dfh) if film_scale is not None else None, rows_per_batch)
    call("fddm_ln_bwd", code(dy_t) if dy_t is not None else F32, ptr(dout), ptr(s), ptr(mean), ptr(rstd), ptr(gamma),
         ptr(beta), ptr(film_scale), ptr(dres), ptr(dy_t), ptr(dgamma), ptr(dbeta), ptr(dfs), ptr(dfh), N, d,
         rows_per_batch, float(drop_p), seed, rng_stream, ptr(part), stream())


class LnPartials:
    """The dgamma / dbeta slab sums of up to 4 LayerNorm backwards (ln_bwd(partials=...)), added to their
    destinations by one ln_fold launch: the slab atomics of ~5 us per LayerNorm backward become one short fold."""

    def __init__(self):
        self.jobs = []

    def add(self, N, d, dgamma, dbeta, dfilm=None, rows_per_batch=0):
        """dfilm = (dfs, dfh) [B, d] with FiLM batches of rows_per_batch rows: folded per batch when the batches
        are whole slabs (the fused pass); otherwise the backward adds them with atomics and leaves zeros here."""
        _chk(len(self.jobs) < 4, "at most 4 LayerNorms per fold")
        _chk(N > 0 and 0 < d <= 1024, "LnPartials.add: N > 0 and d in [1, 1024]")
        _chk(dgamma is not None and dbeta is not None and dgamma.is_cuda, "LnPartials.add: dgamma and dbeta are given, on a GPU")
        _chk_vec("LnPartials.add", "dgamma", dgamma, d, dgamma.device)
        _chk_vec("LnPartials.add", "dbeta", dbeta, d, dgamma.device)
        _chk_film("LnPartials.add", "dfilm", dfilm, N, d, rows_per_batch, dgamma.device)
        rows = lib().fddm_ln_bwd_slab_rows()
        nslab = (N + rows - 1) // rows
        part = torch.empty(nslab, 4, d, device=dgamma.device, dtype=torch.float32)
        dfs = dfh = None
        spb = 0
        if dfilm is not None and rows_per_batch > 0 and rows_per_batch % rows == 0:
            dfs, dfh = dfilm
            spb = rows_per_batch // rows
        self.jobs.append((part, nslab, d, dgamma, dbeta, dfs, dfh, spb))
        return part

    def fold(self):
        import ctypes
        n = len(self.jobs)
        if n == 0:
            return
        P = ctypes.c_void_p * n
        Lg = ctypes.c_long * n
        J = self.jobs
        call("fddm_ln_fold", n, P(*[j[0].data_ptr() for j in J]), Lg(*[j[1] for j in J]), Lg(*[j[2] for j in J]),
             P(*[j[3].data_ptr() for j in J]), P(*[j[4].data_ptr() for j in J]), P(*[ptr(j[5]) for j in J]),
             P(*[ptr(j[6]) for j in J]), Lg(*[j[7] for j in J]), stream())
        self.jobs = []


# -------------------------------------------------------------------------------- small kernels
_F32 = torch.float32


def _chk_rope(name, x, cs, sn, out, L, out_dtypes):
    """The shared preconditions of rope_fwd / rope_bwd: the kernels index every tensor as contiguous [N, d] /
    [L, d] rows from a raw pointer, positions are r % L."""
    _chk(x.dim() == 2 and x.dtype == _F32 and x.is_contiguous(), f"{name}: input is contiguous f32 [N, d]")
    N, d = x.shape
    _chk(d % 2 == 0, f"{name}: d is even")
    _chk(L >= 1, f"{name}: L >= 1")
    _chk(out.shape == x.shape and out.is_contiguous() and out.dtype in out_dtypes,
         f"{name}: output is contiguous [N, d], " + " or ".join(str(t)[6:] for t in out_dtypes))
    for t in (cs, sn):
        _chk(t.dim() == 2 and t.dtype == _F32 and t.is_contiguous() and t.shape[1] == d and t.shape[0] >= L,
             f"{name}: cos and sin are contiguous f32 [>= L, d]")
    _chk(x.device == out.device == cs.device == sn.device and x.is_cuda, f"{name}: every tensor on one GPU")
    return N, d


def rope_fwd(x, cs, sn, out, L):
    """out = RoPE(x), row r at position r % L: x f32 [N, d] (d even), cs / sn f32 [>= L, d], out [N, d] f32 or bf16;
    every tensor contiguous and on one device."""
    N, d = _chk_rope("rope_fwd", x, cs, sn, out, L, (torch.float32, torch.bfloat16))
    call("fddm_rope_fwd", code(out), ptr(x), ptr(cs), ptr(sn), ptr(out), N, L, d, stream())
    return out


def rope_bwd(dy, cs, sn, dx, L):
    """dx += RoPE^T(dy): dy, dx f32 [N, d] (d even), cs / sn f32 [>= L, d]; every tensor contiguous and on one
    device."""
    N, d = _chk_rope("rope_bwd", dy, cs, sn, dx, L, (torch.float32,))
    call("fddm_rope_bwd", ptr(dy), ptr(cs), ptr(sn), ptr(dx), N, L, d, stream())


def _chk_embed(name, tok, E, tb, tb_name, L, d, rows):
    """The shared preconditions of embed_fwd / embed_bwd: E (or dE) [V, d] and tb (tbias or dtb) may be None where the
    kernel allows it; rows: (name, [N, d] tensor or None, dtypes). Returns N, the token count."""
    _chk(tok.dtype == torch.int64 and tok.is_contiguous(), f"{name}: tokens are contiguous int64")
    N, dev = tok.numel(), tok.device
    _chk(L >= 1, f"{name}: L >= 1")
    _chk(E is None or (E.dim() == 2 and E.dtype == _F32 and E.is_contiguous() and E.shape[1] == d),
         f"{name}: the table is contiguous f32 [V, d]")
    _chk(tb is None or (tb.dim() == 2 and tb.dtype == _F32 and tb.is_contiguous() and tb.shape[1] == d
                        and tb.shape[0] * L >= N), f"{name}: {tb_name} is contiguous f32 [>= ceil(N / L), d]")
    for nm, t, dts in rows:
        _chk(t is None or (tuple(t.shape) == (N, d) and t.is_contiguous() and t.dtype in dts),
             f"{name}: {nm} is contiguous [N, d], " + " or ".join(str(x)[6:] for x in dts))
    _chk(tok.is_cuda and all(t is None or t.device == dev for t in (E, tb) + tuple(r[1] for r in rows)),
         f"{name}: every tensor on one GPU")
    return N


def embed_fwd(tok, E, tbias, out, out_t, L):
    """out[r] = E[tok[r]] + tbias[r // L] (f32; out_t: the same value in f32 / bf16; either may be None): tok int64 (N
    of them), E f32 [V, d], tbias None or f32 [>= ceil(N / L), d], out / out_t [N, d]; every tensor contiguous and on
    one device. Token ids outside [0, V) cannot be refused here: checking them needs their values, a device read
    and a stream synchronisation on the step's critical path; they index E unchecked and are the caller's to
    exclude."""
    _chk(E is not None and E.dim() == 2, "embed_fwd: the table is contiguous f32 [V, d]")
    d = E.shape[1]
    N = _chk_embed("embed_fwd", tok, E, tbias, "tbias", L, d,
                   (("out", out, (_F32,)), ("out_t", out_t, (_F32, torch.bfloat16))))
    call("fddm_embed_fwd", code(out_t) if out_t is not None else F32, ptr(tok), ptr(E), ptr(tbias), ptr(out),
         ptr(out_t), N, L, d, stream())


def embed_bwd(tok, dx, dE, dtb, L, pad_id):
    """dE[tok[r]] += dx[r] for tok[r] != pad_id, dtb[r // L] += dx[r] (either may be None): tok int64 (N of them), dx
    f32 [N, d], dE f32 [V, d], dtb f32 [>= ceil(N / L), d]; every tensor contiguous and on one device. Token ids
    outside [0, V) are not checked (see embed_fwd)."""
    _chk(dx is not None and dx.dim() == 2, "embed_bwd: dx is contiguous [N, d], float32")
    d = dx.shape[1]
    N = _chk_embed("embed_bwd", tok, dE, dtb, "dtb", L, d, (("dx", dx, (_F32,)),))
    call("fddm_embed_bwd", ptr(tok), ptr(dx), ptr(dE), ptr(dtb), N, L, d, pad_id, stream())


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    call("fddm_cast", code(x), code(out), ptr(x), ptr(out), x.numel(), stream())
    return out


def sample_q(x0, t, thr, K, seed, rng_stream=1):
    B, L = x0.shape
    xt = torch.empty_like(x0)
    call("fddm_sample_q", ptr(x0), ptr(t), ptr(thr), ptr(xt), B, L, K, seed, rng_stream, stream())
    return xt


# Vocabulary limits of the row kernels (one workgroup holds a whole row in registers; include/fddm_hip.h, KL section)
KL_VEC_MAX_V = 32768        # fddm_kl_fwd/_bwd float4 kernels: V % 4 == 0 and 16-byte-aligned rows
KL_SCALAR_MAX_V = 16384     # fddm_kl_fwd/_bwd scalar kernel (any V, any alignment): 256 threads x 64 elements
KL_FUSED_MAX_V = 32768      # fddm_kl_fused (V % 4 == 0, aligned rows only): 512 threads x 16 float4 per row
SOFTMAX_MAX_V = 16384       # fddm_softmax_rows/_bwd_rows: 256 threads x 64 elements
SOFTMAX_ADD_MAX_V = 32768   # fddm_softmax_bwd_add_bf16 (V % 8 == 0): 256 threads x 16 loads of 8 bf16
WIDE_MAX_V = 1 << 24        # the streamed *_wide forms: 2 <= V <= 2^24 ((float)V exact), any V % 4, any alignment


def _chk_kl_vocab(name, V, *bufs):
    vec = V % 4 == 0 and all(b is None or b.data_ptr() % 16 == 0 for b in bufs)
    if V > (KL_VEC_MAX_V if vec else KL_SCALAR_MAX_V):
        raise ValueError(f"{name}: V = {V} is outside the supported range V <= {KL_VEC_MAX_V} (V % 4 == 0 and "
                         f"16-byte-aligned rows) or V <= {KL_SCALAR_MAX_V} (otherwise)")


def kl_fwd(logits2d, xt, x0, t, betas, L):
    N, V = logits2d.shape
    _chk_kl_vocab("kl_fwd", V, logits2d)
    kl = torch.empty(N, device=logits2d.device, dtype=torch.float32)
    call("fddm_kl_fwd", ptr(logits2d), ptr(xt), ptr(x0), ptr(t), ptr(betas), ptr(kl), N, L, V, stream())
    return kl


def kl_bwd(logits2d, xt, x0, t, betas, w, gscale, L, out_dtype=torch.float32):
    N, V = logits2d.shape
    dz = torch.empty(N, V, device=logits2d.device, dtype=out_dtype)
    _chk_kl_vocab("kl_bwd", V, logits2d, dz)
    call("fddm_kl_bwd", ptr(logits2d), ptr(xt), ptr(x0), ptr(t), ptr(betas), ptr(w), ptr(gscale), ptr(dz),
         code(dz), N, L, V, stream())
    return dz


def kl_fused(logits2d, xt, x0, t, betas, mask_u8, L, out_dtype=torch.float32):
    """(kl_tok [N] f32, dz [N, V]) in one pass: dz = w * d kl_tok / d logits with kl_reduce's weights w (from the
    uint8 mask [N], or None = plain mean over L); the upstream gradient is applied later by scale_if."""
    N, V = logits2d.shape
    _chk(logits2d.dtype == torch.float32 and logits2d.is_contiguous() and N % L == 0, "kl_fused: f32 [B*L, V] rows")
    _chk(mask_u8 is None or (mask_u8.numel() == N and mask_u8.dtype == torch.uint8), "kl_fused mask")
    kl = torch.empty(N, device=logits2d.device, dtype=torch.float32)
    dz = torch.empty(N, V, device=logits2d.device, dtype=out_dtype)
    call("fddm_kl_fused", ptr(logits2d), ptr(xt), ptr(x0), ptr(t), ptr(betas), ptr(mask_u8), ptr(kl), ptr(dz),
         code(dz), N, L, V, stream())
    return kl, dz


def scale_if(x, g):
    """x *= g (a device scalar), in place; no memory traffic when g == 1."""
    _chk(x.is_contiguous() and g.dtype == torch.float32 and g.numel() == 1, "scale_if operands")
    call("fddm_scale_if", ptr(x), code(x), ptr(g), x.numel(), stream())
    return x


def softmax_bwd_add_bf16(y, dy, add, out=None):
    """out = bf16(y * (dy - rowsum(y*dy)) + add), all bf16 [N, V] (out may be `add`)."""
    N, V = y.shape
    _chk(all(t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (N, V) for t in (y, dy, add)),
         "softmax_bwd_add_bf16 operands")
    if out is None:
        out = torch.empty_like(y)
    call("fddm_softmax_bwd_add_bf16", ptr(y), ptr(dy), ptr(add), ptr(out), N, V, stream())
    return out


def axpy_if_bf16(x, y, g):
    """x += (g - 1) * y in place (bf16), no memory traffic when the device scalar g == 1."""
    _chk(x.dtype == y.dtype == torch.bfloat16 and x.numel() == y.numel() and x.is_contiguous() and y.is_contiguous(),
         "axpy_if_bf16 operands")
    call("fddm_axpy_if_bf16", ptr(x), ptr(y), ptr(g), x.numel(), stream())
    return x


def _chk_softmax_vocab(name, V):
    if V > SOFTMAX_MAX_V:
        raise ValueError(f"{name}: V = {V} is outside the supported range V <= {SOFTMAX_MAX_V}")


def softmax_rows(x2d, out_dtype):
    N, V = x2d.shape
    _chk_softmax_vocab("softmax_rows", V)
    y =torch.empty(N, V, device=x2d.device, dtype=out_dtype)
    call("fddm_softmax_rows", ptr(x2d), ptr(y), code(y), N, V, stream())
    return y


def softmax_bwd_rows(y, dy, dz=None, accumulate=False):
    N, V = y.shape
    _chk_softmax_vocab("softmax_bwd_rows", V)
    if dz is None:
        dz = torch.empty(N, V, device=y.device, dtype=torch.float32)
    call("fddm_softmax_bwd_rows", ptr(y), ptr(dy), ptr(dz), code(y), N, V, int(accumulate), stream())
    return dz


# ---- the streamed forms (csrc/kl.hip, "wide" kernels): any 2 <= V <= WIDE_MAX_V, any alignment. The kernels index
# every operand as contiguous [N, V] rows from a raw pointer, so each wrapper checks shape, dtype, layout and device.
def _chk_wide_vocab(name, V):
    if not 2 <= V <= WIDE_MAX_V:
        raise ValueError(f"{name}: V = {V} is outside the supported range 2 <= V <= {WIDE_MAX_V}")


def _chk_wide_rows(name, what, t, N, V, dtypes, dev):
    _chk(t.dim() == 2 and tuple(t.shape) == (N, V) and t.is_contiguous() and t.dtype in dtypes and t.device == dev,
         f"{name}: {what} is contiguous [N, V], " + " or ".join(str(x)[6:] for x in dtypes) + ", on the input's GPU")


def _chk_wide_kl(name, logits2d, xt, x0, t, betas, L):
    _chk(logits2d.dim() == 2, f"{name}: logits are [B*L, V]")
    N, V = logits2d.shape
    _chk_wide_vocab(name, V)
    dev = logits2d.device
    _chk(logits2d.is_cuda, f"{name}: logits are on a GPU")
    _chk_wide_rows(name, "logits", logits2d, N, V, (_F32,), dev)
    _chk(L > 0 and N % L == 0, f"{name}: N is a multiple of L > 0")
    for what, i, n in (("xt", xt, N), ("x0", x0, N), ("t", t, N // L)):
        _chk(i.dtype == torch.long and i.numel() == n and i.is_contiguous() and i.device == dev,
             f"{name}: {what} holds {n} contiguous int64 on the logits' GPU")
    _chk(betas.dtype == _F32 and betas.is_contiguous() and betas.device == dev, f"{name}: betas are contiguous f32")
    return N, V


def kl_fwd_wide(logits2d, xt, x0, t, betas, L, kl_tok=None):
    """kl_tok [N] f32 as kl_fwd, the row streamed (any V up to WIDE_MAX_V, any alignment)."""
    N, V = _chk_wide_kl("kl_fwd_wide", logits2d, xt, x0, t, betas, L)
    if kl_tok is None:
        kl_tok = torch.empty(N, device=logits2d.device, dtype=_F32)
    _chk(kl_tok.dtype == _F32 and kl_tok.numel() == N and kl_tok.is_contiguous() and kl_tok.device == logits2d.device,
         "kl_fwd_wide: kl_tok is contiguous f32 [N]")
    call("fddm_kl_fwd_wide", ptr(logits2d), ptr(xt), ptr(x0), ptr(t), ptr(betas), ptr(kl_tok), N, L, V, stream())
    return kl_tok


def kl_fused_wide(logits2d, xt, x0, t, betas, mask_u8, L, out_dtype=torch.float32, kl_tok=None, dz=None):
    """(kl_tok [N] f32, dz [N, V]) as kl_fused, the row streamed: also V % 4 != 0 and rows that are not 16-byte
    aligned. kl_tok / dz: optional destinations (dz decides the output dtype)."""
    N, V = _chk_wide_kl("kl_fused_wide", logits2d, xt, x0, t, betas, L)
    dev = logits2d.device
    _chk(mask_u8 is None or (mask_u8.numel() == N and mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
                             and mask_u8.device == dev), "kl_fused_wide: mask is contiguous uint8 [N]")
    if kl_tok is None:
        kl_tok = torch.empty(N, device=dev, dtype=_F32)
    if dz is None:
        dz = torch.empty(N, V, device=dev, dtype=out_dtype)
    _chk(kl_tok.dtype == _F32 and kl_tok.numel() == N and kl_tok.is_contiguous() and kl_tok.device == dev,
         "kl_fused_wide: kl_tok is contiguous f32 [N]")
    _chk_wide_rows("kl_fused_wide", "dz", dz, N, V, _FLOATS, dev)
    call("fddm_kl_fused_wide", ptr(logits2d), ptr(xt), ptr(x0), ptr(t), ptr(betas), ptr(mask_u8), ptr(kl_tok),
         ptr(dz), code(dz), N, L, V, stream())
    return kl_tok, dz


def softmax_rows_wide(x2d, out_dtype, out=None):
    _chk(x2d.dim() == 2 and x2d.is_cuda, "softmax_rows_wide: the input is [N, V] on a GPU")
    N, V = x2d.shape
    _chk_wide_vocab("softmax_rows_wide", V)
    _chk_wide_rows("softmax_rows_wide", "x", x2d, N, V, (_F32,), x2d.device)
    if out is None:
        out = torch.empty(N, V, device=x2d.device, dtype=out_dtype)
    _chk_wide_rows("softmax_rows_wide", "out", out, N, V, _FLOATS, x2d.device)
    call("fddm_softmax_rows_wide", ptr(x2d), ptr(out), code(out), N, V, stream())
    return out


def softmax_bwd_rows_wide(y, dy, dz=None, accumulate=False):
    _chk(y.dim() == 2 and y.is_cuda, "softmax_bwd_rows_wide: y is [N, V] on a GPU")
    N, V = y.shape
    _chk_wide_vocab("softmax_bwd_rows_wide", V)
    _chk_wide_rows("softmax_bwd_rows_wide", "y", y, N, V, _FLOATS, y.device)
    _chk_wide_rows("softmax_bwd_rows_wide", "dy", dy, N, V, (y.dtype,), y.device)
    _chk(dz is not None or not accumulate, "softmax_bwd_rows_wide: accumulate needs dz")
    if dz is None:
        dz = torch.empty(N, V, device=y.device, dtype=_F32)
    _chk_wide_rows("softmax_bwd_rows_wide", "dz", dz, N, V, (_F32,), y.device)
    call("fddm_softmax_bwd_rows_wide", ptr(y), ptr(dy), ptr(dz), code(y), N, V, int(accumulate), stream())
    return dz


def softmax_bwd_add_bf16_wide(y, dy, add, out=None):
    """out = bf16(y * (dy - rowsum(y*dy)) + add), all bf16 [N, V], V % 8 == 0 (out may be `add`), the row streamed."""
    _chk(y.dim() == 2 and y.is_cuda, "softmax_bwd_add_bf16_wide: y is [N, V] on a GPU")
    N, V = y.shape
    _chk_wide_vocab("softmax_bwd_add_bf16_wide", V)
    _chk(V % 8 == 0, "softmax_bwd_add_bf16_wide: V % 8 == 0")
    if out is None:
        out = torch.empty_like(y)
    for what, t in (("y", y), ("dy", dy), ("add", add), ("out", out)):
        _chk_wide_rows("softmax_bwd_add_bf16_wide", what, t, N, V, (torch.bfloat16,), y.device)
        _chk(t.data_ptr() % 16 == 0, f"softmax_bwd_add_bf16_wide: {what} is 16-byte aligned")
    call("fddm_softmax_bwd_add_bf16_wide", ptr(y), ptr(dy), ptr(add), ptr(out), N, V, stream())
    return out


def _chk_lfd(name, z, zt=None, vecs=()):
    """z: contiguous f32 [B, C] on a GPU; zt: B C contiguous f32 / bf16 elements; vecs: (what, tensor, n) f32 with n elements
    (None allowed where the kernel allows it)."""
    _chk(z.dim() == 2 and z.dtype == torch.float32 and z.is_contiguous() and z.is_cuda,
         f"{name}: the input is contiguous float32 [B, C], on a GPU")
    B, C = z.shape
    _chk(B > 0, f"{name}: B > 0")
    _chk(zt is None or (zt.numel() == B * C and zt.is_contiguous() and zt.dtype in _FLOATS and zt.device == z.device),
         f"{name}: z~ is contiguous [B, C], float32 or bfloat16, on the input's GPU")
    for what, t, n in vecs:
        _chk_vec(name, what, t, n, z.device)
    return B, C


def _chk_lfd_dtype(name, dt):
    _chk(dt in _FLOATS, f"{name}: the output dtype is float32 or bfloat16")


def lfd_std_fwd(z2d, out_dtype, eps=1e-5):
    """z~ = (z - mean_b z) / sqrt(var_b z + eps) [B, C] in out_dtype and inv_std f32 [C]: z2d contiguous f32 [B, C]."""
    B, C = _chk_lfd("lfd_std_fwd", z2d)
    _chk_lfd_dtype("lfd_std_fwd", out_dtype)
    zt = torch.empty(B, C, device=z2d.device, dtype=out_dtype)
    inv_std = torch.empty(C, device=z2d.device, dtype=torch.float32)
    call("fddm_lfd_std_fwd", code(zt), ptr(z2d), ptr(zt), ptr(inv_std), B, C, float(eps), stream())
    return zt, inv_std


def lfd_std_bwd(dzt, zt, inv_std):
    """dz f32 [B, C] from dz~ (contiguous f32 [B, C]), z~ (B C contiguous f32 / bf16 elements) and inv_std f32 [C]."""
    _chk(zt is not None and inv_std is not None, "lfd_std_bwd: z~ and inv_std are given")
    B, C = _chk_lfd("lfd_std_bwd", dzt, zt, (("inv_std", inv_std, dzt.shape[-1]),))
    dz = torch.empty(B, C, device=dzt.device, dtype=torch.float32)
    call("fddm_lfd_std_bwd", code(zt), ptr(dzt), ptr(zt), ptr(inv_std), ptr(dz), B, C, stream())
    return dz


def lfd_colstat(z2d, out, mean_sum=None, inv_n=0.0):
    """out[c] = sum_b z[b][c], or with mean_sum (f32 [C]) sum_b (z[b][c] - mean_sum[c] inv_n)^2: out f32, C elements."""
    _chk(out is not None, "lfd_colstat: out is given")
    B, C = _chk_lfd("lfd_colstat", z2d, None, (("out", out, z2d.shape[-1]), ("mean_sum", mean_sum, z2d.shape[-1])))
    call("fddm_lfd_colstat", ptr(z2d), ptr(out), ptr(mean_sum), float(inv_n), B, C, stream())
    return out


def lfd_std_apply(z2d, out_dtype, s1, s2, inv_n, eps=1e-5):
    """z~ and inv_std from the global column sums s1 (sum z) and s2 (centred squares), f32 [C] each."""
    _chk(s1 is not None and s2 is not None, "lfd_std_apply: s1 and s2 are given")
    B, C = _chk_lfd("lfd_std_apply", z2d, None, (("s1", s1, z2d.shape[-1]), ("s2", s2, z2d.shape[-1])))
    _chk_lfd_dtype("lfd_std_apply", out_dtype)
    zt = torch.empty(B, C, device=z2d.device, dtype=out_dtype)
    inv_std = torch.empty(C, device=z2d.device, dtype=torch.float32)
    call("fddm_lfd_std_apply", code(zt), ptr(z2d), ptr(zt), ptr(inv_std), ptr(s1), ptr(s2), float(inv_n), float(eps), B,
         C, stream())
    return zt, inv_std


def lfd_bwd_colstat(dzt, zt, out):
    """out[c] = sum_b dz~, out[C + c] = sum_b dz~ z~: out f32, 2 C elements."""
    _chk(zt is not None and out is not None, "lfd_bwd_colstat: z~ and out are given")
    B, C = _chk_lfd("lfd_bwd_colstat", dzt, zt, (("out", out, 2 * dzt.shape[-1]),))
    call("fddm_lfd_bwd_colstat", code(zt), ptr(dzt), ptr(zt), ptr(out), B, C, stream())
    return out


def lfd_std_bwd_apply(dzt, zt, inv_std, sums, inv_n, scale=1.0):
    """dz = scale (dz~ - sums[c] inv_n - z~ sums[C + c] inv_n) inv_std: inv_std f32 [C], sums f32, 2 C elements."""
    _chk(zt is not None and inv_std is not None and sums is not None, "lfd_std_bwd_apply: z~, inv_std and sums are given")
    B, C = _chk_lfd("lfd_std_bwd_apply", dzt, zt, (("inv_std", inv_std, dzt.shape[-1]), ("sums", sums, 2 * dzt.shape[-1])))
    dz = torch.empty(B, C, device=dzt.device, dtype=torch.float32)
    call("fddm_lfd_std_bwd_apply", code(zt), ptr(dzt), ptr(zt), ptr(inv_std), ptr(sums), float(inv_n), float(scale),
         ptr(dz), B, C, stream())
    return dz


def _chk_cm(name, Cm):
    _chk(Cm.dim() == 2 and Cm.shape[0] == Cm.shape[1] and Cm.dtype == torch.float32 and Cm.is_contiguous() and Cm.is_cuda
         and 0 < Cm.shape[0] <= 32768, f"{name}: Cm is contiguous float32 [D, D], 0 < D <= 32768, on a GPU")
    return Cm.shape[0]


def lfd_loss(Cm, lam):
    """sum_j (1 - C_jj)^2 + lam sum_{j != k} C_jk^2 as an f32 scalar: Cm contiguous f32 [D, D]."""
    D = _chk_cm("lfd_loss", Cm)
    loss = torch.empty((), device=Cm.device, dtype=torch.float32)
    call("fddm_lfd_loss", ptr(Cm), ptr(loss), D, float(lam), stream())
    return loss


def lfd_dloss(Cm, gscale, lam, out_dtype):
    """dC = gscale[0] d loss / dC [D, D] in out_dtype: gscale None (1) or one f32 element on Cm's GPU."""
    D = _chk_cm("lfd_dloss", Cm)
    _chk_vec("lfd_dloss", "gscale", gscale, 1, Cm.device)
    _chk_lfd_dtype("lfd_dloss", out_dtype)
    dC = torch.empty(D, D, device=Cm.device, dtype=out_dtype)
    call("fddm_lfd_dloss", code(dC), ptr(Cm), ptr(gscale), ptr(dC), D, float(lam), stream())
    return dC


# ----------------------------------------------------------------------------- small per-batch ops
def rows_mean(x3d):
    """[B, S, d] (f32 / bf16, contiguous) -> f32 [B, d] mean over S."""
    B, S, d = x3d.shape
    _chk(x3d.is_contiguous(), "rows_mean: contiguous input")
    out = torch.empty(B, d, device=x3d.device, dtype=torch.float32)
    call("fddm_rows_mean", code(x3d), ptr(x3d), ptr(out), B, S, d, stream())
    return out


def rows_mean_masked(x3d, key_keep, clamp=False):
    """[B, S, d] (f32 / bf16, contiguous), key_keep [B, S] uint8 -> f32 [B, d]: the sum over kept rows divided by the
    kept count (clamp: by at least 1 — AcousticEncoder pooling; unclamped, an entry with nothing kept is NaN, as the
    reference decoder's masked mean)."""
    B, S, d = x3d.shape
    _chk(x3d.is_contiguous() and x3d.data_ptr() % 16 == 0, "rows_mean_masked: contiguous 16-byte-aligned input")
    _chk(key_keep.dtype == torch.uint8 and key_keep.is_contiguous() and key_keep.numel() == B * S
         and key_keep.device == x3d.device, "rows_mean_masked: contiguous uint8 [B, S] mask")
    out = torch.empty(B, d, device=x3d.device, dtype=torch.float32)
    call("fddm_rows_mean_masked", code(x3d), ptr(x3d), ptr(key_keep), ptr(out), B, S, d, int(bool(clamp)), stream())
    return out


def rows_zero_masked(x2d, key_keep):
    """Rows of x2d [R, E] (f32 / bf16, contiguous; in place) whose key_keep byte (uint8, R of them) is 0 become
    zeros."""
    R, E = x2d.shape
    _chk(x2d.is_contiguous() and x2d.data_ptr() % 16 == 0 and (E * x2d.element_size()) % 16 == 0,
         "rows_zero_masked: contiguous rows of a multiple of 16 bytes")
    _chk(key_keep.dtype == torch.uint8 and key_keep.is_contiguous() and key_keep.numel() == R
         and key_keep.device == x2d.device, "rows_zero_masked: contiguous uint8 mask, one byte per row")
    call("fddm_rows_zero_masked", code(x2d), ptr(x2d), ptr(key_keep), R, E, stream())
    return x2d


def time_embed(t, d, max_steps):
    """SinusoidalTimeEmbedding features of int64 t [B] -> f32 [B, d]."""
    _chk(t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 1, "time_embed: int64 [B]")
    emb = torch.empty(t.numel(), d, device=t.device, dtype=torch.float32)
    call("fddm_time_embed", ptr(t), ptr(emb), t.numel(), d, float(max_steps), stream())
    return emb


def _parr(ts):
    import ctypes
    return (ctypes.c_void_p * len(ts))(*[ptr(x) for x in ts])


def small_linear(inp, Ws, bs, outs, outs2=None, act=0, aux=None, transpose_w=False):
    """out_j = act(inp @ W_j^T + b_j) (transpose_w: inp @ W_j) for a few row-batch (R <= 64 per tile) fp32 Linears
    sharing one input; act 1 also writes silu into outs2; act 2 multiplies by silu'(aux)."""
    R, K = inp.shape
    W0 = Ws[0]
    N = W0.shape[0]
    if transpose_w:
        N = W0.shape[1]
        _chk(W0.shape[0] == K, "small_linear shapes")
    else:
        _chk(W0.shape[1] == K, "small_linear shapes")
    for W, o in zip(Ws, outs):
        _chk(W.dtype == torch.float32 and W.is_contiguous() and W.shape == W0.shape, "small_linear weights")
        _chk(o.dtype == torch.float32 and o.shape == (R, N) and o.stride(1) == 1 and o.stride(0) == N, "small_linear out")
    _chk(inp.dtype == torch.float32 and inp.stride(1) == 1, "small_linear input")
    _chk(len(outs) == len(Ws), "small_linear: one output per weight set")
    if bs is not None:
        _chk(len(bs) == len(Ws), "small_linear: one bias per weight set")
        for b in bs:
            _chk(b is None or (b.dtype == torch.float32 and b.is_contiguous() and tuple(b.shape) == (N,)),
                 "small_linear: biases are contiguous f32 [N]")
    if act == 1:
        _chk(outs2 is not None and len(outs2) == len(outs), "small_linear: act 1 writes silu into outs2, one per output")
        for o2 in outs2:
            _chk(o2.dtype == torch.float32 and tuple(o2.shape) == (R, N) and o2.is_contiguous(),
                 "small_linear: outs2 are contiguous f32 [R, N]")
    if act == 2:
        _chk(aux is not None and aux.dtype == torch.float32 and tuple(aux.shape) == (R, N) and aux.is_contiguous(),
             "small_linear: act 2 reads aux, contiguous f32 [R, N]")
    dev = inp.device
    _chk(inp.is_cuda and all(t is None or t.device == dev for ts in (Ws, outs, bs or (), outs2 or ()) for t in ts)
         and (aux is None or aux.device == dev), "small_linear: every tensor on one GPU")
    ldw = W0.shape[1]
    for i in range(0, len(Ws), 16):
        sl = slice(i, i + 16)
        n = len(Ws[sl])
        call("fddm_small_linear", ptr(inp), inp.stride(0), n, _parr(Ws[sl]), _parr(bs[sl]) if bs is not None else None,
             _parr(outs[sl]), _parr(outs2[sl]) if outs2 is not None else None, ldw, N, ptr(aux), R, N, K, act,
             int(transpose_w), stream())


def small_dw(jobs):
    """For (dy [R, N], x [R, K], dW [N, K], db [N] or None): dW += dy^T x, db += colsum(dy) (fp32, R rows)."""
    import ctypes
    if not jobs:
        return
    R = jobs[0][0].shape[0]
    for dy, x, dW, db in jobs:
        _chk(dy.dtype == x.dtype == dW.dtype == torch.float32 and dy.shape[0] == x.shape[0] == R, "small_dw dtypes")
        _chk(dW.shape == (dy.shape[1], x.shape[1]) and dW.is_contiguous() and dy.stride(1) == 1 and x.stride(1) == 1,
             "small_dw shapes")
        _chk(db is None or (db.numel() == dy.shape[1] and db.is_contiguous()), "small_dw bias")
    for i in range(0, len(jobs), 16):
        ch = jobs[i:i + 16]
        L = ctypes.c_long * len(ch)
        call("fddm_small_dw", len(ch), _parr([j[0] for j in ch]), L(*[j[0].stride(0) for j in ch]),
             _parr([j[1] for j in ch]), L(*[j[1].stride(0) for j in ch]), _parr([j[2] for j in ch]),
             _parr([j[3] for j in ch]), L(*[j[0].shape[1] for j in ch]), L(*[j[1].shape[1] for j in ch]), R, stream())


def kl_reduce(kl_tok, mask_u8, B, L, want_w=True):
    """Masked batch mean of the per-token KL (train.py:247-253) -> (loss f32 scalar, w [B*L] = d loss / d kl_tok,
    or None when not wanted)."""
    _chk(kl_tok.numel() == B * L and (mask_u8 is None or (mask_u8.numel() == B * L and mask_u8.dtype == torch.uint8)),
         "kl_reduce shapes")
    loss = torch.empty((), device=kl_tok.device, dtype=torch.float32)
    w = torch.empty(B * L, device=kl_tok.device, dtype=torch.float32) if want_w else None
    call("fddm_kl_reduce", ptr(kl_tok), ptr(mask_u8), ptr(w), ptr(loss), B, L, stream())
    return loss, w


JUMP_FAST, JUMP_SAMPLE = 1, 2


def jump(logits2d, xt, coef, L, mode=0, temperature=1.0, seed=0, rng_stream=0, x_next=None, x0hat=None):
    """One jumpy-sampler step over logits [N, V] (f32): returns (x_next [N], x0hat [N]) int64."""
    N, V = logits2d.shape
    _chk(logits2d.dtype == torch.float32 and logits2d.stride(1) == 1, "jump: f32 rows with unit stride")
    _chk(xt.numel() == N and xt.dtype == torch.int64 and coef.dtype == torch.float32, "jump: xt/coef")
    _chk(coef.numel() >= 4 * ((N + L - 1) // L), "jump: coef holds 4 floats per batch element")
    if x_next is None:
        x_next = torch.empty(N, device=logits2d.device, dtype=torch.int64)
    if x0hat is None:
        x0hat = torch.empty(N, device=logits2d.device, dtype=torch.int64)
    call("fddm_jump", ptr(logits2d), logits2d.stride(0), ptr(xt), ptr(coef), ptr(x_next), ptr(x0hat), N, L, V, mode,
         float(temperature), seed, rng_stream, stream())
    return x_next, x0hat


# ------------------------------------------------------------------------------------ audio front end
WAV_MAX_CHANNELS = 8


def wav_resample(src, desc, taps, klo, P, Q, W, wave, lengths):
    """Clips of raw interleaved f32 samples at one source rate -> 16 kHz mono rows of a padded batch, one launch
    (csrc/audio.hip; the contract is at fddm_wav_resample in include/fddm_hip.h).
    src f32 1-D on the GPU; desc: one (first float in src, frames, channels, destination row) per clip, host integers;
    taps f32 [NT, P] and klo int32 [P]: the compacted table of fddm_hip.audio.device_taps; wave f32 [rows, T]
    contiguous, lengths int64 [rows]. Writes wave[row] and lengths[row] of every named row; returns (wave, lengths)."""
    import ctypes

    from . import audio as _audio
    dev = wave.device
    P, Q, W = int(P), int(Q), int(W)
    _chk(P >= 1 and Q >= 1 and W >= 0, "wav_resample: P, Q >= 1 and W >= 0")
    KT = 2 * W + Q
    # messages are built only on failure: this is the launch path
    if not (taps.dim() == 2 and taps.shape[1] == P and 1 <= taps.shape[0] <= KT and taps.dtype == torch.float32
            and taps.is_contiguous()):
        raise ValueError(f"wav_resample: taps is a contiguous f32 [NT <= {KT}, P = {P}] table, got "
                         f"{tuple(taps.shape)} {taps.dtype}")
    if not (klo.dtype == torch.int32 and tuple(klo.shape) == (P,) and klo.is_contiguous()):
        raise ValueError(f"wav_resample: klo is a contiguous int32 [{P}] vector")
    if _audio.lds_span_bytes(P, Q, KT) > _audio.LDS_MAX_BYTES:
        raise ValueError(f"wav_resample: the input span of P = {P}, Q = {Q}, W = {W} exceeds the kernel's LDS")
    _chk(wave.dim() == 2 and wave.dtype == torch.float32 and wave.is_contiguous() and wave.shape[1] >= 1,
         "wav_resample: wave is a contiguous f32 [rows, T >= 1] tensor")
    rows, T = wave.shape
    _chk(T <= 2 ** 31 - 1 - _audio.OUT_BLOCK, "wav_resample: T below 2^31 - 1024")
    _chk(lengths.dtype == torch.int64 and tuple(lengths.shape) == (rows,) and lengths.is_contiguous(),
         "wav_resample: lengths is a contiguous int64 [rows] vector")
    _chk(src.dim() == 1 and src.dtype == torch.float32 and src.is_contiguous(), "wav_resample: src is a contiguous f32 vector")
    _chk(wave.is_cuda and all(t.device == dev for t in (src, taps, klo, lengths)), "wav_resample: every tensor on one GPU")
    # the launch goes to the current device's current stream (stream()): tensors of another GPU would be read and written
    # by a kernel running on the wrong device
    if dev.index != _cur_device():
        raise ValueError(f"wav_resample: the tensors are on {dev} but the current device is cuda:{_cur_device()} "
                         "(torch.cuda.set_device / torch.cuda.device first)")
    nsrc = src.numel()
    seen = set()
    flat = []
    for d in desc:
        off, n, nch, row = (int(v) for v in d)
        if not 1 <= nch <= WAV_MAX_CHANNELS:
            raise ValueError(f"wav_resample: {nch} channels (1 .. {WAV_MAX_CHANNELS})")
        if not (0 <= off <= nsrc and n >= 0 and off + n * nch <= nsrc and n * P < 2 ** 31):
            raise ValueError(f"wav_resample: clip (offset {off}, {n} frames, {nch} channels) outside src ({nsrc} floats)")
        if not 0 <= row < rows or row in seen:
            raise ValueError(f"wav_resample: destination row {row} (distinct rows of {rows})")
        seen.add(row)
        flat += (off, n, nch, row)
    if not flat:
        return wave, lengths
    call("fddm_wav_resample", ptr(src), nsrc, (ctypes.c_long * len(flat))(*flat), len(flat) // 4, ptr(taps), ptr(klo),
         int(taps.shape[0]), P, Q, W, ptr(wave), ptr(lengths), rows, T, stream())
    return wave, lengths
