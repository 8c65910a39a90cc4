"""Fused KL forward + gradient (ops.kl_fused, csrc/kl.hip kl4_fused_kernel) at the C2 train-step shape: B*L = 8192
rows of V = 8000 f32 logits in, bf16 gradient out (393 MB). HIP-event timing of 20 back-to-back launches after 3
warm-ups, against a float4 copy of the same bytes as the achievable-HBM yardstick.

--V V1,V2,...: the same at other vocabularies, the rows scaled down to keep at most ~1 GB of logits (8192 rows at
most), with the streamed kernels (ops.kl_fused_wide, ops.softmax_rows_wide) beside the resident ones wherever the
resident ones serve; rates in algorithmic bytes (KL: 4 V read + 2 V written per row; softmax f32 -> bf16 the same)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fddm-asr_amd"))
import torch  # noqa: E402

from fddm_hip import ops  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def run(V, wide):
    dev = torch.device("cuda:0")
    L, T = 256, 200
    B = 32 if not wide else max(1, min(32, (1 << 30) // (4 * V * L)))
    N = B * L
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(N, V, device=dev, generator=g) * 3
    xt = torch.randint(0, V, (N,), device=dev, generator=g)
    x0 = torch.where(torch.rand(N, device=dev, generator=g) < 0.5, xt, torch.randint(0, V, (N,), device=dev, generator=g))
    t = torch.randint(1, T + 1, (B,), device=dev, generator=g)
    betas = 0.2 * torch.sin(torch.pi * torch.arange(1, T + 1, device=dev) / (2 * T)) ** 2
    mask = (torch.rand(N, device=dev, generator=g) < 0.9).to(torch.uint8)
    nbytes = N * V * (4 + 2)
    src = torch.empty(nbytes // 2 // 4, device=dev)
    dst = torch.empty_like(src)
    cu = timeit(lambda: dst.copy_(src))
    del src, dst
    tail = f"copy of {nbytes / 1e6:.0f} MB: {cu:6.1f} us {nbytes / cu / 1e6:5.2f} TB/s"
    rows = []
    if V % 4 == 0 and V <= ops.KL_FUSED_MAX_V:
        rows.append(("kl_fused", lambda: ops.kl_fused(logits, xt, x0, t, betas, mask, L, out_dtype=torch.bfloat16)))
    if wide:
        dz = torch.empty(N, V, device=dev, dtype=torch.bfloat16)
        kl = torch.empty(N, device=dev)
        y = torch.empty(N, V, device=dev, dtype=torch.bfloat16)
        rows.append(("kl_fused_wide", lambda: ops.kl_fused_wide(logits, xt, x0, t, betas, mask, L, kl_tok=kl, dz=dz)))
        if V <= ops.SOFTMAX_MAX_V:
            rows.append(("softmax_rows", lambda: ops.softmax_rows(logits, torch.bfloat16)))
        rows.append(("softmax_rows_wide", lambda: ops.softmax_rows_wide(logits, torch.bfloat16, out=y)))
    for name, fn in rows:
        us = timeit(fn)
        print(f"{name} N={N} V={V}: {us:7.1f} us  {nbytes / us / 1e6:5.2f} TB/s ({nbytes / us / 8e6:.2f} of 8 TB/s) | {tail}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", default="", help="comma-separated vocabularies; adds the streamed kernels' rows")
    a = ap.parse_args()
    if not a.V:
        run(8000, False)
    for V in (int(v) for v in a.V.split(",") if v):
        run(V, True)


if __name__ == "__main__":
    main()
