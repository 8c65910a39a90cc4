"""WavLM-Large encoder forward at the full geometry (hidden 1024, 24 layers, 16 heads, 7 x 512 conv), bf16, random
weights, 10 s utterances: ms per batch and utterances/s in steady state (HIP events, one process), the two kernels of
the "layer" conv stack alone next to a float4 copy moving the same bytes, and the split of one forward by kernel class.

    python tools/wavlm_large_bench.py [--batches 16 32] [--iters 5]

Whole forward: HIP events around `iters` eager forwards after 2 warm-up forwards. Kernel classes: one further forward
with an event pair around every ops call of the class (the launches are long at these sizes, so the event pairs
change little; the classes' sum is printed beside the whole). Kernels alone: 20 launches between one event pair.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fddm-asr_amd"))
import torch  # noqa: E402

from fddm_hip import ops  # noqa: E402
from fddm_hip import runtime as rt  # noqa: E402

CLASSES = {"conv0_ln_gelu": "conv0 + LN + GELU", "conv1d_gemm": "conv GEMMs", "ln_gelu_fwd": "conv ln_gelu",
           "linear": "transformer GEMMs", "attn_fwd_relgate_x": "attention", "ln_fwd": "LayerNorms",
           "posconv_gelu": "positional conv"}


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def class_split(run):
    """ms per class over one forward: every ops call of CLASSES between its own event pair."""
    pairs, saved = [], {}
    for name in CLASSES:
        fn = saved[name] = getattr(ops, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = _fn(*a, **k)
            e.record()
            pairs.append((_name, s, e))
            return r
        setattr(ops, name, wrapped)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    out = {}
    for name, s, e in pairs:
        out[name] = out.get(name, 0.0) + s.elapsed_time(e)
    return out, {n: sum(1 for p in pairs if p[0] == n) for n in out}


def kernels_alone(dev, B, nsamp):
    bf = torch.bfloat16
    C = 512
    T0 = (nsamp - 10) // 5 + 1
    wave = 0.1 * torch.randn(B, nsamp, device=dev)
    w, v1, v0 = 0.3 * torch.randn(C, 10, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    out = torch.empty(B, T0, C, device=dev, dtype=bf)
    t = timeit(lambda: ops.conv0_ln_gelu(wave, w, v0, v1, v0, bf, C, 10, 5, out=out), 20)
    byt = wave.numel() * 4 + out.numel() * 2
    src = torch.empty(byt // 8, device=dev)
    dst = torch.empty_like(src)
    tc = timeit(lambda: dst.copy_(src), 20)
    print(f"  conv0_ln_gelu    B {B}: {t * 1e3:8.1f} us  {byt / t / 1e9:6.2f} TB/s   float4 copy of the same bytes "
          f"{tc * 1e3:8.1f} us  {byt / tc / 1e9:6.2f} TB/s", flush=True)
    T1 = (T0 - 3) // 2 + 1
    x = torch.randn(B * T1, C, device=dev).to(bf)
    t = timeit(lambda: ops.ln_gelu_fwd(x, v1, v0, out=x), 20)
    byt = x.numel() * 4
    src = torch.empty(byt // 8, device=dev)
    dst = torch.empty_like(src)
    tc = timeit(lambda: dst.copy_(src), 20)
    print(f"  ln_gelu_fwd (conv layer 1 rows {B * T1}, in place): {t * 1e3:8.1f} us  {byt / t / 1e9:6.2f} TB/s   float4 "
          f"copy of the same bytes {tc * 1e3:8.1f} us  {byt / tc / 1e9:6.2f} TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    from models.wavlm import WAVLM_LARGE, WavLMModel, wavlm_config
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with rt.use_precision("bf16"):
        m = WavLMModel(wavlm_config(**WAVLM_LARGE)).to(dev).eval()
        nsamp = 16000 * a.seconds
        for B in a.batches:
            wave = 0.1 * torch.randn(B, nsamp, device=dev)
            run = lambda: m.forward_hidden(wave)   # noqa: E731
            ms = timeit(run, a.iters)
            print(f"WavLM-Large forward, bf16, B {B} x {a.seconds} s (S {m.frames(nsamp)}): {ms:8.2f} ms per batch, "
                  f"{B / ms * 1e3:7.1f} utt/s", flush=True)
            split, calls = class_split(run)
            tot = sum(split.values())
            for name, label in CLASSES.items():
                if name in split:
                    print(f"  {label:<20} {split[name]:8.2f} ms  {100 * split[name] / tot:5.1f} %  ({calls[name]} launches)")
            print(f"  {'sum of the classes':<20} {tot:8.2f} ms", flush=True)
            kernels_alone(dev, B, nsamp)


if __name__ == "__main__":
    main()
