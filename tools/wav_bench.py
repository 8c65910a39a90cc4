#!/usr/bin/env python3
"""Timing of the audio front end (csrc/audio.hip, fddm_wav_resample) — bench.py measures the train step, this measures
the inference front end only.

    python tools/wav_bench.py [--clips 32] [--seconds 20] [--replays 500] [--out profiles/wav_bench.json]

Per workload (48 kHz stereo, 44.1 kHz mono; int16 WAV files of white noise written to a temporary directory):
  * kernel: one launch for the whole batch. The launches of a timed window are held in one HIP graph (no host work
    between kernels) that rotates through 6 buffer sets, more than the 256 MiB Infinity Cache between two uses of a
    buffer, and is replayed `replays` times between two HIP events (3000 launches, a few tenths of a second). Timed
    with the compacted table the product uses and with the full [KT][P] table (zero-span skipping off), alternating.
    bytes = source samples read + wave and lengths written, over the best round's time per launch, against the
    8 TB/s HBM spec. The host time of an eager ops.wav_resample call is reported next to it;
  * host, for comparison only: data_io.load_wav_16k (scipy polyphase, CPU) over the same files, and data_io.load_batch
    end to end (file read, pack, one host-to-device copy, launch, synchronise).
Prints one JSON line per workload. Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fddm-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_SPEC = 8.0e12


def write_wav16(path, frames, sr):
    n, ch = frames.shape
    b = frames.astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, ch, sr, sr * ch * 2, ch * 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(b)) + b
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


SETS = 6            # buffer sets a timed window rotates through: a launch's data was last touched 5 launches ago,
                    # with 0.75 GB (44.1 kHz mono) to 1.4 GB (48 kHz stereo) of other traffic in between — beyond the
                    # 256 MiB Infinity Cache, so the reads and writes of a launch go to HBM


def time_kernel(sets, desc, taps, klo, t, replays):
    """Seconds per launch: one HIP graph holding a launch per buffer set (no host work between the kernels), replayed
    `replays` times between two events."""
    from fddm_hip import ops

    def one_round():
        for src, wave, lengths in sets:
            ops.wav_resample(src, desc, taps, klo, t.P, t.Q, t.W, wave, lengths)

    one_round()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_round()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (replays * len(sets))


def host_enqueue(sets, desc, taps, klo, t, calls=200):
    """Seconds of host time per eager ops.wav_resample call (checks, descriptor array, launch), GPU not waited for."""
    from fddm_hip import ops
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        src, wave, lengths = sets[i % len(sets)]
        ops.wav_resample(src, desc, taps, klo, t.P, t.Q, t.W, wave, lengths)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / calls


def workload(name, sr, nch, clips, seconds, replays, tmp, dev):
    import data_io
    from fddm_hip import audio
    rng = np.random.default_rng(sr + nch)
    n = int(seconds * sr)
    paths = []
    for i in range(clips):
        path = os.path.join(tmp, f"{name}_{i}.wav")
        write_wav16(path, rng.integers(-32768, 32768, size=(n, nch)), sr)
        paths.append(path)

    t, taps, klo = audio.device_taps(sr, dev)
    per = (n * nch + 3) // 4 * 4
    desc = [(i * per, n, nch, i) for i in range(clips)]
    T = -((-n * t.P) // t.Q)
    src0 = torch.empty(per * clips, device=dev).uniform_(-1, 1)
    sets = [(src0 if i == 0 else src0.clone(), torch.empty(clips, T, device=dev),
             torch.empty(clips, device=dev, dtype=torch.int64)) for i in range(SETS)]
    full_taps = torch.from_numpy(np.ascontiguousarray(t.h.T)).to(dev)
    full_klo = torch.zeros(t.P, device=dev, dtype=torch.int32)
    # interleaved rounds in one process: compact, full, compact, full, ...
    rounds = {"compact": [], "full": []}
    for _ in range(3):
        rounds["compact"].append(time_kernel(sets, desc, taps, klo, t, replays))
        ref = sets[0][1].clone()
        rounds["full"].append(time_kernel(sets, desc, full_taps, full_klo, t, max(1, replays // 4)))
        diff = float((sets[0][1] - ref).abs().max())
    nbytes = 4 * (clips * n * nch + clips * T) + 8 * clips
    k = min(rounds["compact"])
    enqueue = host_enqueue(sets, desc, taps, klo, t)

    t0 = time.perf_counter()
    for p in paths:
        data_io.load_wav_16k(p)
    scipy_s = time.perf_counter() - t0
    data_io.load_batch(paths[:2], dev)
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        data_io.load_batch(paths, dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return {"workload": name, "clips": clips, "seconds": seconds, "rate": sr, "channels": nch, "P": t.P, "Q": t.Q,
            "KT": t.KT, "NT": t.NT, "outputs_per_clip": T, "bytes": nbytes, "buffer_sets": SETS,
            "launches_per_window": replays * SETS,
            "window_ms_compact": [round(x * replays * SETS * 1e3, 1) for x in rounds["compact"]],
            "kernel_us_compact": [round(x * 1e6, 2) for x in rounds["compact"]],
            "kernel_us_full_table": [round(x * 1e6, 2) for x in rounds["full"]],
            "kernel_TBps": round(nbytes / k / 1e12, 3), "share_of_8TBps_spec": round(nbytes / k / HBM_SPEC, 3),
            "full_vs_compact_max_abs_diff": diff, "host_enqueue_us_per_eager_call": round(enqueue * 1e6, 1),
            "host_scipy_load_wav_16k_s": round(scipy_s, 3), "host_load_batch_end_to_end_s": round(best, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--replays", type=int, default=500, help="graph replays per timed window (6 launches each)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wav_bench: no GPU")
    dev = torch.device("cuda:0")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, sr, nch in (("48k_stereo", 48000, 2), ("44k1_mono", 44100, 1)):
            r = workload(name, sr, nch, args.clips, args.seconds, args.replays, tmp, dev)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
