"""Filter tables of the audio front end (csrc/audio.hip, fddm_wav_resample).

`sinc_resample_taps` restates the kernel of torchaudio.functional.resample (Hann window, `lowpass_filter_width`
zero crossings, `rolloff`) — what the reference's inference.py:59 applies to a clip that is not at 16 kHz — in
float64, rounded once to f32. `device_taps` caches the compacted form the kernel reads per (rate, device).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

TARGET_SR = 16000
OUT_BLOCK = 1024            # csrc/audio.hip: outputs per workgroup
LDS_MAX_BYTES = 65536       # ... and its LDS budget for the block's mono input span
MAX_TABLE = 1 << 22         # entries of the full [P][KT] table (16 MiB of f32): beyond it the rate is refused
ZERO_BELOW = 1e-20          # the window's clamped region: cos^2(pi/2) ~ 4e-33 times the sinc


class ResampleTaps(NamedTuple):
    orig_freq: int
    new_freq: int
    P: int                  # phases = new_freq / gcd
    Q: int                  # source frames per P outputs = orig_freq / gcd
    W: int                  # frames of left context
    KT: int                 # taps per phase = 2 W + Q
    h: np.ndarray           # f32 [P, KT]
    klo: np.ndarray         # int32 [P]: start of phase p's span of entries >= ZERO_BELOW (clamped so klo + NT <= KT)
    compact: np.ndarray     # f32 [NT, P]: compact[i][p] = h[p][klo[p] + i], entries below ZERO_BELOW as exact zeros

    @property
    def NT(self) -> int:
        return int(self.compact.shape[0])


def resample_geometry(orig_freq: int, new_freq: int = TARGET_SR, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(P, Q, W, KT, base) of the polyphase filter."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError(f"sample rate {orig_freq} Hz -> {new_freq} Hz: rates must be positive")
    if orig_freq == new_freq:       # torchaudio returns the input unchanged: one phase, one tap 1.0, no context
        return 1, 1, 0, 1, 1.0
    g = math.gcd(orig_freq, new_freq)
    Q, P = orig_freq // g, new_freq // g
    base = min(Q, P) * rolloff
    W = int(math.ceil(lowpass_filter_width * Q / base))
    return P, Q, W, 2 * W + Q, base


def lds_span_bytes(P: int, Q: int, KT: int) -> int:
    """LDS bytes of one workgroup (the launcher of csrc/audio.hip computes the same number)."""
    return (((OUT_BLOCK - 1) // P + 1) * Q + KT + 6) // 4 * 16


def sinc_resample_table64(orig_freq, new_freq=TARGET_SR, lowpass_filter_width=6, rolloff=0.99) -> np.ndarray:
    """The float64 table h[p][k]."""
    P, Q, W, KT, base = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    if int(orig_freq) == int(new_freq):
        return np.ones((1, 1), dtype=np.float64)
    p = np.arange(P, dtype=np.float64)[:, None]
    k = np.arange(KT, dtype=np.float64)[None, :]
    t = np.clip((-p / P + (k - W) / Q) * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(np.pi * t / (2 * lowpass_filter_width)) ** 2
    a = np.pi * t
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return sinc * window * (base / Q)


_TAPS = {}


def sinc_resample_taps(orig_freq, new_freq=TARGET_SR, lowpass_filter_width=6, rolloff=0.99) -> ResampleTaps:
    """The f32 table of `orig_freq` -> `new_freq` and its compacted form, cached per argument set. A rate whose table
    or whose per-workgroup input span exceeds the kernel's limits raises a ValueError naming the rate."""
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff))
    if key in _TAPS:
        return _TAPS[key]
    P, Q, W, KT, _ = resample_geometry(*key)
    if P * KT > MAX_TABLE:
        raise ValueError(f"sample rate {key[0]} Hz: the {P} x {KT} filter table to {key[1]} Hz exceeds the resampler's "
                         f"limit of {MAX_TABLE} entries")
    if lds_span_bytes(P, Q, KT) > LDS_MAX_BYTES:
        raise ValueError(f"sample rate {key[0]} Hz: the input span of {OUT_BLOCK} outputs at {key[1]} Hz "
                         f"({lds_span_bytes(P, Q, KT)} bytes) exceeds the resampler's {LDS_MAX_BYTES} bytes of LDS")
    h = sinc_resample_table64(*key).astype(np.float32)
    nz = np.abs(h) >= ZERO_BELOW
    first = nz.argmax(axis=1)
    last = KT - nz[:, ::-1].argmax(axis=1)          # every phase has a nonzero entry (the sinc's main lobe)
    NT = int((last - first).max())
    klo = np.minimum(first, KT - NT).astype(np.int32)
    hz = np.where(nz, h, np.float32(0.0))
    compact = np.ascontiguousarray(hz[np.arange(P)[None, :], klo[None, :] + np.arange(NT)[:, None]], dtype=np.float32)
    taps = ResampleTaps(key[0], key[1], P, Q, W, KT, h, klo, compact)
    _TAPS[key] = taps
    return taps


_DEVICE_TAPS = {}


def device_taps(orig_freq, device, new_freq=TARGET_SR):
    """(ResampleTaps, compact f32 [NT, P], klo int32 [P]) with the two arrays on `device`, cached."""
    device = torch.device(device)
    key = (int(orig_freq), int(new_freq), device.type, device.index)
    if key not in _DEVICE_TAPS:
        t = sinc_resample_taps(orig_freq, new_freq)
        _DEVICE_TAPS[key] = (t, torch.from_numpy(t.compact).to(device), torch.from_numpy(t.klo).to(device))
    return _DEVICE_TAPS[key]
