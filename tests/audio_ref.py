"""Float64 numpy restatement of the audio front end's contract (include/fddm_hip.h, fddm_wav_resample): the
Hann-windowed sinc of torchaudio.functional.resample (lowpass_filter_width 6, rolloff 0.99) applied to the f32 channel
mean. Straightforward on purpose: build the table from the formulas, pad, one dot product per output. It shares no code
with fddm_hip/audio.py. The keyword arguments of `resample` are mutation hooks for tests/test_cpu_audio.py (each one
breaks the contract in one way); they default to the contract."""
import math

import numpy as np

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)
# (P, Q, W, KT) per rate, as tabulated in DESIGN §4.16
GEOMETRY = {8000: (2, 1, 7, 15), 11025: (640, 441, 7, 455), 22050: (320, 441, 9, 459), 24000: (2, 3, 10, 23),
            32000: (1, 2, 13, 28), 44100: (160, 441, 17, 475), 48000: (1, 3, 19, 41), 96000: (1, 6, 37, 80)}


def geometry(orig, new=16000, width=6, rolloff=0.99):
    if orig == new:           # torchaudio returns the input: one phase, one tap of 1.0, no context
        return 1, 1, 0, 1, 1.0
    g = math.gcd(orig, new)
    Q, P = orig // g, new // g
    base = min(Q, P) * rolloff
    W = int(math.ceil(width * Q / base))
    return P, Q, W, 2 * W + Q, base


def table(orig, new=16000, width=6, rolloff=0.99):
    """h[p][k] in float64."""
    P, Q, W, KT, base = geometry(orig, new, width, rolloff)
    h = np.zeros((P, KT), dtype=np.float64)
    if orig == new:
        h[0, 0] = 1.0
        return h
    for p in range(P):
        for k in range(KT):
            t = (-p / P + (k - W) / Q) * base
            t = max(-width, min(width, t))
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[p, k] = s * math.cos(math.pi * t / (2 * width)) ** 2 * (base / Q)
    return h


_TABLES = {}


def cached_table(orig):
    if orig not in _TABLES:
        _TABLES[orig] = table(orig)
    return _TABLES[orig]


def channel_mean(x):
    """[n, nch] f32 -> [n] f32: the sum in channel order, then true division, all in f32."""
    x = np.asarray(x, dtype=np.float32)
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(np.float32)
    return (s / np.float32(x.shape[1])).astype(np.float32)


def n_out(n, orig, T=None):
    P, Q, _, _, _ = geometry(orig)
    full = -((-n * P) // Q)
    return full if T is None else min(T, full)


def resample(xm, orig, T=None, *, phase_shift=0, w_shift=0, q_shift=0):
    """xm: mono samples [n] (taken as float64). Returns float64 [T] (T defaults to n_out): the filtered samples up to
    n_out, zeros after."""
    P, Q, W, KT, _ = geometry(orig)
    h = cached_table(orig)
    xm = np.asarray(xm, dtype=np.float64)
    n = xm.shape[0]
    no = n_out(n, orig, T)
    T = no if T is None else T
    pad = KT + Q + 8
    last = (max(no - 1, 0) // P) * (Q + abs(q_shift)) + KT + 4
    xp = np.zeros(pad + max(n, last) + pad, dtype=np.float64)
    xp[pad:pad + n] = xm
    out = np.zeros(T, dtype=np.float64)
    for j in range(no):
        start = pad + (j // P) * (Q + q_shift) - (W + w_shift)
        out[j] = np.dot(h[(j + phase_shift) % P], xp[start:start + KT])
    return out


def resample_clip(x, orig, T=None):
    """x [n, nch] f32 -> (float64 [T], n_out)."""
    x = np.asarray(x, dtype=np.float32)
    if x.shape[0] == 0:
        xm = np.zeros(0, dtype=np.float32)
    else:
        xm = channel_mean(x.reshape(x.shape[0], -1))
    return resample(xm, orig, T), n_out(x.shape[0], orig, T)
