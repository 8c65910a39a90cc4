"""fddm_wav_resample (csrc/audio.hip) through ops.wav_resample and data_io.load_batch against the float64
restatement of its contract (tests/audio_ref.py; tests/test_cpu_audio.py checks that restatement on its own).

Inputs are white noise in [-1, 1], so an indexing error is O(1). Tolerance: the worst-case f32 accumulation error is
(KT + 1) 2^-24 sum|h| <= 476 * 5.96e-8 * 1.87 = 5.3e-5 for |x| <= 1, plus ~1e-7 of table rounding; 1e-4 absolute, the
project's fp32 parity tolerance, sits above it. Output buffers are filled with NaN before each call, so a sample the
kernel does not write shows; lengths are filled with -7."""
import numpy as np
import pytest
import torch

import audio_ref as R
import data_io
from fddm_hip import audio as A
from fddm_hip import ops
from test_cpu_data import _write_wav

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
TOL = 1e-4
SLACK = 37          # T = n_out + 37: the zero tail


def noise(n, nch, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, nch)).astype(np.float32)


def run(clips, rate, rows, T, order=None, align=4):
    """clips: [n_i, nch_i] f32 arrays; row of clip i = order[i]. Returns (wave [rows, T], lengths [rows]) on the CPU."""
    order = list(range(len(clips))) if order is None else order
    t, taps, klo = A.device_taps(rate, dev)
    desc, parts, off = [], [], 0
    for x, row in zip(clips, order):
        desc.append((off, x.shape[0], x.shape[1], row))
        flat = x.reshape(-1)
        pad = (-flat.size) % align
        parts.append(np.concatenate([flat, np.full(pad, np.nan, np.float32)]))
        off += flat.size + pad
    src = torch.from_numpy(np.concatenate(parts + [np.zeros(0, np.float32)])).to(dev)
    wave = torch.full((rows, T), float("nan"), device=dev)
    lengths = torch.full((rows,), -7, device=dev, dtype=torch.int64)
    ops.wav_resample(src, desc, taps, klo, t.P, t.Q, t.W, wave, lengths)
    torch.cuda.synchronize()
    return wave.cpu(), lengths.cpu()


def check_row(got, x, rate, T, what):
    want, n_out = R.resample_clip(x, rate, T)
    got = got.double().numpy()
    assert np.isfinite(got).all(), f"{what}: unwritten or non-finite samples"
    err = np.abs(got - want).max() if T else 0.0
    assert err <= TOL, f"{what}: max abs err {err:.3e}"
    assert (got[n_out:] == 0.0).all(), f"{what}: nonzero samples past n_out = {n_out}"
    return n_out


def _cases():
    cs = []
    for rate in R.RATES:
        Q = R.geometry(rate)[1]
        cs.append((rate, 3 * Q * 64 + 5))
    for rate in (48000, 44100):
        Q = R.geometry(rate)[1]
        cs += [(rate, n) for n in (1, Q - 1, Q, Q + 1)]
    return cs


@pytest.mark.parametrize("rate,n", _cases())
def test_one_utterance_per_rate(rate, n):
    x = noise(n, 1, seed=rate + n)
    n_out = R.n_out(n, rate)
    T = n_out + SLACK
    wave, lengths = run([x], rate, 1, T)
    assert check_row(wave[0], x, rate, T, f"{rate} Hz n={n}") == n_out
    assert lengths.tolist() == [n_out]


def test_more_than_one_block_and_the_block_edges():
    """n_out = 2051 at 48 kHz: three workgroups of 1024 outputs, the last with 3; T ends inside the third."""
    x = noise(3 * 2051 - 1, 2, seed=5)
    wave, lengths = run([x], 48000, 1, 2051 + SLACK)
    assert check_row(wave[0], x, 48000, 2051 + SLACK, "48 kHz stereo, 3 blocks") == 2051 == int(lengths[0])
    x = noise(441 * 8, 1, seed=6)                           # 44.1 kHz: 1280 outputs, phases wrap inside a block
    wave, lengths = run([x], 44100, 1, 1280)
    assert check_row(wave[0], x, 44100, 1280, "44.1 kHz, T = n_out") == 1280 == int(lengths[0])


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
@pytest.mark.parametrize("nch", [1, 2, 3])
def test_channels(rate, nch):
    Q = R.geometry(rate)[1]
    x = noise(3 * Q * 8 + 5, nch, seed=10 * nch + rate)
    n_out = R.n_out(x.shape[0], rate)
    wave, lengths = run([x], rate, 1, n_out + SLACK)
    check_row(wave[0], x, rate, n_out + SLACK, f"{rate} Hz {nch} channels")
    assert int(lengths[0]) == n_out


@pytest.mark.parametrize("nch", [1, 2, 8])
@pytest.mark.parametrize("align", [4, 1])
def test_scalar_path_equals_vector_path(nch, align):
    """Clips packed on 16-byte boundaries take the wide loads (mono, stereo); packed back to back, the second clip
    starts off the boundary and takes the scalar path. Same values either way."""
    a, b = noise(1501, nch, seed=21), noise(1502, nch, seed=22)
    T = R.n_out(1502, 48000) + SLACK
    wave, lengths = run([a, b], 48000, 2, T, align=align)
    check_row(wave[0], a, 48000, T, "first clip")
    check_row(wave[1], b, 48000, T, "second clip")


@pytest.mark.parametrize("nch", [1, 2])
def test_16k_is_load_wav_16k_bit_for_bit(nch, tmp_path):
    frames = np.random.default_rng(30 + nch).integers(-32768, 32768, size=(4099, nch))
    path = str(tmp_path / "a.wav")
    _write_wav(path, frames, 16000)
    want = torch.from_numpy(data_io.load_wav_16k(path))
    x, sr = data_io.read_wav(path)
    assert sr == 16000
    wave, lengths = run([x], 16000, 1, 4099 + SLACK)
    assert int(lengths[0]) == 4099
    assert torch.equal(wave[0, :4099], want)
    assert (wave[0, 4099:] == 0).all()


def test_batch_of_four_rows_in_one_launch():
    rate = 44100
    clips = [noise(1000, 2, seed=41), noise(0, 1, seed=42), noise(4000, 1, seed=43), noise(2500, 3, seed=44)]
    order = [2, 4, 0, 3]                       # row 1 is named by no clip
    T = 1000                                   # clip 2 (4000 frames -> 1452 samples) is cut by T
    wave, lengths = run(clips, rate, 5, T, order=order)
    outs = []
    for x, row in zip(clips, order):
        outs.append(check_row(wave[row], x, rate, T, f"row {row}"))
        assert int(lengths[row]) == outs[-1]
    assert outs == [363, 0, 1000, 908]
    assert (wave[4] == 0).all()                # n = 0: a zero row
    assert torch.isnan(wave[1]).all() and int(lengths[1]) == -7


def _three_files(tmp_path):
    rng = np.random.default_rng(50)
    a = rng.integers(-32768, 32768, size=(14400, 2))                    # 48 kHz stereo int16, 0.3 s
    b = rng.integers(-32768, 32768, size=(8000, 1))                     # 16 kHz mono, 0.5 s
    c = rng.uniform(-1, 1, size=(8820, 1)).astype(np.float32)           # 44.1 kHz mono float32, 0.2 s
    paths = [str(tmp_path / n) for n in ("a48s.wav", "b16m.wav", "c44f.wav")]
    _write_wav(paths[0], a, 48000)
    _write_wav(paths[1], b, 16000)
    _write_wav(paths[2], c, 44100, tag=3, bits=32)
    return paths, [(a / 32768.0).astype(np.float32), (b / 32768.0).astype(np.float32), c], [48000, 16000, 44100]


def test_load_batch(tmp_path, monkeypatch):
    paths, clips, rates = _three_files(tmp_path)
    calls = []
    real = ops.wav_resample

    def counted(src, desc, taps, klo, P, Q, W, wave, lengths):
        calls.append((P, Q, [d[3] for d in desc]))
        return real(src, desc, taps, klo, P, Q, W, wave, lengths)

    monkeypatch.setattr(ops, "wav_resample", counted)
    wave, lengths, info = data_io.load_batch(paths, dev)
    torch.cuda.synchronize()
    assert sorted(calls) == [(1, 1, [1]), (1, 3, [0]), (160, 441, [2])]        # one launch per rate
    assert info["launches"] == 3 and info["sample_rates"] == rates and info["truncated"] == [False] * 3
    assert wave.shape == (3, 8000) and wave.dtype == torch.float32 and lengths.dtype == torch.int64
    assert lengths.tolist() == [4800, 8000, 3200]
    for i in range(3):
        check_row(wave[i].cpu(), clips[i], rates[i], 8000, paths[i])
    assert torch.equal(wave[1].cpu(), torch.from_numpy(data_io.load_wav_16k(paths[1])))

    # two files at one rate share a launch; pad_to and max_seconds cut and say so
    calls.clear()
    wave, lengths, info = data_io.load_batch([paths[0], paths[2], paths[0]], dev, max_seconds=0.25, pad_to=3500)
    torch.cuda.synchronize()
    assert sorted(calls) == [(1, 3, [0, 2]), (160, 441, [1])]
    assert lengths.tolist() == [3500, 3200, 3500] and info["truncated"] == [True, False, True]
    assert info["frames"] == [12000, 8820, 12000]
    check_row(wave[2].cpu(), clips[0][:12000], 48000, 3500, "cut clip")


def test_load_batch_names_a_10_ms_file(tmp_path):
    paths, _, _ = _three_files(tmp_path)
    short = str(tmp_path / "tiny_10ms.wav")
    _write_wav(short, np.zeros((480, 1), dtype=np.int64), 48000)
    with pytest.raises(ValueError, match="tiny_10ms.wav"):
        data_io.load_batch([paths[0], short], dev)


def test_refusals_launch_nothing(monkeypatch):
    from fddm_hip import _lib
    t, taps, klo = A.device_taps(48000, dev)
    launched = []
    monkeypatch.setattr(ops, "call", lambda *a: launched.append(a[0]))
    src = torch.zeros(9 * 64, device=dev)
    wave = torch.full((2, 64), float("nan"), device=dev)
    lengths = torch.zeros(2, device=dev, dtype=torch.int64)
    good = dict(src=src, desc=[(0, 64, 1, 0)], taps=taps, klo=klo, P=t.P, Q=t.Q, W=t.W, wave=wave, lengths=lengths)
    bad = {
        "nch 9": dict(desc=[(0, 64, 9, 0)]),
        "nch 0": dict(desc=[(0, 64, 0, 0)]),
        "table of the wrong shape": dict(taps=taps.t().contiguous()),
        "table longer than KT": dict(taps=torch.zeros(t.KT + 1, t.P, device=dev)),
        "klo of the wrong shape": dict(klo=torch.zeros(t.P + 1, device=dev, dtype=torch.int32)),
        "non-contiguous output": dict(wave=torch.full((2, 128), float("nan"), device=dev)[:, ::2]),
        "clip past the end of src": dict(desc=[(0, 577, 1, 0)]),
        "empty clip past the end of src": dict(desc=[(577, 0, 1, 0)]),
        "row out of range": dict(desc=[(0, 64, 1, 2)]),
        "one row twice": dict(desc=[(0, 64, 1, 0), (64, 64, 1, 0)]),
        "f64 source": dict(src=src.double()),
        "int32 lengths": dict(lengths=lengths.int()),
        "span beyond LDS": dict(Q=4096),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.wav_resample(**{**good, **kw})
        assert not launched, what
    ops.wav_resample(**good)
    assert launched == ["fddm_wav_resample"]
    torch.cuda.synchronize()
    assert torch.isnan(wave).all()             # the launch was intercepted: nothing ran


def test_tensors_of_another_device_than_the_current_one_are_refused(tmp_path, monkeypatch):
    """libfddm_hip launches on the current device's current stream: tensors that live elsewhere must not reach it."""
    t, taps, klo = A.device_taps(48000, dev)
    launched = []
    monkeypatch.setattr(ops, "call", lambda *a: launched.append(a[0]))
    src = torch.zeros(64, device=dev)
    wave = torch.full((1, 64), float("nan"), device=dev)
    lengths = torch.zeros(1, device=dev, dtype=torch.int64)
    monkeypatch.setattr(ops, "_cur_device", lambda: 1)        # as if cuda:1 were current while the tensors are on cuda:0
    with pytest.raises(ValueError, match="current device"):
        ops.wav_resample(src, [(0, 64, 1, 0)], taps, klo, t.P, t.Q, t.W, wave, lengths)
    assert not launched
    monkeypatch.undo()
    paths, _, _ = _three_files(tmp_path)
    assert torch.cuda.current_device() == 0
    with pytest.raises(ValueError, match="current device"):
        data_io.load_batch(paths, torch.device("cuda:1"))
    with pytest.raises(ValueError, match="no CPU fallback"):
        data_io.load_batch(paths, "cpu")


def test_launcher_refuses_what_ops_refuses():
    """The same preconditions once more behind the C ABI: hipErrorInvalidValue (1), nothing launched."""
    import ctypes
    from fddm_hip._lib import lib
    t, taps, klo = A.device_taps(48000, dev)
    src = torch.zeros(9 * 64, device=dev)
    wave = torch.full((2, 64), float("nan"), device=dev)
    lengths = torch.full((2,), -7, device=dev, dtype=torch.int64)

    def launch(desc, NT=t.NT, P=t.P, Q=t.Q, W=t.W, T=64):
        flat = (ctypes.c_long * len(desc))(*desc)
        return lib().fddm_wav_resample(src.data_ptr(), src.numel(), flat, len(desc) // 4, taps.data_ptr(), klo.data_ptr(),
                                       NT, P, Q, W, wave.data_ptr(), lengths.data_ptr(), 2, T, ops.stream())

    assert launch([0, 64, 9, 0]) == 1
    assert launch([0, 64, 0, 0]) == 1
    assert launch([0, 577, 1, 0]) == 1
    assert launch([0, 64, 1, 2]) == 1
    assert launch([0, 64, 1, 0], NT=t.KT + 1) == 1
    assert launch([0, 64, 1, 0], Q=4096) == 1
    assert launch([0, 64, 1, 0], P=0) == 1
    assert launch([0, 64, 1, 0], T=0) == 1
    assert launch([0, 64, 1, 0, 64, 64, 1, 0]) == 1          # one row twice
    assert launch([577, 0, 1, 0]) == 1                       # an empty clip past the end of src
    torch.cuda.synchronize()
    assert torch.isnan(wave).all() and lengths.tolist() == [-7, -7]
    assert launch([0, 64, 1, 1]) == 0
    torch.cuda.synchronize()
    assert torch.isnan(wave[0]).all() and lengths.tolist() == [-7, 22] and (wave[1] == 0).all()
