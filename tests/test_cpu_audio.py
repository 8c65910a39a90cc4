"""The host side of the audio front end (fddm_hip/audio.py, data_io.read_wav, inference.py's command line) and the
float64 restatement the GPU tests compare against (tests/audio_ref.py). torchaudio is not available, so the restatement
is checked on its own here: a resampled sine must be the same sine, and each one-off mutation of its indexing must move
its output by far more than the GPU tolerance."""
import csv
import os

import numpy as np
import pytest

import audio_ref as R
import data_io
from fddm_hip import _lib
from fddm_hip import audio as A
from test_cpu_data import _write_wav

GPU_TOL = 1e-4          # tests/test_gpu_audio.py


# ------------------------------------------------------------------------------------------ table builder
@pytest.mark.parametrize("rate", R.RATES)
def test_table_geometry_and_rounding(rate):
    t = A.sinc_resample_taps(rate)
    assert (t.P, t.Q, t.W, t.KT) == R.GEOMETRY[rate] == R.geometry(rate)[:4]
    h64 = R.table(rate)
    assert t.h.dtype == np.float32 and t.h.shape == h64.shape == (t.P, t.KT)
    # one rounding of the float64 value: 2^-24 relative; below the f32 normal range (the clamped region's ~1e-49
    # entries) the rounding is absolute, half the subnormal spacing 2^-149
    err = np.abs(t.h.astype(np.float64) - h64)
    assert (err <= 2.0 ** -24 * np.abs(h64) + 2.0 ** -150).all(), float((err / np.maximum(np.abs(h64), 1e-300)).max())
    np.testing.assert_allclose(A.sinc_resample_table64(rate), h64, rtol=1e-12, atol=1e-18)
    assert np.abs(h64).sum(axis=1).max() <= 1.87


def test_largest_tap_sum_is_at_8k():
    sums = {r: np.abs(R.table(r)).sum(axis=1).max() for r in R.RATES}
    assert max(sums, key=sums.get) in (8000, 11025)       # the two share min(Q, P) * rolloff / Q = 0.99
    assert 1.86 < sums[8000] <= 1.87


@pytest.mark.parametrize("rate", R.RATES + (16000,))
def test_compact_table_is_the_table(rate):
    """klo / compact hold every entry of at least 1e-20, in place; what is left out changes no output beyond 1e-18."""
    t = A.sinc_resample_taps(rate)
    NT = t.NT
    assert t.compact.shape == (NT, t.P) and t.compact.dtype == np.float32 and t.klo.dtype == np.int32
    assert (t.klo >= 0).all() and (t.klo + NT <= t.KT).all()
    full = np.zeros_like(t.h)
    for p in range(t.P):
        full[p, t.klo[p]:t.klo[p] + NT] = t.compact[:, p]
    kept = np.abs(t.h) >= 1e-20
    np.testing.assert_array_equal(full[kept], t.h[kept])
    assert (full[~kept] == 0).all()
    assert np.abs(t.h[~kept]).sum(axis=None) <= 1e-18
    if rate == 44100:
        assert NT == 34               # the live taps per phase, of 475
    if rate == 16000:
        assert (t.P, t.Q, t.W, t.KT, NT) == (1, 1, 0, 1, 1) and t.compact[0, 0] == np.float32(1.0)


def test_rates_beyond_the_kernel_limits_name_the_rate():
    with pytest.raises(ValueError, match="44101"):
        A.sinc_resample_taps(44101)           # P = 16000, Q = 44101: a 7e8-entry table
    with pytest.raises(ValueError, match="384000"):
        A.sinc_resample_taps(384000)          # 24 source frames per output: the block's span outgrows LDS
    for r in R.RATES + (16000,):
        t = A.sinc_resample_taps(r)
        assert A.lds_span_bytes(t.P, t.Q, t.KT) <= A.LDS_MAX_BYTES


# ------------------------------------------------------------------------ the restatement, on its own
@pytest.mark.parametrize("rate", R.RATES)
def test_reference_resamples_a_sine_to_the_same_sine(rate):
    n = int(round(0.1 * rate))
    x = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / rate)
    y = R.resample(x, rate)
    P, Q = R.geometry(rate)[:2]
    assert y.shape[0] == -((-n * P) // Q) == R.n_out(n, rate)
    want = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(y.shape[0]) / 16000.0)
    err = np.abs(y - want)[200:-200].max()
    print(f"{rate} Hz: sine error {err:.2e}")
    assert err <= 1e-3


@pytest.mark.parametrize("rate", [8000, 24000, 44100])      # P = 2, 2, 160: a phase off by one is another row
@pytest.mark.parametrize("mutant", ["phase", "W", "Q+1", "Q-1", "channel"])
def test_reference_mutants_move_far_beyond_the_gpu_tolerance(rate, mutant):
    rng = np.random.default_rng(rate)
    Q = R.geometry(rate)[1]
    x = rng.uniform(-1, 1, size=(3 * Q * 16 + 5, 2)).astype(np.float32)
    good = R.resample(R.channel_mean(x), rate)
    if mutant == "channel":
        bad = R.resample(x[:, 0], rate)
    else:
        kw = {"phase": dict(phase_shift=1), "W": dict(w_shift=1), "Q+1": dict(q_shift=1), "Q-1": dict(q_shift=-1)}[mutant]
        bad = R.resample(R.channel_mean(x), rate, **kw)
    moved = np.abs(good - bad)
    assert moved.max() > 0.1 and np.median(moved) > 100 * GPU_TOL, (moved.max(), np.median(moved))


def test_reference_zero_tail_and_identity():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, size=(700, 1)).astype(np.float32)
    y, n = R.resample_clip(x, 48000, T=300)
    assert n == 234 and y.shape == (300,) and (y[234:] == 0).all() and (y[:234] != 0).all()
    y, n = R.resample_clip(x, 48000, T=100)
    assert n == 100 and np.array_equal(y, R.resample_clip(x, 48000)[0][:100])
    y, n = R.resample_clip(x, 16000)
    assert n == 700 and np.array_equal(y, x[:, 0].astype(np.float64))
    y, n = R.resample_clip(np.zeros((0, 2), np.float32), 44100, T=5)
    assert n == 0 and (y == 0).all()


# ------------------------------------------------------------------------------------- read_wav
def test_read_wav_and_host_mean_reproduce_load_wav_16k(tmp_path):
    rng = np.random.default_rng(0)
    files = {
        "m16.wav": (rng.integers(-32768, 32768, size=(4000, 1)), {}),
        "s16.wav": (rng.integers(-32768, 32768, size=(3000, 2)), {}),
        "c24.wav": (rng.integers(-(1 << 23), 1 << 23, size=(500, 1)), dict(bits=24)),
        "f32.wav": ((rng.standard_normal((700, 2)) * 0.3).astype(np.float32), dict(tag=3, bits=32)),
    }
    for name, (frames, kw) in files.items():
        path = str(tmp_path / name)
        _write_wav(path, frames, 16000, **kw)
        x, sr = data_io.read_wav(path)
        assert sr == 16000 and x.dtype == np.float32 and x.shape == frames.shape
        want = data_io.load_wav_16k(path)
        mono = x.mean(axis=1, dtype=np.float32) if x.shape[1] > 1 else x[:, 0]
        assert np.array_equal(mono, want), name
        assert np.array_equal(R.channel_mean(x), want), name      # the kernel's order: sum in channel order, then divide


def test_read_wav_keeps_other_rates_and_channels(tmp_path):
    x = np.random.default_rng(2).integers(-32768, 32768, size=(101, 3))
    _write_wav(tmp_path / "t.wav", x, 44100)
    got, sr = data_io.read_wav(str(tmp_path / "t.wav"))
    assert sr == 44100 and np.array_equal(got, (x / 32768.0).astype(np.float32))


def test_check_clip_names_a_short_file(tmp_path):
    _write_wav(tmp_path / "short.wav", np.zeros((480, 1), dtype=np.int64), 48000)       # 10 ms -> 160 samples
    with pytest.raises(ValueError, match="short.wav"):
        data_io.check_clip(str(tmp_path / "short.wav"))
    _write_wav(tmp_path / "ok.wav", np.zeros((1200, 1), dtype=np.int64), 48000)          # 400 samples
    data_io.check_clip(str(tmp_path / "ok.wav"))


# ------------------------------------------------------------------------------------- boundary
def test_header_declares_the_entry_point():
    decls = _lib.parse_header()
    assert "fddm_wav_resample" in decls
    res, args = decls["fddm_wav_resample"]
    assert len(args) == 15


# ------------------------------------------------------------------------------------- command line
REQUIRED = ["--ckpt", "c.pt", "--main-config", "m.yaml", "--diffusion-config", "d.yaml", "--tokenizer", "t.model"]


def test_parse_args_flags_and_defaults():
    import inference
    a = inference.parse_args(["--wav", "x.wav"] + REQUIRED)
    assert (a.wav, a.csv, a.ckpt, a.main_config, a.diffusion_config, a.tokenizer) == \
        ("x.wav", None, "c.pt", "m.yaml", "d.yaml", "t.model")
    assert (a.T_infer, a.r, a.greedy, a.posterior_mode, a.seq_len, a.gpu, a.out_json, a.batch_size) == \
        (20, 5, False, "average", None, None, None, 1)
    b = inference.parse_args(["--csv", "x.csv", "--T-infer", "50", "--r", "10", "--greedy", "--posterior-mode", "max",
                              "--seq-len", "128", "--gpu", "0", "--out-json", "o.json", "--batch-size", "8"] + REQUIRED)
    assert (b.wav, b.csv, b.T_infer, b.r, b.greedy, b.posterior_mode, b.seq_len, b.gpu, b.out_json, b.batch_size) == \
        (None, "x.csv", 50, 10, True, "max", 128, 0, "o.json", 8)


@pytest.mark.parametrize("src", [[], ["--wav", "a.wav", "--csv", "b.csv"]])
def test_parse_args_wants_exactly_one_source(src, capsys):
    import inference
    with pytest.raises(SystemExit):
        inference.parse_args(src + REQUIRED)
    capsys.readouterr()


def test_parse_args_rejects_unknown_posterior_mode(capsys):
    import inference
    with pytest.raises(SystemExit):
        inference.parse_args(["--wav", "a.wav", "--posterior-mode", "map"] + REQUIRED)
    capsys.readouterr()


def test_reference_function_names_exist():
    import inference
    for name in ("load_wav", "build_device", "_build_scheduler", "_build_acoustic_encoder", "_build_decoder",
                 "extract_condition", "SimpleTokenizerAdapter", "infer_one", "infer_batch", "parse_args", "main"):
        assert callable(getattr(inference, name)), name


def test_csv_path_column(tmp_path):
    import inference
    p = tmp_path / "a.csv"
    with open(p, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["path", "text"])
        w.writerow(["clips/a b.wav", "今天, 天氣"])
        w.writerow(["clips/c.wav", ""])
    assert inference.read_csv_paths(str(p)) == ["clips/a b.wav", "clips/c.wav"]
    q = tmp_path / "b.csv"
    q.write_text("path\nx.wav\n", encoding="utf-8")
    assert inference.read_csv_paths(str(q)) == ["x.wav"]
    bad = tmp_path / "c.csv"
    bad.write_text("file,text\nx.wav,hi\n", encoding="utf-8")
    with pytest.raises(ValueError, match="path"):
        inference.read_csv_paths(str(bad))
