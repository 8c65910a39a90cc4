"""Real-data input path: the reference's `CVZhTWDataset` (train.py:86-161) with the same
constructor, filtering, audio/token padding and item layout, built on what this image has offline.

* Audio. The reference reads `processed_path` with `librosa.load(path, sr=16000)`. Its preprocessor writes those
  clips as 16 kHz mono PCM_16 WAV (scripts/preprocess.py:118-135, `sf.write(..., subtype="PCM_16")`), for which
  librosa returns soundfile's float32 samples unchanged: int16 / 32768. `load_wav_16k` parses the RIFF/WAVE
  container itself (PCM 8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE) with the same integer scaling
  and librosa's channel mean for multi-channel files, so those clips load bit-identically. A clip at another rate
  is resampled with a polyphase filter (scipy.signal.resample_poly): librosa's default soxr_hq resampler is not
  in the image, so that case is close to, not identical with, the reference (never produced by its preprocessor).
* Inference audio. `read_wav` is that container parser with the channels kept apart; `load_batch` turns files of any
  rate and 1 - 8 channels into a padded 16 kHz batch on the GPU: the channel mean and torchaudio's sinc resampler (what
  the reference's inference.py:53-61 applies) run in `fddm_wav_resample` (csrc/audio.hip), one launch per source rate.
  `load_wav_16k` keeps its scipy resampler: the training path never meets another rate.
* Text. `tokenizer.encode(item["normalized_sentence"])` with the SentencePiece model at `tokenizer_vocab_path`.
  When the binary `.model` is absent (the reference ships only `spm_zhTW_A.vocab` + `vocab.json`),
  `load_tokenizer` rebuilds the BPE model from the `.vocab` (piece, score) table — the reference trains it as
  `model_type=bpe`, unk/bos/eos/pad = 0/1/2/3, default nmt_nfkc normalisation (scripts/tokenizer_train.py:91-124,
  configs/tokenizer_zhTW.yaml) — and hands it to SentencePiece's own BPE encoder, so ids and segmentation come from
  the same pieces, scores and normaliser as the reference's model.
"""
from __future__ import annotations

import io
import json
import os
import struct

import numpy as np
import torch
from torch.utils.data import Dataset

TARGET_SR = 16000

_WAVE_PCM, _WAVE_FLOAT, _WAVE_EXT = 1, 3, 0xFFFE


def read_wav(path: str):
    """(float32 samples [n, nch], sample rate) of a RIFF/WAVE file: the container parser and the integer scaling of
    `load_wav_16k` (PCM 8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE), channels kept apart."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, nch, sr, _, block, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == _WAVE_EXT and len(fmt) >= 26:
        tag = struct.unpack_from("<H", fmt, 24)[0]     # the sub-format GUID's first two bytes
    width = bits // 8
    n = len(data) // block
    raw = np.frombuffer(data[: n * block], dtype=np.uint8).reshape(n, nch, block // nch)[:, :, :width]
    if tag == _WAVE_PCM:
        if width == 1:
            x = (raw[..., 0].astype(np.float32) - 128.0) / 128.0
        elif width == 2:
            x = raw.copy().view("<i2")[..., 0].astype(np.float32) / 32768.0
        elif width == 3:
            v = raw[..., 0].astype(np.int32) | (raw[..., 1].astype(np.int32) << 8) | (raw[..., 2].astype(np.int32) << 16)
            v = np.where(v >= 1 << 23, v - (1 << 24), v)
            x = v.astype(np.float32) / float(1 << 23)
        elif width == 4:
            x = (raw.copy().view("<i4")[..., 0].astype(np.float64) / float(1 << 31)).astype(np.float32)
        else:
            raise ValueError(f"{path}: {bits}-bit PCM is not supported")
    elif tag == _WAVE_FLOAT and width in (4, 8):
        x = raw.copy().view("<f4" if width == 4 else "<f8")[..., 0].astype(np.float32)
    else:
        raise ValueError(f"{path}: WAVE format tag {tag:#x} is not supported")
    return x, sr


def load_wav_16k(path: str, target_sr: int = TARGET_SR) -> np.ndarray:
    """float32 mono samples of a RIFF/WAVE file at `target_sr` (librosa.load(path, sr=target_sr) for the
    reference's preprocessed clips; see the module docstring)."""
    x, sr = read_wav(path)
    nch = x.shape[1]
    x = x.mean(axis=1, dtype=np.float32) if nch > 1 else x[:, 0]   # librosa.to_mono: channel mean
    if sr != target_sr:
        from math import gcd

        from scipy.signal import resample_poly
        g = gcd(sr, target_sr)
        x = resample_poly(x, target_sr // g, sr // g).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


MIN_OUT_SAMPLES = 400      # the WavLM conv stack's receptive field: a shorter clip has no frame at all


def _clip(path: str, max_seconds, min_samples: int):
    """One file of a batch: (samples [n, nch] cut to max_seconds, rate, filter table, n_out, whether it was cut), or a
    ValueError naming the file."""
    from fddm_hip import audio, ops
    x, sr = read_wav(path)
    keep = x.shape[0] if max_seconds is None else min(x.shape[0], int(max_seconds * sr))
    was_cut = x.shape[0] > keep
    x = x[:keep]
    n, nch = x.shape
    if not 1 <= nch <= ops.WAV_MAX_CHANNELS:
        raise ValueError(f"{path}: {nch} channels (1 .. {ops.WAV_MAX_CHANNELS} are supported)")
    try:
        t = audio.sinc_resample_taps(sr)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    n_out = -((-n * t.P) // t.Q)
    if n_out < min_samples:
        raise ValueError(f"{path}: {n} frames at {sr} Hz give {n_out} samples at {TARGET_SR} Hz, fewer than the "
                         f"{min_samples} the encoder needs for one frame")
    return x, sr, t, n_out, was_cut


def check_clip(path: str, max_seconds=20.0, min_samples: int = MIN_OUT_SAMPLES) -> None:
    """Raises what load_batch would raise for this file alone (host only)."""
    _clip(str(path), max_seconds, min_samples)


def load_batch(paths, device, max_seconds=20.0, pad_to=None, min_samples: int = MIN_OUT_SAMPLES):
    """WAV files of any rates and channel counts -> (wave [B, T] f32, lengths [B] int64, info) on `device`: the
    inference front end (reference inference.py:53-61 per file — channel mean, torchaudio's sinc resampler to 16 kHz —
    here for a padded batch and on the GPU, fddm_hip.ops.wav_resample).

    Each file is read on the host and cut to `max_seconds` of source frames (20 s is the dataset's cap; None: no cut);
    the raw interleaved samples of the whole batch are packed into one buffer and copied to the device once; one launch
    per distinct source rate writes the rows. T is the longest output in the batch, or `pad_to`; samples past a row's
    length are zeros. info: sample_rates, channels, frames (after the cut), truncated (cut by max_seconds or by pad_to),
    launches. A clip with fewer than `min_samples` = 400 output samples raises a ValueError naming the file: the
    encoder would give it no frame, and the decoder a fully masked (NaN) entry."""
    from fddm_hip import audio, ops
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"load_batch: device {device}: the audio front end is a GPU kernel, there is no CPU fallback")
    if device.index is not None and device.index != torch.cuda.current_device():
        raise ValueError(f"load_batch: device {device} is not the current device (cuda:{torch.cuda.current_device()}); "
                         "the kernels launch on the current device: torch.cuda.set_device / torch.cuda.device first")
    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError("load_batch: no files")
    clips, desc, n_outs, cut = [], [], [], []
    off = 0
    for row, path in enumerate(paths):
        x, sr, _, n_out, was_cut = _clip(path, max_seconds, min_samples)
        n, nch = x.shape
        cut.append(was_cut)
        clips.append((off, x.reshape(-1)))
        desc.append((sr, (off, n, nch, row)))
        n_outs.append(n_out)
        off += (n * nch + 3) // 4 * 4       # clips start on 16-byte boundaries (the kernel's wide loads)
    T = int(pad_to) if pad_to is not None else max(n_outs)
    if T < 1:
        raise ValueError(f"load_batch: pad_to = {pad_to}")
    packed = np.zeros(off, dtype=np.float32)
    for o, flat in clips:
        packed[o:o + flat.size] = flat
    src = torch.from_numpy(packed).to(device)
    wave = torch.empty(len(paths), T, device=device, dtype=torch.float32)
    lengths = torch.empty(len(paths), device=device, dtype=torch.int64)
    rates = sorted({sr for sr, _ in desc})
    for sr in rates:
        t, taps, klo = audio.device_taps(sr, device)
        ops.wav_resample(src, [d for r, d in desc if r == sr], taps, klo, t.P, t.Q, t.W, wave, lengths)
    info = {"sample_rates": [sr for sr, _ in desc], "channels": [d[2] for _, d in desc],
            "frames": [d[1] for _, d in desc], "truncated": [c or n > T for c, n in zip(cut, n_outs)],
            "launches": len(rates)}
    return wave, lengths, info


def _nmt_nfkc_normalizer():
    """SentencePiece's built-in nmt_nfkc normaliser spec (its precompiled char map), taken from a throwaway
    model trained in memory — the rule the reference's tokenizer was trained with (the trainer's default)."""
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb
    w = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(["ab cd ef"] * 8), model_writer=w, vocab_size=12,
                                   model_type="bpe", normalization_rule_name="nmt_nfkc", minloglevel=2,
                                   unk_id=0, bos_id=1, eos_id=2, pad_id=3)
    m = pb.ModelProto()
    m.ParseFromString(w.getvalue())
    return m


def spm_model_from_vocab(vocab_path: str) -> bytes:
    """Serialized SentencePiece BPE ModelProto rebuilt from a `.vocab` (piece \\t score per line, id order)."""
    from sentencepiece import sentencepiece_model_pb2 as pb
    base = _nmt_nfkc_normalizer()
    m = pb.ModelProto()
    m.normalizer_spec.CopyFrom(base.normalizer_spec)
    m.trainer_spec.CopyFrom(base.trainer_spec)
    specials = {0: pb.ModelProto.SentencePiece.UNKNOWN, 1: pb.ModelProto.SentencePiece.CONTROL,
                2: pb.ModelProto.SentencePiece.CONTROL, 3: pb.ModelProto.SentencePiece.CONTROL}
    with open(vocab_path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f):
            line = line.rstrip("\n")
            if not line:
                continue
            piece, score = line.split("\t")
            p = m.pieces.add()
            p.piece = piece
            p.score = float(score)
            p.type = specials.get(i, pb.ModelProto.SentencePiece.NORMAL)
    m.trainer_spec.vocab_size = len(m.pieces)
    m.trainer_spec.model_type = pb.TrainerSpec.BPE
    m.trainer_spec.unk_id, m.trainer_spec.bos_id, m.trainer_spec.eos_id, m.trainer_spec.pad_id = 0, 1, 2, 3
    return m.SerializeToString()


def load_tokenizer(model_path: str):
    """SentencePieceProcessor for `model_path` (reference: `spm.SentencePieceProcessor().load(path)`); when only
    the `.vocab` next to it exists, the BPE model rebuilt from it (spm_model_from_vocab)."""
    import sentencepiece as spm
    tok = spm.SentencePieceProcessor()
    if os.path.exists(model_path):
        tok.load(model_path)
        return tok
    vocab = os.path.splitext(model_path)[0] + ".vocab"
    if not os.path.exists(vocab):
        raise FileNotFoundError(f"tokenizer: neither {model_path} nor {vocab} exists")
    tok.LoadFromSerializedProto(spm_model_from_vocab(vocab))
    return tok


class CVZhTWDataset(Dataset):
    """Reference train.py:86-161: items of `json_file` whose `processed_path` exists; each item is (wav float32
    [20 s x 16 kHz], truncated or zero-padded; token ids [max_len] with optional bos/eos, truncated or pad-filled)."""

    def __init__(self, json_file, tokenizer_vocab_path, max_len, pad_id, bos_id=None, eos_id=None):
        super().__init__()
        with open(json_file, "r", encoding="utf-8") as f:
            self.data = json.load(f)
        self.max_len, self.pad_id, self.bos_id, self.eos_id = max_len, pad_id, bos_id, eos_id
        self.tokenizer = load_tokenizer(tokenizer_vocab_path)
        self.max_audio_samples = 20 * TARGET_SR
        self.valid_indices = [i for i, it in enumerate(self.data)
                              if it.get("processed_path") and os.path.exists(it["processed_path"])]

    def __len__(self):
        return len(self.valid_indices)

    def __getitem__(self, idx):
        item = self.data[self.valid_indices[idx]]
        wav = torch.from_numpy(load_wav_16k(item["processed_path"]))
        if wav.numel() > self.max_audio_samples:
            wav = wav[: self.max_audio_samples]
        elif wav.numel() < self.max_audio_samples:
            wav = torch.cat([wav, torch.zeros(self.max_audio_samples - wav.numel())])
        tokens = list(self.tokenizer.encode(item["normalized_sentence"]))
        if self.bos_id is not None:
            tokens = [self.bos_id] + tokens
        if self.eos_id is not None:
            tokens = tokens + [self.eos_id]
        tokens = tokens[: self.max_len] + [self.pad_id] * max(0, self.max_len - len(tokens))
        return wav, torch.tensor(tokens, dtype=torch.long)
