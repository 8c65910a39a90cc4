"""Inference entry point (drop-in for the reference's inference.py): audio files -> acoustic condition -> jumpy
sampling -> text, from one WAV or from a CSV with a `path` column.

    python inference.py --wav clip.wav --ckpt ckpts/ep001.pt --main-config configs/fddm_zhTW_base.yaml \\
        --diffusion-config configs/diffusion.yaml --tokenizer data/tokenizer/zh-TW_A/spm_zhTW_A.model --greedy
    python inference.py --csv test.csv --batch-size 16 ... --out-json results.json

Same function names, flags, defaults and result dict as the reference (inference.py:53-346). What is added:

* Audio decode on the GPU. `load_wav` reads the RIFF container on the host and hands the raw interleaved samples to
  libfddm_hip's `fddm_wav_resample` (csrc/audio.hip): channel mean and torchaudio's Hann-windowed sinc resampler
  (lowpass_filter_width 6, rolloff 0.99) to 16 kHz in one launch. torchaudio is not needed.
* Batching. `infer_batch` runs padded batches through `data_io.load_batch` -> `encoder(wave, lengths)` ->
  `sampler.sample(..., c_mask=feat_mask, graph=...)`; `--batch-size N` (default 1) uses it on chunks of N CSV rows.
  With N = 1, and for `--wav`, the flow is the reference's `infer_one`: batch 1, no lengths, no mask.

* `--gpu N` makes N the current device (`main`), and `load_wav` / `infer_one` / `infer_batch` run under
  `torch.cuda.device(device)`: libfddm_hip launches on the current device, wherever the tensors live.

Deviations from the reference:

* `SimpleTokenizerAdapter` loads through `data_io.load_tokenizer`: a missing `.model` falls back to the `.vocab`
  next to it (the reference ships only the `.vocab`).
* The CSV is read with the `csv` module; pandas is not required. Extra columns (`text`, ...) are ignored.
* `--out-json` without a directory part works (the reference calls `os.makedirs("")`, which raises).
* Nothing is downloaded: a hub name as `model.encoder.wavlm_name` gives WavLM-base geometry with random init, as
  everywhere in this tree (models/acoustic_encoder.py); pass a local HF-format directory to load weights.
* In a batch, a row that cannot be read fails alone: the chunk's other rows are transcribed as one smaller batch.
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import json
import os
from typing import Any, Dict, List, Optional

import torch

import data_io
from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
from models.acoustic_encoder import AcousticEncoder
from models.denoise_decoder import DenoisingTransformerDecoder
from sampler.jumpy_sampler import DiffusionJumpySampler


# ========================== basics
def load_wav(path: str, target_sr: int = 16000, device: Optional[torch.device] = None) -> torch.Tensor:
    """One WAV file as mono samples at `target_sr`, [1, T] on `device` (reference inference.py:53-61). The channel
    mean and the resampling run on the GPU; the clip is not cut."""
    if target_sr != data_io.TARGET_SR:
        raise ValueError(f"load_wav: target_sr {target_sr} (the GPU resampler's tables target {data_io.TARGET_SR} Hz)")
    device = torch.device(device) if device is not None else build_device(None)
    if device.type != "cuda":
        raise RuntimeError("load_wav: the audio front end is a GPU kernel; there is no CPU fallback")
    with _current(device):
        wave, _, _ = data_io.load_batch([path], device, max_seconds=None, min_samples=1)
    return wave


def build_device(gpu: Optional[int]) -> torch.device:
    if gpu is not None and torch.cuda.is_available():
        return torch.device(f"cuda:{gpu}")
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _current(device):
    """Context that makes `device` the current GPU: libfddm_hip launches on the current device's current stream
    (fddm_hip.ops.stream), whatever device the tensors live on, so work for cuda:N must run with N current."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is not None:      # a bare "cuda" already means the current device
        return torch.cuda.device(device)
    return contextlib.nullcontext()


# ========================== modules
def _yaml(path: str) -> dict:
    import yaml
    with open(path, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


def _build_scheduler(diffusion_config_path: str, main_config_path: str, device: torch.device) -> DiscreteDiffusionScheduler:
    diffusion_config = _yaml(diffusion_config_path)
    main_config = _yaml(main_config_path)
    return DiscreteDiffusionScheduler(K=main_config["data"]["vocab_size"], T=diffusion_config["diffusion"]["T"],
                                      device=device, beta_max=diffusion_config["diffusion"]["beta_max"])


def _build_acoustic_encoder(main_config_path: str, device: torch.device) -> AcousticEncoder:
    main_config = _yaml(main_config_path)
    ec = main_config["model"]["encoder"]
    encoder = AcousticEncoder(wavlm_name=ec["wavlm_name"], freeze=ec["freeze"], d_model=main_config["model"]["d_model"],
                              proj=ec["proj"], pooling=ec["pooling"]).to(device)
    encoder.eval()
    if ec["freeze"]:
        for p in encoder.parameters():
            p.requires_grad = False
    return encoder


def _build_decoder(ckpt_path: str, main_config_path: str, device: torch.device) -> DenoisingTransformerDecoder:
    main_config = _yaml(main_config_path)
    m = main_config["model"]
    decoder = DenoisingTransformerDecoder(vocab_size=main_config["data"]["vocab_size"], d_model=m["d_model"],
                                          nhead=m["nhead"], num_layers=m["num_layers"], dim_ff=m["dim_ff"],
                                          dropout=m["dropout"], max_len=1024, pad_id=main_config["data"]["pad_id"])
    sd = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if "decoder" in sd:             # a train.py checkpoint holds several state_dicts
        sd = sd["decoder"]
    elif "state_dict" in sd:
        sd = sd["state_dict"]
    decoder.load_state_dict(sd, strict=False)
    decoder = decoder.to(device)
    decoder.eval()
    return decoder


# ========================== condition and tokenizer
def extract_condition(encoder: AcousticEncoder, wav: torch.Tensor) -> torch.Tensor:
    """[1, T] waveform -> condition [1, N, D]."""
    with torch.no_grad():
        feats, _, _ = encoder(wav)
    return feats


class SimpleTokenizerAdapter:
    """encode / decode / vocab_size over SentencePiece (data_io.load_tokenizer: the `.model`, or the BPE model rebuilt
    from the `.vocab` next to it)."""

    def __init__(self, spm_path: str):
        self.spm = data_io.load_tokenizer(spm_path)

    @property
    def vocab_size(self) -> int:
        return self.spm.vocab_size()

    def encode(self, text: str) -> List[int]:
        return self.spm.encode(text, out_type=int)

    def decode(self, ids: List[int]) -> str:
        return self.spm.decode(ids)


def _sampler(scheduler, decoder, tokenizer, T_infer, r, greedy, posterior_mode, device) -> DiffusionJumpySampler:
    return DiffusionJumpySampler(scheduler=scheduler, decoder=decoder, K=tokenizer.vocab_size,
                                 T_train=getattr(scheduler, "T", 200), T_infer=T_infer, r=r, greedy=greedy,
                                 posterior_mode=posterior_mode, temperature=1.0, device=device)


def _result(path, ids, tokenizer, T_infer, r, greedy, posterior_mode) -> Dict[str, Any]:
    return {"wav": path, "text": tokenizer.decode(ids), "ids": ids, "T_infer": T_infer, "r": r, "greedy": greedy,
            "posterior_mode": posterior_mode}


# ========================== one file (the reference's flow)
@torch.no_grad()
def infer_one(wav_path: str, scheduler: DiscreteDiffusionScheduler, encoder: AcousticEncoder,
              decoder: DenoisingTransformerDecoder, tokenizer: SimpleTokenizerAdapter, T_infer: int, r: int, greedy: bool,
              posterior_mode: str, seq_len: Optional[int], device: torch.device) -> Dict[str, Any]:
    if seq_len is None:
        seq_len = 64
    with _current(device):
        wav = load_wav(wav_path, target_sr=16000, device=device)      # [1, T]
        cond_c = extract_condition(encoder, wav)                      # [1, N, D]
        sampler = _sampler(scheduler, decoder, tokenizer, T_infer, r, greedy, posterior_mode, device)
        x0_idx, _ = sampler.sample(cond_c=cond_c, seq_len=seq_len, init="uniform", return_probs=False)
    return _result(wav_path, x0_idx[0].tolist(), tokenizer, T_infer, r, greedy, posterior_mode)


# ========================== padded batches
@torch.no_grad()
def infer_batch(paths, scheduler: DiscreteDiffusionScheduler, encoder: AcousticEncoder,
                decoder: DenoisingTransformerDecoder, tokenizer: SimpleTokenizerAdapter, T_infer: int, r: int,
                greedy: bool, posterior_mode: str, seq_len: Optional[int], device: torch.device,
                graph: bool = True) -> List[Dict[str, Any]]:
    """One padded batch: data_io.load_batch -> encoder(wave, lengths) -> sampler.sample(c_mask=feat_mask) -> one result
    dict per path, in order."""
    paths = list(paths)
    if seq_len is None:
        seq_len = 64
    with _current(device):
        wave, lengths, _ = data_io.load_batch(paths, device)
        feats, feat_mask, _ = encoder(wave, lengths)
        sampler = _sampler(scheduler, decoder, tokenizer, T_infer, r, greedy, posterior_mode, device)
        x0_idx, _ = sampler.sample(cond_c=feats, seq_len=seq_len, init="uniform", c_mask=feat_mask, graph=graph,
                                   return_probs=False)
    return [_result(p, ids, tokenizer, T_infer, r, greedy, posterior_mode) for p, ids in zip(paths, x0_idx.tolist())]


def _infer_chunk(chunk: List[str], common: dict) -> List[Dict[str, Any]]:
    """infer_batch on a CSV chunk; when it fails, each row is checked on its own (`data_io.read_wav` and the length
    rule of load_batch), the failing rows become {"wav", "error"} and the others run as one smaller batch. The failure
    path reads and parses the chunk's files a second time; the normal path reads each file once."""
    try:
        return infer_batch(chunk, **common)
    except Exception as e:
        whole = str(e)
    errors = {}
    for p in chunk:
        try:
            data_io.check_clip(p)
        except Exception as e:
            errors[p] = str(e)
    good = [p for p in chunk if p not in errors]
    done = {}
    if errors and good:
        try:
            done = {r["wav"]: r for r in infer_batch(good, **common)}
        except Exception as e:
            whole = str(e)
    return [done[p] if p in done else {"wav": p, "error": errors.get(p, whole)} for p in chunk]


def read_csv_paths(csv_path: str) -> List[str]:
    """The `path` column of a CSV (other columns, e.g. `text`, are ignored)."""
    with open(csv_path, "r", encoding="utf-8", newline="") as f:
        reader = csv.DictReader(f)
        if reader.fieldnames is None or "path" not in reader.fieldnames:
            raise ValueError(f"{csv_path}: no `path` column (columns: {reader.fieldnames})")
        return [row["path"] for row in reader]


# ========================== CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="FDDM-ASR Inference (Jumpy Sampling + Greedy)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--wav", type=str, help="one audio file (.wav)")
    src.add_argument("--csv", type=str, help="CSV with a `path` column")

    p.add_argument("--ckpt", type=str, required=True, help="decoder weights (.pt/.ckpt)")
    p.add_argument("--main-config", type=str, required=True, help="main config (configs/fddm_zhTW_base.yaml)")
    p.add_argument("--diffusion-config", type=str, required=True, help="configs/diffusion.yaml")
    p.add_argument("--tokenizer", type=str, required=True, help="SentencePiece model (.model)")

    p.add_argument("--T-infer", type=int, default=20, help="inference steps (10-50)")
    p.add_argument("--r", type=int, default=5, help="jump length")
    p.add_argument("--greedy", action="store_true", help="greedy decoding (argmax)")
    p.add_argument("--posterior-mode", type=str, default="average", choices=["average", "max"],
                   help="average or max posterior approximation")
    p.add_argument("--seq-len", type=int, default=None, help="output length (64 when not set)")

    p.add_argument("--gpu", type=int, default=None, help="GPU index")
    p.add_argument("--out-json", type=str, default=None, help="write the results to this JSON file")
    p.add_argument("--batch-size", type=int, default=1,
                   help="--csv: files per padded batch (1 = the reference's one-file flow)")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    device = build_device(args.gpu)
    if device.type == "cuda" and device.index is not None:
        torch.cuda.set_device(device)       # the kernels launch on the current device: make --gpu N that device

    scheduler = _build_scheduler(args.diffusion_config, args.main_config, device)
    encoder = _build_acoustic_encoder(args.main_config, device)
    decoder = _build_decoder(args.ckpt, args.main_config, device)
    tokenizer = SimpleTokenizerAdapter(args.tokenizer)
    common = dict(scheduler=scheduler, encoder=encoder, decoder=decoder, tokenizer=tokenizer, T_infer=args.T_infer,
                  r=args.r, greedy=args.greedy, posterior_mode=args.posterior_mode, seq_len=args.seq_len, device=device)

    results: List[Dict[str, Any]] = []
    if args.wav:
        res = infer_one(wav_path=args.wav, **common)
        results.append(res)
        print(json.dumps(res, ensure_ascii=False, indent=2))
    else:
        paths = read_csv_paths(args.csv)
        bs = max(1, args.batch_size)
        for i in range(0, len(paths), bs):
            chunk = paths[i:i + bs]
            if bs == 1:
                try:
                    out = [infer_one(wav_path=chunk[0], **common)]
                except Exception as e:
                    out = [{"wav": chunk[0], "error": str(e)}]
            else:
                out = _infer_chunk(chunk, common)
            for res in out:
                results.append(res)
                print(json.dumps(res, ensure_ascii=False))

    if args.out_json:
        d = os.path.dirname(args.out_json)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out_json, "w", encoding="utf-8") as f:
            json.dump(results, f, ensure_ascii=False, indent=2)
    return results


if __name__ == "__main__":
    main()
