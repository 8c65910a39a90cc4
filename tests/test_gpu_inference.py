"""inference.py on the GPU at C1 size (SMALL_WAVLM encoder; decoder V 8000, d 128, 4 heads, 2 layers, L 32;
scheduler T 10, T_infer 10, r 5; fp32 precision mode): the batched path equals the same pipeline run by hand, the
single-file path is the reference's unmasked batch-1 flow, and main() runs a CSV end to end. The audio front end
itself is pinned in tests/test_gpu_audio.py; x_T is pinned as in tests/test_gpu_e2e.py."""
import csv
import gzip
import json
import os

import numpy as np
import pytest
import torch

from helpers import SMALL_WAVLM
from test_gpu_audio import _three_files
from test_gpu_models import _encoder, make_decoder

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
V, d, H, NL, FF, L, Tn, R_ = 8000, 128, 4, 2, 2048, 32, 10, 5


def _tokenizer(tmp_path):
    import inference
    with gzip.open(os.path.join(GOLDEN, "spm_zhTW_A.vocab.gz")) as f:
        (tmp_path / "spm.vocab").write_bytes(f.read())
    tok = inference.SimpleTokenizerAdapter(str(tmp_path / "spm.model"))       # no .model: rebuilt from the .vocab
    assert tok.vocab_size == V
    return tok


def _models():
    from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
    enc = _encoder(SMALL_WAVLM, d)
    dec = make_decoder(V, d, H, NL, FF, dropout=0.1)
    dec.eval()
    return DiscreteDiffusionScheduler(K=V, T=Tn, device=dev, beta_max=0.2), enc, dec


def _pin_xT(monkeypatch, B, seed):
    from sampler import jumpy_sampler as JS
    xT = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(seed)).to(dev)
    monkeypatch.setattr(JS.torch, "randint", lambda low, high, size, device=None: xT.clone())


def _by_hand(sch, dec, cond, mask):
    from sampler.jumpy_sampler import DiffusionJumpySampler
    smp = DiffusionJumpySampler(sch, dec, K=V, T_train=Tn, T_infer=Tn, r=R_, greedy=True, posterior_mode="average",
                                temperature=1.0, device=dev)
    ids, probs = smp.sample(cond, seq_len=L, c_mask=mask, graph=False, return_probs=False)
    assert probs is None
    return ids.cpu()


def test_infer_batch_equals_the_pipeline_by_hand(tmp_path, monkeypatch):
    import data_io
    import inference
    from fddm_hip import runtime as rt
    paths, _, _ = _three_files(tmp_path)
    tok = _tokenizer(tmp_path)
    with rt.use_precision("fp32"):
        sch, enc, dec = _models()
        _pin_xT(monkeypatch, 3, seed=3)
        wave, lengths, _ = data_io.load_batch(paths, dev)
        feats, feat_mask, _ = enc(wave, lengths)
        assert feat_mask is not None and feat_mask.sum(1).tolist() == [15, 24, 10]     # min(ceil(len / 320), S = 24)
        want = _by_hand(sch, dec, feats, feat_mask)
        for graph in (True, False):
            res = inference.infer_batch(paths, sch, enc, dec, tok, T_infer=Tn, r=R_, greedy=True,
                                        posterior_mode="average", seq_len=L, device=dev, graph=graph)
            assert [r["wav"] for r in res] == paths
            got = torch.tensor([r["ids"] for r in res])
            assert torch.equal(got, want), f"graph={graph}: ids differ from the pipeline run by hand"
            for r in res:
                assert r["text"] == tok.decode(r["ids"])
                assert (r["T_infer"], r["r"], r["greedy"], r["posterior_mode"]) == (Tn, R_, True, "average")
                assert set(r) == {"wav", "text", "ids", "T_infer", "r", "greedy", "posterior_mode"}
    assert want.shape == (3, L)


def test_infer_one_is_the_unmasked_batch_1_flow(tmp_path, monkeypatch):
    import data_io
    import inference
    from fddm_hip import runtime as rt
    paths, _, _ = _three_files(tmp_path)
    tok = _tokenizer(tmp_path)
    with rt.use_precision("fp32"):
        sch, enc, dec = _models()
        _pin_xT(monkeypatch, 1, seed=4)
        wave = torch.from_numpy(data_io.load_wav_16k(paths[1]))[None].to(dev)           # the 16 kHz mono file
        assert torch.equal(inference.load_wav(paths[1], device=dev), wave)
        feats, mask, _ = enc(wave)
        assert mask is None
        want = _by_hand(sch, dec, feats, None)
        res = inference.infer_one(paths[1], sch, enc, dec, tok, T_infer=Tn, r=R_, greedy=True,
                                  posterior_mode="average", seq_len=L, device=dev)
    assert res["wav"] == paths[1] and res["ids"] == want[0].tolist() and res["text"] == tok.decode(res["ids"])
    # another rate through the same entry: [1, n_out] at 16 kHz
    w48 = inference.load_wav(paths[0], device=dev)
    assert w48.shape == (1, 4800) and w48.dtype == torch.float32 and torch.isfinite(w48).all()


def test_main_csv_end_to_end(tmp_path, monkeypatch, capsys):
    import yaml

    import inference
    import train as T_
    from fddm_hip import runtime as rt
    from models.projection import SpeechProjector, TextEmbedding, TextProjector
    monkeypatch.chdir(tmp_path)
    paths, _, _ = _three_files(tmp_path)
    _tokenizer(tmp_path)
    main_cfg = {"data": {"vocab_size": V, "pad_id": 0},
                "model": {"d_model": d, "nhead": H, "num_layers": NL, "dim_ff": FF, "dropout": 0.1,
                          "encoder": {"wavlm_name": {k: list(v) if isinstance(v, tuple) else v for k, v in SMALL_WAVLM.items()},
                                      "freeze": True, "proj": "linear", "pooling": "none"}}}
    with open("main.yaml", "w") as f:
        yaml.safe_dump(main_cfg, f)
    with open("diffusion.yaml", "w") as f:
        yaml.safe_dump({"diffusion": {"T": Tn, "beta_max": 0.2}}, f)
    dec = make_decoder(V, d, H, NL, FF, dropout=0.1)
    T_.save_checkpoint("ck.pt", dec, SpeechProjector(d, 256), TextEmbedding(V, 256), TextProjector(256, 256), 7, 1, main_cfg)
    with open("rows.csv", "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["path", "text"])
        w.writerow([paths[0], "你好"])
        w.writerow([str(tmp_path / "missing.wav"), ""])
    made_current = []
    real_set_device = torch.cuda.set_device
    monkeypatch.setattr(torch.cuda, "set_device", lambda dv: (made_current.append(torch.device(dv)), real_set_device(dv))[1])
    with rt.use_precision("fp32"):
        inference.main(["--csv", "rows.csv", "--ckpt", "ck.pt", "--main-config", "main.yaml", "--diffusion-config",
                        "diffusion.yaml", "--tokenizer", "spm.model", "--T-infer", str(Tn), "--r", str(R_), "--greedy",
                        "--seq-len", "24", "--batch-size", "2", "--gpu", "0", "--out-json", "out.json"])
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    with open("out.json", encoding="utf-8") as f:
        out = json.load(f)
    assert made_current == [torch.device("cuda:0")]        # --gpu N becomes the current device: the kernels launch there
    assert out == printed and len(out) == 2
    ok, err = out
    assert ok["wav"] == paths[0] and len(ok["ids"]) == 24 and isinstance(ok["text"], str)
    assert all(0 <= i < V for i in ok["ids"]) and (ok["T_infer"], ok["r"], ok["greedy"]) == (Tn, R_, True)
    assert set(err) == {"wav", "error"} and err["wav"].endswith("missing.wav") and "missing.wav" in err["error"]


def test_main_wav_prints_a_result(tmp_path, monkeypatch, capsys):
    """`python inference.py --wav some_48k_stereo.wav ...`: the single-file flow through main()."""
    import yaml

    import inference
    from fddm_hip import runtime as rt
    monkeypatch.chdir(tmp_path)
    paths, _, _ = _three_files(tmp_path)
    _tokenizer(tmp_path)
    main_cfg = {"data": {"vocab_size": V, "pad_id": 0},
                "model": {"d_model": d, "nhead": H, "num_layers": NL, "dim_ff": FF, "dropout": 0.1,
                          "encoder": {"wavlm_name": {k: list(v) if isinstance(v, tuple) else v for k, v in SMALL_WAVLM.items()},
                                      "freeze": True, "proj": "linear", "pooling": "none"}}}
    with open("main.yaml", "w") as f:
        yaml.safe_dump(main_cfg, f)
    with open("diffusion.yaml", "w") as f:
        yaml.safe_dump({"diffusion": {"T": Tn, "beta_max": 0.2}}, f)
    torch.save(make_decoder(V, d, H, NL, FF).state_dict(), "dec.pt")              # a bare state_dict loads too
    with rt.use_precision("fp32"):
        res = inference.main(["--wav", paths[0], "--ckpt", "dec.pt", "--main-config", "main.yaml", "--diffusion-config",
                              "diffusion.yaml", "--tokenizer", "spm.model", "--T-infer", str(Tn), "--greedy"])
    shown = json.loads(capsys.readouterr().out)
    assert shown == res[0] and shown["wav"] == paths[0] and len(shown["ids"]) == 64 and shown["r"] == 5
