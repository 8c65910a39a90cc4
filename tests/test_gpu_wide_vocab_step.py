"""Vocabularies beyond the resident row kernels, end to end: train steps at V = 32776, 16387 and 16392 against the
oracle (they end in a ValueError of ops.kl_fwd / ops.softmax_rows without the streamed kernels), the no-grad KL route of
evaluate_validation_loss at V = 32772, and one sampler step at V = 50257 (which needs nothing new: fddm_jump takes
any V < 2^30)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import helpers as H
import wide_cases as W
from helpers import _dec_sd, _step_params, close
from oracle import fddm_oracle as O

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _rt():
    from fddm_hip import runtime as rt
    return rt


def make_decoder(V, d, H_, NL, FF):
    from models.denoise_decoder import DenoisingTransformerDecoder
    dec = DenoisingTransformerDecoder(vocab_size=V, d_model=d, nhead=H_, num_layers=NL, dim_ff=FF, dropout=0.0,
                                      max_len=1024, pad_id=0)
    sd = dec.state_dict()
    for n, v in _dec_sd(V, d, H_, NL, FF).items():
        sd[n] = v
    dec.load_state_dict(sd)
    return dec.to(dev)


def _spy(monkeypatch, names):
    """Count the calls of fddm_hip.ops functions `names` (the autograd Functions look them up on the module)."""
    from fddm_hip import ops
    seen = {n: 0 for n in names}
    for n in names:
        def wrap(*a, _f=getattr(ops, n), _n=n, **k):
            seen[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, n, wrap)
    return seen


# V = 32776 (V % 8 == 0, aligned rows), fp32 and bf16: the vector streamed KL, the streamed softmax forward, and in bf16
# the streamed softmax-backward + KL hand-over (fp32: the streamed f32 softmax backward). V = 16387 (odd), fp32: the
# scalar streamed KL in place of the two-pass form, and the streamed f32 softmax pair. V = 16392 (V % 8 == 0), bf16: the
# seam between the two families: the resident one-pass KL, the streamed softmax forward, then the resident
# fddm_softmax_bwd_add_bf16 hand-over on the streamed forward's bf16 probabilities.
@pytest.mark.parametrize("V,prec,tol", [(32776, "fp32", 1e-4), (32776, "bf16", 3e-2), (16387, "fp32", 1e-4),
                                        (16392, "bf16", 3e-2)])
def test_train_step_wide_vocab_matches_oracle(V, prec, tol, monkeypatch):
    """Two teacher-forced train_one_epoch steps (a KL step and an L_fd step) from the same condition as
    oracle_train_step, as tests/test_gpu_models.py::test_train_step_odd_vocab_matches_oracle does at V = 997, with its
    bars; the streamed kernels the step is expected to take are counted."""
    import train as T_
    from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
    from fddm_hip.optim import FusedAdamW
    from models.projection import SpeechProjector, TextEmbedding, TextProjector
    rt = _rt()
    d, Hh, NL, FF, B, L, S, Tn = 128, 2, 2, 256, 3, 24, 30, 20

    class Identity(nn.Module):      # the "encoder": the loader hands the acoustic condition itself
        def forward(self, c):
            return c, None, None

    gen = torch.Generator().manual_seed(12)
    conds = [torch.randn(B, S, d, generator=gen) for _ in range(2)]
    x0s = [torch.randint(1, V, (B, L), generator=gen) for _ in range(2)]
    x0s[0][1, 17:] = 0
    ts = [torch.tensor([1, 9, 20]), torch.tensor([4, 2, 13])]
    betas, ab = O.sched_tables(Tn)
    xts = [O.sample_xt(x0, t, V, ab, seed=5 + i) for i, (x0, t) in enumerate(zip(x0s, ts))]
    params = _step_params(V, d, NL, FF, Hh)
    rec = {"kl": [], "lfd": []}
    seen = _spy(monkeypatch, ("kl_fused", "kl_fused_wide", "softmax_rows_wide", "softmax_bwd_rows_wide",
                              "softmax_bwd_add_bf16", "softmax_bwd_add_bf16_wide"))
    with rt.use_precision(prec):
        dec = make_decoder(V, d, Hh, NL, FF)
        sp, te, tp = SpeechProjector(d, 256), TextEmbedding(V, 256), TextProjector(256, 256)
        for pre, m in (("s_proj.", sp), ("t_embed.", te), ("t_proj.", tp)):
            m.load_state_dict({n: params[pre + n] for n, _ in m.named_parameters()})
            m.to(dev)
        xq = iter([x.to(dev) for x in xts])
        tq = iter([t.to(dev) for t in ts])

        class TF(T_.SchedulerAdapter):
            def sample_q(self, x0, t):
                return next(xq)

            def kl_term(self, *a, **k):
                v = super().kl_term(*a, **k)
                rec["kl"].append(float(v.detach()))
                return v

        orig = T_.lfd_loss

        def rl(*a, **k):
            v = orig(*a, **k)
            rec["lfd"].append(float(v.detach()))
            return v

        monkeypatch.setattr(T_, "lfd_loss", rl)
        trainable = list(dec.parameters()) + list(sp.parameters()) + list(te.parameters()) + list(tp.parameters())
        opt = FusedAdamW(trainable, lr=2e-4, weight_decay=0.01)
        cfg = T_.Config(seed=1, data={"pad_id": 0}, model={}, diffusion={"T": Tn}, inference={}, optim={},
                        lfd={"n_step_fd": 4, "tau": 1.0, "lambda_offdiag": 5e-3}, log={"log_every": 1000})
        loader = list(zip(conds, x0s))
        T_.train_one_epoch(Identity(), dec, sp, te, tp, TF(DiscreteDiffusionScheduler(K=V, T=Tn, device=dev)), loader,
                           opt, dev, cfg, 3, None, 1, False, draw_t=lambda B_: next(tq))
        torch.cuda.synchronize()
    # both steps take one KL kernel (streamed unless the resident one-pass kernel serves V); the L_fd step the streamed
    # softmax forward and one backward form: the bf16 hand-over (streamed past V = 32768) or the streamed f32 backward
    from fddm_hip import ops
    handover = prec == "bf16" and V % 8 == 0
    kl_res = V % 4 == 0 and V <= ops.KL_FUSED_MAX_V
    want = {"kl_fused": 2 * int(kl_res), "kl_fused_wide": 2 * int(not kl_res), "softmax_rows_wide": 1,
            "softmax_bwd_rows_wide": int(not handover),
            "softmax_bwd_add_bf16": int(handover and V <= ops.SOFTMAX_ADD_MAX_V),
            "softmax_bwd_add_bf16_wide": int(handover and V > ops.SOFTMAX_ADD_MAX_V)}
    assert seen == want, (seen, want)
    ocfg = dict(d_model=d, nhead=Hh, num_layers=NL, pad_id=0, n_step_fd=4, tau=1.0, lambda_offdiag=5e-3)
    oopt = O.OracleAdamW()
    ref = [O.oracle_train_step(params, None, None, None, x0s[i], ts[i], xts[i], ocfg, oopt, 3 + i, betas, ab,
                               c=conds[i]) for i in range(2)]
    print(f"V={V} {prec}: kl {rec['kl']} vs {[r['kl'] for r in ref]}, lfd {rec['lfd']} vs {ref[1]['lfd']}")
    close(torch.tensor(rec["kl"]), torch.tensor([r["kl"] for r in ref]), rtol=tol, what=f"{prec} V={V} KL")
    close(torch.tensor(rec["lfd"]), torch.tensor([ref[1]["lfd"]]), rtol=tol, what=f"{prec} V={V} L_fd")
    final = {("decoder." + n): p.detach().cpu() for n, p in dec.named_parameters()}
    for pre, m in (("s_proj.", sp), ("t_embed.", te), ("t_proj.", tp)):
        final.update({pre + n: p.detach().cpu() for n, p in m.named_parameters()})
    init = _step_params(V, d, NL, FF, Hh)
    for n in ("decoder.head.weight", "decoder.head.bias", "decoder.blocks.0.ff.0.weight", "t_embed.proj.weight"):
        # update norms (AdamW's first steps move near-zero-gradient elements by ~lr in a direction rounding picks)
        got = float(((final[n].double() - init[n].double()) ** 2).sum())
        want = float(((params[n].double() - init[n].double()) ** 2).sum())
        assert abs(got - want) <= (5e-3 if prec == "fp32" else 5e-2) * want, f"{prec} V={V} update {n}: {got} vs {want}"


def test_kl_term_no_grad_wide_vocab_matches_float64(monkeypatch):
    """evaluate_validation_loss's route: SchedulerAdapter.kl_term under torch.no_grad() at V = 32772 takes the streamed
    forward-only kernel and returns the float64 mean over utterances of the masked per-utterance mean, within the
    per-token bound of tests/wide_cases.py carried through the weights (plus kl_reduce's 1e-6)."""
    import train as T_
    from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
    V = 32772
    c = W.kl_case(V, True)
    seen = _spy(monkeypatch, ("kl_fwd_wide", "kl_fwd"))
    sch = T_.SchedulerAdapter(DiscreteDiffusionScheduler(K=V, T=W.TN, device=dev))
    # the scheduler's own betas (they differ from the oracle's table in the last bit): the reference takes the same
    betas = sch.sch.betas.float().cpu()
    close(betas, c.betas, rtol=1e-6, atol=0.0, what="scheduler betas")
    kl, _, w, _ = H.kl_term_ref64(c.logits, c.xt, c.x0, c.t, c.xm, betas)
    want = (kl * w).sum().item()
    with torch.no_grad():
        loss = sch.kl_term(c.xt.to(dev), c.x0.to(dev), c.logits.to(dev), c.t.to(dev), c.xm.to(dev))
    assert seen == {"kl_fwd_wide": 1, "kl_fwd": 0}, seen
    A, R = W.tok_bounds(V)
    bound = (w * (A + R * kl.abs())).sum().item() + 1e-6 * abs(want)
    err = abs(float(loss) - want)
    print(f"no-grad KL at V={V}: {float(loss):.8f} vs {want:.8f}, |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_jump_greedy_exact_at_wide_vocab():
    """One greedy exact-mode sampler step at V = 50257 (odd: the scalar path, 786 passes), N = 5 rows, against
    helpers.jump_ref64 under helpers.jump_greedy_bound: the sampler serves wide vocabularies as it is."""
    from fddm_hip import ops
    V, N, L = 50257, 5, 1
    c = H.jump_case(V, N, L)
    ref = H.jump_ref64(c["logits"], c["xt"], c["coef"], L, mode=0)
    z = torch.from_numpy(np.array(c["logits"])).to(dev)
    nx, x0 = ops.jump(z, torch.from_numpy(np.array(c["xt"])).to(dev), torch.from_numpy(np.array(c["coef"])).to(dev), L,
                      mode=0, temperature=1.0, seed=0, rng_stream=H.JUMP_STREAM)
    nx, x0 = nx.cpu().numpy(), x0.cpu().numpy()
    assert np.array_equal(x0, ref.am)
    assert ((nx == ref.x) | (nx == ref.o)).all()
    off = nx != ref.choice
    k = np.abs(ref.margin) / H.jump_greedy_bound(ref, V)
    assert not (off & (k > 1.0)).any(), f"rows {np.nonzero(off & (k > 1.0))[0]} decided against the reference"
