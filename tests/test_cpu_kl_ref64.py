"""helpers.kl_term_ref64 (the float64 reference of tests/test_gpu_kl_softmax.py) checked on the CPU: its closed-form
gradient against autograd through its own per-token KL, and its loss and gradient against the fixture recorded from
the reference implementation and against the fp32 oracle."""
import torch

from helpers import T, kl_term_ref64, load
from oracle import fddm_oracle as O


def _case(V, masked, seed):
    gen = torch.Generator().manual_seed(seed)
    B, L = 4, 6
    betas, _ = O.sched_tables(200)
    logits = 3.0 * torch.randn(B, L, V, generator=gen)
    x0 = torch.randint(0, V, (B, L), generator=gen)
    xt = torch.randint(0, V, (B, L), generator=gen)
    xt[:, ::3] = x0[:, ::3]
    xt[0, 1], x0[0, 1] = 0, V - 1
    t = torch.tensor([1, 2, 117, 200])
    xm = None
    if masked:
        xm = torch.ones(B, L, dtype=torch.bool)
        xm[1] = False
        xm[2, 1:] = False
    return logits, xt, x0, t, xm, betas


def test_ref64_gradient_is_the_derivative_of_its_loss():
    for V, masked in ((36, True), (1000, False)):
        logits, xt, x0, t, xm, betas = _case(V, masked, 5)
        z = logits.double().requires_grad_(True)
        kl_tok, dz, w, s = kl_term_ref64(z, xt, x0, t, xm, betas)
        (kl_tok * w).sum().backward()
        # float64 on both sides: 1e-9 of the error scale (the closed form treats eps as the code does: P + eps
        # and d_p + eps enter the derivative exactly)
        assert ((z.grad - dz.detach()).abs() <= 1e-9 * s.detach() + 1e-300).all()
        assert (s.detach() >= dz.detach().abs() * (1 - 1e-12)).all(), "s_k bounds |dz_k| term by term"
        if masked:
            assert (dz.detach()[w == 0] == 0).all() and torch.isfinite(kl_tok).all()


def test_ref64_matches_fixture_and_fp32_oracle():
    gk = load("kl")
    logits, xt, x0, t, xm, betas = (T(gk[n]) for n in ("logits", "xt", "x0", "t", "x_mask", "betas"))
    kl_tok, dz, w, s = kl_term_ref64(logits, xt, x0, t, xm, betas)
    loss = (kl_tok * w).sum()
    assert abs(loss.item() - float(gk["kl"])) <= 1e-5 * abs(float(gk["kl"]))
    ref = T(gk["dlogits"]).double()
    assert ((dz - ref).abs() <= 1e-4 * ref.abs().max()).all()
    for V, masked in ((36, True), (1000, False)):
        args = _case(V, masked, 6)
        kl_tok, dz, w, s = kl_term_ref64(*args)
        loss32, dz32 = O.kl_term(*args)
        assert abs(loss32.item() - (kl_tok * w).sum().item()) <= 1e-6 * abs(loss32.item())
        # the fp32 oracle against float64, per element: measured 2.45e-6 s_k at most over the GPU test's cases
        assert ((dz32.double() - dz).abs() <= 1e-5 * s).all()
