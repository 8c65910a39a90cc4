"""The float64 reference of the jumpy-sampler step (helpers.jump_ref64), its fp32 emulation and the case table of
tests/test_gpu_jump.py, checked on the CPU from the reference alone: the reference reproduces the golden fixture and the
distribution the sampler's own torch code tempers, the RNG contract's u is strictly inside (0, 1), the stored constants
JUMP_E are what the emulation measures, and the conditions the GPU tests rely on hold (few rows inside their bound, the
constructed rows at +-4 bounds, one candidate class in nearly every sampled row, the extreme draws where they are said
to be)."""
import numpy as np
import pytest
import torch

import helpers as H
from helpers import T, jumpy_case_inputs, load
from oracle import fddm_oracle as O

U24 = 2.0 ** -24
EXACT, FAST, SAMPLE = 0, H.JUMP_FAST, H.JUMP_SAMPLE


def test_greedy_reference_reproduces_golden():
    """jump_ref64's greedy choice is the fixture's x_{t-delta} wherever oracle.jump_argmax's is, and agrees with
    jump_argmax on every row, margins included."""
    g = load("jumpy")
    b, _ = O.sched_tables(200, 0.2)
    for i in range(6):
        logits, xt = jumpy_case_inputs(i, 4, 48, 2000)
        t, delta = T(g[f"c{i}_t"]), int(g[f"c{i}_delta"])
        nx, margin = O.jump_argmax(logits, xt, t, delta, b.numpy(), 2000, 200)
        d = min(delta, int(t.min()))
        coef = np.asarray([O.jump_coeffs(b.numpy(), 2000, 200, int(tb), d) for tb in t], dtype=np.float32)
        ref = H.jump_ref64(logits.reshape(-1, 2000).numpy(), xt.reshape(-1).numpy(), coef, 48)
        assert np.array_equal(ref.choice, nx.reshape(-1).numpy()), f"case {i}"
        np.testing.assert_allclose(ref.margin, margin.reshape(-1).numpy(), rtol=1e-9, atol=1e-12)
        same = (nx == T(g[f"c{i}_next"])).reshape(-1).numpy()
        assert same.mean() > 0.99
        assert np.array_equal(ref.choice[same], g[f"c{i}_next"].reshape(-1)[same]), f"case {i}"
        assert np.array_equal(ref.am, logits.reshape(-1, 2000).argmax(-1).numpy())
        fast = H.jump_ref64(logits.reshape(-1, 2000).numpy(), xt.reshape(-1).numpy(), coef, 48, FAST)
        assert np.array_equal(fast.choice, fast.am)


@pytest.mark.parametrize("temp", H.JUMP_TEMPS)
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_sample_reference_is_the_tempered_posterior(mode, temp, monkeypatch):
    """softmax(score - g), the distribution a Gumbel-max race over jump_ref64's scores draws from, is what
    DiffusionJumpySampler._to_indices hands to Categorical for scheduler.q_posterior_multi_step (exact) or
    _mix_with_uniform (fast), to 1e-12. The sampler's and the scheduler's own expressions run in float64 for this
    (Tensor.float is patched to double during the call: their fp32 rounding of the probabilities is 1e-7)."""
    from fddm.sched.diffusion_scheduler import DiscreteDiffusionScheduler
    from sampler.jumpy_sampler import DiffusionJumpySampler
    V, B, L = 65, 3, 4
    gen = H._gen(7003, V)
    logits = 1.5 * torch.randn(B * L, V, generator=gen)
    if temp != 1.0:        # at temperature 1 the sampler passes its probabilities unclamped; the kernel always clamps
        logits[5] = H.JUMP_PEAK * torch.rand(V, generator=gen)
    xt = torch.randint(0, V, (B * L,), generator=gen)
    sch = DiscreteDiffusionScheduler(K=V, T=200, device=torch.device("cpu"), beta_max=0.2)
    # the C entry point takes the temperature as a float: the reference divides by that fp32 value, so does the sampler here
    smp = DiffusionJumpySampler(sch, None, K=V, T_train=200, T_infer=20, r=5, greedy=False,
                                temperature=float(np.float32(temp)), device=torch.device("cpu"))
    t, delta = torch.tensor([40, 5, 200]), 5
    if mode == "exact":
        coef = torch.stack(sch.multi_step_coeffs(t, delta), 1).float().numpy()
    else:
        ab = sch.alpha_bar[torch.tensor([150, 3, 77])]
        coef = torch.stack([ab, 0 * ab, 0 * ab, 0 * ab], 1).numpy()
    seen = []

    class Capture:
        def __init__(self, probs):
            seen.append(probs / probs.sum(-1, keepdim=True))        # Categorical normalises its probs

        def sample(self):
            return seen[-1].argmax(-1)

    monkeypatch.setattr(torch.distributions, "Categorical", Capture)
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self.double())
    p = torch.softmax(logits.double(), -1).view(B, L, V)
    if mode == "exact":
        oh = torch.nn.functional.one_hot(xt, V).double().view(B, L, V)
        post = sch.q_posterior_multi_step(oh, p, t, delta)
    else:
        post = smp._mix_with_uniform(p, T(coef[:, 0].astype(np.float64)))
    smp._to_indices(post)
    monkeypatch.undo()
    want = seen[0].reshape(B * L, V)
    assert want.dtype == torch.float64
    ref = H.jump_ref64(logits.numpy(), xt.numpy(), coef, L, SAMPLE | (FAST if mode == "fast" else 0), temp, 99, 7)
    got = torch.softmax(T(ref.score - ref.g), -1)
    assert (got - want).abs().max().item() <= 1e-12
    if temp != 1.0 and mode == "exact":            # batch element 1 has b_tg = 0: the peaked row reaches the clamp
        assert (ref.P[5] < 1e-12).sum() > V // 8


def test_contract_u_is_strictly_inside_the_unit_interval():
    """u = ((h >> 41) + 0.5) 2^-23 in fp32 is the float64 value, and 0 < u < 1, for h with its top bits all zero, all
    one and at 2^23 +- 1 (of contract v1's 24 bits); v1's expression gives exactly 1 for the top draw."""
    f = np.float32
    top24 = np.asarray([0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 2, 2 ** 24 - 1], dtype=np.uint64)
    for low in (0, 2 ** 40 - 1):
        h = (top24 << np.uint64(40)) | np.uint64(low)
        u32, u64 = O.jump_uniform(h, f), O.jump_uniform(h)
        assert u32.dtype == f and np.array_equal(u32.astype(np.float64), u64)
        assert (u32 > 0).all() and (u32 < 1).all()
        assert u64.min() == 2.0 ** -24 and u64.max() == 1.0 - 2.0 ** -24
        g = -np.log(-np.log(u32))
        assert np.isfinite(g).all() and g.dtype == f
        v1 = ((h >> np.uint64(40)).astype(f) + f(0.5)) * f(2.0 ** -24)
        assert v1.dtype == f and v1[-1] == f(1.0) and v1[-2] == f(0.9999999)
    idx = np.arange(64 * 256, dtype=np.uint64)
    for seed, row, k in H.JUMP_ONES:
        h = O.mix64(seed, H.JUMP_STREAM, idx)
        assert h[row * 256 + k] >> np.uint64(40) == np.uint64(0xFFFFFF)
        assert O.jump_uniform(h[row * 256 + k:][:1])[0] == 1.0 - 2.0 ** -24
    seed, row, k = H.JUMP_ZERO
    assert O.mix64(seed, H.JUMP_STREAM, idx)[row * 256 + k] >> np.uint64(41) == 0


def _paths(V):
    return (False, True) if V % 4 == 0 else (False,)


def test_greedy_constants_and_conditions():
    """JUMP_E["greedy"] is the emulation's largest excess over every case (both summation orders where V % 4 == 0);
    outside the constructed rows at most 1 % of rows lie within their bound; the constructed rows sit at 3 .. 5 bounds
    on their own side, in numbers; every kind of row is present and the tied rows tie where they say."""
    E, near, total, built = 0.0, 0, 0, {1: 0, -1: 0}
    kinds = {}
    for V in H.JUMP_V:
        for N, L in H.JUMP_NL:
            c = H.jump_case(V, N, L)
            ref, _ = H.jump_case_ref(V, N, L, EXACT)
            assert ref.ok.all()
            b = H.jump_greedy_bound(ref, V)
            for vec in _paths(V):
                m, _ = H.jump_emulate(c["logits"], c["xt"], c["coef"], L, EXACT, vector=vec)
                E = max(E, float((np.abs(m - ref.margin) / (U24 * ref.munit + 2.0 ** -50)).max()))
            free = c["built"] == 0
            near += int((np.abs(ref.margin[free]) <= b[free]).sum())
            total += int(free.sum())
            for s in (1, -1):
                sel = c["built"] == s
                built[s] += int(sel.sum())
                k = ref.margin[sel] / b[sel] * s
                assert ((k >= H.JUMP_BISECT_AT - 1) & (k <= H.JUMP_BISECT_AT + 1)).all(), (V, N, L, k)
                assert np.array_equal(ref.choice[sel], (ref.x if s > 0 else ref.o)[sel])
            z = c["logits"]
            B = (N + L - 1) // L
            assert len({tuple(r) for r in c["coef"]}) == B and c["coef"][B // 2, 2] == 1.0 and c["coef"][B // 2, 3] == 0.0
            assert len(set(c["coef_fast"][:, 0])) == B and c["coef_fast"][B // 2, 0] == 1.0
            for r, kind in enumerate(c["kinds"]):
                kinds[kind] = kinds.get(kind, 0) + 1
                top = z[r].max()
                if kind.startswith("tie"):
                    assert (z[r] == top).sum() == 2 and ref.am[r] == np.nonzero(z[r] == top)[0][0]
                if kind.startswith("ru") and V > 2:
                    assert ref.x[r] == ref.am[r] and (z[r] == top).sum() == 1
                    ru = np.sort(z[r])[-2]
                    assert (z[r] == ru).sum() == 2 and ref.o[r] == np.nonzero(z[r] == ru)[0][0]
                if kind == "const":
                    assert (z[r] == top).all() and ref.am[r] == 0 and ref.o[r] == (1 if ref.x[r] == 0 else 0)
                if kind == "ninf_x":
                    assert z[r, ref.x[r]] == -np.inf
            if N == 64:
                assert {int(v) for v in c["xt"]} >= {0, V - 1, -1, V + 5}
                assert (c["xt"] == ref.am).any() and ((c["xt"] != ref.am) & (c["xt"] >= 0) & (c["xt"] < V)).any()
    assert set(kinds) == set(H.JUMP_KINDS)
    print(f"\nJUMPREF greedy E {E:.3f} (stored {H.JUMP_E['greedy']}), {near} of {total} rows within their bound, "
          f"constructed rows {built}")
    assert E <= H.JUMP_E["greedy"] <= 1.1 * E + H.JUMP_E_FLOOR
    assert H.JUMP_C["greedy"] <= 64.0
    assert near <= 0.01 * total
    assert built[1] >= 60 and built[-1] >= 60


def test_tie_placements_cover_both_paths():
    """Two maxima in one float4, in one lane on consecutive passes of the scalar loop (k, k + 64) and of the float4 loop
    (k, k + 256), and in two lanes all occur, for the maximum and for the runner-up."""
    seen = set()
    for V in H.JUMP_V:
        c = H.jump_case(V, 64, 5)
        for r, kind in enumerate(c["kinds"]):
            if kind.startswith(("tie", "ru")) and V > 2:
                z = c["logits"][r]
                v = z.max() if kind.startswith("tie") else np.sort(z)[-2]
                k1, k2 = np.nonzero(z == v)[0]
                where = "4" if k1 // 4 == k2 // 4 else "256" if k2 - k1 == 256 else "64" if k2 - k1 == 64 else "2"
                seen.add((kind[:2], where, V % 4 == 0))
    for what in ("ti", "ru"):
        assert {(what, "4", True), (what, "4", False), (what, "64", False), (what, "256", True), (what, "2", True),
                (what, "2", False)} <= seen, seen


def test_sample_constants_and_conditions():
    """JUMP_E["sample"] is the emulation's largest excess over every sampled case; the emulation's own draw is a
    candidate in every row; the candidate set has one member in at least 98 % of rows; in the peaked case most P sit on the
    clamp."""
    E, multi, rows, clamped = 0.0, 0, 0, []
    for V in H.JUMP_SAMPLE_V:
        for N, L in H.JUMP_SAMPLE_NL:
            c = H.jump_case(V, N, L)
            for mode in (SAMPLE, SAMPLE | FAST):
                for temp in H.JUMP_TEMPS:
                    ref, seed = H.jump_case_ref(V, N, L, mode, temp)
                    cand = H.jump_candidates(ref)
                    multi += int((cand.sum(1) > 1).sum())
                    rows += N
                    assert cand[np.arange(N), ref.score.argmax(1)].all()
                    for vec in _paths(V):
                        _, sc = H.jump_emulate(c["logits"], c["xt"], c["coef_fast" if mode & FAST else "coef"], L, mode, temp,
                                               seed, H.JUMP_STREAM, vector=vec)
                        E = max(E, float((np.abs(sc - ref.score) / (U24 * ref.unit)).max()))
                        assert cand[np.arange(N), sc.argmax(1)].all(), (V, N, L, mode, temp)
    c = H.jump_peaked_case()
    for mode in (SAMPLE, SAMPLE | FAST):
        for temp in H.JUMP_TEMPS:
            cf = c["coef_fast" if mode & FAST else "coef"]
            ref = H.jump_ref64(c["logits"], c["xt"], cf, c["L"], mode, temp, c["seed"], H.JUMP_STREAM)
            cand = H.jump_candidates(ref)
            multi += int((cand.sum(1) > 1).sum())
            rows += c["N"]
            clamped += list((ref.P < 1e-12).mean(1))
            _, sc = H.jump_emulate(c["logits"], c["xt"], cf, c["L"], mode, temp, c["seed"], H.JUMP_STREAM, vector=True)
            E = max(E, float((np.abs(sc - ref.score) / (U24 * ref.unit)).max()))
            assert cand[np.arange(c["N"]), sc.argmax(1)].all()
    print(f"\nJUMPREF sample E {E:.3f} (stored {H.JUMP_E['sample']}), {multi} of {rows} rows with more than one candidate")
    assert E <= H.JUMP_E["sample"] <= 1.1 * E + H.JUMP_E_FLOOR
    assert H.JUMP_C["sample"] <= 64.0 and H.JUMP_K_DEV == max(H.JUMP_K.values())
    assert multi <= 0.02 * rows
    assert clamped and np.median(clamped) > 0.5


def test_rng_index_is_visible():
    """N = 64, V = 257: a transposed index (k N + row) or a row stride of V - 1 moves the draw out of the candidate
    set in a quarter of the rows at least (one class dominates the others), so the GPU test sees either."""
    V, N, L = 257, 64, 5
    c = H.jump_case(V, N, L)
    ref, seed = H.jump_case_ref(V, N, L, SAMPLE, 1.0)
    cand = H.jump_candidates(ref)
    r, k = np.arange(N, dtype=np.uint64)[:, None], np.arange(V, dtype=np.uint64)[None]
    for name, idx in (("transposed", k * np.uint64(N) + r), ("stride V - 1", r * np.uint64(V - 1) + k)):
        g = -np.log(-np.log(O.jump_uniform(O.mix64(seed, H.JUMP_STREAM, idx))))
        moved = ~cand[np.arange(N), (ref.lp + g).argmax(1)]
        assert moved.mean() >= 0.25, (name, moved.mean())


@pytest.mark.parametrize("which", [0, 1, 2, "zero"])
def test_extreme_draw_cases(which):
    """The all-ones draws: the class that draws it is under the clamp and the reference picks class 3 alone, by far more
    than the bound, while u = 1 (a Gumbel term of +inf) would pick the clamped class. The all-zero draw: its class has
    nearly all the mass and wins alone."""
    c = H.jump_extreme_case(which)
    for mode in (SAMPLE, SAMPLE | FAST):
        ref = H.jump_ref64(c["logits"], c["xt"], c["coef_fast" if mode & FAST else "coef"], c["L"], mode, 1.0, c["seed"],
                           H.JUMP_STREAM)
        cand = H.jump_candidates(ref)
        row, k = c["row"], c["k"]
        assert cand[row].sum() == 1
        gap = np.sort(ref.score[row])[-1] - np.sort(ref.score[row])[-2]
        assert gap > 100 * H.jump_sample_bound(ref)[row]
        if which == "zero":
            assert ref.score[row].argmax() == k and ref.g[row, k] == -np.log(-np.log(2.0 ** -24))
        else:
            assert ref.score[row].argmax() == 3 and ref.P[row, k] < 1e-12 and ref.P[row, 3] > 0.99
            assert ref.g[row, k] == -np.log(-np.log(1.0 - 2.0 ** -24)) and ref.score[row, 3] - ref.score[row, k] > 5.0
