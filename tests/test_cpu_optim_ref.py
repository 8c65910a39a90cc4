"""helpers.adamw_step_ref (the float64 reference of tests/test_gpu_optim.py) checked on the CPU, on the GPU test's own
inputs (helpers.adamw_params / adamw_grads / adamw_scenarios):
  * its torch form against torch.optim.AdamW(foreach=False) + clip_grad_norm_ on float64 parameters;
  * its default form (hyperparameters rounded to float32, as the C ABI receives them) against the torch form: the
    update term differs by at most 1e-5 s_u, all of it from forming 1 - b2 out of float(0.999) — a bounded, documented
    deviation of the float ABI;
  * what evaluating the step in fp32, in the kernel's order, costs per element against float64 (helpers.ADAMW_E);
  * that the GPU test's bounds (helpers.adamw_bounds) tell a wrong hyperparameter from a right one, from the reference
    alone."""
import functools

import pytest
import torch

from helpers import (ADAMW_COUNTERS, ADAMW_E, ADAMW_HP, ADAMW_SKIP, ADAMW_TENSORS, _f32, adamw_bounds, adamw_grads,
                     adamw_hp, adamw_params, adamw_scenario_grads, adamw_scenarios, adamw_step_ref, sumsq64)

SCEN = adamw_scenarios()
NAMES = [t[0] for t in ADAMW_TENSORS]
KIND = {t[0]: (t[2], t[3]) for t in ADAMW_TENSORS}


@functools.lru_cache(maxsize=None)
def trajectory(scen):
    """The scenario's four steps with the state following the fp32 evaluation (as it does on the GPU): a list of
    (k, name, p, g, m, v, counter, total_sq, kwargs) with the state BEFORE step k. Computed once, never modified."""
    cfg = SCEN[scen]
    P = adamw_params()
    M = {n: torch.zeros_like(x) for n, x in P.items()}
    V = {n: torch.zeros_like(x) for n, x in P.items()}
    cnt = {n: 0.0 for n in P}
    out = []
    for k, c0 in enumerate(ADAMW_COUNTERS):
        G = adamw_scenario_grads(cfg, k)
        total = _f32(sumsq64(G))
        if c0 == 999.0:
            cnt = {n: 999.0 for n in P}
        for n, g in G.items():
            kw = dict(adamw_hp(n, cfg["groups"]), max_norm=cfg["max_norm"], grad_scale=cfg["grad_scale"])
            out.append((k, n, P[n], g, M[n], V[n], cnt[n], total, kw))
            P[n], M[n], V[n], _ = adamw_step_ref(P[n], g, M[n], V[n], cnt[n], total, dtype=torch.float32, **kw)
            cnt[n] += 1.0
    if cfg["groups"]:
        assert [c for k, n, *_, c, _, _ in out if n == "b"] == [0.0, 1.0, 999.0]
    return out


def units(err, scale):
    """max err / scale; an element whose scale is 0 must have no error at all."""
    z = scale == 0
    assert (err[z] == 0).all()
    return float((err[~z] / scale[~z]).max()) if (~z).any() else 0.0


@pytest.mark.parametrize("scen", list(SCEN))
def test_torch_form_matches_torch_adamw(scen):
    cfg = SCEN[scen]
    P0 = adamw_params()
    ps = {n: torch.nn.Parameter(x.double()) for n, x in P0.items()}
    if cfg["groups"]:
        groups = []
        for gi in (0, 1):
            hp = adamw_hp([t[0] for t in ADAMW_TENSORS if t[5] == gi][0], True)
            groups.append(dict(params=[ps[t[0]] for t in ADAMW_TENSORS if t[5] == gi], lr=hp["lr"],
                               weight_decay=hp["wd"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"]))
    else:
        hp = ADAMW_HP
        groups = [dict(params=list(ps.values()), lr=hp["lr"], weight_decay=hp["wd"], betas=(hp["b1"], hp["b2"]),
                       eps=hp["eps"])]
    opt = torch.optim.AdamW(groups, foreach=False)
    worst = 0.0
    for k in range(4):
        G = adamw_scenario_grads(cfg, k)
        before = {}
        for n, p in ps.items():
            st = opt.state.get(p, {})
            before[n] = (p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p),
                         st["exp_avg_sq"].clone() if st else torch.zeros_like(p), float(st["step"]) if st else 0.0)
            p.grad = G[n].double() * cfg["grad_scale"] if n in G else None
        if cfg["max_norm"] is not None:
            torch.nn.utils.clip_grad_norm_(list(ps.values()), cfg["max_norm"])
        opt.step()
        total = sumsq64(G)
        for n, g in G.items():
            p0, m0, v0, c0 = before[n]
            kw = dict(adamw_hp(n, cfg["groups"]), max_norm=cfg["max_norm"], grad_scale=cfg["grad_scale"])
            pr, mr, vr, sc = adamw_step_ref(p0, g, m0, v0, c0, total, torch_form=True, **kw)
            st = opt.state[ps[n]]
            assert float(st["step"]) == c0 + 1.0
            worst = max(worst, units((ps[n].detach() - pr).abs(), sc.s_p + sc.s_u),
                        units((st["exp_avg"] - mr).abs(), sc.s_m), units((st["exp_avg_sq"] - vr).abs(), sc.s_v))
        for n in ps:
            if n not in G:
                assert torch.equal(ps[n].detach(), before[n][0])
    print(f"{scen}: torch form against torch.optim.AdamW, worst {worst:.2e} of the scales")
    assert worst <= 1e-12


def test_abi_form_stays_within_1e5_of_torch_form():
    """float(0.999) is 0.999 - 1.0e-8, so the ABI's 1 - b2 is 1.00001e-3: v' and with it the update term differ from
    torch's by up to 5e-6 relative at step 1 (more once b2^t enters). Pinned, not removed: the C ABI keeps its floats."""
    worst = {}
    for scen in SCEN:
        for k, n, p, g, m, v, c, total, kw in trajectory(scen):
            _, _, _, a = adamw_step_ref(p, g, m, v, c, total, **kw)
            _, _, _, t = adamw_step_ref(p, g, m, v, c, total, torch_form=True, **kw)
            key = (kw["b2"],)
            worst[key] = max(worst.get(key, 0.0), units((a.u - t.u).abs(), t.s_u))
    print("ABI form against torch form, |du| / s_u:", {k: f"{w:.2e}" for k, w in worst.items()})
    assert max(worst.values()) <= 1e-5


def test_fp32_evaluation_constants():
    """ADAMW_E: the fp32 evaluation against float64 from the same state, per element, over every scenario and step."""
    mx = dict(P=0.0, U=0.0, M=0.0, V=0.0)
    for scen in SCEN:
        for k, n, p, g, m, v, c, total, kw in trajectory(scen):
            p64, m64, v64, s64 = adamw_step_ref(p, g, m, v, c, total, **kw)
            p32, m32, v32, s32 = adamw_step_ref(p, g, m, v, c, total, dtype=torch.float32, **kw)
            du = s32.u - s64.u
            dp = p32.double() - p64
            u24 = 2.0 ** -24
            mx["P"] = max(mx["P"], units((dp + du).abs(), s64.s_p) / u24)    # p' = p1 - u: dp + du is what is not du
            mx["U"] = max(mx["U"], units(du.abs(), s64.s_u) / u24)
            mx["M"] = max(mx["M"], units((m32.double() - m64).abs(), s64.s_m) / u24)
            mx["V"] = max(mx["V"], units((v32.double() - v64).abs(), s64.s_v) / u24)
    print("fp32 evaluation against float64, units of 2^-24 x scale:", {k: f"{w:.3f}" for k, w in mx.items()})
    for k in mx:
        assert ADAMW_E[k] / 1.1 <= mx[k] <= ADAMW_E[k] * 1.1, (k, mx[k], ADAMW_E[k])
    from helpers import ADAMW_C
    assert ADAMW_C * max(ADAMW_E.values()) <= 64


def _share(scen, names, ks, **mut):
    """Per (tensor, step index): the share of elements of p' that a one-step reference with the mutated hyperparameters
    moves by more than twice the GPU test's bound."""
    out = {}
    for k, n, p, g, m, v, c, total, kw in trajectory(scen):
        if n not in names or k not in ks:
            continue
        pr, _, _, sc = adamw_step_ref(p, g, m, v, c, total, **kw)
        pm, _, _, _ = adamw_step_ref(p, g, m, v, c, total, **dict(kw, **mut))
        out[(n, k)] = float(((pm - pr).abs() > 2.0 * adamw_bounds(sc)[0]).double().mean())
    return out


PLAIN = [s for s in SCEN if not SCEN[s]["groups"]]
UNIT = [n for n in NAMES if KIND[n][0] == "unit" and n != "f"]      # f has one element: no share to speak of
ZERO_LOGU = [n for n in NAMES if KIND[n] == ("zero", "logu")]


@pytest.mark.parametrize("scen", PLAIN)
def test_bounds_discriminate(scen):
    """At the first step from zero state b1 and b2 cancel out of Adam, so those two are judged at steps 2 and 3 (nonzero
    moments); weight decay at every step. eps is judged at step 1, where sqrt(v') / bc = |g'| is this step's log-uniform
    gradient alone and eps shows wherever |g'| is below ~1e-3 (later steps keep the largest of several independent
    draws in v, so fewer elements stay that small: 0.74^k of them without a clip)."""
    wd = _share(scen, UNIT, (0, 1, 2, 3), wd=0.0)
    e0 = _share(scen, ZERO_LOGU, (0,), eps=0.0)
    e6 = _share(scen, ZERO_LOGU, (0,), eps=1e-6)
    b2 = _share(scen, ZERO_LOGU, (1, 2), b2=0.99)
    b1 = _share(scen, ZERO_LOGU, (1, 2), b1=0.8)
    for what, sh, need in (("wd=0", wd, 0.9), ("eps=0", e0, 0.5), ("eps=1e-6", e6, 0.5), ("b2=0.99", b2, 0.5),
                           ("b1=0.8", b1, 0.5)):
        print(f"{scen} {what}: shares {min(sh.values()):.3f} .. {max(sh.values()):.3f}")
        assert sh and min(sh.values()) >= need, (what, sh)
