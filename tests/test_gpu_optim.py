"""The optimizer kernels (csrc/optim.hip through fddm_hip.optim.FusedAdamW) per element against float64, and the two
companion kernels every weight and bias gradient passes through (ops.cast, ops.colsum in csrc/misc.hip).

One optimizer holds the ten tensors of helpers.ADAMW_TENSORS (475 408 elements, 13 chunks of MT_CHUNK = 65 536): a
tensor of one chunk less one element (vector loop + 3-element scalar tail), exactly one chunk, three chunks with a
one-element last chunk, 1-D tensors (no bf16 copy), 70 and 1 elements, and a parameter / gradient pair at element offset 1
of a larger buffer (both kernels' whole-tensor scalar path, across a chunk boundary). After every clip_and_step the
parameters, both moments, the step counters and last_total_sq are read back; the float64 reference of the NEXT step
(helpers.adamw_step_ref) starts from the GPU's own state and uses the GPU's own sum of squares, so nothing compounds and
the norm is judged on its own.

Bounds (helpers.adamw_bounds; set on the CPU by tests/test_cpu_optim_ref.py before any kernel ran):
    |p - p_ref| <= C 2^-24 (E_P s_p + E_U s_u),  |m - m_ref| <= C 2^-24 E_M s_m,  |v - v_ref| <= C 2^-24 E_V s_v
with E_P = 1.19, E_U = 6.17, E_M = 1.03, E_V = 1.98 what evaluating the step in fp32 in the kernel's order costs against
float64 on these very inputs, and C = 4: the kernel uses correctly rounded IEEE operations (no fast-math flag, sqrtf and
the division correctly rounded) and differs from that evaluation only by FMA contraction. C E <= 24.7, hard cap 64. The
CPU test also shows from the reference alone that these bounds tell wd = 0, eps = 0, eps = 1e-6, b2 = 0.99 and b1 = 0.8
from the right values on 0.74 - 1.0 of the elements of the tensors named there.

Gradient norm: last_total_sq within (1 + 2^-24)^NORM_DEPTH - 1 = 6.0e-6 of the float64 sum (hard cap 1e-5), the
worst case of fp32 summation of positive terms: NORM_DEPTH = 1 (the square) + 64 (accumulations per lane of the scalar
path over a full chunk; the vector path has 16 per accumulator + 2 combines) + 6 (wave) + 16 (cross-wave) + 13 (one atomic
per chunk) = 100 roundings on the longest path.

Measured on an MI355X (maxima over the four steps and all tensors; p in units of 2^-24 (E_P s_p + E_U s_u), m and v in
units of 2^-24 s_m and 2^-24 s_v, so the bounds are 4, 4.12 and 7.92; the norm relative to float64):
    scenario             precision   p      m      v      norm
    clipped              fp32        0.65   0.95   1.97   1.1e-7
    not_clipped          fp32        0.61   0.95   1.94   1.1e-7
    no_clip              fp32        0.61   0.95   1.98   1.3e-7
    scaled_clipped       fp32        0.65   0.95   1.97   1.1e-7
    scaled_not_clipped   fp32        0.61   0.95   1.94   1.1e-7
    groups               fp32        0.66   0.95   1.95   1.5e-7
    clipped              bf16        0.65   0.95   1.97   1.1e-7
    groups, zero_grads   bf16        0.66   0.95   1.95   1.5e-7
The total comes out of one atomic per chunk, so its last bit (and the figures above in their last digit) moves from launch
to launch; the bounds do not depend on it because every reference step uses the total the GPU produced.
"""

import numpy as np
import pytest
import torch

from helpers import (ADAMW_C, ADAMW_COUNTERS, ADAMW_E, ADAMW_HP, ADAMW_HP2, ADAMW_TENSORS, MT_CHUNK, adamw_bounds,
                     adamw_grads, adamw_hp, adamw_params, adamw_scenario_grads, adamw_scenarios, adamw_step_ref, sumsq64)

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
BF = torch.bfloat16
SCEN = adamw_scenarios()
NAMES = [t[0] for t in ADAMW_TENSORS]
NUMEL = {t[0]: int(np.prod(t[1])) for t in ADAMW_TENSORS}
NCHUNKS = sum((n + MT_CHUNK - 1) // MT_CHUNK for n in NUMEL.values())
NORM_DEPTH = 1 + MT_CHUNK // 1024 + 6 + 16 + NCHUNKS
NORM_REL = (1.0 + 2.0 ** -24) ** NORM_DEPTH - 1.0
assert NCHUNKS == 13 and NORM_DEPTH == 100 and NORM_REL <= 1e-5
assert ADAMW_C * max(ADAMW_E.values()) <= 64


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    from fddm_hip import runtime as rt
    rt.clear_cache()


def ops():
    from fddm_hip import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ optimizer set-up
def offset_view(n, fill=None):
    """A 1-D fp32 device tensor of n elements at element offset 1 of a larger buffer (4 bytes past a 16-B boundary)."""
    buf = torch.zeros(n + 7, device=dev)
    v = buf[1:1 + n]
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    if fill is not None:
        v.copy_(fill)
    return v


class Rig:
    """The ten parameters on the device, persistent gradient buffers (the unaligned tensor's is an offset view too) and
    a FusedAdamW over them: one group with FusedAdamW's defaults, or the two groups of the groups scenario, or the
    hyperparameters given."""

    def __init__(self, groups=False, arena=False, **hp):
        from fddm_hip.optim import FusedAdamW
        init = adamw_params()
        self.ps, self.gb = {}, {}
        for name, shape, _, _, unaligned, _ in ADAMW_TENSORS:
            if unaligned:
                self.ps[name] = torch.nn.Parameter(offset_view(NUMEL[name], init[name]))
                self.gb[name] = offset_view(NUMEL[name])
            else:
                self.ps[name] = torch.nn.Parameter(init[name].to(dev))
                self.gb[name] = torch.zeros(*shape, device=dev)
                assert self.ps[name].data_ptr() % 16 == 0 and self.gb[name].data_ptr() % 16 == 0
        if groups:
            pg = []
            for gi, h in enumerate((ADAMW_HP, ADAMW_HP2)):
                pg.append(dict(params=[self.ps[t[0]] for t in ADAMW_TENSORS if t[5] == gi], lr=h["lr"],
                               weight_decay=h["wd"], betas=(h["b1"], h["b2"]), eps=h["eps"]))
            self.opt = FusedAdamW(pg)
        elif hp:
            self.opt = FusedAdamW(list(self.ps.values()), **hp)
        else:
            self.opt = FusedAdamW(list(self.ps.values()))
            d = self.opt.defaults
            assert (d["lr"], d["weight_decay"], d["betas"], d["eps"]) == (2e-4, 0.01, (0.9, 0.999), 1e-8)
        self.arena = None
        if arena:
            self.arena = self.opt.use_grad_arena(list(self.ps.values()))
            self.opt.zero_grad()
            self.gb = {n: p.grad for n, p in self.ps.items()}

    def set_grads(self, G):
        """Bind every parameter to its gradient buffer holding G[name]; a name missing from G gets grad None."""
        for n, p in self.ps.items():
            if n in G:
                self.gb[n].copy_(G[n].to(dev).view_as(self.gb[n]))
                p.grad = self.gb[n]
            else:
                p.grad = None

    def state(self, n):
        """(p, m, v, counter) of tensor n on the host; zeros before its first step."""
        p = self.ps[n]
        st = self.opt.state.get(p)
        if not st:
            z = torch.zeros(p.shape)
            return p.detach().cpu(), z, z.clone(), 0.0
        return p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), float(st["step"])

    def snapshot(self):
        return {n: tuple(x.clone() if torch.is_tensor(x) else x for x in self.state(n)) for n in NAMES}


def check_copies(rig, what):
    """Every 2-D tensor's cached bf16 copy is the bf16 rounding of its parameter, bit for bit; 1-D tensors have none."""
    from fddm_hip import runtime as rt
    for n, p in rig.ps.items():
        e = rt.bf16_entry(p)
        if p.dim() < 2:
            assert e is None, (what, n)
            continue
        assert e is not None and e.dtype == BF and e.shape == p.shape, (what, n)
        want = p.detach().to(BF)
        bad = (e.view(torch.int16) != want.view(torch.int16)).flatten().nonzero().flatten()
        assert bad.numel() == 0, f"{what} {n}: {bad.numel()} bf16 copy elements differ, first at {bad[:4].tolist()}"


def unit_max(err, scale):
    """max err / scale over the elements with a nonzero scale (the others are covered by the bound itself: 0)."""
    nz = scale > 0
    return float((err[nz] / scale[nz]).max()) if nz.any() else 0.0


def run_scenario(scen, precision="fp32", zero_grads=False):
    """The scenario's four steps with every assertion of the module docstring; returns the measured maxima."""
    from fddm_hip import runtime as rt
    cfg = SCEN[scen]
    u24 = 2.0 ** -24
    mx = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
    with rt.use_precision(precision):
        rig = Rig(groups=cfg["groups"])
        before = rig.snapshot()
        for k, c0 in enumerate(ADAMW_COUNTERS):
            G = adamw_scenario_grads(cfg, k)
            rig.set_grads(G)
            if c0 == 999.0:
                for p in rig.ps.values():
                    rig.opt.state[p]["step"].fill_(999.0)
                before = {n: b[:3] + (999.0,) for n, b in before.items()}
            norm = rig.opt.clip_and_step(max_norm=cfg["max_norm"], grad_scale=cfg["grad_scale"], zero_grads=zero_grads)
            total = float(rig.opt.last_total_sq)
            assert int(rig.opt.skipped_steps()[0]) == 0
            t64 = sumsq64(G)
            mx["norm"] = max(mx["norm"], abs(total - t64) / t64)
            assert abs(total - t64) <= NORM_REL * t64, (scen, k, total, t64)
            # the returned norm is grad_scale x the device's own fp32 sqrt of that total, exactly (0.125 x is exact), and
            # that sqrt within one fp32 ulp of the float64 root (torch's device sqrt is not correctly rounded: at
            # total = 99791.98 it returns the neighbour of the correctly rounded 315.89865)
            root = float(rig.opt.last_total_sq.sqrt())
            assert float(norm) == cfg["grad_scale"] * root, (scen, k, float(norm), root)
            assert abs(root - total ** 0.5) <= 2.0 ** -23 * total ** 0.5, (scen, k, root, total)
            after = rig.snapshot()
            for n in NAMES:
                p0, m0, v0, cnt0 = before[n]
                p1, m1, v1, cnt1 = after[n]
                if n not in G:      # grad None: the tensor is not in the step at all and its counter lags
                    assert torch.equal(p1, p0) and torch.equal(m1, m0) and torch.equal(v1, v0) and cnt1 == cnt0, (scen, k, n)
                    continue
                assert cnt1 == cnt0 + 1.0, (scen, k, n, cnt0, cnt1)
                kw = dict(adamw_hp(n, cfg["groups"]), max_norm=cfg["max_norm"], grad_scale=cfg["grad_scale"])
                pr, mr, vr, sc = adamw_step_ref(p0, G[n], m0, v0, cnt0, total, **kw)
                if scen.endswith("not_clipped"):
                    assert sc.coef == cfg["grad_scale"]
                elif cfg["max_norm"] is not None:
                    assert sc.coef < 0.1 * cfg["grad_scale"]
                bp, bm, bv = adamw_bounds(sc)
                ep, em, ev = (p1.double() - pr).abs(), (m1.double() - mr).abs(), (v1.double() - vr).abs()
                mx["p"] = max(mx["p"], unit_max(ep, u24 * (ADAMW_E["P"] * sc.s_p + ADAMW_E["U"] * sc.s_u)))
                mx["m"] = max(mx["m"], unit_max(em, u24 * sc.s_m))
                mx["v"] = max(mx["v"], unit_max(ev, u24 * sc.s_v))
                for what, e, b in (("p", ep, bp), ("m", em, bm), ("v", ev, bv)):
                    bad = ~(e <= b)
                    assert not bad.any(), (f"{scen} step {k} {n}.{what}: {int(bad.sum())} of {e.numel()} elements out of "
                                           f"bound, first at {bad.flatten().nonzero().flatten()[:4].tolist()}, worst "
                                           f"{unit_max(e, b) * ADAMW_C:.2f} (bound {ADAMW_C})")
            if cfg["groups"]:
                lag = {n: sum(1 for j in range(k + 1) if n not in adamw_scenario_grads(cfg, j)) for n in NAMES}
                for n in NAMES:
                    assert after[n][3] == (1000.0 if c0 == 999.0 else k + 1.0 - lag[n]), (scen, k, n, after[n][3])
            if precision == "bf16":
                check_copies(rig, f"{scen} step {k}")
            if zero_grads:
                for n in G:
                    assert float(rig.gb[n].abs().max()) == 0.0, (scen, k, n)
            before = after
    print(f"{scen} [{precision}]: p {mx['p']:.2f}  m {mx['m']:.2f}  v {mx['v']:.2f}  norm {mx['norm']:.2e}")
    return mx


# ------------------------------------------------------------------------------------------ AdamW per element
@pytest.mark.parametrize("scen", list(SCEN))
def test_adamw_steps_match_float64(scen):
    run_scenario(scen)


def test_adamw_bf16_copies_follow_every_step():
    """In bf16 mode the same pass writes each 2-D weight's bf16 copy: the packed converts of the vector loop, the scalar
    tail of (257, 255) and the second and third chunk of (3, 43691); the numerics are checked again on the way."""
    run_scenario("clipped", precision="bf16")
    run_scenario("groups", precision="bf16", zero_grads=True)


def tie_patterns(n, rot, seed=5):
    """n fp32 values whose low 16 bits sit at the bf16 rounding edges, by index i: kind (i + rot) % 8 = sign * 4 + one of
    0x7FFF (just below the tie), 0x8000 under an even bit (tie, stays), 0x8000 under an odd bit (tie, goes up), 0x8001
    (just above). Exponent fields 1 .. 254 (no denormal, inf or NaN; every fifth element 254, up to 3.37e38), mantissas
    kept below the value that would round to inf. Returns (values, expected bf16 bit patterns as int64)."""
    gen = g(seed)
    exp = torch.randint(1, 255, (n,), generator=gen)
    exp[::5] = 254
    hi7 = torch.randint(0, 128, (n,), generator=gen)
    hi7 = torch.where(exp == 254, hi7.clamp(max=125), hi7)
    kind = (torch.arange(n) + rot) % 8
    low = torch.tensor([0x7FFF, 0x8000, 0x8000, 0x8001])[kind % 4]
    hi7 = torch.where(kind % 4 == 1, hi7 & ~1, hi7)
    hi7 = torch.where(kind % 4 == 2, hi7 | 1, hi7)
    bits = ((kind // 4) << 31) | (exp << 23) | (hi7 << 16) | low
    x = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())
    want = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16          # round to nearest even on the integer
    up = torch.tensor([0, 0, 1, 1])[kind % 4]
    assert torch.equal(want, (bits >> 16) + up) and torch.isfinite(x).all() and (x.abs() >= 2.0 ** -126).all()
    assert (want & 0x7FFF < 0x7F80).all()                       # finite bf16
    return x, want


def bf16_bits(t):
    return t.view(torch.int16).cpu().long() & 0xFFFF


def test_adamw_bf16_copy_rounding_at_the_ties():
    """lr = 0, wd = 0 and zero gradients leave p' == p bit for bit, so the copy is bf16(p) of chosen bit patterns; eight
    launches rotate the patterns, so every element — both lanes of each packed convert, the scalar tail of (257, 255),
    the one-element last chunk of (3, 43691) — sees every pattern."""
    from fddm_hip import runtime as rt
    from fddm_hip.optim import FusedAdamW
    shapes = [(257, 255), (3, 43691), (5, 3)]
    with rt.use_precision("bf16"):
        ps = [torch.nn.Parameter(torch.ones(*s, device=dev)) for s in shapes]
        opt = FusedAdamW(ps, lr=0.0, weight_decay=0.0)
        for p in ps:
            p.grad = torch.zeros_like(p)
        for rot in range(8):
            exp = []
            for i, p in enumerate(ps):
                x, want = tie_patterns(p.numel(), rot, seed=5 + i)
                with torch.no_grad():
                    p.copy_(x.view_as(p).to(dev))
                exp.append((x, want))
            opt.clip_and_step(max_norm=5.0)
            for p, (x, want) in zip(ps, exp):
                assert torch.equal(p.detach().cpu().view(torch.int32), x.view_as(p).view(torch.int32)), "p changed"
                got = bf16_bits(rt.bf16_entry(p)).flatten()
                bad = (got != want).nonzero().flatten()
                assert bad.numel() == 0, (rot, tuple(p.shape), bad[:4].tolist(), [hex(int(got[b])) for b in bad[:4]])
                assert torch.equal(got, bf16_bits(p.detach().to(BF)).flatten())


@pytest.mark.parametrize("arena", [True, False])
@pytest.mark.parametrize("finite", [True, False])
def test_adamw_zero_grads_is_bit_identical_and_zeroes_everything(finite, arena):
    """clip_and_step(zero_grads=True) gives bit-identical parameters, moments, counters and bf16 copies and leaves every
    gradient element zero — tails, last chunks and the unaligned tensor's scalar path included — for an applied step and
    for a step the non-finite guard skips. arena: the gradients live in a GradArena (every slot aligned); otherwise in
    their own buffers (the unaligned tensor's gradient at element offset 1). The gradients are drawn from +-{0.5, 1, 2}:
    every partial sum of their squares is a multiple of 0.25 below 2^24 x 0.25, so the total — and with it the clip
    coefficient — is the same bit pattern whatever order the chunks' atomics land in (with generic gradients the last bit
    of the total, hence of every parameter, differs from launch to launch)."""
    from fddm_hip import runtime as rt
    out = []
    vals = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
    with rt.use_precision("bf16"):
        for zg in (False, True):
            rig = Rig(arena=arena)
            for k in range(2):          # the second step starts from nonzero moments; the NaN goes into that one
                G = {n: vals[torch.randint(0, 6, (NUMEL[n],), generator=g(60 + 10 * k + i))].view(ADAMW_TENSORS[i][1])
                     for i, n in enumerate(NAMES)}
                exact = sumsq64(G)
                assert exact < 2.0 ** 22
                if k == 1 and not finite:
                    G["c"][2, 43690] = float("nan")
                if arena:
                    rig.opt.zero_grad()
                    for n in NAMES:
                        rig.ps[n].grad.copy_(G[n].to(dev))
                else:
                    rig.set_grads(G)
                rig.opt.clip_and_step(max_norm=5.0, zero_grads=zg)
                assert float(rig.opt.last_total_sq) == exact or (k == 1 and not finite)
                if zg:
                    for n in NAMES:
                        assert float(rig.ps[n].grad.abs().max()) == 0.0, (k, n)
                    if arena:
                        assert rig.arena.clean and float(rig.arena.flat.abs().max()) == 0.0
            assert int(rig.opt.skipped_steps()[0]) == (0 if finite else 1)
            check_copies(rig, f"zero_grads={zg}")
            snap = rig.snapshot()
            assert all(s[3] == (2.0 if finite else 1.0) for s in snap.values())
            out.append(snap)
    for n in NAMES:
        for a, b in zip(out[0][n][:3], out[1][n][:3]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n


# ------------------------------------------------------------------------------------------ gradient norm and guard
def positions(n):
    """Element indices at the edges of the float4 loop, its tail and the unrolled loops' strides, where they exist."""
    return sorted(k for k in {0, 3, 4 * (n // 4) - 1, 4 * (n // 4), n - 1, 32767, 32768, 65535, 65536} if 0 <= k < n)


def test_norm_counts_every_element_exactly_once():
    """All-ones gradients: every partial sum is an integer below 2^24, so the total is sum(numel) exactly. A single 1.0
    at one position (zeros elsewhere): the total is 1.0 exactly, for every edge position of every tensor."""
    from fddm_hip import runtime as rt
    with rt.use_precision("fp32"):
        rig = Rig(lr=0.0, weight_decay=0.0)
        rig.set_grads({n: torch.ones(NUMEL[n]) for n in NAMES})
        norm = rig.opt.clip_and_step(max_norm=5.0)
        assert float(rig.opt.last_total_sq) == float(sum(NUMEL.values())) == 475408.0
        assert abs(float(norm) - 475408.0 ** 0.5) <= 2.0 ** -23 * 475408.0 ** 0.5
        rig.set_grads({n: torch.zeros(NUMEL[n]) for n in NAMES})
        rig.opt.clip_and_step(max_norm=5.0)
        assert float(rig.opt.last_total_sq) == 0.0
        seen = 0
        for n in NAMES:
            flat = rig.gb[n].view(-1)
            for k in positions(NUMEL[n]):
                flat[k] = 1.0
                rig.opt.clip_and_step(max_norm=5.0, return_norm=False)
                assert float(rig.opt.last_total_sq) == 1.0, (n, k, float(rig.opt.last_total_sq))
                flat[k] = 0.0
                seen += 1
        assert seen == 58


def test_nonfinite_guard_sees_every_position():
    """A NaN at any edge position of any tensor skips exactly one step and changes no parameter, moment or counter."""
    from fddm_hip import runtime as rt
    with rt.use_precision("fp32"):
        rig = Rig()
        rig.set_grads(adamw_grads(0, 10.0))
        rig.opt.clip_and_step(max_norm=5.0)             # one applied step: nonzero moments and counters
        rig.set_grads(adamw_grads(1, 10.0))
        ref = rig.snapshot()
        skipped = 0
        for n in NAMES:
            flat = rig.gb[n].view(-1)
            for k in positions(NUMEL[n]):
                old = flat[k].clone()
                flat[k] = float("nan")
                rig.opt.clip_and_step(max_norm=None if skipped % 2 else 5.0, return_norm=False)
                skipped += 1
                assert int(rig.opt.skipped_steps()[0]) == skipped, (n, k)
                flat[k] = old
        now = rig.snapshot()
        for n in NAMES:
            for a, b in zip(ref[n][:3], now[n][:3]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
            assert now[n][3] == ref[n][3] == 1.0
        rig.opt.clip_and_step(max_norm=5.0)             # and the next finite step is applied
        assert int(rig.opt.skipped_steps()[0]) == skipped
        assert all(s[3] == 2.0 for s in rig.snapshot().values())


# ------------------------------------------------------------------------------------------ ops.cast
CAST_N = [1, 3, 4, 5, 1023, 1024, 1025, 65537]


def cast_input(n):
    """Tie patterns on two of every three elements, randn on the third."""
    x, want = tie_patterns(n, rot=n % 8, seed=40)
    r = torch.randn(n, generator=g(41 + n))
    third = torch.arange(n) % 3 == 2
    x = torch.where(third, r, x)
    rb = r.view(torch.int32).long() & 0xFFFFFFFF
    want = torch.where(third, (rb + 0x7FFF + ((rb >> 16) & 1)) >> 16, want)
    return x, want


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", CAST_N)
def test_cast_f32_to_bf16_bit_exact(n, offset):
    """Bit-exact round to nearest even, nothing written past the output; offset 1: the input is a view one element
    into a buffer (not 16-B aligned), which takes the kernel's scalar loop."""
    x, want = cast_input(n)
    xd = offset_view(n, x.to(dev)) if offset else x.to(dev)
    assert xd.data_ptr() % 16 == 4 * offset
    buf = torch.full((n + 2,), -1.5, dtype=BF, device=dev)
    y = ops().cast(xd, BF, out=buf[:n])
    assert y.data_ptr() == buf.data_ptr()
    got = bf16_bits(buf)
    bad = (got[:n] != want).nonzero().flatten()
    assert bad.numel() == 0, (bad[:4].tolist(), [hex(int(got[b])) for b in bad[:4]])
    assert torch.equal(got[:n], bf16_bits(xd.to(BF)))
    assert got[n:].tolist() == [0xBFC0, 0xBFC0], "wrote past the output"
    z = ops().cast(xd, BF)
    assert torch.equal(bf16_bits(z), want)


@pytest.mark.parametrize("n", CAST_N)
def test_cast_bf16_to_f32_exact(n):
    x, _ = cast_input(n)
    xb = x.to(BF).to(dev)
    buf = torch.full((n + 2,), -1.5, device=dev)
    ops().cast(xb, torch.float32, out=buf[:n])
    assert torch.equal(buf[:n].view(torch.int32), xb.float().view(torch.int32))
    assert buf[n:].tolist() == [-1.5, -1.5], "wrote past the output"


# ------------------------------------------------------------------------------------------ ops.colsum
def colsum_input(M, N, dtype, layout):
    """X [M, N] on the device in one of the layouts: plain (contiguous), ld (row stride the next multiple of 8 above N:
    16-B aligned rows, the vector branch), ldodd (an odd row stride: never aligned), off1 (contiguous at element offset
    1 of a buffer: misaligned base)."""
    x = torch.randn(M, N, generator=g(100 * M + N)).to(dtype)
    if layout in ("plain", "acc"):
        xd = x.to(dev)
    elif layout in ("ld", "ldodd"):
        ld = (N // 8 + 1) * 8 + (layout == "ldodd")
        big = torch.full((M, ld), 1000.0, dtype=dtype, device=dev)     # the padding must not be summed
        xd = big[:, :N]
        xd.copy_(x.to(dev))
        assert xd.stride(0) == ld > N
    else:
        buf = torch.zeros(M * N + 9, dtype=dtype, device=dev)
        xd = buf[1:1 + M * N].view(M, N)
        xd.copy_(x.to(dev))
        assert xd.data_ptr() % 16 == x.element_size()
    return x, xd


@pytest.mark.parametrize("layout", ["plain", "ld", "ldodd", "off1", "acc"])
@pytest.mark.parametrize("M,N", [(1, 8), (7, 13), (300, 136), (1000, 1001)])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_colsum_matches_float64(dtype, M, N, layout):
    """Per column within rows x 2^-24 x colsum(|x|) (+ |out| when accumulating) of the float64 sum: a thread adds its
    slab's rows one by one and the slabs meet in atomics, at most rows - 1 roundings on the way to a column's sum (one
    more per slab onto a nonzero out, which its |out| term carries); bf16 inputs convert exactly."""
    x, xd = colsum_input(M, N, dtype, layout)
    ref = x.double().sum(0)
    scale = x.double().abs().sum(0)
    if layout == "acc":
        out0 = torch.randn(N, generator=g(7))
        out = out0.to(dev)
        got = ops().colsum(xd, out=out, accumulate=True)
        assert got.data_ptr() == out.data_ptr()
        ref = ref + out0.double()
        scale = scale + out0.double().abs()
    else:
        got = ops().colsum(xd)
        out = torch.full((N + 2,), 3.0, device=dev)                    # out given, not accumulating: zeroed first
        ops().colsum(xd, out=out[:N])
        assert torch.equal(out[:N], got) or M > 8                      # several slabs: the atomics' order may differ
        assert out[N:].tolist() == [3.0, 3.0], "wrote past the output"
    err = (got.cpu().double() - ref).abs()
    tol = M * 2.0 ** -24 * scale
    assert (err <= tol).all(), (float((err / tol.clamp(min=1e-300)).max()), int((err > tol).sum()))
