"""The jumpy-sampler step (jump_kernel, csrc/jumpy.hip, ops.jump) per element against float64: every token id the
system decodes comes out of this kernel.

Cases (helpers.jump_case): V = 2, 3, 63, 64, 65, 255, 256, 257, 260 (the float4 path with a partial last pass) and 2003
(scalar, 32 passes) x four layouts (contiguous; ldz = V + 4 and V + 1 with +1e30 in the padding columns, so that an
over-read changes the argmax; a view one float past a 16-byte boundary) x N = 1, 5, 64 x L = 1, 5, 16 (L = 5: a block's
four rows belong to two batch elements). coef differs per batch element, one element has t - delta = 0 (a_tg = 1, b_tg =
0; abar = 1). x_t takes 0, V - 1, the argmax, a non-argmax, -1 and V + 5 (which must act as 0 and V - 1). Rows: random;
the maximum twice in one float4, in one lane on two passes (k, k + 64 and k, k + 256) and in two lanes; the same for the
runner-up with x_t on the maximum; constant; -inf in a third of the entries, with and without x_t; a logit spread of
40; and rows whose logit at x_t was bisected until the exact margin sits at +-4 bounds. Both outputs are slices of
sentinel-filled int64 buffers whose other elements must keep their bits. Every row of every case is asserted.

Greedy (exact and fast): x0hat is the reference's first argmax bit for bit, tied rows included; fast x_next = x0hat;
exact x_next is the reference's choice where |margin| exceeds the row's bound
    (C_g + K_exp) u S W + V 2^-126 + 2^-48,       u = 2^-24, S and W in helpers' section
and one of {x_t, o} otherwise; the constructed rows lie at 4 bounds and so must come out on their side.
Sample (exact and fast, temperature 0.7, 1.0, 2.0, V <= 260): the id belongs to {k : score_k >= max score - bound_row},
    bound_row = 2 max_k (C_s + K_dev) u U_k
with score = log(max(P_k, 1e-12)) / temp + g_k in float64, g from the RNG contract's u (oracle.jump_uniform) at index
row V + k. tests/test_cpu_jump_ref.py shows from the reference alone that at most 1 % of rows lie within their greedy
bound (none does), that the candidate set has one member in at least 98 % of the sampled rows (in all of them), and
that a transposed or mis-strided RNG index leaves it.
C = 8 E, E the fp32 emulation's largest excess on the CPU: C_g = 8.8 (E 1.014), C_s = 6.0 (E 0.711); hard cap 64.
K: the device's __expf, __logf and Gumbel term against float64 on one MI355X grid of their own (helpers.JUMP_K).

The extreme draws: seed 2678, stream 7, N = 64, V = 256 gives (row 5, class 144) the draw with every bit set (3227 and
3651: (49, 149), (41, 176)); that class is under the clamp and class 3 has nearly all the mass. Seed 200 gives (28, 109)
the all-zero draw. Rows without an orderable entry (all -inf, all NaN): x0hat = 0 for the all -inf row, every id in [0,
V); these tests pass the ids to nothing else.

K, measured / stored: __expf 1.204 / 1.5, __logf 2.966 / 3.5, the Gumbel term over all 2^23 draws 2.977 / 3.3.

Measured on an MI355X (the JUMPNEED lines this file prints; a greedy row uses |margin| / bound of its bound only when
the kernel decides against the reference, a sampled row (best score - score of the kernel's id) / bound_row):
    greedy 0.000   sample 0.000   sample peaked 0.000   sample extreme 0.000
that is, the kernel took the reference's decision in every greedy row and drew the reference's class in every sampled
row. On the parent commit's kernel exactly the three all-ones draws (both modes: the clamped class wins with a Gumbel
term of +inf) and the rows without an orderable entry (id 2147483647) fail, 26 of the 111 tests.
"""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
EXACT, FAST, SAMPLE = 0, H.JUMP_FAST, H.JUMP_SAMPLE
NEED = {}
GUARD = 8
assert all(v <= 64.0 for v in H.JUMP_C.values())


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import fddm_hip  # noqa: F401  (loads libfddm_hip.so, raises if absent)
    assert torch.cuda.is_available()
    yield
    for k in sorted(NEED):
        print(f"\nJUMPNEED {k:<14} share {NEED[k]:5.3f}", end="")
    print()


def _ops():
    from fddm_hip import ops
    return ops


def _place(z, layout):
    """The logits as the kernel sees them under `layout`, everything around them +1e30."""
    N, V = z.shape
    zt = torch.from_numpy(np.array(z))
    if layout == "off1":
        buf = torch.full((N * V + 8,), H.JUMP_PAD, device=dev)
        view = buf[1:1 + N * V].view(N, V)
        view.copy_(zt)
        assert view.data_ptr() % 16 == 4
    else:
        buf = torch.full((N, H.jump_ldz(V, layout)), H.JUMP_PAD, device=dev)
        view = buf[:, :V]
        view.copy_(zt)
        assert view.data_ptr() % 16 == 0
    assert view.stride(0) == H.jump_ldz(V, layout) and view.stride(1) == 1
    return view


def _jump(c, layout, mode, temp=1.0, seed=0, z=None):
    """ops.jump on case c: (x_next, x0hat) as numpy, both written into slices of sentinel-filled buffers that must keep
    every other element."""
    ops = _ops()
    N = c["N"]
    z = _place(c["logits"], layout) if z is None else z
    xt = torch.from_numpy(np.array(c["xt"])).to(dev)
    coef = torch.from_numpy(np.array(c["coef_fast" if mode & FAST else "coef"])).to(dev)
    bufs = [torch.full((N + 2 * GUARD,), H.JUMP_SENTINEL, dtype=torch.int64, device=dev) for _ in range(2)]
    nx, x0 = ops.jump(z, xt, coef, c["L"], mode=mode, temperature=temp, seed=seed, rng_stream=H.JUMP_STREAM,
                      x_next=bufs[0][GUARD:GUARD + N], x0hat=bufs[1][GUARD:GUARD + N])
    torch.cuda.synchronize()
    for b in bufs:
        b = b.cpu()
        assert (b[:GUARD] == H.JUMP_SENTINEL).all() and (b[GUARD + N:] == H.JUMP_SENTINEL).all(), "wrote outside its slice"
    return nx.cpu().numpy(), x0.cpu().numpy()


def _need(row, share):
    NEED[row] = max(NEED.get(row, 0.0), float(share))


def _check_greedy(c, ref, nx, x0, mode, what):
    V = c["V"]
    assert np.array_equal(x0, ref.am), f"{what}: x0hat rows {np.nonzero(x0 != ref.am)[0][:8]}"
    if mode & FAST:
        assert np.array_equal(nx, x0), what
        return
    b = H.jump_greedy_bound(ref, V)
    assert ((nx == ref.x) | (nx == ref.o)).all(), f"{what}: x_next is neither x_t nor o"
    off = nx != ref.choice
    k = np.abs(ref.margin) / b
    _need("greedy", k[off].max() if off.any() else 0.0)
    bad = off & (k > 1.0)
    assert not bad.any(), (f"{what}: rows {np.nonzero(bad)[0][:8]} decided against the reference at "
                           f"{k[bad][:8]} bounds (kinds {[c['kinds'][r] for r in np.nonzero(bad)[0][:8]]})")
    built = c["built"] != 0
    assert np.array_equal(nx[built], ref.choice[built]), f"{what}: a row constructed at 4 bounds came out on the other side"


def _check_sample(ref, nx, what, row="sample"):
    N, V = ref.score.shape
    assert ((nx >= 0) & (nx < V)).all(), what
    b = H.jump_sample_bound(ref)
    short = ref.score.max(1) - ref.score[np.arange(N), nx]
    _need(row, (short / b).max())
    bad = short > b
    assert not bad.any(), (f"{what}: rows {np.nonzero(bad)[0][:8]} drew {nx[bad][:8]}, whose score lies {short[bad][:8]} "
                           f"under the best (bound {b[bad][:8]}; the reference draws {ref.score.argmax(1)[bad][:8]})")


@pytest.mark.parametrize("layout", H.JUMP_LAYOUTS)
@pytest.mark.parametrize("V", H.JUMP_V)
def test_greedy(V, layout):
    for N, L in H.JUMP_NL:
        c = H.jump_case(V, N, L)
        z = _place(c["logits"], layout)
        for mode in (EXACT, FAST):
            ref, _ = H.jump_case_ref(V, N, L, mode)
            nx, x0 = _jump(c, layout, mode, z=z)
            _check_greedy(c, ref, nx, x0, mode, f"V {V} {layout} N {N} L {L} mode {mode}")


def test_greedy_without_x0hat():
    """x0hat = NULL through the C entry point: x_next alone is written."""
    ops = _ops()
    V, N, L = 260, 64, 5
    c = H.jump_case(V, N, L)
    ref, _ = H.jump_case_ref(V, N, L, EXACT)
    z = _place(c["logits"], "contig")
    xt, coef = torch.from_numpy(np.array(c["xt"])).to(dev), torch.from_numpy(np.array(c["coef"])).to(dev)
    buf = torch.full((N + 2 * GUARD,), H.JUMP_SENTINEL, dtype=torch.int64, device=dev)
    nx = buf[GUARD:GUARD + N]
    ops.call("fddm_jump", ops.ptr(z), z.stride(0), ops.ptr(xt), ops.ptr(coef), ops.ptr(nx), None, N, L, V, EXACT, 1.0, 0, 0,
             ops.stream())
    torch.cuda.synchronize()
    b = buf.cpu()
    assert (b[:GUARD] == H.JUMP_SENTINEL).all() and (b[GUARD + N:] == H.JUMP_SENTINEL).all()
    _check_greedy(c, ref, nx.cpu().numpy(), ref.am, EXACT, "x0hat = NULL")


@pytest.mark.parametrize("layout", H.JUMP_LAYOUTS)
@pytest.mark.parametrize("V", H.JUMP_SAMPLE_V)
def test_sample(V, layout):
    for N, L in H.JUMP_SAMPLE_NL:
        c = H.jump_case(V, N, L)
        z = _place(c["logits"], layout)
        for mode in (SAMPLE, SAMPLE | FAST):
            for temp in H.JUMP_TEMPS:
                ref, seed = H.jump_case_ref(V, N, L, mode, temp)
                nx, x0 = _jump(c, layout, mode, temp, seed, z=z)
                what = f"V {V} {layout} N {N} L {L} mode {mode} temp {temp}"
                assert np.array_equal(x0, ref.am), what
                _check_sample(ref, nx, what)


@pytest.mark.parametrize("temp", H.JUMP_TEMPS)
@pytest.mark.parametrize("mode", [SAMPLE, SAMPLE | FAST])
def test_sample_peaked(mode, temp):
    """Every row with a logit spread of 40 and b_tg = 0 / abar = 1: most P sit on the 1e-12 clamp."""
    c = H.jump_peaked_case()
    ref = H.jump_ref64(c["logits"], c["xt"], c["coef_fast" if mode & FAST else "coef"], c["L"], mode, temp, c["seed"],
                       H.JUMP_STREAM)
    nx, x0 = _jump(c, "contig", mode, temp, c["seed"])
    assert np.array_equal(x0, ref.am)
    _check_sample(ref, nx, f"peaked mode {mode} temp {temp}", "sample peaked")


@pytest.mark.parametrize("mode", [SAMPLE, SAMPLE | FAST])
@pytest.mark.parametrize("which", [0, 1, 2, "zero"])
def test_extreme_draw(which, mode):
    """The draw with every bit set must not hand its row to a class under the clamp (u = 1 gives a Gumbel term of +inf);
    the draw with every bit clear has a finite Gumbel term, -2.81, and its class, with nearly all the mass, still wins."""
    c = H.jump_extreme_case(which)
    ref = H.jump_ref64(c["logits"], c["xt"], c["coef_fast" if mode & FAST else "coef"], c["L"], mode, 1.0, c["seed"],
                       H.JUMP_STREAM)
    nx, x0 = _jump(c, "contig", mode, 1.0, c["seed"])
    assert np.array_equal(x0, ref.am)
    want = c["k"] if which == "zero" else 3
    assert ref.score[c["row"]].argmax() == want
    assert nx[c["row"]] == want, f"row {c['row']} drew class {nx[c['row']]}, the reference {want} (extreme class {c['k']})"
    _check_sample(ref, nx, f"extreme {which} mode {mode}", "sample extreme")


@pytest.mark.parametrize("mode", [EXACT, FAST, SAMPLE, SAMPLE | FAST])
@pytest.mark.parametrize("V,layout", [(3, "contig"), (64, "contig"), (64, "pad1"), (260, "pad4"), (257, "off1")])
def test_no_orderable_entry(V, layout, mode):
    """Row 1 all -inf, row 3 all NaN, the others ordinary (N = 5): x0hat = 0 for the all -inf row as torch.argmax gives,
    every id written lies in [0, V), the ordinary rows are the reference's. The ids go nowhere else."""
    N, L = 5, 5
    base = H.jump_case(V, N, L)
    z = np.array(base["logits"])
    z[1] = -np.inf
    z[3] = np.nan
    c = dict(base, logits=z)
    seed = 77
    ref = H.jump_ref64(z, c["xt"], c["coef_fast" if mode & FAST else "coef"], L, mode, 1.0, seed, H.JUMP_STREAM)
    assert list(ref.ok) == [True, False, True, False, True] and ref.am[1] == 0 and ref.am[3] == 0
    nx, x0 = _jump(c, layout, mode, 1.0, seed)
    what = f"V {V} {layout} mode {mode}: x_next {nx}, x0hat {x0}"
    assert ((nx >= 0) & (nx < V)).all() and ((x0 >= 0) & (x0 < V)).all(), what
    assert x0[1] == 0, what
    ok = ref.ok
    assert np.array_equal(x0[ok], ref.am[ok]), what
    if mode & SAMPLE:
        live = H.Ref(score=ref.score[ok], unit=ref.unit[ok])
        _check_sample(live, nx[ok], what, "sample")
    else:
        live = dict(c, kinds=[k for k, o in zip(c["kinds"], ok) if o], built=c["built"][ok])
        sub = H.Ref(**{k: v[ok] for k, v in ref.__dict__.items()})
        _check_greedy(live, sub, nx[ok], x0[ok], mode, what)
