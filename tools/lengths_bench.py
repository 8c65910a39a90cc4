"""Length-bounded attention (fddm_attn_fwd_kx / _bwd_kx / fddm_attn_fwd_relgate_x_kx) against the launches it stands
next to: HIP-event timing, bf16, the arms of one table alternating round by round inside one process (median and
min-max over the rounds; the spread between rounds is the noise a difference has to exceed).
  python tools/lengths_bench.py [attn] [wavlm] [step]     (default: attn wavlm)
attn   C2 cross-attention (B 32, H 8, Lq 256, S 499, dropout 0.1, keep bits written ahead), forward and backward:
       the cost of the bound when nothing can be skipped (all-true mask + extent vs the unmasked launch on forced
       fwd7 and on the default fwd8), and the gain at extents of S/4 and S/2 (kx entry vs the plain key_keep entry on
       forced fwd7 and on the default dispatch).
wavlm  WavLM's gated relative-position attention at the 20 s window (B 16, H 12, S 999) with extents of 250: the
       masked + bounded entry, the general entry with key_keep alone, and the unmasked relgate_x launch.
step   train_one_epoch on synthetic 20 s batches, B 16, C2 decoder, lengths U{2 s .. 10 s}: ms / step with the lengths
       passed (masked encoder, c_mask, eager encoder) and without (graph-replayed encoder, no mask)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fddm-asr_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from fddm_hip import ops  # noqa: E402

dev = torch.device("cuda:0")
bf = torch.bfloat16


def time_arms(arms, iters=30, rounds=7):
    """arms: {name: (family, fn)} -> {name: (median us, min us, max us)}; the arms alternate within every round."""
    for fam, fn in arms.values():
        old = ops.attn_force_kernels(fam)
        for _ in range(3):
            fn()
        ops.attn_force_kernels(old)
    torch.cuda.synchronize()
    got = {n: [] for n in arms}
    for _ in range(rounds):
        for n, (fam, fn) in arms.items():
            old = ops.attn_force_kernels(fam)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            ops.attn_force_kernels(old)
            got[n].append(1e3 * s.elapsed_time(e) / iters)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in got.items()}


def show(title, res):
    print(title, flush=True)
    for n, (med, lo, hi) in res.items():
        print(f"  {n:34s} {med:7.1f} us  (min {lo:6.1f}, max {hi:6.1f})", flush=True)


def bench_attn():
    B, H, Lq, Lk, p = 32, 8, 256, 499, 0.1
    g = torch.Generator(device=dev).manual_seed(0)
    q, do = (torch.randn(B * Lq, H * 64, device=dev, dtype=bf, generator=g) for _ in range(2))
    k, v = (torch.randn(B * Lk, H * 64, device=dev, dtype=bf, generator=g) for _ in range(2))
    o = torch.empty_like(q)
    lse = torch.empty(B * H, Lq, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    db = ops.drop_bits(B, H, Lq, Lk, dev)
    ops.attn_drop_bits(db.view(1, -1), 1, B, H, Lq, Lk, p, 1, 1, 0)

    def fwd(keep, kl):
        return lambda: ops.attn_fwd(q, k, v, o, lse, B, H, Lq, Lk, key_keep=keep, key_len=kl, drop_p=p, seed=1,
                                    rng_stream=1, dbits=db, bits_ready=True)

    def bwd(keep, kl):
        return lambda: ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Lq, Lk, key_keep=keep, key_len=kl,
                                    drop_p=p, seed=1, rng_stream=1, dbits=db)

    ones = torch.ones(B, Lk, dtype=torch.uint8, device=dev)
    ext_all = ops.key_extent(ones)
    fwd(ones, ext_all)()      # an LSE for the backward arms
    show(f"C2 cross forward, nothing to skip (B {B} H {H} Lq {Lq} S {Lk})",
         time_arms({"all-true mask + extent (fwd7 KX)": ("auto", fwd(ones, ext_all)),
                    "unmasked, forced fwd7": ("fwd7", fwd(None, None)),
                    "unmasked, default (fwd8)": ("auto", fwd(None, None))}))
    show("C2 cross backward, nothing to skip",
         time_arms({"all-true mask + extent (bwdf7 KX)": ("auto", bwd(ones, ext_all)),
                    "unmasked (bwdf7)": ("auto", bwd(None, None))}))
    for frac, e in (("S/4", Lk // 4), ("S/2", Lk // 2)):
        keep = (torch.arange(Lk, device=dev)[None] < e).expand(B, Lk).to(torch.uint8).contiguous()
        kl = ops.key_extent(keep)
        fwd(keep, kl)()
        show(f"C2 cross forward, extents {frac} = {e}",
             time_arms({"key_keep + extent (fwd7 KX)": ("auto", fwd(keep, kl)),
                        "key_keep alone, forced fwd7": ("fwd7", fwd(keep, None)),
                        "key_keep alone, default dispatch": ("auto", fwd(keep, None))}))
        show(f"C2 cross backward, extents {frac} = {e}",
             time_arms({"key_keep + extent (bwdf7 KX)": ("auto", bwd(keep, kl)),
                        "key_keep alone (bwdf7)": ("auto", bwd(keep, None)),
                        "key_keep + extent (dq7 + dkv7 KX)": ("nofused", bwd(keep, kl)),
                        "key_keep alone (dq7 + dkv7)": ("nofused", bwd(keep, None))}))
    show("key extent launch (B 32, S 499)", time_arms({"fddm_key_extent": ("auto", lambda: ops.key_extent(ones))}))


def bench_wavlm():
    B, H, S, e = 16, 12, 999, 250
    E = H * 64
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B * S, E, device=dev, dtype=bf, generator=g)
    qkv = torch.randn(B * S, 3 * E, device=dev, dtype=bf, generator=g)
    W = torch.randn(8, 64, device=dev, generator=g) * 0.2
    bias = torch.randn(8, device=dev, generator=g) * 0.1
    cst = torch.rand(H, device=dev, generator=g) + 0.5
    table = torch.randn(H, 2 * S - 1, device=dev, generator=g)
    gw = torch.cat([W[:4].sum(0), W[4:].sum(0), bias[:4].sum().reshape(1), bias[4:].sum().reshape(1)]).contiguous()
    gate = ops.wavlm_gate(x, W, bias, cst, B, S, H)
    out = torch.empty(B * S, E, device=dev, dtype=bf)
    keep = (torch.arange(S, device=dev)[None] < e).expand(B, S).to(torch.uint8).contiguous()
    kl = ops.key_extent(keep)
    a = (qkv, qkv[:, E:], qkv[:, 2 * E:], out)
    show(f"WavLM REL attention, 20 s window (B {B} H {H} S {S}), extents {e}",
         time_arms({"relgate_x + mask + extent (KX)": ("auto", lambda: ops.attn_fwd_relgate_x(
                        *a, x, gw, cst, table, B, H, S, key_keep=keep, key_len=kl)),
                    "general entry, key_keep alone": ("auto", lambda: ops.attn_fwd(
                        *a, None, B, H, S, S, gate=gate, table=table, key_keep=keep)),
                    "relgate_x unmasked (all 999 keys)": ("auto", lambda: ops.attn_fwd_relgate_x(
                        *a, x, gw, cst, table, B, H, S))}, iters=10))


def bench_step(steps=12, warm=4):
    import bench
    args = argparse.Namespace(batch=16, seq_len=256, layers=6, d_model=512, heads=8, precision="bf16", seconds=20.0)
    torch.manual_seed(1337)
    T_, cfg, models, opt = bench.build(args, dev)
    enc, dec, sp, te, tp, sch = models
    batches = bench.synthetic_batches(args, dev, warm + steps, 7)
    g = torch.Generator(device=dev).manual_seed(8)
    lens = [torch.randint(32000, 160001, (args.batch,), device=dev, generator=g) for _ in batches]
    res = {}
    for rnd in range(2):
        for name, loader in (("with lengths", [(w, x, n) for (w, x), n in zip(batches, lens)]),
                             ("without lengths", batches)):
            gs = cfg.lfd["n_step_fd"]
            gs, _ = T_.train_one_epoch(enc, dec, sp, te, tp, sch, loader[:warm], opt, dev, cfg, gs, None, 0, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T_.train_one_epoch(enc, dec, sp, te, tp, sch, loader[warm:], opt, dev, cfg, gs, None, 1, False)
            torch.cuda.synchronize()
            res.setdefault(name, []).append(1e3 * (time.perf_counter() - t0) / steps)
    print(f"train_one_epoch, 20 s batches, B {args.batch}, C2 decoder, lengths U{{2 s .. 10 s}}, {steps} steps:")
    for n, v in res.items():
        print(f"  {n:18s} " + " / ".join(f"{x:7.1f}" for x in v) + " ms per step (two alternating runs)", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["attn", "wavlm"]
    if "attn" in what:
        bench_attn()
    if "wavlm" in what:
        bench_wavlm()
    if "step" in what:
        bench_step()
