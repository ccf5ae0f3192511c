#!/usr/bin/env python3
"""Rate of measure_stream against the verify and the fill of the same bytes, one GPU.

Four payloads of 8 GiB each (far beyond the L2 and the Infinity Cache), in one
process and one buffer:

    controlled d1 c1 and d4 c2, 1024 x 8 MiB, measured at 4 KiB blocks
    DG1 d1 c1, 8 x 1 GiB, measured at 1 MiB blocks and at 4 KiB blocks

For each, after 5 warm-up launches, 20 launches of each of these are timed with
HIP events and the medians printed in GB/s: the add (k_measure +
k_measure_blocks) into a handle that was reset before the events, the add
with the byte histogram (k_byte_hist as well; the histogram's own time is the
difference of the two medians), and the yardsticks over the same buffer:
verify_stream / verify_dgen_stream and fill_stream / dgen_fill_stream.
result() (the distinct count: two radix sorts on a copy and the count) is
synchronous and timed on the host clock.  The ratios add / verify and add /
fill are the numbers to quote.

    python tools/measure_rate.py [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    total = a.gib << 30
    seed = 0x5EED000000000001
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, before=None):
        ms = []
        for k in range(a.warmup + a.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def gbs(ms):
        return total / (ms * 1e6)

    say(f"measure_rate: {a.gib} GiB per payload, {a.reps} timed after {a.warmup} warm-up, "
        f"digest {lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    ctl = dict(obj_size=8 * MiB, n_objs=total // (8 * MiB))
    dg = dict(obj_size=1 << 30, n_objs=total >> 30)
    cases = [("controlled d1 c1 @ 4 KiB", ctx.fill_stream, ctx.verify_stream, ctl, dict(dedup=1, compress=1), 4096),
             ("controlled d4 c2 @ 4 KiB", ctx.fill_stream, ctx.verify_stream, ctl, dict(dedup=4, compress=2), 4096),
             ("DG1 d1 c1 @ 1 MiB", ctx.dgen_fill_stream, ctx.verify_dgen_stream, dg, dict(dedup=1, compress=1), MiB),
             ("DG1 d1 c1 @ 4 KiB", ctx.dgen_fill_stream, ctx.verify_dgen_stream, dg, dict(dedup=1, compress=1), 4096)]
    for name, fill, verify, shape, knobs, bb in cases:
        kw = dict(shape, seed_base=seed, **knobs)
        fill(buf, **kw)
        torch.cuda.synchronize()
        assert verify(buf, **kw).ok
        res = {}
        with ctx.measurer(bb) as m, ctx.measurer(bb, hist=True) as mh:
            m.add_stream(buf, **shape)          # first add: the array grows to its size
            r = m.result()
            res["add (k_measure + k_measure_blocks)"] = timed(lambda: m.add_stream(buf, **shape), m.reset)
            m.reset()
            m.add_stream(buf, **shape)
            t = []
            for _ in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                r2 = m.result()
                t.append((time.perf_counter() - t0) * 1e3)
            assert r2 == r
            t = t[a.warmup:]
            mh.add_stream(buf, **shape)
            res["add with histogram (+ k_byte_hist)"] = timed(lambda: mh.add_stream(buf, **shape), mh.reset)
            rh = mh.result()
        res["verify"] = timed(lambda: verify(buf, **kw))
        res["fill"] = timed(lambda: fill(buf, **kw))
        say(f"--- {name}: {r.blocks} blocks, {r.unique_blocks} distinct (dedup {r.dedup_ratio:.3f} : 1), "
            f"zero fraction {r.zero_fraction:.4f}, entropy {rh.entropy_bits:.4f} bits/byte")
        for k, (med, lo, hi) in res.items():
            say(f"{k:40s} median {med:8.3f} ms  {gbs(med):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
        say(f"{'result() (distinct count, host clock)':40s} median {statistics.median(t):8.3f} ms"
            f"               (min {min(t):.3f} max {max(t):.3f} ms)")
        add, addh = res["add (k_measure + k_measure_blocks)"][0], res["add with histogram (+ k_byte_hist)"][0]
        v, f = res["verify"][0], res["fill"][0]
        hist_ms = addh - add
        say(f"ratio add / verify = {v / add:.3f}   add / fill = {f / add:.3f}   "
            f"histogram pass alone {hist_ms:.3f} ms = {gbs(hist_ms) if hist_ms > 0 else float('nan'):.1f} GB/s")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
