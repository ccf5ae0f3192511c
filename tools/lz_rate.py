#!/usr/bin/env python3
"""Rate of the LZ4 size add against the chunker's add and the fixed-block
measure of the same bytes, one GPU.

Four payloads of 8 GiB each (far beyond the L2 and the Infinity Cache), in one
process and one buffer:

    controlled d1 c1 and d4 c2, 1024 x 8 MiB
    DG1 d1 c1, 8 x 1 GiB (keystream bytes: no match to walk)
    bytes drawn from 4 values, 1024 x 8 MiB (15 044 matches per 64 KiB block,
    904 per 4 KiB block, measured: the walk's worst case)

For each, after 5 warm-up launches, 20 launches of each of these are timed with
HIP events and the medians printed in GB/s: LzMeasure.add_stream at block_bytes
4096 and 65536 into a handle that was reset before the events,
Measure.add_stream at 4 KiB blocks and Chunker.add_stream at its defaults.  The
ratio LZ add / chunk add is the number to quote: both are one read plus a
data-dependent serial walk.

    python tools/lz_rate.py [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import os
import statistics
import sys

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

    def four_values(t, **_):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(4)
        step = 1 << 30
        for lo in range(0, total, step):
            t[lo:lo + step] = torch.randint(0, 4, (min(step, total - lo),), dtype=torch.uint8, device="cuda:0",
                                            generator=g)

    say(f"lz_rate: {a.gib} GiB per payload, {a.reps} timed after {a.warmup} warm-up, "
        f"digest {lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    ctl = dict(obj_size=8 * MiB, n_objs=total // (8 * MiB))
    dg = dict(obj_size=1 << 30, n_objs=total >> 30)
    cases = [("controlled d1 c1, 1024 x 8 MiB", ctx.fill_stream, ctl, dict(seed_base=seed, dedup=1, compress=1)),
             ("controlled d4 c2, 1024 x 8 MiB", ctx.fill_stream, ctl, dict(seed_base=seed, dedup=4, compress=2)),
             ("DG1 d1 c1, 8 x 1 GiB", ctx.dgen_fill_stream, dg, dict(seed_base=seed, dedup=1, compress=1)),
             ("bytes of 4 values, 1024 x 8 MiB", four_values, ctl, {})]
    for name, fill, shape, knobs in cases:
        fill(buf, **shape, **knobs)
        torch.cuda.synchronize()
        say(f"--- {name}")
        res, lz = {}, {}
        for bb in (4096, 65536):
            with ctx.lz_measurer(bb) as h:
                h.add_stream(buf, **shape)
                lz[bb] = h.result()
                res[f"lz add at {bb}"] = timed(lambda: h.add_stream(buf, **shape), h.reset)
                h.reset()
                h.add_stream(buf, **shape)
                assert h.result() == lz[bb]
            r = lz[bb]
            say(f"block_bytes {bb:5d}: ratio {r.ratio:.3f} (lz_ratio {r.lz_ratio:.3f}), {r.matches / r.blocks:.1f} matches "
                f"per block, match fraction {r.match_fraction:.3f}, raw blocks {r.raw_fraction:.3f}")
        with ctx.chunker() as c, ctx.measurer(4096) as m:
            c.add_stream(buf, **shape)          # first add: the arrays and the scratch grow to their size
            c.result()
            res["chunk add at 2048 / 8192 / 65536"] = timed(lambda: c.add_stream(buf, **shape), c.reset)
            m.add_stream(buf, **shape)
            m.result()
            res["measure add at 4 KiB blocks"] = timed(lambda: m.add_stream(buf, **shape), m.reset)
        for k, (med, lo, hi) in res.items():
            say(f"{k:40s} median {med:9.3f} ms  {gbs(med):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
        chunk = res["chunk add at 2048 / 8192 / 65536"][0]
        say("ratio lz add / chunk add = " + "   ".join(f"{chunk / res[f'lz add at {bb}'][0]:.3f} at {bb}"
                                                        for bb in (4096, 65536)))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
