#!/usr/bin/env python3
"""Rate of the content-defined chunking add against the fixed-block measure and
the verify of the same bytes, one GPU.

Three payloads of 8 GiB each (far beyond the L2 and the Infinity Cache), in one
process and one buffer, chunked at the defaults (2048 / 8192 / 65536):

    controlled d1 c1 and d4 c2, 1024 x 8 MiB
    DG1 d1 c1, 8 x 1 GiB (one wave walks each object's cuts: pass B's share shows here)

For each, after 5 warm-up launches, 20 launches of each of these are timed with
HIP events and the medians printed in GB/s: Chunker.add_stream into a handle
that was reset before the events (G from LDS, the default, and G computed per
byte), Measure.add_stream at 4 KiB blocks and verify_stream /
verify_dgen_stream over the same buffer.  The add's three passes (A candidates,
B cuts, C fingerprints) are timed by the handle's own HIP events in a second
series of 20, medians again.  result() (two radix sorts and the count) is
synchronous and timed on the host clock.  The ratio chunk add / measure add is
the number to quote; the add reads the payload twice (A and C), so about 0.5 is
what to compare it with.

    python tools/chunk_rate.py [--log FILE]
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

    say(f"chunk_rate: {a.gib} GiB per payload, chunks 2048 / 8192 / 65536, {a.reps} timed after {a.warmup} warm-up, "
        f"digest {lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    ctl = dict(obj_size=8 * MiB, n_objs=total // (8 * MiB))
    dg = dict(obj_size=1 << 30, n_objs=total >> 30)
    cases = [("controlled d1 c1, 1024 x 8 MiB", ctx.fill_stream, ctx.verify_stream, ctl, dict(dedup=1, compress=1)),
             ("controlled d4 c2, 1024 x 8 MiB", ctx.fill_stream, ctx.verify_stream, ctl, dict(dedup=4, compress=2)),
             ("DG1 d1 c1, 8 x 1 GiB", ctx.dgen_fill_stream, ctx.verify_dgen_stream, dg, dict(dedup=1, compress=1))]
    for name, fill, verify, shape, knobs in cases:
        kw = dict(shape, seed_base=seed, **knobs)
        fill(buf, **kw)
        torch.cuda.synchronize()
        assert verify(buf, **kw).ok
        res = {}
        with ctx.chunker() as h, ctx.measurer(4096) as m:
            h.add_stream(buf, **shape)          # first add: the arrays and the scratch grow to their size
            r = h.result()
            res["chunk add (A + B + C), G from LDS"] = timed(lambda: h.add_stream(buf, **shape), h.reset)
            h.gear_table(False)
            res["chunk add, G computed per byte"] = timed(lambda: h.add_stream(buf, **shape), h.reset)
            h.reset()
            h.add_stream(buf, **shape)
            assert h.result() == r               # both forms of pass A: the same result
            passes = {}
            for table in (True, False):
                h.gear_table(table)
                h.time_passes(True)
                ps = []
                for k in range(a.warmup + a.reps):
                    h.reset()
                    h.add_stream(buf, **shape)
                    if k >= a.warmup:
                        ps.append(h.pass_seconds())
                h.time_passes(False)
                passes[table] = [statistics.median(p[i] for p in ps) * 1e3 for i in range(3)]
            h.gear_table(True)
            h.reset()
            h.add_stream(buf, **shape)
            t = []
            for _ in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                r2 = h.result()
                t.append((time.perf_counter() - t0) * 1e3)
            assert r2 == r
            t = t[a.warmup:]
            m.add_stream(buf, **shape)
            rm = m.result()
            res["measure add at 4 KiB blocks"] = timed(lambda: m.add_stream(buf, **shape), m.reset)
        res["verify"] = timed(lambda: verify(buf, **kw))
        say(f"--- {name}: {r.chunks} chunks (mean {r.mean_chunk:.0f} B), {r.unique_chunks} distinct, "
            f"dedup {r.dedup_ratio:.3f} : 1 by bytes, {r.candidates} candidates, {r.forced_cuts} forced cuts; "
            f"fixed 4 KiB blocks: dedup {rm.dedup_ratio:.3f} : 1")
        for k, (med, lo, hi) in res.items():
            say(f"{k:40s} median {med:9.3f} ms  {gbs(med):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
        for table, label in ((True, "G from LDS"), (False, "G computed")):
            pa, pb, pc = passes[table]
            say(f"passes, {label:12s}: A candidates {pa:9.3f} ms ({gbs(pa):7.1f} GB/s)  B cuts {pb:9.3f} ms  "
                f"C fingerprints {pc:9.3f} ms ({gbs(pc):7.1f} GB/s)  B's share {pb / (pa + pb + pc):.3f}")
        say(f"{'result() (distinct count, host clock)':40s} median {statistics.median(t):9.3f} ms"
            f"               (min {min(t):.3f} max {max(t):.3f} ms)")
        add = res["chunk add (A + B + C), G from LDS"][0]
        say(f"ratio chunk add / measure add = {res['measure add at 4 KiB blocks'][0] / add:.3f}   "
            f"chunk add / verify = {res['verify'][0] / add:.3f}")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
