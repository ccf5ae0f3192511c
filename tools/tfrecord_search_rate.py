#!/usr/bin/env python3
"""Times of Context.tfrecord_index_search_batch beside
tfrecord_index_batch and beside a device-to-pinned-host copy of the same
streams, one GPU, one process, every figure of a shape from the same run:

  (a) 64 streams of 1 000 records of 2 KiB
  (b) 1 024 streams of 1 000 records of 2 KiB
  (c) one stream of 1 048 576 records of 2 KiB
  (d) one stream of 1 048 576 records of log-uniform length 100 B - 4 KiB
  (e) (c) with the length CRC of every 1 000th record wrong

Two conditions, asserted: the indexes and results the two device calls write
are identical for every shape, and on (c) the search takes less time than the
copy.  The timed calls go through the C ABI over descriptor arrays built once;
the three sides alternate; after the warm-up calls the medians of the timed
ones are printed with the library digest.  All three are synchronous and are
timed with the host clock; the search's passes come from device events around
each launch (s3dg_tfrecord_index_search_timed), in calls of their own.

    timeout -k 10 900 python tools/tfrecord_search_rate.py [--cases abcde] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KiB = 1 << 10
SEED = 0x5EED000000000001
PASSES = ("candidates", "tile sum", "link", "doubling", "anchor walk", "fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import ctypes

    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import TfrStream, TfrWalkRec, call, lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()   # ends in a synchronise of its own
        return (time.perf_counter() - t0) * 1e3

    def line(name, ms, extra=""):
        m = statistics.median(ms)
        say(f"  {name:44s} median {m:10.3f} ms   (min {min(ms):.3f} max {max(ms):.3f} ms, {len(ms)} timed){extra}")
        return m

    T, H = S.tfrecord_search_geometry()
    say(f"tfrecord_search_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, tile {T} B, hop {H} records, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(2)
    shapes = {"a": (64, np.full(1000, 2 * KiB, np.uint64), 0), "b": (1024, np.full(1000, 2 * KiB, np.uint64), 0),
              "c": (1, np.full(1 << 20, 2 * KiB, np.uint64), 0),
              "d": (1, np.floor(np.exp(rng.uniform(np.log(100), np.log(4 * KiB + 1), 1 << 20))).astype(np.uint64), 0),
              "e": (1, np.full(1 << 20, 2 * KiB, np.uint64), 1000)}
    for tag in a.cases:
        nstreams, lens, bad_every = shapes[tag]
        records, payload = len(lens), int(lens.sum())
        framed = payload + 16 * records
        say(f"({tag}) {nstreams} stream(s) of {records} records, {lens.min()}-{lens.max()} B (mean {lens.mean():.0f}), "
            f"{nstreams * framed / 2**30:.2f} GiB of streams" + (f", every {bad_every}th length CRC wrong" if bad_every else ""))
        src = torch.empty(nstreams * payload, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        dst = torch.empty(nstreams * framed, dtype=torch.uint8, device="cuda:0")
        idx = torch.empty(nstreams * records * 16, dtype=torch.uint8, device="cuda:0")
        ctx.tfrecord_frame_var_batch(src, dst, [(k * payload, k * framed, lens, k * records * 16) for k in range(nstreams)], index=idx)
        del src
        if bad_every:
            starts = idx.view(torch.int64).view(-1, 2)[bad_every - 1::bad_every, 0]
            dst[starts + 8] ^= 1
        widx, sidx = torch.zeros_like(idx), torch.zeros_like(idx)
        arr = (TfrStream * nstreams)(*[TfrStream(k * framed, framed, k * records * 16, records) for k in range(nstreams)])
        wres, sres = (TfrWalkRec * nstreams)(), (TfrWalkRec * nstreams)()
        ms6 = (ctypes.c_float * 6)()
        s = int(torch.cuda.current_stream().cuda_stream)
        pd = dst.data_ptr()
        host = torch.empty(nstreams * framed, dtype=torch.uint8).pin_memory()

        def walk():
            call("s3dg_tfrecord_index_batch", ctx._h, pd, widx.data_ptr(), arr, nstreams, s, wres)

        def search():
            call("s3dg_tfrecord_index_search_batch", ctx._h, pd, sidx.data_ptr(), arr, nstreams, s, sres)

        def copy():
            host.copy_(dst, non_blocking=True)
            torch.cuda.synchronize()
        walk()
        search()
        same = torch.equal(widx, sidx) and bytes(wres) == bytes(sres) and torch.equal(widx, idx)
        bad = sum(r.bad_length_crc for r in sres)
        say(f"  indexes and results of the two device calls identical, and the frame's index: {same}; {sum(r.records for r in sres)} records, "
            f"{bad} wrong length CRCs")
        assert same and all(r.records == records and r.status == 0 for r in sres) and bad == (nstreams * (records // bad_every) if bad_every else 0)
        slow = nstreams == 1   # the serial walk of a long stream takes most of a second
        reps, warm = (max(3, a.reps // 4), 1) if slow else (a.reps, a.warmup)
        for _ in range(a.warmup):
            search()
            copy()
        for _ in range(warm):
            walk()
        tw, ts, tc = [], [], []
        for i in range(a.reps):
            ts.append(clock(search))
            if i < reps:
                tw.append(clock(walk))
            tc.append(clock(copy))
        m_s = line("tfrecord_index_search_batch", ts, f"   {statistics.median(ts) * 1e6 / (records * nstreams):.1f} ns per record overall")
        m_w = line("tfrecord_index_batch", tw, f"   {statistics.median(tw) * 1e6 / records:.1f} ns per record per stream")
        m_c = line("device-to-pinned-host copy of the streams", tc, f"   {nstreams * framed / (statistics.median(tc) * 1e6):.1f} GB/s")
        say(f"  ratios (times): walk / search = {m_w / m_s:.3f}, copy / search = {m_c / m_s:.3f}")
        per = []
        for _ in range(a.reps):
            call("s3dg_tfrecord_index_search_timed", ctx._h, pd, sidx.data_ptr(), arr, nstreams, s, sres, ms6)
            per.append(list(ms6))
        meds = [statistics.median(p[i] for p in per) for i in range(6)]
        say("  passes by device events (medians, ms): " + ", ".join(f"{n} {m:.3f}" for n, m in zip(PASSES, meds))
            + f"; sum {sum(meds):.3f} (the rest of the call is its two waits, the sizing and the copies of 8 and {48 * nstreams} bytes)")
        if tag == "c":
            say(f"  condition: search {m_s:.3f} ms < copy {m_c:.3f} ms: {m_s < m_c}")
            assert m_s < m_c, "the search of one long stream is not faster than copying it out"
        del dst, idx, widx, sidx, host
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
