#!/usr/bin/env python3
"""Rates of Context.tfrecord_frame_batch and tfrecord_check_batch
(s3dg_tfrecord_frame_batch / _check_batch), one GPU, one
process, in GB/s of payload.

  (a) 1024 shards of one 8 MiB record: frame and check; against the two passes
      the fused kernel replaces (crc32_batch over the source records plus a
      device-to-device copy of the same bytes into the records' places; the
      record size is a multiple of 16); against ONE s3dg_crc32 over the same
      8 GiB as a single buffer, the ceiling of the row loop; and against the
      host path, s3dg_build_tfrecord over 64 of the records in pinned memory.
  (b) 64 shards of 1 000 records of 128 KiB: frame and check.
  (c) one shard of 1 048 576 records of 2 KiB: frame and check.
  (d) one shard of 1 048 576 records of 100 B: one wave per record bounds tiny
      records; time per record.

The timed calls go through the C ABI over a descriptor array built once, as
tools/crc_batch_rate.py times its calls.  The sides of a comparison alternate;
after the warm-up calls the medians of the timed ones are printed with the
library digest.  The frame form returns without a wait and is timed with HIP
events; the check form ends in a synchronise and is timed with the host clock.  A few records of every list are held to the
oracle before anything is timed, and every list checks clean.

    timeout -k 10 900 python tools/tfrecord_rate.py [--cases abcd] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KiB, MiB = 1 << 10, 1 << 20
SEED = 0x5EED000000000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import Span, TfrRec, call, lib
    from s3dlio_amd.device import _tfr_shards
    from oracle.format_oracle import build_tfrecord_with_index

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

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def med(ms):
        return statistics.median(ms), min(ms), max(ms)

    def line(name, ms, total, extra=""):
        m, lo, hi = med(ms)
        say(f"  {name:40s} median {m:10.3f} ms  {total / (m * 1e6):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms, "
            f"{len(ms)} timed){extra}")
        return m

    def shards_of(nshards, records, rs):
        """Packed shards: payloads back to back, streams back to back (rs a multiple of 16)."""
        return [(k * records * rs, k * records * (rs + 16), records, rs, k * records * 16) for k in range(nshards)]

    def setup(nshards, records, rs):
        total = nshards * records * rs
        src = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        dst = torch.empty(nshards * records * (rs + 16), dtype=torch.uint8, device="cuda:0")
        idx = torch.empty(nshards * records * 16, dtype=torch.uint8, device="cuda:0")
        shards = shards_of(nshards, records, rs)
        ctx.tfrecord_frame_batch(src, dst, shards, index=idx)
        torch.cuda.synchronize()
        for s_off, d_off, n, _, i_off in (shards[0], shards[-1]):   # a few records against the oracle
            m = min(n, 3)
            want, widx = build_tfrecord_with_index(m, rs, src[s_off:s_off + m * rs].cpu().numpy().tobytes())
            assert dst[d_off:d_off + m * (rs + 16)].cpu().numpy().tobytes() == want, "stream differs"
            assert idx[i_off:i_off + 16 * m].cpu().numpy().tobytes() == widx, "index differs"
        res = ctx.tfrecord_check_batch(dst, shards)
        assert res.ok and res.records == nshards * records, res
        return src, dst, idx, shards, total

    def sides(src, dst, idx, shards):
        """The two calls over a descriptor array built once, through the C ABI: what a
        native caller pays, without Python's conversion of the list."""
        arr, n = _tfr_shards(shards)[:2]
        s = int(torch.cuda.current_stream().cuda_stream)
        tot = TfrRec()
        ps, pd, pi = src.data_ptr(), dst.data_ptr(), idx.data_ptr()
        return (lambda: call("s3dg_tfrecord_frame_batch", ctx._h, ps, pd, pi, arr, n, s),
                lambda: call("s3dg_tfrecord_check_batch", ctx._h, pd, arr, n, s, ctypes.byref(tot), None))

    def frame_check(src, dst, idx, shards, total, per=""):
        frame, check = sides(src, dst, idx, shards)
        for _ in range(a.warmup):
            frame()
            check()
        tf, tc = [], []
        for _ in range(a.reps):
            tf.append(events(frame))
            tc.append(clock(check))
        n = sum(s[2] for s in shards)
        mf = line("tfrecord_frame_batch (device events)", tf, total, f"   {med(tf)[0] * 1e6 / n:.1f} ns per record" if per else "")
        mc = line("tfrecord_check_batch", tc, total, f"   {med(tc)[0] * 1e6 / n:.1f} ns per record" if per else "")
        return mf, mc

    say(f"tfrecord_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")

    if "a" in a.cases:
        n, rs = 1024, 8 * MiB
        say(f"(a) {n} shards of one {rs // MiB} MiB record, {n * rs / 2**30:.2f} GiB of payload")
        src, dst, idx, shards, total = setup(n, 1, rs)
        crcs = torch.empty(n, dtype=torch.int32, device="cuda:0")
        spans = np.array([(k * rs, rs) for k in range(n)], np.uint64)
        body = dst.view(n, rs + 16)[:, 12:12 + rs]
        rows = src.view(n, rs)
        v = ctypes.c_uint32()

        frame, check = sides(src, dst, idx, shards)
        span_arr = (Span * n)()
        ctypes.memmove(span_arr, spans.ctypes.data, 16 * n)
        cs = int(torch.cuda.current_stream().cuda_stream)

        def two_pass():
            call("s3dg_crc32_batch_async", ctx._h, src.data_ptr(), span_arr, n, cs, crcs.data_ptr())
            body.copy_(rows)

        def copy_only():
            body.copy_(rows)

        def single():
            call("s3dg_crc32", ctx._h, src.data_ptr(), total, None, ctypes.byref(v))
        for _ in range(a.warmup):
            frame()
            check()
            two_pass()
            single()
        tf, tc, t2, tcp, ts = [], [], [], [], []
        for _ in range(a.reps):
            tf.append(events(frame))
            t2.append(events(two_pass))
            tc.append(clock(check))
            ts.append(clock(single))
            tcp.append(events(copy_only))
        mf = line("tfrecord_frame_batch (device events)", tf, total)
        line("tfrecord_check_batch", tc, total)
        m2 = line("crc32_batch + device copy (two passes)", t2, total)
        line("  of which the device copy alone", tcp, total)
        ms = line("s3dg_crc32, one 8 GiB buffer", ts, total)
        say(f"  ratio two passes / fused frame (times) = {m2 / mf:.3f};  fused frame / single-buffer CRC (rates) = {ms / mf:.3f}")
        # the host path over 64 of the records, pinned
        hn = 64
        hsrc = torch.empty(hn * rs, dtype=torch.uint8).pin_memory()
        hdst = torch.empty(hn * (rs + 16), dtype=torch.uint8).pin_memory()
        hsrc.copy_(src[:hn * rs])
        th = []
        for r in range(a.host_reps + 1):
            t0 = time.perf_counter()
            call("s3dg_build_tfrecord", hn, rs, hsrc.data_ptr(), hdst.data_ptr(), None)
            if r:
                th.append((time.perf_counter() - t0) * 1e3)
        assert bytes(hdst[:rs + 16].numpy()) == dst[:rs + 16].cpu().numpy().tobytes(), "host and device streams differ"
        mh = line(f"s3dg_build_tfrecord, {hn} records, pinned host", th, hn * rs)
        say(f"  ratio device frame / host path (rates) = {(total / mf) / (hn * rs / mh):.0f}")
        del src, dst, idx, body, rows, hsrc, hdst
        torch.cuda.empty_cache()

    if "b" in a.cases:
        say(f"(b) 64 shards of 1000 records of 128 KiB, {64 * 1000 * 128 * KiB / 2**30:.2f} GiB of payload")
        src, dst, idx, shards, total = setup(64, 1000, 128 * KiB)
        frame_check(src, dst, idx, shards, total)
        del src, dst, idx
        torch.cuda.empty_cache()

    if "c" in a.cases:
        say(f"(c) one shard of {1 << 20} records of 2 KiB, {(1 << 20) * 2 * KiB / 2**30:.2f} GiB of payload")
        src, dst, idx, shards, total = setup(1, 1 << 20, 2 * KiB)
        frame_check(src, dst, idx, shards, total, per="record")
        del src, dst, idx
        torch.cuda.empty_cache()

    if "d" in a.cases:
        say(f"(d) one shard of {1 << 20} records of 100 B (packed at a multiple of 16 overall), "
            f"{(1 << 20) * 100 / 2**20:.1f} MiB of payload")
        src, dst, idx, shards, total = setup(1, 1 << 20, 100)
        frame_check(src, dst, idx, shards, total, per="record")
        del src, dst, idx
        torch.cuda.empty_cache()

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
