#!/usr/bin/env python3
"""Rates of Context.npz_frame_batch and Context.npz_check_batch (DESIGN.md
§5.5.5), one GPU, one process.  No threshold: every figure is printed beside
its yardsticks from the same run, on the same bytes:

    a device-to-device copy          of the payload (device events)
    crc32_batch, then that copy      what a caller without the call would do (device events)
    tfrecord_frame_var_batch         one record per member into the same destination (device events)
    the host path                    generate_npz_bytes / build_npz of ONE archive into pinned
                                     memory (host clock); n archives would take n times that,
                                     which is worked out, not run

  (a) 1024 archives of one 8 MiB member
  (b) 1024 archives of x.npy (8 MiB) and y.npy (8 zero bytes)
  (c) 65 536 archives of one 128 KiB member
  (d) BASELINE config 4's sizes (10 000 log-uniform, 4 KiB - 64 MiB) as single-member archives

The frame returns without a wait and is timed with device events; the check is
synchronous and is timed with the host clock.  The sides alternate; after the
warm-up calls the medians of the timed ones are printed with the library
digest.  Before anything is timed the framed buffer is held clean by the check
and its first archive is read back by numpy.

    timeout -k 10 900 python tools/npz_batch_rate.py [--cases abcd] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import ctypes
import io
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import NpzRec, c_u64, c_vp, call, lib
    from s3dlio_amd.device import _npz_archives, _spans, _tfr_var_shards

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
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def line(name, ms, total, n):
        m = statistics.median(ms)
        say(f"  {name:46s} median {m:10.3f} ms  {total / (m * 1e6):8.1f} GB/s   (min {min(ms):.3f} max {max(ms):.3f} ms, "
            f"{len(ms)} timed)   {m * 1e6 / n:.1f} ns per archive")
        return m

    def case(tag, what, sizes, with_y, host_one):
        n, total = len(sizes), int(sum(sizes))
        hy = S.npy_header([1], "<i8")
        archives, shards, spans, so, do = [], [], [], 0, 0
        for sz in sizes:
            members = [("x.npy", S.npy_header([sz], "|u1"), so, sz)] + ([("y.npy", hy, None, 8)] if with_y else [])
            archives.append((do, members))
            shards.append((so, do, [sz]))
            spans.append((so, sz))
            so += (sz + 15) // 16 * 16
            do += (S.npz_archive_size(members) + 15) // 16 * 16
        say(f"({tag}) {what}: {n} archives, {total / 2**30:.2f} GiB of payload, {do / 2**30:.2f} GiB of archives")
        src = torch.empty(so, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        dst = torch.empty(do, dtype=torch.uint8, device="cuda:0")
        crcs = torch.empty(n, dtype=torch.int32, device="cuda:0")
        ctx.npz_frame_batch(src, dst, archives)
        res = ctx.npz_check_batch(dst, archives, per_archive=False)
        assert res.ok and res.members == n * (2 if with_y else 1), res
        size0 = S.npz_archive_size(archives[0][1])
        with np.load(io.BytesIO(dst[:size0].cpu().numpy().tobytes())) as z:
            assert z["x"].tobytes() == src[:sizes[0]].cpu().numpy().tobytes(), "the first archive differs from its source"
        # the descriptors once, the C ABI directly: what is timed is the call, not the wrapper's list handling
        arr, na, marr, nm, blob = _npz_archives(archives)[:5]
        pb = ctypes.cast(ctypes.c_char_p(blob), c_vp)
        sarr, ns, lens = _tfr_var_shards(shards)[:3]
        pl = lens.ctypes.data_as(ctypes.POINTER(c_u64))
        parr = _spans(spans)[0]
        st = int(torch.cuda.current_stream().cuda_stream)
        ps, pd, tot = src.data_ptr(), dst.data_ptr(), NpzRec()
        frame = lambda: call("s3dg_npz_frame_batch", ctx._h, ps, pd, arr, na, marr, nm, pb, len(blob), st)   # noqa: E731
        check = lambda: call("s3dg_npz_check_batch", ctx._h, pd, arr, na, marr, nm, pb, len(blob), st, ctypes.byref(tot), None)   # noqa: E731
        copy = lambda: dst[:so].copy_(src, non_blocking=True)   # noqa: E731
        crc_copy = lambda: (call("s3dg_crc32_batch_async", ctx._h, ps, parr, n, st, crcs.data_ptr()), copy())   # noqa: E731
        tfr = lambda: call("s3dg_tfrecord_frame_var_batch", ctx._h, ps, pd, None, sarr, ns, pl, len(lens), st)   # noqa: E731
        for _ in range(a.warmup):
            frame(), check(), copy(), crc_copy(), tfr()
        tf, tc, tp, tq, tt = [], [], [], [], []
        for _ in range(a.reps):
            tf.append(events(frame))
            tc.append(clock(check))
            assert tot.bad_members == 0 and tot.bad_directory == 0
            tp.append(events(copy))
            tq.append(events(crc_copy))
            tt.append(events(tfr))
        mf = line("npz_frame_batch (device events)", tf, total, n)
        mc = line("npz_check_batch (host clock)", tc, total, n)
        mp = line("device-to-device copy of the payload", tp, total, n)
        mq = line("crc32_batch, then that copy", tq, total, n)
        mt = line("tfrecord_frame_var_batch, a record per member", tt, total, n)
        th = [clock(host_one) for _ in range(5)]
        mh = statistics.median(th)
        say(f"  host path, ONE archive of the first size       median {mh:10.3f} ms; {n} of them one after another: "
            f"{mh * n:.0f} ms (worked out, not run)")
        say(f"    frame / copy = {mf / mp:.3f}; frame / (crc + copy) = {mf / mq:.3f}; frame / tfrecord frame = {mf / mt:.3f}; "
            f"check / copy = {mc / mp:.3f}; {n} host archives / frame = {mh * n / mf:.0f}")
        ctx.npz_frame_batch(src, dst, archives)   # the yardsticks wrote over it; leave what the call writes
        del src, dst, crcs
        torch.cuda.empty_cache()

    say(f"npz_batch_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    raw8 = lambda: S.generate_npz_bytes([8 * MiB // 4], "<f4", 1)   # x.npy of 8 MiB and y.npy   # noqa: E731
    if "a" in a.cases:
        case("a", "one member of 8 MiB", [8 * MiB] * 1024, False, raw8)
    if "b" in a.cases:
        case("b", "x.npy of 8 MiB and y.npy", [8 * MiB] * 1024, True, raw8)
    if "c" in a.cases:
        pay = np.zeros(128 * KiB, np.uint8)
        case("c", "one member of 128 KiB", [128 * KiB] * 65536, False, lambda: S.build_npz(128 * KiB, 1, pay))
    if "d" in a.cases:
        from bench import log_uniform_sizes
        sizes = [int(s) for s in log_uniform_sizes(10000)]
        case("d", "BASELINE config 4's sizes as single-member archives", sizes, False,
             lambda: S.generate_npz_bytes([sizes[0] // 4], "<f4", 1))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
