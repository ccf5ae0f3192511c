#!/usr/bin/env python3
"""Rate of Context.crc32_batch (s3dg_crc32_batch) against s3dg_crc32, the only
device CRC before it, over the same bytes, one GPU, one process.

  (a) BASELINE config 4's objects (10 000 log-uniform sizes, 4 KiB..64 MiB, as
      bench.py --config 4 lays them out) in a dgen_fill_batch arena: one
      crc32_batch against one s3dg_crc32 per object.  Both end in a
      synchronise, so both are timed with the host clock; the per-object loop
      runs through ctypes, which is what a Python caller pays.
  (b) 1024 x 8 MiB of keystream bytes: crc32_batch against ONE s3dg_crc32 over
      the same 8 GiB as a single buffer, the ceiling of the row loop.  The
      ratio is reported; it is not a pass mark.
  (c) 200 000 packed objects of 16 B..8 KiB: time per object, which prices the
      table's build and upload and the fold.

The sides of a comparison alternate; after the warm-up calls the medians of the
timed ones are printed with the library digest.  The asynchronous form into a
device tensor is timed with HIP events beside the synchronous one.  The values
of the two sides are compared before anything is timed.

    timeout -k 10 900 python tools/crc_batch_rate.py [--cases abc] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KiB, MiB = 1 << 10, 1 << 20
SEED = 0x5EED000000000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--each-reps", type=int, default=5, help="timed repeats of the one-call-per-object side of (a)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import Span, call, lib

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
        say(f"  {name:34s} median {m:10.3f} ms  {total / (m * 1e6):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms, "
            f"{len(ms)} timed){extra}")
        return m

    def sides(buf, spans):
        """The batch call's two forms over `spans` of buf, ready to time."""
        n = len(spans)
        arr = (Span * n)()
        flat = np.ascontiguousarray(np.array(spans, np.uint64))   # held until the copy is done
        ctypes.memmove(arr, flat.ctypes.data, 16 * n)
        p, s = buf.data_ptr(), int(torch.cuda.current_stream().cuda_stream)
        host = np.zeros(n, np.uint32)
        hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        dev = torch.empty(n, dtype=torch.int32, device="cuda:0")
        return (host, dev, lambda: call("s3dg_crc32_batch", ctx._h, p, arr, n, s, hp),
                lambda: call("s3dg_crc32_batch_async", ctx._h, p, arr, n, s, dev.data_ptr()))

    say(f"crc_batch_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")

    if "a" in a.cases:
        from bench import log_uniform_sizes
        sizes, offs, cur = log_uniform_sizes(10000), [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 4095) // 4096 * 4096
        total, n = sum(sizes), len(sizes)
        say(f"(a) config 4: {n} objects, {total / 2**30:.2f} GiB in a {cur / 2**30:.2f} GiB dgen_fill_batch arena")
        buf = torch.empty(cur, dtype=torch.uint8, device="cuda:0")
        ctx.dgen_fill_batch(buf, [(o, sz, SEED + k, 1, 1) for k, (o, sz) in enumerate(zip(offs, sizes))])
        torch.cuda.synchronize()
        host, dev, sync_call, async_call = sides(buf, list(zip(offs, sizes)))
        one = np.zeros(n, np.uint32)
        ptrs = [(buf.data_ptr() + o, sz, ctypes.byref(ctypes.c_uint32.from_buffer(one, 4 * k)))
                for k, (o, sz) in enumerate(zip(offs, sizes))]
        h, crc32 = ctx._h, lib.s3dg_crc32

        def each():
            for p, sz, out in ptrs:
                if crc32(h, p, sz, None, out):
                    raise RuntimeError("s3dg_crc32 failed")
        sync_call()
        each()
        async_call()
        torch.cuda.synchronize()
        assert np.array_equal(host, one) and np.array_equal(dev.cpu().numpy().view(np.uint32), one), "values differ"
        for _ in range(a.warmup):
            sync_call()
        tb, te, ta = [], [], []
        for r in range(a.reps):
            tb.append(clock(sync_call))
            ta.append(events(async_call))
            if r < a.each_reps:
                te.append(clock(each))
        mb = line("crc32_batch, one call", tb, total)
        line("crc32_batch async (device events)", ta, total)
        me = line("s3dg_crc32, one call per object", te, total)
        say(f"  ratio per-object / crc32_batch = {me / mb:.1f}")
        del buf
        torch.cuda.empty_cache()

    if "b" in a.cases:
        n, size = 1024, 8 * MiB
        total = n * size
        say(f"(b) 1024 x 8 MiB of keystream bytes, {total / 2**30:.2f} GiB")
        buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(buf, seed_base=SEED)
        torch.cuda.synchronize()
        host, dev, sync_call, async_call = sides(buf, [(j * size, size) for j in range(n)])
        v = ctypes.c_uint32()
        p = buf.data_ptr()

        def single():
            call("s3dg_crc32", ctx._h, p, total, None, ctypes.byref(v))
        for _ in range(a.warmup):
            sync_call()
            single()
            async_call()
        head = buf[:size].cpu().numpy()
        assert int(host[0]) == S.lib.s3dg_crc32_host(0, head.ctypes.data, size), "values differ"
        tb, ts, ta = [], [], []
        for _ in range(a.reps):
            tb.append(clock(sync_call))
            ts.append(clock(single))
            ta.append(events(async_call))
        mb = line("crc32_batch, 1024 objects", tb, total)
        line("crc32_batch async (device events)", ta, total)
        ms = line("s3dg_crc32, one 8 GiB buffer", ts, total)
        say(f"  ratio crc32_batch / single buffer (rates) = {ms / mb:.3f}")
        del buf
        torch.cuda.empty_cache()

    if "c" in a.cases:
        rng = random.Random(12)
        n = 200000
        sizes = [int(16 * (512 ** rng.random())) for _ in range(n)]
        offs, cur = [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 15) // 16 * 16
        total = sum(sizes)
        say(f"(c) {n} packed objects of {min(sizes)} B..{max(sizes)} B, {total / 2**20:.1f} MiB")
        buf = torch.empty((cur + 4095) // 4096 * 4096, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(buf, seed_base=SEED)
        torch.cuda.synchronize()
        host, dev, sync_call, async_call = sides(buf, list(zip(offs, sizes)))
        for _ in range(a.warmup):
            sync_call()
            async_call()
        hb = buf.cpu().numpy()
        for k in (0, 1, n // 2, n - 1):
            assert int(host[k]) == S.lib.s3dg_crc32_host(0, hb.ctypes.data + offs[k], sizes[k]), "values differ"
        tb, ta, th = [], [], []
        for _ in range(a.reps):
            tb.append(clock(sync_call))
            ta.append(events(async_call))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            async_call()   # returns without waiting: the host's share (checks, table, enqueue)
            th.append((time.perf_counter() - t0) * 1e3)
        mb = line("crc32_batch, one call", tb, total, f"   {med(tb)[0] * 1e6 / n:.1f} ns per object")
        line("crc32_batch async (device events)", ta, total, f"   {med(ta)[0] * 1e6 / n:.1f} ns per object")
        line("crc32_batch async, host call alone", th, total, f"   {med(th)[0] * 1e6 / n:.1f} ns per object")
        del buf
        torch.cuda.empty_cache()

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
