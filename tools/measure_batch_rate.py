#!/usr/bin/env python3
"""Rate of the batch adds (s3dg_measure_add_batch, s3dg_chunks_add_batch,
s3dg_lz_add_batch) against the same handle's add_stream, over the same bytes,
one GPU, one process.

  (a) 1024 x 8 MiB d1 c1 described as a batch, against add_stream over the
      same buffer.  The ratio is the figure to quote: the extra work is the
      table's upload, one scalar record load per granule (measure, chunker)
      and one search per block or slot.
  (b) BASELINE config 4's objects (10 000 log-uniform sizes, 4 KiB..64 MiB,
      d2 c1.5, as bench.py --config 4 lays them out in one buffer); the
      results are printed too: dedup_ratio, the chunker's dedup_ratio and the
      LZ ratio at 4 KiB and 64 KiB.
  (c) 200 000 objects of 20 KiB + 5 packed at 16 bytes.

Handles: Measure at 4096, Chunker at the defaults, LzMeasure at 4096 and
65536.  Each buffer is filled once with fill_batch.  After 5 warm-up adds, 20
adds of each are timed with HIP events (the handle is reset before each, outside
the events, so its arrays do not grow) and the medians printed in GB/s with
the library digest.  The span array is built once; the timed calls are the C
calls, table build and upload included.

    timeout -k 10 900 python tools/measure_batch_rate.py [--cases abc] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MiB = 1 << 20
SEED = 0x5EED000000000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import Span, call, lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(pre, fn):
        for _ in range(a.warmup):
            pre()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    handles = [("measure 4096", "measure", lambda: ctx.measurer(4096)),
               ("chunks 2048/8192/65536", "chunks", lambda: ctx.chunker()),
               ("lz 4096", "lz", lambda: ctx.lz_measurer(4096)),
               ("lz 65536", "lz", lambda: ctx.lz_measurer(65536))]

    def run(title, sizes, offs, d, c, stream_kw=None, results=False):
        n, total, end = len(sizes), sum(sizes), max(o + s for o, s in zip(offs, sizes))
        say(f"{title}: {n} objects, {total / 2**30:.2f} GiB in a {end / 2**30:.2f} GiB buffer, dedup {d} compress {c}")
        buf = torch.empty(end, dtype=torch.uint8, device="cuda:0")
        ctx.fill_batch(buf, [(o, sz, S.object_entropy(SEED, k), d, c) for k, (o, sz) in enumerate(zip(offs, sizes))])
        torch.cuda.synchronize()
        arr = (Span * n)()
        for k, (o, sz) in enumerate(zip(offs, sizes)):
            arr[k] = Span(o, sz)
        p, s = buf.data_ptr(), int(torch.cuda.current_stream().cuda_stream)
        for name, sym, make in handles:
            with make() as h:
                fn = f"s3dg_{sym}_add_batch"
                b = timed(h.reset, lambda: call(fn, h._h, p, arr, n, s))
                r = h.result()
                # the call's own time on the host (checks, table build, enqueue), the GPU idle before it
                torch.cuda.synchronize()
                h.reset()
                t0 = time.perf_counter()
                call(fn, h._h, p, arr, n, s)
                host_ms = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                line = f"  {name:24s} add_batch  median {b[0]:9.3f} ms  {total / (b[0] * 1e6):8.1f} GB/s   " \
                       f"(min {b[1]:.3f} max {b[2]:.3f} ms)   host call {host_ms:.3f} ms"
                say(line)
                if sym == "chunks":      # the three passes by their own HIP events, batch and stream
                    h.time_passes(True)
                    h.reset()
                    call(fn, h._h, p, arr, n, s)
                    pb = h.pass_seconds()
                    say("    passes A / B / C of add_batch : " + " / ".join(f"{x * 1e3:.3f}" for x in pb) + " ms")
                    if stream_kw:
                        h.reset()
                        h.add_stream(buf, **stream_kw)
                        ps = h.pass_seconds()
                        say("    passes A / B / C of add_stream: " + " / ".join(f"{x * 1e3:.3f}" for x in ps) + " ms")
                    h.time_passes(False)
                if stream_kw:
                    st = timed(h.reset, lambda: h.add_stream(buf, **stream_kw))
                    assert h.result() == r, (name, "add_stream and add_batch disagree")
                    say(f"  {name:24s} add_stream median {st[0]:9.3f} ms  {total / (st[0] * 1e6):8.1f} GB/s   "
                        f"(min {st[1]:.3f} max {st[2]:.3f} ms)   ratio add_batch / add_stream = {st[0] / b[0]:.3f}")
                if results:
                    if sym == "measure":
                        say(f"    result: blocks {r.blocks} unique {r.unique_blocks} dedup_ratio {r.dedup_ratio:.4f} "
                            f"zero_fraction {r.zero_fraction:.4f}")
                    elif sym == "chunks":
                        say(f"    result: chunks {r.chunks} unique {r.unique_chunks} dedup_ratio {r.dedup_ratio:.4f}")
                    else:
                        say(f"    result: blocks {r.blocks} stored_bytes {r.stored_bytes} ratio {r.ratio:.4f} "
                            f"raw_blocks {r.raw_blocks}")
        del buf
        torch.cuda.empty_cache()

    say(f"measure_batch_rate: {a.reps} timed after {a.warmup} warm-up, digest {lib.s3dg_build_digest().decode()}, "
        f"{torch.cuda.get_device_name(0)}")
    if "a" in a.cases:
        n, size = 1024, 8 * MiB
        run("(a) 1024 x 8 MiB", [size] * n, [j * size for j in range(n)], 1, 1,
            dict(obj_size=size, n_objs=n))
    if "b" in a.cases:
        from bench import log_uniform_sizes
        sizes, offs, cur = log_uniform_sizes(10000), [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 4095) // 4096 * 4096
        run("(b) config 4", sizes, offs, 2, (3, 2), results=True)
    if "c" in a.cases:
        n, size = 200000, 20 * 1024 + 5
        st = (size + 15) // 16 * 16
        run("(c) 200 000 x (20 KiB + 5), 16-byte packed", [size] * n, [j * st for j in range(n)], 1, 1,
            dict(obj_size=size, n_objs=n, stride=st))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
