#!/usr/bin/env python3
"""Rate and ratios of the dedup-then-compress add (Reducer)
against the two calls a user runs today to approximate its figure,
LzMeasure.add_stream plus Measure.add_stream over the same bytes; one GPU, one
process.

  (a) 8 GiB as 1024 x 8 MiB, controlled d1 c1 and d4 c2 and DG1 d3 c2, at 4 KiB
      and 64 KiB blocks: after the warm-up adds, the timed adds of the two
      sides alternate (reducer, then lz + measure, ...), each between HIP
      events, the handles reset outside the events; medians in ms and GB/s.
      Then the three ratios of the result beside the product of the two
      existing handles' ratios.
  (b) BASELINE config 4's objects (10 000 log-uniform sizes, 4 KiB..64 MiB,
      d2 c1.5, as bench.py --config 4 lays them out) through add_batch: the
      ratios, and one timed add of each side.
  (c) growth at 2^21 blocks: a handle that holds 2^21 distinct 4 KiB blocks of
      keystream takes one more block.  That add waits, doubles the kept array
      (32 MiB copied) and rebuilds the table (2^22 to 2^23 slots); its host time
      beside the same add once more, which grows nothing.

    timeout -k 10 900 python tools/reduce_rate.py [--cases abc] [--log FILE]
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
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def compare(total, bb, add):
        """add(handle) enqueues the payload; the two sides alternate."""
        with ctx.reducer(bb) as r, ctx.lz_measurer(bb) as z, ctx.measurer(bb) as m:
            new, old = [], []
            for k in range(a.warmup + a.reps):
                r.reset(), z.reset(), m.reset()
                t_new = once(lambda: add(r))
                t_old = once(lambda: (add(z), add(m)))
                if k >= a.warmup:
                    new.append(t_new)
                    old.append(t_old)
            rr, zr, mr = r.result(), z.result(), m.result()
        mn, mo = statistics.median(new), statistics.median(old)
        say(f"  block_bytes {bb:5d}: reducer add median {mn:9.3f} ms {total / (mn * 1e6):8.1f} GB/s "
            f"(min {min(new):.3f} max {max(new):.3f})   lz add + measure add median {mo:9.3f} ms "
            f"{total / (mo * 1e6):8.1f} GB/s (min {min(old):.3f} max {max(old):.3f})   old / new = {mo / mn:.3f}")
        assert rr.unique_blocks == mr.unique_blocks and (rr.bytes, rr.blocks) == (zr.bytes, zr.blocks)
        product = (mr.blocks / mr.unique_blocks) * zr.ratio
        say(f"                     blocks {rr.blocks} unique {rr.unique_blocks}  dedup_ratio {rr.dedup_ratio:.4f}  "
            f"compress_ratio {rr.compress_ratio:.4f}  reduction_ratio {rr.reduction_ratio:.4f}   "
            f"product of the two handles' ratios {product:.4f} ({(product / rr.reduction_ratio - 1) * 100:+.2f} %)")

    say(f"reduce_rate: {a.reps} timed after {a.warmup} warm-up, digest {lib.s3dg_build_digest().decode()}, "
        f"{torch.cuda.get_device_name(0)}")
    if "a" in a.cases:
        total = a.gib << 30
        buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        shape = dict(obj_size=8 * MiB, n_objs=total // (8 * MiB))
        for name, fill, knobs in (("controlled d1 c1", ctx.fill_stream, dict(dedup=1, compress=1)),
                                  ("controlled d4 c2", ctx.fill_stream, dict(dedup=4, compress=2)),
                                  ("DG1 d3 c2", ctx.dgen_fill_stream, dict(dedup=3, compress=2))):
            fill(buf, **shape, seed_base=SEED, **knobs)
            torch.cuda.synchronize()
            say(f"(a) {name}, {shape['n_objs']} x 8 MiB")
            for bb in (4096, 65536):
                compare(total, bb, lambda h: h.add_stream(buf, **shape))
        del buf
        torch.cuda.empty_cache()
    if "b" in a.cases:
        from bench import log_uniform_sizes
        sizes, offs, cur = log_uniform_sizes(10000), [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 4095) // 4096 * 4096
        buf = torch.empty(cur, dtype=torch.uint8, device="cuda:0")
        ctx.fill_batch(buf, [(o, sz, S.object_entropy(SEED, k), 2, (3, 2)) for k, (o, sz) in enumerate(zip(offs, sizes))])
        torch.cuda.synchronize()
        import numpy as np
        spans = np.array(list(zip(offs, sizes)), np.uint64)
        say(f"(b) config 4: {len(sizes)} objects, {sum(sizes) / 2**30:.2f} GiB, dedup 2 compress (3, 2), add_batch")
        for bb in (4096, 65536):
            compare(sum(sizes), bb, lambda h: h.add_batch(buf, spans))
        del buf
        torch.cuda.empty_cache()
    if "c" in a.cases:
        n = 1 << 21
        buf = torch.empty(n * 4096, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(buf, n * 4096, chunk_bytes=2 * MiB, seed_base=9)
        one = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        with ctx.reducer(4096) as r:
            r.add(buf)
            assert r.result().unique_blocks == n
            ms = []
            for _ in range(2):               # the first grows the arrays, the second does not
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.add(one)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            assert r.result().unique_blocks == n + 1
        say(f"(c) one more block at 2^21 distinct blocks: {ms[0]:.3f} ms with the kept array's copy and the table's "
            f"rebuild (2^22 to 2^23 slots), {ms[1]:.3f} ms without")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
