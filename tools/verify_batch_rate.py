#!/usr/bin/env python3
"""Rate of verify_batch (s3dg_verify_controlled_batch) against the calls it
stands beside, over the same bytes, one GPU, one process.

  (a) 1024 x 8 MiB d1 c1 described as a batch: verify_batch against
      verify_stream and fill_batch over the same buffer.  The ratio to
      verify_stream is the figure to quote: the only extra work per workgroup
      is one scalar record load.
  (b) BASELINE config 4's objects (10 000 log-uniform sizes, 4 KiB..64 MiB,
      d2 c1.5, as bench.py --config 4 lays them out in one buffer): verify_batch
      against fill_batch.
  (c) 200 000 objects of 20 KiB + 5 packed at 16 bytes: verify_batch against
      fill_batch (the descriptor path: 13 sub-batches).

Each buffer is filled once with fill_batch and checked clean.  After 5 warm-up
calls, 20 calls of each are timed with HIP events and the medians printed in
GB/s with the library digest.  The descriptor arrays are built once; the timed
calls are the C calls.  A verify call is synchronous: its events bracket the
record resets, the uploads, the kernels and the copy back.  verify_batch is
timed with per-object results (the default) and with totals only.

    timeout -k 10 900 python tools/verify_batch_rate.py [--cases abc] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import ctypes
import os
import statistics
import sys

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
    from s3dlio_amd._lib import ObjDesc, VerifyRec, call, lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def descs(sizes, offs, d, c):
        fn, fd = S.compress_ratio(c)
        arr = (ObjDesc * len(sizes))()
        for k, (o, sz) in enumerate(zip(offs, sizes)):
            arr[k] = ObjDesc(o, sz, S.object_entropy(SEED, k), d, fn, fd)
        return arr

    def run(title, sizes, offs, d, c, stream_kw=None):
        n, total, end = len(sizes), sum(sizes), max(o + s for o, s in zip(offs, sizes))
        say(f"{title}: {n} objects, {total / 2**30:.2f} GiB in a {end / 2**30:.2f} GiB buffer, dedup {d} compress {c}")
        buf = torch.empty(end, dtype=torch.uint8, device="cuda:0")
        arr = descs(sizes, offs, d, c)
        p, h, s = buf.data_ptr(), ctx._h, int(torch.cuda.current_stream().cuda_stream)
        tot, per = VerifyRec(), (VerifyRec * n)()
        call("s3dg_fill_controlled_batch", h, p, arr, n, s)
        torch.cuda.synchronize()
        call("s3dg_verify_controlled_batch", h, p, arr, n, s, ctypes.byref(tot), per)
        assert tot.mismatched_bytes == 0 and per[n - 1].first_offset == 2**64 - 1, tot.mismatched_bytes
        bad = descs(sizes, offs, d, c)
        bad[n // 2].entropy ^= 1
        call("s3dg_verify_controlled_batch", h, p, bad, n, s, ctypes.byref(tot), per)
        assert tot.mismatched_bytes and per[n // 2].mismatched_bytes == tot.mismatched_bytes
        say(f"  check: clean; object {n // 2} described with another entropy: {tot.mismatched_bytes} bytes in "
            f"{tot.mismatched_blocks} blocks, first at {tot.first_offset} (object + {per[n // 2].first_offset})")
        res = {}
        res["fill_batch"] = timed(lambda: call("s3dg_fill_controlled_batch", h, p, arr, n, s))
        res["verify_batch (per object)"] = timed(
            lambda: call("s3dg_verify_controlled_batch", h, p, arr, n, s, ctypes.byref(tot), per))
        res["verify_batch (totals only)"] = timed(
            lambda: call("s3dg_verify_controlled_batch", h, p, arr, n, s, ctypes.byref(tot), None))
        if stream_kw:
            res["verify_stream"] = timed(lambda: ctx.verify_stream(buf, **stream_kw))
            for w in (1, 4):
                ctx.set_waves_per_block(w)
                res[f"verify_batch (per object, {w} waves)"] = timed(
                    lambda: call("s3dg_verify_controlled_batch", h, p, arr, n, s, ctypes.byref(tot), per))
                ctx.set_waves_per_block(0)
        assert tot.mismatched_bytes == 0
        for name, (med, lo, hi) in res.items():
            say(f"  {name:38s} median {med:9.3f} ms  {total / (med * 1e6):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
        v = res["verify_batch (per object)"][0]
        say(f"  ratio verify_batch / fill_batch = {res['fill_batch'][0] / v:.3f}")
        if stream_kw:
            say(f"  ratio verify_batch / verify_stream = {res['verify_stream'][0] / v:.3f}   "
                f"(totals only: {res['verify_stream'][0] / res['verify_batch (totals only)'][0]:.3f})")
        del buf
        torch.cuda.empty_cache()

    say(f"verify_batch_rate: {a.reps} timed after {a.warmup} warm-up, digest {lib.s3dg_build_digest().decode()}, "
        f"{torch.cuda.get_device_name(0)}")
    if "a" in a.cases:
        n, size = 1024, 8 * MiB
        run("(a) 1024 x 8 MiB", [size] * n, [j * size for j in range(n)], 1, 1,
            dict(obj_size=size, n_objs=n, dedup=1, compress=1, seed_base=SEED))
    if "b" in a.cases:
        from bench import log_uniform_sizes
        sizes, offs, cur = log_uniform_sizes(10000), [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 4095) // 4096 * 4096
        run("(b) config 4", sizes, offs, 2, (3, 2))
    if "c" in a.cases:
        n, size = 200000, 20 * 1024 + 5
        st = (size + 15) // 16 * 16
        run("(c) 200 000 x (20 KiB + 5), 16-byte packed", [size] * n, [j * st for j in range(n)], 1, 1)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
