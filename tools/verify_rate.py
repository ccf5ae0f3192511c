#!/usr/bin/env python3
"""Rate of verify_stream against fill_stream over the same bytes, one GPU.

1024 x 8 MiB objects (8 GiB: far beyond the L2 and the Infinity Cache) are
filled once with fill_stream (dedup 1, compress 1 unless given).  After 5
warm-up launches, 20 verify_stream calls and 20 fill_stream launches of the
same shape are timed with HIP events in this process, and the medians
printed in GB/s with their ratio (verify / fill) and the library digest.  The
verify is a read-only pass and the fill a write-only pass over the same bytes
with the same per-block compute, so the ratio is the number to quote.  A
verify call is synchronous: its events bracket the record reset, the kernel
and the 24-byte copy back.

Also printed: the fill through the 2D stream kernel (stream tiles off), which
is the grid shape the verify kernel uses, and the verify at 1, 2 and 4 waves
per block.

    python tools/verify_rate.py [--objects 1024] [--compress 1] [--log FILE]
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
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--obj-mib", type=int, default=8)
    ap.add_argument("--compress", type=int, default=1)
    ap.add_argument("--dedup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    n, size = a.objects, a.obj_mib * MiB
    total = n * size
    seed = 0x5EED000000000001
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    kw = dict(obj_size=size, n_objs=n, dedup=a.dedup, compress=a.compress, seed_base=seed)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps=None, warmup=None):
        for _ in range(a.warmup if warmup is None else warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps if reps is None else reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def gbs(ms):
        return total / (ms * 1e6)

    say(f"verify_rate: {n} x {a.obj_mib} MiB = {total / 2**30:.1f} GiB, dedup {a.dedup} compress {a.compress}, "
        f"{a.reps} timed after {a.warmup} warm-up, digest {lib.s3dg_build_digest().decode()}, "
        f"{torch.cuda.get_device_name(0)}")
    ctx.fill_stream(buf, **kw)
    torch.cuda.synchronize()
    r = ctx.verify_stream(buf, **kw)
    assert r.ok, r
    bad = ctx.verify_stream(buf, **dict(kw, seed_base=seed + 1))
    assert bad.mismatched_blocks == total // 4096, bad       # every block, through the contended atomics
    say(f"check: clean = {r.ok}; wrong seed: {bad.mismatched_blocks} of {total // 4096} blocks, "
        f"{bad.mismatched_bytes} bytes, first at {bad.first_offset}")

    res = {}
    for name, fn in [("fill_stream (default: tiled kernel)", lambda: ctx.fill_stream(buf, **kw)),
                     ("verify_stream (auto: 2 waves)", lambda: ctx.verify_stream(buf, **kw))]:
        res[name] = timed(fn)
    ctx.set_stream_tiles(0)
    res["fill_stream (2D stream kernel)"] = timed(lambda: ctx.fill_stream(buf, **kw))
    ctx.set_stream_tiles(-1)
    for w in (1, 2, 4):
        ctx.set_waves_per_block(w)
        res[f"verify_stream ({w} waves)"] = timed(lambda: ctx.verify_stream(buf, **kw))
    ctx.set_waves_per_block(0)
    # every workgroup adds to the same three words: correct and finite, not fast (3 timed after 1)
    res["verify_stream (wrong seed: every block mismatches)"] = timed(
        lambda: ctx.verify_stream(buf, **dict(kw, seed_base=seed + 1)), 3, 1)
    for name, (med, lo, hi) in res.items():
        say(f"{name:52s} median {med:8.3f} ms  {gbs(med):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
    f = gbs(res["fill_stream (default: tiled kernel)"][0])
    f2 = gbs(res["fill_stream (2D stream kernel)"][0])
    v = gbs(res["verify_stream (auto: 2 waves)"][0])
    say(f"ratio verify / fill = {v / f:.3f}   (verify {v:.1f} GB/s, fill {f:.1f} GB/s); "
        f"against the 2D stream fill {v / f2:.3f}")
    assert ctx.verify_stream(buf, **kw).ok
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
