#!/usr/bin/env python3
"""Rates of Context.tfrecord_extract_batch, one GPU, one
process.  No threshold: every figure is printed beside its yardsticks from the
same run, on the same bytes:

    tfrecord_frame_var_batch   moves the same bytes the other way (device events)
    tfrecord_check_var_batch   the read-only half (host clock; synchronous)
    a device-to-device copy    of the payload (device events)

  (a) 64 shards of 1 000 records of 128 KiB, one take per shard
  (b) one shard of 1 048 576 records of 2 KiB, one take
  (c) one shard of 1 048 576 records of log-uniform length 100 B - 4 KiB, one take
  (d) 65 536 shuffled single-record picks of 128 KiB out of (a)'s streams into
      rows of 128 KiB, repeats included

The extract is synchronous and is timed with the host clock, like the check;
beside it the device time of its passes from s3dg_tfrecord_extract_timed (plan,
scan, copy with its fold), whose sum leaves out the upload of the takes and the
results' way back.  The sides alternate; after the warm-up calls the medians
of the timed ones are printed with the library digest.  Before anything is
timed the extract of every list is held to the source it was framed from.

    timeout -k 10 900 python tools/tfrecord_extract_rate.py [--cases abcd] [--log FILE]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import TfrExtractRec, TfrRec, TfrTake, c_u64, call, lib
    from s3dlio_amd.device import _tfr_var_shards

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

    def med(ms):
        return statistics.median(ms)

    def line(name, ms, total, n):
        m = med(ms)
        say(f"  {name:44s} median {m:10.3f} ms  {total / (m * 1e6):8.1f} GB/s   (min {min(ms):.3f} max {max(ms):.3f} ms, "
            f"{len(ms)} timed)   {m * 1e6 / n:.1f} ns per record")
        return m

    def layout(lists):
        so = do = io = 0
        shards = []
        for l in lists:
            pay = int(l.sum())
            shards.append((so, do, l, io))
            so += (pay + 15) // 16 * 16
            do += (pay + 16 * len(l) + 15) // 16 * 16
            io += 16 * len(l)
        return shards, so, do, io

    def extract_sides(dst, idx, out, takes):
        n = len(takes)
        arr = (TfrTake * n)(*[TfrTake(*t) for t in takes])
        s = int(torch.cuda.current_stream().cuda_stream)
        tot = TfrExtractRec()
        ms = (ctypes.c_float * 3)()
        pd, pi, po = dst.data_ptr(), idx.data_ptr(), out.data_ptr()
        return (lambda: call("s3dg_tfrecord_extract_batch", ctx._h, pd, pi, po, arr, n, s, ctypes.byref(tot), None),
                lambda: call("s3dg_tfrecord_extract_timed", ctx._h, pd, pi, po, arr, n, s, ctypes.byref(tot), None, ms), ms, tot)

    def report(tx, passes, total, n, yard):
        mx = line("tfrecord_extract_batch", tx, total, n)
        p = [med([q[i] for q in passes]) for i in range(3)]
        say(f"    its passes on the device (timed form): plan {p[0]:.3f} ms, scan {p[1]:.3f} ms, copy and fold {p[2]:.3f} ms; "
            f"sum {sum(p):.3f} ms, the rest of the call (takes up, results back, the wait) {mx - sum(p):.3f} ms")
        for name, m in yard:
            say(f"    extract / {name} (times) = {mx / m:.3f}; copy pass alone / {name} = {p[2] / m:.3f}")

    def whole(tag, what, lists, keep=False):
        shards, so, do, io = layout(lists)
        n, total = sum(len(l) for l in lists), sum(int(l.sum()) for l in lists)
        say(f"({tag}) {what}, {total / 2**30:.2f} GiB of payload: one take per shard")
        src = torch.empty(so, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        dst = torch.empty(do, dtype=torch.uint8, device="cuda:0")
        idx = torch.empty(io, dtype=torch.uint8, device="cuda:0")
        out = torch.zeros(so, dtype=torch.uint8, device="cuda:0")
        ctx.tfrecord_frame_var_batch(src, dst, shards, index=idx)
        takes = [(d, int(l.sum()) + 16 * len(l), i, 0, len(l), s, int(l.sum())) for s, d, l, i in shards]
        res = ctx.tfrecord_extract_batch(dst, idx, out, takes, per_take=False)
        assert res.ok and res.records == n and res.bytes == total, res
        for s_off, _, l, _ in shards:   # gaps between shards' payloads are not written: compare payloads
            pay = int(l.sum())
            assert torch.equal(out[s_off:s_off + pay], src[s_off:s_off + pay]), "extract differs from the source"
        arr, ns, lens = _tfr_var_shards(shards)[:3]
        s = int(torch.cuda.current_stream().cuda_stream)
        trec = TfrRec()
        ps, pd, pi = src.data_ptr(), dst.data_ptr(), idx.data_ptr()
        pl = lens.ctypes.data_as(ctypes.POINTER(c_u64))
        frame = lambda: call("s3dg_tfrecord_frame_var_batch", ctx._h, ps, pd, pi, arr, ns, pl, len(lens), s)   # noqa: E731
        check = lambda: call("s3dg_tfrecord_check_var_batch", ctx._h, pd, arr, ns, pl, len(lens), s, ctypes.byref(trec), None)   # noqa: E731
        copy = lambda: out.copy_(src, non_blocking=True)   # noqa: E731
        ex, ext, ms, _ = extract_sides(dst, idx, out, takes)
        for _ in range(a.warmup):
            frame(), check(), ex(), ext(), copy()
        tf, tc, tx, tp, passes = [], [], [], [], []
        for _ in range(a.reps):
            tf.append(events(frame))
            tc.append(clock(check))
            tx.append(clock(ex))
            ext()
            passes.append(tuple(ms))
            tp.append(events(copy))
        mf = line("tfrecord_frame_var_batch (device events)", tf, total, n)
        mc = line("tfrecord_check_var_batch", tc, total, n)
        mp = line("device-to-device copy of the payload", tp, total, n)
        report(tx, passes, total, n, (("frame", mf), ("check", mc), ("copy", mp)))
        if keep:
            return src, dst, idx, out, shards, (mf, mc, mp)
        del src, dst, idx, out
        torch.cuda.empty_cache()

    say(f"tfrecord_extract_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    if "a" in a.cases or "d" in a.cases:
        rs, records, nshards = 128 * KiB, 1000, 64
        kept = whole("a", f"{nshards} shards of {records} records of {rs} B", [np.full(records, rs, np.uint64)] * nshards, keep=True)
        if "d" in a.cases:
            src, dst, idx, out, shards, (mf, mc, mp) = kept
            npick = 65536
            say(f"(d) {npick} shuffled single-record picks of {rs} B out of (a)'s streams into rows of {rs} B, "
                f"{npick * rs / 2**30:.2f} GiB of payload; yardsticks: (a)'s, scaled by the bytes")
            rng = np.random.default_rng(4)
            rows = torch.zeros(npick * rs, dtype=torch.uint8, device="cuda:0")
            picks = [(int(k), int(r)) for k, r in zip(rng.integers(0, nshards, npick), rng.integers(0, records, npick))]
            takes = [(shards[k][1], records * (rs + 16), shards[k][3], r, 1, q * rs, rs) for q, (k, r) in enumerate(picks)]
            res = ctx.tfrecord_extract_batch(dst, idx, rows, takes, per_take=False)
            assert res.ok and res.records == npick and res.bytes == npick * rs, res
            for q in (0, 1, npick // 2, npick - 1):
                k, r = picks[q]
                at = shards[k][0] + r * rs
                assert torch.equal(rows[q * rs:(q + 1) * rs], src[at:at + rs]), "pick differs from the source"
            ex, ext, ms, _ = extract_sides(dst, idx, rows, takes)
            for _ in range(a.warmup):
                ex(), ext()
            tx, passes = [], []
            for _ in range(a.reps):
                tx.append(clock(ex))
                ext()
                passes.append(tuple(ms))
            scale = npick * rs / (nshards * records * rs)
            report(tx, passes, npick * rs, npick, (("frame", mf * scale), ("check", mc * scale), ("copy", mp * scale)))
            del rows, src, dst, idx, out
        del kept
        torch.cuda.empty_cache()
    if "b" in a.cases:
        whole("b", f"one shard of {1 << 20} records of {2 * KiB} B", [np.full(1 << 20, 2 * KiB, np.uint64)])
    if "c" in a.cases:
        rng = np.random.default_rng(2)
        lens = np.floor(np.exp(rng.uniform(np.log(100), np.log(4 * KiB + 1), 1 << 20))).astype(np.uint64)
        whole("c", f"one shard of {1 << 20} records of log-uniform length 100 B - 4 KiB (mean {lens.mean():.0f} B)", [lens])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
