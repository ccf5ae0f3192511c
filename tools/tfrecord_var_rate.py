#!/usr/bin/env python3
"""Rates of Context.tfrecord_frame_var_batch, tfrecord_check_var_batch and
tfrecord_index_batch, one GPU, one process.  No threshold:
every figure is printed beside what it is measured against, in the same run.

  (e) equal lengths through the var calls against the uniform calls over the
      same bytes: 64 shards of 1 000 records of exactly 128 KiB, and one shard
      of 1 048 576 records of 2 KiB (tools/tfrecord_rate.py's rows b and c).
      The price of the per-record table as a ratio; the host's share is the
      time the frame call takes to return (the checks, the passes over the
      lengths, the table built in pinned memory, the enqueue), printed beside
      the table's bytes and a pinned host-to-device copy of as many bytes.
  (f) 64 shards of 1 000 records, lengths from a normal of mean 128 KiB and
      deviation 32 KiB clipped to >= 1 KiB: against (e)'s equal-length row.
  (g) one shard of 1 048 576 records of log-uniform length 100 B - 4 KiB:
      ns per record.
  (h) the walk: 64 streams of 1 000 records, 1 024 of 1 000, and one stream of
      1 048 576 records (2 KiB each): ns per record per stream; beside it a
      device-to-pinned-host copy of the same streams, the only way to index
      them without the call.

The timed calls go through the C ABI over descriptor arrays built once.  The
sides of a comparison alternate; after the warm-up calls the medians of the
timed ones are printed with the library digest.  The frame forms return
without a wait and are timed with HIP events; the synchronous calls with the
host clock.  A few records of every list are held to a struct + zlib frame
before anything is timed, and every list checks clean.

    timeout -k 10 900 python tools/tfrecord_var_rate.py [--cases efgh] [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import ctypes
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KiB, MiB = 1 << 10, 1 << 20
SEED = 0x5EED000000000001


def masked(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="efgh")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import TfrRec, TfrStream, TfrWalkRec, c_u64, call, lib
    from s3dlio_amd.device import _tfr_shards, _tfr_var_shards

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

    def events(fn, host=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        if host is not None:
            host.append((time.perf_counter() - t0) * 1e3)   # the call has returned; the device still works
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def med(ms):
        return statistics.median(ms), min(ms), max(ms)

    def line(name, ms, total, extra=""):
        m, lo, hi = med(ms)
        say(f"  {name:44s} median {m:10.3f} ms  {total / (m * 1e6):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms, "
            f"{len(ms)} timed){extra}")
        return m

    def layout(lists):
        """Packed shards: payloads, streams and indexes back to back at multiples of 16."""
        so = do = io = 0
        shards = []
        for l in lists:
            pay = int(l.sum())
            shards.append((so, do, l, io))
            so += (pay + 15) // 16 * 16
            do += (pay + 16 * len(l) + 15) // 16 * 16
            io += 16 * len(l)
        return shards, so, do, io

    def setup(lists):
        shards, so, do, io = layout(lists)
        src = torch.empty(so, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        dst = torch.empty(do, dtype=torch.uint8, device="cuda:0")
        idx = torch.empty(io, dtype=torch.uint8, device="cuda:0")
        ctx.tfrecord_frame_var_batch(src, dst, shards, index=idx)
        torch.cuda.synchronize()
        for s_off, d_off, l, i_off in (shards[0], shards[-1]):   # a few records against the definition
            at = pos = 0
            for k in range(min(len(l), 3)):
                n = int(l[k])
                d = src[s_off + at:s_off + at + n].cpu().numpy().tobytes()
                lb = struct.pack("<Q", n)
                want = lb + struct.pack("<I", masked(zlib.crc32(lb))) + d + struct.pack("<I", masked(zlib.crc32(d)))
                assert dst[d_off + pos:d_off + pos + 16 + n].cpu().numpy().tobytes() == want, "stream differs"
                assert idx[i_off + 16 * k:i_off + 16 * k + 16].cpu().numpy().tobytes() == struct.pack("<QQ", pos, 16 + n), "index differs"
                at += n
                pos += 16 + n
        res = ctx.tfrecord_check_var_batch(dst, shards)
        assert res.ok and res.records == sum(len(l) for l in lists), res
        return src, dst, idx, shards, sum(int(l.sum()) for l in lists)

    def var_sides(src, dst, idx, shards):
        arr, n, lens = _tfr_var_shards(shards)[:3]
        s = int(torch.cuda.current_stream().cuda_stream)
        tot = TfrRec()
        ps, pd, pi = src.data_ptr(), dst.data_ptr(), idx.data_ptr()
        pl = lens.ctypes.data_as(ctypes.POINTER(c_u64))
        keep = (arr, lens)
        return (lambda: call("s3dg_tfrecord_frame_var_batch", ctx._h, ps, pd, pi, arr, n, pl, len(lens), s),
                lambda: call("s3dg_tfrecord_check_var_batch", ctx._h, pd, arr, n, pl, len(lens), s, ctypes.byref(tot), None), keep)

    def uni_sides(src, dst, idx, shards):
        arr, n = _tfr_shards(shards)[:2]
        s = int(torch.cuda.current_stream().cuda_stream)
        tot = TfrRec()
        ps, pd, pi = src.data_ptr(), dst.data_ptr(), idx.data_ptr()
        return (lambda: call("s3dg_tfrecord_frame_batch", ctx._h, ps, pd, pi, arr, n, s),
                lambda: call("s3dg_tfrecord_check_batch", ctx._h, pd, arr, n, s, ctypes.byref(tot), None), arr)

    def table_bytes(shards):
        live = sum(1 for s in shards if len(s[2]))
        recs = sum(len(s[2]) for s in shards)
        return 256 + 40 * (live + 1) + 16 * (recs + live)   # short records only: no list of long ones

    def var_only(src, dst, idx, shards, total):
        frame, check, keep = var_sides(src, dst, idx, shards)
        for _ in range(a.warmup):
            frame()
            check()
        tf, tc, th = [], [], []
        for _ in range(a.reps):
            tf.append(events(frame, th))
            tc.append(clock(check))
        n = sum(len(s[2]) for s in shards)
        mf = line("tfrecord_frame_var_batch (device events)", tf, total, f"   {med(tf)[0] * 1e6 / n:.1f} ns per record")
        say(f"    of which the call's host share: median {med(th)[0]:.3f} ms until it returns ({med(th)[0] * 1e6 / n:.1f} ns per record)")
        mc = line("tfrecord_check_var_batch", tc, total, f"   {med(tc)[0] * 1e6 / n:.1f} ns per record")
        return mf, mc

    say(f"tfrecord_var_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")

    equal_b = None
    if "e" in a.cases:
        for tag, nshards, records, rs in (("e1", 64, 1000, 128 * KiB), ("e2", 1, 1 << 20, 2 * KiB)):
            say(f"({tag}) {nshards} shard(s) of {records} records of exactly {rs} B, {nshards * records * rs / 2**30:.2f} GiB of payload: "
                f"var calls against the uniform calls over the same bytes")
            lists = [np.full(records, rs, np.uint64) for _ in range(nshards)]
            src, dst, idx, shards, total = setup(lists)
            uniform = [(s, d, len(l), rs, i) for s, d, l, i in shards]
            u_dst, u_idx = torch.empty_like(dst), torch.empty_like(idx)
            ctx.tfrecord_frame_batch(src, u_dst, uniform, index=u_idx)
            torch.cuda.synchronize()
            assert torch.equal(u_dst, dst) and torch.equal(u_idx, idx), "var and uniform streams differ"
            vf, vc, keep = var_sides(src, dst, idx, shards)
            uf, uc, keep2 = uni_sides(src, u_dst, u_idx, uniform)
            tb = table_bytes(shards)
            pinned = torch.empty(tb, dtype=torch.uint8).pin_memory()
            devtab = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
            for _ in range(a.warmup):
                vf()
                uf()
                vc()
                uc()
            tvf, tuf, tvc, tuc, th, tup = [], [], [], [], [], []
            for _ in range(a.reps):
                tvf.append(events(vf, th))
                tuf.append(events(uf))
                tvc.append(clock(vc))
                tuc.append(clock(uc))
                tup.append(events(lambda: devtab.copy_(pinned, non_blocking=True)))
            n = nshards * records
            mvf = line("tfrecord_frame_var_batch (device events)", tvf, total, f"   {med(tvf)[0] * 1e6 / n:.1f} ns per record")
            muf = line("tfrecord_frame_batch (device events)", tuf, total, f"   {med(tuf)[0] * 1e6 / n:.1f} ns per record")
            mvc = line("tfrecord_check_var_batch", tvc, total, f"   {med(tvc)[0] * 1e6 / n:.1f} ns per record")
            muc = line("tfrecord_check_batch", tuc, total, f"   {med(tuc)[0] * 1e6 / n:.1f} ns per record")
            say(f"  ratio var / uniform (times): frame {mvf / muf:.3f}, check {mvc / muc:.3f}")
            say(f"  host share of the var frame: median {med(th)[0]:.3f} ms until the call returns ({med(th)[0] * 1e6 / n:.1f} ns per record); "
                f"table {tb / MiB:.2f} MiB, a pinned host-to-device copy of as many bytes {med(tup)[0]:.3f} ms (inside the device time above)")
            if tag == "e1":
                equal_b = (mvf, mvc, total)
            del src, dst, idx, u_dst, u_idx, pinned, devtab
            torch.cuda.empty_cache()

    if "f" in a.cases:
        rng = np.random.default_rng(1)
        lists = [np.clip(rng.normal(128 * KiB, 32 * KiB, 1000), KiB, None).astype(np.uint64) for _ in range(64)]
        tot = sum(int(l.sum()) for l in lists)
        say(f"(f) 64 shards of 1000 records, lengths normal(128 KiB, 32 KiB) clipped to >= 1 KiB, {tot / 2**30:.2f} GiB of payload")
        src, dst, idx, shards, total = setup(lists)
        mf, mc = var_only(src, dst, idx, shards, total)
        if equal_b:
            say(f"  against (e1), equal lengths through the same calls (rates): frame {(total / mf) / (equal_b[2] / equal_b[0]):.3f}, "
                f"check {(total / mc) / (equal_b[2] / equal_b[1]):.3f}")
        del src, dst, idx
        torch.cuda.empty_cache()

    if "g" in a.cases:
        rng = np.random.default_rng(2)
        lens = np.floor(np.exp(rng.uniform(np.log(100), np.log(4 * KiB + 1), 1 << 20))).astype(np.uint64)
        say(f"(g) one shard of {1 << 20} records of log-uniform length 100 B - 4 KiB, {int(lens.sum()) / 2**30:.2f} GiB of payload "
            f"(mean {lens.mean():.0f} B)")
        src, dst, idx, shards, total = setup([lens])
        var_only(src, dst, idx, shards, total)
        del src, dst, idx
        torch.cuda.empty_cache()

    if "h" in a.cases:
        rs = 2 * KiB
        for nstreams, records in ((64, 1000), (1024, 1000), (1, 1 << 20)):
            framed = records * (rs + 16)
            say(f"(h) the walk: {nstreams} stream(s) of {records} records of {rs} B, {nstreams * framed / 2**30:.2f} GiB of streams")
            src = torch.empty(nstreams * records * rs, dtype=torch.uint8, device="cuda:0")
            ctx.xoshiro_fill(src, seed_base=SEED)
            dst = torch.empty(nstreams * framed, dtype=torch.uint8, device="cuda:0")
            idx = torch.empty(nstreams * records * 16, dtype=torch.uint8, device="cuda:0")
            widx = torch.zeros_like(idx)
            ctx.tfrecord_frame_batch(src, dst, [(k * records * rs, k * framed, records, rs, k * records * 16) for k in range(nstreams)],
                                     index=idx)
            del src
            walks = ctx.tfrecord_index_batch(dst, [(k * framed, framed, k * records * 16, records) for k in range(nstreams)], widx)
            assert all(w.ok and w.records == records for w in walks) and torch.equal(idx, widx), "walk differs from the frame's index"
            arr = (TfrStream * nstreams)(*[TfrStream(k * framed, framed, k * records * 16, records) for k in range(nstreams)])
            res = (TfrWalkRec * nstreams)()
            s = int(torch.cuda.current_stream().cuda_stream)
            pd, pi = dst.data_ptr(), widx.data_ptr()
            host = torch.empty(nstreams * framed, dtype=torch.uint8).pin_memory()

            def walk():
                call("s3dg_tfrecord_index_batch", ctx._h, pd, pi, arr, nstreams, s, res)

            def copy():
                host.copy_(dst, non_blocking=True)
                torch.cuda.synchronize()
            reps, warm = (a.reps, a.warmup) if records * nstreams < (1 << 20) or nstreams > 1 else (max(3, a.reps // 4), 1)
            for _ in range(warm):
                walk()
                copy()
            tw, tcp = [], []
            for _ in range(reps):
                tw.append(clock(walk))
                tcp.append(clock(copy))
            m = line("tfrecord_index_batch", tw, nstreams * framed,
                     f"   {med(tw)[0] * 1e6 / records:.1f} ns per record per stream, {med(tw)[0] * 1e6 / (records * nstreams):.1f} ns per record overall")
            mc = line("device-to-pinned-host copy of the streams", tcp, nstreams * framed)
            say(f"  ratio copy / walk (times) = {mc / m:.3f}")
            del dst, idx, widx, host
            torch.cuda.empty_cache()

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
