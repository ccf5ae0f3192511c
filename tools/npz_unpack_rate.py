#!/usr/bin/env python3
"""Rates of Context.npz_index_batch and Context.npz_unpack_batch (DESIGN.md
§5.5.6), one GPU, one process.  No threshold: every figure is printed beside
its yardsticks from the same run, on the same bytes:

    a device-to-device copy     of the payload (device events)
    npz_check_batch             the read-side twin that needs the descriptors (host clock)
    tfrecord_extract_batch      the same payload sizes framed as one record each,
                                indexed and extracted (host clock)

  (a) 1024 archives of one 8 MiB member
  (b) BASELINE config 4's sizes (10 000 log-uniform, 4 KiB - 64 MiB) as single-member archives
  (c) 65 536 archives of one 128 KiB member
  (d) 65 536 picks of x.npy out of archives of x.npy (4 KiB) and y.npy (8 bytes), into rows
  (e) one archive of 65 534 members of 8 bytes: the serial directory walk (65 535 in the
      end record is the ZIP64 marker, which the walk refuses)

The calls are synchronous and are timed with the host clock, the copy with
device events.  The sides alternate; after the warm-up calls the medians of the
timed ones are printed with the library digest and the unpack's pass_ms.
Before anything is timed the unpacked bytes are compared with the source.

    timeout -k 10 900 python tools/npz_unpack_rate.py [--cases abcde] [--log FILE]
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
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    from s3dlio_amd._lib import c_vp, call, lib
    from s3dlio_amd.device import _npz_archives

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
            f"{len(ms)} timed)   {m * 1e6 / n:.1f} ns per member")
        return m

    def up16(v):
        return (v + 15) // 16 * 16

    def case(tag, what, per_archive, pick=None, tfr=True):
        """per_archive: the member sizes of every archive; pick: the one member to take of each (rows), or None for all."""
        archives, so, do = [], 0, 0
        for sizes in per_archive:
            members = []
            for i, sz in enumerate(sizes):
                members.append((f"m{i}.npy", S.npy_header([sz], "|u1"), so, sz))
                so += up16(sz)
            archives.append((do, members))
            do += up16(S.npz_archive_size(members))
        n, nm = len(archives), sum(len(s) for s in per_archive)
        src = torch.empty(so, dtype=torch.uint8, device="cuda:0")
        ctx.xoshiro_fill(src, seed_base=SEED)
        arc = torch.empty(do, dtype=torch.uint8, device="cuda:0")
        ctx.npz_frame_batch(src, arc, archives)
        cap = max(len(s) for s in per_archive)
        table = torch.empty(32 * cap * n, dtype=torch.uint8, device="cuda:0")
        spans = [(o, S.npz_archive_size(m)) for o, m in archives]
        streams = [(o, b, 32 * cap * k, cap) for k, (o, b) in enumerate(spans)]
        walks = ctx.npz_index_batch(arc, streams, table)
        assert all(w.ok for w in walks), [w for w in walks if not w.ok][:3]
        takes, at = [], 0
        for k, ((o, b), w, sizes) in enumerate(zip(spans, walks, per_archive)):
            first, count, span = (0, w.members, w.packed_bytes) if pick is None else (pick, 1, up16(sizes[pick]))
            takes.append((o, b, 32 * cap * k, first, count, at, span))
            at += span
        total = int(sum(sum(s) if pick is None else s[pick] for s in per_archive))
        taken = nm if pick is None else n
        say(f"({tag}) {what}: {n} archives, {nm} members, {taken} taken, {total / 2**30:.3f} GiB of payload taken, "
            f"{do / 2**30:.3f} GiB of archives")
        dst = torch.empty(max(16, at), dtype=torch.uint8, device="cuda:0")
        res = ctx.npz_unpack_batch(arc, table, dst, takes, per_take=False)
        assert res.ok and res.members == taken and res.bytes == total, res
        if pick is None and all(sz % 16 == 0 for sizes in per_archive for sz in sizes):
            assert torch.equal(dst[:at], src[:at]), "the unpacked bytes differ from the source"   # both sides pack at multiples of 16
        else:
            first = per_archive[0][pick or 0]
            assert torch.equal(dst[:first], src[:first]), "the first unpacked member differs from its source"
        # the descriptors once, the C ABI directly: what is timed is the call, not the wrapper's list handling
        st = int(torch.cuda.current_stream().cuda_stream)
        sarr = (_lib.NpzStream * n)(*[_lib.NpzStream(*s) for s in streams])
        wres = (_lib.NpzWalkRec * n)()
        tarr = (_lib.NpzTake * n)(*[_lib.NpzTake(*t) for t in takes])
        tot, pass_ms = _lib.NpzUnpackRec(), (ctypes.c_float * 3)()
        pa, pt, pd = arc.data_ptr(), table.data_ptr(), dst.data_ptr()
        index = lambda: call("s3dg_npz_index_batch", ctx._h, pa, pt, sarr, n, st, wres)   # noqa: E731
        unpack = lambda: call("s3dg_npz_unpack_timed", ctx._h, pa, pt, pd, tarr, n, st, ctypes.byref(tot), None, pass_ms)   # noqa: E731
        carr, na, marr, nmem, blob = _npz_archives(archives)[:5]
        ctot = _lib.NpzRec()
        check = lambda: call("s3dg_npz_check_batch", ctx._h, pa, carr, na, marr, nmem,   # noqa: E731
                             ctypes.cast(ctypes.c_char_p(blob), c_vp), len(blob), st, ctypes.byref(ctot), None)
        copy = lambda: dst[:min(at, so)].copy_(src[:min(at, so)], non_blocking=True)   # noqa: E731
        sides = [("npz_index_batch (host clock)", index, clock), ("npz_unpack_batch (host clock)", unpack, clock),
                 ("npz_check_batch (host clock)", check, clock), ("device-to-device copy of the payload", copy, events)]
        if tfr:   # the same payload sizes, one record per taken member
            lens = [s for sizes in per_archive for s in (sizes if pick is None else [sizes[pick]])]
            fr = torch.empty(total + 16 * len(lens), dtype=torch.uint8, device="cuda:0")
            idx = torch.empty(16 * len(lens), dtype=torch.uint8, device="cuda:0")
            ctx.tfrecord_frame_var_batch(src, fr, [(0, 0, lens)])
            (w,) = ctx.tfrecord_index_batch(fr, [(0, fr.numel(), 0, len(lens))], idx)
            assert w.ok and w.records == len(lens), w
            xarr = (_lib.TfrTake * 1)(_lib.TfrTake(0, fr.numel(), 0, 0, w.records, 0, w.payload_bytes))
            xtot, xms = _lib.TfrExtractRec(), (ctypes.c_float * 3)()
            pf, pi = fr.data_ptr(), idx.data_ptr()
            sides.append(("tfrecord_extract_batch, a record per member", lambda: call(
                "s3dg_tfrecord_extract_timed", ctx._h, pf, pi, pd, xarr, 1, st, ctypes.byref(xtot), None, xms), clock))
        times = {name: [] for name, _, _ in sides}
        passes, xpasses = [], []
        for r in range(a.warmup + a.reps):
            for name, fn, how in sides:
                t = how(fn)
                if r >= a.warmup:
                    times[name].append(t)
            if r >= a.warmup:
                passes.append(list(pass_ms))
                if tfr:
                    xpasses.append(list(xms))
            assert tot.bad_crc == 0 and tot.status == 0
        med = {name: line(name, ms, total, taken) for name, ms in times.items()}
        pm = [statistics.median(p[i] for p in passes) for i in range(3)]
        say(f"    unpack pass_ms: plan {pm[0]:.3f}, scan {pm[1]:.3f}, copy and fold {pm[2]:.3f}")
        u, c = med["npz_unpack_batch (host clock)"], med["device-to-device copy of the payload"]
        text = f"    unpack / copy = {u / c:.3f}; unpack / check = {u / med['npz_check_batch (host clock)']:.3f}"
        if tfr:
            xm = [statistics.median(p[i] for p in xpasses) for i in range(3)]
            say(f"    extract pass_ms: plan {xm[0]:.3f}, scan {xm[1]:.3f}, copy and fold {xm[2]:.3f}")
            text += f"; unpack / extract = {u / med['tfrecord_extract_batch, a record per member']:.3f}; " \
                    f"copy pass / extract's copy pass = {pm[2] / xm[2]:.3f}"
        say(text)
        del src, arc, dst, table
        torch.cuda.empty_cache()

    say(f"npz_unpack_rate: {a.reps} timed after {a.warmup} warm-up, sides alternating, digest "
        f"{lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    if "a" in a.cases:
        case("a", "one member of 8 MiB", [[8 * MiB]] * 1024)
    if "b" in a.cases:
        from bench import log_uniform_sizes
        case("b", "BASELINE config 4's sizes as single-member archives", [[int(s)] for s in log_uniform_sizes(10000)])
    if "c" in a.cases:
        case("c", "one member of 128 KiB", [[128 * KiB]] * 65536)
    if "d" in a.cases:
        case("d", "picks of one 4 KiB member out of two-member archives into rows", [[4 * KiB, 8]] * 65536, pick=0)
    if "e" in a.cases:
        case("e", "one archive of 65 534 members of 8 bytes", [[8] * 65534], tfr=False)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
