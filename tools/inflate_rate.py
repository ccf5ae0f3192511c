#!/usr/bin/env python3
"""Rates of Context.npz_zunpack_batch, one GPU, one process.
No threshold: every figure is printed beside its yardsticks from the same run,
on the same arrays:

    host path          the compressed bytes copied to pinned memory, zlib.decompress
                       on 16 threads, the result copied back (host clock)
    npz_unpack_batch   the same arrays in stored archives (host clock)

Arrays: the library's controlled payloads d1 c2 and d4 c2 and keystream bytes
(which deflate to stored blocks), 64 KiB each, one array per archive, written by
zipfile at zlib level 6.  64 distinct archives per kind are written on the host
and laid out 1024 and 65 536 times in device memory, every copy at its own
address.  Last, one archive holding a single 256 MiB d1 c2 member: one wave.

The calls are synchronous and are timed with the host clock; the sides
alternate; after the warm-up calls the medians of the timed ones are printed
with the library digest.  Before anything is timed the unpacked bytes are
compared with the arrays.

    timeout -k 10 900 python tools/inflate_rate.py [--log FILE] [--big-mib 256]
Tooling only: nothing in the product imports this."""
import argparse
import io
import os
import statistics
import sys
import time
import zipfile
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KiB, MiB = 1 << 10, 1 << 20
SEED = 0x5EED000000000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-mib", type=int, default=256)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def up16(v):
        return (v + 15) // 16 * 16

    def payload(kind, nbytes):
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        if kind == "keystream":
            ctx.xoshiro_fill(t, seed_base=SEED)
        else:
            ctx.fill_controlled(t, nbytes, dedup=int(kind[1]), compress=2, entropy=SEED)
        return t.cpu().numpy()

    def archive(arr, method):
        bio = io.BytesIO()
        with zipfile.ZipFile(bio, "w", method, compresslevel=6) as zf:
            with zf.open("x.npy", "w") as f:
                np.lib.format.write_array(f, arr)
        return bio.getvalue()

    def layout(blobs, n):
        """n archives, copy k of blobs[k % len] at a multiple of 16: (device bytes, spans)."""
        spans, at = [], 0
        for k in range(n):
            spans.append((at, len(blobs[k % len(blobs)])))
            at += up16(spans[-1][1])
        host = np.empty(at, np.uint8)
        for (o, b), k in zip(spans, range(n)):
            host[o:o + b] = np.frombuffer(blobs[k % len(blobs)], np.uint8)
        return torch.from_numpy(host).cuda(), spans, host

    def measure(name, sides, total):
        ms = {k: [] for k in sides}
        for r in range(a.warmup + a.reps):
            for k, fn in sides.items():
                t = clock(fn)
                if r >= a.warmup:
                    ms[k].append(t)
        med = {}
        for k, v in ms.items():
            med[k] = statistics.median(v)
            say(f"  {k:34s} median {med[k]:10.3f} ms  {total / (med[k] * 1e6):8.2f} GB/s of arrays   (min {min(v):.3f} max {max(v):.3f}, {len(v)} timed)")
        z = med["npz_zunpack_batch"]
        say(f"  {name}: zunpack is {med['host zlib, 16 threads'] / z:.2f}x the host path's rate and {med['npz_unpack_batch (stored)'] / z:.3f}x the stored unpack's")

    def case(kind, n, member):
        arrs = [payload(kind, 64 * member)[i * member:(i + 1) * member] for i in range(64)]
        zb, sb = [archive(x, zipfile.ZIP_DEFLATED) for x in arrs], [archive(x, zipfile.ZIP_STORED) for x in arrs]
        zsrc, zspans, zhost = layout(zb, n)
        ssrc, sspans, _ = layout(sb, n)
        ztab, stab = (torch.empty(32 * n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        zw = ctx.npz_zindex_batch(zsrc, [(o, b, 32 * k, 1) for k, (o, b) in enumerate(zspans)], ztab)
        sw = ctx.npz_index_batch(ssrc, [(o, b, 32 * k, 1) for k, (o, b) in enumerate(sspans)], stab)
        assert all(w.ok for w in zw) and all(w.ok for w in sw)
        place, file_bytes = up16(zw[0].packed_bytes), zw[0].payload_bytes
        zdst = torch.empty(place * n, dtype=torch.uint8, device="cuda:0")
        sdst = torch.empty(up16(member) * n, dtype=torch.uint8, device="cuda:0")
        ztakes = [(o, b, 32 * k, 0, 1, place * k, place) for k, (o, b) in enumerate(zspans)]
        stakes = [(o, b, 32 * k, 0, 1, up16(member) * k, up16(member)) for k, (o, b) in enumerate(sspans)]
        res = ctx.npz_zunpack_batch(zsrc, ztab, zdst, ztakes, per_take=False)
        assert res.ok and res.bytes == file_bytes * n, res
        got = zdst.cpu().numpy().reshape(n, place)
        for k in (0, 1, 63, 64, n - 1):
            assert np.array_equal(got[k, file_bytes - member:file_bytes], arrs[k % 64]), k
        ents = S.npz_zentries(ztab, 0, n)
        pinned_in = torch.empty(zhost.size, dtype=torch.uint8).pin_memory()
        pinned_out = torch.empty(place * n, dtype=torch.uint8).pin_memory()
        pool = ThreadPoolExecutor(16)

        def host_path():
            pinned_in.copy_(zsrc)
            torch.cuda.synchronize()
            raw, out = pinned_in.numpy(), pinned_out.numpy()

            def one(k):
                o, e = zspans[k][0] + ents[k].data_off, ents[k]
                d = zlib.decompress(raw[o:o + e.csize].tobytes(), -15)
                out[place * k:place * k + len(d)] = np.frombuffer(d, np.uint8)
            list(pool.map(lambda lo: [one(k) for k in range(lo, min(n, lo + 256))], range(0, n, 256)))
            zdst.copy_(pinned_out)

        comp = sum(e.csize for e in ents)
        say(f"{kind}: {n} archives of one {member // KiB} KiB array, compressed to {comp / (member * n):.3f} of the arrays")
        measure(f"{kind} x {n}", {"npz_zunpack_batch": lambda: ctx.npz_zunpack_batch(zsrc, ztab, zdst, ztakes, per_take=False),
                                  "host zlib, 16 threads": host_path,
                                  "npz_unpack_batch (stored)": lambda: ctx.npz_unpack_batch(ssrc, stab, sdst, stakes, per_take=False)},
                member * n)
        pool.shutdown()

    say(f"library digest {lib.s3dg_build_digest().decode()}  device {torch.cuda.get_device_name(0)}")
    for kind in ("d1c2", "d4c2", "keystream"):
        for n in (1024, 65536):
            case(kind, n, 64 * KiB)
    if a.big_mib:
        big = payload("d1c2", a.big_mib * MiB)
        blob = archive(big, zipfile.ZIP_DEFLATED)
        src, spans, _ = layout([blob], 1)
        tab = torch.empty(32, dtype=torch.uint8, device="cuda:0")
        w = ctx.npz_zindex_batch(src, [(0, len(blob), 0, 1)], tab)[0]
        dst = torch.empty(up16(w.packed_bytes), dtype=torch.uint8, device="cuda:0")
        take = [(0, len(blob), 0, 0, 1, 0, dst.numel())]
        ms = [clock(lambda: ctx.npz_zunpack_batch(src, tab, dst, take, per_take=False)) for _ in range(3)]
        assert np.array_equal(dst.cpu().numpy()[w.payload_bytes - big.size:w.payload_bytes], big)
        t0 = time.perf_counter()
        zlib.decompress(blob[S.npz_zentries(tab, 0, 1)[0].data_off:], -15)
        host_ms = (time.perf_counter() - t0) * 1e3
        m = statistics.median(ms)
        say(f"one archive of one {a.big_mib} MiB d1c2 member (one wave, CRC pass included): median {m:.1f} ms, {big.size / (m * 1e6):.3f} GB/s; "
            f"one host thread's zlib.decompress of it: {host_ms:.1f} ms ({m / host_ms:.1f}x faster than the wave)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
