#!/usr/bin/env python3
"""Rate of dgen_fill_batch / verify_dgen_batch (s3dg_dgen_fill_batch,
s3dg_verify_dgen_batch) against the calls they stand beside, over the same
bytes, one GPU, one process.

  (1) uniform, 1024 x 8 MiB at d1 c1 and at d2 c2: dgen_fill_batch against
      dgen_fill_stream and verify_dgen_batch against verify_dgen_stream.  At c2
      the stream writes the zero prefixes in a launch of their own
      (k_zero_prefix) and the batch inside its lanes, so a gap is expected.
  (2) BASELINE config 4's objects (10 000 log-uniform sizes, 4 KiB..64 MiB, d2
      c1.5, laid out as bench.py --config 4 does): dgen_fill_batch against one
      dgen_fill per object and against the controlled fill_batch;
      verify_dgen_batch against one verify_dgen per object; then measure_batch
      at 1 MiB and 4 KiB blocks over the result.
  (3) 200 000 objects of 20 KiB + 5 packed at 16 bytes: the batch fill and
      verify, beside the controlled batch on the same list.

Every shape is warmed; device events bracket work that ends in a synchronise;
medians of --reps after --warmup; the two sides of a comparison alternate call
by call; the same stream call timed against itself gives the run's spread.
Every line carries the library's build digest.

    timeout -k 10 900 python tools/dgen_batch_rate.py [--cases 123] [--log FILE]
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
    ap.add_argument("--cases", default="123")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import ObjDesc, VerifyRec, call, lib

    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    dig = lib.s3dg_build_digest().decode()
    lines = []

    def say(s):
        s = f"[{dig}] {s}"
        print(s, flush=True)
        lines.append(s)

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def ab(fns):
        """Medians (ms) of the functions, called in turn."""
        for _ in range(a.warmup):
            for f in fns:
                f()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(a.reps):
            for k, f in enumerate(fns):
                ms[k].append(one(f))
        return [statistics.median(m) for m in ms]

    def descs(sizes, offs, d, c):
        fn, fd = S.compress_ratio(c)
        arr = (ObjDesc * len(sizes))()
        for k, (o, sz) in enumerate(zip(offs, sizes)):
            arr[k] = ObjDesc(o, sz, S.object_entropy(SEED, k), d, fn, fd)
        return arr

    def line(name, ms, total):
        say(f"  {name:44s} median {ms:10.3f} ms  {total / (ms * 1e6):8.1f} GB/s")

    h = ctx._h
    s = int(torch.cuda.current_stream().cuda_stream)
    tot = VerifyRec()

    def check_clean(p, arr, n):
        per = (VerifyRec * n)()
        call("s3dg_verify_dgen_batch", h, p, arr, n, s, ctypes.byref(tot), per)
        assert tot.mismatched_bytes == 0 and per[n - 1].first_offset == 2**64 - 1, tot.mismatched_bytes
        return per

    say(f"dgen_batch_rate: medians of {a.reps} after {a.warmup} warm-up, alternating, {torch.cuda.get_device_name(0)}")

    if "1" in a.cases:
        n, size = 1024, 8 * MiB
        total = n * size
        buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        p = buf.data_ptr()
        for d, c in ((1, 1), (2, 2)):
            say(f"(1) uniform: {n} x 8 MiB, dedup {d} compress {c}")
            fn, fd = S.compress_ratio(c)
            arr = descs([size] * n, [j * size for j in range(n)], d, c)
            per = (VerifyRec * n)()
            f_stream = lambda: call("s3dg_dgen_fill_stream", h, p, size, size, n, d, fn, fd, SEED, 0, s)   # noqa: E731
            f_batch = lambda: call("s3dg_dgen_fill_batch", h, p, arr, n, s)                                 # noqa: E731
            v_stream = lambda: call("s3dg_verify_dgen_stream", h, p, size, size, n, d, fn, fd, SEED, 0, s,  # noqa: E731
                                    ctypes.byref(tot))
            v_batch = lambda: call("s3dg_verify_dgen_batch", h, p, arr, n, s, ctypes.byref(tot), per)       # noqa: E731
            f_stream()
            check_clean(p, arr, n)                    # the stream's bytes are the batch's
            f_batch()
            v_stream()
            assert tot.mismatched_bytes == 0
            fs, fs2 = ab([f_stream, f_stream])
            fb, fs3 = ab([f_batch, f_stream])
            vs, vs2 = ab([v_stream, v_stream])
            vb, vs3 = ab([v_batch, v_stream])
            assert tot.mismatched_bytes == 0
            line("dgen_fill_stream (against itself)", fs, total)
            line("dgen_fill_stream (second side)", fs2, total)
            line("dgen_fill_batch", fb, total)
            line("dgen_fill_stream (beside the batch)", fs3, total)
            say(f"  fill: batch / stream = {fs3 / fb:.4f}; spread (stream / stream) = {fs2 / fs:.4f}")
            # the stream's launch is persistent from 6 rounds of resident waves, the
            # batch's grid is static: the stream on a static grid too
            ctx.set_keystream_persist(0)
            fb4, fs4 = ab([f_batch, f_stream])
            ctx.set_keystream_persist(-1)
            line("dgen_fill_batch (again)", fb4, total)
            line("dgen_fill_stream (static grid)", fs4, total)
            say(f"  fill: batch / stream on a static grid = {fs4 / fb4:.4f}")
            line("verify_dgen_stream (against itself)", vs, total)
            line("verify_dgen_stream (second side)", vs2, total)
            line("verify_dgen_batch (per object)", vb, total)
            line("verify_dgen_stream (beside the batch)", vs3, total)
            say(f"  verify: batch / stream = {vs3 / vb:.4f}; spread (stream / stream) = {vs2 / vs:.4f}")
        del buf
        torch.cuda.empty_cache()

    if "2" in a.cases:
        from bench import log_uniform_sizes
        sizes, offs, cur = log_uniform_sizes(10000), [], 0
        for sz in sizes:
            offs.append(cur)
            cur += (sz + 4095) // 4096 * 4096
        n, total, d, c = len(sizes), sum(sizes), 2, (3, 2)
        fn, fd = S.compress_ratio(c)
        say(f"(2) config 4: {n} objects, {total / 2**30:.2f} GiB in a {cur / 2**30:.2f} GiB buffer, dedup {d} compress 1.5")
        buf = torch.empty(cur, dtype=torch.uint8, device="cuda:0")
        p = buf.data_ptr()
        arr = descs(sizes, offs, d, c)
        per = (VerifyRec * n)()

        def f_each():
            for k in range(n):
                call("s3dg_dgen_fill", h, p + offs[k], sizes[k], 0, 2**64 - 1, d, fn, fd, arr[k].entropy, s)

        def v_each():
            for k in range(n):
                call("s3dg_verify_dgen", h, p + offs[k], sizes[k], 0, 2**64 - 1, d, fn, fd, arr[k].entropy, s,
                     ctypes.byref(tot))
                assert tot.mismatched_bytes == 0

        f_batch = lambda: call("s3dg_dgen_fill_batch", h, p, arr, n, s)                                 # noqa: E731
        f_ctl = lambda: call("s3dg_fill_controlled_batch", h, p, arr, n, s)                             # noqa: E731
        v_batch = lambda: call("s3dg_verify_dgen_batch", h, p, arr, n, s, ctypes.byref(tot), per)       # noqa: E731
        f_each()
        check_clean(p, arr, n)                        # one dgen_fill per object = the batch's bytes
        fb, fe = ab([f_batch, f_each])
        fb2, fc = ab([f_batch, f_ctl])
        f_batch()
        vb, ve = ab([v_batch, v_each])
        line("dgen_fill_batch", fb, total)
        line("one dgen_fill per object", fe, total)
        say(f"  fill: batch / per object = {fe / fb:.3f}")
        line("dgen_fill_batch (beside the controlled batch)", fb2, total)
        line("fill_batch (controlled layout)", fc, total)
        say(f"  fill: DG1 batch / controlled batch = {fc / fb2:.3f}")
        line("verify_dgen_batch (per object)", vb, total)
        line("one verify_dgen per object", ve, total)
        say(f"  verify: batch / per object = {ve / vb:.3f}")
        f_batch()
        spans = [(o, sz) for o, sz in zip(offs, sizes)]
        for bb in (MiB, 4096):
            m = ctx.measure_batch(buf, spans, block_bytes=bb)
            ms = ab([lambda: ctx.measure_batch(buf, spans, block_bytes=bb)])[0]
            line(f"measure_batch at {bb}-byte blocks", ms, total)
            say(f"    dedup_ratio {m.dedup_ratio:.4f}  zero_fraction {m.zero_fraction:.4f}  "
                f"({m.unique_blocks} of {m.blocks} blocks distinct)")
        del buf
        torch.cuda.empty_cache()

    if "3" in a.cases:
        n, size = 200000, 20 * 1024 + 5
        st = (size + 15) // 16 * 16
        total = n * size
        say(f"(3) small objects: {n} x (20 KiB + 5), 16-byte packed, dedup 1 compress 1")
        buf = torch.empty(n * st, dtype=torch.uint8, device="cuda:0")
        p = buf.data_ptr()
        arr = descs([size] * n, [j * st for j in range(n)], 1, 1)
        per = (VerifyRec * n)()
        f_batch = lambda: call("s3dg_dgen_fill_batch", h, p, arr, n, s)                                 # noqa: E731
        f_ctl = lambda: call("s3dg_fill_controlled_batch", h, p, arr, n, s)                             # noqa: E731
        v_batch = lambda: call("s3dg_verify_dgen_batch", h, p, arr, n, s, ctypes.byref(tot), per)       # noqa: E731
        v_ctl = lambda: call("s3dg_verify_controlled_batch", h, p, arr, n, s, ctypes.byref(tot), per)   # noqa: E731
        f_batch()
        check_clean(p, arr, n)
        fb, fc = ab([f_batch, f_ctl])
        f_batch()
        vb = ab([v_batch])[0]
        assert tot.mismatched_bytes == 0
        f_ctl()
        vc = ab([v_ctl])[0]
        assert tot.mismatched_bytes == 0
        line("dgen_fill_batch", fb, total)
        line("fill_batch (controlled layout)", fc, total)
        line("verify_dgen_batch (per object)", vb, total)
        line("verify_batch (controlled layout)", vc, total)
        del buf
        torch.cuda.empty_cache()

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
