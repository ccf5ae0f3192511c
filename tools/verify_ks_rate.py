#!/usr/bin/env python3
"""Rate of the keystream verify calls against the fills of the same layouts
over the same bytes, one GPU (the sibling of tools/verify_rate.py, which does
this for the 4 KiB-block layouts).

Three cases, 8 GiB each (far beyond the L2 and the Infinity Cache):
  K2       xoshiro_fill / verify_xoshiro, 2 MiB chunks
  DG1 c1   dgen_fill_stream / verify_dgen_stream, 8 x 1 GiB objects, compress 1
  DG1 c2   the same at compress 2 (zero prefixes: all-zero waves, and on the
           fill side the zero prefix + tail split)
For each case the buffer is filled once and checked (clean; a wrong seed
mismatches every 4 KiB granule outside the zero prefixes).  Then, after 5 warm-up launches each, 20
verify calls and 20 fills of the same shape are timed with HIP events in this
process, and the medians printed in GB/s with their ratio (verify / fill) and
the library digest.  The verify is a read-only pass and the fill a write-only
pass over the same bytes with the same generator, so the ratio is the number to
quote: the yardstick of a layout is its own fill in the same run.  A verify
call is synchronous: its events bracket the record reset, the kernel and the
24-byte copy back.

    python tools/verify_ks_rate.py [--gib 8] [--log FILE]
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
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    total = a.gib << 30
    seed = 0x5EED000000000001
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
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

    say(f"verify_ks_rate: {a.gib} GiB per case, {a.reps} timed after {a.warmup} warm-up, "
        f"digest {lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    n_objs = 8
    osz = total // n_objs
    # (name, fill, verify, granules a wrong seed changes: all but those inside zero prefixes)
    cases = [("K2 2 MiB chunks", total // 4096,
              lambda s=seed: ctx.xoshiro_fill(buf, total, chunk_bytes=2 * MiB, seed_base=s),
              lambda s=seed: ctx.verify_xoshiro(buf, total, chunk_bytes=2 * MiB, seed_base=s))]
    for c in (1, 2):
        tail = MiB - MiB * (c - 1) // c          # a block's bytes past its zero prefix (whole granules for c = 1, 2)
        cases.append((f"DG1 c{c} {n_objs} x {osz // MiB} MiB", (total // MiB) * (tail // 4096),
                      lambda s=seed, c=c: ctx.dgen_fill_stream(buf, osz, n_objs, compress=c, seed_base=s),
                      lambda s=seed, c=c: ctx.verify_dgen_stream(buf, osz, n_objs, compress=c, seed_base=s)))
    ratios = []
    for name, nbad, fill, verify in cases:
        fill()
        torch.cuda.synchronize()
        r = verify()
        assert r.ok, (name, r)
        bad = verify(seed + 1)
        assert bad.mismatched_blocks == nbad, (name, bad, nbad)
        say(f"{name}: check clean = {r.ok}; wrong seed: {bad.mismatched_blocks} of {total // 4096} granules "
            f"(all outside zero prefixes), {bad.mismatched_bytes} bytes")
        fm = timed(fill)
        vm = timed(verify)
        assert verify().ok
        for what, (med, lo, hi) in (("fill", fm), ("verify", vm)):
            say(f"  {name:28s} {what:6s} median {med:8.3f} ms  {gbs(med):8.1f} GB/s   (min {lo:.3f} max {hi:.3f} ms)")
        ratios.append((name, gbs(vm[0]) / gbs(fm[0]), gbs(vm[0]), gbs(fm[0])))
    for name, ratio, v, f in ratios:
        say(f"ratio verify / fill  {name:28s} = {ratio:.3f}   (verify {v:.1f} GB/s, fill {f:.1f} GB/s)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
