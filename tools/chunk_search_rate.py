#!/usr/bin/env python3
"""The chunker's cut pass, serial walk beside parallel search,
one GPU, one process, one 8 GiB buffer, one handle per shape at 2048 / 8192 /
65536.  Shapes: DG1 d1 c1 bytes as 8 x 1 GiB, 1 x 8 GiB and 1024 x 8 MiB, zeros
as 8 x 1 GiB, and 1 GiB of byte 57 at 2048 / 64 / 65536 (a run of 57 is a
candidate everywhere at 6 bits and nowhere at 13: over the node bound, so the
search's add walks it serially after deciding so on the device).

Per shape the two walks alternate, add by add, on the same handle (reset before
each add): after the warm-up adds, the cut pass by the handle's own HIP events
(pass_seconds()[1]: everything between the candidate pass and the fingerprints)
and the whole add by HIP events around it; median, min and max over the repeats.
The two results must be equal.

    python tools/chunk_search_rate.py [--log FILE]
Tooling only: nothing in the product imports this."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GiB = 1 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import s3dlio_amd as S
    from s3dlio_amd._lib import lib

    total = a.gib * GiB
    ctx = S.Context(0, base_seed=S.DEFAULT_BASE_SEED)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    H, node_bytes = S.chunks_search_geometry()
    say(f"chunk_search_rate: chunks 2048 / 8192 / 65536, hops of {H} links, {node_bytes} B per node, {a.reps} timed after "
        f"{a.warmup} warm-up per walk, alternating, digest {lib.s3dg_build_digest().decode()}, {torch.cuda.get_device_name(0)}")
    usual = (2048, 8192, 65536)
    shapes = [("random", "8 x 1 GiB", GiB, total // GiB, usual), ("random", "1 x 8 GiB", total, 1, usual),
              ("random", "1024 x 8 MiB", total // 1024, 1024, usual),
              ("zeros", "8 x 1 GiB of zeros", GiB, total // GiB, usual),
              ("57", "1 GiB of byte 57 at 2048 / 64 / 65536 (fallback)", GiB, 1, (2048, 64, 65536))]
    have = None
    for kind, name, size, n, params in shapes:
        if kind != have:
            if kind == "random":
                ctx.dgen_fill_stream(buf, obj_size=GiB, n_objs=total // GiB, seed_base=0x5EED000000000001, dedup=1, compress=1)
            else:
                buf.fill_(0 if kind == "zeros" else 57)
            torch.cuda.synchronize()
            have = kind
        cut = {0: [], 1: []}
        add = {0: [], 1: []}
        res = {}
        with ctx.chunker(*params) as h:
            h.time_passes(True)
            for k in range(a.warmup + a.reps):
                for walk in (0, 1):
                    h.search_walk(walk)
                    h.reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    h.add_stream(buf, size, n)
                    e1.record()
                    e1.synchronize()
                    if k >= a.warmup:
                        cut[walk].append(h.pass_seconds()[1] * 1e3)
                        add[walk].append(e0.elapsed_time(e1))
                    elif k == 0:
                        res[walk] = h.result()
        assert res[0] == res[1], (name, res)
        r = res[0]
        say(f"--- {name}: {r.chunks} chunks, {r.candidates} candidates, {r.forced_cuts} forced cuts, results equal")
        for walk, label in ((0, "serial walk"), (1, "search, threshold 1")):
            c, w = cut[walk], add[walk]
            say(f"{label:20s} cut pass median {statistics.median(c):10.3f} ms (min {min(c):.3f} max {max(c):.3f})   "
                f"whole add median {statistics.median(w):10.3f} ms (min {min(w):.3f} max {max(w):.3f})")
        say(f"cut pass serial / search = {statistics.median(cut[0]) / statistics.median(cut[1]):.1f}   "
            f"whole add serial / search = {statistics.median(add[0]) / statistics.median(add[1]):.2f}")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
