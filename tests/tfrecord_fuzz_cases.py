"""Seeded random cases for the TFRecord calls (tfrecord_frame_batch,
tfrecord_frame_var_batch, tfrecord_index_batch, tfrecord_scan and the two
checks), and the arena the GPU tests of these calls
share.  No torch, no GPU: tests/test_tfrecord_fuzz_cpu.py holds the draws of
SEEDS to a written checklist; tests/test_gpu_tfrecord_fuzz.py runs them on a
device; tests/test_gpu_tfrecord_pipeline.py lays its lists out with Arena.
Not a conftest.

A case is about 5000 record lengths of a mixture that brings zero-length
records, records below one piece, one-region records on every row edge,
records on both sides of a region edge and records of many regions next to
each other, cut into shards at random places.  Beside these stand empty
shards, a shard of zero-length records only, shards of equal lengths (which
can go through the uniform call) and a twin that frames another shard's
source once more.  The shards are dealt to three to five calls, each uniform
or var, in a drawn order; a list of one-bit flips for the checks and a list of
spans cut short or extended for the walks complete the case.

The judges are tests/tfrecord_var_restatement.py's: Arena frames every shard
with J.frame_np.
"""
from __future__ import annotations

import dataclasses
import math
import random

import numpy as np

import tfrecord_var_restatement as J

KiB, MiB = 1 << 10, 1 << 20
POISON = 0xA5
SEEDS = (1, 2, 3, 4, 5, 6)          # the seeds the suites run (times S3DG_FUZZ_SOAK on the device)
SALT = 0x7F4EC000                   # draw(seed) reads random.Random(SALT + seed) and nothing else
RECORDS = 5000
MAX_SHARDS = 40
REGION_ROWS = 32                    # the region every call of a case has
ROWS_LIMIT = 33 * 4096              # whole rows in a call at which its region stops being 32 rows
REGION_DELTAS = (-1025, -1024, -17, -16, -15, -1, 0, 1, 15, 16, 17, 1024, 1025)


def up16(n):
    return (n + 15) // 16 * 16


def regions(n, rows=REGION_ROWS):
    """Regions of a record of n bytes at a call region of `rows` rows."""
    return max(1, -(-((n + 15) // KiB) // rows))


def length(rnd):
    k = rnd.random()
    if k < 0.15:
        return 0
    if k < 0.30:
        return rnd.randint(1, 15)
    if k < 0.62:
        return int(math.exp(rnd.uniform(math.log(16), math.log(4097))))
    if k < 0.80:
        return rnd.randint(1, 31) * KiB + rnd.randint(-17, 17)
    if k < 0.978:
        return rnd.randint(1, 3) * 32 * KiB + rnd.choice(REGION_DELTAS)
    if k < 0.998:
        return rnd.randint(100 * KiB, 300 * KiB)
    return rnd.randint(MiB, 3 * MiB)


class Arena:
    """lists: the lengths of each shard; twins: {k: j} makes shard k frame the
    source of shard j again (equal lengths).  Shards are laid out in the given
    order with gaps of 16-48 bytes in source, destination and index arenas, as
    the Case of tests/test_gpu_tfrecord_var.py does; src, dst and idx are what
    the judge expects after every shard is framed with an index."""

    def __init__(self, lists, seed, first=16, twins=None, build=True):
        rng = random.Random(seed)
        twins = twins or {}
        so = do = io = first
        self.seed, self.twins, self.shards = seed, twins, []
        for k, sh in enumerate(lists):
            l = np.asarray(sh, dtype=np.uint64).reshape(-1)
            pay = int(l.sum())
            if k in twins:
                assert twins[k] < k and np.array_equal(l, self.shards[twins[k]][2])
                s_off = self.shards[twins[k]][0]
            else:
                s_off = so
                so += up16(pay) + rng.choice((16, 32, 48))
            self.shards.append((s_off, do, l, io))
            do += up16(pay + 16 * len(l)) + rng.choice((16, 32, 48))
            io += 16 * len(l) + rng.choice((16, 32, 48))
        self.sizes = (so, do, io)
        self.src = self.dst = self.idx = None
        if build:
            self.build()

    def build(self):
        if self.src is not None:
            return self
        so, do, io = self.sizes
        nrng = np.random.default_rng(self.seed)
        self.src = np.full(so, POISON, np.uint8)
        self.dst = np.full(do, POISON, np.uint8)
        self.idx = np.full(io, POISON, np.uint8)
        for k, (s_off, d_off, l, i_off) in enumerate(self.shards):
            pay = int(l.sum())
            if k not in self.twins and pay:
                words = nrng.integers(0, 2**63, (pay + 7) // 8, dtype=np.int64)
                self.src[s_off:s_off + pay] = words.view(np.uint8)[:pay]
            if len(l):
                st, ix = J.frame_np(self.src[s_off:s_off + pay].tobytes(), l.tolist())
                self.dst[d_off:d_off + len(st)] = st
                self.idx[i_off:i_off + len(ix)] = ix
        return self

    def framed(self, k):
        l = self.shards[k][2]
        return int(l.sum()) + 16 * len(l)

    def is_uniform(self, k):
        l = self.shards[k][2]
        return len(l) == 0 or bool((l == l[0]).all())

    def var(self, ks):
        """The shards ks as tfrecord_frame_var_batch takes them."""
        return [self.shards[k] for k in ks]

    def uniform(self, ks):
        """The shards ks, all of equal lengths, as tfrecord_frame_batch takes them."""
        out = []
        for k in ks:
            s, d, l, i = self.shards[k]
            assert self.is_uniform(k)
            out.append((s, d, len(l), int(l[0]) if len(l) else 0, i))
        return out

    def spans(self, ks, delta=None):
        """The framed streams of the shards ks as tfrecord_index_batch takes
        them: (off, nbytes, idx_off, max_records), nbytes changed by delta[k]."""
        delta = delta or {}
        return [(self.shards[k][1], self.framed(k) + delta.get(k, 0), self.shards[k][3], len(self.shards[k][2])) for k in ks]

    def record_at(self, pos):
        """(shard, record) whose framed bytes hold destination byte `pos`, or
        (shard, None) in the gap behind a shard, or (None, None) before the first."""
        found = None
        for k, (_, d_off, _, _) in enumerate(self.shards):
            if d_off <= pos and (found is None or d_off >= self.shards[found][1]):
                found = k
        if found is None:
            return None, None
        l = self.shards[found][2]
        starts = np.concatenate(([0], np.cumsum(l + np.uint64(16)))).astype(np.int64)
        rel = pos - self.shards[found][1]
        if rel >= int(starts[-1]):
            return found, None
        return found, int(np.searchsorted(starts, rel, side="right")) - 1

    def index_owner(self, pos):
        """(shard, record) whose index entry holds index byte `pos`, as record_at."""
        found = None
        for k, (_, _, _, i_off) in enumerate(self.shards):
            if i_off <= pos and (found is None or i_off >= self.shards[found][3]):
                found = k
        if found is None:
            return None, None
        rec = (pos - self.shards[found][3]) // 16
        return found, rec if rec < len(self.shards[found][2]) else None


@dataclasses.dataclass
class Case:
    seed: int
    lists: list                 # one uint64 array of lengths per shard, in the arena's order
    twins: dict                 # {shard: the earlier shard whose source it frames again}
    calls: list                 # (kind, [shard, ...]) in the order they are enqueued; kind "uniform" | "var"
    flips: list                 # (shard, record, byte of the framed record, bit, class 0 length | 1 length CRC | 2 data CRC)
    deltas: dict                # {shard: bytes added to (> 0) or cut from (< 0) its span for the second walk}
    arena: Arena = None

    def layout(self, build=True):
        if self.arena is None:
            self.arena = Arena(self.lists, SALT + self.seed, twins=self.twins, build=False)
        return self.arena.build() if build else self.arena

    def describe(self) -> str:
        a = self.layout(build=False)
        lines = [f"tfrecord fuzz seed {self.seed}: {len(self.lists)} shards, {sum(len(l) for l in self.lists)} records, "
                 f"arenas {a.sizes} B, {sum(regions(int(n)) for l in self.lists for n in l)} regions"]
        for k, (s, d, l, i) in enumerate(a.shards):
            kind = "empty" if not len(l) else "equal" if a.is_uniform(k) else "mixed"
            twin = f" twin of {self.twins[k]}" if k in self.twins else ""
            lines.append(f"  shard {k}: src {s} dst {d} idx {i}, {len(l)} records of {int(l.sum())} B ({kind}{twin}), "
                         f"longest {int(l.max()) if len(l) else 0}, {sum(regions(int(n)) > 1 for n in l)} of several regions")
        for c, (kind, ks) in enumerate(self.calls):
            lines.append(f"  call {c}: {kind} {ks}")
        for k, i, off, bit, cls in self.flips:
            lines.append(f"  flip: shard {k} record {i} byte {off} of {16 + int(self.lists[k][i])} ^= {1 << bit:#04x} "
                         f"[{('length', 'length CRC', 'data CRC')[cls]}]")
        lines.append(f"  walk spans changed by: {self.deltas}")
        return "\n".join(lines)


def flip_class(off):
    """The class a one-bit flip at byte `off` of a framed record falls in: the
    length field, its CRC, or the data with its footer."""
    return 0 if off < 8 else 1 if off < 12 else 2


def draw(seed: int) -> Case:
    rnd = random.Random(SALT + seed)
    lens = [length(rnd) for _ in range(RECORDS)]
    pieces = rnd.randint(5, 28)
    cuts = [0] + sorted(rnd.sample(range(1, RECORDS), pieces - 1)) + [RECORDS]
    shards = [("cut", lens[a:b]) for a, b in zip(cuts, cuts[1:])]
    shards += [("empty", []) for _ in range(rnd.randint(1, 3))]
    shards.append(("zeros", [0] * rnd.randint(1, 9)))
    for _ in range(rnd.randint(2, 5)):
        rs = 0
        while not 0 < rs <= 40 * KiB:
            rs = length(rnd)
        shards.append(("equal", [rs] * rnd.randint(1, max(1, min(60, MiB // rs)))))
    rnd.shuffle(shards)
    for edge in (0, -1):                            # the arena's order begins and ends with records: the empty shards lie inside
        if not shards[edge][1]:
            j = rnd.choice([j for j in range(1, len(shards) - 1) if shards[j][1]])
            shards[edge], shards[j] = shards[j], shards[edge]
    # the twin: behind its source; a small one, so that the call's whole rows stay the mixture's
    small = [k for k, (_, l) in enumerate(shards) if l and sum(n // KiB for n in l) <= 4096]
    src = rnd.choice(small) if small else min((k for k, (_, l) in enumerate(shards) if l), key=lambda k: sum(shards[k][1]))
    at = rnd.randint(src + 1, len(shards))
    shards.insert(at, ("twin", list(shards[src][1])))
    twins = {at: src}
    assert len(shards) <= MAX_SHARDS
    lists = [np.array(l, dtype=np.uint64) for _, l in shards]

    # the split: one or two uniform calls, the rest var; every call holds a shard with records
    equal = [k for k, (tag, l) in enumerate(shards) if tag in ("equal", "zeros")]
    rnd.shuffle(equal)
    ncalls = rnd.randint(3, 5)
    nuni = rnd.randint(1, 2)
    lead_u = equal[:nuni]
    rest = [k for k in range(len(shards)) if k not in lead_u]
    live = [k for k in rest if shards[k][1] and shards[k][0] not in ("equal", "zeros")]
    rnd.shuffle(live)
    nvar = ncalls - nuni
    lead_v = live[:nvar]
    groups = [("uniform", [k]) for k in lead_u] + [("var", [k]) for k in lead_v]
    for k in rest:
        if k in lead_v:
            continue
        fits = [g for g in groups if g[0] == "var" or not shards[k][1] or shards[k][0] in ("equal", "zeros")]
        rnd.choice(fits)[1].append(k)
    # the var call with the most shards with records holds an empty one: it can lie between two of them
    most = max((g for g in groups if g[0] == "var"), key=lambda g: sum(1 for k in g[1] if shards[k][1]))
    if all(shards[k][1] for k in most[1]):
        k = next(k for k in range(len(shards)) if not shards[k][1])
        for _, ks in groups:
            if k in ks:
                ks.remove(k)
        most[1].append(k)
    for _, ks in groups:
        rnd.shuffle(ks)
        # an empty shard at either end of a call's list goes between two shards with records
        lo = next(j for j, k in enumerate(ks) if shards[k][1])
        hi = max(j for j, k in enumerate(ks) if shards[k][1])
        if lo < hi:
            ends = [k for j, k in enumerate(ks) if not lo < j < hi and not shards[k][1]]
            inner = [k for k in ks if k not in ends]
            for k in ends:
                inner.insert(rnd.randint(1, len(inner) - 1), k)
            ks[:] = inner
    rnd.shuffle(groups)

    flips, seen = [], set()
    for k, l in enumerate(lists):
        for _ in range(min(len(l), 6)):
            i = rnd.randrange(len(l))
            off, bit = rnd.randrange(16 + int(l[i])), rnd.randrange(8)
            if (k, i, off) not in seen:                # one flip per byte: a second could undo it
                seen.add((k, i, off))
                flips.append((k, i, off, bit, flip_class(off)))
    with_records = [k for k, l in enumerate(lists) if len(l)]
    deltas = {k: -min(rnd.randint(1, 19), int(lists[k].sum()) + 16 * len(lists[k]))
              for k in rnd.sample(with_records, min(4, len(with_records)))}
    for k in rnd.sample(range(len(lists)), 4):
        deltas.setdefault(k, rnd.randint(1, 11))
    return Case(seed, lists, twins, groups, flips, deltas)
