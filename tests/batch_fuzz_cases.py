"""Seeded random cases for the batch loop (fill, verify, measure, checksum of
one descriptor list), and the plain judges of its fill and
verify steps.  No torch, no GPU: tests/test_batch_fuzz_cpu.py holds every draw
valid and the draws of its seeds to a written checklist, and holds
`expected_verify` to hand-computed answers; tests/test_gpu_fuzz_batch.py runs
the cases on a device.  Not a conftest.

A case is one arena: 4 KiB guards at both ends, written objects at multiples
of 16 that do not overlap, the arena's order shuffled against the list's.  An
object's payload is `controlled` (Context.fill_batch writes it), `dg1`
(Context.dgen_fill_batch) or host bytes uploaded with the arena (`random`,
`four_valued`, `zeros`).  Around the write list stand a read list for the
measures and the CRC (the objects, repeats, empty spans, sub-spans, spans over
two objects and the gap between them), one verify list per generated kind
(any order, repeats, in about a third of the cases one descriptor with one
field wrong), corruption (position, XOR mask) and the launch knobs.  Every
fourth seed is uniform instead: one controlled and one DG1 run of equal
objects at a constant stride, seeded object_entropy(seed_base, first_obj + j),
so that the stream calls can be held against the batch calls.

The object bytes of a case sum to at most CAP, which is what keeps the Python
restatements of the measures within seconds; the spans the read list adds to
the objects sum to at most EXTRA.
"""
from __future__ import annotations

import dataclasses
import random
import zlib

import numpy as np

from oracle import oracle_py as P
from test_gpu_chunks import PARAMS as CHUNK_PARAMS

KiB, MiB = 1 << 10, 1 << 20
M64 = (1 << 64) - 1
POISON = 0xA9
GUARD = 4096
CAP = 4 * MiB                      # object bytes per case
EXTRA = 2 * MiB                    # bytes of the read list's own spans per case
MAX_OBJECTS = 48
SEEDS = 24                         # the seeds the suites run (times S3DG_FUZZ_SOAK on the device)
SALT = 0xBA7C4700                 # draw(seed) reads random.Random(SALT + seed) and nothing else

GENERATED = ("controlled", "dg1")
HOST = ("random", "four_valued", "zeros")
KINDS = GENERATED + HOST
DEDUPS = (1, 2, 3, 4, 8, 100)
COMPRESS = (1, 2, 3, 4, 7, 16, (3, 2), (5, 3), (9, 4))
WAVES = (0, 1, 2, 4)
TILES = (0, 2, 4, 8, 16, 32, 64)
MEASURE_BLOCKS = (4096, 8192, 12288, 65536, 69632, MiB)
LZ_BLOCKS = (4096, 12288, 65536)
WRONG_FIELDS = ("entropy", "dedup", "compress", "size")
CORRUPT_MODES = ("first", "last", "ragged", "prefix_end", "edge_4k", "edge_1m", "any")


@dataclasses.dataclass(frozen=True)
class Obj:
    off: int
    size: int
    entropy: int          # controlled: the entropy; dg1: the seed; host kinds: the payload's seed
    dedup: int
    compress: object
    kind: str

    @property
    def desc(self):
        return (self.off, self.size, self.entropy, self.dedup, self.compress)


@dataclasses.dataclass(frozen=True)
class Run:
    """A uniform case's run of equal objects, as the stream calls take it."""
    kind: str
    start: int
    size: int
    n: int
    stride: int
    dedup: int
    compress: object
    seed_base: int
    first_obj: int

    @property
    def spans(self):
        return [(self.start + j * self.stride, self.size) for j in range(self.n)]


@dataclasses.dataclass
class Case:
    seed: int
    uniform: bool
    dense: bool
    shared: bool
    arena: int                                   # bytes, guards included
    writes: list                                 # Obj, in the list's order
    reads: list                                  # (off, size)
    verify: dict                                 # kind -> descriptors (off, size, entropy, dedup, compress)
    wrong: dict                                  # kind -> (index in verify[kind], field) or None
    corrupt: list                                # (absolute offset, mask, index in writes, mode)
    waves: int
    tile: int
    measure_block: int
    hist: bool
    lz_block: int
    chunk_params: tuple
    runs: list = dataclasses.field(default_factory=list)     # Run, uniform cases only
    tags: set = dataclasses.field(default_factory=set)       # what the read list holds, for the checklist

    def of_kind(self, kind):
        return [o for o in self.writes if o.kind == kind]

    def describe(self) -> str:
        lines = [f"batch fuzz seed {self.seed}: {'uniform' if self.uniform else 'mixed'}"
                 f"{' dense' if self.dense else ''}{' shared' if self.shared else ''}, arena {self.arena} B, "
                 f"{len(self.writes)} objects of {sum(o.size for o in self.writes)} B, {len(self.reads)} read spans "
                 f"of {sum(n for _, n in self.reads)} B",
                 f"  knobs: waves_per_block {self.waves}, batch_tile {self.tile}, measure {self.measure_block}"
                 f"{' hist' if self.hist else ''}, lz {self.lz_block}, chunks {self.chunk_params}"]
        for k, o in enumerate(self.writes):
            lines.append(f"  object {k}: {o.kind} off {o.off} size {o.size} entropy {o.entropy:#x} dedup {o.dedup} "
                         f"compress {o.compress}")
        for r in self.runs:
            lines.append(f"  run: {r}")
        for kind in GENERATED:
            lines.append(f"  verify {kind}: {len(self.verify[kind])} descriptors, wrong {self.wrong[kind]}")
            if self.wrong[kind]:
                lines.append(f"    descriptor {self.wrong[kind][0]}: {self.verify[kind][self.wrong[kind][0]]}")
        for pos, mask, k, mode in self.corrupt:
            lines.append(f"  corrupt: offset {pos} (object {k} + {pos - self.writes[k].off}) ^= {mask:#04x} [{mode}]")
        lines.append(f"  reads: {self.reads}")
        return "\n".join(lines)


# ---- drawing -------------------------------------------------------------------------------

def _up(x, m):
    return -(-x // m) * m


def _size(rnd):
    k = rnd.random()
    if k < 0.07:
        return 0
    if k < 0.11:
        return 1
    if k < 0.33:
        return rnd.randint(1, 5000)
    if k < 0.63:
        unit, most = rnd.choice([(4096, 40), (1024, 64), (65536, 12)])
        return rnd.randint(1, most) * unit + rnd.randint(-7, 7)
    if k < 0.80:
        return rnd.randint(1, 2) * MiB + rnd.choice([-17, -1, 0, 1, 17])
    return rnd.randint(1, 5 * MiB // 2)


def _entropy(rnd):
    k = rnd.random()
    if k < 0.08:
        return rnd.randint(0, 3)
    if k < 0.16:
        return M64 - rnd.randint(0, 3)
    return rnd.getrandbits(64)


def _knobs(rnd):
    return dict(waves=rnd.choice(WAVES), tile=rnd.choice(TILES), measure_block=rnd.choice(MEASURE_BLOCKS),
                hist=rnd.random() < 0.5, lz_block=rnd.choice(LZ_BLOCKS), chunk_params=tuple(rnd.choice(CHUNK_PARAMS)))


def _place(rnd, params, dense):
    """Offsets for the objects' parameters (size, entropy, dedup, compress,
    kind), the arena's order shuffled against the list's; and the arena's length."""
    order = list(range(len(params)))
    rnd.shuffle(order)
    offs = [0] * len(params)
    off = GUARD + (4096 * rnd.randint(0, 7) if dense else 16 * rnd.randint(0, 512))
    for k in order:
        offs[k] = off
        if dense:
            off = _up(off + params[k][0], 4096)
        else:
            off = _up(off + params[k][0], 16) + 16 * rnd.randint(1, 512)
    return [Obj(o, *p) for o, p in zip(offs, params)], _up(off, 16) + GUARD


def _prefix_end(o, rnd):
    """An offset on one side of the end of a DG1 block's zero prefix, or None."""
    fn, fd = P.compress_ratio(o.compress)
    if o.kind != "dg1" or fn == 0:
        return None
    i = rnd.randrange(-(-o.size // MiB))
    ln = min(MiB, o.size - i * MiB)
    z = ln * fn // fd
    if not 0 < z < ln:
        return None
    return i * MiB + z - rnd.randint(0, 1)


def _corruption(rnd, writes, count):
    live = [k for k, o in enumerate(writes) if o.kind in GENERATED and o.size]
    out, seen = [], set()
    for _ in range(count if live else 0):
        k = rnd.choice(live)
        o = writes[k]
        mode = rnd.choice(CORRUPT_MODES)
        p = None
        if mode == "first":
            p = 0
        elif mode == "last":
            p = o.size - 1
        elif mode == "ragged" and o.size % 4096:
            p = rnd.randint(o.size - o.size % 4096, o.size - 1)
        elif mode == "prefix_end":
            p = _prefix_end(o, rnd)
        elif mode in ("edge_4k", "edge_1m"):
            unit = 4096 if mode == "edge_4k" else MiB
            if o.size > unit:
                p = rnd.randint(1, (o.size - 1) // unit) * unit - rnd.randint(0, 1)
        if p is None:
            mode, p = "any", rnd.randrange(o.size)
        if o.off + p not in seen:                   # two masks on one byte could cancel
            seen.add(o.off + p)
            out.append((o.off + p, rnd.randint(1, 255), k, mode))
    return out


def _reads(rnd, writes, arena, tags):
    spans = [(o.off, o.size) for o in writes]
    left = EXTRA
    by_off = sorted((o for o in writes), key=lambda o: o.off)
    for _ in range(rnd.randint(1, 3)):                                   # repeats
        o, n = rnd.choice(spans)
        if n <= left:
            spans.append((o, n))
            left -= n
            tags.add("repeat")
    for _ in range(rnd.randint(0, 3)):                                   # empty spans, at any offset
        spans.append((rnd.choice([rnd.randrange(arena // 16) * 16, rnd.randrange(arena)]), 0))
        tags.add("empty_span")
    big = [o for o in writes if o.size >= 48]
    for _ in range(rnd.randint(1, 3) if big else 0):                     # sub-spans from a 16-multiple inside
        o = rnd.choice(big)
        start = 16 * rnd.randint(1, (o.size - 1) // 16)
        n = rnd.randint(1, min(o.size - start, left)) if left else 0
        if n:
            spans.append((o.off + start, n))
            left -= n
            tags.add("sub_span")
    for _ in range(rnd.randint(1, 2) if len(by_off) > 1 else 0):         # two objects and the gap between them
        j = rnd.randrange(len(by_off) - 1)
        a, b = by_off[j], by_off[j + 1]
        n = b.off + b.size - a.off
        if a.size and b.size and b.off > a.off + a.size and n <= left:
            spans.append((a.off, n))
            left -= n
            tags.add("across_gap")
    rnd.shuffle(spans)
    return spans


def _wrong(rnd, desc, arena):
    """`desc` with one field changed, and the field's name."""
    off, size, ent, dd, comp = desc
    field = rnd.choice(WRONG_FIELDS)
    if field == "entropy":
        return (off, size, (ent + 1) & M64, dd, comp), field
    if field == "dedup":
        return (off, size, ent, rnd.choice([d for d in DEDUPS if d != dd]), comp), field
    if field == "compress":
        mine = P.compress_ratio(comp)
        return (off, size, ent, dd, rnd.choice([c for c in COMPRESS if P.compress_ratio(c) != mine])), field
    step = rnd.choice([-1, 1])
    if size + step < 1 or off + size + step > arena:
        step = -step
    return (off, size + step, ent, dd, comp), field


def _verify_lists(rnd, case, plain=False):
    for kind in GENERATED:
        descs = [o.desc for o in case.of_kind(kind)]
        if descs and not plain:
            descs += [rnd.choice(descs) for _ in range(rnd.randint(0, 2))]
        rnd.shuffle(descs)
        case.verify[kind], case.wrong[kind] = descs, None
    if plain or rnd.random() >= 0.4:
        return
    kinds = [k for k in GENERATED if any(d[1] > 1 for d in case.verify[k])]
    if kinds:
        kind = rnd.choice(kinds)
        js = sorted((j for j, d in enumerate(case.verify[kind]) if d[1] > 1), key=lambda j: case.verify[kind][j][1])
        j = rnd.choice(js[len(js) // 2:])           # among the larger ones: a wrong field shows in more bytes
        case.verify[kind][j], field = _wrong(rnd, case.verify[kind][j], case.arena)
        case.wrong[kind] = (j, field)


def _draw_mixed(seed, rnd):
    knobs = _knobs(rnd)
    dense, shared = rnd.random() < 0.25, rnd.random() < 0.33
    params, left = [], CAP
    for _ in range(rnd.randint(1, MAX_OBJECTS)):
        fits = [q for q in params if q[0] <= left]
        if shared and fits and rnd.random() < 0.4:
            p = rnd.choice(fits)                    # a group shares size, entropy, dedup, compress and kind
        else:
            size = _size(rnd)
            if size > left:
                size = rnd.randint(0, min(left, 5000))
            kind = rnd.choices(KINDS, weights=(35, 30, 15, 10, 10))[0]
            p = (size, _entropy(rnd), rnd.choice(DEDUPS), rnd.choice(COMPRESS), kind)
        params.append(p)
        left -= p[0]
    writes, arena = _place(rnd, params, dense)
    case = Case(seed, False, dense, shared, arena, writes, [], {}, {}, [], **knobs)
    case.reads = _reads(rnd, writes, arena, case.tags)
    _verify_lists(rnd, case)
    case.corrupt = _corruption(rnd, writes, rnd.choice([0, 0, 1, 2, 3, 4, 5, 6]))
    return case


def _draw_uniform(seed, rnd):
    knobs = _knobs(rnd)
    dense = rnd.random() < 0.25
    runs, writes = [], []
    off = GUARD + (4096 * rnd.randint(0, 7) if dense else 16 * rnd.randint(0, 512))
    for kind in GENERATED:
        size = 0
        while not 0 < size <= CAP // 2:
            size = _size(rnd)
        n = rnd.randint(1, min(12, CAP // 2 // size))
        stride = _up(size, 4096) if dense else _up(size, 16) + 16 * rnd.randint(0, 40)
        run = Run(kind, off, size, n, stride, rnd.choice(DEDUPS), rnd.choice(COMPRESS), _entropy(rnd),
                  rnd.randint(0, 1 << 20))
        runs.append(run)
        writes += [Obj(o, size, P.object_entropy(run.seed_base, run.first_obj + j), run.dedup, run.compress, kind)
                   for j, (o, _) in enumerate(run.spans)]
        off = _up(off + n * stride, 4096) if dense else off + n * stride + 16 * rnd.randint(1, 512)
    rnd.shuffle(writes)
    arena = _up(off, 16) + GUARD
    case = Case(seed, True, dense, False, arena, writes, [], {}, {}, [], runs=runs, **knobs)
    case.reads = _reads(rnd, writes, arena, case.tags)
    _verify_lists(rnd, case, plain=True)          # the stream verifies have no repeats and no wrong descriptor
    case.corrupt = _corruption(rnd, writes, rnd.choice([0, 1, 2, 3, 6]))
    return case


def draw(seed: int) -> Case:
    rnd = random.Random(SALT + seed)
    return _draw_uniform(seed, rnd) if seed % 4 == 3 else _draw_mixed(seed, rnd)


# ---- the judges ----------------------------------------------------------------------------

_cache = {}


def payload(oracle, base, kind, size, entropy, dedup, compress):
    """The bytes of one object: the C oracle's for the generated kinds, numpy's
    for the uploaded ones.  Read-only and kept while the same case is judged."""
    base = np.ascontiguousarray(base, np.uint8)
    key = (kind, size, entropy, dedup, compress, zlib.crc32(base.tobytes()))
    if key not in _cache:
        if sum(a.size for a in _cache.values()) > 64 * MiB:
            _cache.clear()
        fn, fd = P.compress_ratio(compress)
        if kind == "controlled":
            a = oracle.fill_controlled(size, dedup, fn, fd, entropy, base)
        elif kind == "dg1":
            a = oracle.dgen_fill(size, dedup, fn, fd, entropy)
        elif kind == "zeros":
            a = np.zeros(size, np.uint8)
        else:
            a = np.random.default_rng(entropy).integers(0, 256 if kind == "random" else 4, size, dtype=np.uint8)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def upload_image(case) -> np.ndarray:
    """The arena as it is uploaded: poison, guards included, and the host payloads."""
    a = np.full(case.arena, POISON, np.uint8)
    for o in case.writes:
        if o.kind in HOST and o.size:
            a[o.off:o.off + o.size] = payload(None, np.zeros(1, np.uint8), o.kind, o.size, o.entropy, 0, 1)
    return a


def expected_image(case, oracle, base) -> np.ndarray:
    """The arena after the two fills: poison, uploaded payloads and oracle bytes."""
    a = upload_image(case)
    for o in case.writes:
        if o.kind in GENERATED and o.size:
            a[o.off:o.off + o.size] = payload(oracle, base, o.kind, o.size, o.entropy, o.dedup, o.compress)
    return a


def corrupted(image, case) -> np.ndarray:
    a = image.copy()
    for pos, mask, _k, _mode in case.corrupt:
        a[pos] ^= mask
    return a


def expected_verify(image, case, which, oracle, base, descs=None):
    """What the batch verify of kind `which` must report on `image` for the
    case's verify list (or `descs`), each descriptor taken as given:
    ((bytes, blocks, first offset from the base or None), {descriptor index:
    (bytes, 4 KiB blocks counted from the object's start, first offset from the
    object's first byte)} of the descriptors that are not clean).  A repeated
    descriptor counts twice."""
    descs = case.verify[which] if descs is None else descs
    per, nbytes, nblocks, first = {}, 0, 0, None
    for k, (off, size, ent, dd, comp) in enumerate(descs):
        if not size:
            continue
        bad = np.flatnonzero(image[off:off + size] != payload(oracle, base, which, size, ent, dd, comp))
        if bad.size:
            rec = (int(bad.size), int(np.unique(bad // 4096).size), int(bad[0]))
            per[k] = rec
            nbytes += rec[0]
            nblocks += rec[1]
            first = off + rec[2] if first is None else min(first, off + rec[2])
    return (nbytes, nblocks, first), per
