"""Descriptor lists for the batch fill's records ("Batches"),
the smallest that reach each edge of the record machinery: every XCD lead, the
ragged last tile, the own / whole-wave writers of k_batch_map, the dense
layout's first granule and gaps, the split threshold, the sub-batch cuts and
the smallest uniform runs.  No torch, no GPU.  Not a conftest.

A case is (name, objs, shift, tile, split, plan, end):
  objs   (dst_off, size, entropy, dedup, compress) as Context.fill_batch takes them;
  shift  bytes (a multiple of 16) between a 32 KiB-aligned address and dst_base,
         so base contributes (shift >> 12) & 7 to every lead;
  tile   the set_batch_tile knob (0 per launch, 1 dense, 2..64 forced);
  split  the set_batch_split knob;
  plan   what each sub-batch of the call must run as: "uniform", "dense",
         "tiled:S" or "tiled:S+L" (tile shifts of the one or two classes), "empty";
  end    bytes of the arena the objects lie in.

tests/test_batch_records_cpu.py feeds every list to
tests/capi/batch_records_sweep.cpp, which asserts the record rules on it and
prints the plan it got: a list cannot silently stop reaching its path when a
cost constant moves.  tests/test_gpu_batch_records.py runs the lists on a
device against the C oracle.
"""
from __future__ import annotations

import collections
import random

from oracle import oracle_py as P

BLK = 4096
KiB, MiB = 1 << 10, 1 << 20
SEED_BASE = 0x5EED000000000001
DC = ((1, 1), (2, 3), (3, (3, 2)), (0, 7), (4, 2))     # (dedup, compress) in turn
TAILS = (1, 4095, 4096)                                # bytes in an object's last block
TILES = (2, 4, 8, 16, 32, 64)
GAPS = (0, 1, 15, 16, 17, 63, 64, 65, 200)             # granules in front of a dense object
DENSE_BLOCKS = (1, 16, 17, 64, 65, 129)
SUB_FIRST = 16384                                      # kBatchSubFirst: the call's first cut

Case = collections.namedtuple("Case", "name objs shift tile split plan end")


def ent(j: int) -> int:
    return P.object_entropy(SEED_BASE, j)


def lead_of(shift: int, off: int) -> int:
    """obj_lead for a base that is `shift` past a 32 KiB boundary."""
    return ((shift + off) >> 12) & 7


def size_of(nb: int, tail: int) -> int:
    return (nb - 1) * BLK + tail


def _align(x: int, a: int) -> int:
    return -(-x // a) * a


def _obj(j, off, size):
    d, c = DC[j % len(DC)]
    return (off, size, ent(j), d, c)


# ---- leads: every lead two ways, nb + lead around one and two tiles ------------------------

def leads(T: int, shift: int):
    """96 + 32 objects: placement (granule g, at its start or 16 bytes before
    its end) x (m, delta) with nb + lead = m T + delta, tails in turn; then a
    1-byte and a 16-byte object at every placement."""
    objs, at = [], 0
    place = [(g, sub) for g in range(8) for sub in (0, 4080)]
    md = [(m, dl) for m in (1, 2) for dl in (-1, 0, 1)]
    for j in range(len(place) * len(md)):
        g, sub = place[j % 16]
        m, dl = md[(j // 16) % 6]
        off = at + g * BLK + sub
        nb = max(1, m * T + dl - lead_of(shift, off))
        objs.append(_obj(len(objs), off, size_of(nb, TAILS[j % 3])))
        at = _align(off + objs[-1][1], 32 * KiB)
    for g, sub in place:
        for size in (1, 16):
            off = at + g * BLK + sub
            objs.append(_obj(len(objs), off, size))
            at += 32 * KiB
    return objs, at


# ---- dense_front: the dense layout from a first granule 1..7, gaps in front of objects ------

def dense(first_granule: int, pairs, last_blocks: int):
    """Objects of `blocks` blocks behind `gap` granules, from granule
    first_granule of the arena; a last object of last_blocks blocks."""
    objs, at = [], first_granule * BLK
    for gap, nb in pairs:
        at += gap * BLK if objs else 0                  # the first object sits at first_granule itself
        objs.append(_obj(len(objs), at, size_of(nb, TAILS[len(objs) % 3])))
        at += nb * BLK
    objs.append(_obj(len(objs), at, 1 if last_blocks == 1 else size_of(last_blocks, 4095)))
    return objs, at + last_blocks * BLK


# ---- map_paths: k_batch_map's writers ---------------------------------------------------------

def records(T: int, counts, shift: int = 0):
    """One object of exactly r records at tile T for each r, 16-byte packed."""
    objs, at = [], 16
    for j, r in enumerate(counts):
        nb = r * T - lead_of(shift, at)
        objs.append(_obj(j, at, size_of(nb, TAILS[j % 3])))
        at = _align(at + objs[-1][1], 16) + 16 * (j % 3)
    return objs, at


def big_among_small(n: int, big: set[int], T: int = 2, r: int = 17):
    """n objects at 32 KiB steps (lead 0: one record of T = 2 each), the ones at
    the indices `big` of r records."""
    objs, at = [], 0
    for j in range(n):
        size = size_of(r * T, TAILS[j % 3]) if j in big else (1, 16, 4097)[j % 3]
        objs.append(_obj(j, at, size))
        at = _align(at + size, 32 * KiB)
    return objs, at


# ---- split_edges -----------------------------------------------------------------------------

def split_mix(blocks, seed: int, empties: bool = True):
    """Objects of the given block counts, 16-byte packed in address order,
    empty objects between them, the descriptors shuffled."""
    objs, at = [], 32
    for j, nb in enumerate(blocks):
        objs.append(_obj(j, at, size_of(nb, TAILS[j % 3])))
        at = _align(at + objs[-1][1], 16) + 16
        if empties and j % 3 == 1:
            objs.append((at, 0, 5, 9, 1))
    random.Random(seed).shuffle(objs)
    return objs, at


# ---- sub_batch_cuts ----------------------------------------------------------------------------

CUT_SIZES = (1, 16, 17, 4096, 4097)


def packed_small(n: int, first: int = 0, at: int = 0, empty=range(0)):
    objs = []
    for j in range(first, first + n):
        size = 0 if j in empty else CUT_SIZES[j % 5]
        objs.append(_obj(j, at, size))
        at += _align(size, 16)
    return objs, at


def uniform_run(m: int, size: int, stride: int, first: int = 0, at: int = 0, e0: int | None = None, dc=(1, 1)):
    e0 = ent(first) if e0 is None else e0
    objs = [(at + j * stride, size, (e0 + (j << 32)) & (2**64 - 1), dc[0], dc[1]) for j in range(m)]
    return objs, at + m * stride


def _cases():
    out = []

    def add(name, built, shift=0, tile=0, split=0, plan=None):
        objs, end = built
        out.append(Case(name, objs, shift, tile, split, plan, end))

    # leads
    for k, T in enumerate(TILES):
        add(f"leads_t{T}", leads(T, 0), tile=T, plan=(f"tiled:{T.bit_length() - 1}",))
        s = (k % 7 + 1) * BLK + 16
        add(f"leads_t{T}_shift", leads(T, s), shift=s, tile=T, plan=(f"tiled:{T.bit_length() - 1}",))
    add("leads_auto", leads(8, 0), plan=("tiled:3",))
    add("leads_auto_shift", leads(8, 3 * BLK + 16), shift=3 * BLK + 16, plan=("tiled:3",))
    # dense_front
    full = [(g, nb) for nb in DENSE_BLOCKS for g in GAPS]
    add("dense_full_g5", dense(5, full, 1), tile=1, plan=("dense",))
    for g in range(1, 8):
        short = [(GAPS[(j + g) % 9], DENSE_BLOCKS[j % 6]) for j in range(9)]
        add(f"dense_off_g{g}", dense(g, short, 129 if g % 2 else 1), tile=1, plan=("dense",))
        add(f"dense_base_g{g}", dense(0, short, 1 if g % 2 else 129), shift=g * BLK + 16 * (g % 2), tile=1,
            plan=("dense",))
    add("dense_one", ([_obj(0, 3 * BLK, 4097)], 5 * BLK), tile=1, plan=("dense",))
    add("dense_one_base", ([_obj(0, 0, 129 * BLK - 1)], 129 * BLK), shift=7 * BLK, tile=1, plan=("dense",))
    # map_paths
    for T in (2, 8):
        add(f"map_records_t{T}", records(T, (16, 17, 64, 65, 128, 129)), tile=T, plan=(f"tiled:{T.bit_length() - 1}",))
    add("map_t2_64_big", big_among_small(64, set(range(64))), tile=2, plan=("tiled:1",))
    add("map_t2_65_big", big_among_small(65, set(range(65))), tile=2, plan=("tiled:1",))
    add("map_t2_lane0", big_among_small(64, {0}), tile=2, plan=("tiled:1",))
    add("map_t2_lane63", big_among_small(64, {63}), tile=2, plan=("tiled:1",))
    add("map_t64_17_65", records(64, (17, 65), 16), shift=16, tile=64, plan=("tiled:6",))
    for n in (1, 63, 64, 65, 257):
        add(f"map_last_big_n{n}", big_among_small(n, {n - 1}), tile=2, plan=("tiled:1",))
    add("one_record_t64", ([_obj(0, 16, 4097)], 2 * BLK + 16), tile=64, plan=("tiled:6",))
    # split_edges
    for sp in (2, 16):
        edge = [sp - 1, sp, sp + 1]
        add(f"split{sp}_mixed", split_mix(edge * 4 + [300, 511, 260] * 4, sp), split=sp, plan=("tiled:3+5",))
        add(f"split{sp}_all_small", split_mix([sp - 1] * 9 + [1] * 3, sp + 1), split=sp, plan=("tiled:3",))
        add(f"split{sp}_all_large", split_mix([sp, sp + 1, 300] * 4, sp + 2), split=sp,
            plan=("tiled:4",) if sp == 2 else ("tiled:5",))
    add("split16_same_tile", split_mix([15, 14, 17, 18, 16, 15] * 3, 7), split=16, plan=("tiled:3",))
    # sub_batch_cuts
    for n in (16383, 16384, 16385, 49153):
        # a last sub-batch of one object, which happens to start a granule: the dense layout, lead0 = 2
        add(f"cuts_n{n}", packed_small(n), plan={16383: ("tiled:3",), 16384: ("tiled:3",), 16385: ("tiled:3", "dense"),
                                                 49153: ("tiled:3", "tiled:3", "dense")}[n])
    add("cuts_empty_middle", packed_small(49153, empty=range(16384, 49152)), plan=("tiled:3", "empty", "dense"))
    a, end = uniform_run(SUB_FIRST, 20 * KiB + 16, 24 * KiB)
    b, end = packed_small(101, first=SUB_FIRST, at=end)
    add("cuts_uniform_then_mixed", (a + b, end), plan=("uniform", "tiled:3"))
    a, end = packed_small(SUB_FIRST)
    b, end = uniform_run(SUB_FIRST, 20 * KiB + 16, 24 * KiB, first=SUB_FIRST, at=_align(end, 16))
    add("cuts_mixed_then_uniform", (a + b, end), plan=("tiled:3", "uniform"))
    # uniform_min
    add("uniform_m2_16", uniform_run(2, 16, 16, at=4080), plan=("uniform",))
    a, end = uniform_run(2, 16, 16, at=32)
    add("uniform_m2_empty_between", ([a[0], (48, 0, 1, 1, 1), a[1]], end), plan=("uniform",))
    add("uniform_m3_4097", uniform_run(3, 4097, 4112, at=16, dc=(2, 3)), plan=("uniform",))
    add("uniform_wrap", uniform_run(4, 8 * KiB + 1, 12 * KiB, e0=2**64 - 2**32 + 5), plan=("uniform",))
    add("uniform_m1", uniform_run(1, 40 * KiB + 1, 64 * KiB, at=BLK), plan=("dense",))
    add("uniform_tiled_lead5", uniform_run(2048, 32 * KiB, 32 * KiB, at=5 * BLK), plan=("uniform",))
    # repeats
    add("repeat_three", ([_obj(0, 5 * BLK + 16, 70001)] * 3, 5 * BLK + 16 + 70001), plan=("tiled:3",))
    add("empties_only", ([(16 * j, 0, j, 1, 1) for j in range(5)], 64), plan=("empty",))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
GROUPS = {
    "leads": [c.name for c in CASES if c.name.startswith("leads_")],
    "dense_front": [c.name for c in CASES if c.name.startswith("dense_")],
    "map_paths": [c.name for c in CASES if c.name.startswith(("map_", "one_record"))],
    "split_edges": [c.name for c in CASES if c.name.startswith("split")],
    "sub_batch_cuts": [c.name for c in CASES if c.name.startswith("cuts_")],
    "uniform_min": [c.name for c in CASES if c.name.startswith("uniform_")],
    "repeats": ["repeat_three", "empties_only"],
}
assert sorted(sum(GROUPS.values(), [])) == sorted(BY_NAME)

# what a map_paths list must hold, as the sweep counts it: objects of exactly 16
# and 17 records, and objects of more than 64 (the wave loop's second pass)
MAP_COUNTS = {
    "map_records_t2": (1, 1, 3), "map_records_t8": (1, 1, 3), "map_t2_64_big": (0, 64, 0), "map_t2_65_big": (0, 65, 0),
    "map_t2_lane0": (0, 1, 0), "map_t2_lane63": (0, 1, 0), "map_t64_17_65": (0, 1, 1),
    "map_last_big_n1": (0, 1, 0), "map_last_big_n63": (0, 1, 0), "map_last_big_n64": (0, 1, 0),
    "map_last_big_n65": (0, 1, 0), "map_last_big_n257": (0, 1, 0),
}


def sweep_input(case: Case, base: int = 0x7F3A00000000) -> str:
    """The case as tests/capi/batch_records_sweep.cpp reads it."""
    lines = [f"list {case.name} {base + case.shift} {case.tile} {case.split} {len(case.objs)}"]
    for off, size, e, d, c in case.objs:
        fn, fd = P.compress_ratio(c)
        lines.append(f"{off} {size} {e} {d} {fn} {fd}")
    return "\n".join(lines) + "\n"
