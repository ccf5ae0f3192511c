"""Crafted blocks for the LZ4 size measurement: every builder
returns the bytes together with the match they are meant to contain, as
(match start, offset, L), and the restatement's parse that shows it.  Random
filler can displace a table entry, so a builder walks seeds 0..63 and returns
the first block whose parse (tests/lz_restatement.py) contains the intended
triple; it raises if none does.  Used by tests/test_lz_cpu.py (which checks
that every case means what it says) and tests/test_gpu_lz.py; not a conftest.
The cached lists are shared: nobody writes to a case's block."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import lz_restatement as R

SEEDS = 64
N = 2304                      # the block of the length sweeps: nine steps of the extension loop
LENGTHS_MISMATCH = range(4, 1031)
LENGTHS_BLOCK_END = range(7, 1031)
DENSE_LENGTHS = range(4, 41)


class Case(NamedTuple):
    name: str
    block: np.ndarray         # read-only
    triple: tuple             # (match start, offset, L)
    parse: R.Parse
    seed: int                 # the first seed whose block parses as meant


def triples(parse: R.Parse) -> list:
    """The parse's matches as (match start, offset, L)."""
    out, pos = [], 0
    for lit, off, L in parse.seqs[:-1]:
        out.append((pos + lit, off, L))
        pos += lit + L
    return out


def result(parse: R.Parse) -> dict:
    """One block's eight fields (R.measure of that block alone) from its parse."""
    return {"bytes": parse.n, "blocks": 1, "lz_bytes": parse.size, "stored_bytes": min(parse.size, parse.n),
            "raw_blocks": int(parse.size >= parse.n), "matches": parse.matches, "match_bytes": parse.match_bytes,
            "literal_bytes": parse.literal_bytes}


def total(cases) -> dict:
    rs = [result(c.parse) for c in cases]
    return {k: sum(r[k] for r in rs) for k in R.FIELDS}


def worst_seed(cases) -> int:
    return max(c.seed for c in cases)


def _first(name, make, only=False):
    """The first of seeds 0..63 whose block contains its triple (and, with
    `only`, no other match)."""
    for seed in range(SEEDS):
        block, triple = make(seed)
        block = np.ascontiguousarray(block, np.uint8)
        parse = R.parse_block(block)
        found = triples(parse)
        if triple in found and (not only or len(found) == 1):
            block.flags.writeable = False
            return Case(name, block, triple, parse, seed)
    raise AssertionError(f"{name}: no seed below {SEEDS} gives a block with its match")


def _rng(*key):
    return np.random.default_rng([0x1C45E5, *key])


def _to_residue(x, r):
    """The smallest value >= x that is r mod 4 (x itself when r is None)."""
    return x if r is None else x + (r - x) % 4


# ---- match lengths ----------------------------------------------------------------------------

def ended_by_mismatch(L, i_align=None, s_align=None) -> Case:
    """A source in group 0 and, from group 17 on, a copy of L bytes with a
    differing byte behind it and in front of it.  The match start and the
    source are i_align and s_align mod 4 when given; the start's lane varies
    with L."""
    s = _to_residue(5 + L % 7, s_align)
    i = _to_residue(1100 + 37 * L % 64, i_align)
    assert 1 <= s and s + L < 1088 and i + L + 1 <= N - 5

    def make(seed):
        a = _rng(1, L, s, i, seed).integers(0, 256, N, dtype=np.uint8)
        a[i:i + L] = a[s:s + L]
        a[i + L] = a[s + L] ^ 0xFF
        a[i - 1] = a[s - 1] ^ 0xFF
        return a, (i, i - s, L)
    return _first(f"mismatch L={L} i%4={i % 4} s%4={s % 4}", make)


def ended_by_block_end(L) -> Case:
    """The copy starts at n - 5 - L and is still equal through the block's
    last byte: the match ends because the last five bytes are literals."""
    assert L >= 7                   # a match starts at or before n - 12
    s, i = 5 + L % 7, N - 5 - L

    def make(seed):
        a = _rng(2, L, seed).integers(0, 256, N, dtype=np.uint8)
        a[i:N] = a[s:s + L + 5]
        a[i - 1] = a[s - 1] ^ 0xFF
        return a, (i, i - s, L)
    return _first(f"block end L={L}", make)


def ended_in_last_five(L, j) -> Case:
    """The copy starts at n - 5 - L, is equal for L + j bytes and differs at
    byte n - 5 + j, one of the last five: the match still ends at n - 5, and
    the extension's last lane holds equal bytes that do not count."""
    assert L >= 7 and 0 <= j <= 4
    s, i = 5 + L % 7, N - 5 - L

    def make(seed):
        a = _rng(7, L, j, seed).integers(0, 256, N, dtype=np.uint8)
        a[i:i + L + j] = a[s:s + L + j]
        a[i + L + j] = a[s + L + j] ^ 0xFF
        a[i - 1] = a[s - 1] ^ 0xFF
        return a, (i, i - s, L)
    return _first(f"last five L={L} j={j}", make)


LENGTHS_LAST_FIVE = (*range(7, 136), *range(250, 263))     # lanes 1 to 33 of step 0, and the edge of step 1


@functools.lru_cache(maxsize=None)
def last_five_sweep() -> tuple:
    return tuple(ended_in_last_five(L, j) for L in LENGTHS_LAST_FIVE for j in range(5))


@functools.lru_cache(maxsize=None)
def mismatch_sweep() -> tuple:
    return tuple(ended_by_mismatch(L) for L in LENGTHS_MISMATCH)


@functools.lru_cache(maxsize=None)
def block_end_sweep() -> tuple:
    return tuple(ended_by_block_end(L) for L in LENGTHS_BLOCK_END)


@functools.lru_cache(maxsize=None)
def dense_sweep() -> tuple:
    """L 4..40 at every (match start mod 4, source mod 4): both funnel shifts of every compare."""
    return tuple(ended_by_mismatch(L, ia, sa) for L in DENSE_LENGTHS for ia in range(4) for sa in range(4))


# ---- offsets -----------------------------------------------------------------------------------

def _far(name, n, src, start, L, to_end=False) -> Case:
    """Zeros (one hash, and the run match swallows them) around a string of
    non-zero bytes at src and its copy at start: nothing but the string's own
    positions can displace its entry.  With to_end the copy runs through the
    block's last byte and L = n - 5 - start; else a differing byte ends it."""
    assert src + L + (5 if to_end else 0) < start or to_end and src + L + 5 == start
    assert n - 5 - start == L if to_end else start + L + 1 <= n - 5

    def make(seed):
        span = L + 5 if to_end else L
        a = np.zeros(n, np.uint8)
        a[src:src + span] = _rng(3, n, src, start, L, seed).integers(1, 256, span, dtype=np.uint8)
        a[start:start + span] = a[src:src + span]
        if src:
            a[start - 1] = 0xFF         # a zero stands in front of the source: no earlier start
        if not to_end:
            a[start + L] = 0xFF         # the source goes on with a zero
        return a, (start, start - src, L)
    return _first(name, make)


def far_match(n, L=7) -> Case:
    """The greatest offset of a block of n bytes: the source at 0, the match at
    the last permitted start n - 12, so L = 7."""
    assert L == 7
    return _far(f"far n={n}", n, 0, n - 12, 7, to_end=True)


@functools.lru_cache(maxsize=None)
def far_cases() -> tuple:
    n = 65536
    cases = [far_match(65536), far_match(65535)]
    # a source at and above 2^15: the table's entry is position + 1 in 16 bits
    for src, start, L in ((32766, 40003, 9), (32767, 40001, 12), (32768, 40002, 40), (50001, 65000, 100),
                          (65400, 65500, 24)):
        cases.append(_far(f"source at {src}", n, src, start, L))
    cases.append(_far("source at 65449, to the end", n, 65449, n - 5 - 20, 20, to_end=True))
    # far sources with many extension steps
    for src, start, L in ((0, 61001, 256), (3, 61002, 257), (0, 61530, 4000), (2, 61430, 4096)):
        cases.append(_far(f"offset {start - src} L={L}", n, src, start, L))
    cases.append(_far("offset 61435 L=4096 to the end", n, 0, n - 5 - 4096, 4096, to_end=True))
    return tuple(cases)


# ---- the table ---------------------------------------------------------------------------------

def _hash(v):
    return ((np.asarray(v, np.uint64) * R.HASH_MUL) & 0xFFFFFFFF) >> 20


def same_hash_words(rng, k) -> list:
    """k different u32 of one hash, none with a zero byte."""
    v = rng.integers(0, 1 << 32, 1 << 17, dtype=np.uint64)
    b = v.astype(np.uint32).view(np.uint8).reshape(-1, 4)
    v = np.unique(v[(b != 0).all(axis=1)])
    h = _hash(v)
    best = int(np.bincount(h.astype(np.int64), minlength=4096).argmax())
    hit = v[h == best]
    assert hit.size >= k
    return [int(x) for x in rng.permutation(hit)[:k]]


def chained_hash_bytes(rng) -> np.ndarray:
    """Five bytes with H(b0..b3) == H(b1..b4) and different words."""
    b = rng.integers(1, 256, (1 << 17, 5), dtype=np.uint8)
    w = b.astype(np.uint64)
    v0 = w[:, 0] | w[:, 1] << 8 | w[:, 2] << 16 | w[:, 3] << 24
    v1 = w[:, 1] | w[:, 2] << 8 | w[:, 3] << 16 | w[:, 4] << 24
    hit = np.nonzero((_hash(v0) == _hash(v1)) & (v0 != v1))[0]
    assert hit.size
    return b[hit[0]]


def put32(a, pos, v):
    a[pos:pos + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


TABLE_N, TABLE_AT, TABLE_L = 400, 300, 16


def same_hash_group(K) -> tuple:
    """K words of one hash four bytes apart in group 1 (positions 64, 68, ...),
    and in group 4 a repeat of 16 bytes from one of them: K cases, one per
    word.  The group's entry is the greatest position, so only the last word's
    repeat is found at its first byte; any other is found one byte late, from
    the next position's own entry.  Every case has that one match alone."""
    assert 2 <= K <= 16
    cases = []
    for j in range(K):
        pj = 64 + 4 * j
        late = 0 if j == K - 1 else 1

        def make(seed):
            rng = _rng(4, K, seed)           # one layout for all j of a seed
            a = rng.integers(0, 256, TABLE_N, dtype=np.uint8)
            for k, v in enumerate(same_hash_words(rng, K)):
                put32(a, 64 + 4 * k, v)
            a[TABLE_AT:TABLE_AT + TABLE_L] = a[pj:pj + TABLE_L]
            a[TABLE_AT + TABLE_L] = a[pj + TABLE_L] ^ 0xFF
            a[TABLE_AT - 1] = a[pj - 1] ^ 0xFF
            return a, (TABLE_AT + late, TABLE_AT - pj, TABLE_L - late)
        cases.append(_first(f"same hash K={K} word {j}", make, only=True))
    return tuple(cases)


def chained_hash_pair(p, at, L) -> Case:
    """Five bytes at p whose two words share a hash: position p leaves the
    entry to p + 1 unless p is the last lane of its group.  A repeat at `at`.
    In a later group than p + 1 the entry is p + 1, whose word differs, so the
    repeat is found one byte late; in p + 1's own group (p at lane 63) the
    lookup sees p, which had to enter itself, and finds it at its first byte."""
    late = 0 if at // 64 == (p + 1) // 64 and p % 64 == 63 else 1
    assert at // 64 > p // 64 and p + L <= at

    def make(seed):
        rng = _rng(5, p, at, seed)
        a = rng.integers(0, 256, TABLE_N, dtype=np.uint8)
        a[p:p + 5] = chained_hash_bytes(rng)
        a[at:at + L] = a[p:p + L]
        a[at + L] = a[p + L] ^ 0xFF
        a[at - 1] = a[p - 1] ^ 0xFF
        return a, (at + late, at - p, L - late)
    return _first(f"chained hash at {p}, repeat at {at}", make, only=True)


@functools.lru_cache(maxsize=None)
def table_cases() -> dict:
    return {"groups": {K: same_hash_group(K) for K in (3, 5, 16)},
            "chained": (chained_hash_pair(84, 300, 16),       # lanes 20 and 21 of one group
                        chained_hash_pair(127, 300, 16),      # lanes 63 and 0, seen from a later group
                        chained_hash_pair(127, 140, 8))}      # and from lane 0's own group


LANE_N = 320


@functools.lru_cache(maxsize=None)
def source_at_every_lane() -> tuple:
    """A first occurrence at each position 0..127 (every lane of two groups)
    and its repeat in group 3, one block per position."""
    cases = []
    for q in range(128):
        L, at = 8 + q % 5, 192 + q * 7 % 64

        def make(seed):
            a = _rng(6, q, seed).integers(0, 256, LANE_N, dtype=np.uint8)
            a[at:at + L] = a[q:q + L]
            a[at + L] = a[q + L] ^ 0xFF
            if q:
                a[at - 1] = a[q - 1] ^ 0xFF
            return a, (at, at - q, L)
        cases.append(_first(f"source at {q}", make))
    return tuple(cases)
