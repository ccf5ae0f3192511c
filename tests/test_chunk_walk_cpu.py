"""CPU: the inputs of tests/test_gpu_chunk_walk.py (tests/chunk_walk_cases.py)
without a GPU, judged by the restatement (tests/chunk_restatement.py) alone.

The written checklist, read off the restatement's cuts:
  - a candidate cut at every (round, lane, bit) with round 0, 1 and the search's last
    (of at least three), lane 0..63 and bit 0, 31, 32, 63 (family 1);
  - every lo & 63 with a candidate at lo - 1, cut at lo and cut at lo + 1, the chunk's
    start at every residue mod 64 along the way (family 2);
  - every hi & 63 with a candidate cut at hi = cap and with a forced cut before a
    candidate at hi + 1 (family 3);
  - wlo == whi with a candidate on both sides of [lo, hi], cut and forced; min = max
    at 37 (lo = hi at every bit) and at 64 (family 4);
  - the lower bit of a word, the lower lane of a round, the earlier round although the
    next one holds a lower lane (family 5);
  - every object end: tails of 1 and min - 1, of min with and without a candidate on
    the last byte, cap = len - 1 forced, cap = len not, hi clipped inside a word
    (family 6);
  - a batch whose first four live spans have 1, 2, 70 and 300 chunks, an object of
    more than 64 slots, a span below min, empty spans, five live spans (family 7).
The echo's premises hold for every part, and each of nine wrong walks changes the
totals of every part whose cuts it changes.  Conditions on the inputs, not
measurements."""
import numpy as np
import pytest

import chunk_restatement as R
import chunk_walk_cases as C


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def parts():
    return C.parts()


def family(n):
    return C.FAMILIES[n]()


def evs(n, kind=None):
    return [e for p in family(n) for e in p.all_events if kind is None or e.kind == kind]


# ---- marker, zeros, the byte-57 device ---------------------------------------------------------

def test_marker_and_zeros():
    assert C.MARKER.size == 32 and C.MARKER.min() >= 1
    assert np.flatnonzero(R.candidates(C.MARKER, 24)[0]).tolist() == [31]
    assert R.window_hash(C.MARKER[None])[0, 0] >> 8 == 0
    zeros = np.zeros(4096 + 64, np.uint8)
    assert R.window_hash(zeros[None, :32])[0, 0] >> 8 != 0 and not R.candidates(zeros, 24).any()
    assert not R.candidates(zeros, 6).any()
    pattern = np.concatenate([C.run57(), np.array(C.RUN_XY, np.uint8), C.run57()])
    assert np.flatnonzero(R.candidates(pattern, 6)[0]).tolist() == [31, 33, 65]
    for k in (0, 1, 5):
        assert np.flatnonzero(R.candidates(C.run57(k), 6)[0]).tolist() == list(range(31, 32 + k))


# ---- the echo's premises -------------------------------------------------------------------------

def test_echo_premises(S, parts):
    assert tuple(p.name for p in parts) == C.PART_NAMES and all(C.part(p.name) is p for p in parts)
    for p in parts:
        assert len({o.name for o in p.objs}) == len(p.objs), p.name
        mine = R.restate(S, [o.data for o in p.objs], p.params)
        for o in p.objs:                                            # no stray candidate
            assert np.flatnonzero(R.candidates(o.data, p.bits)[0]).tolist() == list(o.pos), (p.name, o.name)
        assert mine.unique_chunks == mine.chunks and mine.unique_bytes == mine.bytes, p.name
        both = p.expected(S)
        assert both.chunks == 2 * mine.chunks and both.unique_chunks == mine.chunks, p.name
        assert both.bytes == 2 * mine.bytes and both.unique_bytes == mine.bytes, p.name
        assert both.forced_cuts >= mine.forced_cuts and both.candidates >= mine.candidates, p.name
        single = p.single(len(p.objs) // 2).expected(S)             # the per-object form of a GPU miss
        assert single.chunks == 2 * single.unique_chunks, p.name


def test_layout_keeps_objects_apart(parts):
    for p in parts:
        buf, adds, espans = p.layout()
        assert buf.size <= 16 << 20, p.name
        used = np.zeros(buf.size, np.uint8)
        spans = list(espans)
        for add in adds:
            if add[0] == "stream":
                _, off, size, n, stride = add
                assert off % 16 == 0 and stride % 16 == 0
                spans += [(off + j * stride, size) for j in range(n)]
            else:
                spans += add[1]
        for off, size in spans:
            assert off % 16 == 0
            used[off:off + size] += 1
        assert used.max() == 1 and (buf[used == 0] == C.POISON).all() and used[-16:].max() == 0, p.name
        assert int(used.sum()) == 2 * sum(o.data.size for o in p.objs), p.name
        ends = sorted((off + size, off) for off, size in spans if size)
        assert all(b[1] > a[0] for a, b in zip(ends, ends[1:])), p.name       # poison between any two


# ---- the three forms of the cut rule ---------------------------------------------------------------

def test_sparse_rule_and_walk_equal_the_dense_rule(S, parts):
    for p in parts:
        mn, _avg, mx = p.params
        for a, pos in zip(p.everything, p.positions):
            cand = np.zeros(a.size, bool)
            cand[pos] = True
            dense = R.cuts_of(cand, mn, mx)[:2]
            assert R.cuts_sparse(pos, a.size, mn, mx) == dense, p.name
            assert C.device_walk(pos, a.size, mn, mx) == dense, p.name
        want = p.expected(S)
        assert p.walked()[1] == tuple(getattr(want, f) for f in R.FIELDS), p.name
    rng = np.random.default_rng(3)                                   # and on candidates at random
    for n, mn, mx, density in [(1, 32, 64, .5), (5000, 32, 256, .02), (5000, 37, 37, .1), (70000, 100, 9000, .001),
                               (70000, 64, 64 + C.WIDE, .0002), (300, 64, 300, 0), (299, 64, 300, 0)]:
        for _ in range(6):
            cand = rng.random(n) < density
            cand[:31] = False
            pos = np.flatnonzero(cand).tolist()
            dense = R.cuts_of(cand, mn, mx)[:2]
            assert R.cuts_sparse(pos, n, mn, mx) == dense and C.device_walk(pos, n, mn, mx) == dense


def test_beyond_4_gib_expectation(S):
    """The zero object of the GPU file: its six fields by the sparse rule, stated here as
    computed, and the same construction at a size a host array holds, against the dense
    restatement."""
    n, ends = C.big_case((1 << 20) + 2)
    assert n == (1 << 32) + 8192 and ends[0] < 1 << 32 < ends[1] and ends[2] >= n - 4096
    assert C.zero_fields(n, ends, C.BIG_PARAMS) == (n, 7, 5, (1 << 30) + (1 << 30) - 4999 + 5005 + 8086 + 100, 3, 3)
    out, forced = R.cuts_sparse(ends, n, C.BIG_PARAMS[0], C.BIG_PARAMS[2])
    assert forced == 3 and [e for _, e in out] == [(1 << 30) - 1, (2 << 30) - 1, (3 << 30) - 1, *ends, n - 1]
    small = (64, C.AVG24, 1000)
    for n, ends in [(3 * 4096 + 77, [2900, 3005, 3 * 4096 - 24]), (5000, [31, 4999]), (4000, [999, 1031, 3999])]:
        a = np.zeros(n, np.uint8)
        for e in ends:
            a[e - 31:e + 1] = C.MARKER
        want = R.restate(S, [a], small)
        assert C.zero_fields(n, ends, small) == tuple(getattr(want, f) for f in R.FIELDS), n


# ---- the checklist --------------------------------------------------------------------------------------

def checklist():
    have = {}
    cut1 = evs(1, "cand")
    for rnd in (0, 1, "last"):
        got = {(e.lane, e.bit) for e in cut1 if (e.rnd == e.last >= 2 if rnd == "last" else e.rnd == rnd)}
        for lane in range(64):
            for bit in C.BITS:
                have[f"1: a cut in round {rnd}, lane {lane}, bit {bit}"] = (lane, bit) in got
    have["1: a cut in round 3, the last of an unclipped search"] = any(e.rnd == e.last == 3 and not e.clipped
                                                                      for e in cut1)
    have["1: at least 768 cuts"] = len(cut1) >= 768
    have["1: objects of 16 to 21 KiB"] = all(16 << 10 <= o.data.size <= 21 << 10 for o in family(1)[0].objs[:256])

    cut2 = evs(2, "cand")
    for v in range(64):
        have[f"2: lo & 63 = {v}, a candidate at lo - 1, cut at lo"] = any(
            e.lo63 == v and e.decoy_lo and e.e == e.s + 39 for e in cut2)
        have[f"2: lo & 63 = {v}, a candidate at lo - 1, none at lo, cut at lo + 1"] = any(
            e.lo63 == v and e.decoy_lo and e.e == e.s + 40 for e in cut2)
        have[f"2: a chunk with a candidate at lo - 1 starts at {v} mod 64"] = any(
            e.s & 63 == v and e.decoy_lo for e in cut2)

    for v in range(64):
        have[f"3: hi & 63 = {v}, a candidate cut at hi = cap"] = any(
            e.hi63 == v and e.e - e.s + 1 == 200 and not e.clipped for e in evs(3, "cand"))
        have[f"3: hi & 63 = {v}, a forced cut, a candidate at hi + 1"] = any(
            e.hi63 == v and e.decoy_hi for e in evs(3, "forced"))

    ev4 = [e for e in family(4)[0].all_events]
    for kind in ("cand", "forced"):
        for v in range(32):
            have[f"4: one word, lo & 63 = {v}, candidates at lo - 1 and hi + 1, {kind}"] = any(
                e.kind == kind and e.one_word and e.lo63 == v and e.decoy_lo and e.decoy_hi for e in ev4)
        have[f"4: one word, both of them in that word, {kind}"] = any(
            e.kind == kind and e.one_word and e.decoy_lo and e.decoy_hi and e.lo63 >= 1 and e.hi63 <= 62 for e in ev4)
    for part, m in zip(family(4)[1:], (37, 64)):
        assert part.params[0] == part.params[2] == m
        for kind in ("cand", "forced"):
            bits = {e.lo63 for e in part.all_events if e.kind == kind and e.one_word and e.lo63 == e.hi63}
            have[f"4: min = max = {m}, {kind} at every bit it can fall on"] = \
                bits == (set(range(64)) if m == 37 else {63})
        have[f"4: min = max = {m}, an object that ends with a chunk"] = part.objs[1].data.size % m == 0

    cut5 = evs(5, "cand")
    have["5: the lower of two bits in a word (markers)"] = any(e.same_word for e in family(5)[0].all_events)
    have["5: the lower of five bits in a word (a run)"] = any(e.same_word for e in family(5)[1].all_events)
    have["5: a run that starts below lo"] = any(e.same_word and e.decoy_lo for e in family(5)[1].all_events)
    have["5: the lower of two lanes in a round"] = sum(e.same_round for e in cut5) >= 4
    have["5: ... the higher lane holding the lower bit"] = any(
        e.same_round and e.lane < 40 and e.bit > 2 for e in cut5)
    have["5: lanes 0 and 63 of one round"] = any(e.same_round and e.lane == 0 and e.rnd == 0 for e in cut5)
    for r in (0, 1, 2):
        have[f"5: round {r} before round {r + 1}"] = any(e.next_round and e.rnd == r for e in cut5)
    have["5: the earlier round although the next holds a lower lane"] = any(e.next_round_lower_lane for e in cut5)

    ev6 = evs(6)
    tails = {e.e - e.s + 1 for e in ev6 if e.kind == "tail" and e.s > 0}
    have["6: a tail of 1 byte"] = 1 in tails
    have["6: a tail of min - 1 bytes"] = 63 in tails
    have["6: a tail of min bytes, no candidate"] = any(
        e.kind == "end" and e.s > 0 and e.e - e.s + 1 == 64 and e.one_word and e.lo63 == e.hi63 for e in ev6)
    have["6: a tail of min bytes, a candidate on its last byte"] = any(
        e.kind == "cand" and e.s > 0 and e.e - e.s + 1 == 64 and e.clipped for e in ev6)
    have["6: cap = len - 1 is forced"] = any(e.kind == "forced" and e.s > 0 and e.hi63 != 63 and not e.clipped
                                            and not e.decoy_hi for e in ev6)
    have["6: cap = len is not forced"] = any(e.kind == "end" and e.cap_at_len and e.s > 0 for e in ev6)
    have["6: hi clipped inside a word, no candidate"] = any(
        e.kind == "end" and e.clipped and e.hi63 != 63 and not e.cap_at_len and e.e - e.s + 1 == 150 for e in ev6)
    have["6: hi clipped inside a word, a candidate on it"] = any(
        e.kind == "cand" and e.clipped and e.hi63 != 63 and e.e - e.s + 1 == 150 for e in ev6)
    have["6: three word alignments of each"] = len({e.e & 63 for e in ev6 if e.kind == "end" and e.cap_at_len}) >= 3
    have["6: an object of one byte"] = any(e.kind == "tail" and e.s == 0 and e.e == 0 for e in ev6)
    have["6: an object of exactly max bytes, forced"] = any(e.kind == "forced" and e.s == 0 and e.e == 299 for e in ev6)

    batch, stream = family(7)
    counts = [len(batch.cuts[i][0]) for i in (i for i in batch.adds[0][1] if i is not None)]
    have["7: the first four live spans hold 1, 2, 70 and 300 chunks"] = counts[:4] == [1, 2, 70, 300]
    have["7: an object of more than 64 slots"] = any(-(-o.data.size // 48) + 1 > 64 for o in batch.objs)
    have["7: a span shorter than min"] = any(o.data.size < 48 for o in batch.objs)
    have["7: empty spans in between"] = all(None in idx[1:-1] for _, idx in batch.adds)
    have["7: a live count that is no multiple of four"] = all(
        sum(i is not None for i in idx) % 4 for _, idx in batch.adds)
    have["7: a second add of five spans"] = sum(i is not None for i in batch.adds[1][1]) == 5
    have["7: the same five objects as a stream"] = stream.adds == [("stream", [0, 1, 2, 3, 4])] and all(
        a is b for a, b in zip(stream.objs, batch.objs[5:]))
    have["7: forced and candidate cuts in one object"] = {"cand", "forced", "tail"} <= {e.kind for e in batch.events(3)}
    return have


def test_the_families_meet_the_checklist():
    have = checklist()
    assert len(have) > 1000
    missing = [name for name, ok in have.items() if not ok]
    assert not missing, missing


# ---- the wrong rules ----------------------------------------------------------------------------------------

def test_every_wrong_rule_shows_in_the_totals(parts):
    """A wrong walk cuts the echo objects wrongly too; even so, wherever it changes a cut of X
    the six totals change, and it does change a cut in the family built for it."""
    right = {p.name: p.walked() for p in parts}
    for rule in C.RULES:
        hit = set()
        for p in parts:
            cuts, totals = p.walked(rule)
            if cuts != right[p.name][0]:
                hit.add(int(p.name.split()[0]))
                assert totals != right[p.name][1], (rule, p.name)
            if totals != right[p.name][1]:
                hit.add(int(p.name.split()[0]))
        assert C.BUILT_FOR[rule] in hit, (rule, sorted(hit))
        print(f"{rule}: seen by families {sorted(hit)}")
    cuts, totals = family(6)[0].walked("forced_at_cap_eq_len")          # moves no cut: the forced count alone
    assert cuts == right["6 object ends"][0] and totals[5] > right["6 object ends"][1][5]
