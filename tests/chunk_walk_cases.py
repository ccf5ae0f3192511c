"""Crafted inputs for pass B of the chunker, the cut walk (chunk_walk in
csrc/s3dg_chunks.hip): objects whose candidates lie exactly
where a case wants them, the "echo" that makes their cuts visible in the six
totals of a ChunkResult, the events of the walk read off the restatement's cuts,
and a model of the walk with one wrong rule at a time.  No GPU is needed here;
tests/test_chunk_walk_cpu.py holds these inputs to a written checklist and
tests/test_gpu_chunk_walk.py runs them.  Not a conftest.

Candidates.  At avg_bytes = 2^24 a window is a candidate when h >> 8 == 0, about
one position in 16 MiB of random bytes; MARKER is a 32-byte string that is one,
so a candidate stands where MARKER ends and nowhere else.  Two candidates less
than 32 bytes apart come from byte 57 at avg_bytes = 64: a run of 32 + k bytes
of 57 is k + 1 adjacent candidates, and RUN_XY behind such a run is one more
candidate two bytes on.  Every object is checked against the restatement when it
is built: its candidates are exactly the intended ones, else its next seed is
taken.

The echo.  The expected chunks of an object X, each copied into a span of its
own, are X's echo.  A chunk alone is cut as that one chunk, so X and its echo in
one handle give chunks = 2C and unique_chunks = C; a device that cuts X anywhere
else has a chunk that matches no echo.  That needs every chunk to have content
of its own: the background is seeded random non-zero bytes."""
import bisect
import dataclasses
import functools

import numpy as np

import chunk_restatement as R

AVG24 = 1 << 24
# Found by search: numpy.random.default_rng(24), batches of 2^18 rows of 32 bytes in 1..255, the first row
# whose window hash passes at 24 bits (batch 45, row 250017).
MARKER = np.frombuffer(bytes.fromhex("4c515165d52dd5b91b7c82d31af788d13d4deee15d7cd45bde9ea60f567cbea1"), np.uint8)
# 32 x 57 | X | Y | 32 x 57 has, at 6 bits, the candidates 31, 33 and 65 and no other (the first such pair
# with X > 1, by search over all pairs).
RUN_XY = (6, 90)
POISON = 57                       # a candidate wherever it is read at 6 bits
BITS = (0, 31, 32, 63)
WIDE = 3 * 4096 + 100             # max - min of the four-round families


def run57(k=0):
    return np.full(32 + k, 57, np.uint8)


@dataclasses.dataclass(frozen=True)
class Obj:
    name: str                     # the object and the event it is built for
    data: np.ndarray
    pos: tuple                    # its candidates (the intended ones, checked when built)


def make(name, n, pieces, want, bits, key):
    """An object of n seeded random non-zero bytes with `pieces` ((offset, bytes)) laid over
    them: the first seed at which the restatement finds exactly the candidates `want`."""
    want = sorted(int(w) for w in want)
    for attempt in range(4000):
        a = np.random.default_rng([*key, attempt]).integers(1, 256, n, dtype=np.uint8)
        for off, b in pieces:
            assert 0 <= off and off + len(b) <= n, (name, off, len(b), n)
            a[off:off + len(b)] = b
        if np.flatnonzero(R.candidates(a, bits)[0]).tolist() == want:
            a.setflags(write=False)
            return Obj(name, a, tuple(want))
    raise AssertionError(f"no seed gives {name} its candidates")


def marked(name, n, ends, key):
    """MARKER ending at every offset of `ends`, at 24 bits."""
    assert all(b - a >= 32 for a, b in zip(sorted(ends), sorted(ends)[1:])), name
    return make(name, n, [(e - 31, MARKER) for e in ends], ends, 24, key)


# ---- the walk, with one wrong rule at a time ---------------------------------------------------

RULES = ("lo_plus_1", "no_low_mask", "no_high_mask", "round0_only", "highest_bit", "lane63_dropped",
         "lane0_later_dropped", "high_half_lost", "forced_at_cap_eq_len")


def device_walk(pos, n, mn, mx, rule=None):
    """The walk as the kernel arranges it (words, 64 lanes to a round, two masks), over the
    sorted candidates `pos` of an object of n bytes: chunks [s, e] and forced cuts.  Without
    a rule it is the cut rule.  The rules:
      lo_plus_1             the search starts one position late
      no_low_mask           it starts at the first bit of lo's word (never before s: a cut
                            before the chunk's start would not end)
      no_high_mask          it runs to the last bit of hi's word
      round0_only           only the first 64 words are searched
      highest_bit           the found word's highest bit instead of its lowest
      lane63_dropped        the word of lane 63 of every round is skipped
      lane0_later_dropped   the word of lane 0 of every round after the first is skipped
      high_half_lost        the found word's high 32 bits are lost: a lowest bit >= 32 reads
                            as 64, the count of trailing zeros of an empty word
      forced_at_cap_eq_len  a chunk that ends with the object after max - 1 bytes counts as forced"""
    assert rule is None or rule in RULES
    out, forced, s = [], 0, 0
    while s < n:
        e = n - 1
        lo = s + mn - 1 + (rule == "lo_plus_1")
        if lo < n:
            cap = s + mx - 1
            hi = min(cap, n - 1)
            wlo, whi = lo >> 6, hi >> 6
            a = max(wlo << 6, s) if rule == "no_low_mask" else lo
            b = min((whi << 6) + 63, n - 1) if rule == "no_high_mask" else hi
            k, found = bisect.bisect_left(pos, a), None
            while k < len(pos) and pos[k] <= b:
                rnd, lane = divmod((pos[k] >> 6) - wlo, 64)
                if rule == "round0_only" and rnd > 0:
                    break
                if (rule == "lane63_dropped" and lane == 63) or (rule == "lane0_later_dropped" and rnd and not lane):
                    k += 1
                    continue
                found = pos[k]
                break
            if found is None:
                e = hi
                forced += cap <= n if rule == "forced_at_cap_eq_len" else cap < n
            else:
                e = found
                if rule == "highest_bit":
                    while k + 1 < len(pos) and pos[k + 1] <= b and pos[k + 1] >> 6 == found >> 6:
                        k += 1
                    e = pos[k]
                elif rule == "high_half_lost" and found & 63 >= 32:
                    e = (found | 63) + 1
        out.append((s, e))
        s = e + 1
    return out, forced


# ---- events --------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Event:
    """What the walk met at one chunk [s, e] (the definitions of the search's lo, cap, hi)."""
    kind: str                     # "tail": lo >= len; "cand": a candidate cut; "forced"; "end": the object's end
    s: int
    e: int
    lo63: int = -1
    hi63: int = -1
    rnd: int = -1
    lane: int = -1
    bit: int = -1
    last: int = -1                # the search's last round
    clipped: bool = False         # hi = len - 1 < cap
    one_word: bool = False        # wlo == whi
    decoy_lo: bool = False        # a candidate at lo - 1
    decoy_hi: bool = False        # a candidate at hi + 1
    same_word: bool = False       # a cut with a later candidate in its word, inside [lo, hi]
    same_round: bool = False      # ... with a candidate in a later lane of its round
    next_round: bool = False      # ... with a candidate in the next round
    next_round_lower_lane: bool = False
    cap_at_len: bool = False      # cap == len


def events(pos, n, mn, mx):
    """The events of the restatement's cuts of one object."""
    pos = [int(p) for p in pos]
    have = set(pos)
    out = []
    for s, e in R.cuts_sparse(pos, n, mn, mx)[0]:
        lo = s + mn - 1
        if lo >= n:
            out.append(Event("tail", s, e))
            continue
        cap = s + mx - 1
        hi = min(cap, n - 1)
        wlo, whi = lo >> 6, hi >> 6
        common = dict(lo63=lo & 63, hi63=hi & 63, last=(whi - wlo) // 64, clipped=hi < cap, one_word=wlo == whi,
                      decoy_lo=lo - 1 in have, decoy_hi=hi + 1 in have, cap_at_len=cap == n)
        inside = [p for p in pos[bisect.bisect_left(pos, lo):] if p <= hi]
        if inside:
            assert e == inside[0]
            rnd, lane = divmod((e >> 6) - wlo, 64)
            later = [divmod((p >> 6) - wlo, 64) for p in inside[1:]]
            out.append(Event("cand", s, e, rnd=rnd, lane=lane, bit=e & 63,
                             same_word=(rnd, lane) in later,
                             same_round=any(r == rnd and l > lane for r, l in later),
                             next_round=any(r == rnd + 1 for r, l in later),
                             next_round_lower_lane=any(r == rnd + 1 and l < lane for r, l in later), **common))
        else:
            assert e == hi
            out.append(Event("forced" if cap < n else "end", s, e, **common))
    return out


# ---- a part: objects, parameters, adds, echo --------------------------------------------------------

def _up16(x):
    return (x + 15) // 16 * 16


class Part:
    """The objects of one handle.  `adds` lists the adds that bring them in: ("batch", [i or
    None, ...]) with None an empty span, or ("stream", [i, ...]) for objects of one length;
    by default one batch of them all.  The echo follows as one more batch add."""

    def __init__(self, name, params, objs, adds=None):
        self.name, self.params, self.objs = name, tuple(params), list(objs)
        self.adds = adds or [("batch", list(range(len(self.objs))))]
        used = sorted(i for _, idx in self.adds for i in idx if i is not None)
        assert used == list(range(len(self.objs))), name       # every object once

    @property
    def bits(self):
        return self.params[1].bit_length() - 1

    @functools.cached_property
    def cuts(self):
        """Per object (chunks, forced cuts) by the restatement's dense rule."""
        out = []
        for o in self.objs:
            cand = np.zeros(o.data.size, bool)
            cand[list(o.pos)] = True
            out.append(R.cuts_of(cand, self.params[0], self.params[2])[:2])
        return out

    @functools.cached_property
    def echo(self):
        """Per object, its expected chunks as arrays of their own."""
        return [[o.data[s:e + 1] for s, e in c] for o, (c, _f) in zip(self.objs, self.cuts)]

    @functools.cached_property
    def everything(self):
        """Every object of the handle: X, then the echoes."""
        return [o.data for o in self.objs] + [c for cs in self.echo for c in cs]

    @functools.cached_property
    def positions(self):
        """The candidates of everything(), by the restatement."""
        return [np.flatnonzero(R.candidates(a, self.bits)[0]).tolist() for a in self.everything]

    def events(self, i):
        return events(self.objs[i].pos, self.objs[i].data.size, self.params[0], self.params[2])

    @functools.cached_property
    def all_events(self):
        return [ev for i in range(len(self.objs)) for ev in self.events(i)]

    def expected(self, S):
        """The handle's result by the restatement over X and the echo."""
        return R.restate(S, self.everything, self.params)

    def walked(self, rule=None):
        """(the chunks of X, the six totals of X and the echo) under device_walk with `rule`.
        A chunk is its length and its bytes: the fingerprint takes both."""
        mn, _avg, mx = self.params
        seen, cuts = {}, []
        nbytes = chunks = forced = 0
        for k, (a, pos) in enumerate(zip(self.everything, self.positions)):
            out, f = device_walk(pos, a.size, mn, mx, rule)
            if k < len(self.objs):
                cuts.append(out)
            mv = memoryview(a)
            for s, e in out:
                seen[(e - s + 1, bytes(mv[s:e + 1]))] = e - s + 1
            nbytes, chunks, forced = nbytes + a.size, chunks + len(out), forced + f
        return cuts, (nbytes, chunks, len(seen), sum(seen.values()), sum(len(p) for p in self.positions), forced)

    def single(self, i):
        """Object i alone with its own echo."""
        return Part(f"{self.name}: {self.objs[i].name}", self.params, [self.objs[i]])

    def layout(self):
        """(buffer, adds, echo spans): every object and every echo chunk at a 16-byte aligned
        offset of one buffer, POISON in the gaps and behind the last one.  An add is
        ("batch", spans) or ("stream", offset, size, count, stride)."""
        at, cur = {}, 16
        adds = []
        for kind, idx in self.adds:
            if kind == "stream":
                size = self.objs[idx[0]].data.size
                assert all(self.objs[i].data.size == size for i in idx)
                stride = _up16(size) + 16
                for j, i in enumerate(idx):
                    at[i] = cur + j * stride
                adds.append(("stream", cur, size, len(idx), stride))
                cur += len(idx) * stride
            else:
                spans = []
                for i in idx:
                    if i is None:
                        spans.append((cur, 0))
                        continue
                    at[i] = cur
                    spans.append((cur, self.objs[i].data.size))
                    cur = _up16(cur + self.objs[i].data.size) + 16 * (1 + len(spans) % 3)
                adds.append(("batch", spans))
        espans = []
        for cs in self.echo:
            for c in cs:
                espans.append((cur, c.size))
                cur = _up16(cur + c.size) + 16 * (1 + len(espans) % 2)
        buf = np.full(cur + 64, POISON, np.uint8)
        for i, off in at.items():
            buf[off:off + self.objs[i].data.size] = self.objs[i].data
        for (off, size), c in zip(espans, (c for cs in self.echo for c in cs)):
            buf[off:off + size] = c
        return buf, adds, espans


# ---- 1. lane x round x bit ------------------------------------------------------------------------

def _at(s, mn, rnd, lane, bit):
    """The offset of bit `bit` of the word of (rnd, lane) in the search of a chunk from s."""
    return ((((s + mn - 1) >> 6) + 64 * rnd + lane) << 6) + bit


@functools.lru_cache(maxsize=None)
def family1():
    """max - min = 3 * 4096 + 100: four rounds.  Object k holds three cuts: in round 0 at
    (lane, bit) number k, in round 1 at the mirrored lane, and in round 2 with the object
    ending at most 64 bytes behind, so that round 2 is that search's last.  Eight more
    objects cut in round 3, the last one of a search that is not clipped."""
    mn, mx = 65, 65 + WIDE
    objs = []
    grid = [(lane, bit) for lane in range(64) for bit in BITS]
    for k, (lane, bit) in enumerate(grid):
        lane2, bit2 = grid[(k * 5 + 3) % 256]                  # another pairing for the last round
        e0 = _at(0, mn, 0, lane, bit)
        e1 = _at(e0 + 1, mn, 1, 63 - lane, bit)
        e2 = _at(e1 + 1, mn, 2, lane2, bit2)
        tail = 1 + (7 * k) % 64
        if lane2 == 63:
            tail = min(tail, 63 - bit2)                        # hi stays in the cut's word
        objs.append(marked(f"object {k}: round 0 lane {lane} bit {bit} | round 1 lane {63 - lane} bit {bit} | "
                           f"last round 2 lane {lane2} bit {bit2}, {tail} bytes behind",
                           e2 + 1 + tail, [e0, e1, e2], (1, k)))
    for k, (lane, bit) in enumerate([(0, b) for b in BITS] + [(1, 0), (1, 31), (1, 32), (1, 36)]):
        e = _at(0, mn, 3, lane, bit)
        objs.append(marked(f"object {256 + k}: last round 3 lane {lane} bit {bit}", mx + 10, [e], (1, 256 + k)))
    return [Part("1 lane x round x bit", (mn, AVG24, mx), objs)]


# ---- 2. low mask -------------------------------------------------------------------------------------

def _lead57(e0):
    """A first chunk [0, e0] closed by the one candidate of a run of 32."""
    return [(e0 - 31, run57())], [e0]


@functools.lru_cache(maxsize=None)
def family2():
    """(40, 64, 1024).  A first chunk of 40 + r bytes, r = 0..63, so that s and lo = s + 39
    take every residue; then a run of 33 that ends at lo (candidates lo - 1 and lo), or a
    run of 32 that ends at lo - 1 with RUN_XY behind it (candidates lo - 1 and lo + 1)."""
    mn = 40
    objs = []
    for r in range(64):
        e0 = 39 + r
        lo = e0 + mn
        pieces, want = _lead57(e0)
        objs.append(make(f"object {2 * r}: lo & 63 = {lo & 63}, candidates at lo - 1 and lo", lo + 1 + 9,
                         pieces + [(lo - 32, run57(1))], want + [lo - 1, lo], 6, (2, r, 0)))
        objs.append(make(f"object {2 * r + 1}: lo & 63 = {lo & 63}, candidates at lo - 1 and lo + 1", lo + 2 + 9,
                         pieces + [(lo - 32, run57()), (lo, np.array(RUN_XY, np.uint8))], want + [lo - 1, lo + 1], 6,
                         (2, r, 1)))
    return [Part("2 low mask", (mn, 64, 1024), objs)]


# ---- 3. high mask ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family3():
    """(64, 2^24, 200).  A first chunk of 64 + r bytes, r = 0..63, then MARKER ending at
    hi = cap (a candidate cut at max bytes) or at hi + 1 (a forced cut; the next chunk
    starts on a candidate)."""
    mn, mx = 64, 200
    objs = []
    for r in range(64):
        e0 = 63 + r
        hi = e0 + mx
        objs.append(marked(f"object {2 * r}: hi & 63 = {hi & 63}, candidate at hi", hi + 1 + 20, [e0, hi], (3, r, 0)))
        objs.append(marked(f"object {2 * r + 1}: hi & 63 = {hi & 63}, candidate at hi + 1", hi + 1 + 20, [e0, hi + 1],
                           (3, r, 1)))
    return [Part("3 high mask", (mn, AVG24, mx), objs)]


# ---- 4. one word -------------------------------------------------------------------------------------

def _pieces_of(total, lo, hi):
    """`total` (or total + 64, + 128) split into lengths from lo to hi."""
    for t in (total, total + 64, total + 128):
        for k in range(1, 8):
            if lo * k <= t <= hi * k:
                q, rem = divmod(t, k)
                return [q + (j < rem) for j in range(k)]
    raise AssertionError(total)


@functools.lru_cache(maxsize=None)
def family4():
    """(40, 64, 72): hi = lo + 32, both masks on one word for lo & 63 <= 31, a candidate at
    lo - 1 and one at hi + 1 (in the same word for lo & 63 from 1 to 30): between them one at
    lo + 1, or none (a forced cut).  And min = max at 37 and at 64: lo = hi, one bit."""
    mn, mx = 40, 72
    objs = []
    for v in range(32):                                            # lo & 63
        lead = _pieces_of(mn + (v - 2 * mn + 1) % 64, mn, mx)       # s = sum(lead), s + 39 = v mod 64
        pieces, want, s = [], [], 0
        for n in lead:
            s += n
            pieces.append((s - 32, run57()))
            want.append(s - 1)
        lo = s + mn - 1
        assert lo & 63 == v
        both = [(lo - 32, run57()), (lo + 2, run57())]
        objs.append(make(f"object {2 * v}: lo & 63 = {v}, candidates at lo - 1, lo + 1 and hi + 1", lo + 34 + 5,
                         pieces + both + [(lo, np.array(RUN_XY, np.uint8))], want + [lo - 1, lo + 1, lo + 33], 6,
                         (4, v, 0)))
        objs.append(make(f"object {2 * v + 1}: lo & 63 = {v}, candidates at lo - 1 and hi + 1 only", lo + 34 + 5,
                         pieces + both, want + [lo - 1, lo + 33], 6, (4, v, 1)))
    parts = [Part("4 one word", (mn, 64, mx), objs)]
    for m, count in ((37, 200), (64, 40)):
        ends = [m * (k + 1) - 1 for k in range(count) if k % 3 != 2]      # a marker closes two chunks of three
        parts.append(Part(f"4 one word, min = max = {m}", (m, AVG24, m),
                          [marked(f"object 0: {count} chunks of {m} and 11 bytes", m * count + 11, ends, (4, m, 0)),
                           marked(f"object 1: {count // 2} chunks of {m} to the byte", m * (count // 2),
                                  ends[:count // 4], (4, m, 1))]))
    return parts


# ---- 5. order ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family5():
    """Two candidates in one search: in one word (MARKER twice 32 bytes apart; runs of 36
    and 37 of byte 57), in two lanes of one round, in a round and the next."""
    mn, mx = 65, 65 + WIDE
    pairs = [("word", (0, 5, 3), (0, 5, 35)), ("word", (1, 63, 0), (1, 63, 32)), ("word", (0, 0, 31), (0, 0, 63)),
             ("lane", (0, 3, 10), (0, 40, 2)), ("lane", (0, 0, 63), (0, 63, 0)), ("lane", (1, 31, 20), (1, 32, 5)),
             ("lane", (2, 62, 9), (2, 63, 1)),
             ("round", (0, 63, 20), (1, 0, 0)), ("round", (0, 10, 20), (1, 5, 7)), ("round", (1, 50, 33), (2, 3, 1)),
             ("round", (2, 63, 10), (3, 0, 0))]
    objs = []
    for k, (what, a, b) in enumerate(pairs):
        e1, e2 = _at(0, mn, *a), _at(0, mn, *b)
        objs.append(marked(f"object {k}: {what}, candidates at {a} and {b}", e2 + 1 + 30, [e1, e2], (5, k)))
    parts = [Part("5 order, four rounds", (mn, AVG24, mx), objs)]
    objs = []
    for k, (r, d, run) in enumerate([(0, 0, 4), (9, 3, 4), (20, -2, 4), (45, 1, 5), (57, -3, 5)]):
        e0 = 39 + r
        lo = e0 + 40
        c = lo + d                                                # the run's first candidate
        pieces, want = _lead57(e0)
        objs.append(make(f"object {k}: lo & 63 = {lo & 63}, candidates from lo{d:+d} to lo{d + run:+d}",
                         c + run + 1 + 9, pieces + [(c - 31, run57(run))], want + list(range(c, c + run + 1)), 6,
                         (5, k, 6)))
    parts.append(Part("5 order, runs of byte 57", (40, 64, 1024), objs))
    return parts


# ---- 6. object ends ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family6():
    """(64, 2^24, 300).  After a first chunk of 64 + r bytes: tails of 1 and of min - 1 bytes
    (lo >= len), of exactly min with and without a candidate on the last byte, a last chunk of
    max bytes (cap = len - 1, forced) and of max - 1 (cap = len, not forced), and hi clipped
    to len - 1 inside a word.  And objects that are one chunk from their first byte."""
    mn, mx = 64, 300
    objs = []

    def add(what, n, ends):
        objs.append(marked(f"object {len(objs)}: {what}", n, ends, (6, len(objs))))

    for r in (0, 17, 40):
        e0 = 63 + r
        s = e0 + 1
        add(f"r = {r}, a tail of 1 byte", s + 1, [e0])
        add(f"r = {r}, a tail of min - 1 bytes", s + mn - 1, [e0])
        add(f"r = {r}, a tail of min bytes, no candidate", s + mn, [e0])
        add(f"r = {r}, a tail of min bytes, a candidate on the last one", s + mn, [e0, s + mn - 1])
        add(f"r = {r}, cap = len - 1", s + mx, [e0])
        add(f"r = {r}, cap = len", s + mx - 1, [e0])
        add(f"r = {r}, hi clipped inside a word", s + 150, [e0])
        add(f"r = {r}, hi clipped inside a word, a candidate on it", s + 150, [e0, s + 149])
    for n in (1, 20, mn - 1, mn, mx - 1, mx, mx + 1):
        add(f"{n} bytes and no candidate", n, [])
    return [Part("6 object ends", (mn, AVG24, mx), objs)]


# ---- 7. batch shape --------------------------------------------------------------------------------------

def _chunky(name, key, count=None, size=None):
    """An object of `count` chunks, or of `size` bytes, under (48, 2^24, 256): chunks of 48 to
    256 bytes closed by MARKER, every fifth one 256 bytes without (a forced cut), and a tail
    of 1 to 47 bytes."""
    rng = np.random.default_rng([7, *key])
    ends, s, k = [], 0, 0
    while (count is not None and k < count - 1) or (size is not None and size - s > 256 + 47):
        n = 256 if k % 5 == 4 else int(rng.integers(48, 257))
        if k % 5 != 4:
            ends.append(s + n - 1)
        s, k = s + n, k + 1
    if size is not None:                                          # one more marked chunk, so that the tail fits
        n = size - s - 23 if size - s - 23 >= 48 else size - s - 1
        ends.append(s + n - 1)
        s += n
        tail = size - s
    else:
        tail = int(rng.integers(1, 48))
    assert 1 <= tail <= 47
    return marked(name, s + tail, ends, (7, *key))


@functools.lru_cache(maxsize=None)
def family7():
    """(48, 2^24, 256).  One batch add whose first workgroup (four waves, one per live span)
    holds objects of 1, 2, 70 and 300 chunks, then a span shorter than min, empty spans in
    between; a second batch add of five equal objects; the echo.  And those five through
    add_stream, so that both forms of the cut kernel make the same cuts."""
    params = (48, AVG24, 256)
    first = [marked("object 0: 1 chunk", 100, [], (7, 0)), _chunky("object 1: 2 chunks", (1,), count=2),
             _chunky("object 2: 70 chunks", (2,), count=70), _chunky("object 3: 300 chunks", (3,), count=300),
             marked("object 4: shorter than min", 20, [], (7, 4))]
    five = [_chunky(f"object {5 + j}: equal length {j}", (5 + j,), size=3001) for j in range(5)]
    return [Part("7 batch shape", params, first + five,
                 [("batch", [0, None, 1, 2, None, 3, 4, None]), ("batch", [5, None, 6, 7, 8, None, 9])]),
            Part("7 batch shape, the five as a stream", params, five, [("stream", [0, 1, 2, 3, 4])])]


FAMILIES = {1: family1, 2: family2, 3: family3, 4: family4, 5: family5, 6: family6, 7: family7}
# the family built for each wrong rule: there the rule must change a cut (for the last rule, which moves no
# cut, the forced count)
BUILT_FOR = {"lo_plus_1": 2, "no_low_mask": 2, "no_high_mask": 3, "round0_only": 1, "highest_bit": 5,
             "lane63_dropped": 1, "lane0_later_dropped": 1, "high_half_lost": 1, "forced_at_cap_eq_len": 6}


# the parts by name, so that a test file can be collected without building them
PART_NAMES = ("1 lane x round x bit", "2 low mask", "3 high mask", "4 one word", "4 one word, min = max = 37",
              "4 one word, min = max = 64", "5 order, four rounds", "5 order, runs of byte 57", "6 object ends",
              "7 batch shape", "7 batch shape, the five as a stream")


def parts():
    return [p for f in FAMILIES.values() for p in f()]


def part(name):
    return next(p for p in FAMILIES[int(name.split()[0])]() if p.name == name)


# ---- 8. beyond 2^32 -----------------------------------------------------------------------------------------

BIG_PARAMS = (2048, AVG24, 1 << 30)


def big_case(granules):
    """(length, marker ends) of a zero object of `granules` 4 KiB granules: MARKER ends 5000
    bytes below 2^32, 5 bytes above it and 100 bytes before the object's end."""
    n = granules * 4096
    return n, [(1 << 32) - 5000, (1 << 32) + 5, n - 1 - 100]


def zero_fields(n, ends, params):
    """The six fields for n zero bytes with MARKER ending at `ends`, by the sparse cut rule.
    Zeros are no candidate at 24 bits, and a marker lies whole in the chunk it closes or
    whole in a later one, so a chunk is its length and where the markers end in it."""
    mn, _avg, mx = params
    ends = sorted(ends)
    assert all(b - a >= 32 for a, b in zip(ends, ends[1:])) and ends[0] >= 31 and ends[-1] < n
    out, forced = R.cuts_sparse(ends, n, mn, mx)
    seen = {}
    for s, e in out:
        inside = tuple(p - s for p in ends if s <= p <= e)
        assert all(p >= 31 for p in inside) and not any(p - 31 <= e < p for p in ends)
        seen[(e - s + 1, inside)] = e - s + 1
    return (n, len(out), len(seen), sum(seen.values()), len(ends), forced)
