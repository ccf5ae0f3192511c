"""The definition of content-defined chunking restated in
numpy, written from the document: G, the 32-byte window sums (vectorised), the
cut rule (a Python loop over the cuts) and `bytes` of every chunk in a dict for
the distinct counts, never a restatement of the fingerprint.  The cut rule
comes in two forms that tests/test_chunk_walk_cpu.py holds to each other: dense
(`cuts_of`, over a candidate array) and sparse (`cuts_sparse`, over a sorted
candidate list and a length, for an object that no host array can hold).  The
judge of tests/test_gpu_chunks.py, tests/test_gpu_chunk_walk.py and the CPU
files beside them; not a conftest."""
import numpy as np

FIELDS = ("bytes", "chunks", "unique_chunks", "unique_bytes", "candidates", "forced_cuts")


def _gear():
    x = (np.arange(256, dtype=np.uint64) + 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


G = _gear()


def window_hash(rows):
    """h_i for i >= 31 of every row (one object per row): shape (n, len - 31)."""
    g = G[rows]
    m = rows.shape[1] - 31
    h = np.zeros((rows.shape[0], m), np.uint32)
    for k in range(32):
        h += g[:, 31 - k:31 - k + m] << np.uint32(k)
    return h


def candidates(rows, bits):
    """Candidate cuts of equal-length objects, one per row."""
    rows = np.atleast_2d(np.ascontiguousarray(rows, np.uint8))
    n = rows.shape[1]
    cand = np.zeros(rows.shape, bool)
    step = max(1, (1 << 22) // rows.shape[0])
    for lo in range(31, n, step):
        hi = min(n, lo + step)
        cand[:, lo:hi] = (window_hash(rows[:, lo - 31:hi]) >> np.uint32(32 - bits)) == 0
    return cand


def cuts_of(cand, mn, mx):
    """The chunks [s, e] of one object, its forced cuts and the events of the cut rule met."""
    n = cand.size
    pos = np.flatnonzero(cand)
    out, forced, ev = [], 0, set()
    s = 0
    while s < n:
        lo = s + mn - 1
        if lo >= n:
            e = n - 1                                   # the object's end closes the last chunk
        else:
            if lo - 1 >= s and cand[lo - 1]:
                ev.add("skipped_before_min")
            k = int(np.searchsorted(pos, lo))
            c = int(pos[k]) if k < pos.size else None   # the smallest candidate >= s + min - 1
            if c is not None and c - s + 1 <= mx:
                e = c
                if e == lo:
                    ev.add("cut_at_min")
                if e == s + mx - 1:
                    ev.add("candidate_at_max")
            elif s + mx <= n:
                e = s + mx - 1                          # cut at max_bytes
                forced += 1
                ev.add("forced")
                if e + 1 < n and cand[e + 1]:
                    ev.add("forced_then_candidate")
            else:
                e = n - 1
        out.append((s, e))
        s = e + 1
    return out, forced, ev


def cuts_sparse(pos, n, mn, mx):
    """The cut rule over the sorted candidate offsets `pos` of an object of n bytes: its
    chunks [s, e] and its forced cuts.  Python integers throughout, so n may pass 2^32."""
    import bisect
    pos = [int(p) for p in pos]
    out, forced = [], 0
    s = 0
    while s < n:
        e = n - 1                                       # the object's end, unless a cut comes first
        if s + mn - 1 < n:
            k = bisect.bisect_left(pos, s + mn - 1)
            if k < len(pos) and pos[k] - s + 1 <= mx:
                e = pos[k]
            elif s + mx <= n:
                e = s + mx - 1
                forced += 1
        out.append((s, e))
        s = e + 1
    return out, forced


def restate(S, objs, params, events=None):
    """The result of chunking the objects (host arrays) in one handle."""
    mn, avg, mx = params
    bits = avg.bit_length() - 1
    seen = {}
    nbytes = chunks = ncand = forced = 0
    by_len = {}
    for a in objs:
        by_len.setdefault(len(a), []).append(np.ascontiguousarray(a, np.uint8))
    for n, group in by_len.items():
        rows = np.stack(group)
        cand = candidates(rows, bits)
        ncand += int(cand.sum())
        for a, c in zip(group, cand):
            out, f, ev = cuts_of(c, mn, mx)
            mv = memoryview(a)
            for s, e in out:
                seen[bytes(mv[s:e + 1])] = e - s + 1
            chunks += len(out)
            forced += f
            nbytes += n
            if events is not None:
                events |= ev
    return S.ChunkResult(nbytes, chunks, len(seen), sum(seen.values()), ncand, forced)
