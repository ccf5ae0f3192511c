"""The pure case builders of tests/test_gpu_tfrecord_extract_edges.py and
tests/test_gpu_npz_batch_edges.py: lengths, cuts, member lists and flip targets
of calls with more regions than the launch has waves, so that a wave of
k_tfx_regions / k_npz_regions takes a run of regions and steps from entry to
entry.  No device, no library: tests/test_region_runs_cpu.py holds what the GPU
tests rely on, by a restatement of the plan's region count and of tfv_run."""
import functools
import random

import numpy as np

from oracle import npz_oracle as O

KiB = 1 << 10
REGION = 32 * KiB          # the region of a call below 128 MiB
WAVES = 4096               # 2 workgroups of 8 waves on each of 256 CUs
MAX_REGIONS = 4096         # kCrcBatchMaxRegions
DELTAS = (-17, -16, -15, -1, 0, 1, 1008, 1009, 1010)


def region_rows(total_rows):
    """crc_batch_region_rows."""
    return 256 if total_rows // 256 >= 4096 else max(32, total_rows // 4096)


def rec_regions(n, rows):
    """tfv_rec_regions(n, tfv_rec_rows(n, rows))."""
    obj = (n + 15) // KiB
    while obj > MAX_REGIONS * rows:
        rows *= 2
    return max(1, -(-obj // rows))


def take_reach(nbytes, count, cap):
    """tfx_reach."""
    return min(nbytes, cap + 16 * count) if count else 0


def runs(nreg, waves=WAVES):
    """(per, [(lo, hi)]): tfv_run_len and tfv_run of every wave with a region."""
    per = -(-nreg // waves)
    out = []
    for w in range(waves):
        lo = min(w * per, nreg)
        hi = nreg if nreg - lo < per else lo + per
        if lo < hi:
            out.append((lo, hi))
    return per, out


def owner(reg0, r):
    """The entry that owns region r of first regions reg0[0..ents]: the linear scan."""
    return int(np.searchsorted(reg0, r, side="right")) - 1


def no_run_starts_in(reg0, j, per):
    """Entry j is the first of no wave's run: no multiple of per among its regions."""
    lo, hi = int(reg0[j]), int(reg0[j + 1])
    return lo < hi and -(-lo // per) * per >= hi


def log_uniform(rng, n):
    """n lengths 0..4 KiB, log-uniform (tests/test_gpu_tfrecord_var.py::test_lists' draw)."""
    return np.floor(np.exp(rng.uniform(0, np.log(4 * KiB + 1), n))).astype(np.uint64) - np.uint64(1)


# ---- extract --------------------------------------------------------------------------------
CUTS = [0, 1, 17, 5000, 5001, 12000, 19999, 20000]
LONG_AT = list(range(331, 20000, 660))          # 30 fixed positions of long records
REFUSED = 5                                     # the take of records [5001, 12000), one byte short


@functools.lru_cache(maxsize=None)
def extract_case():
    """lens: 20 000 record lengths; takes: (first, count, short) in call order,
    an empty take among them; reg0: first regions of the call's entries;
    flips: (record, where, class) with where in length | length_crc | data |
    footer and class (bad_length, bad_length_crc, bad_data_crc)."""
    lens = log_uniform(np.random.default_rng(7), 20000)
    for q, at in enumerate(LONG_AT):
        lens[at] = REGION + 1009 if q % 2 == 0 else 3 * REGION + 5
    takes = [(a, b - a, False) for a, b in zip(CUTS, CUTS[1:])]
    takes.insert(2, (17, 0, False))             # an empty take between [1, 17) and [17, 5000)
    takes[REFUSED] = takes[REFUSED][:2] + (True,)
    assert takes[REFUSED][:2] == (5001, 6999)
    stream_bytes = int(lens.sum()) + 16 * len(lens)
    caps = [int(lens[f:f + c].sum()) - short for f, c, short in takes]
    rows = region_rows(sum(take_reach(stream_bytes, c, cap) for (_, c, _), cap in zip(takes, caps)) // KiB)
    ent_rec = np.concatenate([np.arange(f, f + c) for f, c, _ in takes])        # the call's entries: their records
    ent_take = np.concatenate([np.full(c, k) for k, (_, c, _) in enumerate(takes)])
    nr = np.array([0 if takes[k][2] else rec_regions(int(lens[i]), rows) for i, k in zip(ent_rec, ent_take)], np.int64)
    reg0 = np.concatenate([[0], np.cumsum(nr)])
    per, _ = runs(int(reg0[-1]))

    def pick(lo, hi, want):
        for j in range(lo, hi):
            if want(int(lens[ent_rec[j]]), int(nr[j])) and no_run_starts_in(reg0, j, per):
                return int(ent_rec[j])
        raise AssertionError("no such record")
    e3, e6 = int(np.flatnonzero(ent_take == 3)[0]), int(np.flatnonzero(ent_take == 6)[0])
    flips = [(pick(e3 + 100, e3 + 4000, lambda n, r: r == 1 and n >= 100), "length", (1, 0, 0)),
             (pick(e3 + 100, e3 + 4983, lambda n, r: r == 3), "data", (0, 0, 1)),
             (pick(e6 + 3000, e6 + 7000, lambda n, r: r == 1 and n >= 100), "length_crc", (0, 1, 0)),
             (12000, "data" if lens[12000] else "footer", (0, 0, 1)),       # the record after the refused take
             (19999, "footer", (0, 0, 1))]                                  # the last record of the call
    return dict(lens=lens, takes=takes, caps=caps, stream_bytes=stream_bytes, rows=rows, ent_rec=ent_rec, ent_take=ent_take,
                reg0=reg0, per=per, flips=flips)


# ---- NPZ ------------------------------------------------------------------------------------
ARCHIVES, MEMBERS = 200, 100


@functools.lru_cache(maxsize=None)
def npz_case():
    """specs: (members, style) per archive, a member (name, NPY header, src_off
    or None, size); order: the order of the call; src: the source bytes; ent:
    (archive, member) of the call's entries; reg0: their first regions; a: the
    payload's place past a 16-byte boundary per entry; targets: 16 (archive,
    member), one per a, none the first of a wave's run; behind_three: the
    member behind a run of exactly three empty members; last_full: the call's
    last member with payload."""
    sizes = log_uniform(np.random.default_rng(21), ARCHIVES * MEMBERS).astype(np.int64).reshape(ARCHIVES, MEMBERS)
    for k in range(ARCHIVES):
        row = sizes[k]
        for j in (9, 11, 19, 22, 29, 33):                  # the neighbours of the empty runs hold payload
            row[j] = row[j] or 100 + k
        if k % 3 == 0:
            row[10] = 0                                    # an empty member on its own
        elif k % 3 == 1:
            row[20:22] = 0                                 # a run of two
        else:
            row[30:33] = 0                                 # a run of three
        if k % 6 == 3:
            row[50] = REGION + 1 if k % 12 == 3 else 2 * REGION + 17
    order = list(range(ARCHIVES))
    random.Random(5).shuffle(order)
    sizes[order[0], 0] = 0                                 # the call's first and last members are empty
    sizes[order[-1], MEMBERS - 1] = 0
    specs, at = [], 0
    for k in range(ARCHIVES):
        members = []
        for j in range(MEMBERS):
            size, nl = int(sizes[k, j]), 1 + (k * MEMBERS + j) % 16
            so = None if j % 9 == 4 else at                # every ninth member is zeros without a source
            if so is not None:
                at += (size + 15) // 16 * 16
            members.append((chr(97 + j % 26) * nl, O.npy_header([size], "|u1"), so, size))
        specs.append((members, k % 2))
    src = np.random.default_rng(22).integers(0, 256, at + 16, dtype=np.uint8)
    total_rows = int((sizes // KiB).sum())
    rows = region_rows(total_rows)
    ent, nr, a = [], [], []
    for k in order:
        off = 0
        for j, (name, hdr, _, size) in enumerate(specs[k][0]):
            off += 30 + len(name) + len(hdr)
            ent.append((k, j))
            nr.append(rec_regions(size, rows) if size else 0)
            a.append(off % 16)
            off += size
    reg0 = np.concatenate([[0], np.cumsum(np.array(nr, np.int64))])
    per, _ = runs(int(reg0[-1]))
    at_ent = {e: i for i, e in enumerate(ent)}
    targets, used = [], set()
    for want in range(16):                                 # one archive per residue a
        for k in range(ARCHIVES):
            hit = [j for j in range(1, MEMBERS) if k not in used and a[at_ent[(k, j)]] == want and 40 <= sizes[k, j] < REGION
                   and no_run_starts_in(reg0, at_ent[(k, j)], per)]
            if hit:
                targets.append((k, hit[0]))
                used.add(k)
                break
    behind_three = next((k, 33) for k in range(2, ARCHIVES, 3) if k not in used and not sizes[k, 30:33].any() and sizes[k, 29])
    last_full = next(e for e, n in zip(reversed(ent), reversed(nr)) if n)
    return dict(specs=specs, order=order, src=src, sizes=sizes, rows=rows, ent=ent, reg0=reg0, a=a, per=per, targets=targets,
                behind_three=behind_three, last_full=last_full)
