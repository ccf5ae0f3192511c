"""CPU: the TFRecord fuzz's case generator (tests/tfrecord_fuzz_cases.py)
without a GPU.  Every seed that tests/test_gpu_tfrecord_fuzz.py runs is held
to the written checklist below, computed from the lengths alone with the
restatement of the plan the GPU test files use (call_rows; regions of a record
= max(1, ceil(((len + 15) // 1024) / rows))), so that what the fuzz is meant to
bring together does occur in every seed that runs; the judge's streams parse
back and walk complete; and every flip's expected class follows from the
byte's position alone."""
import numpy as np
import pytest

import tfrecord_fuzz_cases as F
import tfrecord_var_restatement as J
from test_gpu_tfrecord_var import call_rows, parse

KiB = 1024


@pytest.fixture(scope="module", params=F.SEEDS)
def case(request):
    return F.draw(request.param)


def test_draws_are_deterministic():
    assert F.draw(1).describe() == F.draw(1).describe()
    assert F.draw(1).describe() != F.draw(2).describe()
    assert len(set(F.SEEDS)) == len(F.SEEDS) >= 6


def test_the_mixture():
    """The shares of the length classes in 5000 draws, within four standard
    deviations of a binomial around the written shares."""
    import random
    rnd = random.Random(99)
    lens = np.array([F.length(rnd) for _ in range(F.RECORDS)])
    edge = np.zeros(len(lens), bool)
    for m in (1, 2, 3):
        for d in F.REGION_DELTAS:
            edge |= lens == m * 32 * KiB + d
    shares = {
        "zero": (0.15, lens == 0),
        "below a piece": (0.15, (lens >= 1) & (lens <= 15)),
        "region edges": (0.178, edge),
        "100-300 KiB": (0.02, (lens >= 100 * KiB) & (lens <= 300 * KiB)),
        "1-3 MiB": (0.002, lens >= 1024 * KiB),
    }
    for name, (p, hit) in shares.items():
        # the 1 KiB and log-uniform classes can land on another class's values: a little room above
        dev = 4 * (F.RECORDS * p * (1 - p)) ** 0.5
        assert F.RECORDS * p - dev <= int(hit.sum()) <= F.RECORDS * p + dev + 25, (name, int(hit.sum()))
    rows = (lens[~edge & (lens > 4096) & (lens < 40 * KiB)] + 17) // KiB
    assert set(rows.tolist()) >= set(range(5, 32))           # r KiB + d over the whole range of r
    assert int(lens.max()) <= 3 * 1024 * KiB


def test_the_draw_is_valid(case):
    text = case.describe()
    a = case.layout(build=False)
    n = len(case.lists)
    assert 1 <= n <= F.MAX_SHARDS and F.RECORDS <= sum(len(l) for l in case.lists), text
    # the layout: multiples of 16, disjoint, gaps of 16-48 bytes
    for arena, size in ((0, lambda l: int(l.sum())), (1, lambda l: int(l.sum()) + 16 * len(l)), (3, lambda l: 16 * len(l))):
        used = sorted((sh[arena], size(sh[2])) for k, sh in enumerate(a.shards) if arena or k not in case.twins)
        assert all(off % 16 == 0 for off, _ in used) and used[0][0] == 16, text
        assert all(16 <= b[0] - F.up16(a_[0] + a_[1]) <= 48 for a_, b in zip(used, used[1:])), text
    for k, j in case.twins.items():
        assert j < k and a.shards[k][0] == a.shards[j][0] and np.array_equal(case.lists[k], case.lists[j]), text
    # the split: three to five calls over every shard once, uniform calls of equal lengths only
    assert 3 <= len(case.calls) <= 5 and sorted(k for _, ks in case.calls for k in ks) == list(range(n)), text
    assert {kind for kind, _ in case.calls} == {"uniform", "var"}, text
    for kind, ks in case.calls:
        assert kind == "var" or all(a.is_uniform(k) for k in ks), text
    # the flips: at most one per byte, at most 6 records per shard, inside their record
    assert len({f[:3] for f in case.flips}) == len(case.flips) > 0, text
    for k in range(n):
        assert len({i for kk, i, *_ in case.flips if kk == k}) <= 6, text
    for k, i, off, bit, cls in case.flips:
        assert 0 <= i < len(case.lists[k]) and 0 <= off < 16 + int(case.lists[k][i]) and 0 <= bit < 8, text
    # the walks' spans: cut by 1-19 bytes where there are that many, extended by 1-11 into the gap
    cut = [d for d in case.deltas.values() if d < 0]
    assert cut and len(cut) < len(case.deltas) and all(-19 <= d <= 11 and d for d in case.deltas.values()), text
    for k, d in case.deltas.items():
        assert a.framed(k) + d >= 0, text


def test_the_checklist(case):
    text = case.describe()
    lists = [[int(x) for x in l] for l in case.lists]
    # every call's region is 32 rows, and so is that of the whole list in one call
    assert call_rows(lists) == F.REGION_ROWS and sum(x // KiB for l in lists for x in l) < F.ROWS_LIMIT, text
    for _, ks in case.calls:
        assert call_rows([lists[k] for k in ks]) == F.REGION_ROWS, text
        assert sum(len(lists[k]) for k in ks) > 0, text              # every call of the split is non-empty
    reg = [[F.regions(x) for x in l] for l in lists]
    assert all(r == max(1, -(-((x + 15) // KiB) // 32)) for l, rl in zip(lists, reg) for x, r in zip(l, rl))
    assert sum(map(sum, reg)) > 4096, text                           # at 256 CUs every wave's run holds two regions or more
    assert sum(r > 1 for rl in reg for r in rl) >= 100, text
    beside = sum(1 for l, rl in zip(lists, reg) for j in range(len(l) - 1)
                 if (l[j] == 0 and rl[j + 1] > 1) or (l[j + 1] == 0 and rl[j] > 1))
    assert beside >= 20, text
    # a shard's end and an empty shard strictly inside a list: the whole list's and a var call's
    for order in [list(range(len(lists)))] + [ks for kind, ks in case.calls if kind == "var"][:1]:
        live = [j for j, k in enumerate(order) if lists[k]]
        assert len(live) >= 2, text
    whole = [j for j, l in enumerate(lists) if l]
    assert any(not lists[j] for j in range(whole[0], whole[-1])), text
    inside = 0
    for kind, ks in case.calls:
        live = [j for j, k in enumerate(ks) if lists[k]]
        inside += kind == "var" and any(not lists[ks[j]] for j in range(live[0], live[-1]))
    assert inside >= 1, text
    pre = set()
    for l in lists:
        pre |= set((np.concatenate(([0], np.cumsum(l[:-1]))).astype(np.int64) % 16).tolist()) if l else set()
    assert pre == set(range(16)), text


def test_the_judge_parses_and_walks(case):
    """J.frame's streams parse back to the payload, and J.walk finds every
    record of every framed shard."""
    a = case.layout()
    for k, (s_off, d_off, l, i_off) in enumerate(a.shards):
        framed = a.framed(k)
        stream = a.dst[d_off:d_off + framed].tobytes()
        recs = parse(stream, l.tolist())
        assert b"".join(recs) == a.src[s_off:s_off + int(l.sum())].tobytes(), (case.seed, k)
        w = J.walk(stream)
        assert (w["records"], w["status"], w["stop_offset"], w["trailing"], w["bad_length_crc"]) == (len(l), 0, framed, 0, 0)
        assert np.array(w["entries"], "<u8").tobytes() == a.idx[i_off:i_off + 16 * len(l)].tobytes(), (case.seed, k)
        if framed:
            assert a.record_at(d_off) == (k, 0) and a.record_at(d_off + framed - 1) == (k, len(l) - 1)
        assert a.record_at(d_off + framed) == (k, None)


def test_a_flip_s_class_follows_from_its_position(case):
    """Bytes 0-7 of a framed record are its length, 8-11 the length's CRC, the
    rest data and footer; the flip's place in the arena is inside that record."""
    a = case.layout(build=False)
    for k, i, off, bit, cls in case.flips:
        l = case.lists[k]
        n = int(l[i])
        assert cls == F.flip_class(off) == (0 if off < 8 else 1 if off < 12 else 2)
        assert (cls == 2) == (12 <= off < 16 + n)
        pos = a.shards[k][1] + int(l[:i].sum()) + 16 * i + off
        assert a.record_at(pos) == (k, i)
