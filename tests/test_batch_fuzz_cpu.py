"""CPU: the batch fuzz's case generator (tests/batch_fuzz_cases.py) without a
GPU.  Every draw of the seeds that tests/test_gpu_fuzz_batch.py runs is valid;
their union meets the written checklist below, so that what the fuzz is meant
to bring together does occur in the seeds that run; and `expected_verify`, the
judge of the batch verifies, gives hand-computed answers on hand-written
images (one of them counted a second time with the Python oracle)."""
import numpy as np
import pytest

import batch_fuzz_cases as C
from oracle import oracle_py as P

SEEDS = range(C.SEEDS)


@pytest.fixture(scope="module")
def cases():
    return [C.draw(s) for s in SEEDS]


@pytest.fixture(scope="module")
def base(golden_base):
    return np.frombuffer(golden_base, np.uint8)


def test_draws_are_deterministic():
    for s in (0, 3, 17):
        assert C.draw(s).describe() == C.draw(s).describe()
    assert C.draw(0).describe() != C.draw(1).describe()


def test_every_draw_is_valid(cases):
    for c in cases:
        text = c.describe()
        assert 1 <= len(c.writes) <= C.MAX_OBJECTS and c.arena % 16 == 0, text
        assert sum(o.size for o in c.writes) <= C.CAP, text
        assert sum(n for _, n in c.reads) <= C.CAP + C.EXTRA, text
        taken = np.zeros(c.arena, np.uint8)
        for o in c.writes:
            assert o.off % 16 == 0 and C.GUARD <= o.off and o.off + o.size <= c.arena - C.GUARD, text
            assert o.kind in C.KINDS and o.dedup in C.DEDUPS and o.compress in C.COMPRESS, text
            assert 0 <= o.entropy < 2**64, text
            taken[o.off:o.off + o.size] += 1
            if c.dense:
                assert o.off % 4096 == 0, text
        assert taken.max(initial=0) <= 1, text                       # the writes are disjoint
        if c.dense:                                                   # packed: no free granule between two objects
            used = sorted((o.off, o.size) for o in c.writes)
            assert all(b[0] == C._up(a[0] + a[1], 4096) for a, b in zip(used, used[1:])), text
        else:
            used = sorted((o.off, o.size) for o in c.writes)
            assert all(16 <= b[0] - C._up(a[0] + a[1], 16) <= 8192 for a, b in zip(used, used[1:])), text
        for off, n in c.reads:
            assert n == 0 or (off % 16 == 0 and off + n <= c.arena), text
        assert {(o.off, o.size) for o in c.writes} <= set(c.reads), text
        for kind in C.GENERATED:
            mine = {o.desc for o in c.of_kind(kind)}
            for j, d in enumerate(c.verify[kind]):
                assert d[0] % 16 == 0 and d[0] + d[1] <= c.arena, text
                assert (d in mine) != (c.wrong[kind] is not None and c.wrong[kind][0] == j), text
            if c.wrong[kind] is None:
                assert mine == set(c.verify[kind]), text
            else:
                assert len(set(c.verify[kind]) - mine) == 1 and len(mine - set(c.verify[kind])) <= 1, text
        for pos, mask, k, _mode in c.corrupt:
            o = c.writes[k]
            assert o.kind in C.GENERATED and o.off <= pos < o.off + o.size and 1 <= mask <= 255, text
        assert len({pos for pos, *_ in c.corrupt}) == len(c.corrupt) <= 6, text
        assert c.waves in C.WAVES and c.tile in C.TILES and c.measure_block in C.MEASURE_BLOCKS, text
        assert c.lz_block in C.LZ_BLOCKS and c.chunk_params in [tuple(p) for p in C.CHUNK_PARAMS], text
        assert c.uniform == (c.seed % 4 == 3), text
        if c.uniform:
            assert [r.kind for r in c.runs] == list(C.GENERATED) and not any(c.wrong.values()), text
            for r in c.runs:
                assert r.stride % 16 == 0 and r.stride >= r.size > 0 and r.n >= 1, text
                want = {(off, r.size, P.object_entropy(r.seed_base, r.first_obj + j), r.dedup, r.compress)
                        for j, (off, _) in enumerate(r.spans)}
                assert want == {o.desc for o in c.of_kind(r.kind)} == set(c.verify[r.kind]), text
                assert len(c.verify[r.kind]) == r.n, text


def near(size, unit, side):
    """`size` lies within 17 bytes below (side -1) or above (side +1) a positive multiple of `unit`."""
    r = size % unit
    return size > unit - 18 and (1 <= unit - r <= 17 if side < 0 else size > unit and 1 <= r <= 17)


def checklist(cases):
    """Name -> whether the cases hold it."""
    objs = [o for c in cases for o in c.writes]
    mixed = [c for c in cases if not c.uniform]
    have = {}
    for kind in C.KINDS:
        have[f"payload kind {kind}"] = any(o.kind == kind and o.size for o in objs)
    for name, values, got in [("waves", C.WAVES, {c.waves for c in cases}), ("tile", C.TILES, {c.tile for c in cases}),
                              ("measure block", C.MEASURE_BLOCKS, {c.measure_block for c in cases}),
                              ("hist", (False, True), {c.hist for c in cases}),
                              ("lz block", C.LZ_BLOCKS, {c.lz_block for c in cases}),
                              ("chunk parameters", [tuple(p) for p in C.CHUNK_PARAMS], {c.chunk_params for c in cases}),
                              ("dedup", C.DEDUPS, {o.dedup for o in objs if o.size}),
                              ("compress", C.COMPRESS, {o.compress for o in objs if o.size})]:
        for v in values:
            have[f"{name} {v}"] = v in got
    have["an empty object"] = any(o.size == 0 for o in objs)
    have["size 1"] = any(o.size == 1 for o in objs)
    for unit in (1024, 4096, 65536, C.MiB):
        for side in (-1, 1):
            have[f"a size just {'below' if side < 0 else 'above'} a multiple of {unit}"] = \
                any(near(o.size, unit, side) for o in objs)
    have["a DG1 object of more than one block with a ragged last block"] = \
        any(o.kind == "dg1" and o.size > C.MiB and o.size % C.MiB for o in objs)
    have["an entropy within 3 of 0"] = any(o.entropy <= 3 for o in objs)
    have["an entropy within 3 of 2^64"] = any(o.entropy >= 2**64 - 4 for o in objs)
    have["a dense layout"] = any(c.dense for c in mixed)
    have["a layout at odd 16-byte offsets"] = any(not c.dense for c in mixed)
    have["a group of objects with shared parameters"] = any(
        len({(o.size, o.entropy, o.dedup, o.compress, o.kind) for o in c.writes if o.size}) <
        len([o for o in c.writes if o.size]) for c in mixed)
    for tag in ("repeat", "sub_span", "across_gap", "empty_span"):
        have[f"a read list with {tag}"] = any(tag in c.tags for c in cases)
    have["a repeated verify descriptor"] = any(len(set(c.verify[k])) < len(c.verify[k]) for c in mixed
                                               for k in C.GENERATED)
    have["a clean case"] = any(not c.corrupt for c in cases)
    have["a mixed case with three kinds of content"] = any(len({o.kind for o in c.writes if o.size}) >= 3 for c in mixed)
    hits = [(c.writes[k], pos - c.writes[k].off) for c in cases for pos, _m, k, _mode in c.corrupt]
    have["corruption of a first byte"] = any(p == 0 for o, p in hits)
    have["corruption of a last byte"] = any(p == o.size - 1 for o, p in hits)
    have["corruption in a ragged last block"] = any(o.size % 4096 and p >= o.size - o.size % 4096 and o.size > 4096
                                                    for o, p in hits)
    have["corruption on both kinds"] = {o.kind for o, _ in hits} == set(C.GENERATED)
    for mode in C.CORRUPT_MODES:
        have[f"corruption drawn as {mode}"] = any(m == mode for c in cases for *_, m in c.corrupt)
    for field in C.WRONG_FIELDS:
        have[f"a wrong {field}"] = any(w is not None and w[1] == field for c in mixed for w in c.wrong.values())
    have["a wrong descriptor of each kind"] = {k for c in mixed for k, w in c.wrong.items() if w} == set(C.GENERATED)
    have["a case with no wrong descriptor"] = any(not any(c.wrong.values()) for c in mixed)
    have["at least four uniform cases"] = sum(c.uniform for c in cases) >= 4
    have["a uniform run of one object"] = any(r.n == 1 for c in cases for r in c.runs)
    have["a uniform run of several objects"] = any(r.n > 2 for c in cases for r in c.runs)
    return have


def test_the_seeds_meet_the_checklist(cases):
    have = checklist(cases)
    missing = [name for name, ok in have.items() if not ok]
    assert not missing, missing


# ---- expected_verify on hand-written images --------------------------------------------------

A_OFF, A_SIZE = 4096 + 16, 5000           # controlled, two 4 KiB blocks, the second ragged
B_OFF, B_SIZE = 16384 + 32, 4112          # DG1, two granules


def hand_case():
    a = C.Obj(A_OFF, A_SIZE, 77, 1, 2, "controlled")
    b = C.Obj(B_OFF, B_SIZE, 78, 1, (3, 2), "dg1")
    return C.Case(-1, False, False, False, 32768, [a, b], [], {"controlled": [a.desc, a.desc], "dg1": [b.desc]},
                  {"controlled": None, "dg1": None}, [], 0, 0, 4096, False, 4096, (32, 64, 256))


def test_expected_verify_by_hand(oracle, base):
    case = hand_case()
    clean = C.expected_image(case, oracle, base)
    inside = np.zeros(case.arena, bool)
    inside[A_OFF:A_OFF + A_SIZE] = inside[B_OFF:B_OFF + B_SIZE] = True
    assert (clean[~inside] == C.POISON).all()
    assert np.array_equal(clean[A_OFF:A_OFF + A_SIZE], np.frombuffer(P.fill_controlled(A_SIZE, 1, 1, 2, 77, bytes(base)),
                                                                     np.uint8))
    assert np.array_equal(clean[B_OFF:B_OFF + B_SIZE], np.frombuffer(P.dgen_fill(B_SIZE, 1, 1, 3, 78), np.uint8))
    for kind in C.GENERATED:
        assert C.expected_verify(clean, case, kind, oracle, base) == ((0, 0, None), {})

    # 1. one flipped byte at each object's last byte; the controlled descriptor stands twice in its list
    img = clean.copy()
    img[A_OFF + A_SIZE - 1] ^= 0x01
    img[B_OFF + B_SIZE - 1] ^= 0x80
    assert C.expected_verify(img, case, "controlled", oracle, base) == \
        ((2, 2, A_OFF + 4999), {0: (1, 1, 4999), 1: (1, 1, 4999)})
    assert C.expected_verify(img, case, "dg1", oracle, base) == ((1, 1, B_OFF + 4111), {0: (1, 1, 4111)})
    # the gap bytes are nobody's
    img = clean.copy()
    img[A_OFF - 1] ^= 0xFF
    img[A_OFF + A_SIZE] ^= 0xFF
    assert C.expected_verify(img, case, "controlled", oracle, base) == ((0, 0, None), {})

    # 2. two in one block and one in the other, one descriptor: blocks count from the object's start
    img = clean.copy()
    for p in (4100, 4200, 7):
        img[A_OFF + p] ^= 0xFF
    one = [case.verify["controlled"][0]]
    assert C.expected_verify(img, case, "controlled", oracle, base, descs=one) == ((3, 2, A_OFF + 7), {0: (3, 2, 7)})
    # bytes 4095 and 4096 of the object are two blocks, although one 4 KiB page of the arena holds both
    img = clean.copy()
    img[A_OFF + 4095] ^= 0x10
    img[A_OFF + 4096] ^= 0x10
    assert (A_OFF + 4095) // 4096 == (A_OFF + 4096) // 4096
    assert C.expected_verify(img, case, "controlled", oracle, base, descs=one) == ((2, 2, A_OFF + 4095), {0: (2, 2, 4095)})

    # 3. a second, shorter descriptor over the same bytes, listed first: the totals' offset is the lowest
    sub = (A_OFF, 4096, 77, 1, 2)                       # one block: the same first 4096 bytes (dedup 1)
    img = clean.copy()
    img[A_OFF + 4999] ^= 0xFF
    img[A_OFF + 100] ^= 0xFF
    assert C.expected_verify(img, case, "controlled", oracle, base, descs=[sub, one[0], (0, 0, 1, 1, 1)]) == \
        ((3, 3, A_OFF + 100), {0: (1, 1, 100), 1: (2, 2, 100)})


def test_expected_verify_of_a_wrong_descriptor(oracle, base):
    """A descriptor with entropy + 1 on clean bytes, counted with the Python oracle."""
    case = hand_case()
    clean = C.expected_image(case, oracle, base)
    wrong = (A_OFF, A_SIZE, 78, 1, 2)
    other = np.frombuffer(P.fill_controlled(A_SIZE, 1, 1, 2, 78, bytes(base)), np.uint8)
    bad = np.flatnonzero(clean[A_OFF:A_OFF + A_SIZE] != other)
    blocks = np.unique(bad // 4096).size
    assert bad.size >= 32 and bad[0] == 2048             # block 0's first window, behind its zero prefix
    tot, per = C.expected_verify(clean, case, "controlled", oracle, base, descs=[wrong])
    assert tot == (bad.size, blocks, A_OFF + 2048) and per == {0: (bad.size, blocks, 2048)}


def test_corrupted_applies_every_mask():
    c = C.draw(next(s for s in SEEDS if C.draw(s).corrupt))
    img = np.zeros(c.arena, np.uint8)
    out = C.corrupted(img, c)
    assert not img.any() and np.count_nonzero(out) == len(c.corrupt)
    assert all(out[pos] == mask for pos, mask, *_ in c.corrupt)
