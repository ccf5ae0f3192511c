"""CPU: the cases of tests/region_run_cases.py do what the GPU tests of the
extract and NPZ kernels rely on.  The launch of k_tfx_regions and k_npz_regions
on 256 CUs has 4096 waves; tfv_run is restated for them: every wave takes a run
of more than one region, some run starts inside a long record (g != 0 at its
first step), runs cross take and archive boundaries and stretches of entries
without regions of every listed length, and no flip target is the first entry
of a run, where the one binary search would find it."""
import numpy as np

import region_run_cases as R


def run_entries(reg0, lo, hi):
    """The entries a wave visits for regions [lo, hi), skipped ones included."""
    return R.owner(reg0, lo), R.owner(reg0, hi - 1)


def zero_stretches(reg0, first, last):
    """Lengths of the stretches of entries without regions strictly inside [first, last]."""
    out, n = set(), 0
    for j in range(first + 1, last):
        if reg0[j + 1] == reg0[j]:
            n += 1
        else:
            out.add(n)
            n = 0
    out.add(n)
    return out - {0}


def test_restatements():
    assert [R.region_rows(t) for t in (0, 4096 * 32, 4096 * 33 - 1, 4096 * 45, 4096 * 256 - 1, 4096 * 256, 1 << 40)] == \
        [32, 32, 32, 45, 255, 256, 256]
    assert [R.rec_regions(n, 32) for n in (0, 1, R.REGION - 15, R.REGION + 1008, R.REGION + 1009, 3 * R.REGION + 5)] == [1, 1, 1, 1, 2, 3]
    assert R.rec_regions(4096 * R.REGION + 2 * R.KiB + 5, 32) == 2049 and R.rec_regions(4096 * R.REGION + 1008, 32) == 4096
    per, rs = R.runs(10, 4)
    assert per == 3 and rs == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert R.runs(4, 8) == (1, [(0, 1), (1, 2), (2, 3), (3, 4)])
    reg0 = np.array([0, 0, 2, 2, 2, 5])
    assert [R.owner(reg0, r) for r in range(5)] == [1, 1, 4, 4, 4]
    assert R.no_run_starts_in(reg0, 4, 4) is False and R.no_run_starts_in(reg0, 4, 6) and not R.no_run_starts_in(reg0, 0, 2)


def test_extract_case():
    c = R.extract_case()
    reg0, per = c["reg0"], c["per"]
    nreg = int(reg0[-1])
    assert c["rows"] == 32 and nreg > 3 * 16 * 256 and per >= 2 and len(c["lens"]) == 20000
    assert [t[:2] for t in c["takes"]] == [(0, 1), (1, 16), (17, 0), (17, 4983), (5000, 1), (5001, 6999), (12000, 7999), (19999, 1)]
    assert sum(int(c["lens"][i]) in (R.REGION + 1009, 3 * R.REGION + 5) for i in R.LONG_AT) == len(R.LONG_AT) == 30
    _, rs = R.runs(nreg)
    inside = takes_crossed = 0
    stretches = set()
    for lo, hi in rs:
        first, last = run_entries(reg0, lo, hi)
        inside += reg0[first] != lo                                  # g != 0 at the run's first step
        takes_crossed += c["ent_take"][first] != c["ent_take"][last]
        stretches |= zero_stretches(reg0, first, last)
    assert inside >= 1 and takes_crossed >= 3
    assert stretches == {6999}                                       # the refused take's entries, stepped over by one run
    # the refused take has no regions, and the runs on both sides of it meet inside one wave
    refused = np.flatnonzero(c["ent_take"] == R.REFUSED)
    assert reg0[refused[0]] == reg0[refused[-1] + 1] and reg0[refused[0]] % per != 0
    assert len({r for r, _, _ in c["flips"]}) == 5 and [f[1] for f in c["flips"]][:3] == ["length", "data", "length_crc"]
    rec_ent = {int(r): j for j, r in enumerate(c["ent_rec"]) if c["ent_take"][j] != R.REFUSED}
    for rec, _, _ in c["flips"][:3]:
        assert R.no_run_starts_in(reg0, rec_ent[rec], per)
    assert reg0[rec_ent[c["flips"][1][0]] + 1] - reg0[rec_ent[c["flips"][1][0]]] == 3     # a record the fold launch finishes
    assert c["flips"][3][0] == 12000 and c["flips"][4][0] == 19999


def test_npz_case():
    c = R.npz_case()
    reg0, per, ent, sizes = c["reg0"], c["per"], c["ent"], c["sizes"]
    nreg = int(reg0[-1])
    assert c["rows"] == 32 and nreg > 3 * 16 * 256 and per >= 2 and len(ent) == 20000
    assert sorted(c["order"]) == list(range(R.ARCHIVES)) and c["order"] != sorted(c["order"])
    k0, k1 = c["order"][0], c["order"][-1]
    assert sizes[k0, 0] == 0 and sizes[k1, -1] == 0 and ent[0] == (k0, 0) and ent[-1] == (k1, R.MEMBERS - 1)
    longs = [int(n) for n in sizes.ravel() if n >= R.REGION]
    assert 25 <= len(longs) <= 40 and set(longs) == {R.REGION + 1, 2 * R.REGION + 17}
    assert sum(m[2] is None for ms, _ in c["specs"] for m in ms) > 2000 and {s for _, s in c["specs"]} == {0, 1}
    assert {len(m[0]) for ms, _ in c["specs"] for m in ms} == set(range(1, 17)) and set(c["a"]) == set(range(16))
    _, rs = R.runs(nreg)
    inside = archives_crossed = 0
    stretches = set()
    for lo, hi in rs:
        first, last = run_entries(reg0, lo, hi)
        inside += reg0[first] != lo
        archives_crossed += ent[first][0] != ent[last][0]
        stretches |= zero_stretches(reg0, first, last)
    assert inside >= 1 and archives_crossed >= 100 and {1, 2, 3} <= stretches
    at = {e: j for j, e in enumerate(ent)}
    assert len(c["targets"]) == 16 and len({k for k, _ in c["targets"]}) == 16
    assert [c["a"][at[t]] for t in c["targets"]] == list(range(16))
    for t in c["targets"]:
        assert R.no_run_starts_in(reg0, at[t], per) and sizes[t] >= 40
    k, j = c["behind_three"]
    assert not sizes[k, j - 3:j].any() and sizes[k, j - 4] and sizes[k, j] and k not in {t[0] for t in c["targets"]}
    k, j = c["last_full"]
    assert sizes[k, j] and all(sizes[e] == 0 for e in ent[at[(k, j)] + 1:]) and k not in {t[0] for t in c["targets"]}
