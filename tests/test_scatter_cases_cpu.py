"""The cases of tests/_scatter_cases.py are what they claim (no GPU): every
kernel instantiation, refusal and kind of seam of csrc/scatter_max.hip occurs,
the witness data makes every seam row count, and the reference agrees with the
oracle where the oracle is defined."""
import numpy as np
import pytest

import _scatter_cases as SC
from oracle import gnn_oracle as gn

CUS = SC.CPU_TEST_CUS
RUNNABLE = SC.runnable(SC.MAX_CASES)
STRIDE = SC.grid_stride_cases(CUS)
_MODELS = {}


def model(c):
    if c.name not in _MODELS:
        _MODELS[c.name] = SC.Model(c, CUS)
    return _MODELS[c.name]


def test_names_are_unique_and_inputs_small():
    names = [c.name for c in SC.MAX_CASES + STRIDE]
    assert len(set(names)) == len(names)
    for c in SC.MAX_CASES + STRIDE:
        assert (c.n_rows + 1) * c.ld_data * 4 <= 2.6e6, c.name
        assert c.n_seg >= 1 and c.n_rows >= 1, c.name
    for n in SC.ONE_PATTERN_CASES:
        assert n in names


def test_dispatch_at_the_launcher_thresholds():
    """The restated launcher at the column counts beside each of its tests
    (scatter_max.hip:227-250)."""
    d = SC.dispatch
    for n_cols, want in ((4, (4, 1, 16)), (256, (4, 1, 16)), (260, (4, 2, 8)),
                         (512, (4, 2, 8)), (516, (4, 4, 4)),
                         (1024, (4, 4, 4)), (1028, (4, 8, 2)),
                         (2048, (4, 8, 2)), (2052, "unsupported"),
                         (1, (1, 1, 16)), (63, (1, 1, 16)), (65, (1, 4, 8)),
                         (255, (1, 4, 8)), (257, (1, 16, 2)),
                         (1023, (1, 16, 2)), (1025, "unsupported")):
        assert d(n_cols, n_cols, n_cols) == want, n_cols
    assert d(64, 65, 64) == (1, 1, 16)
    assert d(256, 256, 256, 1, 0) == (1, 4, 8)
    assert d(256, 256, 256, 0, 1) == (1, 4, 8)
    assert d(256, 256, 256, 4, 8) == (4, 1, 16)
    assert d(1024, 1024, 1025) == (1, 16, 2)
    assert d(300, 304, 300, 1, 0) == (1, 16, 2)
    assert d(300, 300, 304) == (4, 2, 8)
    assert d(1028, 1028, 1028, 1, 0) == "unsupported"
    assert d(300, 300, 296) == "invalid" and d(300, 296, 300) == "invalid"


def test_rows_per_wave_model():
    r = SC.resolve_rpw
    assert r(333, 16, 0, 256) == 32                   # the lower clamp
    assert r(500000, 16, 0, 256) == 256               # ceil(244.1 / 16) * 16
    assert r(500000, 4, 0, 256) == 248
    assert r(10 ** 8, 8, 0, 256) == 4096              # the upper clamp
    assert r(100, 16, 1, 256) == 16 and r(100, 2, 1, 256) == 2
    assert r(100, 8, 9, 256) == 9 and r(100, 16, 33, 256) == 33
    assert SC.partition(70, 33, 16) == [(0, 33), (33, 66), (66, 70)]
    # the small cases do not depend on the device: the same chunks anywhere
    for c in RUNNABLE:
        b = SC.case_dispatch(c)[2]
        assert len({SC.resolve_rpw(c.n_rows, b, c.rpw_tunable, cus)
                    for cus in (64, 256, 304)}) == 1, c.name


def test_runs_model_on_a_hand_made_list():
    ids = np.array([-1, -1, 0, 0, 1, 1, 1, 1, 1, 2, 9, 9], np.int32)
    got = SC.runs(ids, [(0, 4), (4, 8), (8, 12)], 1, 3)
    assert got == [(-1, 0, 2, "ignored"), (0, 2, 4, "store"),
                   (1, 4, 8, "atomic"),             # continues past r1 = 8
                   (1, 8, 9, "atomic"),             # continues from r0 = 8
                   (2, 9, 10, "store"), (9, 10, 12, "ignored")]
    assert all(k in ("atomic", "ignored")
               for _, _, _, k in SC.runs(ids, [(0, 12)], 0, 3))
    assert list(SC.edge_rows([(0, 5), (5, 7)], 2, [(0, 0, 7, "atomic")])) == \
        [0, 1, 2, 3, 4, 5, 6]
    assert list(SC.edge_rows([(0, 10)], 4, [(0, 0, 6, "store"),
                                            (1, 6, 10, "store")])) == \
        [0, 3, 4, 5, 6, 7, 8, 9]


def test_every_instantiation_both_ends_sorted_and_nt():
    for inst in SC.INSTANTIATIONS:
        for n_cols, kw in SC.COLS[inst]:
            hits = [c for c in RUNNABLE if SC.case_dispatch(c) == inst
                    and c.n_cols == n_cols
                    and all(getattr(c, k) == v for k, v in kw.items())]
            assert hits, (inst, n_cols)
            assert {(c.sorted, c.nt) for c in hits} >= {
                (0, 0), (0, 1), (1, 0), (1, 1)}, (inst, n_cols)
        # the column range's two ends are those of the launcher
        cols = [n for n, _ in SC.COLS[inst]]
        step = inst[0]
        assert SC.dispatch(cols[0] - step, cols[0] - step,
                           cols[0] - step) != inst
        assert SC.dispatch(cols[-1] + step, cols[-1] + step,
                           cols[-1] + step) != inst


def test_refusals_occur():
    got = {c.name: SC.case_dispatch(c) for c in SC.refused(SC.MAX_CASES)}
    assert got == {"refuse_c2052_aligned": "unsupported",
                   "refuse_c1025": "unsupported",
                   "refuse_c1028_dataoff1": "unsupported",
                   "refuse_ldout_below_ncols": "invalid"}
    assert set(got) == set(SC.REFUSAL_TEXT)
    c = {c.name: c for c in SC.MAX_CASES}
    # both exits: the vector one and the scalar one
    assert c["refuse_c2052_aligned"].n_cols % 4 == 0
    assert c["refuse_c1028_dataoff1"].n_cols % 4 == 0 and \
        c["refuse_c1028_dataoff1"].data_off % 4 != 0


def test_three_ways_of_300_columns():
    c = {c.name: c for c in SC.MAX_CASES}
    for s in (0, 1):
        assert SC.case_dispatch(c["c300_aligned_s%d" % s]) == (4, 2, 8)
        assert SC.case_dispatch(c["c300_lddata304_off1_s%d" % s]) == (1, 16, 2)
        assert SC.case_dispatch(c["c300_ldout304_s%d" % s]) == (4, 2, 8)
        assert c["c300_ldout304_s%d" % s].ld_out == 304
    assert SC.case_dispatch(c["c256_outoff1_s1"]) == (1, 4, 8)


def _classes(m):
    """The run classes of a sorted case."""
    got = set()
    r0s = {r0 for r0, _ in m.chunks}
    r1s = {r1 for _, r1 in m.chunks}
    starts, ends = r0s - {0}, r1s - {m.case.n_rows}   # those with a neighbour
    for _, a, b, kind in m.runs:
        if kind == "ignored":
            continue
        if a not in r0s and b not in r1s and kind == "store":
            got.add("interior store")
        if a in starts:
            got.add(kind + " at r0")
        if b in ends:
            got.add(kind + " at r1")
    # one segment in at least 3 chunks running
    seg_chunks = {}
    for ci, (r0, r1) in enumerate(m.chunks):
        for s in np.unique(m.ids[r0:r1]):
            if 0 <= s < m.case.n_seg:
                seg_chunks.setdefault(int(s), []).append(ci)
    if any(len(v) >= 3 for v in seg_chunks.values()):
        got.add("run over 3 chunks")
    if m.chunks[-1][1] - m.chunks[-1][0] < m.batch:
        got.add("last chunk shorter than BATCH")
    if m.rpw % m.batch:
        got.add("rpw no multiple of BATCH")
    return got


def test_run_classes_occur_in_sorted_cases():
    want = {"interior store", "store at r0", "atomic at r0", "store at r1",
            "atomic at r1", "run over 3 chunks",
            "last chunk shorter than BATCH", "rpw no multiple of BATCH"}
    per_inst = {inst: set() for inst in SC.INSTANTIATIONS}
    for c in RUNNABLE:
        if c.sorted:
            per_inst[SC.case_dispatch(c)] |= _classes(model(c))
    for inst, got in per_inst.items():
        assert got >= want, (inst, sorted(want - got))


def test_id_recipes_are_what_they_say():
    seen = set()
    for c in RUNNABLE:
        m = model(c)
        ids, k = m.ids, c.recipe[0]
        seen.add((k, c.sorted))
        if c.sorted:
            assert np.all(np.diff(ids) >= 0), c.name
        if k == "own":
            assert len(np.unique(ids)) == c.n_rows == c.n_seg
        elif k == "gaps":
            used = np.unique(ids)
            assert used[0] > 0 and used[-1] < c.n_seg - 1
            assert np.all(np.diff(used) == 2)
        elif k == "oob":
            assert ids[0] < 0 and ids[-1] >= c.n_seg
            assert np.any((ids >= 0) & (ids < c.n_seg))
        elif k == "all_oob":
            assert not np.any((ids >= 0) & (ids < c.n_seg))
            assert ids[0] < 0 and ids[-1] >= c.n_seg
        elif k == "minus1":
            assert ids[0] == -1 and ids[-1] == c.n_seg - 1
        elif k == "random_oob":
            assert ids.min() < 0 and ids.max() >= c.n_seg
    assert seen >= {(k, 1) for k in SC.SORTED_KINDS}
    assert seen >= {("random", 0), ("random_oob", 0), ("shuffled", 0),
                    ("period", 0)}
    # a run cut exactly at r0 and one continuing across it, by name
    c = {c.name: c for c in SC.MAX_CASES}
    for n_cols in (300, 65):
        kinds = {k for _, _, _, k in model(c["ids_period_32_0_c%d" % n_cols]).runs}
        assert kinds == {"store"}
        m = model(c["ids_period_32_16_c%d" % n_cols])
        kinds = {k for _, a, b, k in m.runs if a > 0 and b < m.case.n_rows}
        assert kinds == {"atomic"}       # all but the list's first and last


def test_rows_and_tunables_per_instantiation():
    for inst in SC.INSTANTIATIONS:
        b = inst[2]
        mine = [c for c in RUNNABLE if SC.case_dispatch(c) == inst]
        assert {c.n_rows for c in mine} >= {1, b - 1, b, b + 1} - {0}
        assert {c.rpw_tunable for c in mine if c.sorted} >= {
            0, 1, b, b + 1, 32, 33}
        # a range shorter than a batch: clamped duplicate rows
        assert any(r1 - r0 < b for c in mine for r0, r1 in model(c).chunks)


def test_grid_stride_cases_stride():
    assert [SC.case_dispatch(c) for c in STRIDE] == [(4, 1, 16), (1, 1, 16)]
    for c in STRIDE:
        m = model(c)
        assert m.rpw == 16
        assert len(m.chunks) > 4 * 8 * CUS
        assert m.strides
    for c in RUNNABLE:
        assert not model(c).strides, c.name


@pytest.mark.parametrize("c", RUNNABLE + STRIDE, ids=lambda c: c.name)
def test_witness_property(c):
    """Each edge row with an id in range is the sole maximum of its segment in
    some column under some seed; pad-free, distinct, mixed sign."""
    m = model(c)
    datas = m.witness()
    assert 1 <= len(datas) <= 48, len(datas)
    ok = (m.ids >= 0) & (m.ids < c.n_seg)
    need = m.edges[ok[m.edges]]
    got = SC.witnessed_rows(datas, m.ids, c.n_seg)
    assert np.isin(need, got).all(), (c.name, np.setdiff1d(need, got)[:8])
    for d in datas:
        assert d.dtype == np.float32 and d.shape == (c.n_rows, c.n_cols)
        assert np.isfinite(d).all()
        if d.size > 8:
            assert (d > 0).any() and (d < 0).any()
    # both branches of the float atomic max meet in one cell: some segment
    # made of two or more atomic runs has a cell with a run maximum of either
    # sign (checked where there is such a segment and more than a few rows)
    atomic = {}
    for s, a, b, kind in m.runs:
        if kind == "atomic":
            atomic.setdefault(s, []).append((a, b))
    multi = [v for v in atomic.values() if len(v) >= 2]
    if multi and c.n_rows >= 64:
        met = False
        for d in datas:
            for v in multi:
                tops = np.stack([d[a:b].max(0) for a, b in v])
                met |= bool(((tops >= 0).any(0) & (tops < 0).any(0)).any())
        assert met, c.name


def test_reference_equals_the_oracle_where_it_is_defined():
    n = 0
    for c in RUNNABLE:
        m = model(c)
        if not np.all((m.ids >= 0) & (m.ids < c.n_seg)):
            continue
        d = m.witness()[0]
        assert np.array_equal(SC.reference(d, m.ids, c.n_seg),
                              gn.scatter_max(d, m.ids, c.n_seg)), c.name
        n += 1
    assert n > 100


def test_reference_on_out_of_range_ids_and_special_values():
    d = np.array([[1.0], [7.0], [-np.inf], [9.0], [-0.0]], np.float32)
    ref = SC.reference(d, np.array([0, -1, 1, 3, 2]), 3)
    assert ref[0, 0] == 1.0 and ref[1, 0] == SC.LOWEST
    assert ref[2, 0] == 0.0
    assert SC.canonical_bits(ref)[2, 0] == 0            # +0.0
    assert SC.canonical_bits(ref)[1, 0] == 0xFF7FFFFF   # lowest()


@pytest.mark.parametrize("n_cols", [4, 3])
def test_special_segments_take_both_paths(n_cols):
    data, ids = SC.special_input(n_cols)
    kinds = {}
    for v in SC.SPECIAL_VARIANTS:
        c = SC.special_case(n_cols, v)
        m = SC.Model(c, CUS)
        assert np.array_equal(m.ids, ids)
        for s, _, _, kind in m.runs:
            kinds.setdefault(s, set()).add(kind)
        by_kind = {k: {s for s, _, _, kk in m.runs if kk == k}
                   for k in ("store", "atomic")}
        if v[0] == "sorted":                 # 32 rows per wave: 10 * 3 + 2
            assert by_kind["atomic"] == {10}
        if v[0] == "sorted_batch":           # 16 rows per wave: 5 * 3 + 1
            assert m.rpw == 16 and by_kind["atomic"] == {5, 10}
        if v[0] == "sorted_rpw33":           # a cut between two segments
            assert by_kind["atomic"] == set() and len(m.chunks) == 2
        if v[0] == "unsorted":
            assert by_kind["store"] == set()
    assert all(kinds[s] == {"store", "atomic"}
               for s in range(len(SC.SPECIAL_SEGMENTS)))
    # the table holds what the issue lists
    flat = data[:, 0].view(np.uint32)
    for v in (-0.0, 0.0, -np.inf, np.inf, SC.LOWEST, SC.FLT_MAX, 1.4e-45,
              -1.4e-45, 1e-39, -1e-39):
        assert np.float32(v).view(np.uint32) in flat, v
    assert not np.isnan(data).any()
    assert SC.DENORM_MIN.view(np.uint32) == 1 and 0 < SC.DENORM < 1.1754944e-38


def test_sum_cases():
    cases = SC.sum_cases(CUS)
    assert {c.n_cols for c in cases} >= {1, 37, 300}
    assert any(c.n_rows * c.n_cols > 256 * 16 * CUS for c in cases)
    assert any(c.n_seg * c.n_cols > 256 * 4096 for c in cases)
    for c in cases:
        assert c.ld_data > c.n_cols and c.ld_out > c.n_cols
        assert (c.n_rows * c.ld_data + c.n_seg * c.ld_out) * 4 < 6e6
        data, ids, s, cnt = SC.sum_input(c)
        assert ids.min() == -2 and ids.max() == c.n_seg + 2
        assert cnt[0] == 0 and cnt[-1] == 0 and cnt[1] == 1
        assert np.all(data == np.round(data)) and np.abs(data).max() <= 8
        assert np.abs(s).max() < 2 ** 24 and cnt.sum() < c.n_rows
