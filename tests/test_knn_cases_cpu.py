"""The kNN cases reach the branches they are named for, the NumPy restatement
of the contract has the properties the device tests rely on, and the five
entries exist and validate their arguments before any HIP call.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from oracle import graph_oracle as go

import _graph_cases as GC
import _knn_cases as KC

ENTRIES = ("pgnn_knn_graph_workspace_bytes", "pgnn_knn_graph_count",
           "pgnn_knn_graph_fill", "pgnn_knn_graph_count_f64",
           "pgnn_knn_graph_fill_f64")


def _lib():
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    return L, L.load()


def _native(case):
    return KC.hoods_of(case, np.asarray(case.points).dtype)


def _fanin(hoods):
    return np.array([len(i) for i, _ in hoods])


# ---- the cases reach their branches -----------------------------------------
def test_sweep_has_every_fanin_round_every_k():
    case, ms = KC.sweep()
    fan = _fanin(_native(case))
    mid = np.arange(0, len(ms) - 2, 2)          # the mid-cell centres
    assert np.array_equal(fan[mid], ms[mid])
    assert fan[-2] == ms[-2] == KC.EXTRA_M and fan[-1] == ms[-1] == 0
    # off-middle centres: candidates that are not neighbours
    assert (fan[mid + 1] < ms[mid + 1]).sum() > 150
    have = set(fan.tolist())
    assert case.ks == KC.K_EDGES
    for k in case.ks:
        assert {0, 1, k - 1, k, k + 1} <= have, k
    # candidate totals at the chunk and double-chunk seams, fan-in the same
    grid = GC.RadiusGrid(case.points, case.r)
    for m in KC.CHUNK_TOTALS:
        q = 2 * GC.SWEEP_M.index(m)
        n_cells, total, _ = grid.query(case.centers[q])
        assert (n_cells, total, fan[q]) == (27, m, m)
        assert grid.query(case.centers[q + 1])[1] == m


def test_dense_is_many_times_every_k_in_a_64_cell_box():
    case = KC.dense()
    fan = _fanin(_native(case))
    assert fan[0] == KC.DENSE_N >= KC.MANY * KC.K_MAX
    assert max(case.ks) == KC.K_MAX and min(case.ks) == 1
    grid = GC.RadiusGrid(case.points, case.r)
    n_cells, total, _ = grid.query(case.centers[0])
    assert n_cells == 64 and total >= KC.DENSE_N > 18 * 64
    assert len(np.unique(grid.cells, axis=0)) == 8
    assert fan[-1] < fan[0]                      # a centre beside the cube


def test_lattice_r2_cuts_tied_shells_and_the_shell_at_r():
    for case in KC.lattice_r2():
        hoods = _native(case)
        q = 3 * 64 + 3 * 8 + 3                   # the interior centre (3, 3, 3)
        assert np.array_equal(np.asarray(case.points)[q], [3, 3, 3])
        assert np.bincount(hoods[q][1].astype(int)).tolist() == [1, 6, 12, 8, 6]
        for k, shell in ((4, 1.0), (10, 2.0), (30, 4.0)):
            kept, dropped = KC.cut_ties(hoods, k)[q]
            assert kept > 0 and dropped > 0 and hoods[q][1][k - 1] == shell
        assert KC.cut_ties(hoods, 33)[q] == (0, 0) and len(hoods[q][0]) == 33
        # the last shell is at exactly r, bit for bit
        assert hoods[q][1][-1] == case.r * case.r
        assert GC.exact_r_pairs(case.points, case.centers, case.r) > 0


def test_lattices_have_64_cell_boxes_exact_r_and_index_decided_cuts():
    cases = {c.name: c for c in KC.lattices()}
    assert len(cases) == len(GC.lattices())
    for tag in ("f32", "f64"):
        c = cases["lattice12_r5_" + tag]
        grid = GC.RadiusGrid(c.points, c.r)
        assert (grid.profile(c.centers)[0] == 64).any()
        assert max(_fanin(_native(c))) > 4 * c.ks[0]
        c = cases["lattice8_r1_" + tag]
        assert GC.exact_r_pairs(c.points, c.centers, c.r) > 0
        ties = KC.cut_ties(_native(c), c.ks[0])
        assert sum(d > 0 for _, d in ties) > 100   # six at exactly r, k = 4
        c = cases["lattice12_scaled_" + tag]
        assert list(c.scale) == [1.0, 2.0, 0.5]
        assert (_fanin(_native(c)) > c.ks[0]).any()


def test_duplicates_cut_inside_a_triple():
    case = KC.duplicates()
    hoods = _native(case)
    for k in case.ks:
        ties = KC.cut_ties(hoods, k)
        assert all(kept > 0 and dropped > 0 for kept, dropped in ties)
    assert all(d2[0] == 0.0 and d2[2] == 0.0 for _, d2 in hoods)


def test_tie_spans_two_chunks():
    case = KC.tie_two_chunks()
    (idx, d2), = _native(case)
    k, = case.ks
    assert len(idx) == 6 + KC.TIE_NEAR + KC.TIE_FAR
    tied = idx[d2 == 0.5625]
    assert len(tied) == 6 and d2[k - 1] == 0.5625 == d2[k]
    kept = [i for i in idx[:k] if i in tied]
    dropped = [i for i in idx[k:] if i in tied]
    assert kept == [0, 1, 2] and len(dropped) == 3
    pos, total = KC.walk_positions(case.points, case.centers[0], case.r)
    chunk = {int(i): pos[int(i)] // 64 for i in tied}
    assert total >= 156
    # kept and dropped members on both sides of at least one whole chunk
    assert sorted(chunk[i] for i in kept) == [0, 2, 2]
    assert sorted(chunk[i] for i in dropped) == [0, 0, 2]


def test_shared_bucket_boxes_are_cut():
    case, info = KC.shared_bucket()
    grid = GC.RadiusGrid(case.points, case.r)
    fan = _fanin(_native(case))
    for q, rec in enumerate(info):
        _, _, buckets = grid.query(case.centers[q])
        assert (buckets == rec["bucket"]).sum() == 2
        assert fan[q] >= 6
        kept = set(_native(case)[q][0][:4].tolist())
        assert rec["idx_far"] not in kept
    assert min(case.ks) < 6 < max(case.ks)


def test_blobs_have_no_ties_and_fanins_on_both_sides_of_k():
    for case in KC.blobs() + [KC.blob_shuffled()[0]]:
        hoods = _native(case)
        fan = _fanin(hoods)
        k, = case.ks
        assert (fan > k).sum() > 20 and (fan < k).sum() > 20, case.name
        assert all(len(np.unique(d2)) == len(d2) for _, d2 in hoods)
    pts, ctr = KC._blob()
    own = (pts[None] == ctr[:, None]).all(-1).any(1)
    assert own.sum() == 200 and (~own).sum() == 50


def test_restatement_is_invariant_under_point_order():
    base = KC.blobs()[0]
    shuf, perm = KC.blob_shuffled()
    assert np.array_equal(shuf.points, base.points[perm])
    k, = base.ks
    a, b = _native(base), _native(shuf)
    for (ia, _), (ib, _) in zip(a, b):
        assert np.array_equal(ia[:k], perm[ib[:k]])


def test_degenerate_sizes():
    none, one = KC.degenerate()
    e, off = KC.knn_reference(none.points, none.centers, none.r, 4)
    assert e.shape == (0, 2) and off.tolist() == [0]
    assert len(one.points) == 1
    e, off = KC.knn_reference(one.points, one.centers, one.r, 4)
    assert e.tolist() == [[0, 0], [0, 1]] and off.tolist() == [0, 1, 2, 2]


# ---- the restatement ----------------------------------------------------------
@pytest.mark.parametrize("case", KC.all_cases(), ids=repr)
def test_restatement_counts_and_subset(case):
    """offsets[q+1] - offsets[q] == min(k, radius fan-in) and the rows of a
    centre are a subset of its radius-graph rows -- against the oracle's radius
    graph, which counts the pairs at exactly r (exact_r_pairs) in."""
    hoods = _native(case)
    p, c = case.cast(np.asarray(case.points).dtype)
    ref = go.radius_graph_c(p, c, case.r, case.scale) if len(c) else \
        np.zeros((0, 2), np.int64)
    deg = np.bincount(ref[:, 1], minlength=len(c))
    assert np.array_equal(deg, _fanin(hoods))
    full = set(map(tuple, ref.tolist()))
    exact = sum(int((d2 == float(case.r) * float(case.r)).sum())
                for _, d2 in hoods)
    assert exact == GC.exact_r_pairs(p, c, case.r, case.scale)
    for k in case.ks:
        edges, off = KC.take_k(hoods, k)
        assert edges.dtype == np.int32 and off.dtype == np.int32
        assert np.array_equal(np.diff(off), np.minimum(k, deg))
        assert set(map(tuple, edges.tolist())) <= full
        assert np.array_equal(edges[:, 1], np.repeat(np.arange(len(c)),
                                                     np.diff(off)))
        for q, (idx, d2) in enumerate(hoods):
            key = list(zip(d2[:k].tolist(), idx[:k].tolist()))
            assert key == sorted(key)
            if len(idx) > k:      # nothing dropped sorts before a kept row
                assert (d2[k - 1], idx[k - 1]) < (d2[k], idx[k])
    if len(c):
        e_all, _ = KC.take_k(hoods, max(int(deg.max()), 1))
        assert set(map(tuple, e_all.tolist())) == full


# ---- the library ----------------------------------------------------------------
def test_knn_entries_are_exported_and_bound():
    L, lib = _lib()
    for name in ENTRIES:
        assert hasattr(lib, name), "missing export: " + name
        assert name in L.exported_symbols()
    from pointgnn_amd import graph_gen
    assert {"knn_graph_device", "gen_disjointed_knn_local_graph_v3"} <= \
        set(graph_gen.__all__)


def test_registry_resolves_the_knn_generator():
    from pointgnn_amd import graph_gen
    fn = graph_gen.get_graph_generate_fn('disjointed_knn_local_graph_v3')
    assert fn is graph_gen.gen_disjointed_knn_local_graph_v3
    # the existing keys keep their functions
    assert graph_gen.get_graph_generate_fn('disjointed_rnn_local_graph_v3') \
        is graph_gen.gen_disjointed_rnn_local_graph_v3
    assert graph_gen.get_graph_generate_fn('multi_level_local_graph_v3') \
        is graph_gen.gen_multi_level_local_graph_v3
    with pytest.raises(ValueError):
        fn(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), 1.0, 0)


@pytest.mark.parametrize("wide", [False, True])
def test_knn_arguments_are_validated_before_hip(wide):
    L, lib = _lib()
    count = lib.pgnn_knn_graph_count_f64 if wide else lib.pgnn_knn_graph_count
    fill = lib.pgnn_knn_graph_fill_f64 if wide else lib.pgnn_knn_graph_fill
    dt = np.float64 if wide else np.float32
    pts, ctr = np.zeros((5, 3), dt), np.zeros((2, 3), dt)
    ws = np.zeros(1 << 20, np.uint8)
    off, edges = np.zeros(3, np.int32), np.zeros((8, 2), np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    null = ctypes.c_void_p(0)

    def run_count(k=4, radius=1.0, points=P(pts), offsets=P(off)):
        return count(points, 5, P(ctr), 2, radius, null, k, P(ws), ws.size,
                     offsets, null)

    def run_fill(k=4, radius=1.0, points=P(pts), out=P(edges), offsets=P(off)):
        return fill(points, 5, P(ctr), 2, radius, null, k, P(ws), ws.size,
                    offsets, out, 8, null)

    for run in (run_count, run_fill):
        for k in (0, -3):
            assert run(k=k) == L.E_INVALID
            assert b"k < 1" in lib.pgnn_last_error()
        assert run(k=257) == L.E_UNSUPPORTED
        assert b"256" in lib.pgnn_last_error()
        for radius in (0.0, -1.0):
            assert run(radius=radius) == L.E_INVALID
            assert b"knn_graph" in lib.pgnn_last_error()
        assert run(points=null) == L.E_INVALID
        assert b"null" in lib.pgnn_last_error()
        assert run(offsets=null) == L.E_INVALID
        assert b"knn_graph" in lib.pgnn_last_error()
    assert run_fill(out=null) == L.E_INVALID
    assert b"null" in lib.pgnn_last_error()
    # k < 1 is reported even when everything else is wrong too
    assert count(null, -1, null, -1, -1.0, null, 0, null, 0, null,
                 null) == L.E_INVALID
    assert b"k < 1" in lib.pgnn_last_error()


def test_knn_workspace_is_a_function_of_its_three_arguments():
    L, lib = _lib()
    q = lib.pgnn_knn_graph_workspace_bytes
    assert q(1000, 100, 0) == 0 and q(1000, 100, 257) == 0
    assert q(-1, 100, 4) == 0 and q(1000, -1, 4) == 0
    assert 0 < q(1000, 100, 1) <= q(1000, 100, 256)
    assert q(1000, 100, 256) < q(100000, 100, 256)
    assert q(1000, 100, 256) < q(1000, 100000, 256)
    # nothing in it grows with the fan-in: the radius builder's own tables
    assert q(1000, 100, 256) == lib.pgnn_radius_graph_workspace_bytes(1000,
                                                                      100)
