"""The plain-kNN cases reach the places of knn_nearest_kernel they are named
for (a NumPy walk of the search, tests/_nearest_cases.py: shell_walk), the
restatement has the arithmetic row stride, the registry key exists, the C
entries validate their arguments before any HIP call and the capacity form
accepts the new key only.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401

import _knn_cases as KC
import _nearest_cases as NC

ENTRIES = ("pgnn_knn_nearest_workspace_bytes", "pgnn_knn_nearest",
           "pgnn_knn_nearest_f64")
NEAREST_KEY = "disjointed_nearest_local_graph_v3"
CASES = NC.all_cases()
BY_NAME = {c.name: c for c in CASES}


def _lib():
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    return L, L.load()


def _walk(case, q, k):
    p, c = case.cast(np.asarray(case.points).dtype)
    return NC.shell_walk(p, c[q], k, case.cell, case.scale)


def _ref_rows(case, q, k):
    hoods = KC.hoods_of(case, np.asarray(case.points).dtype)
    return hoods[q][0][:k].tolist(), hoods[q][1][:k]


# ---- the restatement ----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_restatement_has_the_arithmetic_stride(case):
    """knn_reference(..., r=inf): every centre has exactly min(k, N) rows, in
    ascending (d2, index) order, centre q at rows [q m, (q + 1) m)"""
    p, c = case.cast(np.asarray(case.points).dtype)
    for k in case.ks:
        edges, off = KC.knn_reference(p, c, np.inf, k, case.scale)
        m = min(k, len(p))
        assert np.array_equal(off, np.arange(len(c) + 1) * m)
        assert edges.shape == (len(c) * m, 2) and edges.dtype == np.int32
        assert np.array_equal(edges[:, 1], np.repeat(np.arange(len(c)), m))
        assert np.array_equal(edges, NC.reference(case, p.dtype, k))
    for idx, d2 in KC.hoods_of(case, p.dtype):
        key = list(zip(d2.tolist(), idx.tolist()))
        assert len(idx) == len(p) and key == sorted(key)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_walk_stops_exactly(case):
    """the restated search returns the restatement's rows: the stopping bound
    drops nothing on these clouds (first three centres and the last, every k)"""
    n_c = len(case.points if case.same else case.centers)
    for q in sorted(set(list(range(min(3, n_c))) + [n_c - 1])):
        for k in case.ks:
            got, _ = _walk(case, q, k)
            assert got == _ref_rows(case, q, k)[0], (case.name, q, k)


# ---- the cases reach their places ---------------------------------------------
def test_small_clouds_stride_is_n():
    sizes = {c.name: len(c.points) for c in NC.small_n()}
    assert sizes == {"n_lt_k": 5, "n_eq_k": 8, "n_eq_k1": 9}
    for case in NC.small_n():
        assert case.ks == (8,)
        got, info = _walk(case, 0, 8)
        assert len(got) == min(8, len(case.points))
        if len(case.points) <= 8:       # every point is kept: only a cover ends it
            assert info["stop"] == "cover"


def test_k_seams_runs_every_seam_on_a_cloud_larger_than_k():
    case = BY_NAME["k_seams"]
    assert case.ks == KC.K_EDGES and len(case.points) > 4 * KC.K_MAX
    _, info = _walk(case, 0, 256)
    assert len(info["shells"]) >= 3     # k = 256 needs several shells


def test_shell0_stops_after_the_centres_own_cell():
    case = BY_NAME["shell0"]
    got, info = _walk(case, 0, NC.SHELL0_K)
    assert info["stop"] == "bound" and [s["s"] for s in info["shells"]] == [0]
    sh = info["shells"][0]
    assert sh["cells"] == 1 and sh["hits"] >= 4 * NC.SHELL0_K
    assert sh["kth"] < sh["b"] ** 2 and sh["b"] == 0.5


def test_shell_tie_sits_on_the_seam():
    case = BY_NAME["shell_tie"]
    q = 3 * 64 + 3 * 8 + 3              # the interior centre (3, 3, 3)
    assert np.array_equal(case.points[q], [3, 3, 3]) and case.cell == 1.0
    for k in case.ks:
        idx, d2 = _ref_rows(case, q, k)
        got, info = _walk(case, q, k)
        by_s = {s["s"]: s for s in info["shells"]}
        # after shell 1 the list is full and its k-th d2 EQUALS b_1^2
        assert by_s[1]["kth"] == d2[k - 1] == 1.0 == by_s[1]["b"] ** 2
        assert info["stop"] == "bound" and max(by_s) == 2
        assert got == idx
    kept, dropped = KC.cut_ties(KC.hoods_of(case, np.float32), 4)[q]
    assert kept > 0 and dropped > 0     # k = 4: the index decides


def test_face_tie_is_won_by_an_unscanned_point():
    case = BY_NAME["face_tie"]
    k = NC.FACE_TIE_K
    idx, d2 = _ref_rows(case, 0, k)
    got, info = _walk(case, 0, k)
    sh0 = info["shells"][0]
    assert sh0["s"] == 0 and sh0["hits"] == 3 and sh0["kth"] == 0.0625
    assert sh0["b"] == 0.25 and sh0["kth"] == sh0["b"] ** 2
    assert idx == [5, 7, 2] == got and d2[-1] == 0.0625
    full = KC.hoods_of(case, np.float32)[0]
    assert full[0][3] == 9 and full[1][3] == 0.0625   # the loser of the tie
    assert len(info["shells"]) >= 2


@pytest.mark.parametrize("name,s,cells,batches", [("shell2", 2, 98, 2),
                                                  ("shell3", 3, 218, 4)])
def test_shell_cases_find_their_neighbours_in_that_shell(name, s, cells,
                                                         batches):
    case = BY_NAME[name]
    got, info = _walk(case, 0, NC.SHELL_K)
    by_s = {x["s"]: x for x in info["shells"]}
    assert info["stop"] == "bound" and max(by_s) == s
    assert all(by_s[t]["hits"] == 0 for t in range(s))
    assert (by_s[s]["cells"], by_s[s]["batches"]) == (cells, batches)
    assert by_s[s]["hits"] == NC.SHELL_K == len(got)
    # the six sit in the first and in the last lane batch of the shell
    grid_cells = NC.gc.rcell_of(np.asarray(case.points, np.float64), 1.0)
    shell = NC.shell_cells(np.array([12, 12, 12]), s, grid_cells.min(0),
                           grid_cells.max(0)).tolist()
    where = sorted(shell.index(grid_cells[i].tolist()) // 64 for i in got)
    assert where[0] == 0 and where[-1] == batches - 1


def test_far_centre_ends_by_cover_and_skips_the_empty_shells():
    case = BY_NAME["far_centre"]
    assert tuple(case.centers[0]) == NC.FAR_CENTRE
    for q in (0, 1):
        for k in case.ks:
            got, info = _walk(case, q, k)
            # the diagonal centre is farther from every kept point than from
            # any face: only the cover ends its walk (the other one sees the
            # cloud through one face, whose distance grows with the shell)
            assert info["first"] > 30 and (q == 1 or info["stop"] == "cover")
            assert info["shells"][0]["cells"] >= 1
            assert all(s["cells"] <= 6 * 6 * 6 for s in info["shells"])
            assert got == _ref_rows(case, q, k)[0]


def test_duplicates_are_cut_by_index():
    case = BY_NAME["nn_duplicates"]
    hoods = KC.hoods_of(case, np.float32)
    assert max(case.ks) < NC.DUP_COPIES
    for k in case.ks:
        kept, dropped = KC.cut_ties(hoods, k)[0]
        assert kept == k and dropped == NC.DUP_COPIES - k
        assert (hoods[0][1][:NC.DUP_COPIES] == 0.0).all()
        idx = hoods[0][0][:NC.DUP_COPIES]
        assert np.array_equal(idx, np.sort(idx))


def test_shared_bucket_cells_are_walked_twice():
    case, info = NC.shared_bucket()
    grid = NC.gc.RadiusGrid(case.points, case.cell)
    for q, rec in enumerate(info):
        cc = NC.gc.rcell_of(np.asarray(case.centers[q], np.float64), 1.0)
        lo, hi = grid.cells.min(0), grid.cells.max(0)
        near = np.concatenate([NC.shell_cells(cc, s, lo, hi) for s in (0, 1)])
        assert (NC.gc.cell_hash(near, grid.mask) == rec["bucket"]).sum() == 2
        kept = _ref_rows(case, q, 8)[0]
        assert rec["idx_far"] not in kept
        assert set(rec["idx_a"] + rec["idx_b"]) <= set(kept)


def test_scaled_same_and_shuffled():
    assert list(BY_NAME["nn_scaled"].scale) == [1.0, 2.0, 0.5]
    case = BY_NAME["nn_same"]
    assert case.same and case.points is case.centers
    hoods = KC.hoods_of(case, np.float32)
    assert all(idx[0] == q and d2[0] == 0.0
               for q, (idx, d2) in enumerate(hoods))
    base, shuf, perm = NC.blob_shuffled()
    assert np.array_equal(shuf.points, base.points[perm])
    k, = base.ks
    for (ia, da), (ib, _) in zip(KC.hoods_of(base, np.float32),
                                 KC.hoods_of(shuf, np.float32)):
        assert len(np.unique(da[:k + 1])) == k + 1      # no tie at the cut
        assert np.array_equal(ia[:k], perm[ib[:k]])


# ---- the Python surface -------------------------------------------------------
def test_registry_and_names():
    from pointgnn_amd import graph_gen
    fn = graph_gen.get_graph_generate_fn(NEAREST_KEY)
    assert fn is graph_gen.gen_disjointed_nearest_local_graph_v3
    assert {"knn_nearest_device", "gen_disjointed_nearest_local_graph_v3"} <= \
        set(graph_gen.__all__)
    # the existing keys keep their functions
    assert graph_gen.get_graph_generate_fn('disjointed_rnn_local_graph_v3') \
        is graph_gen.gen_disjointed_rnn_local_graph_v3
    assert graph_gen.get_graph_generate_fn('disjointed_knn_local_graph_v3') \
        is graph_gen.gen_disjointed_knn_local_graph_v3
    with pytest.raises(ValueError):
        fn(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), 0)


def _levels(method1, kwargs1):
    from pointgnn_amd import configs
    lv0, lv1 = [dict(l) for l in configs.get_config("car_auto_T1")[
        "runtime_graph_gen_kwargs"]["level_configs"]]
    lv1["graph_gen_method"], lv1["graph_gen_kwargs"] = method1, kwargs1
    return [lv0, lv1]


def test_capacity_form_accepts_the_new_key_only():
    """Both refusals come before any device work: the argument check of
    _multi_level_graph_deferred needs a tensor, not a GPU."""
    import torch
    from pointgnn_amd import graph_gen
    xyz = torch.zeros((16, 3), dtype=torch.float32)
    hints = graph_gen.CountHints(k=16, edges=[100, 100])
    with pytest.raises(NotImplementedError, match="no capacity form"):
        graph_gen._multi_level_graph_deferred(
            xyz, 0.8, _levels("disjointed_knn_local_graph_v3",
                              {"radius": 4.0, "num_neighbors": 8}),
            [0.5, 0.5], False, "center", hints)
    with pytest.raises(ValueError, match="cell_size"):
        graph_gen._multi_level_graph_deferred(
            xyz, 0.8, _levels(NEAREST_KEY, {"num_neighbors": 8}),
            [0.5, 0.5], False, "center", hints)
    with pytest.raises(ValueError, match="num_neighbors"):
        graph_gen._multi_level_graph_deferred(
            xyz, 0.8, _levels(NEAREST_KEY, {"num_neighbors": 0,
                                            "cell_size": 1.0}),
            [0.5, 0.5], False, "center", hints)


# ---- the library ----------------------------------------------------------------
def test_nearest_entries_are_exported_and_bound():
    L, lib = _lib()
    for name in ENTRIES:
        assert hasattr(lib, name), "missing export: " + name
        assert name in L.exported_symbols()


@pytest.mark.parametrize("wide", [False, True])
def test_nearest_arguments_are_validated_before_hip(wide):
    L, lib = _lib()
    fn = lib.pgnn_knn_nearest_f64 if wide else lib.pgnn_knn_nearest
    dt = np.float64 if wide else np.float32
    pts, ctr = np.zeros((5, 3), dt), np.zeros((2, 3), dt)
    ws = np.zeros(1 << 20, np.uint8)
    edges = np.zeros((16, 2), np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    null = ctypes.c_void_p(0)

    def run(k=4, cell=1.0, points=P(pts), out=P(edges), n_ws=ws.size,
            centers_cap=2):
        return fn(points, 5, null, P(ctr), centers_cap, null, null, k, cell,
                  P(ws), n_ws, out, 16, null, null)

    for k in (0, -3):
        assert run(k=k) == L.E_INVALID
        assert b"k < 1" in lib.pgnn_last_error()
    assert run(k=257) == L.E_UNSUPPORTED
    assert b"256" in lib.pgnn_last_error()
    for cell in (0.0, -1.0, float("nan")):
        assert run(cell=cell) == L.E_INVALID
        assert b"cell_size" in lib.pgnn_last_error()
    assert run(points=null) == L.E_INVALID
    assert b"null" in lib.pgnn_last_error()
    assert run(out=null) == L.E_INVALID
    assert b"null" in lib.pgnn_last_error()
    assert run(n_ws=64) == L.E_WORKSPACE
    assert run(centers_cap=1 << 30) == L.E_INVALID
    assert b"int32" in lib.pgnn_last_error()
    # k < 1 is reported even when everything else is wrong too
    assert fn(null, -1, null, null, -1, null, null, 0, -1.0, null, 0, null,
              -1, null, null) == L.E_INVALID
    assert b"k < 1" in lib.pgnn_last_error()


def test_nearest_workspace_is_a_function_of_its_arguments():
    L, lib = _lib()
    q = lib.pgnn_knn_nearest_workspace_bytes
    assert q(1000, 100, 0) == 0 and q(1000, 100, 257) == 0
    assert q(-1, 100, 4) == 0 and q(1000, -1, 4) == 0
    assert 0 < q(1000, 100, 1) == q(1000, 100, 256)
    assert q(1000, 100, 256) < q(100000, 100, 256)
    # no counts, no scan: nothing in it grows with the centres
    assert q(1000, 100, 256) == q(1000, 100000, 256)
