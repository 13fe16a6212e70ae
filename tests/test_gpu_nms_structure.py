"""The control flow of the detection kernels (csrc/detect.hip) at the sizes
where it branches, against oracle/detect_oracle.py and the references of
tests/_nms_cases.py (proved on the CPU in tests/test_nms_cases_cpu.py):

  * the scan (nms_resolve_kernel): chunk and mask-word edges, a prefetched row
    that is taken / that was removed meanwhile, more than 64 mask words, keep
    bits in global memory with removed boxes that must not remove others, a
    partial last keep word, top_k at word edges;
  * the merge (nms_merge_kernel): removed sets of 1023 / 1024 / 1025 entries
    (the in-LDS list holds 1024), two spilling sets at once, value ties in the
    rank-count median;
  * the sort: equal scores across radix-sort tiles, +0.0 against -0.0;
  * the polygon clip at its 8-vertex limit and degenerate contacts;
  * candidate selection at workgroup-chunk edges, with capacity < count, and
    the capacity form called directly.

Bars (those of tests/test_gpu_detect.py): kept indices, labels and merged
boxes bit-exact; accumulated scores rtol 1e-6; overlaps rtol 5e-7 / atol 5e-9
against the oracle and 1e-6 relative against the closed form.  The scenes keep
every overlap a scan can evaluate either at an exact 0 or farther than 0.05
from the threshold (asserted by their builders), so the decisions are exact.
"""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _nms_cases as NC
from oracle import detect_oracle as DO

pytestmark = pytest.mark.gpu

MODES = ("plain", "uncertainty", "merge_only", "score_only")
THR_CHAIN = 0.1
THR_CLUSTER = 0.01
SENTINEL = -7


def _fn(mode):
    from pointgnn_amd import nms
    return {"plain": nms.nms_boxes_3d,
            "uncertainty": nms.nms_boxes_3d_uncertainty,
            "merge_only": nms.nms_boxes_3d_merge_only,
            "score_only": nms.nms_boxes_3d_score_only}[mode]


def _device(mode, labels, boxes, scores, thr, top_k=-1):
    from pointgnn_amd import nms
    keep_in = (labels.copy(), boxes.copy(), scores.copy())
    got = _fn(mode)(labels, boxes, scores, overlapped_thres=thr,
                    overlapped_fn=nms.overlapped_boxes_3d_fast_poly,
                    appr_factor=100.0, top_k=top_k,
                    attributes=np.arange(len(labels)))
    for a, b in zip(keep_in, (labels, boxes, scores)):
        assert np.array_equal(a, b)          # inputs untouched
    return got


def _oracle(mode, labels, boxes, scores, thr, top_k=-1):
    return DO.nms_boxes_3d(labels, boxes, scores, thr, mode,
                           appr_factor=100.0, top_k=top_k)


def _same(got, want):
    """(labels, boxes, scores, attrs) of the device against a reference."""
    assert np.array_equal(got[3], want[3])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-6)


# ---------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize("entry", NC.OVERLAP_TABLE, ids=lambda e: e[0])
def test_overlap_closed_forms_both_argument_orders(entry):
    from pointgnn_amd import nms
    name, a, b, area = entry
    corners = DO.boxes_3d_to_corners(np.stack([a, b]))
    closed = NC.overlap_from_area(a, b, area)
    for one, other, c1, c2 in ((a, b, corners[0], corners[1]),
                               (b, a, corners[1], corners[0])):
        got = nms.overlapped_boxes_3d_fast_poly(one, other[None])
        want = DO.overlapped_boxes_3d_fast_poly(c1, c2[None])
        print(name, "device %.17g oracle %.17g closed form %.17g" % (
            got[0], want[0], closed))
        np.testing.assert_allclose(got, want, rtol=5e-7, atol=5e-9)
        np.testing.assert_allclose(got[0], closed, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- 2. scan order
_EDGE_CASES = [(1, m, order) for m in (63, 64, 65, 128, 129, 130)
               for order in ("desc", "asc", "random")] + \
              [(2, 70, "interleaved")]


@pytest.mark.parametrize("n_chains,length,order", _EDGE_CASES)
def test_scan_order_at_word_and_chunk_edges(n_chains, length, order):
    """One chain of m boxes: every decision depends on the one before it.
    "desc": the row prefetched while box p is processed is p + 1, which p
    removes (prefetch miss); "interleaved": the prefetched row is the next one
    taken (prefetch hit)."""
    labels, boxes, scores, nb = NC.chain_scene(n_chains, length,
                                               100 + length, order)
    for mode in MODES:
        want = _oracle(mode, labels, boxes, scores, THR_CHAIN)
        got = _device(mode, labels, boxes, scores, THR_CHAIN)
        _same(got, want)
        assert 0 < len(want[3]) < len(labels)
        if order == "desc":
            assert set(got[3].tolist()) == NC.desc_survivors(labels, nb)


# ---------------------------------------------------------------- 3. > 64 words
@pytest.fixture(scope="module")
def chains_66_words():
    scene = NC.chain_scene(840, 5, 1, "random")
    assert (len(scene[0]) + 63) // 64 == 66
    return scene


@pytest.mark.parametrize("mode", ["uncertainty", "merge_only", "score_only"])
def test_more_than_64_mask_words(chains_66_words, mode):
    """4200 boxes = 66 mask words: the second trip of the scan's lane loop,
    with suppression bits in word indices >= 64."""
    labels, boxes, scores, nb = chains_66_words
    want = NC.nms_sparse(labels, boxes, scores, THR_CHAIN, mode, nb)
    got = _device(mode, labels, boxes, scores, THR_CHAIN)
    _same(got, want)
    # some survivor removes a box that sits beyond word 63 of its row
    order = np.argsort(-scores, kind="stable")
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    _, by = NC.keep_only(labels, scores, nb, return_removed_by=True)
    assert np.any(pos[by >= 0] >= 64 * 64)


# ---------------------------------------------------------------- 4. global keep
def test_keep_bits_in_global_memory():
    """65 540 boxes = 1025 keep words (more than the 1024 held in LDS), 4 bits
    in the last one.  In chains a removed box has a non-empty row of its own:
    it must not remove others."""
    labels, boxes, scores, nb = NC.chain_scene(13108, 5, 2, "random")
    n = len(labels)
    assert n == 65540 and (n + 63) // 64 == 1025 and n % 64 == 4
    kept, by = NC.keep_only(labels, scores, nb, return_removed_by=True)
    got = _device("uncertainty", labels, boxes, scores, THR_CHAIN)
    assert np.array_equal(got[3], kept)
    assert np.array_equal(got[0], labels[kept])
    order = np.argsort(-scores, kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    # removed boxes whose own row is not empty (a later same-label neighbour)
    gone = np.nonzero(by >= 0)[0]
    has_row = np.zeros(n, bool)
    for col in (0, 1):
        j = nb[:, col]
        ok = j >= 0
        has_row[ok] |= (pos[j[ok]] > pos[ok]) & (labels[j[ok]] == labels[ok])
    assert has_row[gone].sum() > 1000
    assert pos[kept].max() >= 65536 or pos[gone].max() >= 65536
    # survivors that removed nothing come through unchanged
    owners = np.unique(by[gone])
    quiet = ~np.isin(kept, owners)
    assert np.array_equal(got[1][quiet], boxes[kept[quiet]])
    assert np.array_equal(got[2][quiet], scores[kept[quiet]])
    # 200 seeded survivors: the oracle's arithmetic on their removed sets
    rng = np.random.default_rng(4)
    out_row = np.empty(n, np.int64)
    out_row[kept] = np.arange(len(kept))
    sizes = set()
    for s in rng.choice(owners, 200, replace=False):
        removed = np.nonzero(by == s)[0]
        removed = removed[np.argsort(pos[removed])]
        sizes.add(len(removed))
        sub = np.concatenate([[s], removed])
        b, sc = boxes[sub].copy(), scores[sub].copy()
        NC.row_arithmetic(b, sc, DO.boxes_3d_to_corners(b), 0,
                          np.arange(1, len(sub)), True, True)
        assert np.array_equal(got[1][out_row[s]], b[0])
        np.testing.assert_allclose(got[2][out_row[s]], sc[0], rtol=1e-6)
        assert sc[0] > scores[s]
    assert sizes == {1, 2}


# ---------------------------------------------------------------- 5. list capacity
@pytest.fixture(scope="module")
def clusters():
    return NC.cluster_scene([1024, 1025, 1026, 1500, 7, 2], 2,
                            [None, 1.0 / 32, None, None, None, None])


@pytest.mark.parametrize("mode", ["uncertainty", "merge_only", "score_only"])
def test_list_capacity_and_concurrent_spills(clusters, mode):
    """Removed sets of 1023, 1024 (the last that fits the LDS list), 1025 and
    1499 entries (two spill segments handed out in one launch), 6 and 1; the
    1024-entry set is quantised to 1/32: value ties at an odd median count."""
    labels, boxes, scores = clusters
    want = _oracle(mode, labels, boxes, scores, THR_CLUSTER)
    got = _device(mode, labels, boxes, scores, THR_CLUSTER)
    assert len(want[3]) == 6
    obj = np.round((boxes[:, 0] - 1.0) / 30.0).astype(int)
    removed = np.bincount(obj) - 1
    assert sorted(removed.tolist()) == [1, 6, 1023, 1024, 1025, 1499]
    assert sorted(obj[want[3]].tolist()) == list(range(6))
    _same(got, want)
    if mode != "score_only":
        assert not np.array_equal(want[1], boxes[want[3]])     # merged


# ---------------------------------------------------------------- 6. top_k
@pytest.fixture(scope="module")
def mixed_scene():
    cl, cb, cs, _ = NC.chain_scene(1, 130, 6, "random")
    ul, ub, us = NC.cluster_scene([40, 9], 7, thr=THR_CHAIN)
    ub = ub.copy()
    ub[:, 2] += 20.0            # clusters at z = 40, the chain at z = 0
    labels = np.concatenate([cl, ul])
    boxes = np.concatenate([cb, ub])
    scores = np.concatenate([cs, us])
    assert len(np.unique(scores)) == len(scores) == 179
    perm = np.random.default_rng(8).permutation(len(labels))
    return labels[perm], boxes[perm], scores[perm]


@pytest.mark.parametrize("mode", ["plain", "uncertainty"])
def test_top_k_at_word_edges(mixed_scene, mode):
    labels, boxes, scores = mixed_scene
    m = len(labels)
    seen = set()
    for top_k in (1, 64, 65, m - 1, m, m + 7, -1):
        want = _oracle(mode, labels, boxes, scores, THR_CHAIN, top_k)
        got = _device(mode, labels, boxes, scores, THR_CHAIN, top_k)
        _same(got, want)
        seen.add(len(want[3]))
    assert len(seen) >= 4


# ---------------------------------------------------------------- 7. sort
def _sort_check(labels, boxes, scores):
    got = _device("uncertainty", labels, boxes, scores, THR_CLUSTER)
    order = np.argsort(-scores, kind="stable")
    assert np.array_equal(got[3], order)
    assert np.array_equal(got[0], labels[order])
    assert np.array_equal(got[1], boxes[order])
    assert np.array_equal(got[2], scores[order])


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4096, 4097])
def test_sort_at_tile_edges(n):
    labels, boxes = NC.isolated_grid(n, n)
    rng = np.random.default_rng(n)
    scores = ((rng.permutation(n) - n // 3) / np.float32(n)).astype(np.float32)
    assert len(np.unique(scores)) == n and (scores < 0).sum() > n // 4
    _sort_check(labels, boxes, scores)


def test_sort_keeps_input_order_of_equal_scores():
    """Seven score values, each spread over all three 2048-key sort tiles of
    the input; +0.0 and -0.0 are equal and must keep their input order too."""
    n = 5000
    labels, boxes = NC.isolated_grid(n, 9)
    values = np.array([0.75, 0.5, 0.0, -0.0, -0.25, 0.125, 0.3125], np.float32)
    pick = np.random.default_rng(10).integers(0, 7, n)
    scores = values[pick]
    for v in range(7):
        where = np.nonzero(pick == v)[0]
        assert {int(w) // 2048 for w in where} == {0, 1, 2}
    neg0 = np.nonzero(pick == 3)[0]
    pos0 = np.nonzero(pick == 2)[0]
    assert np.all(np.signbit(scores[neg0])) and neg0.min() < pos0.max()
    assert not np.any(np.signbit(scores[pos0]))
    _sort_check(labels, boxes, scores)


# ---------------------------------------------------------------- 8. candidates
def _candidates_abi(probs, capacity, k_dev=None):
    """pgnn_detection_candidates[_dyn] through ctypes with the outputs
    prefilled -> (out_index, out_label) of `room` entries each, count."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).to(dev)
    k, nc = probs.shape
    room = k * nc + 8
    assert capacity <= room
    idx = torch.full((room,), SENTINEL, dtype=torch.int32, device=dev)
    lab = torch.full((room,), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if k_dev is None:
            rc = lib.pgnn_detection_candidates(
                _lib.ptr(p), k, nc, _lib.ptr(idx), _lib.ptr(lab), capacity,
                _lib.ptr(cnt), _lib.stream_ptr())
        else:
            kd = torch.tensor([k_dev], dtype=torch.int32, device=dev)
            rc = lib.pgnn_detection_candidates_dyn(
                _lib.ptr(p), k, _lib.ptr(kd), nc, _lib.ptr(idx), _lib.ptr(lab),
                capacity, _lib.ptr(cnt), _lib.stream_ptr())
        _lib.check(rc, "pgnn_detection_candidates")
        torch.cuda.synchronize()
    return idx.cpu().numpy(), lab.cpu().numpy(), int(cnt.item())


def _probs(k, nc, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 1.5, (k, nc))
    probs = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(
        np.float32)
    flat = probs.reshape(-1)
    edge = rng.choice(k * nc, 9, replace=False)
    flat[edge] = np.float32(1.0 / nc)               # boundary: not selected
    # candidates on both sides of every 256-entry chunk edge of the kernel
    for p0 in range(256, k * nc, 256):
        for p in range(max(p0 - 3, 0), min(p0 + 3, k * nc)):
            flat[p] = 0.9
    return probs


def _totals(nc):
    """k for which k*nc is the multiple of nc at or next below / above each of
    255, 256, 257, 1023, 1024, 1025 (a total is always a multiple of nc)."""
    ks = set()
    for t in (255, 256, 257, 1023, 1024, 1025):
        ks.add(t // nc)
        ks.add(-(-t // nc))
    return sorted(ks)


@pytest.mark.parametrize("nc", [4, 6, 8])
def test_candidates_at_chunk_edges(nc):
    for k in _totals(nc):
        probs = _probs(k, nc, 1000 * nc + k)
        widx, wlab = DO.select_candidates(probs)
        idx, lab, cnt = _candidates_abi(probs, k * nc)
        assert cnt == len(widx) > 0
        assert np.array_equal(idx[:cnt], widx)
        assert np.array_equal(lab[:cnt], wlab)
        assert np.all(idx[cnt:] == SENTINEL) and np.all(lab[cnt:] == SENTINEL)
        assert set(np.unique(wlab)) <= {1, 3, 5}


@pytest.mark.parametrize("nc", [4, 6])
def test_candidates_capacity_below_count(nc):
    """*out_count receives the full count; entries beyond `capacity` are
    dropped and nothing past it is written (include/pointgnn_hip.h)."""
    probs = _probs(600, nc, 77 + nc)
    widx, wlab = DO.select_candidates(probs)
    full = len(widx)
    assert full > 258
    for capacity in (0, 1, 255, 256, 257, full - 1):
        idx, lab, cnt = _candidates_abi(probs, capacity)
        assert cnt == full
        assert np.array_equal(idx[:capacity], widx[:capacity])
        assert np.array_equal(lab[:capacity], wlab[:capacity])
        assert np.all(idx[capacity:] == SENTINEL)
        assert np.all(lab[capacity:] == SENTINEL)


@pytest.mark.parametrize("nc", [4, 6])
def test_candidates_capacity_form(nc):
    """probs has 300 rows of which the first k_dev exist; the others hold 1.0
    in every class, so a kernel that read them would select them."""
    import torch
    from pointgnn_amd import nms
    cap_rows = 300
    dev = torch.device("cuda", 0)
    for k_dev in (0, 1, 299, 300, 305, -3):
        live = min(max(k_dev, 0), cap_rows)
        probs = _probs(cap_rows, nc, 5 * nc + live)
        probs[live:] = 1.0
        widx, wlab = DO.select_candidates(probs[:live]) if live else \
            (np.zeros(0, np.int64), np.zeros(0, np.int64))
        # the C entry itself, outputs prefilled
        idx, lab, cnt = _candidates_abi(probs, cap_rows * nc, k_dev=k_dev)
        assert cnt == len(widx)
        assert np.array_equal(idx[:cnt], widx)
        assert np.array_equal(lab[:cnt], wlab)
        assert np.all(idx[cnt:] == SENTINEL) and np.all(lab[cnt:] == SENTINEL)
        # the Python entry of the frame loop
        kd = torch.tensor([k_dev], dtype=torch.int32, device=dev)
        t_idx, t_lab, t_cnt = nms.select_candidates_dyn(
            torch.from_numpy(probs).to(dev), kd)
        c = int(t_cnt.item())
        assert c == len(widx) and t_idx.numel() == cap_rows * nc
        assert np.array_equal(t_idx[:c].cpu().numpy(), widx)
        assert np.array_equal(t_lab[:c].cpu().numpy(), wlab)
