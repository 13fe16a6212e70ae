"""The standalone scatter-max / scatter-sum (csrc/scatter_max.hip) at every
point where its launcher or its kernels branch, through the C ABI (strides and
pointer offsets are what a case says), against the references of
tests/_scatter_cases.py (proved on the CPU in tests/test_scatter_cases_cpu.py):

  * the launcher: all seven scatter_max_kernel<VEC, NJ, BATCH> at both ends of
    their column ranges, each with non-temporal and plain loads (scatter_nt),
    sorted and unsorted; the scalar kernels forced by a row stride, by a data
    pointer and by an output pointer that is not 16-byte aligned; both
    PGNN_E_UNSUPPORTED exits and the stride check;
  * strides: ld_out != n_cols (fill_rows_kernel), ld_data != n_cols with +inf
    in the pad columns, in front of an offset pointer and behind the last row;
  * chunking: scatter_rows_per_wave 0 (auto), 1 (raised to BATCH), BATCH,
    BATCH + 1, 32 and 33; 1, BATCH - 1, BATCH and BATCH + 1 rows; runs cut at
    and continuing across r0 and r1, a segment over several whole chunks, a
    last chunk shorter than a batch (clamped duplicate rows), and more chunks
    than the capped grid has waves (the chunk loop's second turn);
  * ids: every row its own segment, empty segments, a negative prefix and a
    suffix >= n_seg, nothing in range, -1 in the first row (`cur` starts
    there);
  * special values: signed zeros, infinities, lowest(), FLT_MAX and denormals
    of both signs give the same bits on the plain-store and the atomic path;
  * sum / mean: padded strides (the 2-D memset), ids out of range, segments
    of 0 and 1 rows, the add kernel and the mean finish with a strided grid,
    mean without its workspace.

Max is idempotent, so the data is made of witnesses: every row at a seam
(chunk, batch and run edges) is the sole maximum of its segment in some column,
and a seam row read twice cannot hide one that was skipped.

Bars: max bit-exact against init-with-lowest-then-max (exact in float32); sum
equal to the int64 reference on integer-valued data, mean within 2^-22 of
sum / max(count, 1) (tests/test_gpu_aggregation.py, part A); every float
outside [n_seg, n_cols] of `out` keeps its sentinel bits.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _scatter_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD            # a NaN no kernel here produces
RUNNABLE = SC.runnable(SC.MAX_CASES)
REFUSED = SC.refused(SC.MAX_CASES)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def cus(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@contextlib.contextmanager
def tunables(rows_per_wave, nt):
    """scatter_rows_per_wave and scatter_nt for the block, their defaults
    afterwards."""
    from pointgnn_amd import _lib
    try:
        _lib.set_tunable("scatter_rows_per_wave", rows_per_wave)
        _lib.set_tunable("scatter_nt", nt)
        yield
    finally:
        _lib.set_tunable("scatter_rows_per_wave", 0)
        _lib.set_tunable("scatter_nt", 1)


def upload_data(dev, c, data):
    """[offset][n_rows x ld_data][one more row]: everything that is not data
    is +inf, so a read of it wins the max and is seen."""
    host = np.full(c.data_off + (c.n_rows + 1) * c.ld_data, np.inf, np.float32)
    host[c.data_off:c.data_off + c.n_rows * c.ld_data].reshape(
        c.n_rows, c.ld_data)[:, :c.n_cols] = data
    return T(host, dev)


class Out(object):
    """[offset][guard row][n_seg rows of `ld`][guard row], all sentinel."""

    def __init__(self, dev, c, ld=None):
        import torch
        self.c, self.ld = c, ld or c.ld_out
        self.front = c.out_off + self.ld
        self.buf = torch.full((self.front + (c.n_seg + 1) * self.ld,),
                              SENTINEL, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.front)

    def bits(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def result(self):
        """-> the [n_seg, n_cols] result as uint32, guards checked."""
        c, b = self.c, self.bits()
        body = b[self.front:self.front + c.n_seg * self.ld].reshape(
            c.n_seg, self.ld)
        assert np.all(b[:self.front] == SENTINEL), \
            "%s: wrote in front of out" % c.name
        assert np.all(b[self.front + c.n_seg * self.ld:] == SENTINEL), \
            "%s: wrote behind the last segment" % c.name
        assert np.all(body[:, c.n_cols:] == SENTINEL), \
            "%s: wrote pad columns of out" % c.name
        return body[:, :c.n_cols].copy()


def call_max(dev, c, dbuf, ids_t, sorted_=None, rpw=None, nt=None):
    """pgnn_scatter_max_f32 on the case's layout -> (code, Out)."""
    from pointgnn_amd import _lib
    import torch
    lib = _lib.load()
    out = Out(dev, c, ld=max(c.ld_out, c.n_cols))
    assert dbuf.data_ptr() % 16 == 0
    with tunables(c.rpw_tunable if rpw is None else rpw,
                  c.nt if nt is None else nt):
        rc = lib.pgnn_scatter_max_f32(
            ctypes.c_void_p(dbuf.data_ptr() + 4 * c.data_off), c.ld_data,
            _lib.ptr(ids_t), c.n_rows, c.n_cols, c.n_seg, out.ptr, c.ld_out,
            c.sorted if sorted_ is None else sorted_, _lib.stream_ptr())
        torch.cuda.synchronize()
    return rc, out


def same_bits(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d cells differ, first at %r: %08x != %08x" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def check_case(dev, c, cus):
    m = SC.Model(c, cus)
    ids_t = T(m.ids, dev)
    for k, data in enumerate(m.witness()):
        rc, out = call_max(dev, c, upload_data(dev, c, data), ids_t)
        assert rc == 0, c.name
        got = out.result().view(np.float32)
        ref = SC.reference(data, m.ids, c.n_seg)
        assert np.array_equal(got, ref), "%s seed %d: %d cells differ" % (
            c.name, k, int((got != ref).sum()))
    return m


# ------------------------------------------------------------ 1. max, reference
@pytest.mark.parametrize("c", RUNNABLE, ids=lambda c: c.name)
def test_max_matches_reference(dev, cus, c):
    """Every case and witness seed: out == reference over [n_seg, n_cols], and
    nothing else of the buffer written."""
    check_case(dev, c, cus)


def test_device_cu_count_is_torchs(dev, cus):
    """The grid-stride cases are sized with torch's CU count; the launcher
    caps its grid with its own."""
    import torch
    from pointgnn_amd import _lib
    # a 1-CU mask must be accepted and a (cus + 1)-wide one refused
    lib = _lib.load()
    s = ctypes.c_void_p(0)
    assert lib.pgnn_stream_create_cu_mask(0, cus + 1, 0, ctypes.byref(s)) == \
        _lib.E_INVALID
    assert lib.pgnn_stream_create_cu_mask(0, cus, 0, ctypes.byref(s)) == 0
    assert lib.pgnn_stream_destroy(s) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", [0, 1], ids=["vector", "scalar"])
def test_max_with_more_chunks_than_waves(dev, cus, which):
    """16 rows per wave and 4 x 8 x CUs + 1000 chunks: the chunk loop strides
    on this device (asserted, not assumed)."""
    c = SC.grid_stride_cases(cus)[which]
    m = check_case(dev, c, cus)
    assert m.rpw == 16 and len(m.chunks) > 4 * 8 * cus and m.strides


# ------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("c", REFUSED, ids=lambda c: c.name)
def test_refusals(dev, c):
    from pointgnn_amd import _lib
    want = SC.case_dispatch(c)
    data = np.zeros((c.n_rows, c.n_cols), np.float32)
    ids = SC.make_ids(c.recipe, c.n_rows, c.n_seg)
    rc, out = call_max(dev, c, upload_data(dev, c, data), T(ids, dev))
    msg = _lib.load().pgnn_last_error()
    assert rc == {"unsupported": _lib.E_UNSUPPORTED,
                  "invalid": _lib.E_INVALID}[want], (c.name, rc)
    assert SC.REFUSAL_TEXT[c.name] in msg, msg
    if want == "invalid":
        assert np.all(out.bits() == SENTINEL), "a refused call wrote `out`"
    else:
        out.result()                         # the guards


# --------------------------------------------------- 3. one result, one pattern
def _paths(batch):
    """(name, ids_sorted, rows-per-wave tunable, nt)"""
    return (("sorted", 1, 0, 1), ("sorted_batch", 1, batch, 1),
            ("sorted_rpw33", 1, 33, 1), ("unsorted", 0, 0, 1),
            ("sorted_nt0", 1, 0, 0))


@pytest.mark.parametrize("n_cols", [4, 3], ids=["vector", "scalar"])
def test_special_values_one_bit_pattern(dev, n_cols):
    """Signed zeros, infinities, lowest(), FLT_MAX, denormals: the plain-store
    path (sorted; every segment takes it at 33 rows per wave, all but one or
    two otherwise) and the atomic path (unsorted, shuffled) write the same
    bits -- the canonical form of include/pointgnn_hip.h: +0.0 for a zero,
    lowest() for a segment of only -inf."""
    data, ids = SC.special_input(n_cols)
    ref = SC.reference(data, ids, len(SC.SPECIAL_SEGMENTS))
    want = SC.canonical_bits(ref)
    names = [n for n, _ in SC.SPECIAL_SEGMENTS]
    assert ref[names.index("neg_inf_only"), 0] == SC.LOWEST
    assert want[names.index("neg_zero_only"), 0] == 0
    got = {}
    for v in SC.SPECIAL_VARIANTS:
        c = SC.special_case(n_cols, v)
        d, i = data, ids
        if v[4]:
            perm = np.random.default_rng(3).permutation(len(ids))
            d, i = data[perm], ids[perm]
        rc, out = call_max(dev, c, upload_data(dev, c, d), T(i, dev))
        assert rc == 0
        got[v[0]] = out.result()
        for s, name in enumerate(names):
            print(v[0], name, ["%08x" % b for b in got[v[0]][s]])
    for name, bits in got.items():
        assert np.array_equal(bits.view(np.float32), ref), name
    for name, bits in got.items():
        same_bits(bits, got["sorted"], "%s against sorted" % name)
        same_bits(bits, want, "%s against the canonical form" % name)


@pytest.mark.parametrize("name", SC.ONE_PATTERN_CASES)
def test_ordinary_cases_one_bit_pattern(dev, cus, name):
    c = {c.name: c for c in SC.MAX_CASES}[name]
    m = SC.Model(c, cus)
    data = m.witness()[0]
    dbuf, ids_t = upload_data(dev, c, data), T(m.ids, dev)
    want = SC.canonical_bits(SC.reference(data, m.ids, c.n_seg))
    for path, sorted_, rpw, nt in _paths(m.batch):
        rc, out = call_max(dev, c, dbuf, ids_t, sorted_, rpw, nt)
        assert rc == 0
        same_bits(out.result(), want, "%s %s" % (name, path))


# -------------------------------------------------------------------- 4. wrapper
def test_wrapper_on_a_column_slice_and_sorted_against_the_abi(dev, cus):
    from pointgnn_amd import gnn
    c = {c.name: c for c in SC.MAX_CASES}["c300_aligned_s1"]
    m = SC.Model(c, cus)
    data = m.witness()[0]
    ref = SC.reference(data, m.ids, c.n_seg)
    wide = np.full((c.n_rows, 304), np.inf, np.float32)
    wide[:, 2:302] = data
    view = T(wide, dev)[:, 2:302]
    assert not view.is_contiguous()
    ids_t = T(m.ids, dev)
    for sorted_ in (False, True):
        got = gnn.graph_scatter_max_fn(view, ids_t, c.n_seg,
                                       ids_sorted=sorted_).cpu().numpy()
        assert np.array_equal(got, ref), sorted_
    rc, out = call_max(dev, c, upload_data(dev, c, data), ids_t)
    assert rc == 0
    got = gnn.graph_scatter_max_fn(T(data, dev), ids_t, c.n_seg,
                                   ids_sorted=True).cpu().numpy()
    same_bits(got.view(np.uint32), out.result(), "wrapper against the ABI")
    # int64 ids of any shape, as the layers pass them
    got = gnn.graph_scatter_max_fn(T(data, dev),
                                   T(m.ids.astype(np.int64)[:, None], dev),
                                   c.n_seg).cpu().numpy()
    assert np.array_equal(got, ref)


# --------------------------------------------------------------- 5. sum and mean
def call_sum(dev, c, data, ids, mean, with_counts=True):
    """pgnn_scatter_sum_f32 -> (code, result [n_seg, n_cols] float32)."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    layout = SC.Case(c.name, c.n_rows, c.n_cols, c.n_seg, c.ld_data, c.ld_out,
                     0, 0, 0, 0, 1, None)
    dbuf = upload_data(dev, layout, data)
    out = Out(dev, layout)
    counts = torch.full((c.n_seg + 2,), SENTINEL, dtype=torch.int32, device=dev)
    cptr = ctypes.c_void_p(counts.data_ptr() + 4) if with_counts else None
    rc = lib.pgnn_scatter_sum_f32(
        _lib.ptr(dbuf), c.ld_data, _lib.ptr(T(ids, dev)), c.n_rows, c.n_cols,
        c.n_seg, out.ptr, c.ld_out, mean, cptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    cnt = counts.cpu().numpy()
    assert cnt[0] == SENTINEL and cnt[-1] == SENTINEL, "counts guards"
    if rc != 0:
        assert np.all(out.bits() == SENTINEL), "a refused call wrote `out`"
        return rc, None
    if not mean:
        assert np.all(cnt == SENTINEL), "sum wrote the counts workspace"
    return rc, out.result().view(np.float32)


@pytest.mark.parametrize("mean", [0, 1], ids=["sum", "mean"])
@pytest.mark.parametrize("which", range(5),
                         ids=[c.name for c in SC.sum_cases(SC.CPU_TEST_CUS)])
def test_sum_and_mean_exact(dev, cus, which, mean):
    c = SC.sum_cases(cus)[which]
    if c.name == "add_strides":
        assert c.n_rows * c.n_cols > 256 * 16 * cus
    if c.name == "finish_strides":
        assert c.n_seg * c.n_cols > 256 * 4096
    data, ids, s, cnt = SC.sum_input(c)
    rc, got = call_sum(dev, c, data, ids, mean)
    assert rc == 0
    assert np.all(got[cnt == 0] == 0), "an empty segment is not zero"
    if not mean:
        bad = np.argwhere(got != s)
        assert bad.size == 0, "%d elements differ, first at %r" % (
            len(bad), tuple(bad[0]))
    else:
        want = s / np.maximum(cnt, 1)[:, None]
        err = np.abs(got.astype(np.float64) - want)
        print("mean: largest relative error %g" % (
            err / np.maximum(np.abs(want), 1e-300)).max())
        assert np.all(err <= 2.0 ** -22 * np.abs(want))
        one = cnt == 1
        assert one.any() and np.all(got[one] == s[one])


def test_mean_without_workspace_is_refused(dev, cus):
    from pointgnn_amd import _lib
    c = SC.sum_cases(cus)[1]
    data, ids, _, _ = SC.sum_input(c)
    rc, _ = call_sum(dev, c, data, ids, 1, with_counts=False)
    assert rc == _lib.E_INVALID
    assert b"workspace" in _lib.load().pgnn_last_error()
