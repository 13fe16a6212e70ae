"""Cases, models and reference for the structural tests of the standalone
scatter-max / scatter-sum (csrc/scatter_max.hip): tests/test_scatter_cases_cpu.py
proves them, tests/test_gpu_scatter_structure.py runs them on the device.

To AIM, this module restates the host side of the kernel in Python:

  dispatch      scatter_max.hip:201-251  argument checks, the 16-byte test and
                                         the seven <VEC, NJ, BATCH> launches
  resolve_rpw   scatter_max.hip:165-174  `launch`: rows per wave
  n_blocks      scatter_max.hip:175-179  `launch`: the capped grid
  partition     scatter_max.hip:91-93    a wave's row range [r0, r1)
  runs          scatter_max.hip:98-115   `flush`: plain store or atomic

The restatement only CHARACTERISES a case (which kernel runs, which rows sit at
a seam, which run is stored and which is combined atomically).  Expected values
always come from `reference` below, which knows nothing of chunks.  If the
launcher changes, the GPU tests still hold the kernels to the reference -- they
only lose their aim, and tests/test_scatter_cases_cpu.py says so.
"""
import collections

import numpy as np

LOWEST = np.float32(np.finfo(np.float32).min)      # pgnn_common.h:66
FLT_MAX = np.float32(np.finfo(np.float32).max)
CPU_TEST_CUS = 256                                  # MI355X

# scatter_max.hip:227-249, in the order of the launcher
INSTANTIATIONS = ((4, 1, 16), (4, 2, 8), (4, 4, 4), (4, 8, 2),
                  (1, 1, 16), (1, 4, 8), (1, 16, 2))


# --------------------------------------------------------------------------
# the restated launcher
# --------------------------------------------------------------------------
def dispatch(n_cols, ld_data, ld_out, data_off_floats=0, out_off_floats=0):
    """-> (VEC, NJ, BATCH), "unsupported" or "invalid" for a call with rows
    and segments.  The offsets are those of the two pointers from a 16-byte
    aligned allocation, in floats."""
    if n_cols <= 0:                                        # :201
        return "invalid"
    if ld_data < n_cols or ld_out < n_cols:                # :203
        return "invalid"
    vec4 = (n_cols % 4 == 0 and ld_data % 4 == 0           # :222
            and ld_out % 4 == 0                            # :223
            and (4 * data_off_floats) % 16 == 0            # :223 data % 16
            and (4 * out_off_floats) % 16 == 0)            # :224 out % 16
    if vec4:
        nv = n_cols // 4                                   # :226
        if nv <= 64:                                       # :227
            return (4, 1, 16)
        if nv <= 128:                                      # :230
            return (4, 2, 8)
        if nv <= 256:                                      # :233
            return (4, 4, 4)
        if nv <= 512:                                      # :236
            return (4, 8, 2)
        return "unsupported"                               # :239
    if n_cols <= 64:                                       # :241
        return (1, 1, 16)
    if n_cols <= 256:                                      # :244
        return (1, 4, 8)
    if n_cols <= 1024:                                     # :247
        return (1, 16, 2)
    return "unsupported"                                   # :250


def resolve_rpw(n_rows, batch, tunable, cus):
    """Rows per wave of `launch` for the tunable scatter_rows_per_wave."""
    rpw = int(tunable)                                     # :165
    if rpw <= 0:                                           # :166
        waves = cus * 8                                    # :169
        r = -(-n_rows // waves)                            # :170
        r = -(-r // batch) * batch                         # :171
        rpw = 32 if r < 32 else (4096 if r > 4096 else r)  # :172
    if rpw < batch:                                        # :174
        rpw = batch
    return int(rpw)


def n_blocks(n_chunks, cus):
    blocks = (n_chunks + 3) // 4                           # :176
    return max(1, min(blocks, cus * 8))                    # :177-179


def grid_strides(n_rows, rpw, cus):
    """Does some wave take a second chunk (the loop of :91)?"""
    n_chunks = -(-n_rows // rpw)                           # :80
    return n_chunks > 4 * n_blocks(n_chunks, cus)          # :79 n_waves


def partition(n_rows, rpw, batch):
    """The chunk ranges [r0, r1) (:92-93).  `batch` does not move them; it is
    taken so that a caller cannot pass an rpw below it (:174)."""
    assert rpw >= batch
    return [(r0, min(r0 + rpw, n_rows)) for r0 in range(0, n_rows, rpw)]


def runs(ids, chunks, sorted_flag, n_seg):
    """Every run the kernel flushes: (segment, start, end, kind) with kind
    "store", "atomic" or "ignored" (:98-115).  A chunk's `cur` starts at -1
    (:94), so rows of id -1 at its head open no run of their own: they are the
    ignored run the chunk began with, which is what comes out here too."""
    ids = np.asarray(ids)
    n_rows = len(ids)
    out = []
    for r0, r1 in chunks:
        s = ids[r0:r1]
        cut = np.flatnonzero(s[1:] != s[:-1]) + 1 + r0
        for a, b in zip(np.concatenate([[r0], cut]), np.concatenate([cut, [r1]])):
            cur = int(ids[a])
            if cur < 0 or cur >= n_seg:                            # :99
                kind = "ignored"
            else:
                whole = bool(sorted_flag)                          # :100
                if whole and a == r0 and r0 > 0:                   # :101
                    whole = int(ids[r0 - 1]) != cur                # :102
                if whole and b == r1 and r1 < n_rows:              # :103
                    whole = int(ids[r1]) != cur                    # :104
                kind = "store" if whole else "atomic"
            out.append((cur, int(a), int(b), kind))
    return out


def edge_rows(chunks, batch, run_list):
    """The rows at which an off-by-one of the kernel drops or doubles a row:
    first and last row of every chunk, of every batch inside a chunk (the last
    batch ends at the last real row, before the clamped duplicates of :120-127)
    and of every run."""
    rows = []
    for r0, r1 in chunks:
        rb = np.arange(r0, r1, batch)
        rows += [rb, np.minimum(rb + batch, r1) - 1]
    rows.append(np.array([a for _, a, _, _ in run_list], np.int64))
    rows.append(np.array([b - 1 for _, _, b, _ in run_list], np.int64))
    return np.unique(np.concatenate(rows).astype(np.int64))


# --------------------------------------------------------------------------
# the reference: TF's init-then-max, no chunks, no sorting
# --------------------------------------------------------------------------
def reference(data, ids, n_seg):
    """unsorted_segment_max in float32 (max is exact): every cell starts at
    lowest(), ids outside [0, n_seg) are dropped."""
    data = np.asarray(data, np.float32)
    ids = np.asarray(ids).astype(np.int64)
    ref = np.full((n_seg, data.shape[1]), LOWEST, np.float32)
    ok = (ids >= 0) & (ids < n_seg)
    np.maximum.at(ref, ids[ok], data[ok])
    return ref


def canonical_bits(ref):
    """The one bit pattern of a result (include/pointgnn_hip.h): what
    `reference` gives with a zero written as +0.0."""
    return (np.asarray(ref, np.float32) + np.float32(0.0)).view(np.uint32)


# --------------------------------------------------------------------------
# witness data
# --------------------------------------------------------------------------
def witness_data(n_rows, n_cols, n_seg, ids, edges, seed=0):
    """-> list of [n_rows, n_cols] float32 arrays (one per seed).  All values
    of an array are distinct, of mixed sign, and exact.  Over the seeds every
    row of `edges` with an id in range is, in some column, the sole maximum of
    its segment: skip the row and that cell changes.  In such a column every
    other row of the segment is negative and the witness is positive or a
    small negative number in turn, so a segment combined from several atomic
    runs meets both branches of atomic_max_f32 in one cell."""
    ids = np.asarray(ids).astype(np.int64)
    assert n_rows * n_cols + 4 < 2 ** 24          # magnitudes stay exact
    ok = (ids >= 0) & (ids < n_seg)
    e = np.asarray(edges, np.int64)
    e = e[ok[e]]
    e = e[np.lexsort((e, ids[e]))]                # by segment, then by row
    seg = ids[e]
    idx = np.arange(len(e))
    first = np.ones(len(e), bool)
    first[1:] = seg[1:] != seg[:-1]
    rank = idx - np.maximum.accumulate(np.where(first, idx, 0))
    n_seeds = int(rank.max()) // n_cols + 1 if len(e) else 1
    assert len(e) < 2 ** 21
    out = []
    for k in range(n_seeds):
        rng = np.random.default_rng(1000 * seed + k)
        mag = (rng.permutation(n_rows * n_cols) + 4).astype(
            np.float32).reshape(n_rows, n_cols)
        data = mag * (rng.integers(0, 2, mag.shape) * 2 - 1).astype(np.float32)
        sel = rank // n_cols == k
        rows, cols, segs = e[sel], rank[sel] % n_cols, seg[sel]
        wit = np.zeros((max(n_seg, 1), n_cols), bool)
        wit[segs, cols] = True
        mask = np.zeros((n_rows, n_cols), bool)
        mask[ok] = wit[ids[ok]]
        data[mask] = -mag[mask]
        j = np.arange(len(rows))
        data[rows, cols] = np.where(
            j % 2 == 0, mag[rows, cols],
            -(0.5 + j * 2.0 ** -21)).astype(np.float32)   # in (-1.5, -0.5]
        out.append(data)
    return out


def witnessed_rows(datas, ids, n_seg):
    """Rows that are the sole maximum of their segment in some column of some
    array of `datas` (values are distinct, so a maximum is the sole one)."""
    ids = np.asarray(ids).astype(np.int64)
    ok = np.flatnonzero((ids >= 0) & (ids < n_seg))
    hit = np.zeros(len(ids), bool)
    for d in datas:
        assert np.unique(d).size == d.size, "witness values are not distinct"
        hit[ok] |= (d[ok] == reference(d, ids, n_seg)[ids[ok]]).any(1)
    return np.flatnonzero(hit)


# --------------------------------------------------------------------------
# id recipes
# --------------------------------------------------------------------------
def make_ids(recipe, n_rows, n_seg):
    """int32 ids of a recipe (a tuple of a name and integers).

      ("period", p, shift)   (row + shift) // p: non-decreasing runs of p rows
      ("own",)               every row its own segment
      ("gaps", p)            1 + 2 * (row // p): empty segments at both ends
                             and between any two that are not
      ("oob", p)             row // p - 2: a negative prefix; the recipe's
                             n_seg leaves a suffix >= n_seg
      ("all_oob",)           -3 for the first half, n_seg + 1 for the rest
      ("minus1", p)          row // p - 1: -1 in the first p rows
      ("random", s)          uniform in [0, n_seg), seeded s, unsorted
      ("random_oob", s)      uniform in [-2, n_seg + 2), unsorted
      ("shuffled", p, s)     ("period", p, 0) in a random order
    """
    r = np.arange(n_rows, dtype=np.int64)
    kind = recipe[0]
    if kind == "period":
        ids = (r + recipe[2]) // recipe[1]
    elif kind == "own":
        ids = r
    elif kind == "gaps":
        ids = 1 + 2 * (r // recipe[1])
    elif kind == "oob":
        ids = r // recipe[1] - 2
    elif kind == "all_oob":
        ids = np.where(r < n_rows // 2, -3, n_seg + 1)
    elif kind == "minus1":
        ids = r // recipe[1] - 1
    elif kind == "random":
        ids = np.random.default_rng(recipe[1]).integers(0, n_seg, n_rows)
    elif kind == "random_oob":
        ids = np.random.default_rng(recipe[1]).integers(-2, n_seg + 3, n_rows)
    elif kind == "shuffled":
        ids = np.random.default_rng(recipe[2]).permutation(r // recipe[1])
    else:
        raise ValueError(recipe)
    return ids.astype(np.int32)


def recipe_n_seg(recipe, n_rows):
    kind = recipe[0]
    last = n_rows - 1
    if kind == "period":
        return (last + recipe[2]) // recipe[1] + 1
    if kind == "own":
        return n_rows
    if kind == "gaps":
        return 1 + 2 * (last // recipe[1]) + 2      # one empty one at the end
    if kind == "oob":
        return max(1, last // recipe[1] - 2 - 1)    # the last two ids are past
    if kind == "all_oob":
        return 5
    if kind == "minus1":
        return max(1, last // recipe[1])
    if kind in ("random", "random_oob"):
        return max(1, n_rows // 6)
    if kind == "shuffled":
        return last // recipe[1] + 1
    raise ValueError(recipe)


SORTED_KINDS = ("period", "own", "gaps", "oob", "all_oob", "minus1")


# --------------------------------------------------------------------------
# the case table
# --------------------------------------------------------------------------
Case = collections.namedtuple(
    "Case", "name n_rows n_cols n_seg ld_data ld_out data_off out_off sorted "
            "rpw_tunable nt recipe")

# columns at both ends of every instantiation: n_cols -> what forces the form
COLS = {
    (4, 1, 16): ((4, {}), (256, {})),
    (4, 2, 8): ((260, {}), (512, {})),
    (4, 4, 4): ((516, {}), (1024, {})),
    (4, 8, 2): ((1028, {}), (2048, {})),
    (1, 1, 16): ((1, {}), (63, {}), (64, {"ld_data": 65})),
    (1, 4, 8): ((65, {}), (255, {}), (256, {"data_off": 1})),
    (1, 16, 2): ((257, {}), (1023, {}), (1024, {"ld_out": 1025})),
}


def _case(name, n_rows, n_cols, recipe, sorted_, rpw, nt, ld_data=None,
          ld_out=None, data_off=0, out_off=0, n_seg=None):
    if n_seg is None:
        n_seg = recipe_n_seg(recipe, n_rows)
    assert bool(sorted_) <= (recipe[0] in SORTED_KINDS), name
    return Case(name, n_rows, n_cols, n_seg, ld_data or n_cols,
                ld_out or n_cols, data_off, out_off, int(sorted_), rpw, nt,
                recipe)


def _rows_for(n_cols):
    return 203 if n_cols >= 1024 else 333       # <= 2.5 MB of data


def _rpw_tunables(batch):
    return (0, 1, batch, batch + 1, 32, 33)


def _sorted_recipes(rpw):
    return (("period", 3, 0),                # every kind of seam
            ("period", rpw, 0),              # a cut at every r0 and r1
            ("period", rpw, rpw // 2),       # a run across every r0 and r1
            ("period", 3 * rpw + 5, 0),      # runs over three whole chunks
            ("own",), ("gaps", 5), ("oob", 7), ("all_oob",), ("minus1", 3))


def _unsorted_recipes(i):
    return (("random", i), ("random_oob", i), ("shuffled", 5, i),
            ("period", 3, 0))                # sorted ids without the promise


def _spec_name(inst, n_cols, kw):
    forced = "".join("_%s%d" % (k.replace("_", ""), v)
                     for k, v in sorted(kw.items()))
    return "v%dj%db%d_c%d" % (inst + (n_cols,)) + forced


def _build_max_cases():
    cases = []
    i = n_sorted = n_unsorted = 0
    # A. both ends of every instantiation x sorted x nt; the rows-per-wave
    #    tunable and the id recipe rotate
    for inst in INSTANTIATIONS:
        batch = inst[2]
        for n_cols, kw in COLS[inst]:
            n_rows = _rows_for(n_cols)
            for sorted_ in (1, 0):
                for nt in (1, 0):
                    tun = _rpw_tunables(batch)[i % 6]
                    rpw = resolve_rpw(n_rows, batch, tun, CPU_TEST_CUS)
                    if sorted_:
                        rec = _sorted_recipes(rpw)[n_sorted % 9]
                        n_sorted += 1
                    else:
                        rec = _unsorted_recipes(i)[n_unsorted % 4]
                        n_unsorted += 1
                    cases.append(_case(
                        "ends_%s_s%d_nt%d" % (_spec_name(inst, n_cols, kw),
                                              sorted_, nt),
                        n_rows, n_cols, rec, sorted_, tun, nt, **kw))
                    i += 1
    # B. rows around one batch, as one short range (auto: 32 rows per wave)
    #    and at one batch per wave (tunable 1, raised to BATCH)
    for inst in INSTANTIATIONS:
        batch = inst[2]
        n_cols, kw = COLS[inst][0]
        for n_rows in sorted({1, batch - 1, batch, batch + 1} - {0}):
            for tun in (0, 1):
                cases.append(_case(
                    "rows%d_%s_rpw%d" % (n_rows, _spec_name(inst, n_cols, kw),
                                         tun),
                    n_rows, n_cols, ("period", 3, 1), 1, tun, i % 2, **kw))
                i += 1
    # C. every rows-per-wave tunable on every instantiation, sorted, on the
    #    recipe with every kind of seam
    for inst in INSTANTIATIONS:
        batch = inst[2]
        n_cols, kw = COLS[inst][-1]
        for tun in _rpw_tunables(batch):
            cases.append(_case(
                "rpw%d_%s" % (tun, _spec_name(inst, n_cols, kw)),
                _rows_for(n_cols), n_cols, ("period", 3, 0), 1, tun, i % 2,
                **kw))
            i += 1
        # ... and one segment over several whole chunks of one batch each
        cases.append(_case("span_%s" % _spec_name(inst, n_cols, kw),
                           _rows_for(n_cols), n_cols,
                           ("period", 3 * batch + 5, 0), 1, batch, i % 2, **kw))
    # D. every sorted recipe at 32 rows per wave, vector and scalar
    for n_cols in (300, 65):
        for rec in _sorted_recipes(32):
            cases.append(_case(
                "ids_%s_c%d" % ("_".join(map(str, rec)), n_cols),
                333, n_cols, rec, 1, 0, i % 2))
            i += 1
    # E. the same 300 columns taken three ways
    for sorted_ in (1, 0):
        rec = ("period", 3, 0) if sorted_ else ("random", 7)
        for tag, kw in (("aligned", {}),
                        ("lddata304_off1", {"ld_data": 304, "data_off": 1}),
                        ("ldout304", {"ld_out": 304})):
            cases.append(_case("c300_%s_s%d" % (tag, sorted_), 333, 300, rec,
                               sorted_, 0, 1, **kw))
    # F. an offset output pointer alone (a scalar kernel on an aligned shape)
    cases.append(_case("c256_outoff1_s1", 333, 256, ("period", 3, 0), 1, 0, 1,
                       out_off=1))
    # G. refusals
    rec = ("period", 3, 0)
    cases += [
        _case("refuse_c2052_aligned", 8, 2052, rec, 1, 0, 1),
        _case("refuse_c1025", 8, 1025, rec, 1, 0, 1),
        _case("refuse_c1028_dataoff1", 8, 1028, rec, 1, 0, 1, data_off=1),
        _case("refuse_ldout_below_ncols", 8, 300, rec, 1, 0, 1, ld_out=296),
    ]
    return cases


MAX_CASES = _build_max_cases()

# what pgnn_last_error() must say for the refused cases
REFUSAL_TEXT = {"refuse_c2052_aligned": b"n_cols > 2048",
                "refuse_c1025": b"n_cols > 1024",
                "refuse_c1028_dataoff1": b"n_cols > 1024",
                "refuse_ldout_below_ncols": b"row stride smaller than n_cols"}


def grid_stride_cases(cus):
    """More chunks than the capped grid has waves (4 x 8 x CUs): the chunk
    loop of scatter_max.hip:91 takes a second turn.  One vector, one scalar."""
    n_rows = 16 * (4 * 8 * cus + 1000)
    return [_case("stride_v4_c4", n_rows, 4, ("period", 3, 0), 1, 16, 1),
            _case("stride_v1_c3", n_rows, 3, ("period", 3, 0), 1, 16, 0)]


def case_dispatch(c):
    # the output pointer sits one guard row behind the offset: with a row
    # stride that is no multiple of 4 the vector form is already off, with one
    # that is the guard row does not move the pointer's 16-byte phase
    return dispatch(c.n_cols, c.ld_data, c.ld_out, c.data_off, c.out_off)


class Model(object):
    """What the launcher does with a case on a device of `cus` CUs."""

    def __init__(self, c, cus=CPU_TEST_CUS, sorted_=None, rpw_tunable=None):
        self.case = c
        self.inst = case_dispatch(c)
        assert not isinstance(self.inst, str), c.name
        self.batch = self.inst[2]
        self.sorted = c.sorted if sorted_ is None else sorted_
        tun = c.rpw_tunable if rpw_tunable is None else rpw_tunable
        self.rpw = resolve_rpw(c.n_rows, self.batch, tun, cus)
        self.chunks = partition(c.n_rows, self.rpw, self.batch)
        self.ids = make_ids(c.recipe, c.n_rows, c.n_seg)
        self.runs = runs(self.ids, self.chunks, self.sorted, c.n_seg)
        self.edges = edge_rows(self.chunks, self.batch, self.runs)
        self.strides = grid_strides(c.n_rows, self.rpw, cus)

    def witness(self):
        c = self.case
        return witness_data(c.n_rows, c.n_cols, c.n_seg, self.ids, self.edges,
                            seed=len(c.name))


def runnable(cases):
    return [c for c in cases if not isinstance(case_dispatch(c), str)]


def refused(cases):
    return [c for c in cases if isinstance(case_dispatch(c), str)]


# --------------------------------------------------------------------------
# special values
# --------------------------------------------------------------------------
DENORM_MIN = np.float32(1.4e-45)
DENORM = np.float32(1e-39)
_NINF, _PINF = np.float32(-np.inf), np.float32(np.inf)

# the rows of one segment each (no NaN: unspecified in TF, not pinned here)
SPECIAL_SEGMENTS = (
    ("neg_zero_only", (-0.0, -0.0)),
    ("neg_zero_pos_zero", (-0.0, 0.0)),
    ("neg_inf_only", (_NINF, _NINF)),
    ("neg_inf_finite", (_NINF, -5.0)),
    ("neg_inf_lowest", (_NINF, LOWEST)),
    ("pos_inf", (_PINF, 3.0)),
    ("lowest_only", (LOWEST, LOWEST)),
    ("flt_max", (FLT_MAX, 1.0)),
    ("denorm_min_both_signs", (DENORM_MIN, -DENORM_MIN)),
    ("neg_denorms", (-DENORM_MIN, -DENORM)),
    ("pos_denorms", (DENORM, DENORM_MIN)),
    ("neg_denorm_normal", (-DENORM, -1.0)),
    ("denorm_both_signs", (-DENORM, DENORM)),
    ("neg_denorm_neg_zero", (-DENORM_MIN, -0.0)),
)

# (name, ids_sorted, rows-per-wave tunable (1 = one batch), nt, shuffle rows)
SPECIAL_VARIANTS = (("sorted", 1, 0, 1, False), ("sorted_batch", 1, 1, 1, False),
                    ("sorted_rpw33", 1, 33, 1, False),
                    ("unsorted", 0, 0, 1, False), ("shuffled", 0, 0, 1, True),
                    ("sorted_nt0", 1, 0, 0, False))


def special_input(n_cols):
    """-> (data [3 * segments, n_cols], ids): segment s holds the two values
    (a, b) of SPECIAL_SEGMENTS[s] as rows a, b, a in even columns and b, a, b
    in odd ones.  Three rows each put a segment across row 16 and one across
    row 32, where one batch or 32 rows per wave end: sorted, most segments are
    plain-stored and those two are combined atomically; at 33 rows per wave
    the cut falls between two segments."""
    vals = np.array([v for _, v in SPECIAL_SEGMENTS], np.float32)   # [S, 2]
    data = np.empty((3 * len(vals), n_cols), np.float32)
    for c in range(n_cols):
        v = vals if c % 2 == 0 else vals[:, ::-1]
        data[:, c] = v[:, [0, 1, 0]].reshape(-1)
    ids = np.repeat(np.arange(len(vals)), 3).astype(np.int32)
    return data, ids


def special_case(n_cols, variant):
    name, sorted_, tun, nt, _ = variant
    n = 3 * len(SPECIAL_SEGMENTS)
    return Case("special_c%d_%s" % (n_cols, name), n, n_cols,
                len(SPECIAL_SEGMENTS), n_cols, n_cols, 0, 0, sorted_, tun, nt,
                ("period", 3, 0))


# the ordinary cases that must give one bit pattern on every path too
ONE_PATTERN_CASES = ("c300_aligned_s1", "ids_period_3_0_c65",
                     "rpw0_v4j8b2_c2048")


# --------------------------------------------------------------------------
# scatter-sum / scatter-mean
# --------------------------------------------------------------------------
SumCase = collections.namedtuple(
    "SumCase", "name n_rows n_cols n_seg ld_data ld_out seed")


def sum_cases(cus):
    """Padded strides (the hipMemset2DAsync fill), ids from -2 to n_seg + 2.
    `add_strides`: n_rows * n_cols above the add kernel's 256 * 16 * CUs
    threads; `finish_strides`: n_seg * n_cols above the mean finish's
    256 * 4096 (scatter_max.hip:401-403, :441-442)."""
    big = -(-(256 * 16 * cus + 1) // 300)
    fin = -(-(256 * 4096 + 1) // 300)
    return [SumCase("c1", 500, 1, 40, 3, 2, 1),
            SumCase("c37", 500, 37, 40, 40, 41, 2),
            SumCase("c300", 500, 300, 40, 304, 301, 3),
            SumCase("add_strides", big, 300, 40, 301, 304, 4),
            SumCase("finish_strides", 500, 300, fin, 301, 304, 5)]


def sum_input(c):
    """-> (data int-valued float32 in [-8, 8], ids, sum int64 [n_seg, n_cols],
    counts).  Segment 0 and the last one are empty, segment 1 has one row."""
    rng = np.random.default_rng(c.seed)
    data = rng.integers(-8, 9, (c.n_rows, c.n_cols)).astype(np.float32)
    ids = rng.integers(-2, c.n_seg + 3, c.n_rows).astype(np.int32)
    ids[(ids == 0) | (ids == c.n_seg - 1)] = 2
    ids[ids == 1] = 3
    ids[c.n_rows // 2] = 1
    ids[:4] = [-2, -1, c.n_seg, c.n_seg + 2]
    ok = (ids >= 0) & (ids < c.n_seg)
    s = np.zeros((c.n_seg, c.n_cols), np.int64)
    np.add.at(s, ids[ok], data[ok].astype(np.int64))
    cnt = np.bincount(ids[ok], minlength=c.n_seg)
    return data, ids, s, cnt
