"""Beam decimation, no GPU: the NumPy restatement of the DEFINED clustering
(tests/_beam.py) against what scripts/point_cloud_downsample.py computes where
that is defined (the cosine :22-25, the selection :27-35), against the scan
generator's true beams, and against sklearn's KMeans started at our centres.
The device is compared with the same restatement in
test_gpu_beam_downsample.py."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import beam_downsample as BD
import _beam as B

RATES = (1, 2, 3, 4, 8, 64, 65)
# (seed, n_az, dropout, jitter in degrees): the issue's table
SCANS = ((0, 1, 0.0, 0.02), (1, 2, 0.0, 0.02), (2, 8, 0.5, 0.02),
         (3, 40, 0.5, 0.02), (4, 300, 0.5, 0.03), (5, 2000, 0.9, 0.03))

_cache = {}


def scan_result(case):
    if case not in _cache:
        velo, beam = B.hdl64_scan(*case)
        _cache[case] = (velo, beam, B.beam_centers(velo))
    return _cache[case]


# ---- 1. the cosine ------------------------------------------------------------
def test_cos_equals_the_scripts_numpy_expressions():
    rng = np.random.default_rng(11)
    xyz = (rng.standard_normal((10000, 3)) *
           10.0 ** rng.uniform(-3, 2, (10000, 1))).astype(np.float32)
    # norms whose squares are denormal, underflow to zero, or overflow
    xyz[:40] = (rng.standard_normal((40, 3)) * 3e-23).astype(np.float32)
    xyz[40:60] = (rng.standard_normal((20, 3)) * 1e-30).astype(np.float32)
    xyz[60:80] = (rng.standard_normal((20, 3)) * 1e25).astype(np.float32)
    xyz[80] = (0, 0, 0)
    xyz[81] = (0, 0, -0.0)
    xyz[82] = (np.nan, 1, 1)
    xyz[83] = (1, np.inf, 1)
    xyz[84] = (1, 1, -np.inf)
    velo = np.hstack([xyz, np.zeros((10000, 1), np.float32)])
    with np.errstate(all="ignore"):
        # :23-25
        norm = np.sqrt(np.sum(xyz * xyz, axis=1, keepdims=True))
        ref = xyz.dot(np.array([[0], [0], [1]])) / norm
    assert ref.dtype == np.float64 and norm.dtype == np.float32
    cos, valid = B.cos_valid(velo)
    # bit for bit on every valid row; what the script turns into nan or inf
    # (its dot product also multiplies a non-finite x or y by 0) is invalid
    assert np.array_equal(cos[valid], ref[valid, 0])
    assert not valid[~np.isfinite(ref[:, 0])].any()
    sq = (xyz.astype(np.float64) ** 2).sum(1)
    assert ((sq > 0) & (sq < 1.2e-38)).sum() >= 20   # denormal squares
    assert not valid[80:85].any() and not valid[40:60].any()
    assert valid[:40].sum() >= 20 and valid[60:80].all() and valid[85:].all()
    # the int32 key of the kernels holds every q: |cos| <= sqrt(1.5)
    assert np.abs(cos[valid]).max() <= np.sqrt(1.5)


# ---- 2. the selection -----------------------------------------------------------
def _script_selection(cos, centers, rate):
    """:27-35 restated: Python-list bounds with integer ends, strict
    inequalities, the masks of the kept beams or-ed together."""
    bounds = [-1] + np.sort(centers).tolist() + [1]
    total = np.zeros(len(cos), dtype=bool)
    for i in range(0, len(bounds) - 2, rate):
        lower = (bounds[i] + bounds[i + 1]) / 2
        higher = (bounds[i + 1] + bounds[i + 2]) / 2
        total += (cos > lower) * (cos < higher)
    return total


def selection_case():
    """64 hand-set centres and rows that lie exactly on inner boundaries,
    below (-1 + c_0) / 2 and above (c_63 + 1) / 2, among ordinary ones.
    -> (velo, centres, indices of the on-boundary rows)."""
    # integer right triangles: norm and cos = z / norm are exact quotients
    tri = [(4, -3), (12, -5), (15, -8), (24, -7), (40, -9), (35, -12),
           (60, -11), (84, -13), (45, -28), (63, 16), (56, 33)]
    on = np.array([[a, 0, z, 0.5] for a, z in tri], np.float32)
    on_cos = np.array([z / float(np.hypot(a, z)) for a, z in tri])
    d = 2.0 ** -10
    pairs = np.concatenate([on_cos - d, on_cos + d])
    filler = np.linspace(-0.70, 0.52, 200)
    filler = filler[np.abs(filler[:, None] - on_cos[None, :]).min(1) > 0.01]
    centers = np.sort(np.concatenate(
        [pairs, filler[np.linspace(0, len(filler) - 1, 64 - len(pairs)
                                   ).astype(int)]]))
    assert len(np.unique(centers)) == 64
    outer = np.array([[0.1, 0, -1, 1], [0, 0, -5, 2], [0.3, 0.1, -2, 3],
                      [0.1, 0, 1, 4], [0, 0, 2, 5], [0.2, 0.2, 3, 6]],
                     np.float32)
    scan, _ = B.hdl64_scan(21, 30, 0.3)
    rng = np.random.default_rng(5)
    rnd = rng.standard_normal((500, 4)).astype(np.float32)
    velo = np.concatenate([scan[:700], on, rnd, outer, scan[700:]])
    idx_on = 700 + np.arange(len(on))
    return np.ascontiguousarray(velo), centers, idx_on


def test_selection_case_has_boundary_and_outer_rows():
    velo, centers, idx_on = selection_case()
    cos, valid = B.cos_valid(velo)
    assert valid.all()
    mids = (centers[:-1] + centers[1:]) / 2
    assert np.isin(cos[idx_on], mids).all()        # exactly on a boundary
    assert (cos < (-1 + centers[0]) / 2).sum() >= 3
    assert (cos > (centers[-1] + 1) / 2).sum() >= 3
    # strict inequalities: at rate 1 exactly these rows and the outer ones go
    kept = B.kept_mask(velo, centers, 1)
    assert not kept[idx_on].any()
    inner = (cos > (-1 + centers[0]) / 2) & (cos < (centers[-1] + 1) / 2)
    assert np.array_equal(~kept, ~inner | np.isin(cos, mids))


@pytest.mark.parametrize("rate", RATES)
def test_selection_equals_the_scripts_loop(rate):
    velo, centers, _ = selection_case()
    cos, _ = B.cos_valid(velo)
    ref = _script_selection(cos, centers, rate)
    assert np.array_equal(B.kept_mask(velo, centers, rate), ref)
    assert 0 < ref.sum() < len(ref)
    out = B.select(velo, centers, rate)
    assert out.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), velo[ref].view(np.uint32))


# ---- 3. clustering against the generator's beams --------------------------------
@pytest.mark.parametrize("case", SCANS)
def test_every_point_lands_in_its_beam(case):
    velo, beam, res = scan_result(case)
    assert res.status == 0 and res.n_valid == len(velo)
    assert res.iterations >= 2       # the first pass has nothing to equal
    assert np.all(np.diff(res.centers) > 0)
    assert res.counts.min() > 0 and res.counts.sum() == len(velo)
    assert np.array_equal(res.labels, 63 - beam)       # cap 0
    assert B.boundary_margin(velo, res.centers) >= 1e-6
    # the selection's intervals are the clusters: rate 2 keeps clusters 0, 2, ..
    assert np.array_equal(B.kept_mask(velo, res.centers, 2),
                          res.labels % 2 == 0)


def test_result_does_not_depend_on_row_order():
    velo, _, res = scan_result(SCANS[3])
    perm = np.random.default_rng(3).permutation(len(velo))
    again = B.beam_centers(velo[perm])
    assert np.array_equal(again.centers, res.centers)
    assert np.array_equal(again.info, res.info)


# ---- 4. sklearn stays at our centres ---------------------------------------------
@pytest.mark.parametrize("case", SCANS[2:5])
def test_sklearn_kmeans_started_at_our_centres_stays(case):
    cluster = pytest.importorskip("sklearn.cluster")
    velo, _, res = scan_result(case)
    cos, _ = B.cos_valid(velo)
    km = cluster.KMeans(n_clusters=64, init=res.centers.reshape(-1, 1),
                        n_init=1).fit(cos[:, None])
    # a mean of values each quantised by at most 2^-31 moves by at most 2^-31
    assert np.abs(km.cluster_centers_[:, 0] - res.centers).max() <= 2.0 ** -30
    assert np.array_equal(km.labels_, res.labels)


# ---- 5. status, invalid rows, arguments ------------------------------------------
def test_status_1_with_63_valid_rows():
    velo, _ = B.hdl64_scan(0, 1)
    velo = velo.copy()
    velo[7, :3] = 0
    pad = np.zeros((10, 4), np.float32)
    pad[3, 0] = np.nan
    velo = np.concatenate([velo, pad])
    out, res = B.downsample(velo, 1)
    assert res.status == 1 and res.n_valid == 63 and res.iterations == 0
    assert np.array_equal(res.centers, np.zeros(64)) and len(out) == 0
    assert B.beam_centers(velo, n_beams=63).status == 0


def test_status_2_with_63_distinct_values():
    velo, _ = B.hdl64_scan(0, 1)
    velo = np.tile(velo[:63], (4, 1))[:200]
    out, res = B.downsample(velo, 1)
    assert res.status == 2 and res.n_valid == 200 and len(out) == 0
    assert B.beam_centers(velo, n_beams=63).status == 0


def test_invalid_rows_are_excluded_and_never_kept():
    velo, _, res = scan_result(SCANS[3])
    bad = np.array([[0, 0, 0, 1], [np.nan, 1, 1, 1], [1, np.inf, 1, 1],
                    [1, 1, -np.inf, 1], [1e-30, 0, 1e-30, 1]], np.float32)
    pos = np.sort(np.random.default_rng(2).integers(0, len(velo), 40))
    mixed = np.insert(velo, pos, bad[np.arange(40) % len(bad)], axis=0)
    got = B.beam_centers(mixed)
    assert np.array_equal(got.centers, res.centers)
    assert got.n_valid == len(velo) and got.status == 0
    for rate in (1, 2):
        assert np.array_equal(B.select(mixed, got.centers, rate),
                              B.select(velo, res.centers, rate))


def test_max_iter_reached_is_status_3():
    velo, _, full = scan_result(SCANS[3])
    one = B.beam_centers(velo, max_iter=1)
    assert one.status == 3 and one.iterations == 1
    assert np.all(np.diff(one.centers) > 0)
    assert B.beam_centers(velo, max_iter=full.iterations).status == 0


@pytest.mark.parametrize("kwargs", [
    dict(rate=0), dict(rate=-2), dict(rate=1.5), dict(rate=2, n_beams=1),
    dict(rate=2, n_beams=65), dict(rate=2, max_iter=0), dict(rate=True)])
def test_downsample_rejects_bad_arguments(kwargs):
    velo = np.zeros((100, 4), np.float32)
    with pytest.raises(ValueError):
        BD.downsample(velo, **kwargs)


def test_downsample_rejects_bad_shape():
    with pytest.raises(ValueError, match="n, 4"):
        BD.downsample(np.zeros((100, 3), np.float32), 2)


def test_dataset_rejects_bad_rate(tmp_path):
    from pointgnn_amd.kitti_dataset import KittiDataset
    d = str(tmp_path)
    with pytest.raises(ValueError):
        KittiDataset(d, d, d, beam_downsample_rate=0)
    with pytest.raises(ValueError):
        KittiDataset(d, d, d, beam_downsample_rate=2, beam_count=65)
    assert KittiDataset(d, d, d, beam_downsample_rate=2).num_files == 0


def test_cli_parser():
    ap = BD.build_parser()
    a = ap.parse_args(["in", "out", "--rate", "4"])
    assert (a.point_dir, a.output_dir, a.rate, a.beams, a.split) == \
        ("in", "out", 4, 64, None)
    a = ap.parse_args(["in", "out", "--rate", "2", "--beams", "32",
                       "--split", "val.txt"])
    assert (a.rate, a.beams, a.split) == (2, 32, "val.txt")
    for argv in (["in", "out"], ["in", "--rate", "2"],
                 ["in", "out", "--rate", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    with pytest.raises(SystemExit):
        BD.main(["in", "out", "--rate", "0"])
