"""Beam decimation on the device (csrc/beam.hip: pgnn_beam_centers,
pgnn_beam_select) through pointgnn_amd.beam_downsample and KittiDataset,
against the NumPy restatement of the DEFINED clustering in tests/_beam.py.
Centres, passes, n_valid, status and the kept rows are compared with ==, the
rows as uint32."""
import os
import warnings

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import beam_downsample as BD
from pointgnn_amd import configs
import _beam as B

pytestmark = pytest.mark.gpu

SORT_TILE = 2048     # PGNN_SORT_TILE of csrc/sort.h: keys per block per pass
SCAN_TILE = 2048     # kScanTile of csrc/beam.hip: rows per block of the scan
TABLE = 4096         # kTable of csrc/beam.hip: above it the LDS search table
#                      holds every 2nd, 3rd, ... sorted key instead of every one
RATES = (1, 2, 3, 4, 8, 64, 65)

_scans = {}


def scan(seed, n_az, drop=0.0, jitter=0.02, rows=None):
    key = (seed, n_az, drop, jitter)
    if key not in _scans:
        _scans[key] = B.hdl64_scan(seed, n_az, drop, jitter)[0]
    velo = _scans[key]
    assert rows is None or len(velo) >= rows
    return velo if rows is None else np.ascontiguousarray(velo[:rows])


def device_centers(velo, n_beams=64, max_iter=300):
    c, info = BD.beam_centers(velo, n_beams=n_beams, max_iter=max_iter)
    return c.cpu().numpy(), info.cpu().numpy()


def device_select(velo, centers, rate, info=None):
    rows, count = BD.beam_select(velo, centers, rate, info=info)
    m = int(count.item())
    assert tuple(rows.shape) == (len(velo), 4)
    return rows[:m].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_restatement(velo, n_beams=64, max_iter=300, rates=(1, 2)):
    want = B.beam_centers(velo, n_beams, max_iter)
    c, info = device_centers(velo, n_beams, max_iter)
    print("n=%d beams=%d: info device %s host %s" % (
        len(velo), n_beams, info.tolist(), want.info.tolist()))
    assert np.array_equal(info, want.info)
    assert np.array_equal(c, want.centers)
    for rate in rates:
        got = device_select(velo, c, rate, info=info)
        assert same_bits(got, B.select(velo, want.centers, rate, want.status))
    return want


# ---- 1. sizes ---------------------------------------------------------------------
def test_every_point_a_centre():
    want = check_against_restatement(scan(0, 1))
    assert want.n_valid == 64 and want.status == 0


@pytest.mark.parametrize("n", [
    65, 371, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, TABLE - 1, TABLE,
    TABLE + 1, 2 * TABLE + 1])
def test_sizes_at_the_tile_edges(n):
    assert SCAN_TILE == SORT_TILE   # one set of sizes serves both
    src = scan(1, 2) if n == 65 else scan(2, 8, 0.3) if n == 371 \
        else scan(3, 200, 0.4)
    want = check_against_restatement(scan_rows(src, n))
    assert want.status == 0 and want.n_valid == n


def scan_rows(velo, n):
    assert len(velo) >= n
    return np.ascontiguousarray(velo[:n])


@pytest.mark.parametrize("case,passes", [
    ((4, 300, 0.5, 0.03), None),      # about 15 k rows
    ((5, 2000, 0.9, 0.03), None),     # about 63 k rows, beams of unequal size
    ((7, 2000, 0.5, 0.06), 5),        # about 99 k rows, beams overlap: the
    #                                   partition is not the beams any more
])
def test_generated_scans(case, passes):
    velo = scan(*case)
    want = check_against_restatement(velo, rates=(2, 8))
    assert want.status == 0
    if passes is not None:
        assert want.iterations == passes


@pytest.mark.parametrize("n_beams", [2, 3, 63, 64])
def test_beam_counts(n_beams):
    check_against_restatement(scan(2, 8, 0.3, rows=371), n_beams=n_beams,
                              rates=(1, 2, 3))


# ---- 2. ties ----------------------------------------------------------------------
def test_ties_go_to_the_first_sorted_index():
    """40 beams below the horizon and their mirror images above it, every row
    eight times at ranges scaled by powers of two: every cosine is shared by
    eight rows bit for bit and -cos belongs to eight more, so equal farthest
    candidates occur from the third centre on."""
    one, beam = B.hdl64_scan(0, 1)
    low = one[np.argsort(beam)][20:60]
    assert (low[:, 2] < 0).all()
    both = np.concatenate([low, low * np.float32([1, 1, -1, 1])])
    velo = np.concatenate([both * np.float32([s, s, s, 1])
                           for s in (1, 2, 4, 8, 0.5, 0.25, 16, 32)])
    velo = np.ascontiguousarray(
        velo[np.random.default_rng(9).permutation(len(velo))])
    cos, _ = B.cos_valid(velo)
    s = np.sort(B.quantise(cos))
    assert len(np.unique(s)) == 80 and np.array_equal(s, -s[::-1])
    d = np.minimum(np.abs(s - s[0]), np.abs(s - s[-1]))
    assert len(np.unique(s[d == d.max()])) == 2    # two farthest candidates
    for n_beams in (64, 33, 4):
        check_against_restatement(velo, n_beams=n_beams, rates=(1, 2))


# ---- 3. invalid rows, status --------------------------------------------------------
BAD_ROWS = np.array([[0, 0, 0, 1], [np.nan, 1, 1, 1], [1, np.inf, 1, 1],
                     [1, 1, -np.inf, 1], [1e-30, 0, 1e-30, 1],
                     [0, -0.0, 0, 1]], np.float32)


def test_invalid_rows_sprinkled_through_a_scan():
    velo = scan(3, 40, 0.5)
    pos = np.sort(np.random.default_rng(2).integers(0, len(velo), 60))
    mixed = np.ascontiguousarray(
        np.insert(velo, pos, BAD_ROWS[np.arange(60) % len(BAD_ROWS)], axis=0))
    want = check_against_restatement(mixed, rates=(1, 2, 4))
    assert want.n_valid == len(velo) and want.status == 0
    clean, _ = device_centers(velo)
    assert np.array_equal(clean, want.centers)


def test_rows_whose_squares_are_denormal():
    """x*x + y*y + z*z in float32 denormals: the norm loses bits and cos
    leaves [-1, 1] (up to sqrt(1.5)); the device must not flush them."""
    tiny = (np.random.default_rng(4).standard_normal((60, 4)) * 3e-23
            ).astype(np.float32)
    cos, valid = B.cos_valid(tiny)
    assert valid.sum() >= 30 and np.abs(cos[valid]).max() > 1.0
    velo = np.ascontiguousarray(np.concatenate([scan(3, 40, 0.5), tiny]))
    want = check_against_restatement(velo, rates=(1, 2))
    assert want.n_valid == len(velo) - 60 + valid.sum()


def test_status_1_and_2_keep_nothing():
    velo = np.concatenate([scan(0, 1), BAD_ROWS, BAD_ROWS])
    velo[7, :3] = 0
    want = check_against_restatement(velo)
    assert want.status == 1 and want.n_valid == 63
    with pytest.raises(ValueError, match="valid points"):
        BD.downsample(velo, 2)
    dup = np.ascontiguousarray(np.tile(scan(0, 1)[:63], (4, 1))[:200])
    want = check_against_restatement(dup)
    assert want.status == 2 and want.n_valid == 200
    with pytest.raises(ValueError, match="distinct"):
        BD.downsample(dup, 2)
    # the select entry keeps rows when it is not told
    c = B.beam_centers(scan(3, 40, 0.5)).centers
    assert len(device_select(dup, c, 1)) == len(B.select(dup, c, 1)) > 0


def test_max_iter_1_is_status_3_with_valid_centres():
    velo = scan(3, 40, 0.5)
    want = check_against_restatement(velo, max_iter=1)
    assert want.status == 3 and want.iterations == 1
    with pytest.warns(RuntimeWarning, match="max_iter"):
        out = BD.downsample(velo, 2, max_iter=1)
    assert same_bits(out, B.select(velo, want.centers, 2))
    full = B.beam_centers(velo)
    exact = check_against_restatement(velo, max_iter=full.iterations)
    assert exact.status == 0


def test_no_points():
    empty = np.zeros((0, 4), np.float32)
    c, info = device_centers(empty)
    assert info.tolist() == [0, 0, 1, 0] and np.array_equal(c, np.zeros(64))
    rows, count = BD.beam_select(empty, np.linspace(-0.4, 0.03, 64), 2)
    assert int(count.item()) == 0 and tuple(rows.shape) == (0, 4)


def test_entries_reject_bad_arguments():
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    t = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = _lib.ptr(t)
    for n_beams, max_iter in ((1, 300), (65, 300), (64, 0)):
        assert lib.pgnn_beam_centers(p, 10, n_beams, max_iter, p, 32768, p, p,
                                     None) == _lib.E_INVALID
    assert lib.pgnn_beam_centers(None, 10, 64, 300, p, 32768, p, p,
                                 None) == _lib.E_INVALID
    assert lib.pgnn_beam_centers(p, 10, 64, 300, p, 16, p, p,
                                 None) == _lib.E_WORKSPACE
    for n_beams, rate in ((1, 1), (65, 1), (64, 0)):
        assert lib.pgnn_beam_select(p, 10, p, n_beams, rate, None, p, 32768, p,
                                    p, None) == _lib.E_INVALID
    assert lib.pgnn_beam_select(p, 10, None, 64, 1, None, p, 32768, p, p,
                                None) == _lib.E_INVALID
    assert lib.pgnn_beam_workspace_bytes(10) <= 32768


# ---- 4. the select entry alone ------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_select_with_hand_set_centres(rate):
    from test_beam_downsample_cpu import selection_case
    velo, centers, idx_on = selection_case()
    velo = velo.copy()
    bits = velo.view(np.uint32)
    bits[::7, 3] = 0x80000000        # -0.0
    bits[3::11, 3] = 0x7FC12345      # a NaN with a payload
    bits[5::13, 3] = 0xFFA00001
    got = device_select(velo, centers, rate)
    want = B.select(velo, centers, rate)
    assert same_bits(got, want)
    assert 0 < len(want) < len(velo)
    w = want.view(np.uint32)[:, 3]
    assert (w == 0x80000000).any() and (w == 0x7FC12345).any()
    if rate == 1:
        # strict bounds: rows exactly on a boundary go even when every beam
        # is kept; the kept rows are a subsequence in the original order
        keep = B.kept_mask(velo, centers, 1)
        assert not keep[idx_on].any()


# ---- 5. two streams -----------------------------------------------------------------
def test_two_streams_at_once_give_the_same_bits():
    import torch
    a, b = scan(4, 300, 0.5, 0.03), scan(3, 200, 0.4)
    dev = torch.device("cuda", 0)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    want = [(B.beam_centers(v), v) for v in (a, b)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    out = []
    for _ in range(3):
        for s, t in zip(streams, (ta, tb)):
            with torch.cuda.stream(s):
                c, info = BD.beam_centers(t)
                rows, count = BD.beam_select(t, c, 2, info=info)
                out.append((c, info, rows, count))
    torch.cuda.synchronize()
    for k, (c, info, rows, count) in enumerate(out):
        res, v = want[k % 2]
        assert np.array_equal(c.cpu().numpy(), res.centers)
        assert np.array_equal(info.cpu().numpy(), res.info)
        assert same_bits(rows[:int(count.item())].cpu().numpy(),
                         B.select(v, res.centers, 2))


def test_cuda_in_cuda_out_numpy_in_numpy_out():
    import torch
    velo = scan(3, 40, 0.5)
    want, _ = B.downsample(velo, 4)
    out = BD.downsample(velo, 4)
    assert isinstance(out, np.ndarray) and same_bits(out, want)
    out = BD.downsample(torch.from_numpy(velo).cuda(), 4)
    assert out.is_cuda and same_bits(out.cpu().numpy(), want)


# ---- 6. / 7. the dataset and the frame loop --------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Three generated frames of about 5 k rows as a KITTI-object tree, and
    the same tree with write_downsampled_dataset(rate=2)'s velodyne."""
    from pointgnn_amd import kitti_dataset as KD, synthetic as S
    root = tmp_path_factory.mktemp("beam_kitti")
    dirs = [str(root / d) for d in ("image_2", "velodyne", "calib")]
    for d in dirs:
        os.makedirs(d)
    scans = []
    for i in range(3):
        velo = B.hdl64_scan(30 + i, 100, 0.4)[0]
        name = "%06d" % i
        velo.tofile(os.path.join(dirs[1], name + ".bin"))
        # the calibration is fitted to the returns in front of the camera
        front = velo[(velo[:, 0] > 3) & (np.abs(velo[:, 1]) < 0.8 * velo[:, 0])]
        cam = np.stack([-front[:, 1] - 0.004, -front[:, 2] - 0.076,
                        front[:, 0] - 0.272], 1)
        lines, (height, width) = S.synthetic_calib(cam)
        with open(os.path.join(dirs[2], name + ".txt"), "w") as f:
            f.writelines(lines)
        S.write_png_header(os.path.join(dirs[0], name + ".png"), height, width)
        scans.append(velo)
    out_dir = str(root / "velodyne_rate2")
    paths = BD.write_downsampled_dataset(KD.KittiDataset(*dirs), out_dir, 2)
    assert [os.path.basename(p) for p in paths] == \
        ["%06d.bin" % i for i in range(3)]
    return dirs, out_dir, scans


def test_written_files_equal_the_restatement(tree):
    dirs, out_dir, scans = tree
    for i, velo in enumerate(scans):
        want, res = B.downsample(velo, 2)
        assert res.status == 0 and 0.3 * len(velo) < len(want) < 0.7 * len(velo)
        with open(os.path.join(out_dir, "%06d.bin" % i), "rb") as f:
            assert f.read() == want.tobytes()


def _same_points(a, b):
    import torch
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x, y)
        else:
            assert x.dtype == y.dtype and np.array_equal(x, y)
    return int(a[0].shape[0])


def test_dataset_fetch_equals_the_written_directory(tree):
    import torch
    from pointgnn_amd import kitti_dataset as KD
    dirs, out_dir, scans = tree
    dec = KD.KittiDataset(*dirs, beam_downsample_rate=2)
    pre = KD.KittiDataset(dirs[0], out_dir, dirs[2])
    plain = KD.KittiDataset(*dirs)
    xyz_range = ((0.0, 60.0), (-30.0, 30.0), (-3.0, 1.0))
    image = np.random.default_rng(1).integers(
        0, 256, KD.png_size(os.path.join(dirs[0], "000000.png")) + (3,),
        dtype=np.uint8)
    for i in range(3):
        n = _same_points(dec.get_velo_points(i), pre.get_velo_points(i))
        assert n < len(plain.get_velo_points(i).xyz) == len(scans[i])
        for kw in (dict(), dict(xyz_range=xyz_range)):
            assert _same_points(dec.get_velo_points(i, **kw),
                                pre.get_velo_points(i, **kw)) > 0
        for kw in (dict(), dict(xyz_range=xyz_range),
                   dict(downsample_voxel_size=0.8),
                   dict(downsample_voxel_size=0.4, xyz_range=xyz_range)):
            for method in ("get_cam_points", "get_cam_points_in_image",
                           "get_cam_points_in_image_with_rgb"):
                assert _same_points(getattr(dec, method)(i, **kw),
                                    getattr(pre, method)(i, **kw)) > 0, \
                    (method, kw)
            got, want = [ds.get_cam_points_in_image_with_rgb(
                i, deferred=True, **kw) for ds in (dec, pre)]
            torch.cuda.current_stream().wait_event(got.event)
            torch.cuda.current_stream().wait_event(want.event)
            assert _same_points(got.result(), want.result()) > 0
        if i == 0:
            assert _same_points(
                dec.get_cam_points_in_image_with_rgb(i, image=image),
                pre.get_cam_points_in_image_with_rgb(i, image=image)) > 0
    # the crop sees fewer rows than the plain dataset's
    assert dec.get_cam_points_in_image(0).xyz.shape[0] < \
        plain.get_cam_points_in_image(0).xyz.shape[0]


def test_frame_loop_decimating_in_the_fetch(tree, tmp_path):
    """run_dataset over the frames, decimated in the fetch (on the loader
    thread when pipelined) and read from the written directory: the same txt
    files byte for byte."""
    import torch
    from pointgnn_amd import kitti_dataset as KD, run as RUN, weights
    dirs, out_dir, _ = tree
    cfg = configs.get_config("car_auto_T3")
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    dec = KD.KittiDataset(*dirs, beam_downsample_rate=2)
    pre = KD.KittiDataset(dirs[0], out_dir, dirs[2])
    files = {}
    for name, ds, pipelined in (("pre_seq", pre, False), ("pre_pipe", pre, True),
                                ("dec_seq", dec, False), ("dec_pipe", dec, True)):
        out = str(tmp_path / name)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            td = RUN.run_dataset(ds, cfg, None, out, params=params,
                                 pipelined=pipelined, in_flight=2, prefetch=2)
        torch.cuda.synchronize()
        assert td['frames'] == 3
        files[name] = []
        for i in range(3):
            with open(os.path.join(out, "data", "%06d.txt" % i), "rb") as f:
                files[name].append(f.read())
    print("bytes per frame:", [len(b) for b in files["pre_seq"]])
    assert sum(len(b) > 1 for b in files["pre_seq"]) >= 1, "no detections"
    for name in ("pre_pipe", "dec_seq", "dec_pipe"):
        assert files[name] == files["pre_seq"], name
