"""Shared by test_voxel_cpu.py and test_gpu_voxel.py: the seeded inputs of
tests/golden/voxel_average.npz, a NumPy evaluation of the DEFINED form of the
voxel-average down-sampling (kitti_dataset.py:16-48 with a stable argsort and
an explicitly sequential float32 sum), and the three-way comparison rule."""
import hashlib
import os

import numpy as np

from oracle import ingest_oracle as IO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOXELS = (0.05, 0.1, 0.4, 0.8)
# share of rows with more than two points (not bit-compared against the
# reference): measured on the fixture's input, asserted as caps
WIDE_SHARE_CAP = {0.05: 1e-4, 0.1: 1e-4, 0.4: 0.019, 0.8: 0.131}


def tag(voxel):
    return ("%g" % voxel).replace(".", "p")


def load_fixture():
    return np.load(os.path.join(GOLD, "voxel_average.npz"))


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def inputs(fix):
    """(velo [60000,4], image, cam xyz float32 [60000,3]) of the fixture,
    regenerated from their seeds and verified against the stored digests."""
    velo = IO.synthetic_velo_scan(0, n=60000)
    image = IO.synthetic_image(0)
    assert np.array_equal(sha256(velo), fix["velo_sha256"])
    assert np.array_equal(sha256(image), fix["image_sha256"])
    cam = IO.velo_to_cam(velo[:, :3], IO.get_calib(IO.CALIB_LINES))
    assert cam.dtype == np.float32
    assert np.array_equal(sha256(cam), fix["cam_sha256"])
    return velo, image, cam


def wrap_cloud():
    """A few hundred float32 points spread over +-3 km, some sharing a 0.01
    voxel (two at the most, so the sums do not depend on the order): dim_x *
    dim_y * dim_z ~ 2e17, the int32 key wraps."""
    rng = np.random.RandomState(7)
    base = rng.uniform(-3000.0, 3000.0, size=(200, 3))
    twins = base[rng.permutation(200)[:40]] + \
        rng.uniform(0.0, 0.002, size=(40, 3))
    xyz = np.concatenate([base, twins]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    attr = rng.uniform(0.0, 1.0, size=(len(xyz), 1)).astype(np.float32)
    return xyz, attr


def defined_voxel_average(xyz, attr, voxel):
    """-> (xyz f64 [m,3], attr f64 [m,a] or None, lens int64 [m], abs_sums f64
    [m,3+a]).  Points of a voxel are added in ascending original index."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32
    off = np.amin(xyz, axis=0, keepdims=True)
    idx = ((xyz - off) // np.float32(voxel)).astype(np.int32)
    dim = (np.amax(idx, axis=0) + 1).astype(np.int32)
    # wrapping 32-bit arithmetic, spelled out in uint32 and read as int32
    u = idx.astype(np.uint32)
    d = dim.astype(np.uint32)
    keys = (u[:, 0] + u[:, 1] * d[0] + u[:, 2] * d[1] * d[0]).view(np.int32)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    head = np.ones(len(skeys), bool)
    head[1:] = skeys[1:] != skeys[:-1]
    starts = np.nonzero(head)[0]
    lens = np.diff(np.append(starts, len(skeys)))
    cols = xyz if attr is None else np.concatenate(
        [xyz, np.asarray(attr, np.float32)], axis=1)
    rows = cols[order]
    acc = rows[starts].copy()                      # float32
    mag = np.abs(acc).astype(np.float64)
    for s in range(1, int(lens.max())):
        m = lens > s
        if not m.any():
            break
        nxt = rows[starts[m] + s]
        acc[m] = acc[m] + nxt                      # one float32 add per step
        mag[m] += np.abs(nxt)
    out = acc.astype(np.float64) / lens[:, None].astype(np.float64)
    a = None if attr is None else out[:, 3:]
    return out[:, :3], a, lens, mag


def order_bound(lens, abs_sums):
    """Per-row, per-column bound on the difference of two sequential float32
    sums of the same k terms in different orders, after the float64 division:
    2 * gamma_{k-1} * sum|x_i| / k, gamma_n = n u / (1 - n u), u = 2^-24, times
    (1 + 2^-20) for the two float64 divisions."""
    k = lens.astype(np.float64)[:, None]
    u = 2.0 ** -24
    gamma = (k - 1) * u / (1 - (k - 1) * u)
    return 2 * gamma * abs_sums / k * (1 + 2.0 ** -20)


def check_against_reference(voxel, got_xyz, got_attr, lens, abs_sums,
                            ref_lens, ref_wide, ref_narrow_sha, label=""):
    """The three-way rule.  ref_wide: the reference's rows with lens > 2
    ([w, 3+a] float64); ref_narrow_sha: sha256 over the bytes of its rows with
    lens <= 2 (xyz rows, then attr rows)."""
    assert len(lens) == len(ref_lens), "row count"
    assert np.array_equal(lens, ref_lens), "lens"
    wide = lens > 2
    share = float(wide.mean())
    print("%s voxel %g: %d rows, %.4f%% with lens > 2" % (
        label, voxel, len(lens), 100 * share))
    if voxel in WIDE_SHARE_CAP:
        assert share <= WIDE_SHARE_CAP[voxel]
    got = np.concatenate([got_xyz, got_attr], axis=1)
    assert got.dtype == np.float64
    assert np.array_equal(
        sha256(got_xyz[~wide], got_attr[~wide]), ref_narrow_sha), \
        "rows with lens <= 2 are not bit-identical"
    if wide.any():
        diff = np.abs(got[wide] - ref_wide)
        bound = order_bound(lens[wide], abs_sums[wide])
        ratio = float((diff / np.maximum(bound, 1e-300)).max())
        print("%s voxel %g: lens > 2 rows, max |diff| %.3g = %.3f of the "
              "bound; %.2f%% of them differ" % (
                  label, voxel, diff.max(), ratio,
                  100 * float((diff.max(axis=1) > 0).mean())))
        assert (diff <= bound).all()
