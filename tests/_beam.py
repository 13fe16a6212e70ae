"""Shared by test_beam_downsample_cpu.py and test_gpu_beam_downsample.py: the
float64 / int64 NumPy restatement of the DEFINED beam decimation
(include/pointgnn_hip.h, "beam decimation"; scripts/point_cloud_downsample.py
:19-53 with the unseeded KMeans replaced by a deterministic clustering) and a
seeded HDL-64-like scan generator."""
import numpy as np

SCALE = 2.0 ** 30


def cos_valid(velo):
    """(cos float64 [n], valid bool [n]) of [n,4] float32 rows: :22-25, :29
    restated per column -- float32 squares added left to right, a correctly
    rounded float32 root, the quotient in float64."""
    velo = np.asarray(velo, np.float32).reshape(-1, 4)
    x, y, z = velo[:, 0], velo[:, 1], velo[:, 2]
    with np.errstate(all="ignore"):
        total = ((x * x + y * y) + z * z).astype(np.float32)
        norm = np.sqrt(total.astype(np.float64)).astype(np.float32)
        cos = z.astype(np.float64) / norm.astype(np.float64)
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (norm != 0)
    return cos, valid


def quantise(cos):
    return np.rint(cos * SCALE).astype(np.int64)


class Centers(object):
    """centers float64 [B]; info int32 [4] = (n_valid, passes, status, 0);
    labels int64 [n]: the cluster of every row under the last pass's
    partition (-1 for invalid rows or status 1 / 2); counts: rows per cluster."""

    def __init__(self, centers, info, labels, counts):
        self.centers, self.info = centers, info
        self.labels, self.counts = labels, counts

    n_valid = property(lambda self: int(self.info[0]))
    iterations = property(lambda self: int(self.info[1]))
    status = property(lambda self: int(self.info[2]))


def beam_centers(velo, n_beams=64, max_iter=300):
    B = int(n_beams)
    cos, valid = cos_valid(velo)
    n = len(cos)
    labels = np.full(n, -1, np.int64)
    q_all = quantise(np.where(valid, cos, 0.0))
    s = np.sort(q_all[valid])
    v = len(s)

    def failed(status):
        return Centers(np.zeros(B), np.array([v, 0, status, 0], np.int32),
                       labels, np.zeros(B, np.int64))
    if v < B:
        return failed(1)
    # farthest-first: np.argmax returns the smallest index of the maximum
    chosen = [s[0]]
    d = np.abs(s - s[0])
    for _ in range(B - 1):
        i = int(np.argmax(d))
        if d[i] == 0:
            return failed(2)
        chosen.append(s[i])
        d = np.minimum(d, np.abs(s - s[i]))
    c = np.sort(np.array(chosen, np.int64)).astype(np.float64)
    S = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    s2 = 2.0 * s.astype(np.float64)
    prev, status, passes = None, 3, 0
    for it in range(1, int(max_iter) + 1):
        m = c[:-1] + c[1:]
        hi = np.concatenate([np.searchsorted(s2, m, side="right"), [v]])
        lo = np.concatenate([[0], hi[:-1]])
        cnt = hi - lo
        mean = (S[hi] - S[lo]).astype(np.float64) / np.where(cnt > 0, cnt, 1)
        c = np.where(cnt > 0, mean, c)
        passes = it
        if prev is not None and np.array_equal(prev, hi):
            status = 0
            break
        prev = hi
    # 2 s <= m_{j+1} puts a row in cluster <= j: rows on a midpoint go down
    labels[valid] = np.searchsorted(m, 2.0 * q_all[valid], side="left")
    return Centers(c / SCALE, np.array([v, passes, status, 0], np.int32),
                   labels, cnt.astype(np.int64))


def kept_mask(velo, centers, rate, status=0):
    """:27-35 vectorised per kept beam; invalid rows and status 1 / 2 keep
    nothing."""
    cos, valid = cos_valid(velo)
    mask = np.zeros(len(cos), bool)
    if status in (1, 2):
        return mask
    ext = np.concatenate([[-1.0], np.asarray(centers, np.float64), [1.0]])
    with np.errstate(invalid="ignore"):
        for i in range(0, len(ext) - 2, int(rate)):
            lower = (ext[i] + ext[i + 1]) / 2
            upper = (ext[i + 1] + ext[i + 2]) / 2
            mask |= (cos > lower) & (cos < upper)
    return mask & valid


def select(velo, centers, rate, status=0):
    velo = np.asarray(velo, np.float32).reshape(-1, 4)
    return velo[kept_mask(velo, centers, rate, status)]


def downsample(velo, rate, n_beams=64, max_iter=300):
    """-> (rows [m,4] float32, Centers)."""
    res = beam_centers(velo, n_beams, max_iter)
    return select(velo, res.centers, rate, res.status), res


def boundary_margin(velo, centers):
    """Smallest |cos - boundary| over the valid rows and the inner cluster
    boundaries (the midpoints of adjacent centres)."""
    cos, valid = cos_valid(velo)
    cos = cos[valid]
    mids = (centers[:-1] + centers[1:]) / 2
    j = np.clip(np.searchsorted(mids, cos), 1, len(mids) - 1)
    return float(np.minimum(np.abs(cos - mids[j - 1]),
                            np.abs(cos - mids[j])).min())


def hdl64_scan(seed, n_az, drop=0.0, jitter_deg=0.02, n_beams=64):
    """A seeded scan like an HDL-64E's: n_beams elevations from +2 to -24.8
    degrees, n_az azimuth steps, per-beam dropout drawn in [0, drop], Gaussian
    elevation jitter, ranges 3-70 m clipped at a ground plane 1.73 m below the
    sensor, rows shuffled.  -> (rows [n,4] float32, beam int64 [n]); beam 0 is
    the highest, so its cosine is the largest."""
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(2.0, -24.8, n_beams))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False)
    el, a = np.meshgrid(elev, az, indexing="ij")
    beam = np.repeat(np.arange(n_beams), n_az)
    el = el.ravel() + np.deg2rad(jitter_deg) * rng.standard_normal(el.size)
    a = a.ravel()
    r = rng.uniform(3, 70, el.size)
    ground = np.where(np.sin(el) < 0,
                      1.73 / np.maximum(-np.sin(el), 1e-6), np.inf)
    r = np.minimum(r, ground)
    keep_p = 1 - rng.uniform(0, drop, n_beams)[beam]
    keep = rng.random(el.size) < keep_p
    xyz = np.stack([r * np.cos(el) * np.cos(a), r * np.cos(el) * np.sin(a),
                    r * np.sin(el)], 1)[keep].astype(np.float32)
    p = rng.permutation(len(xyz))
    refl = rng.random(len(xyz)).astype(np.float32)
    return (np.ascontiguousarray(np.hstack([xyz[p], refl[:, None]])),
            beam[keep][p])
