"""NumPy restatement of `classaware_all_class_box_canonical_{encoding,decoding}`
written from the arithmetic contract, for
the tests of the HIP entries.

An anchor is horizontal (label) or vertical (label + 1, turned by H = pi/2);
Q = pi/4; (p, q) = (l, w) horizontal, (w, l) vertical.

  encode  d = box[0:3] - xyz (every column, every label)
          a = yaw (horizontal) or yaw - H (vertical)
          out0 = (d0 cos a - d2 sin a)/p, out1 = d1/h,
          out2 = (d0 sin a + d2 cos a)/q, out3..5 = log(size/median),
          out6 = a/Q
  decode  a = e6 Q
          out0 = e0 p cos a + e2 q sin a, out1 = e1 h,
          out2 = -e0 p sin a + e2 q cos a, out3..5 = exp(e) median,
          out6 = a (horizontal) or a + H (vertical); then + xyz on 0..2

Only column 0 of a row whose label has an anchor is transformed.

float32 form: medians, Q, H and the angle are float32; cos, sin, exp and log
are evaluated in double on the float32 argument and rounded once; products,
sums and quotients are float32 in the order written above.  float64 form:
everything in double on the inputs as they are.

Each function also returns M [R, 2]: for output columns 0 and 2 of box column
0 the term magnitude (|t1| + |t2|)/divisor of the two-term sum (divisor 1 when
decoding; 0 for rows that are not transformed) -- the scale the rounding-error
bounds of the tests are stated in.
"""
import os

import numpy as np

MEDIAN_SIZE = {            # (l, h, w), KITTI training-set medians
    'Cyclist': (1.76, 1.75, 0.6),
    'Van': (4.98, 2.13, 1.88),
    'Tram': (14.66, 3.61, 2.6),
    'Car': (3.88, 1.5, 1.63),
    'Misc': (2.52, 1.65, 1.51),
    'Pedestrian': (0.88, 1.77, 0.65),
    'Truck': (10.81, 3.34, 2.63),
    'Person_sitting': (0.75, 1.26, 0.59),
}

LABEL_MAPS = {
    "car": {'Background': 0, 'Car': 1, 'DontCare': 3},
    "ped": {'Background': 0, 'Pedestrian': 1, 'Cyclist': 3, 'DontCare': 5},
}


def anchors(label_map):
    """(label value, (l, h, w), vertical) in the order the codec visits them;
    a later anchor with the same label value wins."""
    for name, label in label_map.items():
        if name in ("Background", "DontCare"):
            continue
        yield int(label), MEDIAN_SIZE[name], False
        yield int(label) + 1, MEDIAN_SIZE[name], True


def active_rows(labels, label_map):
    """bool [R]: rows whose label has an anchor."""
    values = [label for label, _, _ in anchors(label_map)]
    return np.isin(np.asarray(labels).reshape(-1), values)


class _F32(object):
    """The float32 contract: float32 constants, double transcendentals
    rounded once."""
    dtype = np.float32

    @staticmethod
    def fn(f, x):
        return f(x.astype(np.float64)).astype(np.float32)


class _F64(object):
    dtype = np.float64

    @staticmethod
    def fn(f, x):
        return f(x)


def _encode(A, labels, xyz, boxes, label_map):
    t = A.dtype
    lab = np.asarray(labels).reshape(-1)
    if t == np.float32:
        b = np.asarray(boxes, np.float32)
        x = np.asarray(xyz, np.float32)
    else:
        b = np.asarray(boxes, np.float64)
        x = np.asarray(xyz)     # float32 vertices widen in the subtraction
    d = b.astype(t, copy=True)
    d[:, :, 0:3] = b[:, :, 0:3] - x[:, None, :]
    out = d.copy()
    mag = np.zeros((len(lab), 2), np.float64)
    Q, H = t(np.pi * 0.25), t(np.pi * 0.5)
    for label, (l, h, w), vertical in anchors(label_map):
        m = lab == label
        l, h, w = t(l), t(h), t(w)
        p, q = (w, l) if vertical else (l, w)
        a = d[m, 0, 6] - H if vertical else d[m, 0, 6]
        c, s = A.fn(np.cos, a), A.fn(np.sin, a)
        d0, d2 = d[m, 0, 0], d[m, 0, 2]
        t1, t2 = d0 * c, d2 * s
        out[m, 0, 0] = (t1 - t2) / p
        mag[m, 0] = (np.abs(t1.astype(np.float64)) + np.abs(t2)) / p
        t1, t2 = d0 * s, d2 * c
        out[m, 0, 2] = (t1 + t2) / q
        mag[m, 1] = (np.abs(t1.astype(np.float64)) + np.abs(t2)) / q
        out[m, 0, 1] = d[m, 0, 1] / h
        out[m, 0, 3] = A.fn(np.log, d[m, 0, 3] / l)
        out[m, 0, 4] = A.fn(np.log, d[m, 0, 4] / h)
        out[m, 0, 5] = A.fn(np.log, d[m, 0, 5] / w)
        out[m, 0, 6] = a / Q
    return out, mag


def _decode(A, labels, xyz, encoded, label_map):
    t = A.dtype
    lab = np.asarray(labels).reshape(-1)
    e = np.asarray(encoded, t)
    x = np.asarray(xyz, t)
    out = e.copy()
    mag = np.zeros((len(lab), 2), np.float64)
    Q, H = t(np.pi * 0.25), t(np.pi * 0.5)
    for label, (l, h, w), vertical in anchors(label_map):
        m = lab == label
        l, h, w = t(l), t(h), t(w)
        p, q = (w, l) if vertical else (l, w)
        a = e[m, 0, 6] * Q
        c, s = A.fn(np.cos, a), A.fn(np.sin, a)
        e0p, e2q = e[m, 0, 0] * p, e[m, 0, 2] * q
        t1, t2 = e0p * c, e2q * s
        out[m, 0, 0] = t1 + t2
        mag[m, 0] = np.abs(t1.astype(np.float64)) + np.abs(t2)
        t1, t2 = -e0p * s, e2q * c
        out[m, 0, 2] = t1 + t2
        mag[m, 1] = np.abs(t1.astype(np.float64)) + np.abs(t2)
        out[m, 0, 1] = e[m, 0, 1] * h
        out[m, 0, 3] = A.fn(np.exp, e[m, 0, 3]) * l
        out[m, 0, 4] = A.fn(np.exp, e[m, 0, 4]) * h
        out[m, 0, 5] = A.fn(np.exp, e[m, 0, 5]) * w
        out[m, 0, 6] = a + H if vertical else a
    out[:, :, 0:3] = out[:, :, 0:3] + x[:, None, :]
    return out, mag


def canonical_encode_f32(labels, xyz, boxes, label_map):
    """-> (encoded float32 [R,B,7], M [R,2])"""
    return _encode(_F32, labels, xyz, boxes, label_map)


def canonical_decode_f32(labels, xyz, encoded, label_map):
    """-> (decoded float32 [R,B,7], M [R,2])"""
    return _decode(_F32, labels, xyz, encoded, label_map)


def canonical_encode_f64(labels, xyz, boxes, label_map):
    """float64 boxes, float32 or float64 vertices -> (encoded float64, M)."""
    return _encode(_F64, labels, xyz, boxes, label_map)


def canonical_decode_f64(labels, xyz, encoded, label_map):
    return _decode(_F64, labels, xyz, encoded, label_map)


# ---- the bars both test files hold a codec to (tests/test_box_codec_cpu.py's
# docstring derives them)
EPS = 2.0 ** -23


def fixture(name):
    """The reference's values for label map `name` (keys without the prefix)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "golden", "detect_codec_canonical.npz"))
    return {k[len(name) + 1:]: z[k] for k in z.files
            if k.startswith(name + "_")}


def check_f32(kind, got, ref, mag, active):
    """The float32 bars; returns the measured maxima
    (columns 0/2 in units of 2^-23 * M, columns 3-5 in ulp or absolute)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got[:, 1:], ref[:, 1:])          # other columns
    assert np.array_equal(got[~active], ref[~active])      # inactive labels
    g, r = got[active, 0].astype(np.float64), ref[active, 0].astype(np.float64)
    assert np.array_equal(g[:, 1], r[:, 1])
    assert np.array_equal(g[:, 6], r[:, 6])
    m = mag[active]
    if kind == "decode":
        m = m + np.abs(r[:, [0, 2]])
    ratio = np.abs(g[:, [0, 2]] - r[:, [0, 2]]) / (EPS * m)
    size = np.abs(g[:, 3:6] - r[:, 3:6])
    if kind == "decode":
        size = size / np.spacing(np.maximum(
            np.abs(got[active, 0, 3:6]), np.abs(ref[active, 0, 3:6]))
        ).astype(np.float64)
    out = (float(ratio.max()), float(size.max()))
    print("%s: columns 0/2 max |diff|/(2^-23 %s) = %.3f, columns 3-5 max %s = "
          "%.3g" % (kind, "(M+|out|)" if kind == "decode" else "M", out[0],
                    "ulp" if kind == "decode" else "|diff|", out[1]))
    assert ratio.max() <= 6.0
    if kind == "decode":
        assert size.max() <= 3.0
    else:
        np.testing.assert_allclose(got[active, 0, 3:6], ref[active, 0, 3:6],
                                   rtol=3e-7, atol=3e-7)
    return out


def check_f64(got, ref, mag, active):
    """One float32 spacing, plus 2^-50 * M on columns 0 and 2."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape
    tol = np.spacing(np.maximum(np.abs(got), np.abs(ref))).astype(np.float64)
    tol[:, 0, 0] += 2.0 ** -50 * mag[:, 0]
    tol[:, 0, 2] += 2.0 ** -50 * mag[:, 1]
    diff = np.abs(got.astype(np.float64) - ref)
    print("float64 encode: identical %.5f, max diff/tol %.3g" % (
        np.mean(got == ref), (diff / tol).max()))
    assert np.all(diff <= tol)
    assert np.array_equal(got[~active], ref[~active])
