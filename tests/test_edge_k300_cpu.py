"""The K = 300 order of the scaled edge kernel's last K group (csrc/edge_ws.h,
K300; pgnn_k300_source, pgnn_pack_fc_k300), host side: the permutation restated
in NumPy, the packer's image against the restated one, and the reason the
permutation is what it is -- the MFMA steps meet the twelve real features of
the group in the order they met them in the natural layout, and the fourth
step meets the padding alone."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401


def restated(n=304):
    """src[p]: the feature position p holds.  Position 288 + 4g + s is element
    s of lane group g in the last K group, consumed by MFMA step s; it holds
    element j = 4s + g of the sequence 288, 292, 296, 289, 293, 297, ... (the
    natural layout's chain without its padding), the padding for j >= 12."""
    src = np.arange(n)
    for p in range(288, 304):
        g, s = (p - 288) // 4, (p - 288) % 4
        j = 4 * s + g
        src[p] = 288 + 4 * (j % 3) + j // 3 if j < 12 else 300 + g
    return src


def chain(feature_at):
    """Features in the order the last K group's MFMAs accumulate them: step by
    step, lane groups ascending; None marks a step's padding."""
    return [[feature_at(288 + 4 * g + s) for g in range(4)] for s in range(4)]


def _lib():
    from pointgnn_amd import _lib as L
    return L, L.load()


def test_source_is_the_restated_permutation():
    L, lib = _lib()
    src = restated(336)
    got = np.array([lib.pgnn_k300_source(p) for p in range(336)])
    assert np.array_equal(got, src)
    assert np.array_equal(src[:288], np.arange(288))
    assert np.array_equal(src[304:], np.arange(304, 336))
    assert sorted(src[288:304].tolist()) == list(range(288, 304))
    # the padding: element 3 of every lane group
    assert [p for p in range(288, 304) if src[p] >= 300] == [291, 295, 299, 303]
    from pointgnn_amd import gnn
    assert np.array_equal(gnn.edge_k300_order(), src[:304])
    assert L.EDGE_K300_ORDER == 4


def test_real_products_keep_their_place_in_the_chain():
    src = restated()
    natural = chain(lambda p: p)
    permuted = chain(lambda p: int(src[p]))
    real = lambda steps: [f for step in steps for f in step if f < 300]
    assert real(natural) == real(permuted) == \
        [288, 292, 296, 289, 293, 297, 290, 294, 298, 291, 295, 299]
    # natural: every step ends in a padding feature; permuted: three full
    # steps, then the padding alone
    assert all(step[3] >= 300 and max(step[:3]) < 300 for step in natural)
    assert all(max(step) < 300 for step in permuted[:3])
    assert all(f >= 300 for f in permuted[3])


def test_packed_image_is_the_restated_one():
    L, lib = _lib()
    rng = np.random.default_rng(300)
    k_in = n_out = 300
    w = rng.standard_normal((k_in, n_out)).astype(np.float32)
    b = rng.standard_normal(n_out).astype(np.float32)
    n = lib.pgnn_packed_fc_floats(k_in, n_out)
    got = np.full(n, np.nan, np.float32)
    assert lib.pgnn_pack_fc_k300(w.ctypes.data, b.ctypes.data, k_in, n_out,
                                 got.ctypes.data) == 0
    src = restated()
    padded = np.zeros((304, 304), np.float32)
    padded[:300, :300] = w
    q, t, lane, s = np.meshgrid(np.arange(19), np.arange(19), np.arange(64),
                                np.arange(4), indexing="ij")
    want = np.zeros(n, np.float32)
    want[:19 * 19 * 256] = padded[src[16 * q + 4 * (lane >> 4) + s],
                                  16 * t + (lane & 15)].reshape(-1)
    want[19 * 19 * 256:19 * 19 * 256 + 300] = b
    assert got.tobytes() == want.tobytes()
    # ... which is pgnn_pack_fc's image of the weights with their rows permuted
    rows = padded[src][:, :300].copy()
    plain = np.full(n, np.nan, np.float32)
    assert lib.pgnn_pack_fc(rows.ctypes.data, b.ctypes.data, 304, n_out,
                            plain.ctypes.data) == 0
    assert got.tobytes() == plain.tobytes()
    # and differs from the natural image in the last K group only
    nat = np.empty(n, np.float32)
    assert lib.pgnn_pack_fc(w.ctypes.data, b.ctypes.data, k_in, n_out,
                            nat.ctypes.data) == 0
    differs = np.flatnonzero(got != nat)
    assert len(differs) and differs.min() >= 18 * 19 * 256 and \
        differs.max() < 19 * 19 * 256


def test_columns_helper_and_refusals():
    L, lib = _lib()
    from pointgnn_amd import gnn
    src = restated()
    a = np.arange(3 * 300, dtype=np.float32).reshape(3, 300) + 1
    cols = gnn.edge_k300_columns(a)
    assert cols.shape == (3, 304) and cols.dtype == np.float32
    for p in range(304):
        want = a[:, src[p]] if src[p] < 300 else np.zeros(3, np.float32)
        assert np.array_equal(cols[:, p], want), p
    assert np.array_equal(gnn.edge_k300_columns(a[0]), cols[0])
    w = np.zeros((256, 256), np.float32)
    out = np.zeros(lib.pgnn_packed_fc_floats(256, 256), np.float32)
    for k_in in (256, 299, 304):
        assert lib.pgnn_pack_fc_k300(w.ctypes.data, None, k_in, 256,
                                     out.ctypes.data) == L.E_UNSUPPORTED
    assert lib.pgnn_pack_fc_k300(None, None, 300, 300, None) == L.E_INVALID
