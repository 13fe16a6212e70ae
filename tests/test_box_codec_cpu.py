"""The NumPy restatement of the canonical box codec (tests/_box_codecs.py, the
yardstick of tests/test_gpu_codec_canonical.py) against the values the
reference's own code wrote into tests/golden/detect_codec_canonical.npz -- on
every machine -- and, where the reference checkout is present, against the
imported reference on fresh seeds; and the registry of
pointgnn_amd.box_encoding.

Bars (float32 path; the restatement evaluates cos/sin/exp/log in double and
rounds once, NumPy's float32 routines are ~1.5 ulp accurate):
  columns 1, 6          single float32 operations: bit for bit
  columns 3-5, decode   3 float32 ulp (exp ~1.5 ulp, one rounding of ours, one
                        that can differ in the multiply)
  columns 3-5, encode   rtol = atol = 3e-7 (log of a ratio near 1)
  columns 0, 2          |diff| <= 6 * 2^-23 * M, M the term magnitude of the
                        two-term sum (decode: M + |out|, the xyz add rounds
                        once more): <= 2 ulp per product from the cos/sin
                        discrepancy, then one rounding each for the two
                        products, the sum and the quotient
float64 path: one float32 spacing plus 2^-50 * M on columns 0 and 2."""
import os
import sys

import numpy as np
import pytest

import _box_codecs as BC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.environ.get("POINTGNN_REFERENCE", "/root/reference")
CANONICAL = 'classaware_all_class_box_canonical_encoding'


@pytest.mark.parametrize("name", ["car", "ped"])
def test_restatement_matches_reference_fixture(name):
    f, lm = BC.fixture(name), BC.LABEL_MAPS[name]
    active = BC.active_rows(f["labels"], lm)
    assert active.sum() > 100 and (~active).sum() > 100
    dec, m = BC.canonical_decode_f32(f["labels"], f["xyz"], f["encoded"], lm)
    BC.check_f32("decode", dec, f["decoded"], m, active)
    enc, m = BC.canonical_encode_f32(f["labels"], f["xyz"], f["boxes"], lm)
    BC.check_f32("encode", enc, f["boxes_encoded"], m, active)
    for key, xyz in (("enc64_xyz32", f["xyz"]), ("enc64_xyz64", f["xyz64"])):
        e64, m = BC.canonical_encode_f64(f["labels"], xyz, f["boxes64"], lm)
        BC.check_f64(e64.astype(np.float32), f[key], m, active)
    # the reference's own round trip on these inputs (the GPU test's bar of
    # 2e-5 is ten times its error: half a float32 spacing at |x| ~ 40)
    err = np.abs(f["roundtrip"].astype(np.float64) - f["boxes"])
    print("reference round trip: max |diff| = %.3g" % err.max())
    assert err.max() < 4e-6


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")),
                    reason="reference checkout not present")
@pytest.mark.parametrize("name", ["car", "ped"])
@pytest.mark.parametrize("seed", [11, 12])
def test_restatement_matches_imported_reference(name, seed):
    sys.path.insert(0, REF)
    try:
        from models import box_encoding as ref
    finally:
        sys.path.remove(REF)
    sys.path.insert(0, GOLD)
    try:
        import make_golden_codec_canonical as G
    finally:
        sys.path.remove(GOLD)
    lm = BC.LABEL_MAPS[name]
    labels, xyz64, encoded, boxes64 = G.draw(np.random.default_rng(seed), lm,
                                             4000)
    xyz, boxes = xyz64.astype(np.float32), boxes64.astype(np.float32)
    active = BC.active_rows(labels, lm)
    dec, m = BC.canonical_decode_f32(labels, xyz, encoded, lm)
    BC.check_f32("decode", dec, ref.classaware_all_class_box_canonical_decoding(
        labels, xyz, encoded, lm), m, active)
    enc, m = BC.canonical_encode_f32(labels, xyz, boxes, lm)
    BC.check_f32("encode", enc, ref.classaware_all_class_box_canonical_encoding(
        labels, xyz, boxes, lm), m, active)
    e64, m = BC.canonical_encode_f64(labels, xyz64, boxes64, lm)
    want = ref.classaware_all_class_box_canonical_encoding(
        labels, xyz64, boxes64, lm)
    BC.check_f64(e64.astype(np.float32), want.astype(np.float32), m, active)
    d64, _ = BC.canonical_decode_f64(labels, xyz64, want, lm)
    np.testing.assert_allclose(d64[active, 0], boxes64[active, 0], rtol=1e-12,
                               atol=1e-12)


def test_restatement_leaves_inputs_alone_and_passes_columns_through():
    lm = BC.LABEL_MAPS["ped"]
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 6, (50, 1)).astype(np.int32)
    xyz = rng.uniform(-5, 5, (50, 3)).astype(np.float32)
    boxes = rng.uniform(0.5, 3, (50, 3, 7)).astype(np.float32)
    keep = boxes.copy()
    enc, _ = BC.canonical_encode_f32(labels, xyz, boxes, lm)
    assert np.array_equal(boxes, keep)
    off = boxes.copy()
    off[:, :, 0:3] = boxes[:, :, 0:3] - xyz[:, None, :]
    assert np.array_equal(enc[:, 1:], off[:, 1:])
    plain = ~BC.active_rows(labels, lm)
    assert np.array_equal(enc[plain], off[plain])


def test_registry_serves_both_four_argument_keys():
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import box_encoding as BE
    plain = 'classaware_all_class_box_encoding'
    assert BE.get_box_encoding_fn(plain) is BE.classaware_all_class_box_encoding
    assert BE.get_box_decoding_fn(plain) is BE.classaware_all_class_box_decoding
    assert BE.get_box_encoding_fn(CANONICAL) is \
        BE.classaware_all_class_box_canonical_encoding
    assert BE.get_box_decoding_fn(CANONICAL) is \
        BE.classaware_all_class_box_canonical_decoding
    for key in ('direct_encoding', 'center_box_encoding',
                'voxelnet_box_encoding', 'classaware_voxelnet_box_encoding'):
        for get in (BE.get_box_encoding_fn, BE.get_box_decoding_fn):
            with pytest.raises(NotImplementedError, match="three arguments"):
                get(key)
        assert BE.get_encoding_len(key) == 7
    assert BE.get_encoding_len(plain) == BE.get_encoding_len(CANONICAL) == 7
    with pytest.raises(KeyError):
        BE.get_box_encoding_fn('no_such_encoding')
    # the restatement's medians are the package's
    assert BC.MEDIAN_SIZE == BE.median_object_size_map


def test_new_entries_validate_before_any_hip_call():
    """Sizes, null pointers and n_rows == 0 are decided without a device."""
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    lib = L.load()
    for name in ("pgnn_box_decode_canonical_f32",
                 "pgnn_box_encode_canonical_f32",
                 "pgnn_box_encode_canonical_f64",
                 "pgnn_box_encode_canonical_f64_xyz64"):
        fn = getattr(lib, name)
        assert name in L.exported_symbols()
        assert fn(None, None, None, None, 0, 0, 1, None, None) == 0
        assert fn(None, None, None, None, 0, -1, 1, None, None) == -1
        assert b"bad size" in lib.pgnn_last_error()
        assert fn(None, None, None, None, 0, 4, 0, None, None) == -1
        assert fn(None, None, None, None, -1, 4, 1, None, None) == -1
        assert fn(None, None, None, None, 0, 4, 1, None, None) == -1
        assert b"null pointer" in lib.pgnn_last_error()
