#!/usr/bin/env python
"""Generate tests/golden/detect_codec_canonical.npz by RUNNING THE REFERENCE'S
OWN CODE (needs the reference checkout; the fixture travels, this script's
imports do not): models/box_encoding.py is pure NumPy and is imported
unmodified, like make_golden_detect.py does.

Per label map (`car`, `ped`; 500 rows each, labels over the whole table plus
Background and DontCare):

  labels, xyz (+-40), encoded ~ N(0, 0.6)        -> decoded
  boxes (centre = xyz + N(0, 1.5), sizes 0.3-6,
         yaw +-pi), float32                      -> boxes_encoded, roundtrip
  boxes64 / xyz64 (the same draws before the
         float32 cast)                           -> enc64_xyz32, enc64_xyz64
                                                    (float64 encode cast to
                                                    float32, train.py:120-130)

    python tests/golden/make_golden_codec_canonical.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("POINTGNN_REFERENCE", "/root/reference")

LABEL_MAPS = {
    # run.py:244-250
    "car": {'Background': 0, 'Car': 1, 'DontCare': 3},
    "ped": {'Background': 0, 'Pedestrian': 1, 'Cyclist': 3, 'DontCare': 5},
}


def reference_box_encoding():
    sys.path.insert(0, REF)
    try:
        from models import box_encoding
    finally:
        sys.path.remove(REF)
    return box_encoding


def draw(rng, label_map, rows):
    """The inputs of one label map; float64 draws and their float32 casts."""
    nlab = max(label_map.values()) + 1
    labels = rng.integers(0, nlab, (rows, 1)).astype(np.int32)
    xyz64 = rng.uniform(-40, 40, (rows, 3))
    encoded = rng.normal(0, 0.6, (rows, 1, 7)).astype(np.float32)
    boxes64 = np.concatenate([
        xyz64[:, None, :] + rng.normal(0, 1.5, (rows, 1, 3)),
        rng.uniform(0.3, 6, (rows, 1, 3)),
        rng.uniform(-np.pi, np.pi, (rows, 1, 1))], axis=2)
    return labels, xyz64, encoded, boxes64


def main():
    be = reference_box_encoding()
    enc_fn = be.get_box_encoding_fn(
        'classaware_all_class_box_canonical_encoding')
    dec_fn = be.get_box_decoding_fn(
        'classaware_all_class_box_canonical_encoding')
    out = {}
    for seed, (name, lm) in enumerate(LABEL_MAPS.items()):
        rng = np.random.default_rng(301 + seed)
        labels, xyz64, encoded, boxes64 = draw(rng, lm, 500)
        xyz = xyz64.astype(np.float32)
        boxes = boxes64.astype(np.float32)
        pre = "%s_" % name
        out[pre + "labels"] = labels
        out[pre + "xyz"] = xyz
        out[pre + "xyz64"] = xyz64
        out[pre + "encoded"] = encoded
        out[pre + "decoded"] = dec_fn(labels, xyz, encoded, lm)
        out[pre + "boxes"] = boxes
        out[pre + "boxes64"] = boxes64
        enc = enc_fn(labels, xyz, boxes, lm)
        out[pre + "boxes_encoded"] = enc
        back = dec_fn(labels, xyz, enc, lm)
        out[pre + "roundtrip"] = back
        out[pre + "enc64_xyz32"] = enc_fn(labels, xyz, boxes64, lm).astype(
            np.float32)
        out[pre + "enc64_xyz64"] = enc_fn(labels, xyz64, boxes64, lm).astype(
            np.float32)
        for k in ("decoded", "boxes_encoded", "roundtrip"):
            assert out[pre + k].dtype == np.float32
        err = np.abs(back.astype(np.float64) - boxes)
        print("%s: reference round trip max |diff| = %.3g" % (name, err.max()))
    np.savez_compressed(os.path.join(HERE, "detect_codec_canonical.npz"),
                        **out)


if __name__ == "__main__":
    main()
