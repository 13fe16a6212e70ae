"""The canonical box codec on the device
(`classaware_all_class_box_canonical_{encoding,decoding}`:
pgnn_box_{decode,encode}_canonical_f32, pgnn_box_encode_canonical_f64[_xyz64])
through the public functions: against the values the reference's own code
wrote into tests/golden/detect_codec_canonical.npz, against the NumPy
restatement of the arithmetic contract (tests/_box_codecs.py), and through
every caller the registry reaches -- detect_boxes, the deferred candidate
path, the frame loop and the training targets.

Bars: tests/test_box_codec_cpu.py's docstring (the restatement is held to the
same ones on every machine).  Measured on the fixture, MI355X:
  decode  columns 0/2 max |diff|/(2^-23 (M+|out|)): car 0.451, ped 0.864
          columns 3-5 max ulp: car 2, ped 3
  encode  columns 0/2 max |diff|/(2^-23 M): car 1.025, ped 1.645
          columns 3-5 max |diff|: car 1.19e-07, ped 2.38e-07
  round trip max |diff|: car 1.26e-06, ped 9.54e-07 (bar 2e-5; the
          reference's own 1.43e-06)
  float64 encode: every value identical to the reference's
"""
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs
import _box_codecs as BC

pytestmark = pytest.mark.gpu

PLAIN = 'classaware_all_class_box_encoding'
CANONICAL = 'classaware_all_class_box_canonical_encoding'


def _fns():
    from pointgnn_amd import box_encoding as BE
    return (BE.get_box_encoding_fn(CANONICAL),
            BE.get_box_decoding_fn(CANONICAL))


# ---- 1. fixture parity ---------------------------------------------------------
@pytest.mark.parametrize("name", ["car", "ped"])
def test_fixture_parity_f32(name):
    enc_fn, dec_fn = _fns()
    f, lm = BC.fixture(name), BC.LABEL_MAPS[name]
    active = BC.active_rows(f["labels"], lm)
    keep = {k: f[k].copy() for k in ("labels", "xyz", "encoded", "boxes")}
    dec = dec_fn(f["labels"], f["xyz"], f["encoded"], lm)
    _, m = BC.canonical_decode_f32(f["labels"], f["xyz"], f["encoded"], lm)
    BC.check_f32("decode", dec, f["decoded"], m, active)
    enc = enc_fn(f["labels"], f["xyz"], f["boxes"], lm)
    _, m = BC.canonical_encode_f32(f["labels"], f["xyz"], f["boxes"], lm)
    BC.check_f32("encode", enc, f["boxes_encoded"], m, active)
    for k, v in keep.items():
        assert np.array_equal(f[k], v)           # inputs are never written


# ---- 2. pass-through -----------------------------------------------------------
def test_pass_through_equals_the_plain_codec_and_tensor_io():
    import torch
    from pointgnn_amd import box_encoding as BE
    enc_fn, dec_fn = _fns()
    lm = BC.LABEL_MAPS["ped"]
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 8, (300, 1)).astype(np.int32)  # out of table too
    xyz = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    boxes = np.concatenate([
        rng.uniform(-6, 6, (300, 3, 3)), rng.uniform(0.3, 6, (300, 3, 3)),
        rng.uniform(-np.pi, np.pi, (300, 3, 1))], axis=2).astype(np.float32)
    inactive = ~BC.active_rows(labels, lm)
    assert 50 < inactive.sum() < 250
    for fn, plain_fn, restated in (
            (enc_fn, BE.classaware_all_class_box_encoding,
             BC.canonical_encode_f32),
            (dec_fn, BE.classaware_all_class_box_decoding,
             BC.canonical_decode_f32)):
        got = fn(labels, xyz, boxes, lm)
        plain = plain_fn(labels, xyz, boxes, lm)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        assert got.shape == (300, 3, 7)
        assert np.array_equal(got[inactive], plain[inactive])
        assert np.array_equal(got[:, 1:], plain[:, 1:])
        assert not np.array_equal(got[~inactive, 0], plain[~inactive, 0])
        assert np.array_equal(got, restated(labels, xyz, boxes, lm)[0])
        dev = fn(torch.from_numpy(labels).cuda(), torch.from_numpy(xyz).cuda(),
                 torch.from_numpy(boxes).cuda(), lm)
        assert dev.is_cuda and dev.dtype == torch.float32
        assert np.array_equal(dev.cpu().numpy(), got)


# ---- 3. launch edges -----------------------------------------------------------
@pytest.mark.parametrize("rows,per_row", [(1, 1), (255, 1), (256, 1), (257, 1),
                                          (86, 3)])
def test_launch_edges_equal_the_restatement(rows, per_row):
    enc_fn, dec_fn = _fns()
    lm = BC.LABEL_MAPS["car"]
    rng = np.random.default_rng(rows)
    labels = rng.integers(0, 4, (rows, 1)).astype(np.int32)
    labels[-1] = 2                      # the last box is a transformed one
    xyz = rng.uniform(-40, 40, (rows, 3)).astype(np.float32)
    boxes = np.concatenate([
        xyz[:, None, :] + rng.normal(0, 1.5, (rows, per_row, 3)),
        rng.uniform(0.3, 6, (rows, per_row, 3)),
        rng.uniform(-np.pi, np.pi, (rows, per_row, 1))],
        axis=2).astype(np.float32)
    encoded = rng.normal(0, 0.6, (rows, per_row, 7)).astype(np.float32)
    got = enc_fn(labels, xyz, boxes, lm)
    want, _ = BC.canonical_encode_f32(labels, xyz, boxes, lm)
    assert got.shape == want.shape and np.array_equal(got, want)
    got = dec_fn(labels, xyz, encoded, lm)
    want, _ = BC.canonical_decode_f32(labels, xyz, encoded, lm)
    assert got.shape == want.shape and np.array_equal(got, want)
    b64 = boxes.astype(np.float64) + 1e-9
    got = enc_fn(labels, xyz.astype(np.float64), b64, lm)
    want, m = BC.canonical_encode_f64(labels, xyz.astype(np.float64), b64, lm)
    assert got.shape == want.shape
    BC.check_f64(got, want.astype(np.float32), m, BC.active_rows(labels, lm))


def test_zero_rows():
    import torch
    enc_fn, dec_fn = _fns()
    lm = BC.LABEL_MAPS["car"]
    lab, xyz = np.zeros((0, 1), np.int32), np.zeros((0, 3), np.float32)
    for fn in (enc_fn, dec_fn):
        out = fn(lab, xyz, np.zeros((0, 1, 7), np.float32), lm)
        assert isinstance(out, np.ndarray)
        assert out.shape == (0, 1, 7) and out.dtype == np.float32
        out = fn(torch.from_numpy(lab).cuda(), torch.from_numpy(xyz).cuda(),
                 torch.zeros((0, 4, 7), device="cuda"), lm)
        assert out.is_cuda and tuple(out.shape) == (0, 4, 7)
    out = enc_fn(lab, xyz.astype(np.float64), np.zeros((0, 1, 7)), lm)
    assert out.shape == (0, 1, 7) and out.dtype == np.float32


# ---- 4. round trip -------------------------------------------------------------
@pytest.mark.parametrize("name", ["car", "ped"])
def test_round_trip(name):
    enc_fn, dec_fn = _fns()
    f, lm = BC.fixture(name), BC.LABEL_MAPS[name]
    back = dec_fn(f["labels"], f["xyz"],
                  enc_fn(f["labels"], f["xyz"], f["boxes"], lm), lm)
    print("round trip: max |diff| = %.3g (the reference's own: %.3g)" % (
        np.abs(back.astype(np.float64) - f["boxes"]).max(),
        np.abs(f["roundtrip"].astype(np.float64) - f["boxes"]).max()))
    np.testing.assert_allclose(back, f["boxes"], rtol=2e-5, atol=2e-5)


# ---- 5. float64 encode ---------------------------------------------------------
@pytest.mark.parametrize("name", ["car", "ped"])
@pytest.mark.parametrize("xyz_key,ref_key", [("xyz", "enc64_xyz32"),
                                             ("xyz64", "enc64_xyz64")])
def test_float64_encode(name, xyz_key, ref_key):
    import torch
    enc_fn, _ = _fns()
    f, lm = BC.fixture(name), BC.LABEL_MAPS[name]
    assert f["boxes64"].dtype == np.float64
    assert f[xyz_key].dtype == (np.float64 if xyz_key == "xyz64"
                                else np.float32)
    active = BC.active_rows(f["labels"], lm)
    _, m = BC.canonical_encode_f64(f["labels"], f[xyz_key], f["boxes64"], lm)
    got = enc_fn(f["labels"], f[xyz_key], f["boxes64"], lm)
    BC.check_f64(got, f[ref_key], m, active)
    dev = enc_fn(torch.from_numpy(f["labels"]).cuda(),
                 torch.from_numpy(f[xyz_key]).cuda(),
                 torch.from_numpy(f["boxes64"]).cuda(), lm)
    assert dev.is_cuda and dev.dtype == torch.float32
    assert np.array_equal(dev.cpu().numpy(), got)


# ---- 6. detection wiring -------------------------------------------------------
def test_detect_boxes_honours_the_canonical_key():
    import torch
    from pointgnn_amd import nms
    enc_fn, dec_fn = _fns()
    lm = BC.LABEL_MAPS["car"]
    k, nc = 300, 4
    rng = np.random.default_rng(6)
    logits = rng.normal(0, 0.3, (k, nc))
    logits[:, 0] += 3.0                           # background wins ...
    hot = rng.choice(k, 40, replace=False)        # ... except at 40 vertices
    logits[hot, rng.integers(1, 3, 40)] += 5.0
    probs = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
             ).astype(np.float32)
    xyz = np.stack([rng.uniform(-6, 6, k), rng.uniform(0.8, 1.6, k),
                    rng.uniform(8, 20, k)], 1).astype(np.float32)
    enc = rng.normal(0, 0.25, (k, nc, 7)).astype(np.float32)
    p_d, x_d, e_d = (torch.from_numpy(a).cuda() for a in (probs, xyz, enc))
    got = nms.detect_boxes(p_d, e_d, x_d, lm, 0.01,
                           box_encoding_method=CANONICAL)
    # by hand: decode all K*nc boxes, select, the same NMS entry
    box_labels = torch.arange(nc, dtype=torch.int32, device="cuda").repeat(k)
    decoded = dec_fn(box_labels.reshape(-1, 1),
                     x_d.repeat_interleave(nc, dim=0),
                     e_d.reshape(k * nc, 1, 7), lm)
    idx, labels = nms.select_candidates(p_d)
    n = int(idx.numel())
    assert 30 <= n <= 60
    sel = idx.long()
    want = nms.nms_boxes_3d_uncertainty(
        labels, decoded[sel, 0], p_d.reshape(-1)[sel], overlapped_thres=0.01,
        overlapped_fn=nms.overlapped_boxes_3d_fast_poly, appr_factor=100.0,
        top_k=-1, attributes=torch.arange(n, dtype=torch.int32, device="cuda"))
    assert len(got) == 4 and 0 < int(got[0].numel()) <= n
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # the deferred candidate path keeps the same rows
    out, cnt, cand_xyz = nms.detect_candidates_deferred(
        p_d, e_d, x_d, idx, labels, lm, 0.01, box_encoding_method=CANONICAL)
    kept = int(cnt.item())
    assert kept == int(got[0].numel())
    for a, b in zip(out, got):
        assert torch.equal(a[:kept], b)
    assert torch.equal(cand_xyz, x_d[(sel // nc)])
    # and the key was honoured: the plain method decodes other boxes
    from pointgnn_amd import box_encoding as BE
    plain = BE.classaware_all_class_box_decoding(
        box_labels.reshape(-1, 1), x_d.repeat_interleave(nc, dim=0),
        e_d.reshape(k * nc, 1, 7), lm)
    a, b = decoded[sel, 0], plain[sel, 0]
    assert bool((a[:, 0] != b[:, 0]).all()) and bool((a[:, 2] != b[:, 2]).all())
    assert torch.equal(a[:, 3:], b[:, 3:]) and torch.equal(a[:, 1], b[:, 1])
    other = nms.detect_boxes(p_d, e_d, x_d, lm, 0.01,
                             box_encoding_method=PLAIN)
    assert other[1].shape != got[1].shape or not torch.equal(other[1], got[1])


# ---- 7. frame loop -------------------------------------------------------------
def test_frame_loop_under_the_canonical_key(tmp_path):
    import torch
    from pointgnn_amd import kitti_dataset as KD, run as RUN, synthetic as S
    from pointgnn_amd import weights
    cfg = dict(configs.get_config("car_auto_T1"), box_encoding_method=CANONICAL)
    root = str(tmp_path / "kitti")
    for i, preset in enumerate(["small", "tiny"]):
        S.write_kitti_frames(root, [i], preset=preset, behind_points=4000)
    ds = KD.KittiDataset(*[os.path.join(root, d)
                           for d in ("image_2", "velodyne", "calib")])
    assert ds.num_files == 2
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    seq, pipe = str(tmp_path / "seq"), str(tmp_path / "pipe")
    RUN.run_dataset(ds, cfg, None, seq, params=params, pipelined=False)
    td = RUN.run_dataset(ds, cfg, None, pipe, params=params, in_flight=2,
                         prefetch=2)
    torch.cuda.synchronize()
    assert td['frames'] == 2
    sizes = []
    for i in range(2):
        name = ds.get_filename(i) + ".txt"
        with open(os.path.join(seq, "data", name), "rb") as f:
            want = f.read()
        with open(os.path.join(pipe, "data", name), "rb") as f:
            assert f.read() == want, i
        sizes.append(len(want))
    print("frame loop: file sizes %s, sequential fallbacks %d" % (
        sizes, td['sequential fallbacks']))
    assert max(sizes) > 1, "no detections at all"
    # the second frame went through the deferred decode, not the fallback
    assert td['sequential fallbacks'] == 0
    # the same frames under the plain key give other boxes
    other = str(tmp_path / "plain")
    RUN.run_dataset(ds, dict(cfg, box_encoding_method=PLAIN), None, other,
                    params=params, pipelined=False)
    differ = False
    for i in range(2):
        name = ds.get_filename(i) + ".txt"
        with open(os.path.join(seq, "data", name), "rb") as f, \
                open(os.path.join(other, "data", name), "rb") as g:
            differ = differ or f.read() != g.read()
    assert differ


# ---- 8. training ---------------------------------------------------------------
def test_training_targets_under_the_canonical_key(tmp_path):
    import torch
    from test_gpu_e2e import _velodyne_scan
    from test_ingest_cpu import _write_png_header_only
    from oracle import ingest_oracle as IO
    from oracle import labels_oracle as LO
    from pointgnn_amd import kitti_dataset as KD, train, weights
    cfg = dict(configs.get_config("car_auto_T1"), box_encoding_method=CANONICAL)
    for d in ("image_2", "velodyne", "calib", "label_2"):
        (tmp_path / d).mkdir()
    velo = _velodyne_scan(31)
    velo.tofile(str(tmp_path / "velodyne" / "000000.bin"))
    (tmp_path / "calib" / "000000.txt").write_text("".join(IO.CALIB_LINES))
    _write_png_header_only(str(tmp_path / "image_2" / "000000.png"), 375, 1242)
    cam, _, _ = IO.cam_points_in_image(velo, IO.get_calib(IO.CALIB_LINES),
                                       (375, 1242))
    LO.write_label_file(str(tmp_path / "label_2" / "000000.txt"),
                        LO.synthetic_labels(31, cam, n_boxes=10))
    ds = KD.KittiDataset(str(tmp_path / "image_2"), str(tmp_path / "velodyne"),
                         str(tmp_path / "calib"), str(tmp_path / "label_2"),
                         is_training=True, num_classes=cfg["num_classes"])
    tcfg = {'data_aug_configs': []}     # no augmentation: vertices stay float32
    np.random.seed(3)                   # the training-mode graph draws from it
    batch = train.fetch_data(ds, 0, cfg, tcfg)
    np.random.seed(3)
    plain = train.fetch_data(ds, 0, dict(cfg, box_encoding_method=PLAIN), tcfg)
    cls, enc = batch[4], batch[5]
    last = batch[1][-1]
    assert enc.is_cuda and enc.dtype == torch.float32
    assert torch.equal(cls, plain[4]) and torch.equal(last, plain[1][-1])
    # the float64 restatement on the same vertices / ground-truth boxes
    _, boxes3d, _, lm = ds.assign_classaware_car_label_to_points(
        ds.get_label(0), last, expend_factor=(1.0, 1.0, 1.0))
    assert boxes3d.dtype == torch.float64
    labels = cls.cpu().numpy()
    want, m = BC.canonical_encode_f64(labels, last.cpu().numpy(),
                                      boxes3d.cpu().numpy(), lm)
    active = BC.active_rows(labels, lm)
    assert active.sum() > 10
    BC.check_f64(enc.cpu().numpy(), want.astype(np.float32), m, active)
    # other targets than the plain key's where a label is active, the same
    # elsewhere
    e, p = enc.cpu().numpy(), plain[5].cpu().numpy()
    assert np.array_equal(e[~active], p[~active])
    turned = active & (np.abs(want[:, 0, 6]) > 1e-3)
    assert turned.sum() > 10
    assert np.all((e[turned, 0, 0] != p[turned, 0, 0]) |
                  (e[turned, 0, 2] != p[turned, 0, 2]))
    assert np.array_equal(e[active][:, 0, [1, 3, 4, 5, 6]],
                          p[active][:, 0, [1, 3, 4, 5, 6]])
    tr = train.Trainer(cfg, params=weights.init_params(cfg, seed=1),
                       device=last.device)
    out = tr.train_step(batch, apply=False)
    assert np.isfinite([out['cls_loss'], out['loc_loss']]).all()
    assert out['loc_loss'] > 0
    # eval.py's pass reaches the codec through the same fetch_data
    from pointgnn_amd import eval as EV
    ev = EV.eval_once(ds, cfg, {'data_aug_configs': [], 'NUM_TEST_SAMPLE': -1},
                      params=weights.init_params(cfg, seed=1))
    assert np.isfinite([ev['cls_loss'], ev['loc_loss']]).all()
    assert ev['loc_loss'] > 0
