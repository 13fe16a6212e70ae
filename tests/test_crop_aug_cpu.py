"""crop_aug without a GPU: the committed fixtures still are what the
reference's models/crop_aug.py produces (where its checkout is present: the
generator's database and one case are run again and compared), and the new
entry point is declared, exported and validates its arguments before any HIP
call."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_crop_aug", os.path.join(GOLD, "make_golden_crop_aug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_files_are_small_and_complete():
    import test_gpu_crop_aug as T
    for path in (T.FIXTURE, T.DB_FILE):
        assert 0 < os.path.getsize(path) <= 1 << 20
    with np.load(T.FIXTURE) as f:
        keys = set(f.files)
        for name in T.CASES:
            for field in ("k_points", "xyz", "attr", "names", "labels",
                          "rng_after", "accepted", "trials", "y3d_adjust"):
                assert name + "_" + field in keys
            assert len(f[name + "_xyz"]) == len(f[name + "_attr"])
            assert len(f[name + "_names"]) == len(f[name + "_labels"])
    with open(T.DB_FILE) as f:
        labels, points = json.load(f)
    assert set(labels) == set(points) == {"Car", "Pedestrian", "Cyclist"}


def test_fixture_is_what_the_reference_produces(tmp_path):
    gen = _generator()
    if not os.path.isdir(os.path.join(gen.REF, "models")):
        pytest.skip("the reference checkout is not on this machine")
    import test_gpu_crop_aug as T
    ca, kd = gen.load_reference()
    path = str(tmp_path / "db.json")
    gen.write_database(ca, kd, path)
    with open(path) as f, open(T.DB_FILE) as g:
        assert json.load(f) == json.load(g)
    sampler = ca.CropAugSampler(T.DB_FILE)
    name = "ground_required"
    case = T.CASES[name]
    res = gen.run_reference_case(ca, kd, sampler, name, case, case["seed"],
                                 case["k"])
    with np.load(T.FIXTURE) as f:
        for key, value in res.items():
            assert np.array_equal(f[key], value), key


def test_entry_point_is_declared_exported_and_validates():
    from pointgnn_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "pointgnn_hip.h")).read()
    assert re.search(r"\bint pgnn_crop_aug_place\(", header)
    assert "pgnn_crop_aug_place" in L.exported_symbols()
    lib = L.load()
    expand = (np.ones(3)).ctypes.data

    def call(n_base=0, n_samples=0, m=0, n_labels=0, max_trails=1, mode=0,
             expand=expand, record=1):
        # `record` non-null: validation ends before anything is launched
        return lib.pgnn_crop_aug_place(
            None, n_base, None, None, n_samples, m, None, None, n_labels,
            None, max_trails, mode, 0, 0, 0.01, 100.0, 1.0, expand, None,
            None, None, None, record, None)
    assert call(n_base=-1) == L.E_INVALID
    assert b"crop_aug_place" in lib.pgnn_last_error()
    assert call(mode=3) == L.E_INVALID
    assert call(expand=None) == L.E_INVALID
    assert call(record=None) == L.E_INVALID
    assert call(n_samples=7, n_labels=250) == L.E_UNSUPPORTED
    assert b"256" in lib.pgnn_last_error()
    assert call(n_base=1 << 30) == L.E_UNSUPPORTED
    # within the limits, but the buffers are missing
    assert call(n_samples=6, n_labels=250) == L.E_INVALID
    assert b"null pointer" in lib.pgnn_last_error()
    assert call(n_base=5) == L.E_INVALID
