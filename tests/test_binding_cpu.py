"""The ctypes binding is derived from include/pointgnn_hip.h by
pointgnn_amd/_header.py: the reader on a synthetic header, the derived struct
layouts against the C compiler's, and the Python names of the header's
numbers.  No GPU and no shared library needed."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int32, c_int64,
                    c_size_t, c_uint32, c_uint64, c_void_p)

import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pointgnn_hip.h")

# every construct the reader knows, once
_DEMO = """\
/* a comment that holds a prototype: int pgnn_not_this(int x); */
#ifndef DEMO_H_
#define DEMO_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PGNN_NEG (-3)   // a negative number
#define PGNN_BIG (1 << 24)
#define PGNN_N 4
#define PGNN_SUM (PGNN_N * 2 + 1 - 3)
typedef struct pgnn_inner {
  int64_t a, b; /* two declarators */
  const float *p;
} pgnn_inner;
typedef struct pgnn_outer {
  int32_t n;
  pgnn_inner one;
  pgnn_inner many[PGNN_N];
  float grid[PGNN_N + 1][3];
  void *ptrs[2];
} pgnn_outer;
int pgnn_none(void);
const char *pgnn_name(const char *key, int value);
size_t pgnn_scalars(int32_t a, int64_t b, uint32_t c, uint64_t d, size_t e,
                    double f, float g);
int pgnn_ptrs(const pgnn_outer *o, pgnn_inner *i, void **out,
              const float **pp, float *const *acts, int32_t *count /* [2] */,
              char *buf, void *stream);
#ifdef __cplusplus
}
#endif
#endif /* DEMO_H_ */
"""


def test_reader_on_a_synthetic_header():
    fns, structs, consts = _header.parse(_DEMO)
    assert consts == {"PGNN_NEG": -3, "PGNN_BIG": 1 << 24, "PGNN_N": 4,
                      "PGNN_SUM": 6}
    assert list(structs) == ["pgnn_inner", "pgnn_outer"]
    inner, outer = structs["pgnn_inner"], structs["pgnn_outer"]
    assert issubclass(inner, ctypes.Structure)
    assert inner._fields_ == [("a", c_int64), ("b", c_int64), ("p", c_void_p)]
    assert outer._fields_ == [("n", c_int32), ("one", inner),
                              ("many", inner * 4), ("grid", (c_float * 3) * 5),
                              ("ptrs", c_void_p * 2)]
    assert ctypes.sizeof(outer) == 8 + 24 + 4 * 24 + 60 + 4 + 16
    assert fns == {
        "pgnn_none": (c_int32, []),
        "pgnn_name": (c_char_p, [c_char_p, c_int32]),
        "pgnn_scalars": (c_size_t, [c_int32, c_int64, c_uint32, c_uint64,
                                    c_size_t, c_double, c_float]),
        "pgnn_ptrs": (c_int32, [POINTER(outer), POINTER(inner),
                                POINTER(c_void_p), c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    }


@pytest.mark.parametrize("line, names", [
    ("int pgnn_bad(int32_t n, unsigned flags);", ["pgnn_bad", "unsigned flags"]),
    ("int pgnn_bad(int32_t n, int16_t small);", ["pgnn_bad", "int16_t small"]),
    ("int pgnn_bad(int32_t);", ["pgnn_bad", "int32_t"]),
    ("int pgnn_bad(pgnn_inner by_value);", ["pgnn_bad", "by_value"]),
    ("int pgnn_bad(const float xyz[3]);", ["pgnn_bad", "xyz[3]"]),
    ("void pgnn_bad(int32_t n);", ["pgnn_bad", "void"]),
    ("int pgnn_bad(int (*callback)(int));", ["callback"]),
    ("int other_entry(void);", ["other_entry"]),
    ("int pgnn_none(void);", ["pgnn_none", "twice"]),
    ("typedef struct pgnn_s { char tag; } pgnn_s;", ["pgnn_s", "char tag"]),
    ("typedef struct pgnn_s { int32_t n : 3; } pgnn_s;", ["pgnn_s", "n : 3"]),
    ("typedef struct pgnn_s { float v[PGNN_MISSING]; } pgnn_s;",
     ["pgnn_s", "PGNN_MISSING"]),
    ("typedef struct pgnn_s { int32_t n; } pgnn_t;", ["pgnn_s", "pgnn_t"]),
    ("#define PGNN_HALF 0.5", ["PGNN_HALF"]),
    ("#define PGNN_DIV (8 / 2)", ["PGNN_DIV"]),
    ("#define PGNN_SQUARE(x) ((x) * (x))", ["PGNN_SQUARE"]),
    ("#if 0", ["#if 0"]),
])
def test_reader_refuses_what_it_does_not_know(line, names):
    text = _DEMO.replace("int pgnn_none(void);", "int pgnn_none(void);\n" + line)
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(text)
    for name in names:
        assert name in str(e.value), str(e.value)


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof and every offsetof of every struct of the header, as gcc lays
    them out, against the ctypes classes the reader builds."""
    structs = _header.structs()
    assert len(structs) >= 9
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found (oracle/graph_oracle.py needs it as well)"
    src = ['#include <stdio.h>', '#include "pointgnn_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        src.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            src.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));'
                       % (name, field, name, field))
    src += ['  return 0;', '}', '']
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.dirname(HEADER), "-o", exe,
                           str(tmp_path / "layout.c")])
    compiled = dict(line.split() for line in subprocess.check_output(
        [exe]).decode().splitlines())
    derived = {}
    for name, cls in structs.items():
        derived[name] = str(ctypes.sizeof(cls))
        for field, _ in cls._fields_:
            derived[name + "." + field] = str(getattr(cls, field).offset)
    assert derived == compiled
    assert compiled["pgnn_train_model"] == "6032"
    assert compiled["pgnn_train_model.loc_split"] == "6024"


def test_reader_covers_the_header():
    """Every pgnn_* name a cruder parse finds is a bound prototype, and the
    aliases of _lib.py are the reader's classes."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pgnn_[a-z0-9_]+)\s*\(", text))
    assert len(declared) >= 176
    assert declared == set(_header.functions())
    from pointgnn_amd import _lib
    assert set(_lib.exported_symbols()) == declared
    s = _header.structs()
    for alias, name in [("FcLayer", "pgnn_fc_layer"),
                        ("DynCount", "pgnn_dyn_count"),
                        ("WgradJob", "pgnn_wgrad_job"),
                        ("MergeJob", "pgnn_merge_job"),
                        ("FrameArrays", "pgnn_frame_arrays"),
                        ("TrainFc", "pgnn_train_fc"),
                        ("TrainStage", "pgnn_train_stage"),
                        ("TrainModel", "pgnn_train_model"),
                        ("TrainBatch", "pgnn_train_batch")]:
        assert getattr(_lib, alias) is s[name]
    assert _header.functions()["pgnn_mlp_fwd_dyn"][1][7] is POINTER(_lib.FcLayer)


def test_python_names_equal_the_headers_defines():
    """The numbers Python code uses are the header's, read here with a plain
    regex (not with the reader that binds them)."""
    from pointgnn_amd import _lib, comm, kitti_eval, render
    text = open(HEADER).read()
    defines = {k: int(v) for k, v in re.findall(
        r"^#define\s+(PGNN_\w+)\s+\(?(-?\d+)\)?[ \t]*(?:/\*|$)", text,
        flags=re.M)}
    assert _header.constants()["PGNN_KITTI_MAX_FRAMES"] == 1 << 24
    expect = {
        _lib: dict(PGNN_MAX_LAYERS="PGNN_MAX_LAYERS",
                   MERGE_MAX_LEVELS="PGNN_MERGE_MAX_LEVELS",
                   TRAIN_MAX_FC="PGNN_TRAIN_MAX_FC",
                   TRAIN_MAX_STAGES="PGNN_TRAIN_MAX_STAGES",
                   TRAIN_MAX_CLASSES="PGNN_TRAIN_MAX_CLASSES",
                   TRAIN_MAX_LEVELS="PGNN_TRAIN_MAX_LEVELS",
                   E_INVALID="PGNN_E_INVALID", E_WORKSPACE="PGNN_E_WORKSPACE",
                   E_UNSUPPORTED="PGNN_E_UNSUPPORTED", AGG_MAX="PGNN_AGG_MAX",
                   AGG_SUM="PGNN_AGG_SUM", AGG_MEAN="PGNN_AGG_MEAN",
                   SCHED_WS_INTS="PGNN_SCHED_WS_INTS"),
        kitti_eval: dict(ROW="PGNN_KITTI_ROW",
                         N_SAMPLE_PTS="PGNN_KITTI_SAMPLE_PTS",
                         N_COMBOS="PGNN_KITTI_COMBOS",
                         MAX_DET="PGNN_KITTI_MAX_DET",
                         MAX_GT="PGNN_KITTI_MAX_GT"),
        render: dict(MAX_DIM="PGNN_RENDER_MAX_DIM"),
        comm: dict(ID_BYTES="PGNN_COMM_ID_BYTES"),
    }
    for module, names in expect.items():
        for py, c in names.items():
            assert getattr(module, py) == defines[c], (module.__name__, py, c)
    assert (_lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED) == (-1, -2, -3)
