"""ctypes binding of libpointgnn_hip.so (include/pointgnn_hip.h).

The product path has no CPU fallback: if the shared library is missing or a
call fails, this module raises.  torch is imported first so that the library's
`libamdhip64.so.7` dependency resolves to the HIP runtime PyTorch already
loaded (one runtime per process: torch's streams and allocations are then
valid inside the library).
"""
import ctypes
import os

import torch  # noqa: F401  (must precede CDLL, see module docstring)

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGNN_LIB selects another build of the same library (kernel A/B runs in tools/)
LIB_PATH = os.environ.get("PGNN_LIB") or os.path.join(_HERE, "libpointgnn_hip.so")

c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

# Signatures, structs and numbers all come from the header (_header.py reads it
# when this module is imported): to add or change an entry, edit the header.
_S, _C = _header.structs(), _header.constants()

FcLayer = _S["pgnn_fc_layer"]
# a size that lives in device memory (`dev`, an int32) plus the value the host
# expects (`hint`)
DynCount = _S["pgnn_dyn_count"]
WgradJob = _S["pgnn_wgrad_job"]          # pgnn_weight_grad_many_f32
MergeJob = _S["pgnn_merge_job"]          # pgnn_merge_rows
FrameArrays = _S["pgnn_frame_arrays"]    # pgnn_merge_frames_dyn
TrainFc = _S["pgnn_train_fc"]
TrainStage = _S["pgnn_train_stage"]
TrainModel = _S["pgnn_train_model"]
TrainBatch = _S["pgnn_train_batch"]


class PackJob(ctypes.Structure):
    """One record of pgnn_pack_fc_many's job table.  Hand-written because the
    header has no struct for it: the table is device memory behind a
    `const void *`, laid out by csrc (it never crosses the ABI as a type)."""
    _fields_ = [("w", c_vp), ("b", c_vp), ("dst", c_vp), ("k_in", c_i32),
                ("n_out", c_i32), ("kind", c_i32), ("first_block", c_i32),
                ("ld", c_i32), ("reserved", c_i32)]


PGNN_MAX_LAYERS = _C["PGNN_MAX_LAYERS"]
MERGE_MAX_LEVELS = _C["PGNN_MERGE_MAX_LEVELS"]
TRAIN_MAX_FC = _C["PGNN_TRAIN_MAX_FC"]
TRAIN_MAX_STAGES = _C["PGNN_TRAIN_MAX_STAGES"]
TRAIN_MAX_CLASSES = _C["PGNN_TRAIN_MAX_CLASSES"]
TRAIN_MAX_LEVELS = _C["PGNN_TRAIN_MAX_LEVELS"]
E_INVALID = _C["PGNN_E_INVALID"]
E_WORKSPACE = _C["PGNN_E_WORKSPACE"]
E_UNSUPPORTED = _C["PGNN_E_UNSUPPORTED"]
# `aggregation` of the pgnn_*_agg_* entries
AGG_MAX, AGG_SUM, AGG_MEAN = (_C["PGNN_AGG_MAX"], _C["PGNN_AGG_SUM"],
                              _C["PGNN_AGG_MEAN"])
SCHED_WS_INTS = _C["PGNN_SCHED_WS_INTS"]
# `edges_sorted` of pgnn_edge_mlp_scatter_max_scaled_fwd
EDGE_K300_ORDER = _C["PGNN_EDGE_K300_ORDER"]


class PointGnnHipError(RuntimeError):
    pass


_lib = None


def exported_symbols():
    """Names every entry point include/pointgnn_hip.h declares."""
    return sorted(_header.functions())


def _build_missing():
    """A source checkout without the built library (the .so is git-ignored):
    compile it once with hipcc if there is one.  Ranks of one node serialise
    on a lock file so that `torch.distributed.run` does not start N builds."""
    import fcntl
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        return
    lock = os.path.join(os.path.dirname(LIB_PATH), ".build.lock")
    with open(lock, "w") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        try:
            if not os.path.exists(LIB_PATH):
                from . import build as _build
                _build.build(verbose=False)
        finally:
            fcntl.flock(f, fcntl.LOCK_UN)


def load():
    """Load (once) and return the ctypes library.  Raises when it is missing:
    build it with `python -m pointgnn_amd.build` (or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and not os.environ.get("PGNN_LIB"):
        _build_missing()
    if not os.path.exists(LIB_PATH):
        raise PointGnnHipError(
            "libpointgnn_hip.so not found at %s -- the HIP extension is "
            "required (no CPU fallback); run `python -m pointgnn_amd.build`"
            % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _header.functions().items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks the symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # PGNN_TUNE="key=value,key=value": tunables applied when the library is
    # loaded (pgnn_set_tunable) -- runs a whole test session under, e.g., the
    # frame pipeline's capped builder grids
    for kv in filter(None, os.environ.get("PGNN_TUNE", "").split(",")):
        k, v = kv.split("=")
        check(lib.pgnn_set_tunable(k.strip().encode(), int(v)),
              "PGNN_TUNE " + kv)
    return lib


def check(rc, what=""):
    """Raise on a non-zero return code of a pgnn_* call."""
    if rc != 0:
        msg = load().pgnn_last_error()
        raise PointGnnHipError("%s failed (code %d): %s" % (
            what or "pgnn call", rc, msg.decode() if msg else "?"))


_SCHED_WS = {}


def sched_ws(device=None):
    """The zeroed int32 counters of the fused kernels' tile pools (sched_ws of
    pgnn_point_set_pooling_fwd / pgnn_edge_mlp_scatter_max_fwd;
    PGNN_SCHED_WS_INTS of them): one set per (device, current stream) --
    launches of one stream are serialised and the kernels hand the counters
    back zeroed."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) \
        if device is None or device.index is None else device
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    t = _SCHED_WS.get(key)
    if t is None:
        t = _SCHED_WS[key] = torch.zeros(SCHED_WS_INTS, dtype=torch.int32,
                                         device=dev)
    return t


def stream_ptr():
    """hipStream_t of torch's current stream as void* (0 = null stream)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


class DeviceCount(object):
    """A size that exists only in device memory (capacity form, struct
    pgnn_dyn_count): `dev` is a 1-element int32 CUDA tensor, `hint` the value
    the host expects (it chooses between kernels with identical results and
    sizes strided grids, nothing else), `frame` the FrameCounts record it
    belongs to.  Tensors whose leading dimension is a capacity carry one as
    `t._pgnn_count` (tag_count / count_of)."""
    __slots__ = ("dev", "hint", "frame")

    def __init__(self, dev, hint=0, frame=None):
        self.dev = dev
        self.hint = int(hint)
        self.frame = frame

    def arg(self):
        """ctypes pgnn_dyn_count* for a *_dyn entry (valid during the call)."""
        return ctypes.byref(DynCount(self.dev.data_ptr(), self.hint))


def tag_count(t, count):
    """Mark tensor `t` as capacity-form: only the first `count` rows exist."""
    if count is not None:
        t._pgnn_count = count
    return t


def count_of(t):
    return getattr(t, "_pgnn_count", None) if t is not None else None


def kernel_occupancy(kernel, lds_bytes=-1):
    """pgnn_kernel_occupancy -> dict(vgprs, scratch_bytes, workgroups_per_cu,
    lds_bytes); lds_bytes < 0: that of the kernel's last launch."""
    v, sc, wg = c_i32(0), c_i32(0), c_i32(0)
    used = c_i64(0)
    check(load().pgnn_kernel_occupancy(
        kernel.encode(), int(lds_bytes), ctypes.byref(v), ctypes.byref(sc),
        ctypes.byref(wg), ctypes.byref(used)), "pgnn_kernel_occupancy")
    return {"vgprs": v.value, "scratch_bytes": sc.value,
            "workgroups_per_cu": wg.value, "lds_bytes": used.value}


def set_tunable(key, value):
    check(load().pgnn_set_tunable(key.encode(), int(value)), "pgnn_set_tunable")
