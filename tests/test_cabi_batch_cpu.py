"""CPU-side checks of the batched points-to-boxes entries (qv2x_voxelize_batch_f32, qv2x_postprocess_batch_f32): declared, exported, and
their argument checks answer on the host without touching a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["qv2x_voxelize_batch_workspace_bytes", "qv2x_voxelize_batch_f32", "qv2x_postprocess_batch_workspace_bytes", "qv2x_postprocess_batch_f32"]


def _lib():
    from quantv2x_amd import build, lib
    build.build()
    return lib.load()


def _desc():
    from quantv2x_amd import lib
    d = lib.PostprocessDesc()
    d.h, d.w, d.anchors_per_cell, d.num_classes, d.max_boxes, d.score_threshold = 48, 88, 2, 1, 64, 0.2
    d.max_extent, d.z_min, d.z_max = 6.0, -3.0, 1.0
    return d


def test_header_and_binding_declare_the_batch_entries():
    from quantv2x_amd import lib
    header = open(os.path.join(ROOT, "include", "qv2x.h")).read()
    declared = set(re.findall(r"\b(qv2x_[a-z0-9_]+)\s*\(", header))
    l = _lib()
    for n in NAMES:
        assert n in declared and n in lib.SYMBOLS and hasattr(l, n), n
    assert l.qv2x_version() == 9 == lib.ABI_VERSION


def test_voxelize_batch_workspace_rejects_bad_sweep_lists():
    l = _lib()
    ok = (C.c_int32 * 65)(*([1000] * 65))
    assert l.qv2x_voxelize_batch_workspace_bytes(0, ok) == -1 and b"sweeps" in l.qv2x_last_error()
    assert l.qv2x_voxelize_batch_workspace_bytes(65, ok) == -1 and b"sweeps" in l.qv2x_last_error()
    assert l.qv2x_voxelize_batch_workspace_bytes(2, None) == -1
    big = (C.c_int32 * 2)(1000, 1 << 20)
    assert l.qv2x_voxelize_batch_workspace_bytes(2, big) == -1 and b"2^20" in l.qv2x_last_error()
    neg = (C.c_int32 * 2)(1000, -1)
    assert l.qv2x_voxelize_batch_workspace_bytes(2, neg) == -1
    # valid lists: 64 sweeps, the largest sweep the key holds, empty sweeps; the workspace grows with the points
    edge = (C.c_int32 * 3)(0, (1 << 20) - 1, 0)
    assert l.qv2x_voxelize_batch_workspace_bytes(3, edge) > 20 * ((1 << 20) - 1)
    assert l.qv2x_voxelize_batch_workspace_bytes(64, ok) > l.qv2x_voxelize_batch_workspace_bytes(32, ok) > 0
    none = (C.c_int32 * 2)(0, 0)
    assert l.qv2x_voxelize_batch_workspace_bytes(2, none) > 0


def test_voxelize_batch_refuses_on_the_host():
    """bad arguments are answered before any launch (no GPU here)"""
    import numpy as np
    from quantv2x_amd import lib
    l = _lib()
    buf = np.zeros(4096, np.uint8)
    p = lib.ptr(buf)
    rng, vs = (C.c_float * 6)(-12.8, -6.4, -3.0, 12.8, 6.4, 1.0), (C.c_float * 3)(0.4, 0.4, 4.0)
    n = (C.c_int32 * 1)(10)
    tab = (C.c_void_p * 1)(buf.ctypes.data)
    assert l.qv2x_voxelize_batch_f32(tab, n, 0, rng, vs, 0, 32, 16, p, 1 << 20, p, p, p, p, None) == -1
    assert l.qv2x_voxelize_batch_f32(tab, n, 1, rng, vs, 0, 32, 16, p, 16, p, p, p, p, None) == -1 and b"workspace" in l.qv2x_last_error()
    assert l.qv2x_voxelize_batch_f32(tab, n, 1, rng, vs, 0, 0, 16, p, 1 << 20, p, p, p, p, None) == -1
    # a grid whose cells need 40 bits: 7 sweep bits + 40 + 20 index bits do not fit the 64-bit key
    huge = (C.c_float * 6)(0.0, 0.0, 0.0, 1048576.0, 1048576.0, 1.0)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    n64 = (C.c_int32 * 64)(*([1] * 64))
    tab64 = (C.c_void_p * 64)(*([buf.ctypes.data] * 64))
    assert l.qv2x_voxelize_batch_f32(tab64, n64, 64, huge, one, 0, 32, 16, p, 1 << 20, p, p, p, p, None) == -1 and b"64-bit key" in l.qv2x_last_error()


def test_postprocess_batch_workspace_bytes():
    l = _lib()
    d = _desc()
    assert l.qv2x_postprocess_batch_workspace_bytes(C.byref(d), 0) == -1 and b"frames" in l.qv2x_last_error()
    assert l.qv2x_postprocess_batch_workspace_bytes(C.byref(d), 65) == -1 and b"frames" in l.qv2x_last_error()
    single = l.qv2x_postprocess_workspace_bytes(C.byref(d))
    one = l.qv2x_postprocess_batch_workspace_bytes(C.byref(d), 1)
    assert single > 0 and one >= single
    assert l.qv2x_postprocess_batch_workspace_bytes(C.byref(d), 64) >= 64 * single
    bad = _desc()
    bad.max_boxes = 5000
    assert l.qv2x_postprocess_batch_workspace_bytes(C.byref(bad), 4) == -1 and b"max_boxes" in l.qv2x_last_error()
    bad = _desc()
    bad.num_classes = 0
    assert l.qv2x_postprocess_batch_workspace_bytes(C.byref(bad), 4) == -1
    assert l.qv2x_postprocess_batch_workspace_bytes(None, 4) == -1


def test_postprocess_batch_refuses_on_the_host():
    import numpy as np
    from quantv2x_amd import lib
    l = _lib()
    d = _desc()
    buf = np.zeros(4096, np.uint8)
    p = lib.ptr(buf)
    need = l.qv2x_postprocess_batch_workspace_bytes(C.byref(d), 2)
    assert l.qv2x_postprocess_batch_f32(C.byref(d), 2, p, 0, p, 0, None, 0, p, p, p, 16, p, p, None, p, None) == -1 and b"workspace" in l.qv2x_last_error()
    assert l.qv2x_postprocess_batch_f32(C.byref(d), 2, p, 0, p, 0, None, 0, p, None, p, need, p, p, None, p, None) == -1 and b"null" in l.qv2x_last_error()
    assert l.qv2x_postprocess_batch_f32(C.byref(d), 2, p, -1, p, 0, None, 0, p, p, p, need, p, p, None, p, None) == -1 and b"stride" in l.qv2x_last_error()
    d.num_bins = 2
    assert l.qv2x_postprocess_batch_f32(C.byref(d), 2, p, 0, p, 0, None, 0, p, p, p, need, p, p, None, p, None) == -1 and b"direction" in l.qv2x_last_error()
