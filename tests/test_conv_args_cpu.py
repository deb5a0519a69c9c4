"""CPU-side pins of the int8 convolution family's host layer, next to tests/test_conv_layers_cpu.py (which holds the rejects of
``qv2x_conv3x3_i8``, ``_wide``, ``_pack_wide`` and ``_chain64``): every reject of ``qv2x_conv3x3_i8_res``, ``qv2x_conv1x1_i8``,
``qv2x_gconv3x3_i8`` and ``qv2x_bottleneck_i8`` -- code, wording, the entry's name, one null and one misaligned case per pointer -- and a
truth table of ``qv2x_conv3x3_i8_wide_ok``.  Rejected calls only, on host addresses: nothing launches, no pointer is dereferenced."""
import ctypes as C

import numpy as np
import pytest

from test_conv_layers_cpu import REGULAR_REJECTS, TWO_GROUPS, _good

vp = C.c_void_p


@pytest.fixture(scope="module")
def l():
    from quantv2x_amd import build, lib
    build.build()
    return lib.load()


_RAW = np.zeros(4096 + 16, np.uint8)


@pytest.fixture(scope="module")
def base():
    return _RAW.ctypes.data + (-_RAW.ctypes.data) % 16               # a 16-byte aligned host address: no kernel ever sees it


def _set(d, change):
    for k, v in change.items():
        setattr(d, k, v)
    return d


# ---- qv2x_conv3x3_i8_res -------------------------------------------------------------------------------------------------------------------

def test_conv3x3_res_rejects(l, base):
    """the wrapper's own reject, every reject of conv3x3_entry in front of the shortcut rule (they name qv2x_conv3x3_i8: the shared entry),
    then the shortcut rule itself"""
    err, p = l.qv2x_last_error, vp(base)

    def res(d, ptrs=None, res_mode=3, shortcut=p):
        q = ptrs or [p] * 7
        return l.qv2x_conv3x3_i8_res(C.byref(d) if d is not None else None, *q[:6], res_mode, shortcut, 128, 0.1, q[6], None)

    good = lambda **change: _good(**{"cout": 64, **change})
    for mode in (0, 1, 4, -2):
        assert res(good(), res_mode=mode) == -1 and b"qv2x_conv3x3_i8_res: res_mode 2 (fp32 shortcut) or 3 (shortcut codes)" in err(), mode
    in_front = [r for r in REGULAR_REJECTS if b"multi-group input needs" not in r[2]]      # (that reject sits behind the shortcut rule)
    assert len(in_front) == len(REGULAR_REJECTS) - 2
    for change, rc, msg in in_front:
        for mode in (2, 3):
            assert res(_good(**change), res_mode=mode) == rc, change
            assert msg in err() and b"qv2x_conv3x3_i8:" in err(), (change, err())
    rule = b"qv2x_conv3x3_i8_res: one input group of 64 channels, cout 64, res_mode 2 | 3, aligned shortcut"
    for change in (TWO_GROUPS, dict(cout=128), dict(cout=256), dict(cin_total=256, group_c0=[0], group_c=[128])):
        assert res(good(**change)) == -1 and rule in err(), (change, err())
    for mode in (2, 3):
        assert res(good(), res_mode=mode, shortcut=vp(None)) == -1 and rule in err()
        assert res(good(), res_mode=mode, shortcut=vp(base + 4)) == -1 and rule in err()
    for hole in range(7):
        ptrs = [p] * 7
        ptrs[hole] = vp(None)
        assert res(good(), ptrs) == -1 and b"qv2x_conv3x3_i8: null pointer" in err(), hole
    assert res(None) == -1 and b"qv2x_conv3x3_i8: null pointer" in err()
    for hole in (0, 1, 6):                                           # in, w, out
        ptrs = [p] * 7
        ptrs[hole] = vp(base + 4)
        assert res(good(), ptrs) == -2 and b"qv2x_conv3x3_i8: in / w / out must be 16-byte aligned" in err(), hole


# ---- qv2x_conv1x1_i8 -----------------------------------------------------------------------------------------------------------------------

def _c1(**change):
    from quantv2x_amd import lib
    d = lib.Conv1x1Desc()
    d.n, d.h, d.w, d.cin, d.cout, d.stride, d.mode, d.relu = 1, 5, 32, 64, 128, 1, 0, 1
    d.out_ctotal, d.out_c0, d.out_delta, d.out_zp, d.res_zx, d.res_delta = 160, 16, 0.05, 7.0, 120, 0.1
    return _set(d, change)


C1_REJECTS = [
    (dict(n=0), -1, b"bad shape / stride"), (dict(h=0), -1, b"bad shape / stride"), (dict(w=-1), -1, b"bad shape / stride"),
    (dict(stride=0), -1, b"bad shape / stride"), (dict(stride=3), -1, b"bad shape / stride"),
    (dict(cin=96), -2, b"cin 64 | 128 | 256 | 512, cout % 64"), (dict(cin=32), -2, b"cin 64 | 128"), (dict(cin=1024), -2, b"cin 64 | 128"),
    (dict(cout=96, out_ctotal=112), -2, b"cout % 64"),
    (dict(mode=-1), -1, b"mode 0..3"), (dict(mode=4), -1, b"mode 0..3"),
    (dict(out_delta=0.0), -1, b"out_delta must be positive"), (dict(out_delta=-1.0, mode=2), -1, b"out_delta must be positive"),
    (dict(out_ctotal=168), -2, b"out channel window (% 16)"), (dict(out_c0=8), -2, b"out channel window (% 16)"),
    (dict(out_ctotal=128), -2, b"out channel window (% 16)"),        # [16, 144) ends past 128 channels
    (dict(out_c0=48, mode=3), -2, b"out channel window (% 16)"),
]


def test_conv1x1_rejects(l, base):
    err, p = l.qv2x_last_error, vp(base)

    def c1(d, ptrs=None):                                            # in, w_frag, scale, corr, aw, bias, res, out
        return l.qv2x_conv1x1_i8(C.byref(d) if d is not None else None, *(ptrs or [p] * 8), None)

    for change, rc, msg in C1_REJECTS:
        assert c1(_c1(**change)) == rc, change
        assert msg in err() and b"qv2x_conv1x1_i8:" in err(), (change, err())
    for mode in (2, 3):
        ptrs = [p] * 8
        ptrs[6] = vp(None)
        assert c1(_c1(mode=mode), ptrs) == -1 and b"qv2x_conv1x1_i8: mode %d needs the shortcut" % mode in err()
    for mode in (0, 2):
        for hole in range(8):
            ptrs = [p] * 8
            ptrs[hole] = vp(base + 4)
            assert c1(_c1(mode=mode), ptrs) == -2 and b"qv2x_conv1x1_i8: 16-byte aligned pointers" in err(), (mode, hole)
            if hole != 6:                                            # (a missing shortcut is no fault in modes 0 and 1; above for 2 and 3)
                ptrs[hole] = vp(None)
                assert c1(_c1(mode=mode), ptrs) == -1 and b"qv2x_conv1x1_i8: null pointer" in err(), (mode, hole)
    assert c1(None) == -1 and b"qv2x_conv1x1_i8: null pointer" in err()
    # the order of the checks: shape before channels before mode before the shortcut before alignment before the quantizer before the window
    # (fault k and every later one present: fault k is the one reported)
    faults = [dict(n=0), dict(cin=96), dict(mode=4), dict(res=None), dict(inp=base + 4), dict(out_delta=0.0), dict(out_c0=8)]
    words = [b"bad shape", b"cin 64", b"mode 0..3", b"needs the shortcut", b"aligned pointers", b"out_delta", b"out channel window"]
    for first in range(len(faults)):
        change = {"mode": 2}
        for f in faults[first:]:
            change.update(f)
        ptrs = [p] * 8
        if "res" in change:
            ptrs[6] = vp(change.pop("res"))
        if "inp" in change:
            ptrs[0] = vp(change.pop("inp"))
        c1(_c1(**change), ptrs)
        assert words[first] in err(), (first, err())


# ---- qv2x_gconv3x3_i8 ----------------------------------------------------------------------------------------------------------------------

def _gc(**change):
    from quantv2x_amd import lib
    d = lib.GconvDesc()
    d.n, d.h, d.w, d.c, d.cg, d.stride, d.relu, d.out_delta, d.out_zp = 1, 5, 33, 160, 8, 2, 1, 0.05, 7.0
    return _set(d, change)


GC_REJECTS = [
    (dict(n=0), -1, b"bad shape / stride"), (dict(h=-2), -1, b"bad shape / stride"), (dict(w=0), -1, b"bad shape / stride"),
    (dict(stride=0), -1, b"bad shape / stride"), (dict(stride=4), -1, b"bad shape / stride"),
    (dict(c=144), -2, b"channels % 32, 4 | 8 | 16 channels per group"), (dict(cg=2), -2, b"4 | 8 | 16 channels per group"),
    (dict(cg=32), -2, b"4 | 8 | 16 channels per group"), (dict(cg=12), -2, b"4 | 8 | 16 channels per group"),
    (dict(out_delta=0.0), -1, b"out_delta must be positive"), (dict(out_delta=float("nan")), -1, b"out_delta must be positive"),
]


def test_gconv3x3_rejects(l, base):
    err, p = l.qv2x_last_error, vp(base)

    def gc(d, ptrs=None):                                            # in, w_frag, scale, corr, aw, bias, out
        return l.qv2x_gconv3x3_i8(C.byref(d) if d is not None else None, *(ptrs or [p] * 7), None)

    for change, rc, msg in GC_REJECTS:
        assert gc(_gc(**change)) == rc, change
        assert msg in err() and b"qv2x_gconv3x3_i8:" in err(), (change, err())
    for hole in range(7):
        ptrs = [p] * 7
        ptrs[hole] = vp(base + 8)
        assert gc(_gc(), ptrs) == -2 and b"qv2x_gconv3x3_i8: 16-byte aligned pointers" in err(), hole
        assert gc(_gc(out_delta=0.0), ptrs) == -2 and b"aligned pointers" in err(), hole       # alignment is tested before the quantizer
        assert gc(_gc(c=144), ptrs) == -2 and b"channels % 32" in err(), hole                 # ... and after the channels
        ptrs[hole] = vp(None)
        assert gc(_gc(n=0), ptrs) == -1 and b"qv2x_gconv3x3_i8: null pointer" in err(), hole
    assert gc(None) == -1 and b"qv2x_gconv3x3_i8: null pointer" in err()


# ---- qv2x_bottleneck_i8 --------------------------------------------------------------------------------------------------------------------

def _bn(**change):
    from quantv2x_amd import lib
    d = lib.BottleneckDesc()
    d.n, d.h, d.w, d.planes, d.width, d.cg, d.in_zx, d.in_delta = 1, 3, 33, 128, 256, 8, 120, 0.1
    d.delta1, d.zp1, d.delta2, d.zp2, d.out_delta, d.out_zp = 0.05, 3.0, 0.04, 5.0, 0.03, 7.0
    return _set(d, change)


BN_SHAPE = b"planes 64 | 128 | 256, width = 2 x planes, 4 | 8 | 16 channels per group"
BN_REJECTS = [
    (dict(n=0), -1, b"bad shape"), (dict(h=0), -1, b"bad shape"), (dict(w=-5), -1, b"bad shape"),
    (dict(planes=96, width=192), -1, BN_SHAPE), (dict(planes=512, width=1024), -1, BN_SHAPE), (dict(width=128), -1, BN_SHAPE),
    (dict(width=512), -1, BN_SHAPE), (dict(cg=2), -1, BN_SHAPE), (dict(cg=32), -1, BN_SHAPE),
    (dict(delta1=0.0), -1, b"quantizer steps must be positive"), (dict(delta2=-1.0), -1, b"quantizer steps must be positive"),
    (dict(out_delta=0.0), -1, b"quantizer steps must be positive"),
]


def test_bottleneck_rejects(l, base):
    err, p = l.qv2x_last_error, vp(base)

    def bn(d, x=p, out=p, arrays=None, holes=()):
        """``holes``: (array 0..4 = w, scale, corr, aw, bias; layer 0..2; address) entries to plant; ``arrays``: the five array pointers"""
        rows = [(vp * 3)(*[base + 64 * (3 * a + i) for i in range(3)]) for a in range(5)]
        for a, i, addr in holes:
            rows[a][i] = addr
        return l.qv2x_bottleneck_i8(C.byref(d) if d is not None else None, x, *(arrays or rows), out, None)

    for change, rc, msg in BN_REJECTS:
        assert bn(_bn(**change)) == rc, change
        assert msg in err() and b"qv2x_bottleneck_i8:" in err(), (change, err())
    assert bn(None) == -1 and b"qv2x_bottleneck_i8: null pointer" in err()
    assert bn(_bn(), x=vp(None)) == -1 and b"qv2x_bottleneck_i8: null pointer" in err()
    assert bn(_bn(), out=vp(None)) == -1 and b"qv2x_bottleneck_i8: null pointer" in err()
    good = [(vp * 3)(base, base, base) for _ in range(5)]
    for a in range(5):
        arrays = list(good)
        arrays[a] = None
        assert bn(_bn(), arrays=arrays) == -1 and b"qv2x_bottleneck_i8: null pointer" in err(), a
    for a in range(5):
        for i in range(3):
            for addr in (None, base + 4):
                assert bn(_bn(n=0), holes=[(a, i, addr)]) == -2, (a, i, addr)          # (tested before the shape)
                assert b"qv2x_bottleneck_i8: layer %d constants null or not 16-byte aligned" % i in err(), (a, i, addr, err())
    assert bn(_bn(), holes=[(4, 2, base + 4), (0, 1, None)]) == -2 and b"layer 1 constants" in err()    # the first bad layer is named
    for kw in (dict(x=vp(base + 4)), dict(out=vp(base + 8))):
        assert bn(_bn(), **kw) == -2 and b"qv2x_bottleneck_i8: 16-byte aligned maps" in err(), kw
        assert bn(_bn(out_delta=0.0), **kw) == -1 and b"quantizer steps" in err(), kw       # the maps' alignment is the last check


# ---- qv2x_conv3x3_i8_wide_ok ---------------------------------------------------------------------------------------------------------------

CAT = [(0, 128), (128, 128), (256, 128)]
# n, h, w, stride, cout, input groups (c0, c), other fields, the answer -- taken from the library before the family's host layer was shared.
# cin_total = the end of the last group, the out window = [0, cout) of cout channels, out_delta 0.05, unless `other fields` say otherwise.
WIDE_OK = [
    (1, 200, 704, 2, 64, [(0, 64)], {}, 0),          # the full-size model at 1 frame: level 0, first layer
    (1, 100, 352, 1, 64, [(0, 64)], {}, 0),          # level 0
    (1, 100, 352, 2, 128, [(0, 64)], {}, 0),         # level 1, first layer
    (1, 50, 176, 1, 128, [(0, 128)], {}, 0),         # level 1
    (1, 50, 176, 2, 256, [(0, 128)], {}, 0),         # level 2, first layer
    (1, 25, 88, 1, 256, [(0, 256)], {}, 0),          # level 2
    (1, 100, 352, 1, 256, CAT, {}, 1),               # shrinker 0: the three deblock outputs
    (1, 100, 352, 1, 256, [(0, 256)], {}, 1),        # shrinker 1
    (8, 200, 704, 2, 64, [(0, 64)], {}, 1),          # ... at 8 frames
    (8, 100, 352, 1, 64, [(0, 64)], {}, 1),
    (8, 100, 352, 2, 128, [(0, 64)], {}, 0),
    (8, 50, 176, 1, 128, [(0, 128)], {}, 1),
    (8, 50, 176, 2, 256, [(0, 128)], {}, 1),
    (8, 25, 88, 1, 256, [(0, 256)], {}, 1),
    (8, 100, 352, 1, 256, CAT, {}, 1),
    (8, 100, 352, 1, 256, [(0, 256)], {}, 1),
    (32, 200, 704, 2, 64, [(0, 64)], {}, 1),         # ... at 32 frames
    (32, 100, 352, 1, 64, [(0, 64)], {}, 1),
    (32, 100, 352, 2, 128, [(0, 64)], {}, 1),
    (32, 50, 176, 1, 128, [(0, 128)], {}, 1),
    (32, 50, 176, 2, 256, [(0, 128)], {}, 1),
    (32, 25, 88, 1, 256, [(0, 256)], {}, 1),
    (32, 100, 352, 1, 256, CAT, {}, 1),
    (32, 100, 352, 1, 256, [(0, 256)], {}, 1),
    (102, 2, 3, 1, 512, [(0, 64)], {}, 0),           # 16320 | 16480 patch pixels (102 | 103 patches of 5 x 32)
    (103, 2, 3, 1, 512, [(0, 64)], {}, 1),
    (191, 2, 3, 1, 128, [(0, 128)], {}, 0),          # 191 | 192 workgroups of 128 channels
    (192, 2, 3, 1, 128, [(0, 128)], {}, 1),
    (191, 2, 3, 1, 256, [(0, 64)], {}, 1),           # wide_bn: 191 | 192 patches x 256 channels (128- | 256-channel workgroups)
    (192, 2, 3, 1, 256, [(0, 64)], {}, 1),
    (1023, 2, 3, 1, 64, [(0, 128)], {}, 0),          # 1023 | 1024 workgroups of 64 channels
    (1024, 2, 3, 1, 64, [(0, 128)], {}, 1),
    (1023, 2, 3, 1, 64, [(0, 64)], {}, 0),           # ws64_takes (1023 | 1024 patches of 10 x 32) chooses the kernel, not the answer
    (1024, 2, 3, 1, 64, [(0, 64)], {}, 1),
    (1023, 3, 5, 2, 64, [(0, 64)], {}, 0),           # ws2_takes: 1023 | 1024 patches of 8 x 32 outputs, cout 64 and 128
    (1024, 3, 5, 2, 64, [(0, 64)], {}, 1),
    (1023, 3, 5, 2, 128, [(0, 64)], {}, 0),
    (1024, 3, 5, 2, 128, [(0, 64)], {}, 1),
    (8, 100, 352, 1, 256, [(0, 1536)], {}, 1),       # MAX_CHUNKS: 24 | 25 chunks of 64 channels
    (8, 100, 352, 1, 256, [(0, 1600)], {}, 0),
    (8, 100, 352, 1, 256, [(0, 768), (768, 768)], {}, 1),        # ... over two groups
    (8, 100, 352, 1, 256, [(0, 768), (768, 832)], {}, 0),
    (8, 200, 704, 2, 256, [(0, 384)], {}, 1),        # ... at stride 2: 4 x 6 | 4 x 7
    (8, 200, 704, 2, 256, [(0, 448)], {}, 0),
    (8, 100, 352, 1, 256, [(0, 128), (128, 128)], {}, 1),        # two groups
    (8, 100, 352, 1, 512, [(64, 64), (0, 64)], {}, 1),           # ... out of channel order
    (8, 100, 352, 1, 128, [(0, 64), (64, 64)], {}, 0),           # ... need cout % 256 == 0
    (8, 200, 704, 2, 256, [(0, 64), (64, 64)], {}, 0),           # ... and stride 1
    (8, 200, 704, 2, 64, [(0, 128)], {}, 0),         # stride 2, 128 input channels (not ws2): cout 64 | 128 | 256
    (8, 200, 704, 2, 128, [(0, 128)], {}, 0),
    (8, 200, 704, 2, 256, [(0, 128)], {}, 1),
    (8, 200, 704, 2, 256, [(0, 64)], {}, 1),         # stride 2, 64 input channels, cout 256
    (8, 100, 352, 3, 256, [(0, 64)], {}, 0),         # malformed: stride, cout, group count, group channels, an empty map
    (8, 100, 352, 1, 192, [(0, 64)], {}, 0),
    (8, 100, 352, 1, 384, [(0, 64)], {}, 0),
    (8, 100, 352, 1, 256, [(0, 64)], {"ngroups": 0}, 0),
    (8, 100, 352, 1, 256, [(0, 64)], {"ngroups": 5}, 0),
    (8, 100, 352, 1, 256, [(0, 96)], {}, 0),
    (8, 100, 352, 1, 256, [(0, 0)], {}, 0),
    (8, 100, 352, 1, 256, [(8, 64)], {}, 0),
    (0, 100, 352, 1, 256, [(0, 64)], {}, 0),
    (8, 0, 352, 1, 256, [(0, 64)], {}, 0),
    (8, 100, -3, 1, 256, [(0, 64)], {}, 0),
]
# Descriptors qv2x_conv3x3_i8_wide itself refuses (asserted below) and the earlier qv2x_conv3x3_i8_wide_ok did not look at: it answered 1
# for each of them.  It now takes its rules from the code that fills the wide kernel's arguments and answers 0.
WIDE_OK_REFUSED = [
    (8, 100, 352, 1, 256, [(64, 64)], {"cin_total": 64}, 0),                       # group window past cin_total
    (8, 100, 352, 1, 256, [(0, 64)], {"cin_total": 72}, 0),                        # cin_total % 16
    (8, 100, 352, 1, 256, [(0, 64)], {"out_ctotal": 272, "out_c0": 8}, 0),         # out_c0 % 16
    (8, 100, 352, 1, 256, [(0, 64)], {"out_ctotal": 264}, 0),                      # out_ctotal % 16
    (8, 100, 352, 1, 256, [(0, 64)], {"out_ctotal": 256, "out_c0": 16}, 0),        # the window ends past out_ctotal
    (8, 100, 352, 1, 256, [(0, 64)], {"out_delta": 0.0}, 0),                       # no quantizer step
    (-8, -100, 352, 1, 256, [(0, 64)], {}, 0),                                     # two negative extents (a positive patch count)
]


def _wide_desc(n, h, w, stride, cout, groups, other):
    from quantv2x_amd import lib
    d = lib.ConvDesc()
    d.n, d.h, d.w, d.stride, d.cout, d.ngroups = n, h, w, stride, cout, len(groups)
    for i, (c0, c) in enumerate(groups):
        d.group_c0[i], d.group_c[i], d.group_zx[i] = c0, c, 100
    d.cin_total = max(c0 + c for c0, c in groups)
    d.out_ctotal, d.out_c0, d.relu, d.out_delta, d.out_zp = cout, 0, 1, 0.05, 0.0
    return _set(d, other)


def test_wide_ok_truth_table(l, base):
    l.qv2x_conv3x3_i8(None, *[None] * 8)                              # leaves a message behind: wide_ok must not touch it
    before = l.qv2x_last_error()
    assert b"null pointer" in before
    for row in WIDE_OK + WIDE_OK_REFUSED:
        assert l.qv2x_conv3x3_i8_wide_ok(C.byref(_wide_desc(*row[:-1]))) == row[-1], row
    assert l.qv2x_conv3x3_i8_wide_ok(None) == 0
    assert l.qv2x_last_error() == before
    p = vp(base)
    for row in WIDE_OK_REFUSED:
        assert l.qv2x_conv3x3_i8_wide(C.byref(_wide_desc(*row[:-1])), *[p] * 7, None) in (-1, -2), row
