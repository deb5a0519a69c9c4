"""``orc_conv3x3`` -- the reference of tests/test_hip_conv_layers.py -- pinned against an independent float64 statement of the layer at relu
0 / 1, stride 1 / 2, one to four groups with gaps and out of channel order, inside an output window; the helpers of tests/_conv_layers.py
checked on themselves; every argument reject of the three convolution entries and of the weight packer on host addresses.  No GPU.

numpy side (``float64_codes``): T_g exact (float64 matrix products of integers below 2^53), y = bias + sum_g T_g scale_g and the quantizer
p = max(y, 0) / delta + zp, code = clip(rint(p), 0, 255), in float64, scale_g the fp32 product dx_g * dw the oracle is given.  The oracle's fp32
evaluation -- (float)T_g, one product and one sum per group, the fma of the quantizer -- differs from that by at most
(G + 3) 2^-24 (|bias| + sum_g |T_g scale_g|) / delta code units, plus 1.2e-7 |y / delta| for the multiplication by fl(1 / delta) in place
of the division (csrc/common.h).  Excluded are exactly the positions whose p lies within that bound of a half-integer; every other position
and every byte outside the window must be equal.  The excluded share is a condition on the inputs and may be at most 1 %.  Measured shares
(printed by the test):

    k64_ragged_spare_channels   relu 1 zp 7: 0.026 %    relu 0 zp 120: 0.032 %
    k64_stride2_odd_input       relu 1 zp 7: 0.020 %    relu 0 zp 120: 0.020 %
    k128_stride2                relu 1 zp 7: 0.038 %    relu 0 zp 120: 0.040 %
    multi_out_of_order_gaps     relu 1 zp 7: 0.028 %    relu 0 zp 120: 0.039 %    relu 1 zp 0: 0.024 %    relu 0 zp 64: 0.024 %
    multi_three_groups_gap      relu 1 zp 7: 0.050 %    relu 0 zp 120: 0.084 %
    multi_four_groups           relu 1 zp 7: 0.093 %    relu 0 zp 120: 0.078 %
    multi_stride2               relu 1 zp 7: 0.025 %    relu 0 zp 120: 0.045 %
"""
import ctypes as C

import numpy as np
import pytest

from _conv_layers import (BACK, CHAIN_CASES, EXTRA_CASES, EXTRA_VARIANTS, EXTREME_SHAPES, FRONT, REGULAR_CASES, SENT, VARIANTS, WIDE_CASES, Case, Plan,
                          Prepared, PreparedChain, assert_extreme_reference, extreme_input, extreme_layer, float64_codes, launch_plan, oracle_conv,
                          zx_sensitivity)

CAP = 0.01
PINS = [(name, v) for name in ("k64_ragged_spare_channels", "k64_stride2_odd_input", "k128_stride2", "multi_out_of_order_gaps", "multi_three_groups_gap",
                               "multi_four_groups", "multi_stride2") for v in VARIANTS] + [("multi_out_of_order_gaps", v) for v in EXTRA_VARIANTS]
_vid = lambda v: v if isinstance(v, str) else f"relu{v[0]}_zp{v[1]}"


@pytest.mark.parametrize("name,variant", PINS, ids=_vid)
def test_orc_conv3x3_matches_float64(name, variant):
    prep = Prepared(REGULAR_CASES[name], variant)
    cout = prep.case.cout
    want, near = float64_codes(prep.layer, prep.x)
    share = float(near.mean())
    print(f"{name} relu {variant[0]} zp {variant[1]}: excluded share {100 * share:.3f} % of {near.size}")
    assert share <= CAP, f"{100 * share:.2f} % of the positions sit on a rounding boundary: pick another seed"
    got = (prep.expect[:, 1:-1, 1:-1].astype(np.int16) + 128).astype(np.uint8)      # the oracle's whole destination, window at FRONT
    assert (got[..., :FRONT] == SENT + 128).all() and (got[..., FRONT + cout:] == SENT + 128).all(), "the oracle wrote outside its window"
    assert got.shape[-1] == FRONT + cout + BACK
    np.testing.assert_array_equal(got[..., FRONT:FRONT + cout][~near], want[~near])
    # and the same layer without the window
    np.testing.assert_array_equal(oracle_conv(prep.layer, prep.x), prep.want)


# ---- the helpers on themselves -------------------------------------------------------------------------------------------------------------

def _plan(entry, shape, stride, groups, cout):
    return launch_plan(entry, Case(entry, None, shape, stride, groups, cout))


def test_launch_rule_restatement():
    """one row per form and both sides of every threshold, written by hand from conv3x3_entry, qv2x_conv3x3_i8_wide, ws64_takes, ws2_takes"""
    reg = lambda *a: _plan("regular", *a).form
    assert launch_plan("regular", Case("regular", None, (1, 8, 8), 1, [(0, 64)], 64), res_mode=2).form == "res"
    assert reg((1, 8, 8), 1, [(0, 64), (64, 64)], 128) == "multi"
    assert reg((1, 128, 128), 1, [(0, 128), (128, 128)], 256) == "multi"                 # multi is tested before large
    assert reg((1, 127, 129), 1, [(0, 64)], 128) == "k64" and reg((1, 128, 128), 1, [(0, 64)], 128) == "large"        # M 16383 | 16384
    assert reg((1, 128, 128), 1, [(0, 64)], 64) == "k64" and reg((1, 128, 128), 1, [(0, 64)], 192) == "k64"           # large needs cout % 128 == 0
    assert reg((1, 128, 128), 1, [(0, 256)], 256) == "large"                              # ... and is tested before k256
    assert reg((1, 64, 64), 1, [(0, 256)], 256) == "k256" and reg((1, 64, 65), 1, [(0, 256)], 256) == "k128"          # wgs64 256 | 260
    assert reg((1, 64, 128), 1, [(0, 256)], 128) == "k256" and reg((1, 64, 129), 1, [(0, 256)], 128) == "k128"        # ... with cout 128: 256 | 258
    assert reg((2, 64, 128), 1, [(0, 256)], 64) == "k256" and reg((2, 64, 129), 1, [(0, 256)], 64) == "k128"          # ... with cout 64, M = 16384
    assert reg((1, 13, 37), 1, [(0, 128)], 64) == "k128" and reg((1, 13, 37), 1, [(0, 192)], 64) == "k64"
    assert reg((1, 511, 513), 1, [(0, 64)], 64) == "k64" and reg((1, 512, 512), 1, [(0, 64)], 64) == "m192"           # M 262143 | 262144
    assert reg((1, 512, 512), 1, [(0, 128)], 64) == "k128"                                # m192 is for K chunks of 64 only
    assert reg((4, 512, 514), 2, [(0, 64)], 64) == "m192" and reg((4, 512, 514), 2, [(0, 64)], 128) == "large"
    wide = lambda *a: _plan("wide", *a)
    assert wide((1023, 2, 3), 1, [(0, 64)], 64) == Plan("bn64", 1024, 1024, 1, 1)         # patches 1023 | 1024 for ws64
    assert wide((1024, 2, 3), 1, [(0, 64)], 64) == Plan("ws64", 512, 1024, 2, 2)
    assert wide((1024, 2, 3), 1, [(0, 128)], 64).form == "bn64" and wide((1024, 2, 3), 1, [(0, 64)], 128).form == "bn128"
    assert wide((103, 100, 33), 1, [(0, 64)], 64) == Plan("ws64", 512, 2060, 5, 4)        # 10 x 2 patches of 10 x 32 per image
    assert wide((1023, 3, 5), 2, [(0, 64)], 64) == Plan("s2_bn64", 768, 1024, 2, 1)       # patches 1023 | 1024 for ws2, both widths
    assert wide((1024, 3, 5), 2, [(0, 64)], 64) == Plan("ws2_2x2", 512, 1024, 2, 2)
    assert wide((1023, 3, 5), 2, [(0, 64)], 128) == Plan("s2_bn128", 512, 1024, 2, 2)
    assert wide((1024, 3, 5), 2, [(0, 64)], 128) == Plan("ws2_4x1", 512, 1024, 2, 2)
    assert wide((1024, 3, 5), 2, [(0, 64)], 256).form == "s2_bn256" and wide((1024, 3, 5), 2, [(0, 128)], 64).form == "s2_bn64"
    assert wide((64, 17, 65), 2, [(0, 64)], 64) == Plan("s2_bn64", 256, 256, 1, 1)        # 9 x 33 outputs: 2 x 2 tiles of 8 x 32, 64 x 4 = 256 < 1024
    assert wide((95, 2, 3), 1, [(0, 64)], 512) == Plan("bn128", 384, 384, 1, 1)           # patches * cout / 256 = 190 | 192
    assert wide((96, 2, 3), 1, [(0, 64)], 512) == Plan("bn256", 192, 192, 1, 1)
    assert wide((191, 2, 3), 1, [(0, 64)], 256) == Plan("bn128", 384, 384, 1, 1) and wide((192, 2, 3), 1, [(0, 64)], 256) == Plan("bn256", 192, 192, 1, 1)
    assert wide((191, 2, 3), 1, [(0, 64), (64, 64)], 256) == Plan("multi_bn128", 256, 384, 2, 1)     # one multi-group workgroup per CU
    assert wide((297, 2, 3), 1, [(0, 64)], 256) == Plan("bn256", 256, 304, 2, 1)
    assert wide((12, 50, 96), 1, [(0, 64)], 768) == Plan("bn256", 240, 1080, 5, 4)        # the slots are a multiple of 8 x 3: 256 -> 240
    assert wide((1, 10, 64), 2, [(0, 384)], 256) == Plan("s2_bn128", 16, 16, 1, 1)
    assert launch_plan("chain", (2, 23, 70, 3, 2)) == Plan(("chain", 3, 2), 2 * 3 * 2, 2 * 3 * 2, 1, 1)
    for case in list(REGULAR_CASES.values()) + list(WIDE_CASES.values()) + list(CHAIN_CASES.values()):
        case.assert_plan()
    for entry, form, c, cout, stride, (n, h, w) in EXTREME_SHAPES:
        plan = launch_plan("chain", (n, h, w, 1, stride)) if entry == "chain" else _plan(entry, (n, h, w), stride, [(0, c)], cout)
        assert plan.form == form


SENSITIVE = [(name, v) for name in ("k64_ragged_spare_channels", "k64_stride2_odd_input", "multi_out_of_order_gaps", "multi_four_groups")
             for v in VARIANTS + EXTRA_VARIANTS]
SENSITIVE += [(name, v) for name in ("k64_less_than_a_tile", "bn256_one_item_each", "multi_bn256_three_groups", "s2_bn256") for v in VARIANTS]


@pytest.mark.parametrize("name,variant", SENSITIVE, ids=_vid)
def test_cases_are_sensitive_to_every_input_zero_point(name, variant):
    """a condition on the inputs, on the oracle: one code of ONE group's zx either way changes at least 10 % of the reference codes, so a
    kernel that dropped a group's correction term, used another group's or was one off in it cannot pass.  Every generator configuration of
    the GPU list: one, two, three and four groups, images that are all edge (ZX_TINY), the four quantizers.  (One code of zx moves T by
    sum(w - zw) = 9 c (127.5 - zw) +- 73.9 sqrt(9 c): several output steps for most channels.)"""
    case = (REGULAR_CASES | WIDE_CASES)[name]
    prep = Prepared(case, variant)
    share = zx_sensitivity(prep.layer, prep.x, prep.want)
    print(f"{name} relu {variant[0]} zp {variant[1]}: zx +- 1 of one group changes at least {100 * share:.1f} % of the reference codes")
    assert share >= 0.10


SMALL = [(n, c) for n, c in (REGULAR_CASES | WIDE_CASES).items() if not n.startswith("m192")]


@pytest.mark.parametrize("name", [n for n, _ in SMALL])
def test_gpu_cases_are_live(name):
    """``live`` on the oracle's codes (asserted in Prepared) for every case and variant of the GPU list: a case that is not live fails here first"""
    case = (REGULAR_CASES | WIDE_CASES)[name]
    for variant in case.variants + (EXTRA_VARIANTS if name in EXTRA_CASES else ()):
        Prepared(case, variant)


@pytest.mark.parametrize("name", ["m192_stride2", "m192"])
def test_m192_cases_are_live(name):
    """the two large cases (10 GMAC each in the oracle, twice under ReLU with zp 7)"""
    case = REGULAR_CASES[name]
    Prepared(case, case.variants[0])


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chain_cases_are_live_and_sensitive(name):
    """``live`` on every layer of the chain (asserted in PreparedChain), and every layer's zx -- the pad code of the map before it -- matters"""
    prep = PreparedChain(CHAIN_CASES[name])
    for l, (layer, want) in enumerate(zip(prep.layers, prep.wants)):
        share = zx_sensitivity(layer, prep.x if l == 0 else prep.wants[l - 1], want)
        print(f"{name} layer {l}: zx +- 1 changes at least {100 * share:.1f} % of the reference codes")
        assert share >= 0.10


@pytest.mark.parametrize("relu,zp", [(1, 7), (0, 120)])
@pytest.mark.parametrize("zx", [0, 255])
def test_extreme_reference_meets_the_kernels_conditions(zx, relu, zp):
    for entry, form, c, cout, stride, (n, h, w) in EXTREME_SHAPES:
        layer, x = extreme_layer(c, cout, stride, relu, zp, zx), extreme_input(n, h, w, c)
        want = oracle_conv(layer, x)
        assert_extreme_reference(layer, x, want)
        ref, near = float64_codes(layer, x)
        assert not near.any()                                        # (80, 53.3 and 35.6 steps from an integer: far from every boundary)
        np.testing.assert_array_equal(want, ref)


# ---- argument rejects ----------------------------------------------------------------------------------------------------------------------

def _good(**change):
    from quantv2x_amd import lib
    d = lib.ConvDesc()
    d.n, d.h, d.w, d.cin_total, d.stride, d.cout, d.ngroups = 1, 5, 32, 128, 1, 256, 1
    d.group_c0[0], d.group_c[0], d.group_zx[0] = 64, 64, 100
    d.out_ctotal, d.out_c0, d.relu, d.out_delta, d.out_zp = 304, 16, 0, 0.05, 120.0
    for k, v in change.items():
        if k.startswith("group_"):
            for i, e in enumerate(v):
                getattr(d, k)[i] = e
        else:
            setattr(d, k, v)
    return d


TWO_GROUPS = dict(ngroups=2, group_c0=[64, 0], group_c=[64, 64])
REGULAR_REJECTS = [      # fields to change, return code, a piece of the message
    (dict(n=0), -1, b"bad shape"), (dict(h=0), -1, b"bad shape"), (dict(stride=3), -1, b"bad shape n=1 h=5 w=32 stride=3"),
    (dict(ngroups=0), -1, b"1..4 input groups"), (dict(ngroups=5), -1, b"1..4 input groups"),
    (dict(cout=96), -2, b"cout % 64"), (dict(cin_total=72), -2, b"cin_total % 16"),
    (dict(out_ctotal=256), -2, b"out channel window"),                       # out_ctotal < out_c0 + cout: [16, 272) ends past 256 channels
    (dict(out_c0=8), -2, b"out_ctotal and out_c0 must be multiples of 16"), (dict(out_ctotal=312), -2, b"must be multiples of 16"),
    (dict(group_c=[0]), -2, b"group 0 (c0=64, c=0)"), (dict(group_c=[96]), -2, b"multiples of 64"), (dict(group_c0=[8]), -2, b"group 0 (c0=8"),
    (dict(group_c0=[80]), -2, b"group 0 (c0=80, c=64)"),                     # group c0 + c > cin_total
    (dict(ngroups=2, group_c0=[0, 64], group_c=[64, 128]), -2, b"group 1 (c0=64, c=128)"),
    (dict(out_delta=0.0), -1, b"out_delta must be positive"),
    (dict(cout=64, **TWO_GROUPS), -1, b"multi-group input needs cout % 128 == 0"), (dict(cout=192, **TWO_GROUPS), -1, b"multi-group input needs"),
]
WIDE_REJECTS = [
    (dict(n=0), -1, b"bad shape"), (dict(w=0), -1, b"bad shape"),
    (dict(stride=3), -1, b"stride 1 | 2 and cout 64 | 128 | a multiple of 256"), (dict(cout=192), -1, b"a multiple of 256"), (dict(cout=384), -1, b"a multiple of 256"),
    (dict(stride=2, **TWO_GROUPS), -1, b"the stride-2 form takes one input group"),
    (dict(cout=128, **TWO_GROUPS), -1, b"the 64 / 128-channel form takes one input group"), (dict(cout=64, ngroups=0), -1, b"takes one input group"),
    (dict(ngroups=0), -1, b"1..4 input groups"), (dict(ngroups=5), -1, b"1..4 input groups"),
    (dict(cin_total=72), -2, b"out channel window"), (dict(out_ctotal=256), -2, b"out channel window"), (dict(out_c0=8), -2, b"out_c0 % 16"),
    (dict(out_ctotal=312), -2, b"out_ctotal, out_c0 % 16"),
    (dict(out_delta=-1.0), -1, b"out_delta must be positive"),
    (dict(group_c=[0]), -2, b"group 0 (c0=64, c=0)"), (dict(group_c=[96]), -2, b"multiples of 64"), (dict(group_c0=[8]), -2, b"group 0 (c0=8"),
    (dict(group_c0=[80]), -2, b"group 0 (c0=80, c=64)"),
    (dict(cin_total=1600, group_c0=[0], group_c=[1600]), -1, b"more than 24 64-channel chunks"),
    (dict(cin_total=1600, ngroups=2, group_c0=[0, 1536], group_c=[1536, 64]), -1, b"more than 24"),
    (dict(stride=2, cin_total=448, group_c0=[0], group_c=[448]), -1, b"stride 2 takes at most 384 input channels"),
]


def test_argument_errors_of_the_convolution_entries_without_gpu():
    """rejected calls only (an accepted one would launch): every reject of conv3x3_entry, of fill_args through qv2x_conv3x3_i8_wide and
    qv2x_conv3x3_i8_pack_wide, and of qv2x_conv3x3_i8_chain64.  No pointer is dereferenced on a reject: they are host addresses."""
    from quantv2x_amd import build, lib
    build.build()
    l = lib.load()
    l.qv2x_conv3x3_i8_pack_wide.restype = C.c_int
    raw = np.zeros(4096 + 16, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16                 # a 16-byte aligned host address: no kernel ever sees it
    p, vp = C.c_void_p(base), C.c_void_p
    err = l.qv2x_last_error

    def conv(fn, d, ptrs=None):
        return fn(C.byref(d), *(ptrs or [p] * 7), None)

    for change, rc, msg in REGULAR_REJECTS:
        assert conv(l.qv2x_conv3x3_i8, _good(**change)) == rc, change
        assert msg in err() and b"qv2x_conv3x3_i8:" in err(), (change, err())
    for change, rc, msg in WIDE_REJECTS:
        assert conv(l.qv2x_conv3x3_i8_wide, _good(**change)) == rc, change
        assert msg in err() and b"qv2x_conv3x3_i8_wide:" in err(), (change, err())
        assert l.qv2x_conv3x3_i8_pack_wide(C.byref(_good(**change)), p, p, None) == rc, change
        assert msg in err(), (change, err())
    for who, fn in (("qv2x_conv3x3_i8", l.qv2x_conv3x3_i8), ("qv2x_conv3x3_i8_wide", l.qv2x_conv3x3_i8_wide)):
        for hole in range(7):
            ptrs = [p] * 7
            ptrs[hole] = vp(None)
            assert conv(fn, _good(), ptrs) == -1 and who.encode() + b": null pointer" in err(), (who, hole)
        assert fn(None, *[p] * 7, None) == -1 and b"null pointer" in err()
        for hole in (0, 1, 6):                                       # in, w, out
            ptrs = [p] * 7
            ptrs[hole] = vp(base + 4)
            assert conv(fn, _good(), ptrs) == -2 and who.encode() + b": in / w / out must be 16-byte aligned" in err(), (who, hole)
    for args in ((None, p, p), (C.byref(_good()), vp(None), p), (C.byref(_good()), p, vp(None))):
        assert l.qv2x_conv3x3_i8_pack_wide(*args, None) == -1 and b"qv2x_conv3x3_i8_pack_wide: null pointer" in err()
    for args in ((vp(base + 8), p), (p, vp(base + 4))):
        assert l.qv2x_conv3x3_i8_pack_wide(C.byref(_good()), *args, None) == -2 and b"qv2x_conv3x3_i8_pack_wide: 16-byte alignment" in err()

    def chain(**change):
        d = lib.ChainDesc()
        d.n, d.h, d.w, d.in_h, d.in_w, d.depth, d.stride0, d.relu = 1, 5, 31, 9, 61, 4, 2, 0
        for i in range(4):
            d.out_delta[i], d.out_zp[i] = 0.05, 120.0
        for k, v in change.items():
            if k == "out_delta":
                d.out_delta[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    who = b"qv2x_conv3x3_i8_chain64: "
    for change, rc, msg in [(dict(n=0), -1, b"bad shape"), (dict(h=0), -1, b"bad shape"), (dict(stride0=3), -1, b"bad shape n=1 h=5 w=31 stride0=3"),
                            (dict(stride0=0), -1, b"bad shape"), (dict(depth=0), -1, b"1..4 layers"), (dict(depth=5), -1, b"1..4 layers"),
                            (dict(in_h=11), -1, b"a 11 x 61 input does not give 5 x 31 at stride 2"), (dict(w=32), -1, b"does not give 5 x 32"),
                            (dict(stride0=1), -1, b"does not give"), (dict(out_delta=(3, 0.0)), -1, b"out_delta must be positive"),
                            (dict(out_delta=(0, -1.0)), -1, b"out_delta must be positive")]:
        assert conv(l.qv2x_conv3x3_i8_chain64, chain(**change)) == rc, change
        assert who + msg in err() or (who in err() and msg in err()), (change, err())
    for hole in range(7):
        ptrs = [p] * 7
        ptrs[hole] = vp(None)
        assert conv(l.qv2x_conv3x3_i8_chain64, chain(), ptrs) == -1 and who + b"null pointer" in err(), hole
    assert l.qv2x_conv3x3_i8_chain64(None, *[p] * 7, None) == -1 and b"null pointer" in err()
    for hole in (0, 1, 6):
        ptrs = [p] * 7
        ptrs[hole] = vp(base + 4)
        assert conv(l.qv2x_conv3x3_i8_chain64, chain(), ptrs) == -2 and who + b"in / w / out must be 16-byte aligned" in err(), hole
