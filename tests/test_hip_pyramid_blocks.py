"""The Pyramid model's int8 kernels one by one against the CPU oracle on random layers, bit for bit: qv2x_conv1x1_i8 (modes 0-3),
qv2x_gconv3x3_i8, qv2x_bottleneck_i8, qv2x_conv3x3_i8_res and qv2x_occ_score_i8.

The whole-frame tests (test_hip_pyramid.py, test_pyramid_variants.py) fix shapes and quantizers to one calibrated model: every post-ReLU zero
point is 0, stride 2 only reads even maps, channel counts are multiples of 128.  Here: zero points that are neither 0 nor 128 and differ
between the layers of a block, stride 2 on odd maps, maps smaller than / one pixel past a tile, several images, channel counts down to 32,
output channel windows, every tiles-per-wave form of the 1x1 kernel.  States come from tests/_pyramid_layers.py and go through the engine's
own packers, outputs are allocated full of a sentinel, and every case first asserts ON THE ORACLE'S OUTPUT that at least a third of the
codes lie strictly between the lowest code and 255 (tests/test_pyramid_blocks_cpu.py pins the oracle itself against numpy)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _pyramid_layers import (block_quantizer, bottleneck_state, conv1x1_state, conv3x3_state, f32_variant, gconv_state, occ_state, padded,
                             uniform_stats)

pytestmark = pytest.mark.gpu

SENT = -77
DX, ZX = np.float32(0.05), 7            # the input quantizer of every case: a zero point that is neither 0 nor 128
XQ = (DX, ZX)


def _oracle(state):
    from oracle.spec_pyramid import OraclePyramid
    orc = OraclePyramid.__new__(OraclePyramid)
    orc.s = state
    return orc


def _live(codes, lowest):
    """the condition on every case, on reference codes: a third of them strictly inside (lowest, 255)"""
    share = float(((codes > lowest) & (codes < 255)).mean())
    assert share >= 1 / 3, f"reference output mostly saturated: {share:.3f} inside"


def _dev():
    return torch.device("cuda")


def _to_dev(x_u8, zp):
    return torch.from_numpy(padded(x_u8, zp)).to(_dev())


def _sentinel_map(n, h, w, c):
    return torch.full((n, h + 2, w + 2, c), SENT, dtype=torch.int8, device=_dev())


def _codes(out, c0=0, c=None):
    """interior of a padded i8 map as u8 codes"""
    o = out.cpu().numpy() if hasattr(out, "cpu") else out
    c = o.shape[-1] - c0 if c is None else c
    return (o[:, 1:-1, 1:-1, c0:c0 + c].astype(np.int16) + 128).astype(np.uint8)


def _assert_untouched(out, c0=0, c=None):
    """the padded border and every channel outside [c0, c0 + c) still hold the sentinel"""
    o = out.cpu().numpy()
    c = o.shape[-1] - c0 if c is None else c
    for name, part in (("top", o[:, 0]), ("bottom", o[:, -1]), ("left", o[:, :, 0]), ("right", o[:, :, -1]),
                       ("channels below the window", o[..., :c0]), ("channels above the window", o[..., c0 + c:])):
        assert (part == SENT).all(), f"{name}: written"


def _out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


# ---- qv2x_conv1x1_i8 -------------------------------------------------------------------------------------------------------------------

def _launch_c1(layer, xin, n, h, w, mode, relu=1, out_q=(1.0, 0), res=None, res_q=(0.0, 128), out_c0=0, extra=0):
    from quantv2x_amd import lib as L
    ho, wo = _out_hw(h, w, layer.stride)
    if mode == 1:
        out = torch.full((n * ho * wo, layer.cout), float(SENT), dtype=torch.float32, device=_dev())
    else:
        out = _sentinel_map(n, ho, wo, layer.cout + extra)
    d = L.Conv1x1Desc()
    d.n, d.h, d.w, d.cin, d.cout, d.stride = n, h, w, layer.cin, layer.cout, layer.stride
    d.mode, d.relu = mode, relu
    d.out_ctotal, d.out_c0 = layer.cout + extra, out_c0
    d.out_delta, d.out_zp = float(out_q[0]), float(out_q[1])
    d.res_zx, d.res_delta = int(res_q[1]), float(res_q[0])
    L.check(L.load().qv2x_conv1x1_i8(C.byref(d), L.ptr(xin), L.ptr(layer.w), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw), L.ptr(layer.bias),
                                     L.ptr(res), L.ptr(out), L.current_stream()), "qv2x_conv1x1_i8")
    torch.cuda.synchronize()
    return out


C1_SHAPES = [        # cin, cout, n, h, w, stride
    (64, 128, 1, 3, 5, 1),          # 15 pixels: less than one 32-pixel tile
    (128, 64, 2, 5, 9, 1),          # M = 90: the second tile spans two images, the third is ragged
    (256, 512, 1, 9, 13, 2),        # stride 2 on (odd, odd) -> 5 x 7
    (512, 256, 2, 9, 12, 2),        # (odd, even) -> 5 x 6, the first tile spans two images
    (64, 64, 3, 8, 13, 2),          # (even, odd) -> 4 x 7
    (128, 128, 1, 7, 11, 1),        # M = 77
]
C1_VARIANTS = ["mode0", "mode0_norelu", "mode0_window", "mode1", "mode2", "mode3"]


@pytest.mark.parametrize("variant", C1_VARIANTS)
@pytest.mark.parametrize("cin,cout,n,h,w,stride", C1_SHAPES)
def test_conv1x1(cin, cout, n, h, w, stride, variant):
    from quantv2x_amd.engine_pyramid import _Conv1x1
    rng = np.random.default_rng(cin * 1000 + h * 37 + w)
    relu = variant != "mode0_norelu"
    out_zp = 5 if relu else 120
    sigma = 73.9 * float(DX)                                         # the shortcut's spread (modes 2 and 3)
    state = conv1x1_state(rng, "l", cin, cout, XQ, uniform_stats(ZX), out_zp, relu=relu, sigma=sigma)
    state.update(f32_variant(state, "l", "l_f32"))
    state.update(f32_variant(conv1x1_state(rng, "s", cin, cout, XQ, uniform_stats(ZX), 0, sigma=sigma), "s", "s_f32"))   # a 1x1 shortcut branch
    rq = (np.float32(0.04), 9)                                       # shortcut codes: res_zx neither 0 nor 128
    state.update(block_quantizer("b", rq, uniform_stats(rq[1]), sigma, 5))
    orc = _oracle(state)
    x = rng.integers(0, 256, size=(n, h, w, cin), dtype=np.uint8)
    ho, wo = _out_hw(h, w, stride)

    if variant.startswith("mode0"):
        want, oq = orc.convg("l", x, XQ, stride=stride, relu=relu)
        _live(want, out_zp if relu else 0)
        xin = _to_dev(x, ZX)
        c0, extra = (16, 32) if variant == "mode0_window" else (0, 0)
        layer = _Conv1x1(state, "l", XQ, stride, _dev())
        out = _launch_c1(layer, xin, n, h, w, 0, relu=int(relu), out_q=oq, out_c0=c0, extra=extra)
        _assert_untouched(out, c0, cout)
        np.testing.assert_array_equal(_codes(out, c0, cout), want)
        return
    y = orc.convg("l_f32", x, XQ, stride=stride, f32_out=True)
    if variant == "mode2":                                           # the fp32 shortcut a mode-1 launch of the strided branch leaves
        res = orc.convg("s_f32", x, XQ, stride=stride, f32_out=True)
    elif variant == "mode3":                                         # the block input's codes, dequantized in the epilogue
        r = rng.integers(0, 256, size=(n, ho, wo, cout), dtype=np.uint8)
        res = orc.dequant(r, rq)
    if variant != "mode1":
        want, oq = orc.finish("b", y, res)
        _live(want, 5)
    layer, xin = _Conv1x1(state, "l_f32", XQ, stride, _dev()), _to_dev(x, ZX)
    if variant == "mode1":
        out = _launch_c1(layer, xin, n, h, w, 1)
        np.testing.assert_array_equal(out.cpu().numpy().reshape(y.shape), y)       # bias + float(T) * scale: the same two roundings
        return
    if variant == "mode2":
        out = _launch_c1(layer, xin, n, h, w, 2, out_q=oq, res=torch.from_numpy(res.reshape(-1, cout)).to(_dev()))
    else:
        out = _launch_c1(layer, xin, n, h, w, 3, out_q=oq, res=_to_dev(r, rq[1]), res_q=rq)
    _assert_untouched(out)
    np.testing.assert_array_equal(_codes(out), want)


# 32-pixel tiles per wave (qv2x_conv1x1_i8's launch rule, restated):  tiles = ceil(M / 32), slices = cout / 64, tpw = 1;
#     while tpw < 8 and ceil(tiles / (8 tpw)) * slices >= 512: tpw *= 2
# At cout 512 (8 slices) a doubling needs ceil(tiles / (8 tpw)) >= 64, i.e. tiles >= 504 tpw + 1, M >= 16 128 tpw + 1: tpw = 2 from
# M = 16 129, 4 from 32 257, 8 from 64 513.  A workgroup walks 4 tpw tiles; with M just past a threshold the last workgroup holds one or
# two live tiles, waves that stop in the middle of their walk and waves whose whole walk lies past M.
@pytest.mark.parametrize("tpw,n,h,w", [
    (1, 1, 127, 126),           # M = 16 002 = 500 tiles + 2 pixels
    (2, 1, 127, 127),           # M = 16 129 = 504 tiles + 1 pixel: of the last workgroup's 8 tiles one is live
    (4, 2, 127, 127),           # M = 32 258 = 1008 tiles + 2 pixels: one live tile of 16
    (8, 3, 147, 147),           # M = 64 827 = 2025 tiles + 27 pixels: wave 0 walks 8 tiles, wave 1 stops after 2, waves 2 and 3 run none
])
def test_conv1x1_tiles_per_wave(tpw, n, h, w):
    from quantv2x_amd.engine_pyramid import _Conv1x1
    cin, cout, M = 64, 512, n * h * w
    tiles, t = (M + 31) // 32, 1
    while t < 8 and (tiles + 8 * t - 1) // (8 * t) * (cout // 64) >= 512:
        t *= 2
    assert t == tpw and M % 32 and (tiles + 4 * t - 1) // (4 * t) * 4 * t - tiles >= 2 * t      # two waves' worth of tiles past M
    rng = np.random.default_rng(tpw)
    state = conv1x1_state(rng, "l", cin, cout, XQ, uniform_stats(ZX), 5)
    x = rng.integers(0, 256, size=(n, h, w, cin), dtype=np.uint8)
    want, oq = _oracle(state).convg("l", x, XQ)
    _live(want, 5)
    out = _launch_c1(_Conv1x1(state, "l", XQ, 1, _dev()), _to_dev(x, ZX), n, h, w, 0, out_q=oq)
    _assert_untouched(out)
    np.testing.assert_array_equal(_codes(out), want)


# ---- qv2x_gconv3x3_i8 ------------------------------------------------------------------------------------------------------------------

def _launch_gconv(layer, xin, n, h, w, relu=1):
    from quantv2x_amd import lib as L
    ho, wo = _out_hw(h, w, layer.stride)
    out = _sentinel_map(n, ho, wo, layer.c)
    d = L.GconvDesc()
    d.n, d.h, d.w, d.c, d.cg, d.stride, d.relu = n, h, w, layer.c, layer.cg, layer.stride, relu
    d.out_delta, d.out_zp = layer.out_q[0], float(layer.out_q[1])
    L.check(L.load().qv2x_gconv3x3_i8(C.byref(d), L.ptr(xin), L.ptr(layer.w), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw), L.ptr(layer.bias),
                                      L.ptr(out), L.current_stream()), "qv2x_gconv3x3_i8")
    torch.cuda.synchronize()
    return out


G_CHANNELS = [(128, 4), (256, 8), (512, 16),          # the model's pairs
              (32, 4), (64, 8), (96, 4),              # one, two, three slabs: idle waves, fewer 16-byte pieces per patch pixel
              (160, 16)]                              # a second channel block with ONE slab
G_MAPS = [       # n, h, w, stride
    (1, 4, 32, 1),              # one exact 4 x 32 tile
    (1, 5, 33, 1),              # one row and one column into the next tile
    (2, 3, 4, 1),               # smaller than a tile, two images
    (1, 1, 1, 1),
    (1, 1, 1, 2),
    (1, 8, 64, 2),              # -> 4 x 32: an exact tile under stride 2
    (1, 13, 71, 2),             # (odd, odd) -> 7 x 36: ragged on both axes, the patch rows and columns clamp at the map's end
    (2, 12, 70, 2),             # (even, even) -> 6 x 35
]


def _gconv_case(c, cg, n, h, w, stride, relu):
    from quantv2x_amd.engine_pyramid import _GConv
    rng = np.random.default_rng(c * 100 + cg + 7 * h + w + stride)
    out_zp = 11 if relu else 120
    state = gconv_state(rng, "g", c, cg, XQ, uniform_stats(ZX), out_zp, relu=relu)
    x = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    want, oq = _oracle(state).convg("g", x, XQ, stride=stride, relu=relu)
    _live(want, out_zp if relu else 0)
    layer = _GConv(state, "g", XQ, stride, _dev())
    assert layer.out_q == (float(oq[0]), oq[1])
    out = _launch_gconv(layer, _to_dev(x, ZX), n, h, w, relu=int(relu))
    _assert_untouched(out)
    np.testing.assert_array_equal(_codes(out), want)


@pytest.mark.parametrize("n,h,w,stride", G_MAPS)
@pytest.mark.parametrize("c,cg", G_CHANNELS)
def test_gconv3x3(c, cg, n, h, w, stride):
    _gconv_case(c, cg, n, h, w, stride, True)


@pytest.mark.parametrize("c,cg,n,h,w,stride", [(96, 4, 1, 5, 33, 1), (256, 8, 1, 13, 71, 2)])
def test_gconv3x3_without_relu(c, cg, n, h, w, stride):
    _gconv_case(c, cg, n, h, w, stride, False)


# ---- qv2x_bottleneck_i8 ----------------------------------------------------------------------------------------------------------------

BN_ZP1, BN_ZP2, BN_OUT_ZP = 3, 11, 5               # with in_zx = 7: all non-zero, all different


def _launch_bottleneck(blk, xin, n, h, w):
    from quantv2x_amd import lib as L
    out = _sentinel_map(n, h, w, blk.cout)
    d = L.BottleneckDesc()
    d.n, d.h, d.w, d.planes, d.width, d.cg = n, h, w, blk.cout, blk.conv2.c, blk.conv2.cg
    d.in_zx, d.in_delta = int(blk.in_q[1]), float(blk.in_q[0])
    d.delta1, d.zp1 = blk.conv1.out_q[0], float(blk.conv1.out_q[1])
    d.delta2, d.zp2 = blk.conv2.out_q[0], float(blk.conv2.out_q[1])
    d.out_delta, d.out_zp = blk.out_q[0], float(blk.out_q[1])
    layers = (blk.conv1, blk.conv2, blk.conv3)
    arr = lambda name: (C.c_void_p * 3)(*[getattr(l, name).data_ptr() for l in layers])
    L.check(L.load().qv2x_bottleneck_i8(C.byref(d), L.ptr(xin), arr("w"), arr("scale"), arr("corr"), arr("aw"), arr("bias"), L.ptr(out),
                                        L.current_stream()), "qv2x_bottleneck_i8")
    torch.cuda.synchronize()
    return out


def _refill_border(t, zp):
    """a sentinel-checked intermediate map becomes the next layer's input: its border takes that layer's pad code"""
    code = int(zp) - 128
    t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = code, code, code, code
    return t


BN_CASES = [(planes, cg, n, h, w) for planes, cg in [(64, 4), (128, 8), (256, 16)]
            for n, h, w in [(1, 2, 32), (1, 1, 5), (1, 3, 33), (2, 7, 40)]]          # one exact 2 x 32 patch; less than one; one past it on
BN_CASES.append((256, 16, 1, 6, 70))                                                 # both axes; two images; nine patches of the 256-plane form


@pytest.mark.parametrize("planes,cg,n,h,w", BN_CASES)
def test_bottleneck(planes, cg, n, h, w):
    """One launch and the three separate launches against ``residual_block``; the block's intermediate maps against its taps."""
    from quantv2x_amd.engine_pyramid import _Block
    rng = np.random.default_rng(planes + 10 * h + w)
    name = "blk"
    state = bottleneck_state(rng, name, planes, cg, XQ, uniform_stats(ZX), BN_ZP1, BN_ZP2, BN_OUT_ZP)
    x = rng.integers(0, 256, size=(n, h, w, planes), dtype=np.uint8)
    taps = {}
    want, oq = _oracle(state).residual_block(name, x, XQ, 1, ["conv1", "conv2", "conv3"], taps)
    t1_want, t2_want = taps[name + ".conv1"], taps[name + ".conv2"]
    _live(t1_want, BN_ZP1), _live(t2_want, BN_ZP2), _live(want, BN_OUT_ZP)
    edge = np.concatenate([t1_want[:, 0].ravel(), t1_want[:, -1].ravel(), t1_want[:, :, 0].ravel(), t1_want[:, :, -1].ravel()])
    assert (edge != BN_ZP1).mean() > 1 / 3                           # non-zero conv1 outputs next to the halo: its fill matters
    blk = _Block(state, name, (float(DX), ZX), 1, True, _dev())
    assert (blk.conv1.out_q[1], blk.conv2.out_q[1], blk.out_q[1]) == (BN_ZP1, BN_ZP2, BN_OUT_ZP) and blk.out_q == (float(oq[0]), oq[1])
    xin = _to_dev(x, ZX)

    fused = _launch_bottleneck(blk, xin, n, h, w)
    _assert_untouched(fused)
    np.testing.assert_array_equal(_codes(fused), want, err_msg="qv2x_bottleneck_i8 vs the oracle")

    # conv1x1 mode 0 -> gconv -> conv1x1 mode 3, the borders of t1 / t2 at each layer's own pad code
    t1 = _launch_c1(blk.conv1, xin, n, h, w, 0, out_q=blk.conv1.out_q)
    _assert_untouched(t1)
    np.testing.assert_array_equal(_codes(t1), t1_want, err_msg="conv1")
    t2 = _launch_gconv(blk.conv2, _refill_border(t1, BN_ZP1), n, h, w)
    _assert_untouched(t2)
    np.testing.assert_array_equal(_codes(t2), t2_want, err_msg="conv2")
    out = _launch_c1(blk.conv3, _refill_border(t2, BN_ZP2), n, h, w, 3, out_q=blk.out_q, res=xin, res_q=XQ)
    _assert_untouched(out)
    np.testing.assert_array_equal(_codes(out), want, err_msg="three launches vs the oracle")
    np.testing.assert_array_equal(fused.cpu().numpy(), out.cpu().numpy(), err_msg="one launch vs three")


# ---- qv2x_conv3x3_i8_res ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res_mode", [2, 3])
@pytest.mark.parametrize("n,h,w", [(1, 5, 32), (1, 6, 33), (1, 3, 4), (2, 13, 37)])
def test_conv3x3_res(n, h, w, res_mode):
    from quantv2x_amd import lib as L
    from quantv2x_amd.engine import _ConvLayer
    rng = np.random.default_rng(100 * h + w + res_mode)
    sigma = 73.9 * float(DX)
    state = conv3x3_state(rng, "c2", 64, 64, XQ, uniform_stats(ZX), 0, sigma=sigma, a_off=True)
    rq = (np.float32(0.04), 9)
    state.update(block_quantizer("b", rq, uniform_stats(rq[1]), sigma, 5))
    orc = _oracle(state)
    x = rng.integers(0, 256, size=(n, h, w, 64), dtype=np.uint8)
    y = orc.convg("c2", x, XQ, f32_out=True)
    if res_mode == 2:
        res = rng.normal(0.0, sigma, size=y.shape).astype(np.float32)
    else:
        r = rng.integers(0, 256, size=y.shape, dtype=np.uint8)
        res = orc.dequant(r, rq)
    want, oq = orc.finish("b", y, res)
    _live(want, 5)
    res_dev = torch.from_numpy(res.reshape(-1, 64)).to(_dev()) if res_mode == 2 else _to_dev(r, rq[1])
    layer = _ConvLayer(state, "c2", [(0, 64, DX, ZX)], 1, _dev())
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin_total, d.stride, d.cout, d.ngroups = n, h, w, 64, 1, 64, 1
    d.group_c0[0], d.group_c[0], d.group_zx[0] = 0, 64, ZX
    d.out_ctotal, d.out_c0, d.relu = 64, 0, 1
    d.out_delta, d.out_zp = float(oq[0]), float(oq[1])
    out = _sentinel_map(n, h, w, 64)
    L.check(L.load().qv2x_conv3x3_i8_res(C.byref(d), L.ptr(_to_dev(x, ZX)), L.ptr(layer.w), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw),
                                         L.ptr(layer.bias), res_mode, L.ptr(res_dev), int(rq[1]), float(rq[0]), L.ptr(out), L.current_stream()),
            "qv2x_conv3x3_i8_res")
    torch.cuda.synchronize()
    _assert_untouched(out)
    np.testing.assert_array_equal(_codes(out), want)


# ---- qv2x_occ_score_i8 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [64, 128, 256])
def test_occ_score(c):
    from oracle.spec_pyramid import sigmoid_lut
    from quantv2x_amd import lib as L
    from quantv2x_amd.engine_pyramid import _Occ
    n, h, w = 2, 9, 17                                               # 306 pixels: two workgroups, the second ragged; no multiple of 64
    rng = np.random.default_rng(c)
    state = occ_state(rng, "occ", c, XQ, uniform_stats(ZX))
    x = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    want, oq = _oracle(state).convg("occ", x, XQ, relu=False)
    _live(want, 0)
    oc = _Occ(state, "occ", XQ, _dev())
    lut = oc.lut.cpu().numpy()
    np.testing.assert_array_equal(lut, sigmoid_lut(*oq)[0])
    d = L.OccDesc()
    d.n, d.h, d.w, d.c, d.aw, d.corr = n, h, w, oc.c, oc.aw, oc.corr
    d.scale, d.bias, d.out_delta, d.out_zp = oc.scale, oc.bias, oc.out_q[0], float(oc.out_q[1])
    xin = _to_dev(x, ZX)
    for with_codes in (True, False):                                 # occ_code = NULL: the score alone
        score = torch.full((n * h * w + 64,), float(SENT), dtype=torch.float32, device=_dev())
        code = torch.full((n * h * w + 64,), 201, dtype=torch.uint8, device=_dev()) if with_codes else None
        L.check(L.load().qv2x_occ_score_i8(C.byref(d), L.ptr(xin), L.ptr(oc.w), L.ptr(oc.lut), L.ptr(score), L.ptr(code), L.current_stream()),
                "qv2x_occ_score_i8")
        torch.cuda.synchronize()
        score = score.cpu().numpy()
        assert (score[n * h * w:] == SENT).all()
        np.testing.assert_array_equal(score[:n * h * w], lut[want.reshape(-1)])
        if with_codes:
            code = code.cpu().numpy()
            assert (code[n * h * w:] == 201).all()
            np.testing.assert_array_equal(code[:n * h * w], want.reshape(-1))
