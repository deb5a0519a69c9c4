"""``orc_deconv`` and ``orc_deconv_f32in`` -- the references of tests/test_hip_deblock_layers.py -- pinned against plain numpy in float64 at
shapes the golden vectors do not hold (s 3 and 8, Cout 32 and 96, Cin 16 and 48, no ReLU with zp 128, ReLU with zp 7); the helpers of
tests/_deblock_layers.py checked on themselves; the argument rejects of the three deblock entries on host buffers.  No GPU.

numpy side:  y64 = sum_c float64(x^_c) float64(w_c) + b  with x^ the fp32 dequantized input exactly as the oracle forms it
(float32(code - zx) * dx; the fp32 map itself for orc_deconv_f32in), p = y64 / da + za, code = clip(rint(p), 0, 255).  The oracle's fp32 fma
chain differs from y64 by at most  (Cin + 2) 2^-24 (sum_c |x^_c w_c| + |b|).  Excluded are exactly the elements whose p lies within that
bound (in code units, plus 1e-6 for the fp32 reciprocal multiply) of a half-integer; every other element must be equal.  The excluded
share of a case is a condition on the inputs and may be at most 3 %.  Shares of the cases below (printed by the test):

    i8  cin16_cout32_s8_relu_zp7     0.13 %        f32 cin16_cout96_s3_norelu_zp128   0.04 %
    i8  cin48_cout96_s3_norelu_zp128 0.32 %        f32 cin48_cout32_s8_relu_zp7       0.19 %
    i8  cin16_cout96_s2_norelu_zp128 0.07 %        f32 cin128_cout96_s2_relu_zp7      0.76 %
    i8  cin48_cout32_s2_relu_zp7     0.22 %
    i8  cin128_cout96_s2_relu_zp7    1.34 %
    i8  cin64_cout32_s3_relu_zp0     0.29 %

(The saturating steps of these layers put 64 to 128 codes on one sigma of y, two to four times what the backbone's own quantizers do, and the
band grows with it; in_zx 255 or 3 makes |x^| large beside its spread.  Cin 256 would exceed the cap at these steps and is left to the
golden vectors.)
"""
import ctypes as C

import numpy as np
import pytest

from _deblock_layers import (DX, F32_CASES, I8_CASES, QUANT_GRID, X_STD_F32, Prepared, assert_plan, deblock_layer, launch_plan, live,
                             oracle_codes, out_step, quant_case, zx_sensitivity)

CAP = 0.03

# name: cin, cout, s, n, h, w, relu, zp, zx, seed
PIN_I8 = {
    "cin16_cout32_s8_relu_zp7": (16, 32, 8, 1, 3, 5, 1, 7, 3, 1),
    "cin48_cout96_s3_norelu_zp128": (48, 96, 3, 2, 5, 7, 0, 128, 255, 2),
    "cin16_cout96_s2_norelu_zp128": (16, 96, 2, 2, 9, 13, 0, 128, 0, 3),
    "cin48_cout32_s2_relu_zp7": (48, 32, 2, 2, 9, 13, 1, 7, 131, 4),
    "cin128_cout96_s2_relu_zp7": (128, 96, 2, 1, 9, 13, 1, 7, 3, 5),
    "cin64_cout32_s3_relu_zp0": (64, 32, 3, 1, 5, 7, 1, 0, 199, 6),
}
PIN_F32 = {
    "cin16_cout96_s3_norelu_zp128": (16, 96, 3, 2, 5, 7, 0, 128, 0, 7),
    "cin48_cout32_s8_relu_zp7": (48, 32, 8, 1, 3, 5, 1, 7, 0, 8),
    "cin128_cout96_s2_relu_zp7": (128, 96, 2, 1, 9, 13, 1, 7, 0, 9),
}


def _numpy_codes(xhat, wdeq, bias, s, relu, da, za):
    """(codes u8 [n, h s, w s, cout], mask of the elements within the fp32 chain's error bound of a rounding boundary)"""
    n, h, w, cin = xhat.shape
    cout = wdeq.shape[1]
    x64, w64 = xhat.astype(np.float64), wdeq.astype(np.float64)
    y = np.einsum("nhwc,coij->nhiwjo", x64, w64) + bias.astype(np.float64)
    mag = np.einsum("nhwc,coij->nhiwjo", np.abs(x64), np.abs(w64)) + np.abs(bias.astype(np.float64))
    y, mag = y.reshape(n, h * s, w * s, cout), mag.reshape(n, h * s, w * s, cout)
    da64 = float(np.float32(da))
    p = (np.maximum(y, 0.0) if relu else y) / da64 + float(za)
    # (fma(y, fl(1 / da), za) itself carries up to |p| 2^-23 = 3e-5 code units at p = 255, more than the 1e-6 allowed for it.  The chain term
    #  is what absorbs it: a worst-case bound, Cin + 2 >= 18 roundings of mag >= |y| where the chain's real error grows like sqrt(Cin), so it
    #  leaves more than |y / da| 2^-23 spare; only the rounding that za adds, at most 128 2^-24 = 8e-6, stands outside, and the guard below
    #  keeps the band at several times that: a new seed or step that shrinks it fails here, by name, and not with a stray code)
    band = (cin + 2) * 2.0 ** -24 * mag / da64 + 1e-6
    assert band.min() >= 2e-5, "the chain term no longer covers the quantizer's own fp32 rounding: choose a larger layer or step"
    near = np.abs(p - np.floor(p) - 0.5) <= band
    return np.clip(np.rint(p), 0, 255).astype(np.uint8), near


def _pin(name, p, f32in):
    cin, cout, s, n, h, w, relu, zp, zx, seed = p
    rng = np.random.default_rng(seed)
    da = out_step(1.0, zp, relu)
    if f32in:
        x = (rng.standard_normal((n, h, w, cin)) * X_STD_F32).astype(np.float32)
        wdeq, bias, _ = deblock_layer(rng, cin, cout, s, 1.0, X_STD_F32)
        xhat = x
    else:
        x = rng.integers(0, 256, size=(n, h, w, cin), dtype=np.uint8)
        wdeq, bias, _ = deblock_layer(rng, cin, cout, s)
        xhat = ((x.astype(np.int32) - zx).astype(np.float32) * np.float32(DX)).astype(np.float32)
    want, near = _numpy_codes(xhat, wdeq, bias, s, relu, da, zp)
    share = float(near.mean())
    print(f"{'f32' if f32in else 'i8 '} {name}: excluded share {100 * share:.2f} % of {near.size}")
    assert share <= CAP, f"{name}: {100 * share:.2f} % of the elements sit on a rounding boundary: pick another seed"
    norelu = _numpy_codes(xhat, wdeq, bias, s, 0, da, zp)[0] if relu and zp > 0 else None
    live(want, relu, zp, norelu)                                     # the pinned cases saturate like the GPU cases do
    got = oracle_codes(x, wdeq, bias, s, relu, da, zp, DX, zx)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[~near], want[~near])


@pytest.mark.parametrize("name", list(PIN_I8))
def test_orc_deconv_matches_numpy(name):
    _pin(name, PIN_I8[name], False)


@pytest.mark.parametrize("name", list(PIN_F32))
def test_orc_deconv_f32in_matches_numpy(name):
    _pin(name, PIN_F32[name], True)


# ---- the helpers on themselves -------------------------------------------------------------------------------------------------------------

def _codes(sigma, da, relu, zp, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(2, 5, 7, 64), dtype=np.uint8)
    wdeq, bias, _ = deblock_layer(rng, 64, 64, 2, sigma)
    return oracle_codes(x, wdeq, bias, 2, relu, da, zp, DX, 100)


def test_live_accepts_a_saturating_layer_and_rejects_a_tame_one():
    for relu, zp in [(1, 0), (1, 7), (0, 128)]:
        da = out_step(1.0, zp, relu)
        live(_codes(1.0, da, relu, zp), relu, zp, _codes(1.0, da, 0, zp) if relu and zp else None)
    # the generator of test_hip_deconv_batch.py: y of spread ~ 2.7 on a step of 0.047 never reaches 255 under ReLU ...
    tame = _codes(0.6 * 73.9 * DX, 0.047, 1, 2)
    assert (tame == 255).mean() < 0.005
    with pytest.raises(AssertionError, match="255"):
        live(tame, 1, 2, _codes(0.6 * 73.9 * DX, 0.047, 0, 2))
    # ... nor, without ReLU, the upper clamp
    with pytest.raises(AssertionError, match="no ReLU"):
        live(_codes(0.6 * 73.9 * DX, 0.047, 0, 2), 0, 2)
    with pytest.raises(AssertionError, match="without ReLU"):
        live(_codes(1.0, out_step(1.0, 7, 1), 1, 7), 1, 7)          # a ReLU case with zp > 0 must bring the codes without ReLU


@pytest.mark.parametrize("relu,zp,zx", QUANT_GRID)
@pytest.mark.parametrize("shape", ["ps", "wave"])
def test_quantizer_grid_is_sensitive_to_the_input_zero_point(shape, relu, zp, zx):
    """a condition on the inputs, on the oracle: one code of in_zx either way changes at least 10 % of a grid case's reference codes, so a
    kernel that ignored in_zx, was one off in it or wrapped at 255 cannot pass.  (One code moves y by 0.0034 sigma = 0.21 .. 0.43 output
    steps; under ReLU half the codes sit at the clamp and do not move: 0.21 x 0.95 at (0, 128), 0.32 x 0.5 at (1, 64).  Measured: 14 .. 21 %.)"""
    share = zx_sensitivity(Prepared(quant_case(shape, relu, zp, zx)))
    print(f"{shape} relu {relu} zp {zp} in_zx {zx}: in_zx +- 1 changes at least {100 * share:.1f} % of the reference codes")
    assert share >= 0.10


def test_table_cases_are_sensitive_to_the_input_zero_point():
    for name in ("straddle_np1", "cin_tails_wave", "four_layers_two_destinations", "mixed"):
        assert zx_sensitivity(Prepared(I8_CASES[name])) >= 0.10, name


def test_launch_rule_restatement_at_the_cases_of_the_gpu_file():
    """the forms and pairs per item the case table claims, and the rule's thresholds from both sides"""
    for case in list(I8_CASES.values()) + list(F32_CASES.values()) + [quant_case(sh, *q) for sh in ("ps", "wave") for q in QUANT_GRID]:
        assert_plan(case)
        for l in case.plan_layers():
            assert launch_plan("single", [l]) == ("wave32", None)
    ps = lambda *layers: launch_plan("batch", list(layers))
    # the 2560-item loop: 128 -> 96 s 2 has 6 pairs, so np = 2 at every cap >= 2 and 3 items per pixel tile; 853 tiles give 2559 items
    assert ps((128, 96, 2, 853 * 32)) == ("ps", [1]) and ps((128, 96, 2, 853 * 32 + 1)) == ("ps", [2])
    # 128 -> 128 s 3: 18 pairs, np <= 2; 284 tiles x 9 = 2556, 285 x 9 = 2565
    assert ps((128, 128, 3, 284 * 32)) == ("ps", [1]) and ps((128, 128, 3, 284 * 32 + 1)) == ("ps", [2])
    # 128 -> 32 s 2: 2 pairs, one item per pixel tile at np = 2
    assert ps((128, 32, 2, 2559 * 32)) == ("ps", [1]) and ps((128, 32, 2, 2559 * 32 + 1)) == ("ps", [2])
    # the workload's own batch: 8 pairs per item at Cin 128 | 256 from enough pixels on, Cin 64 (two pixel tiles, 2 pairs) keeps all its columns
    assert ps((64, 128, 1, 12 * 100 * 88), (128, 128, 2, 12 * 50 * 44), (256, 128, 4, 12 * 25 * 22)) == ("ps", [2, 8, 8])
    assert ps((64, 128, 1, 20 * 44), (128, 128, 2, 10 * 22), (256, 128, 4, 5 * 11)) == ("ps", [1, 1, 1])
    assert ps((64, 192, 1, 2 * 31 * 33)) == ("ps", [1])                                   # three pairs: no power of two divides them
    # Cin 32 | 96 are no pixel-stationary shapes; 16384 wave tiles from both sides (2 columns tiles x 8192 pixel tiles)
    assert ps((32, 64, 1, 8192 * 32 - 32)) == ("wave32", None) and ps((32, 64, 1, 8192 * 32 - 31)) == ("wave64", None)
    assert ps((96, 64, 2, 100), (64, 64, 2, 100)) == ("wave32", None)
    # the fp32-map entry: pixel-stationary only up to Cin 128
    assert launch_plan("f32in", [(64, 64, 1, 35)]) == ("ps", [1]) and launch_plan("f32in", [(128, 128, 2, 874)]) == ("ps", [1])
    assert launch_plan("f32in", [(256, 128, 4, 99)]) == ("wave32", None) and launch_plan("f32in", [(32, 64, 2, 81)]) == ("wave32", None)
    assert launch_plan("f32in", [(128, 128, 2, 32 * 2560)]) == ("ps", [8]) and launch_plan("f32in", [(128, 128, 2, 32 * 2559)]) == ("ps", [4])


# ---- argument rejects ----------------------------------------------------------------------------------------------------------------------

def _good_desc():
    from quantv2x_amd import lib
    d = lib.DeconvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.s, d.in_zx, d.in_delta = 1, 4, 4, 64, 64, 2, 0, 0.05
    d.out_ctotal, d.out_c0, d.relu, d.out_delta, d.out_zp, d.out_h, d.out_w = 96, 16, 1, 0.05, 0.0, 8, 8
    return d


REJECTS = [      # fields to change, return code, a piece of the message
    (dict(cin=24), -2, b"cin % 16"),
    (dict(cout=48, out_ctotal=96), -2, b"cout % 32"),
    (dict(s=1, cout=32, out_h=4, out_w=4), -2, b"s*s*cout % 64"),
    (dict(s=0, out_h=0, out_w=0), -1, b"bad shape"),
    (dict(s=9, out_h=36, out_w=36), -1, b"bad shape"),
    (dict(out_h=9), -1, b"destination is 9 x 8, this layer writes 8 x 8"),
    (dict(out_ctotal=64), -1, b"out channel window"),                # the window [16, 80) ends past 64 channels
    (dict(out_c0=8), -2, b"out_c0 % 16"),
    (dict(out_delta=0.0), -1, b"out_delta must be positive"),
]


def test_argument_errors_of_the_deblock_entries_without_gpu():
    """rejected calls only (an accepted one would launch): each reject of deconv_args through the three entries, the batch entry's own checks"""
    from quantv2x_amd import build, lib
    build.build()
    l = lib.load()
    raw = np.zeros(4096 + 16, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16                 # a 16-byte aligned host address: no kernel ever sees it
    p, vp = C.c_void_p(base), C.c_void_p
    entries = {"qv2x_deconv_i8": lambda d, i=p, w=p, b=p, o=p: l.qv2x_deconv_i8(C.byref(d), i, w, b, o, None),
               "qv2x_deconv_f32in": lambda d, i=p, w=p, b=p, o=p: l.qv2x_deconv_f32in(C.byref(d), i, w, b, o, None),
               "qv2x_deconv_i8_batch": lambda d, i=p, w=p, b=p, o=p: l.qv2x_deconv_i8_batch(C.byref(d), 1, (vp * 1)(i), (vp * 1)(w), (vp * 1)(b), (vp * 1)(o), None)}
    for who, call in entries.items():
        for change, rc, msg in REJECTS:
            d = _good_desc()
            for k, v in change.items():
                setattr(d, k, v)
            assert call(d) == rc, (who, change)
            err = l.qv2x_last_error()
            assert msg in err and who.encode() + b":" in err, (who, change, err)
        d = _good_desc()
        assert call(d, i=vp(base + 4)) == -2 and b"in / w must be 16-byte aligned" in l.qv2x_last_error(), who      # a misaligned `in`
        assert call(d, w=vp(base + 8)) == -2 and b"in / w must be 16-byte aligned" in l.qv2x_last_error(), who
        assert call(d, o=vp(base + 4)) == -2 and b"out / bias 16-byte aligned" in l.qv2x_last_error(), who
        assert call(d, b=vp(None)) == -1 and who.encode() + b": null pointer" in l.qv2x_last_error(), who
    # the batch entry: 1 .. 4 layers, no null array; a bad layer behind a good one is found
    descs = (lib.DeconvDesc * 5)(*[_good_desc() for _ in range(5)])
    arr = (vp * 5)(*[base] * 5)
    for n in (0, 5, -1):
        assert l.qv2x_deconv_i8_batch(descs, n, arr, arr, arr, arr, None) == -1 and b"qv2x_deconv_i8_batch: 1..4 layers" in l.qv2x_last_error(), n
    for hole in range(4):
        args = [arr] * 4
        args[hole] = None
        assert l.qv2x_deconv_i8_batch(descs, 2, *args, None) == -1 and b"qv2x_deconv_i8_batch: null pointer" in l.qv2x_last_error(), hole
    assert l.qv2x_deconv_i8_batch(None, 2, arr, arr, arr, arr, None) == -1 and b"null pointer" in l.qv2x_last_error()
    descs[1].cin = 24
    assert l.qv2x_deconv_i8_batch(descs, 2, arr, arr, arr, arr, None) == -2 and b"qv2x_deconv_i8_batch: cin % 16" in l.qv2x_last_error()
    assert l.qv2x_deconv_i8(None, p, p, p, p, None) == -1 and b"qv2x_deconv_i8: null pointer" in l.qv2x_last_error()
