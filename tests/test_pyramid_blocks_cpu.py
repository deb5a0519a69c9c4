"""``orc_convg`` and ``orc_add_relu_quant`` -- the reference of tests/test_hip_pyramid_blocks.py -- pinned once against plain numpy at shapes
the golden vectors do not hold: grouped layers whose channel count is no multiple of 128, stride 2 on odd maps, no ReLU, the fp32 output,
a non-zero block zero point.

numpy side:  T in int64 over an explicitly zero-padded (x - zx);  y = bias + float32(T) * scale in float32;  code = clip(rint(float64(y) / da
+ za), 0, 255).  The oracle multiplies by fl(1 / da) in one fp32 fma (its documented restatement of the division), so a code may differ where
float64(y) / da + za lies within 1e-3 of a half-integer: those elements are excluded, and they may be at most 0.1 % of a case."""
import numpy as np
import pytest

from _pyramid_layers import block_quantizer, conv1x1_state, f32_variant, gconv_state, uniform_stats

DX, ZX = np.float32(0.05), 7


def _oracle(state):
    from oracle.spec_pyramid import OraclePyramid
    orc = OraclePyramid.__new__(OraclePyramid)
    orc.s = state
    return orc


def _np_conv_y(state, name, x, xq, stride):
    """y f32 [N,Ho,Wo,Cout] = bias + float32(T) * scale, T exact in int64"""
    code = state[name + "/w_code"].astype(np.int64)
    cout, cg, k = code.shape[0], code.shape[1], code.shape[2]
    n, h, w, cin = x.shape
    groups, pad = cin // cg, k // 2
    og = cout // groups
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, cin), np.int64)
    xp[:, pad:pad + h, pad:pad + w] = x.astype(np.int64) - int(xq[1])
    wz = (code - state[name + "/w_zp"].astype(np.int64).reshape(-1, 1, 1, 1)).reshape(groups, og, cg, k, k)
    T = np.zeros((n, ho, wo, groups, og), np.int64)
    for i in range(k):
        for j in range(k):
            win = xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride].reshape(n, ho, wo, groups, cg)
            T += np.einsum("nhwgc,goc->nhwgo", win, wz[:, :, :, i, j])
    T = T.reshape(n, ho, wo, cout)
    assert np.abs(T).max() < 2 ** 24                     # float32(T) is exact
    scale = (np.float32(xq[0]) * state[name + "/w_delta"].astype(np.float32)).astype(np.float32)
    return (state[name + "/bias"].astype(np.float32) + T.astype(np.float32) * scale).astype(np.float32)


def _np_codes(y, da, za):
    """codes and the mask of elements whose pre-rounding value is within 1e-3 of a half-integer"""
    p = y.astype(np.float64) / float(da) + float(za)
    near = np.abs(p - np.floor(p) - 0.5) < 1e-3
    return np.clip(np.rint(p), 0, 255).astype(np.uint8), near


def _compare(got, want, near):
    assert near.mean() <= 1e-3, f"{near.sum()} of {near.size} elements sit on a rounding boundary: pick another seed"
    np.testing.assert_array_equal(got[~near], want[~near])


# seeds: the first for which the numpy side alone keeps the excluded share under its cap (about 0.2 % of the unsaturated elements
# fall inside the 1e-3 band, so roughly every third seed does)
CASES = {
    "grouped_c96_cg4_s2_odd": dict(kind="g", c=96, cg=4, stride=2, n=1, h=7, w=37, relu=True, a_zp=3, seed=6),
    "grouped_c128_cg16_s1": dict(kind="g", c=128, cg=16, stride=1, n=2, h=5, w=9, relu=True, a_zp=0, seed=10),
    "1x1_s2_odd_norelu": dict(kind="1", c=64, cout=64, stride=2, n=1, h=9, w=13, relu=False, a_zp=120, seed=7),
}


@pytest.mark.parametrize("case", list(CASES))
def test_convg_codes_match_numpy(case):
    p = CASES[case]
    rng = np.random.default_rng(p["seed"])
    xq = (DX, ZX)
    if p["kind"] == "g":
        state = gconv_state(rng, "l", p["c"], p["cg"], xq, uniform_stats(ZX), p["a_zp"], relu=p["relu"])
    else:
        state = conv1x1_state(rng, "l", p["c"], p["cout"], xq, uniform_stats(ZX), p["a_zp"], relu=p["relu"])
    x = rng.integers(0, 256, size=(p["n"], p["h"], p["w"], p["c"]), dtype=np.uint8)
    got, oq = _oracle(state).convg("l", x, xq, stride=p["stride"], relu=p["relu"])
    y = _np_conv_y(state, "l", x, xq, p["stride"])
    assert got.shape == y.shape and got.shape[1:3] == ((p["h"] - 1) // p["stride"] + 1, (p["w"] - 1) // p["stride"] + 1)
    want, near = _np_codes(np.maximum(y, 0) if p["relu"] else y, *oq)
    lowest = p["a_zp"] if p["relu"] else 0
    assert ((want > lowest) & (want < 255)).mean() >= 1 / 3
    _compare(got, want, near)


def test_convg_f32_output_matches_numpy():
    rng = np.random.default_rng(5)
    xq = (DX, ZX)
    state = f32_variant(conv1x1_state(rng, "l", 128, 64, xq, uniform_stats(ZX), 0), "l", "l_f32")
    x = rng.integers(0, 256, size=(2, 5, 7, 128), dtype=np.uint8)
    got = _oracle(state).convg("l_f32", x, xq, f32_out=True)
    np.testing.assert_array_equal(got, _np_conv_y(state, "l_f32", x, xq, 1))         # the same two fp32 roundings: bit for bit


def test_finish_matches_numpy_with_a_block_zero_point():
    rng = np.random.default_rng(29)
    xq = (DX, ZX)
    sigma = 73.9 * float(DX)
    state = block_quantizer("b", xq, uniform_stats(ZX), sigma, 5)
    orc = _oracle(state)
    r = rng.integers(0, 256, size=(2, 6, 9, 64), dtype=np.uint8)
    res = orc.dequant(r, xq)
    np.testing.assert_array_equal(res, ((r.astype(np.int64) - ZX).astype(np.float32) * DX).astype(np.float32))
    y = rng.normal(0.3 * sigma, sigma, size=r.shape).astype(np.float32)
    got, oq = orc.finish("b", y, res)
    assert oq == (state["b/a_delta"], 5)
    want, near = _np_codes(np.maximum((y + res).astype(np.float32), 0), *oq)
    assert ((want > 5) & (want < 255)).mean() >= 1 / 3
    _compare(got, want, near)
