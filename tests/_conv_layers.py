"""Random 3x3 QuantModule layers for csrc/conv_i8.hip, conv_i8_wide.hip, conv_i8_ws.hip, conv_i8_ws2.hip and conv_i8_chain.hip, their launches
through the three entries and their references (no tests here).

Used by tests/test_hip_conv_layers.py (GPU) and tests/test_conv_layers_cpu.py (no GPU).

**Layers.**  ``conv_layer`` draws one layer over input groups ``[(c0, c, zx)]`` that lie ANYWHERE inside a tensor of ``cin_total`` channels:
out of channel order, with gaps, with spare channels in front and behind.  The weight tensor is the oracle's ``[cout][cin_total][3][3]`` over
absolute channels (engine._ConvLayer slices it by c0); weight codes are uniform on 0..255 and ``zw`` is drawn per output channel from the
WHOLE range 0..255, so rms(w - zw) = sqrt(73.9^2 + (127.5 - zw)^2) differs per channel and the weight step is set per channel:
dw[co] rms(w - zw[co]) = W_DELTA u[co], u in [0.85, 1.15).  Every group contributes sigma / sqrt(G):

    std(T_g) = x_std sqrt(9 c_g) rms(w - zw)    (the weights are fixed, the codes vary)      dx_g = sigma / (sqrt(G) x_std sqrt(9 c_g) W_DELTA)

so std(y[co]) = u[co] sigma and every group moves codes.  The bias takes out the per-channel offset  sum_g mean(x - zx_g) sum(w - zw) scale_g
(up to 35 sigma at zx = 3, zw = 0) and adds N(0, ``bias_spread`` sigma), 0.3 sigma as a rule.  That offset is exact only where all nine taps lie inside the map:
an edge pixel loses a third of it, a corner five ninths.  The random cases therefore keep zx within +-40 of the middle (ZX), the 2 x 3 and
3 x 5 images -- all edge -- within +-23 (ZX_TINY): the shift stays below about 2.6 sigma for the worst channel and acts as spread.  128 - zx
and 128 - zw are never 0: both correction terms matter, which ``zx_sensitivity`` states on the oracle.  Codes and zero points of 0 and 255
are the extremes case's (``extreme_layer``).  ``out_step`` (from _deblock_layers) puts 2 sigma at the nearer reachable end of the code range.
For an off-centre two-sided quantizer (no ReLU, zp 64 or 99) the far end lies 6 or 3.2 sigma out: such layers draw the bias with a spread of
2.5 or 1.0 sigma (``bias_spread``), so that channels sit near either end and both clamps decide codes.

**live(want, relu, zp)** (from _deblock_layers) is asserted ON THE ORACLE'S OUTPUT in ``Prepared`` before any kernel result is looked at.

**launch_plan(entry, desc)** restates the host launch rules of conv3x3_entry, qv2x_conv3x3_i8_wide (ws64_takes, ws2_takes, wide_bn, the
grid of persistent workgroups) and the chain entry in plain Python.  Every GPU case names the form it was written for and asserts it
through this function, the persistent ones also the items per workgroup: after a change of a rule the case list fails instead of silently
aiming at something else.

**Destinations** are [n][Ho + 2][Wo + 2][FRONT + cout + BACK] int8 maps allocated full of SENT with out_c0 = FRONT; ``check_outputs`` compares
the window with the oracle bit for bit and requires SENT everywhere else.  The chain entry has no window: only its pad ring holds SENT.
Input channels outside the groups hold random codes, border included (a hostile fill): neither the oracle nor a kernel may read them.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from _deblock_layers import BACK, CODE_STD, FRONT, SENT, live, out_step, padded
from _pyramid_layers import uniform_stats

W_DELTA = 0.004                     # dw[co] * rms(w - zw[co]), before the per-channel factor u
ZX = (101, 160, 88, 167)            # input zero points of the random cases, by group
ZX_TINY = (117, 140, 109, 150)      # ... of the cases whose images are all edge
VARIANTS = ((1, 7), (0, 120))       # (relu, out_zp): every case runs under both unless it is marked single
EXTRA_VARIANTS = ((1, 0), (0, 64))  # a few small cases also run these


def out_hw(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


# ---- layers ----------------------------------------------------------------------------------------------------------------------------

class Layer:
    """one QuantModule 3x3 layer: groups [(c0, c, dx, zx)], code u8 [cout][cin_total][3][3], zw / dw / bias [cout], (relu, da, zp)"""

    def __init__(self, groups, cin_total, stride, code, zw, dw, bias, relu, da, zp):
        self.groups, self.cin_total, self.stride, self.cout = [tuple(g) for g in groups], cin_total, stride, code.shape[0]
        self.code, self.zw, self.dw, self.bias = code, np.asarray(zw, np.int64), np.asarray(dw, np.float32), np.asarray(bias, np.float32)
        self.relu, self.da, self.zp = int(relu), float(np.float32(da)), int(zp)

    def scale(self):
        """f32 [G][cout] = dx_g * dw[co], the fp32 product the engine's packer makes"""
        return np.stack([np.float32(dx) * self.dw for (_, _, dx, _) in self.groups]).astype(np.float32)

    def state(self, name="layer"):
        """the ptq_state keys engine._ConvLayer reads"""
        return {name + "/w_code": self.code, name + "/w_delta": self.dw, name + "/w_zp": self.zw.astype(np.float32), name + "/bias": self.bias,
                name + "/a_delta": np.float32(self.da), name + "/a_zp": np.float32(self.zp), name + "/a_off": np.bool_(False)}


def bias_spread(relu, zp):
    """the spread of the bias's random part in units of sigma: 0.3, or what puts the FAR end of a two-sided quantizer's code range at 2.2
    spreads of y over all channels, sqrt(1 + spread^2) sigma, where out_step leaves it more than 2.45 sigma out (zp 64: 5.97, zp 99: 3.15)"""
    far = 0.0 if relu else 2.0 * max(zp, 255.0 - zp) / min(zp, 255.0 - zp)
    return 0.3 if far <= 2.45 else float(np.sqrt((far / 2.2) ** 2 - 1.0))


def conv_layer(rng, groups, cin_total, cout, stride, relu, zp, sigma=1.0, x_stats=None, zw_range=(0, 256)):
    """groups: [(c0, c, zx)]; x_stats: per group (mean, std) of the input CODES (default: uniform on 0..255).  std(y) ~ sigma."""
    G = len(groups)
    code = rng.integers(0, 256, size=(cout, cin_total, 3, 3), dtype=np.uint8)
    zw = rng.integers(zw_range[0], zw_range[1], size=cout)
    w_rms = np.sqrt(CODE_STD ** 2 + (127.5 - zw) ** 2)
    dw = (W_DELTA * rng.uniform(0.85, 1.15, size=cout) / w_rms).astype(np.float32)
    in_groups, offset = [], np.zeros(cout)
    for g, (c0, c, zx) in enumerate(groups):
        mean_x, std_x = x_stats[g] if x_stats is not None else (uniform_stats(zx)[0] + zx, CODE_STD)
        dx = np.float32(sigma / (np.sqrt(G) * std_x * np.sqrt(9.0 * c) * W_DELTA))
        wsum = (code[:, c0:c0 + c].astype(np.float64) - zw[:, None, None, None]).sum(axis=(1, 2, 3))
        offset += (mean_x - zx) * wsum * (dx * dw).astype(np.float64)
        in_groups.append((c0, c, dx, int(zx)))
    bias = (rng.normal(0.0, bias_spread(relu, zp) * sigma, size=cout) - offset).astype(np.float32)
    return Layer(in_groups, cin_total, stride, code, zw, dw, bias, relu, out_step(sigma, zp, relu), zp)


def hostile_input(rng, n, h, w, cin_total):
    """codes uniform on 0..255 in EVERY channel: the groups' operands and, outside them, bytes nobody may read"""
    return rng.integers(0, 256, size=(n, h, w, cin_total), dtype=np.uint8)


def padded_input(rng, x, layer):
    """padded i8 [n][h + 2][w + 2][cin_total]: each group's border holds its pad code zx_g, everything outside the groups stays random"""
    n, h, w, ct = x.shape
    p = rng.integers(-128, 128, size=(n, h + 2, w + 2, ct), dtype=np.int8)
    p[:, 1:-1, 1:-1] = (x.astype(np.int16) - 128).astype(np.int8)
    for (c0, c, _, zx) in layer.groups:
        p[..., c0:c0 + c] = padded(x[..., c0:c0 + c], zx)
    return p


# ---- references ------------------------------------------------------------------------------------------------------------------------

def oracle_conv(layer, x, relu=None, zx=None, out_ct=None, out_c0=0, fill=0):
    """u8 [n][ho][wo][out_ct] of orc_conv3x3 written at out_c0 into an array full of ``fill`` (Oracle.conv hard-codes relu = 1 and has no
    window); ``relu`` / ``zx`` override the layer's"""
    from oracle.spec import _cf, _f32, _i32, _p, lib as olib
    n, h, w, ct = x.shape
    assert ct == layer.cin_total and x.dtype == np.uint8
    ho, wo = out_hw(h, w, layer.stride)
    out_ct = layer.cout if out_ct is None else out_ct
    out = np.full((n, ho, wo, out_ct), fill, np.uint8)
    zxs = [g[3] for g in layer.groups] if zx is None else list(zx)
    olib().orc_conv3x3(_p(np.ascontiguousarray(x)), n, h, w, ct, layer.stride, len(layer.groups), _p(_i32([g[0] for g in layer.groups])),
                       _p(_i32([g[1] for g in layer.groups])), _p(_i32(zxs)), _p(np.ascontiguousarray(layer.code)), _p(_i32(layer.zw)), layer.cout,
                       _p(layer.scale()), _p(_f32(layer.bias)), int(layer.relu if relu is None else relu), _cf(layer.da), _cf(layer.zp), _p(out),
                       out_ct, out_c0)
    return out


def window_sums(x, layer, g):
    """(T_g, window sum of xs = code - 128 over the taps, pad ring included) of group g as exact int64 [n][ho][wo][cout] / [n][ho][wo]:
    float64 matrix products of integers whose sums stay below 2^53"""
    c0, c, _, zx = layer.groups[g]
    n, h, w, _ = x.shape
    ho, wo = out_hw(h, w, layer.stride)
    s = layer.stride
    xp = np.zeros((n, h + 2, w + 2, c))
    xp[:, 1:-1, 1:-1] = x[..., c0:c0 + c].astype(np.float64) - zx
    T, xs = np.zeros((n, ho, wo, layer.cout)), np.zeros((n, ho, wo))
    wc = layer.code[:, c0:c0 + c].astype(np.float64) - layer.zw[:, None, None, None].astype(np.float64)
    for kh in range(3):
        for kw in range(3):
            win = xp[:, kh:kh + (ho - 1) * s + 1:s, kw:kw + (wo - 1) * s + 1:s]
            T += win @ wc[:, :, kh, kw].T
            xs += (win + (zx - 128)).sum(axis=-1)                 # the kernels sum the stored bytes: the ring holds zx - 128
    assert np.abs(T).max() < 2.0 ** 53
    return T.astype(np.int64), xs.astype(np.int64)


def float64_codes(layer, x):
    """(codes u8 [n][ho][wo][cout], mask of the positions within the fp32 evaluation's error bound of a rounding boundary): exact integer T_g,
    then y and the quantizer in float64.  The bound, in code units:  (G + 3) 2^-24 (|bias| + sum_g |T_g scale_g|) / delta  -- one rounding
    per int-to-float conversion, product and sum of the oracle's chain plus the fma -- and 1.2e-7 |y / delta| for the multiplication by
    fl(1 / delta) instead of the division (csrc/common.h)."""
    sc = layer.scale().astype(np.float64)
    ts = [window_sums(x, layer, g)[0] * sc[g] for g in range(len(layer.groups))]
    y = np.broadcast_to(layer.bias.astype(np.float64), ts[0].shape).copy()
    mag = np.abs(y)
    for t in ts:
        y += t
        mag += np.abs(t)
    if layer.relu:
        y = np.maximum(y, 0.0)
    p = y / layer.da + layer.zp
    tol = (len(layer.groups) + 3) * 2.0 ** -24 * mag / layer.da + 1.2e-7 * np.abs(y / layer.da)
    near = np.abs(p - np.floor(p) - 0.5) <= tol
    return np.clip(np.rint(p), 0, 255).astype(np.uint8), near


def zx_sensitivity(layer, x, want):
    """the smallest share of the ORACLE's codes that one group's zx + 1 or zx - 1 changes (the oracle takes any integer zero point)"""
    worst = 1.0
    for g in range(len(layer.groups)):
        for step in (-1, 1):
            zx = [q[3] + (step if i == g else 0) for i, q in enumerate(layer.groups)]
            worst = min(worst, float((oracle_conv(layer, x, zx=zx) != want).mean()))
    return worst


# ---- the host launch rules, restated -----------------------------------------------------------------------------------------------------

Plan = namedtuple("Plan", "form grid items most least", defaults=(None, None, None, None))
MAX_CHUNKS = 24


def _cdiv(a, b):
    return -(-a // b)


def _patches(n, ho, wo, th, tw=32):
    return n * _cdiv(ho, th) * _cdiv(wo, tw)


def launch_plan(entry, d, res_mode=0):
    """entry "regular" (qv2x_conv3x3_i8; res_mode != 0: qv2x_conv3x3_i8_res) | "wide" (qv2x_conv3x3_i8_wide) with d = anything that has
    n, h, w, stride, cout and groups [(c0, c, ...)];  "chain" with d = (n, in_h, in_w, depth, stride0).
    regular: Plan(form) with form in res | multi | large | k256 | m192 | k128 | k64, in the order conv3x3_entry tests them.
    wide: Plan(form, grid, items, most, least): ws64 | ws2_2x2 | ws2_4x1 | [s2_ | multi_]bn64 | bn128 | bn256, the grid of persistent
    workgroups and the largest and smallest number of items one of them takes (padded items included).
    chain: Plan(("chain", depth, stride0), grid = items = patches of 5 x 32)."""
    if entry == "chain":
        n, in_h, in_w, depth, stride0 = d
        h, w = out_hw(in_h, in_w, stride0)
        p = _patches(n, h, w, 5)
        return Plan(("chain", depth, stride0), p, p, 1, 1)
    gc = [g[1] for g in d.groups]
    ho, wo = out_hw(d.h, d.w, d.stride)
    M, multi = d.n * ho * wo, len(gc) > 1
    if entry == "regular":
        if res_mode:
            return Plan("res")
        if multi:
            assert d.cout % 128 == 0
            return Plan("multi")
        if d.cout % 128 == 0 and M >= 16384:
            return Plan("large")
        wgs64 = _cdiv(M, 64) * (d.cout // 64)
        if gc[0] % 256 == 0 and wgs64 <= 256:
            return Plan("k256")
        k128 = all(c % 128 == 0 for c in gc)
        if not k128 and d.cout == 64 and M >= 262144:
            return Plan("m192")
        return Plan("k128" if k128 else "k64")
    assert entry == "wide" and d.stride in (1, 2) and (d.cout in (64, 128) or d.cout % 256 == 0)
    assert not multi or (d.stride == 1 and d.cout >= 256)
    persistent = lambda form, items, slots: Plan(form, min(items, slots), items, _cdiv(items, min(items, slots)), items // min(items, slots))
    if d.stride == 1 and not multi and gc[0] == 64 and d.cout == 64 and _patches(d.n, ho, wo, 10) >= 1024:
        return persistent("ws64", _patches(d.n, ho, wo, 10), 512)
    if d.stride == 2 and not multi and gc[0] == 64 and d.cout in (64, 128) and _patches(d.n, ho, wo, 8) >= 1024:
        return persistent("ws2_2x2" if d.cout == 64 else "ws2_4x1", _patches(d.n, ho, wo, 8), 512)
    patches = _patches(d.n, ho, wo, 5)
    bn = d.cout if d.cout % 256 else (256 if patches * (d.cout // 256) >= 192 else 128)
    items = _cdiv(patches, 8) * 8 * (d.cout // bn)
    period = 8 * (d.cout // bn)
    per_cu = 1 if bn == 256 else ((1 if multi else 2) if bn == 128 else (3 if d.stride == 2 else 4))
    slots = 256 * per_cu // period * period
    assert sum(gc) // 64 * (4 if d.stride == 2 else 1) <= MAX_CHUNKS
    return persistent(("s2_" if d.stride == 2 else "multi_" if multi else "") + f"bn{bn}", items, slots)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

class Case:
    """one layer shape: (n, h, w) of the input, groups [(c0, c)] inside cin_total, the form launch_plan must name for ``entry`` and, for the
    persistent forms, (grid, most, least items per workgroup).  variants: the (relu, out_zp) pairs it runs under."""

    def __init__(self, entry, form, shape, stride, groups, cout, cin_total=None, variants=VARIANTS, per_wg=None, seed=0, zx=None):
        self.entry, self.form, (self.n, self.h, self.w), self.stride, self.cout = entry, form, shape, stride, cout
        self.groups = [tuple(g) for g in groups]
        self.cin_total = cin_total if cin_total is not None else max(c0 + c for c0, c in self.groups)
        self.variants, self.per_wg, self.seed = tuple(variants), per_wg, seed
        self.zx = zx if zx is not None else (ZX_TINY if self.h * self.w < 64 else ZX)

    def assert_plan(self):
        plan = launch_plan(self.entry, self)
        assert plan.form == self.form, f"the launch rule changed: {plan}"
        if self.per_wg is not None:
            assert (plan.grid, plan.most, plan.least) == self.per_wg, f"the launch rule changed: {plan}"


R1, R0 = (VARIANTS[0],), (VARIANTS[1],)            # the single variants: they alternate down each list

REGULAR_CASES = {
    "k64_less_than_a_tile": Case("regular", "k64", (1, 3, 4), 1, [(0, 64)], 64, seed=1),                          # M = 12
    "k64_ragged_spare_channels": Case("regular", "k64", (2, 13, 37), 1, [(64, 64)], 64, cin_total=192, seed=2),     # M = 962
    "k64_stride2_odd_input": Case("regular", "k64", (1, 9, 61), 2, [(0, 64)], 64, seed=3),                        # 5 x 31 outputs
    "k64_cout192": Case("regular", "k64", (1, 6, 33), 1, [(0, 192)], 192, seed=4),          # three column blocks, three chunks per tap
    "k128_cout128": Case("regular", "k128", (2, 13, 37), 1, [(0, 128)], 128, seed=5),
    "k128_cout64": Case("regular", "k128", (2, 13, 37), 1, [(0, 128)], 64, seed=6),
    "k128_stride2": Case("regular", "k128", (1, 20, 130), 2, [(0, 128)], 256, seed=7),
    "k256": Case("regular", "k256", (1, 13, 37), 1, [(0, 256)], 256, seed=8),
    "k256_wgs64_256": Case("regular", "k256", (1, 64, 64), 1, [(0, 256)], 256, variants=R1, seed=9),               # wgs64 = 64 x 4
    "k128_wgs64_260": Case("regular", "k128", (1, 64, 65), 1, [(0, 256)], 256, variants=R0, seed=10),              # wgs64 = 65 x 4
    "large_ragged_last_tile": Case("regular", "large", (1, 127, 130), 1, [(0, 64)], 128, seed=11),               # M = 16510
    "large_tiles_straddle_images": Case("regular", "large", (3, 74, 75), 1, [(0, 128)], 256, seed=12),           # M = 16650
    "large_stride2": Case("regular", "large", (1, 255, 259), 2, [(0, 64)], 128, seed=13),                        # 128 x 130 outputs
    "k64_just_below_large": Case("regular", "k64", (1, 127, 129), 1, [(0, 64)], 128, variants=R1, seed=14),      # M = 16383
    "m192_stride2": Case("regular", "m192", (4, 512, 514), 2, [(0, 64)], 64, variants=R0, seed=15),              # M = 4 x 256 x 257 = 263168
    "m192": Case("regular", "m192", (8, 128, 257), 1, [(0, 64)], 64, variants=R1, seed=16),                      # M = 263168 = 1370 x 192 + 128
    "multi_out_of_order_gaps": Case("regular", "multi", (2, 13, 37), 1, [(128, 64), (0, 64)], 128, cin_total=256, seed=17),
    "multi_four_groups": Case("regular", "multi", (1, 5, 32), 1, [(0, 64), (64, 128), (192, 192), (384, 64)], 256, cin_total=448, seed=18),
    "multi_three_groups_gap": Case("regular", "multi", (1, 7, 40), 1, [(0, 64), (192, 64), (64, 64)], 128, cin_total=256, seed=20),
    "multi_stride2": Case("regular", "multi", (1, 9, 61), 2, [(64, 64), (192, 128)], 128, cin_total=320, seed=19),
}

WS_G, WS_CT = [(64, 64)], 128                       # the weights-stationary cases: cin_off = 64 in a tensor of 128 channels

WIDE_CASES = {
    "bn64_spare_channels": Case("wide", "bn64", (2, 13, 37), 1, [(64, 64)], 64, cin_total=192, per_wg=(16, 1, 1), seed=31),
    # 1100 patches pad to 1104 items on 1024 slots: 80 workgroups take two items, the last four items are padding
    "bn64_one_or_two_items": Case("wide", "bn64", (1100, 2, 3), 1, [(0, 128)], 64, per_wg=(1024, 2, 1), seed=32),
    "bn128": Case("wide", "bn128", (2, 13, 37), 1, [(0, 64)], 128, per_wg=(16, 1, 1), seed=33),
    "bn128_persistent": Case("wide", "bn128", (520, 2, 3), 1, [(0, 192)], 128, per_wg=(512, 2, 1), seed=34),
    "bn128_few_patches_cout256": Case("wide", "bn128", (1, 6, 33), 1, [(0, 192)], 256, per_wg=(16, 1, 1), seed=35),
    "bn256_one_item_each": Case("wide", "bn256", (200, 2, 3), 1, [(0, 64)], 256, per_wg=(200, 1, 1), seed=36),
    "bn256_padded_items": Case("wide", "bn256", (297, 2, 3), 1, [(0, 64)], 256, per_wg=(256, 2, 1), seed=37),          # 304 items, 7 of them padding
    "bn256_at_192": Case("wide", "bn256", (96, 2, 3), 1, [(0, 64)], 512, per_wg=(192, 1, 1), seed=38),                        # 96 x 2 = 192
    "bn128_at_190": Case("wide", "bn128", (95, 2, 3), 1, [(0, 64)], 512, per_wg=(384, 1, 1), seed=39),                        # 95 x 2 = 190
    "multi_bn128_out_of_order_gap": Case("wide", "multi_bn128", (1, 5, 32), 1, [(128, 64), (0, 64)], 256, cin_total=256, per_wg=(16, 1, 1), seed=40),
    "multi_bn256_three_groups": Case("wide", "multi_bn256", (192, 2, 3), 1, [(0, 64), (128, 128), (64, 64)], 256, per_wg=(192, 1, 1), seed=41),
    "s2_bn256": Case("wide", "s2_bn256", (200, 3, 5), 2, [(0, 64)], 256, per_wg=(200, 1, 1), seed=42),
    "s2_bn128": Case("wide", "s2_bn128", (2, 27, 75), 2, [(0, 128)], 128, per_wg=(16, 1, 1), seed=43),
    "s2_bn64_spare_channels": Case("wide", "s2_bn64", (2, 27, 75), 2, [(64, 64)], 64, cin_total=192, per_wg=(16, 1, 1), seed=44),
    "s2_max_chunks": Case("wide", "s2_bn128", (1, 10, 64), 2, [(0, 384)], 256, per_wg=(16, 1, 1), seed=45),
    "ws64_two_items_each": Case("wide", "ws64", (1024, 2, 3), 1, WS_G, 64, cin_total=WS_CT, per_wg=(512, 2, 2), seed=46),
    "ws64_two_or_three_items": Case("wide", "ws64", (1300, 2, 3), 1, WS_G, 64, cin_total=WS_CT, per_wg=(512, 3, 2), seed=47),
    # 2 x 2 patches of 10 x 32 per image: one row and one column reach into the second patch
    "ws64_ragged_second_patch": Case("wide", "ws64", (257, 11, 33), 1, WS_G, 64, cin_total=WS_CT, per_wg=(512, 3, 2), seed=48),
    "bn64_below_ws64": Case("wide", "bn64", (1023, 2, 3), 1, WS_G, 64, cin_total=WS_CT, variants=R1, per_wg=(1024, 1, 1), seed=49),
    "ws2_2x2": Case("wide", "ws2_2x2", (1024, 3, 5), 2, WS_G, 64, cin_total=WS_CT, per_wg=(512, 2, 2), seed=50),
    "ws2_4x1": Case("wide", "ws2_4x1", (1024, 3, 5), 2, WS_G, 128, cin_total=WS_CT, per_wg=(512, 2, 2), seed=51),
    "ws2_2x2_ragged": Case("wide", "ws2_2x2", (257, 18, 66), 2, WS_G, 64, cin_total=WS_CT, per_wg=(512, 3, 2), seed=52),        # 9 x 33 outputs
    "ws2_4x1_ragged": Case("wide", "ws2_4x1", (257, 18, 66), 2, WS_G, 128, cin_total=WS_CT, per_wg=(512, 3, 2), seed=53),
    # 64 output columns: input column 64 of a tile is interior in tile 0 and the right pad in tile 1
    "ws2_2x2_extra_column": Case("wide", "ws2_2x2", (512, 2, 128), 2, WS_G, 64, cin_total=WS_CT, per_wg=(512, 2, 2), seed=54),
    "ws2_4x1_extra_column": Case("wide", "ws2_4x1", (512, 2, 128), 2, WS_G, 128, cin_total=WS_CT, per_wg=(512, 2, 2), seed=55),
}

# the small cases that also run (relu 1, zp 0) and (relu 0, zp 64)
EXTRA_CASES = {
    "k64_stride2_odd_input": REGULAR_CASES["k64_stride2_odd_input"], "k128_cout64": REGULAR_CASES["k128_cout64"],
    "multi_out_of_order_gaps": REGULAR_CASES["multi_out_of_order_gaps"], "bn128": WIDE_CASES["bn128"], "s2_bn64_spare_channels": WIDE_CASES["s2_bn64_spare_channels"],
}


def expect_from(want, window=True):
    """the expected bytes of a whole destination: the oracle's codes ``want`` (u8 [n][ho][wo][cout]) minus 128 in the interior of the window,
    SENT in the pad ring and (``window``) in FRONT spare channels in front and BACK behind"""
    n, ho, wo, cout = want.shape
    front, back = (FRONT, BACK) if window else (0, 0)
    expect = np.full((n, ho + 2, wo + 2, front + cout + back), SENT, np.int8)
    expect[:, 1:-1, 1:-1, front:front + cout] = (want.astype(np.int16) - 128).astype(np.int8)
    return expect


class Prepared:
    """a Case under one (relu, zp): the layer, the input codes, the oracle's window and the expected bytes of the whole destination; ``live``
    asserted on the oracle's codes"""

    def __init__(self, case, variant, check_live=True):
        self.case, (relu, zp) = case, variant
        rng = np.random.default_rng(2000 + case.seed)
        groups = [(c0, c, case.zx[g]) for g, (c0, c) in enumerate(case.groups)]
        self.layer = conv_layer(rng, groups, case.cin_total, case.cout, case.stride, relu, zp)
        self.x = hostile_input(rng, case.n, case.h, case.w, case.cin_total)
        self.rng = rng
        ct = FRONT + case.cout + BACK
        win = oracle_conv(self.layer, self.x, out_ct=ct, out_c0=FRONT, fill=SENT + 128)
        self.want = win[..., FRONT:FRONT + case.cout]
        if check_live:
            norelu = oracle_conv(self.layer, self.x, relu=0) if relu and zp > 0 else None
            live(self.want, relu, zp, norelu)
        n, ho, wo, _ = win.shape
        self.expect = np.full((n, ho + 2, wo + 2, ct), SENT, np.int8)
        self.expect[:, 1:-1, 1:-1] = (win.astype(np.int16) - 128).astype(np.int8)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------

class ChainCase:
    def __init__(self, shape, depth, stride0, relu, zps, seed, zw_range=(0, 256)):
        (self.n, self.in_h, self.in_w), self.depth, self.stride0, self.relu, self.zps, self.seed = shape, depth, stride0, relu, zps, seed
        self.zw_range = zw_range

    def assert_plan(self):
        h, w = out_hw(self.in_h, self.in_w, self.stride0)
        plan = launch_plan("chain", (self.n, self.in_h, self.in_w, self.depth, self.stride0))
        assert plan == Plan(("chain", self.depth, self.stride0), _patches(self.n, h, w, 5), _patches(self.n, h, w, 5), 1, 1)


NO_RELU_ZPS = [120, 128, 99, 140]                  # per-layer out_zp without ReLU: the pad codes of the intermediate maps
CHAIN_CASES = {
    "odd_input_depth4_stride2": ChainCase((1, 9, 61), 4, 2, 0, NO_RELU_ZPS, 61),
    "two_images_depth3_stride2": ChainCase((2, 23, 70), 3, 2, 0, NO_RELU_ZPS, 62),
    "smaller_than_the_halo_depth4": ChainCase((1, 3, 4), 4, 1, 0, NO_RELU_ZPS, 65),
    "depth1": ChainCase((1, 17, 33), 1, 1, 0, NO_RELU_ZPS, 64),
    # the existing chain test's zero points through this generator; post-ReLU inputs carry a large mean (x - zx), so zw stays in [64, 192)
    "relu_exact_patch_depth4_stride2": ChainCase((1, 10, 64), 4, 2, 1, [7, 0, 11, 5], 66, zw_range=(64, 192)),
}


class PreparedChain:
    """the layers of a ChainCase, each drawn for the measured statistics of the ORACLE's codes of the layer before it; ``live`` on every layer"""

    def __init__(self, case):
        self.case = case
        rng = np.random.default_rng(3000 + case.seed)
        self.x = hostile_input(rng, case.n, case.in_h, case.in_w, 64)
        self.layers, self.wants = [], []
        cur, zx, stats = self.x, (ZX_TINY if case.in_h * case.in_w < 64 else ZX)[0], None
        for l in range(case.depth):
            layer = conv_layer(rng, [(0, 64, zx)], 64, 64, case.stride0 if l == 0 else 1, case.relu, case.zps[l], x_stats=stats, zw_range=case.zw_range)
            want = oracle_conv(layer, cur)
            live(want, case.relu, case.zps[l], oracle_conv(layer, cur, relu=0) if case.relu and case.zps[l] > 0 else None)
            self.layers.append(layer)
            self.wants.append(want)
            cur, zx, stats = want, case.zps[l], [(float(want.mean()), float(want.std()))]
        self.expect = expect_from(cur, window=False)


# ---- the extremes --------------------------------------------------------------------------------------------------------------------------

def extreme_layer(c, cout, stride, relu, zp, zx):
    """(layer, per-image input code) of the extremes case: one group of ``c`` channels; output channel co has all its weight codes at 255
    and zw = 0 (co even) or codes 0 and zw = 255 (co odd), so w - zw = +-255 and, over the two runs zx = 0 and zx = 255, all four pairs
    (zx, zw) occur.  Images alternate between code 0 and code 255: x - zx is 0 in one half of them and +-255 in the other.  With out_delta 1,
    nine taps move a code by 80 steps, six by 53.3 and four by 35.6; the bias puts T = 0 at zp + 100 under ReLU (so that no sign of T
    saturates) and at zp without, plus a per-channel shift of -3 .. 3 steps."""
    odd = np.arange(cout) % 2
    code = np.broadcast_to(np.where(odd, 0, 255).astype(np.uint8)[:, None, None, None], (cout, c, 3, 3)).copy()
    zw = np.where(odd, 255, 0)
    dw = np.full(cout, 80.0 / (9.0 * c * 255.0 * 255.0), np.float32)
    bias = ((100.0 if relu else 0.0) + np.linspace(-3.0, 3.0, cout)).astype(np.float32)
    return Layer([(0, c, np.float32(1.0), zx)], c, stride, code, zw, dw, bias, relu, 1.0, zp)


# (entry, form, c, cout, stride, (n, h, w)): the smallest n that reaches each form; images of a few pixels
EXTREME_SHAPES = [
    ("wide", "bn128", 1536, 256, 1, (2, 3, 4)),                   # MAX_CHUNKS chunks; the regular entry takes k256 for it
    ("regular", "k256", 256, 256, 1, (2, 3, 4)),
    ("regular", "k64", 64, 64, 2, (2, 5, 7)),
    ("wide", "ws64", 64, 64, 1, (1024, 2, 3)),
    ("wide", "ws2_2x2", 64, 64, 2, (1024, 3, 5)),
    ("wide", "ws2_4x1", 64, 128, 2, (1024, 3, 5)),
    ("chain", ("chain", 1, 1), 64, 64, 1, (2, 3, 4)),
    ("chain", ("chain", 1, 2), 64, 64, 2, (2, 5, 7)),
]


def extreme_input(n, h, w, c):
    x = np.zeros((n, h, w, c), np.uint8)
    x[1::2] = 255
    return x


def assert_extreme_reference(layer, x, want):
    """on the numpy reference: max |T| >= 2^24 (the int-to-float conversion rounds) while |T|, |corr| and |aw * window sum| stay below 2^31
    and the window sum inside 24 bits -- the conditions under which the kernels are specified; at least three distinct codes per channel"""
    T, xs = window_sums(x, layer, 0)
    c, zx = layer.groups[0][1], layer.groups[0][3]
    aw, ax = 128 - layer.zw, 128 - zx
    wsum = (layer.code.astype(np.int64) - 128).sum(axis=(1, 2, 3))
    corr = ax * wsum + 9 * c * ax * aw
    assert np.abs(T).max() >= 2 ** 24, np.abs(T).max()
    assert np.abs(T).max() < 2 ** 31 and np.abs(corr).max() < 2 ** 31
    assert np.abs(xs).max() < 2 ** 23, "the window sum must fit 24 bits (__mul24)"
    assert np.abs(xs[..., None] * aw).max() < 2 ** 31
    # the kernels' decomposition is the same integer: sum xs ws + aw sum xs + corr
    acc = T - xs[..., None] * aw - corr
    assert np.abs(acc).max() < 2 ** 31
    distinct = np.array([len(np.unique(want[..., co])) for co in range(layer.cout)])
    assert distinct.min() >= 3, f"channels with fewer than three distinct reference codes: {np.nonzero(distinct < 3)[0]}"
    assert want.min() > 0 and want.max() < 255, "the extremes case must not saturate"


# ---- launches (GPU) ------------------------------------------------------------------------------------------------------------------------

def _desc(layer, n, h, w, out_ct, out_c0):
    from quantv2x_amd import lib as L
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin_total, d.stride, d.cout, d.ngroups = n, h, w, layer.cin_total, layer.stride, layer.cout, len(layer.groups)
    for i, (c0, c, _, zx) in enumerate(layer.groups):
        d.group_c0[i], d.group_c[i], d.group_zx[i] = c0, c, zx
    d.out_ctotal, d.out_c0, d.relu, d.out_delta, d.out_zp = out_ct, out_c0, layer.relu, layer.da, float(layer.zp)
    return d


def launch(entry, layer, x, xpad, window=True, fill=SENT):
    """one layer through "regular" (qv2x_conv3x3_i8) or "wide" (qv2x_conv3x3_i8_pack_wide + qv2x_conv3x3_i8_wide) into a fresh destination
    full of ``fill`` (with the FRONT / BACK spare channels when ``window``); returns it as a numpy int8 array"""
    import torch
    from quantv2x_amd import lib as L
    from quantv2x_amd.engine import _ConvLayer
    lib, dev = L.load(), torch.device("cuda", 0)
    n, h, w, _ = x.shape
    ho, wo = out_hw(h, w, layer.stride)
    dl = _ConvLayer(layer.state(), "layer", layer.groups, layer.stride, dev)
    ct, c0 = (FRONT + layer.cout + BACK, FRONT) if window else (layer.cout, 0)
    d = _desc(layer, n, h, w, ct, c0)
    xin = torch.from_numpy(xpad).to(dev)
    out = torch.full((n, ho + 2, wo + 2, ct), fill, dtype=torch.int8, device=dev)
    st = L.current_stream()
    if entry == "wide":
        w_wide = torch.empty_like(dl.w)
        L.check(lib.qv2x_conv3x3_i8_pack_wide(C.byref(d), L.ptr(dl.w), L.ptr(w_wide), st), "qv2x_conv3x3_i8_pack_wide")
        L.check(lib.qv2x_conv3x3_i8_wide(C.byref(d), L.ptr(xin), L.ptr(w_wide), L.ptr(dl.scale), L.ptr(dl.corr), L.ptr(dl.aw), L.ptr(dl.bias),
                                         L.ptr(out), st), "qv2x_conv3x3_i8_wide")
    else:
        assert entry == "regular"
        L.check(lib.qv2x_conv3x3_i8(C.byref(d), L.ptr(xin), L.ptr(dl.w), L.ptr(dl.scale), L.ptr(dl.corr), L.ptr(dl.aw), L.ptr(dl.bias),
                                    L.ptr(out), st), "qv2x_conv3x3_i8")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def launch_chain(layers, x, xpad, relu):
    """(the chain entry's destination, the destinations of the layer-wise qv2x_conv3x3_i8 launches, one per layer) as numpy int8
    [n][h + 2][w + 2][64]; the chain's is allocated full of SENT, the layer-wise maps hold each layer's pad code in their ring"""
    import torch
    from quantv2x_amd import lib as L
    from quantv2x_amd.engine import _ChainLayers, _ConvLayer
    lib, dev = L.load(), torch.device("cuda", 0)
    n, in_h, in_w, _ = x.shape
    h, w = out_hw(in_h, in_w, layers[0].stride)
    dls = [_ConvLayer(l.state(f"l{i}"), f"l{i}", l.groups, l.stride, dev) for i, l in enumerate(layers)]
    assert _ChainLayers.eligible(dls)
    chain = _ChainLayers(dls, dev)
    xin = torch.from_numpy(xpad).to(dev)
    st = L.current_stream()
    cur, hh, ww, maps = xin, in_h, in_w, []
    for l, dl in zip(layers, dls):
        out = torch.full((n, h + 2, w + 2, 64), l.zp - 128, dtype=torch.int8, device=dev)
        d = _desc(l, n, hh, ww, 64, 0)
        L.check(lib.qv2x_conv3x3_i8(C.byref(d), L.ptr(cur), L.ptr(dl.w), L.ptr(dl.scale), L.ptr(dl.corr), L.ptr(dl.aw), L.ptr(dl.bias), L.ptr(out), st),
                "qv2x_conv3x3_i8")
        cur, hh, ww = out, h, w
        maps.append(out)
    got = torch.full((n, h + 2, w + 2, 64), SENT, dtype=torch.int8, device=dev)
    cd = L.ChainDesc()
    cd.n, cd.h, cd.w, cd.in_h, cd.in_w, cd.depth, cd.stride0, cd.relu = n, h, w, in_h, in_w, len(layers), layers[0].stride, relu
    for i, l in enumerate(layers):
        cd.out_delta[i], cd.out_zp[i] = l.da, float(l.zp)
    L.check(lib.qv2x_conv3x3_i8_chain64(C.byref(cd), L.ptr(xin), L.ptr(chain.w), L.ptr(chain.scale), L.ptr(chain.corr), L.ptr(chain.aw),
                                        L.ptr(chain.bias), L.ptr(got), st), "qv2x_conv3x3_i8_chain64")
    torch.cuda.synchronize()
    return got.cpu().numpy(), [m.cpu().numpy() for m in maps]


def check_outputs(got, expect, what, window=True):
    """the sentinel in the pad ring and (``window``) in the spare channels, the window equal to the oracle bit for bit, nothing else anywhere"""
    assert got.shape == expect.shape
    for name, part in (("top row", got[:, 0]), ("bottom row", got[:, -1]), ("left column", got[:, :, 0]), ("right column", got[:, :, -1])):
        assert (part == SENT).all(), f"{what}: pad ring written ({name})"
    if window:
        assert (got[..., :FRONT] == SENT).all(), f"{what}: channels in front of the window written"
        assert (got[..., got.shape[-1] - BACK:] == SENT).all(), f"{what}: channels behind the window written"
    np.testing.assert_array_equal(got, expect, err_msg=f"{what}: the window against the oracle")
