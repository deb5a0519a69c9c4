"""Random deblock layers (ConvTranspose2d, kernel == stride == s) for csrc/deconv_f32.hip, their launches and their references (no tests here).

Used by tests/test_hip_deblock_layers.py (GPU) and tests/test_deblock_layers_cpu.py (no GPU).

**Layers.**  ``deblock_layer`` draws ``wdeq [Cin, Cout, s, s]`` whose columns have a CONTROLLED sum over Cin:  +-COL_SUM sigma / x_std, the
sign drawn per column.  A free sum (std sqrt(Cin) of a weight) times the mean of the dequantized input (up to 127.5 dx at in_zx 0 or 255)
would pin whole columns to one end of the code range, and a per-channel bias could not take that out, since the s * s sub-positions of a
channel have different weights; a zero sum would make y blind to in_zx.  With this sum the offset is at most +-0.43 sigma, and ONE code of
in_zx moves every y by COL_SUM sigma / 73.9 = 0.0034 sigma: 0.2 to 0.4 output steps (``zx_sensitivity`` states the share of the oracle's codes
that in_zx +- 1 changes; tests/test_deblock_layers_cpu.py asserts it for the quantizer grid).  With  var(x^) = ``x_std`` ^ 2  per input
channel,  std(y) = ``sigma``:  w - mean ~ N(0, sigma / (sqrt(Cin) x_std)),  bias ~ N(0, 0.3 sigma).  ``out_step`` puts 2 sigma on the codes between
the zero point and the nearer end that the output can reach, so about 2 % of the outputs saturate there: the clamps decide codes.

**live(want, relu, zp)** is the condition every case states ON THE ORACLE'S OUTPUT before any kernel result is looked at:
with ReLU 20-80 % of the codes equal zp and at least 0.5 % equal 255; without, at least 0.5 % at 0, 0.5 % at 255 and 20 % below zp.  For
a ReLU layer with zp > 0 the oracle also runs without ReLU and at least 20 % of THOSE codes must lie below zp: the folded clamp decides them.

**launch_plan** restates the host launch rule of deconv_f32.hip in plain Python (``ps_takes``, ``ps_plan`` and the 2560-item loop, the
16384-wave-tile threshold, qv2x_deconv_f32in's cin <= 128).  Every GPU case names the form and the pairs per item it was written for and
asserts them through this function: after a change of the rule the case list fails instead of silently aiming at nothing.

**Destinations** are [n][H + 2][W + 2][FRONT + sum cout + BACK] int8 maps allocated full of SENT; ``check_outputs`` compares the windows
with the oracle bit for bit and requires SENT everywhere else: pad ring, channels in front of and behind the windows.
"""
import ctypes as C

import numpy as np

SENT = -77
FRONT, BACK = 16, 32        # spare channels in front of / behind the windows of a destination
CODE_STD = 73.9             # std of codes uniform on 0..255
DX = 0.031                  # the input step of every int8 case
COL_SUM = 0.25              # |sum over Cin| of a weight column, in units of sigma / x_std


# ---- layers ----------------------------------------------------------------------------------------------------------------------------

def deblock_layer(rng, cin, cout, s, sigma=1.0, x_std=CODE_STD * DX):
    """(wdeq [Cin, Cout, s, s] f32, bias [Cout] f32, packed weights as engine._DeconvLayer builds them) with std(y) ~ sigma"""
    from quantv2x_amd.engine import _pack_k4p
    w = rng.standard_normal((cin, cout, s, s))
    w -= w.mean(axis=0, keepdims=True)
    col_sum = COL_SUM * (sigma / x_std) * rng.choice([-1.0, 1.0], size=(1, cout, s, s))
    wdeq = (w * (sigma / (np.sqrt(cin) * x_std)) + col_sum / cin).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.3 * sigma).astype(np.float32)
    cols = wdeq.transpose(0, 2, 3, 1).reshape(cin, s * s * cout)              # col = (i*s + j)*Cout + co
    return wdeq, bias, _pack_k4p(np.ascontiguousarray(cols.T))


def out_step(sigma, zp, relu):
    """the output step that puts 2 sigma at the nearer reachable end of the code range"""
    span = (255.0 - zp) if relu else min(zp, 255.0 - zp)
    return float(np.float32(2.0 * sigma / span))


def padded(x_u8, zp):
    """u8 [N,H,W,C] -> padded i8 [N,H+2,W+2,C] (code - 128) whose border holds the pad code ``zp``"""
    n, h, w, c = x_u8.shape
    p = np.full((n, h + 2, w + 2, c), int(zp), np.int16)
    p[:, 1:-1, 1:-1] = x_u8
    return (p - 128).astype(np.int8)


# ---- the condition on the inputs ---------------------------------------------------------------------------------------------------------

def live(want, relu, zp, want_norelu=None):
    """asserts that both clamps decide codes of the ORACLE's output ``want`` (u8); ``want_norelu``: the same layer's codes without ReLU"""
    at = lambda v: float((want == v).mean())
    if relu:
        assert 0.2 <= at(zp) <= 0.8, f"ReLU: {at(zp):.3f} of the reference codes equal zp = {zp}"
        assert at(255) >= 0.005, f"ReLU: {at(255):.4f} of the reference codes are 255"
        if zp > 0:
            assert want_norelu is not None, "a ReLU case with zp > 0 also needs the oracle's codes without ReLU"
            below = float((want_norelu < zp).mean())
            assert below >= 0.2, f"without ReLU only {below:.3f} of the reference codes lie below zp = {zp}"
    else:
        below = float((want < zp).mean())
        assert at(0) >= 0.005 and at(255) >= 0.005, f"no ReLU: {at(0):.4f} at 0, {at(255):.4f} at 255"
        assert below >= 0.2, f"no ReLU: {below:.3f} of the reference codes lie below zp = {zp}"


# ---- the host launch rule, restated --------------------------------------------------------------------------------------------------------

PS_CINS = (64, 128, 256)    # ps_takes: the pixel-stationary form's operand registers are sized at compile time


def _ps_plan(layers, cap):
    nps, total = [], 0
    for cin, cout, s, m in layers:
        pairs, mt, np_ = s * s * cout // 64, 2 if cin == 64 else 1, 1
        while np_ * 2 <= cap and pairs % (np_ * 2) == 0:
            np_ *= 2
        total += -(-m // (32 * mt)) * (pairs // np_)
        nps.append(np_)
    return nps, total


def _ps_items(layers):
    cap = 8
    nps, total = _ps_plan(layers, cap)
    while cap > 1 and total < 2560:
        cap >>= 1
        nps, total = _ps_plan(layers, cap)
    return nps


def launch_plan(entry, layers):
    """entry: "single" (qv2x_deconv_i8) | "batch" (qv2x_deconv_i8_batch) | "f32in" (qv2x_deconv_f32in); layers: [(cin, cout, s, M)], M = n h w.
    Returns (form, [column pairs per item of each layer, in the caller's order] or None):  "ps" = pixel-stationary items, "wave32" = 32 x 32
    wave tiles, "wave64" = 64 x 64 wave tiles."""
    layers = [tuple(l) for l in layers]
    if entry == "single":
        assert len(layers) == 1
        return "wave32", None
    if entry == "f32in":
        assert len(layers) == 1
        if layers[0][0] in PS_CINS and layers[0][0] <= 128:
            return "ps", _ps_items(layers)
        return "wave32", None
    assert entry == "batch" and 1 <= len(layers) <= 4
    if all(l[0] in PS_CINS for l in layers):
        return "ps", _ps_items(layers)                        # (the host's sort by falling Cin changes neither a layer's np nor the total)
    tiles = sum(-(-m // 32) * (s * s * cout // 32) for cin, cout, s, m in layers)
    return ("wave64" if tiles >= 16384 else "wave32"), None


# ---- cases: inputs and references (CPU only) -----------------------------------------------------------------------------------------------

class Case:
    """layers: [(cin, cout, s, h, w)] with equal h s, w s; dests[i]: the destination layer i writes to (windows side by side behind FRONT spare
    channels, in layer order); f32in: the input is an fp32 map with both signs instead of codes.  ``form`` / ``nps``: what launch_plan must say
    for the batch entry (the fp32-map entry when f32in)."""

    def __init__(self, layers, n, form, nps=None, relu=1, zp=7, zx=3, dests=None, f32in=False, seed=0):
        self.layers, self.n, self.form, self.nps = [tuple(l) for l in layers], n, form, nps
        self.relu, self.zp, self.zx, self.f32in, self.seed = relu, zp, zx, f32in, seed
        self.dests = list(dests) if dests is not None else [0] * len(layers)
        self.H, self.W = layers[0][3] * layers[0][2], layers[0][4] * layers[0][2]
        assert all((h * s, w * s) == (self.H, self.W) for (_ci, _co, s, h, w) in self.layers)

    def plan_layers(self):
        return [(cin, cout, s, self.n * h * w) for (cin, cout, s, h, w) in self.layers]


def oracle_codes(x, wdeq, bias, s, relu, da, za, dx=None, zx=None):
    """u8 [n, h s, w s, cout] of orc_deconv (x u8 codes) or orc_deconv_f32in (x f32)"""
    from oracle.spec import _cf, _f32, _p, lib as olib
    n, h, w, cin = x.shape
    cout = wdeq.shape[1]
    out = np.zeros((n, h * s, w * s, cout), np.uint8)
    if x.dtype == np.uint8:
        olib().orc_deconv(_p(x), n, h, w, cin, _cf(dx), int(zx), _p(wdeq), _p(_f32(bias)), cout, s, int(relu), _cf(da), _cf(za), _p(out), cout, 0)
    else:
        assert x.dtype == np.float32
        olib().orc_deconv_f32in(_p(x), n, h, w, cin, _p(wdeq), _p(_f32(bias)), cout, s, int(relu), _cf(da), _cf(za), _p(out), cout, 0)
    return out


X_STD_F32 = 1.7             # spread of the fp32 maps


class Prepared:
    """a Case's operands and the expected bytes of every destination; ``live`` asserted on every layer"""

    def __init__(self, case, sigma=1.0):
        self.case = case
        rng = np.random.default_rng(1000 + case.seed)
        self.da = out_step(sigma, case.zp, case.relu)
        ndest = max(case.dests) + 1
        ctot = [FRONT + sum(l[1] for l, d in zip(case.layers, case.dests) if d == k) + BACK for k in range(ndest)]
        self.expect = [np.full((case.n, case.H + 2, case.W + 2, c), SENT, np.int8) for c in ctot]
        self.windows = [[] for _ in range(ndest)]                     # per destination: (c0, cout)
        self.x, self.wdeq, self.packed, self.bias, self.c0 = [], [], [], [], []
        nxt = [FRONT] * ndest
        for (cin, cout, s, h, w), dst in zip(case.layers, case.dests):
            if case.f32in:
                x = (rng.standard_normal((case.n, h, w, cin)) * X_STD_F32).astype(np.float32)
                wdeq, bias, packed = deblock_layer(rng, cin, cout, s, sigma, X_STD_F32)
            else:
                x = rng.integers(0, 256, size=(case.n, h, w, cin), dtype=np.uint8)
                wdeq, bias, packed = deblock_layer(rng, cin, cout, s, sigma)
            want = oracle_codes(x, wdeq, bias, s, case.relu, self.da, case.zp, DX, case.zx)
            norelu = oracle_codes(x, wdeq, bias, s, 0, self.da, case.zp, DX, case.zx) if case.relu and case.zp > 0 else None
            live(want, case.relu, case.zp, norelu)
            c0 = nxt[dst]
            nxt[dst] += cout
            self.expect[dst][:, 1:-1, 1:-1, c0:c0 + cout] = (want.astype(np.int16) - 128).astype(np.int8)
            self.windows[dst].append((c0, cout))
            self.x.append(x); self.wdeq.append(wdeq); self.packed.append(packed); self.bias.append(bias); self.c0.append(c0)


def zx_sensitivity(prep):
    """the smallest share of a layer's ORACLE codes that in_zx + 1 or in_zx - 1 changes (the oracle takes any integer zero point)"""
    case, worst = prep.case, 1.0
    assert not case.f32in
    for (cin, cout, s, h, w), x, wdeq, bias, c0, dst in zip(case.layers, prep.x, prep.wdeq, prep.bias, prep.c0, case.dests):
        want = (prep.expect[dst][:, 1:-1, 1:-1, c0:c0 + cout].astype(np.int16) + 128).astype(np.uint8)
        for zx in (case.zx - 1, case.zx + 1):
            worst = min(worst, float((oracle_codes(x, wdeq, bias, s, case.relu, prep.da, case.zp, DX, zx) != want).mean()))
    return worst


# ---- launches (GPU) ------------------------------------------------------------------------------------------------------------------------

def launch(prep, entry):
    """runs the case through ``entry`` ("single": one qv2x_deconv_i8 per layer | "batch" | "f32in") into fresh destinations full of SENT;
    returns them as numpy int8 arrays"""
    import torch
    from quantv2x_amd import lib as L
    case = prep.case
    assert (entry == "f32in") == case.f32in
    lib, dev = L.load(), torch.device("cuda", 0)
    outs = [torch.full(e.shape, SENT, dtype=torch.int8, device=dev) for e in prep.expect]
    descs, ins, ws, bs = [], [], [], []
    for i, (cin, cout, s, h, w) in enumerate(case.layers):
        d = L.DeconvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.s, d.in_zx, d.in_delta = case.n, h, w, cin, cout, s, case.zx, DX
        d.out_ctotal, d.out_c0, d.relu = prep.expect[case.dests[i]].shape[-1], prep.c0[i], case.relu
        d.out_delta, d.out_zp, d.out_h, d.out_w = prep.da, float(case.zp), case.H, case.W
        descs.append(d)
        ins.append(torch.from_numpy(prep.x[i] if case.f32in else padded(prep.x[i], case.zx)).to(dev))
        ws.append(torch.from_numpy(prep.packed[i]).to(dev))
        bs.append(torch.from_numpy(prep.bias[i]).to(dev))
    dst = [outs[k] for k in case.dests]
    k = len(descs)
    if entry == "batch":
        arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
        L.check(lib.qv2x_deconv_i8_batch((L.DeconvDesc * k)(*descs), k, arr(ins), arr(ws), arr(bs), arr(dst), L.current_stream()), "qv2x_deconv_i8_batch")
    else:
        fn, name = (lib.qv2x_deconv_f32in, "qv2x_deconv_f32in") if entry == "f32in" else (lib.qv2x_deconv_i8, "qv2x_deconv_i8")
        for d, xt, wt, bt, ot in zip(descs, ins, ws, bs, dst):
            L.check(fn(C.byref(d), L.ptr(xt), L.ptr(wt), L.ptr(bt), L.ptr(ot), L.current_stream()), name)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check_outputs(prep, outs, what):
    """the sentinel in the pad ring and in the spare channels, the windows equal to the oracle bit for bit, nothing else anywhere"""
    for k, (got, exp) in enumerate(zip(outs, prep.expect)):
        tag = f"{what}, destination {k}"
        first, last = prep.windows[k][0][0], prep.windows[k][-1][0] + prep.windows[k][-1][1]
        assert first == FRONT and last == exp.shape[-1] - BACK
        for name, part in (("top row", got[:, 0]), ("bottom row", got[:, -1]), ("left column", got[:, :, 0]), ("right column", got[:, :, -1])):
            assert (part == SENT).all(), f"{tag}: pad ring written ({name})"
        assert (got[..., :first] == SENT).all(), f"{tag}: channels in front of the window written"
        assert (got[..., last:] == SENT).all(), f"{tag}: channels behind the window written"
        np.testing.assert_array_equal(got, exp, err_msg=f"{tag}: the windows against the oracle")


# ---- the GPU cases -------------------------------------------------------------------------------------------------------------------------
# (n h w) are the smallest that reach each path; the form and the pairs per item in the comments are asserted through launch_plan

I8_CASES = {
    # pair 1 of the three holds channels 64-95 of sub-position (0, 0) and 0-31 of (0, 1)
    "straddle_np1": Case([(128, 96, 2, 9, 13)], 2, "ps", [1], seed=1),
    # 863 pixel tiles x 3 items = 2589 >= 2560: the rule keeps two pairs per item; item 1 starts at column 128 = channel 32 of sub-position 1
    # and runs into sub-position 2 = (1, 0): dj carries into di inside the item
    "straddle_np2": Case([(128, 96, 2, 100, 92)], 3, "ps", [2], zp=0, seed=2),
    # M = 70, two pixel tiles per item: the second item's second pixel tile lies entirely past the end
    "cout32_dead_second_pixel_tile": Case([(64, 32, 2, 5, 7)], 2, "ps", [1], seed=3),
    "s3": Case([(256, 64, 3, 5, 7)], 1, "ps", [1], seed=4),
    # one item = both pairs = all four sub-positions: the step from pair 0 to pair 1 carries dj into di INSIDE an item ((0, 1) -> (1, 0));
    # 2568 pixel tiles x 1 item >= 2560 keeps np = 2; M = 82170 = 2567 tiles + 26 pixels
    "s2_cout32_np2_carry": Case([(128, 32, 2, 166, 165)], 3, "ps", [2], zp=0, seed=14),
    # 18 pairs: np caps at 2; 285 pixel tiles x 9 items = 2565 >= 2560 keeps it; M = 9100 = 284 tiles + 12 pixels
    "s3_np2": Case([(128, 128, 3, 65, 70)], 2, "ps", [2], zp=0, seed=5),
    # M = 15 < 32, 32 pairs that each straddle two sub-positions
    "s8": Case([(64, 32, 8, 3, 5)], 1, "ps", [1], seed=6),
    "one_pixel": Case([(128, 64, 1, 1, 1)], 1, "ps", [1], seed=7),
    "one_pixel_wide": Case([(256, 128, 2, 37, 1)], 2, "ps", [1], seed=8),
    # Cin 16: the K loop's `two` is never true; 48 and 80: an odd number of 16-channel steps.  M = 420 | 105 | 105
    "cin_tails_wave": Case([(16, 64, 1, 10, 14), (48, 64, 2, 5, 7), (80, 96, 2, 5, 7)], 3, "wave32", seed=9),
    # M = 32770: 1025 x (4 + 12) = 16400 wave tiles >= 16384; M mod 64 = 2: the last 64-pixel tile's second half is dead
    "wave64": Case([(48, 32, 2, 145, 113), (80, 96, 2, 145, 113)], 2, "wave64", zp=0, seed=10),
    # MAX_BATCH layers, the falling-Cin sort moves entries (64, 256, 128, 64 -> 256, 128, 64, 64), equal Cin twice; one 12 x 20 output
    "four_layers_one_destination": Case([(64, 64, 1, 12, 20), (256, 32, 4, 3, 5), (128, 96, 2, 6, 10), (64, 128, 1, 12, 20)], 2, "ps", [1, 1, 1, 1], seed=11),
    "four_layers_two_destinations": Case([(64, 64, 1, 12, 20), (256, 32, 4, 3, 5), (128, 96, 2, 6, 10), (64, 128, 1, 12, 20)], 2, "ps", [1, 1, 1, 1],
                                         dests=[0, 1, 0, 1], seed=12),
    # a pixel-stationary shape beside one that is not: everything falls back to wave tiles
    "mixed": Case([(128, 64, 2, 7, 9), (48, 64, 2, 7, 9)], 3, "wave32", seed=13),
}

# the quantizer grid on one pixel-stationary and one wave-only shape
QUANT_SHAPES = {"ps": (128, 64, 2, 7, 9), "wave": (48, 64, 2, 7, 9)}
QUANT_GRID = [(relu, zp, zx) for (relu, zp) in [(1, 0), (1, 7), (1, 64), (0, 128)] for zx in (0, 255)]


def quant_case(shape, relu, zp, zx):
    return Case([QUANT_SHAPES[shape]], 3, "ps" if shape == "ps" else "wave32", [1] if shape == "ps" else None, relu=relu, zp=zp, zx=zx,
                seed=100 + 10 * zp + zx + relu)


F32_CASES = {
    "cin64_dead_second_pixel_tile": Case([(64, 32, 2, 5, 7)], 2, "ps", [1], f32in=True, seed=21),        # M = 70
    "straddle": Case([(128, 96, 2, 9, 13)], 2, "ps", [1], f32in=True, seed=22),
    "wave_cin16": Case([(16, 64, 1, 5, 9)], 2, "wave32", f32in=True, seed=23),                           # M = 90
    "wave_cin48": Case([(48, 32, 2, 5, 7)], 2, "wave32", f32in=True, seed=24),
    "wave_cin256_s3": Case([(256, 64, 3, 5, 7)], 1, "wave32", f32in=True, seed=25),                      # fp32 rows of 256 channels keep the wave tiles
}


def assert_plan(case):
    """the form (and pairs per item) the case was written for, by the restated rule; the one-layer entry always takes 32 x 32 wave tiles"""
    entry = "f32in" if case.f32in else "batch"
    assert launch_plan(entry, case.plan_layers()) == (case.form, case.nps), f"the launch rule changed: {launch_plan(entry, case.plan_layers())}"
