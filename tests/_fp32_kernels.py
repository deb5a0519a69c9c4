"""Cases, operands, references, launches and checks for the entries of csrc/fp32_path.hip and for qv2x_codebook_decode_f32 (no tests here).

Used by tests/test_fp32_kernels_cpu.py (no GPU: the references pinned, every case's aim asserted on the reference) and
tests/test_hip_fp32_kernels.py (GPU).

**The fp32 GEMM** (qv2x_conv3x3_f32 / qv2x_deconv_f32).  Reference: ``orc_gemm_f32``, bit for bit (one fma chain per output, K walked
k0 k4 k1 k5 k2 k6 k3 k7 inside every group of 8).  A ``Gemm`` case is a list of ``Layer`` s that write side by side into ONE destination
``[n][Ho + 2][Wo + 2][front + sum cout + back]`` allocated full of ``SENT``.  Inputs are padded maps whose ring is zero inside the channel
window and whose channels outside every window a layer reads hold NaN, ring included: one stray read poisons an output.  Weights
~ N(0, 1 / fan_in), x ~ N(0, 1), bias ~ N(0, 0.5): with ReLU about half of the outputs are exactly 0.  ``facts`` names what a case is aimed at
(row count, tile count, a column span over two sub-positions ...); ``gemm_facts`` computes the same from the shapes by the kernel's own
tiling rule (32 rows x 64 columns per wave, four waves per workgroup) and the CPU file asserts that they agree.

**natural_order** runs the oracle on operands whose channels are permuted inside every group of 8 so that its k0 k4 k1 ... walk visits the
ORIGINAL operands in natural order: the same layer as a k0 k1 k2 ... chain, from the oracle's own arithmetic.

**PFN** (qv2x_pfn_scatter_f32): ``orc_pfn_f32`` + the scatter in numpy, bit for bit; **add_relu**, **occ_sigmoid**, **decode**: numpy.
"""
import ctypes as C

import numpy as np

SENT = np.float32(-777.25)
ORC_K8 = np.array([0, 4, 1, 5, 2, 6, 3, 7])


# ---- the fp32 GEMM: cases ----------------------------------------------------------------------------------------------------------------

class Layer:
    """one launch: input map h x w with ``cin_total`` channels, window [cin0, cin0 + cin); ``form``: "dense" | "centre" (a 1x1 weight as
    engine_pyramid_fp32.centre_tap3x3 lays it out) | "slab" (slab ``slab`` of a grouped 3x3, engine_pyramid_fp32.grouped_slabs)"""

    def __init__(self, h, w, stride, cin, cout, cin_total=None, cin0=0, form="dense", slab=0):
        self.h, self.w, self.stride, self.cin, self.cout, self.cin0 = h, w, stride, cin, cout, cin0
        self.cin_total = cin0 + cin if cin_total is None else cin_total
        self.form, self.slab = form, slab


class Gemm:
    """``layers`` write side by side, in order, behind ``front`` spare channels of one destination; ``share_input``: every layer reads layer
    0's map (the grouped slabs).  ``facts``: what the case is aimed at, asserted against ``gemm_facts`` on the CPU."""

    def __init__(self, aim, deconv, n, layers, relu=1, front=4, back=4, share_input=False, seed=0, **facts):
        self.aim, self.deconv, self.n, self.layers, self.relu, self.front, self.back = aim, deconv, n, layers, relu, front, back
        self.share_input, self.seed, self.facts = share_input, seed, facts
        self.Ho, self.Wo = out_hw(layers[0], deconv)
        assert all(out_hw(l, deconv) == (self.Ho, self.Wo) for l in layers)


def out_hw(l, deconv):
    if deconv:
        return l.h * l.stride, l.w * l.stride
    return (l.h + 2 - 3) // l.stride + 1, (l.w + 2 - 3) // l.stride + 1


def gemm_facts(case):
    """the kernel's tiling of every layer, from the shapes alone: M rows, 32-row x 64-column wave tiles, four per workgroup"""
    f = dict(M=[], tiles=[], K=[], ncols=[])
    spans_images = straddle = early_return = False
    for l in case.layers:
        ho, wo = out_hw(l, case.deconv)
        per = l.h * l.w if case.deconv else ho * wo
        m = case.n * per
        ncols = l.stride * l.stride * l.cout if case.deconv else l.cout
        tiles = -(-m // 32) * (ncols // 64)
        f["M"].append(m); f["tiles"].append(tiles); f["K"].append(l.cin if case.deconv else 9 * l.cin); f["ncols"].append(ncols)
        spans_images |= any(r0 // per != min(r0 + 31, m - 1) // per for r0 in range(0, m, 32))
        if case.deconv:                                                   # a 32-column span (one accumulator) over two sub-positions
            straddle |= any(c0 // l.cout != (c0 + 31) // l.cout for c0 in range(0, ncols, 32))
        early_return |= tiles % 4 != 0
    f.update(spans_images=spans_images, straddle=straddle, early_return=early_return)
    return f


L_ = Layer
CONV_CASES = {
    "m1": Gemm("M = 1: 31 dead rows, one K group per tap, one tile", 0, 1, [L_(1, 1, 1, 8, 64)], M=[1], tiles=[1], K=[72], seed=1),
    "m15": Gemm("M = 15 < 32, cin 24", 0, 1, [L_(3, 5, 1, 24, 64)], M=[15], seed=2),
    "m32_cout128_norelu": Gemm("M = 32 exactly, two column tiles, no ReLU", 0, 1, [L_(4, 8, 1, 8, 128)], relu=0, M=[32], tiles=[2], seed=3),
    "m33_cin64": Gemm("M = 33: a second row tile with one live row, cin 64", 0, 1, [L_(3, 11, 1, 64, 64)], M=[33], tiles=[2], K=[576], seed=4),
    "two_images_cout192": Gemm("n = 2, 3 x 7: row tile 0 spans both images; three column tiles", 0, 2, [L_(3, 7, 1, 24, 192)],
                               M=[42], tiles=[6], spans_images=True, seed=5),
    "nine_tiles": Gemm("3 row tiles x 3 column tiles = 9: three waves of the last workgroup return early", 0, 1, [L_(5, 13, 1, 8, 192)],
                       M=[65], tiles=[9], early_return=True, seed=6),
    "s2_4x6": Gemm("stride 2 on an even map: 2 x 3 outputs", 0, 1, [L_(4, 6, 2, 24, 64)], M=[6], seed=7),
    "s2_5x7_n2": Gemm("stride 2 on an odd map: 3 x 4 outputs, the last taps on the pad ring", 0, 2, [L_(5, 7, 2, 8, 64)], M=[24], seed=8),
    "s2_1x1": Gemm("stride 2 on a 1 x 1 map", 0, 1, [L_(1, 1, 2, 24, 64)], M=[1], seed=9),
    "s2_2x1_norelu": Gemm("stride 2 on a 2 x 1 map: one output, row 1 unread by tap row 0", 0, 1, [L_(2, 1, 2, 8, 64)], relu=0, M=[1], seed=10),
    "cin_window": Gemm("input window 12 + 24 of 40: cin0 a multiple of 4 but not of 8, NaN around it", 0, 1,
                       [L_(5, 7, 1, 24, 64, cin_total=40, cin0=12)], M=[35], seed=11),
    "out_c0_5": Gemm("output window at channel 5: out_c0 not a multiple of 4", 0, 1, [L_(3, 5, 1, 24, 64)], front=5, back=3, M=[15], seed=12),
    "whole_destination": Gemm("out_c0 = 0 and nothing behind the window", 0, 1, [L_(3, 5, 1, 8, 128)], front=0, back=0, relu=0, seed=13),
    "centre_tap_s2": Gemm("the strided 1x1 shortcut: centre tap only, stride 2, no ReLU", 0, 2, [L_(5, 7, 2, 24, 64, form="centre")], relu=0,
                          M=[24], seed=14),
    "grouped_slabs": Gemm("a grouped 3x3 (16 groups of 8) on a 128-channel map: two slabs, cin0 = out_c0 = 64 i, one destination", 0, 2,
                          [L_(4, 5, 1, 64, 64, cin_total=128, cin0=0, form="slab", slab=0),
                           L_(4, 5, 1, 64, 64, cin_total=128, cin0=64, form="slab", slab=1)], front=0, back=0, share_input=True,
                          M=[40, 40], spans_images=True, seed=15),
}

DECONV_CASES = {
    "s1_cout64": Gemm("the 1x1 convolution, M = 15", 1, 1, [L_(3, 5, 1, 16, 64)], M=[15], tiles=[1], straddle=False, seed=21),
    "s1_cout128_norelu": Gemm("the 1x1 convolution, two column tiles, M = 32 exactly, no ReLU", 1, 1, [L_(4, 8, 1, 64, 128)], relu=0,
                              M=[32], tiles=[2], seed=22),
    "s2_cout16_m33": Gemm("s 2, cout 16: all four sub-positions in one column tile; M = 33; K = 8, one group", 1, 1, [L_(3, 11, 2, 8, 16)],
                          M=[33], ncols=[64], K=[8], straddle=True, seed=23),
    "s2_cout32_two_images": Gemm("s 2, cout 32: one sub-position per accumulator; row tile 0 spans both images", 1, 2, [L_(3, 7, 2, 24, 32)],
                                 M=[42], ncols=[128], spans_images=True, straddle=False, seed=24),
    "s2_cout48": Gemm("s 2, cout 48: columns 32..63 hold channels 32-47 of (0, 0) and 0-15 of (0, 1)", 1, 1, [L_(5, 7, 2, 24, 48)],
                      M=[35], ncols=[192], tiles=[6], straddle=True, early_return=True, seed=25),
    "s3_cout64_m1": Gemm("s 3, cout 64, one input pixel: nine column tiles", 1, 1, [L_(1, 1, 3, 16, 64)], M=[1], ncols=[576], tiles=[9], seed=26),
    "s4_cout4": Gemm("s 4, cout 4: eight sub-positions per accumulator, dj carries into di inside it", 1, 1, [L_(3, 5, 4, 8, 4)],
                     M=[15], ncols=[64], straddle=True, seed=27),
    "s4_cout20_norelu": Gemm("s 4, cout 20: five column tiles, every accumulator straddles, no ReLU", 1, 1, [L_(2, 3, 4, 24, 20)], relu=0,
                             M=[6], ncols=[320], tiles=[5], straddle=True, seed=28),
    "s8_cout1": Gemm("s 8, cout 1: the 64 columns are one channel at 64 sub-positions", 1, 1, [L_(3, 5, 8, 16, 1)], M=[15], ncols=[64],
                     straddle=True, seed=29),
    "shared_destination": Gemm("two layers (s 2 and s 1) into one 6 x 10 destination at different out_c0, as the deblocks' concat", 1, 2,
                               [L_(3, 5, 2, 16, 32), L_(6, 10, 1, 24, 64)], M=[30, 120], seed=30),
    "cin_window": Gemm("input window 12 + 24 of 40 with NaN around it, s 2", 1, 1, [L_(3, 5, 2, 24, 32, cin_total=40, cin0=12)], seed=31),
}


# ---- the fp32 GEMM: operands and references (CPU only) ------------------------------------------------------------------------------------

def _wmat(rng, l, deconv):
    """(wmat [columns][K] f32 as the engines build it, the torch-layout weight it came from)"""
    from quantv2x_amd.engine_pyramid_fp32 import centre_tap3x3
    if deconv:
        w = (rng.standard_normal((l.cin, l.cout, l.stride, l.stride)) / np.sqrt(l.cin)).astype(np.float32)       # [Cin][Cout][s][s]
        return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, l.cin)), w
    if l.form == "centre":
        w = (rng.standard_normal((l.cout, l.cin, 1, 1)) / np.sqrt(l.cin)).astype(np.float32)
        return centre_tap3x3(w), w
    assert l.form == "dense", "slabs are drawn once per case"
    w = (rng.standard_normal((l.cout, l.cin, 3, 3)) / np.sqrt(9 * l.cin)).astype(np.float32)                     # [Cout][Cin][3][3]
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(l.cout, -1)), w


GROUP_CG = 8                # (with 4 channels per group an output's live k are k0..k3 or k4..k7 of every K group: both walks visit them in one order)


def orc_gemm(x, l, deconv, wmat, bias, relu, out=None, out_c0=0):
    """orc_gemm_f32 on the UNPADDED map x [n][h][w][cin_total]; returns out [n][Ho][Wo][..]"""
    from oracle.spec import _f32, _p, lib as olib
    n = x.shape[0]
    ho, wo = out_hw(l, deconv)
    if out is None:
        out = np.zeros((n, ho, wo, l.cout), np.float32)
    wmat, bias = _f32(wmat), _f32(bias)
    olib().orc_gemm_f32(_p(x), n, l.h, l.w, l.cin_total, l.cin0, l.cin, l.stride, l.cout, int(deconv), _p(wmat), _p(bias), int(relu),
                        _p(out), out.shape[3], out_c0)
    return out


def natural_order(x, l, deconv, wmat, bias, relu):
    """the same layer as a k0 k1 k2 ... chain: channel 8 g + ORC_K8[e] of the permuted operands holds channel 8 g + e of the originals"""
    perm = np.empty(l.cin, np.int64)
    for g in range(0, l.cin, 8):
        perm[g + ORC_K8] = g + np.arange(8)
    xw = np.ascontiguousarray(x[..., l.cin0:l.cin0 + l.cin][..., perm])
    taps = wmat.shape[1] // l.cin
    wp = np.ascontiguousarray(wmat.reshape(wmat.shape[0], taps, l.cin)[..., perm].reshape(wmat.shape))
    ll = Layer(l.h, l.w, l.stride, l.cin, l.cout)
    return orc_gemm(xw, ll, deconv, wp, bias, relu)


class GemmPrepared:
    """operands of a case, the oracle's output of every layer (with the case's ReLU and without), the expected destination"""

    def __init__(self, case):
        from quantv2x_amd.engine_fp32 import pack_k8
        from quantv2x_amd.engine_pyramid_fp32 import grouped_slabs
        self.case = case
        rng = np.random.default_rng(7000 + case.seed)
        ctot = case.front + sum(l.cout for l in case.layers) + case.back
        self.expect = np.full((case.n, case.Ho + 2, case.Wo + 2, ctot), SENT, np.float32)
        self.x, self.xpad, self.wmat, self.wtorch, self.packed, self.bias, self.c0, self.want, self.want_norelu = [], [], [], [], [], [], [], [], []
        slabs = None
        if any(l.form == "slab" for l in case.layers):
            c = case.layers[0].cin_total
            self.wgroup = (rng.standard_normal((c, GROUP_CG, 3, 3)) / np.sqrt(9 * GROUP_CG)).astype(np.float32)
            slabs = grouped_slabs(self.wgroup)
        c0 = case.front
        for i, l in enumerate(case.layers):
            if i == 0 or not case.share_input:
                x = rng.standard_normal((case.n, l.h, l.w, l.cin_total)).astype(np.float32)
                used = np.zeros(l.cin_total, bool)
                for ll in (case.layers if case.share_input else [l]):
                    used[ll.cin0:ll.cin0 + ll.cin] = True
                x[..., ~used] = np.nan
                xpad = np.zeros((case.n, l.h + 2, l.w + 2, l.cin_total), np.float32)
                xpad[..., ~used] = np.nan
                xpad[:, 1:-1, 1:-1] = x
            if l.form == "slab":
                wmat, wt = slabs[l.slab], None
            else:
                wmat, wt = _wmat(rng, l, case.deconv)
            bias = (rng.standard_normal(l.cout) * 0.5).astype(np.float32)
            want = orc_gemm(x, l, case.deconv, wmat, bias, case.relu)
            self.want_norelu.append(orc_gemm(x, l, case.deconv, wmat, bias, 0) if case.relu else want)
            self.expect[:, 1:-1, 1:-1, c0:c0 + l.cout] = want
            self.x.append(x); self.xpad.append(xpad); self.wmat.append(wmat); self.wtorch.append(wt); self.packed.append(pack_k8(wmat))
            self.bias.append(bias); self.c0.append(c0); self.want.append(want)
            c0 += l.cout


def ref64(x, l, deconv, wmat, bias, relu):
    """(float64 torch convolution of the same operands, the bound (K + 2) 2^-24 (sum |x w| + |bias|) per output), both [n][Ho][Wo][cout]"""
    import torch
    import torch.nn.functional as F
    xw = torch.from_numpy(x[..., l.cin0:l.cin0 + l.cin].astype(np.float64)).permute(0, 3, 1, 2)
    b = torch.from_numpy(bias.astype(np.float64))
    k = wmat.shape[1]
    if deconv:
        s = l.stride
        w = torch.from_numpy(wmat.astype(np.float64).reshape(s, s, l.cout, l.cin)).permute(3, 2, 0, 1).contiguous()
        y = F.conv_transpose2d(xw, w, b, stride=s)
        mag = F.conv_transpose2d(xw.abs(), w.abs(), b.abs(), stride=s)
    else:
        w = torch.from_numpy(wmat.astype(np.float64).reshape(l.cout, 3, 3, l.cin)).permute(0, 3, 1, 2).contiguous()
        y = F.conv2d(xw, w, b, stride=l.stride, padding=1)
        mag = F.conv2d(xw.abs(), w.abs(), b.abs(), stride=l.stride, padding=1)
    if relu:
        y = y.clamp_min(0.0)
    return y.permute(0, 2, 3, 1).numpy(), (k + 2) * 2.0 ** -24 * mag.permute(0, 2, 3, 1).numpy()


# ---- the fp32 GEMM: launch and check (GPU) --------------------------------------------------------------------------------------------------

def gemm_launch(prep):
    """every layer of the case into one fresh destination full of SENT; returns it as a numpy array"""
    import torch
    from quantv2x_amd import lib as L
    case = prep.case
    lib, dev = L.load(), torch.device("cuda", 0)
    out = torch.full(prep.expect.shape, float(SENT), dtype=torch.float32, device=dev)
    fn, name = (lib.qv2x_deconv_f32, "qv2x_deconv_f32") if case.deconv else (lib.qv2x_conv3x3_f32, "qv2x_conv3x3_f32")
    keep = []
    for i, l in enumerate(case.layers):
        d = L.F32ConvDesc()
        d.n, d.h, d.w, d.cin_total, d.cin0, d.cin, d.stride, d.cout = case.n, l.h, l.w, l.cin_total, l.cin0, l.cin, l.stride, l.cout
        d.out_ctotal, d.out_c0, d.relu = prep.expect.shape[-1], prep.c0[i], case.relu
        xt, wt, bt = (torch.from_numpy(a).to(dev) for a in (prep.xpad[i], prep.packed[i], prep.bias[i]))
        keep += [xt, wt, bt]
        L.check(fn(C.byref(d), L.ptr(xt), L.ptr(wt), L.ptr(bt), L.ptr(out), L.current_stream()), name)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits; first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]!r} against {want[bad][0]!r}")


def gemm_check(prep, got, what):
    """the sentinel in the pad ring and the spare channels, the windows equal to the oracle bit for bit"""
    case = prep.case
    last = prep.c0[-1] + case.layers[-1].cout
    for name, part in (("top row", got[:, 0]), ("bottom row", got[:, -1]), ("left column", got[:, :, 0]), ("right column", got[:, :, -1])):
        assert (part == SENT).all(), f"{what}: pad ring written ({name})"
    assert (got[..., :case.front] == SENT).all(), f"{what}: channels in front of the window written"
    assert (got[..., last:] == SENT).all(), f"{what}: channels behind the window written"
    assert not np.isnan(got).any(), f"{what}: NaN in the output (a read outside the input channel window)"
    same_bits(got, prep.expect, f"{what}: the windows against orc_gemm_f32")


# ---- PFN ------------------------------------------------------------------------------------------------------------------------------------

PFN_N, PFN_NY, PFN_NX = 2, 4, 6
PFN_VOX = np.array([0.4, 0.4, 4.0], np.float32)
PFN_OFF = np.array([-1.0, -0.6, -1.0], np.float32)         # centre of voxel 0 (voxel / 2 + range minimum)
CH_MASKED, CH_DEAD = 3, 7                                  # channel 3: only a masked slot can win; channel 7: every value negative


def pfn_weights(rng):
    """Linear(10 -> 64) with folded BN.  Channel CH_MASKED reads only the (positive) intensity with weight -1 and has bias +0.5: every real
    point gives less than the bias, so a pillar with a masked slot returns exactly the bias and a full pillar less.  Channel CH_DEAD has
    bias -100: every value is negative and the output exactly 0."""
    w = (rng.standard_normal((64, 10)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(64) * 0.3).astype(np.float32)
    w[CH_MASKED] = 0.0
    w[CH_MASKED, 3] = -1.0
    b[CH_MASKED] = 0.5
    b[CH_DEAD] = -100.0
    return w, b


class Pfn:
    """pillars: list of (b, z, y, x, np) -- np the REPORTED point count; slots past min(np, P) are zero"""

    def __init__(self, aim, P, pillars, seed):
        self.aim, self.P, self.pillars, self.seed = aim, P, pillars, seed


def _cells(count, skip=()):
    """``count`` distinct in-canvas cells (b, y, x), none of ``skip``"""
    cells = [(b, y, x) for b in range(PFN_N) for y in range(PFN_NY) for x in range(PFN_NX) if (b, y, x) not in skip]
    assert count <= len(cells)
    step = len(cells) // count
    return cells[::step][:count]


def _plain(count, P, nps=None):
    return [(b, 0, y, x, (nps[i] if nps else 1 + (i * 3) % P)) for i, (b, y, x) in enumerate(_cells(count))]


_LAST = PFN_N - 1
_CORNERS = [(_LAST, 0, 0), (_LAST, 0, PFN_NX - 1), (_LAST, PFN_NY - 1, 0), (_LAST, PFN_NY - 1, PFN_NX - 1)]
_OUTSIDE = [(-1, 0, 1, 1), (PFN_N, 0, 1, 1), (0, 0, -1, 2), (0, 0, PFN_NY, 2), (0, 0, 2, -1), (0, 0, 2, PFN_NX), (0, 1, 2, PFN_NX - 1), (0, -1, 2, 0)]
PFN_CASES = {
    "m1_p1": Pfn("M = 1 (three idle waves), P = 1: a full one-point pillar", 1, _plain(1, 1), 41),
    "m5_p5": Pfn("M = 5: a second workgroup with one pillar; P = 5", 5, _plain(5, 5), 42),
    "m9_p32": Pfn("M = 9: a third workgroup with one pillar; P = 32", 32, _plain(9, 32, [1, 32, 7, 31, 2, 32, 16, 40, 5]), 43),
    # pillar 0: one point; 1: full; 2: np > P (mean over 9, sums over 5 slots); 3: z = 1, lands at x + 1; 4-7: the corners of the last agent;
    # 8-15: outside the canvas on every side (b, y, z + x; the last two through z) -- they write nothing
    "edges_p5": Pfn("one point, full, np > P, z = 1, the last agent's corners, eight pillars outside the canvas", 5,
                    [(0, 0, 1, 1, 1), (0, 0, 1, 3, 5), (0, 0, 2, 2, 9), (0, 1, 3, 2, 3)] + [(b, 0, y, x, 2 + i) for i, (b, y, x) in enumerate(_CORNERS)]
                    + [(b, z, y, x, 3) for (b, z, y, x) in _OUTSIDE], 44),
}


def pfn_inside(p):
    b, z, y, x = p[:4]
    return 0 <= b < PFN_N and 0 <= y < PFN_NY and 0 <= z + x < PFN_NX


class PfnPrepared:
    def __init__(self, case):
        from oracle.spec import _p, lib as olib
        self.case = case
        rng = np.random.default_rng(7000 + case.seed)
        m, P = len(case.pillars), case.P
        self.w, self.b = pfn_weights(rng)
        self.coords = np.array([p[:4] for p in case.pillars], np.int32).reshape(m, 4)
        self.npts = np.array([p[4] for p in case.pillars], np.int32)
        self.vf = np.zeros((m, P, 4), np.float32)
        for i, (b, z, y, x, npt) in enumerate(case.pillars):
            real = min(npt, P)
            centre = np.array([x * 0.4 - 1.0, y * 0.4 - 0.6, z * 4.0 - 1.0])
            pts = centre + rng.uniform(-0.5, 0.5, (real, 3)) * PFN_VOX
            self.vf[i, :real, :3] = pts
            self.vf[i, :real, 3] = rng.uniform(0.05, 1.0, real)              # intensity, positive
        self.feats = np.zeros((m, 64), np.float32)
        olib().orc_pfn_f32(_p(self.vf), _p(self.coords), _p(self.npts), m, P, _p(self.w), _p(self.b), _p(PFN_VOX), _p(PFN_OFF), _p(self.feats))
        self.cells = [(b, y + 1, z + x + 1) for (b, z, y, x, _n) in case.pillars if pfn_inside((b, z, y, x))]
        assert len(set(self.cells)) == len(self.cells), "two pillars share a cell: the kernel's order between waves is not defined"

    def canvas(self, fill):
        """the expected padded canvas after a launch into one full of ``fill``"""
        out = np.full((PFN_N, PFN_NY + 2, PFN_NX + 2, 64), fill, np.float32)
        for i, p in enumerate(self.case.pillars):
            if pfn_inside(p):
                b, z, y, x = p[:4]
                out[b, y + 1, z + x + 1] = self.feats[i]
        return out


def pfn_ref64(prep):
    """PillarVFE in float64 (pillar_vfe.py:105-155 with BN folded): ten features, the mean over all P slots divided by the reported count,
    Linear, zero-masked slots contribute the bias, max over the slots, ReLU.  Returns (y [M][64], bound [M][64]): the fp32 chain's
    (10 + 2) 2^-24 (sum_k |f_k w_k| + |b|) plus what the fp32 features themselves carry into it, sum_k |w_k| df_k with
    df = 2^-24 ((real + 1) sum_p |x_p| / np + |x - mean|) for the mean features and 2^-24 (2 (|c vox| + |off|) + |x - centre|) for the centre features."""
    vf, w, b = prep.vf.astype(np.float64), prep.w.astype(np.float64), prep.b.astype(np.float64)
    vox, off = PFN_VOX.astype(np.float64), PFN_OFF.astype(np.float64)
    m, P = vf.shape[:2]
    y, bound = np.zeros((m, 64)), np.zeros((m, 64))
    u = 2.0 ** -24
    for i in range(m):
        npt = int(prep.npts[i])
        real = min(npt, P)
        xyz = vf[i, :, :3]
        mean = xyz.sum(axis=0) / npt
        dmean = u * (real + 1) * np.abs(xyz).sum(axis=0) / npt
        bz, z, yy, x = (int(v) for v in prep.coords[i])
        cidx = np.array([x, yy, z], np.float64)
        centre = cidx * vox + off
        dcentre = u * 2 * (np.abs(cidx * vox) + np.abs(off))
        best, bbound = np.full(64, -np.inf), np.zeros(64)
        for p in range(P):
            if p < real:
                f = np.concatenate([vf[i, p], xyz[p] - mean, xyz[p] - centre])
                df = np.concatenate([np.zeros(4), dmean + u * np.abs(xyz[p] - mean), dcentre + u * np.abs(xyz[p] - centre)])
                val = w @ f + b
                vb = 12 * u * (np.abs(w) @ np.abs(f) + np.abs(b)) + np.abs(w) @ df
            else:
                val, vb = b.copy(), np.zeros(64)
            best, bbound = np.maximum(best, val), np.maximum(bbound, vb)
        y[i], bound[i] = np.maximum(best, 0.0), bbound
    return y, bound


def pfn_launch(prep, fill):
    import torch
    from quantv2x_amd import lib as L
    lib, dev = L.load(), torch.device("cuda", 0)
    canvas = torch.full((PFN_N, PFN_NY + 2, PFN_NX + 2, 64), float(fill), dtype=torch.float32, device=dev)
    vf, co, npt = (torch.from_numpy(a).to(dev) for a in (prep.vf, prep.coords, prep.npts))
    fp = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
    hold = [np.ascontiguousarray(a, dtype=np.float32) for a in (prep.w, prep.b, PFN_VOX, PFN_OFF)]
    L.check(lib.qv2x_pfn_scatter_f32(L.ptr(vf), L.ptr(co), L.ptr(npt), len(prep.case.pillars), prep.case.P, *[fp(a) for a in hold], L.ptr(canvas),
                                     PFN_N, PFN_NY, PFN_NX, L.current_stream()), "qv2x_pfn_scatter_f32")
    torch.cuda.synchronize()
    return canvas.cpu().numpy()


# ---- add_relu, occ_sigmoid ------------------------------------------------------------------------------------------------------------------

ADD_RELU_COUNTS = (4, 1020, 1024, 1028)


def add_relu_operands(count, seed=51):
    """(a, b): random values of magnitudes 1e-3 .. 1e30 with exact cancellation, -0.0 + -0.0, +-inf against finite values, inf + inf and sums
    that overflow; never inf - inf (fmaxf and np.maximum disagree on NaN, and no engine produces one)"""
    rng = np.random.default_rng(7000 + seed + count)
    a = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(np.float32)
    b = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(np.float32)
    special = [(1.5, -1.5), (-0.0, -0.0), (np.inf, 1.0), (-np.inf, 1.0), (0.0, -0.0), (np.inf, np.inf), (-np.inf, -np.inf), (3e38, 3e38),
               (-3e38, -3e38), (1e30, -1e30), (1e30, 1.0), (-1e-30, 1e-30)]
    for i, (u, v) in enumerate(special[:count]):
        a[(i * 89) % count if count > 16 else i % count], b[(i * 89) % count if count > 16 else i % count] = u, v
    return a, b


def add_relu_launch(a, b, tail=8):
    """returns (out[:count], the ``tail`` floats behind it, which were SENT before the launch)"""
    import torch
    from quantv2x_amd import lib as L
    lib, dev = L.load(), torch.device("cuda", 0)
    out = torch.full((a.size + tail,), float(SENT), dtype=torch.float32, device=dev)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    L.check(lib.qv2x_add_relu_f32(L.ptr(at), L.ptr(bt), L.ptr(out), a.size, L.current_stream()), "qv2x_add_relu_f32")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got[:a.size], got[a.size:]


OCC_SHAPES = {"n2_3x5_c64": (2, 3, 5, 64), "n1_1x257_c4": (1, 1, 257, 4)}       # 257 cells: a second workgroup with one thread
OCC_VALUES = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e30, -1e30]


def occ_operands(n, h, w, ct, seed=61):
    """padded map [n][h+2][w+2][ct]: NaN in the ring and in channels 1..; channel 0 of the interior holds OCC_VALUES, then N(0, 4)"""
    rng = np.random.default_rng(7000 + seed)
    v = (rng.standard_normal(n * h * w) * 4.0).astype(np.float32)
    at = rng.permutation(n * h * w)[:len(OCC_VALUES)]
    v[at] = np.array(OCC_VALUES, np.float32)
    x = np.full((n, h + 2, w + 2, ct), np.nan, np.float32)
    x[:, 1:-1, 1:-1, 0] = v.reshape(n, h, w)
    return x, v


def occ_score64(v):
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-v.astype(np.float64))) + 1e-4).astype(np.float32)


def occ_launch(x, n, h, w, ct, tail=8):
    import torch
    from quantv2x_amd import lib as L
    lib, dev = L.load(), torch.device("cuda", 0)
    occ = torch.full((n * h * w + tail,), float(SENT), dtype=torch.float32, device=dev)
    score = torch.full((n * h * w + tail,), float(SENT), dtype=torch.float32, device=dev)
    xt = torch.from_numpy(x).to(dev)
    L.check(lib.qv2x_occ_sigmoid_f32(L.ptr(xt), n, h, w, ct, L.ptr(occ), L.ptr(score), L.current_stream()), "qv2x_occ_sigmoid_f32")
    torch.cuda.synchronize()
    return occ.cpu().numpy(), score.cpu().numpy()


# ---- decode ---------------------------------------------------------------------------------------------------------------------------------

class Decode:
    """layout "engine": level_stride = agents * hw, agent_stride = hw;  "agent_major": agent_stride = levels * level_stride + 3,
    level_stride = hw + 2 (gaps between the planes, filled with valid codes that no row may use)"""

    def __init__(self, aim, d, levels, kc, agents, hw, layout, seed):
        self.aim, self.d, self.levels, self.kc, self.agents, self.hw, self.layout, self.seed = aim, d, levels, kc, agents, hw, layout, seed
        if layout == "engine":
            self.level_stride, self.agent_stride = agents * hw, hw
        else:
            self.level_stride = hw + 2
            self.agent_stride = levels * self.level_stride + 3
        self.work = agents * hw * (d // 4)


DECODE_CASES = {
    "d4_l1_kc1": Decode("one float4 per row, one level, one entry: every code is 0 = kc - 1", 4, 1, 1, 1, 7, "engine", 71),
    "d64_l3_kc128": Decode("the engines' shape on a 21-cell map, two agents: 672 work items", 64, 3, 128, 2, 21, "engine", 72),
    "d68_l16_kc256_agent_major": Decode("d = 68 (rows not a multiple of 64 bytes), 16 levels, agent-major planes with gaps: 255 work items",
                                        68, 16, 256, 3, 5, "agent_major", 73),
    "d256_l3_kc256": Decode("d = 256, one agent, three cells: 192 work items", 256, 3, 256, 1, 3, "engine", 74),
    "d64_l3_kc128_agent_major": Decode("the engines' shape in the agent-major layout, 1040 work items", 64, 3, 128, 5, 13, "agent_major", 75),
}


class DecodePrepared:
    def __init__(self, case):
        self.case = c = case
        rng = np.random.default_rng(7000 + c.seed)
        self.lut = (rng.standard_normal((c.levels, c.kc, c.d)) * 10.0 ** rng.uniform(-3, 3, (c.levels, c.kc, c.d))).astype(np.float32)
        self.bias = (rng.standard_normal(c.d) * 10.0 ** rng.uniform(-3, 3, c.d)).astype(np.float32)
        size = (c.agents - 1) * c.agent_stride + (c.levels - 1) * c.level_stride + c.hw
        self.codes = rng.integers(0, c.kc, size=size + 5, dtype=np.uint8) if c.kc < 256 else rng.integers(0, 256, size=size + 5).astype(np.uint8)
        self.idx = np.zeros((c.agents, c.hw, c.levels), np.int64)
        k = 0
        for ag in range(c.agents):
            for l in range(c.levels):
                base = ag * c.agent_stride + l * c.level_stride
                self.codes[base + (k % c.hw)] = 0 if (k // c.hw + k) % 2 == 0 else c.kc - 1             # both ends of the table in every plane
                k += 1
                self.idx[ag, :, l] = self.codes[base:base + c.hw]

    def want(self, order=None):
        """((bias + T0[c0]) + T1[c1]) + ... in numpy fp32; ``order``: another order of the levels"""
        c = self.case
        v = np.broadcast_to(self.bias, (c.agents, c.hw, c.d)).astype(np.float32)
        for l in (range(c.levels) if order is None else order):
            v = (v + self.lut[l][self.idx[:, :, l]]).astype(np.float32)
        return v.reshape(c.agents * c.hw, c.d)


def decode_launch(prep, tail=8):
    import torch
    from quantv2x_amd import lib as L
    c = prep.case
    lib, dev = L.load(), torch.device("cuda", 0)
    out = torch.full((c.agents * c.hw * c.d + tail,), float(SENT), dtype=torch.float32, device=dev)
    ct, lt, bt = (torch.from_numpy(a).to(dev) for a in (prep.codes, prep.lut, prep.bias))
    L.check(lib.qv2x_codebook_decode_f32(L.ptr(ct), c.agent_stride, c.level_stride, c.agents, c.hw, c.levels, c.kc, c.d, L.ptr(lt), L.ptr(bt), L.ptr(out),
                                         L.current_stream()), "qv2x_codebook_decode_f32")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got[:-tail].reshape(c.agents * c.hw, c.d), got[-tail:]
