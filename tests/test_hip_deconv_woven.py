"""The pixel-stationary deblock items of csrc/deconv_f32.hip with MORE THAN ONE pair of column tiles, bit for bit against orc_deconv /
orc_deconv_f32in.  Written for a form of the pair loop that ran the epilogue of pair P (bias, quantizer, v_permlane32_swap, store) inside
the K loop of pair P + 1 out of a second accumulator set (profiles/r10_deconv_woven.md: bit-exact on these cases, not faster, not kept);
they are what any change to the pair loop has to pass: the tiles' channel, sub-position and bias step from pair to pair inside an item.
tests/test_hip_deblock_layers.py has the edges of the launch rule and of the quantizers on items of one and two pairs; here:

  * for Cin 64 (two pixel tiles per item), 128 and 256: items of 1, 2, 4 and 8 pairs;
  * pixel counts of 32 MT k + 1 and exact multiples: the lanes past the end stay silent in every pair;
  * a pair that straddles the channel wrap and a sub-position (Cout 96, s = 2: tiles 2 | 3 sit at channel 64 of one sub-position |
    channel 0 of the next), and Cout 32 with s = 4 and s = 2, where every tile is its own sub-position: a channel, a sub-position or a
    bias taken from the wrong pair shows in the bytes;
  * ReLU with zp 0 and zp 7, no ReLU with zp 128; every window sits at a channel offset behind spare channels;
  * Cin 64 + 128 + 256 in one launch, given in rising Cin (the host reorders), into two destinations;
  * the fp32-map entry for Cin 64 and 128 with two pairs per item.

**How the pairs per item are reached.**  The host takes 8 pairs per item only while the launch has >= 2560 items (_deblock_layers.launch_plan
restates the rule; every case asserts its form and pairs through it).  A single layer of 8-pair items then costs the CPU oracle 2560 x 8 x
2048 x Cin multiply-adds: 10 s at Cin 256.  So the int8 cases are batches of TWO layers: the layer under test and a filler, 64 -> 192
channels with s = 1 (three pairs, odd: one pair per item whatever the cap), whose 2592 / 2979 items hold the cap at 8; the layer under
test then has min(8, largest power of two in its pairs) pairs per item on a few thousand pixels.  The fp32-map entry takes one layer: two
pairs per item at 2560 items.  A layer's operands and oracle codes are computed once per process and shared by the cases that use them.

Needs an MI355X."""
import numpy as np
import pytest

from _deblock_layers import (BACK, DX, FRONT, SENT, X_STD_F32, Case, assert_plan, check_outputs, deblock_layer, launch, live, oracle_codes,
                             out_step)

pytestmark = pytest.mark.gpu

# output maps (n = 1): EXACT -- 192 x 288, the pixel counts 55296 (s = 1) | 13824 (s = 2) | 3456 (s = 4) are multiples of 64;
# TAIL -- 252 x 252: 63504 = 64 x 992 + 16 | 15876 = 64 x 248 + 4 | 3969 = 64 x 62 + 1
EXACT, TAIL = (192, 288), (252, 252)
FILLER = (64, 192, 1)
Q_RELU0, Q_RELU7, Q_PLAIN = dict(relu=1, zp=0), dict(relu=1, zp=7), dict(relu=0, zp=128)


def _case(layer, hw, np_, quant):
    """the layer under test (cin, cout, s) and the filler on one H x W output map"""
    (cin, cout, s), (H, W) = layer, hw
    return Case([(cin, cout, s, H // s, W // s), FILLER + (H, W)], 1, "ps", [np_, 1], **quant)


CASES = {}
for _cin in (64, 128, 256):
    CASES[f"cin{_cin}_np1_exact"] = _case((_cin, 64, 1), EXACT, 1, Q_RELU0)
    # Cout 32, s = 2: an item is all four sub-positions, one per tile; 15876 pixels: the last item of Cin 64 has a dead second pixel tile
    CASES[f"cin{_cin}_np2_tail"] = _case((_cin, 32, 2), TAIL, 2, Q_RELU7)
    CASES[f"cin{_cin}_np4_exact"] = _case((_cin, 64, 2), EXACT, 4, Q_PLAIN)
    # Cout 32, s = 4: sixteen tiles, sixteen sub-positions; 3969 = 32 MT k + 1 pixels for both MT
    CASES[f"cin{_cin}_np8_tail"] = _case((_cin, 32, 4), TAIL, 8, Q_RELU0)
# the workload's own level-2 deblock: four items of eight pairs per pixel tile, every pair inside one sub-position
CASES["cin256_cout128_s4_np8"] = _case((256, 128, 4), EXACT, 8, Q_PLAIN)
CASES["cin128_cout128_s4_np8_tail"] = _case((128, 128, 4), TAIL, 8, Q_RELU7)
# six pairs, two per item: item 0's tiles are channels 0 | 32 | 64 of sub-position 0 and 0 of sub-position 1 -- its second pair straddles;
# item 1 starts at channel 32 of sub-position 1 and runs into sub-position 2 = (1, 0)
CASES["cin64_straddle_np2"] = _case((64, 96, 2), TAIL, 2, Q_RELU7)
CASES["cin256_straddle_np2"] = _case((256, 96, 2), EXACT, 2, Q_PLAIN)
# the three Cin in one launch, rising (the host sorts by falling Cin), two destinations; 236 x 460 outputs: 1697 + 849 + 213 x 1 items
# = 2759 >= 2560 keep the cap at 8; 6785 = 64 x 106 + 1 pixels at s = 4
CASES["three_deblocks"] = Case([(64, 64, 1, 236, 460), (128, 32, 2, 118, 230), (256, 32, 4, 59, 115)], 1, "ps", [1, 2, 8], dests=[0, 1, 0], **Q_RELU7)

F32_CASES = {
    # 2561 | 2561 items of two pairs (four sub-positions); 81921 = 32 x 2560 + 1, 163905 = 64 x 2561 + 1
    "cin128_np2": Case([(128, 32, 2, 249, 329)], 1, "ps", [2], f32in=True, **Q_RELU7),
    "cin64_np2": Case([(64, 32, 2, 245, 669)], 1, "ps", [2], f32in=True, **Q_PLAIN),
}

_LAYERS = {}


def _layer(layer, case):
    """(x, packed weights, bias, expected int8 window) of one layer under the case's quantizer: drawn and run through the oracle once"""
    key = (layer, case.n, case.relu, case.zp, case.zx, case.f32in)
    if key not in _LAYERS:
        cin, cout, s, h, w = layer
        rng = np.random.default_rng([cin, cout, s, h, w, case.relu, case.zp])
        da = out_step(1.0, case.zp, case.relu)
        if case.f32in:
            x = (rng.standard_normal((case.n, h, w, cin)) * X_STD_F32).astype(np.float32)
            wdeq, bias, packed = deblock_layer(rng, cin, cout, s, 1.0, X_STD_F32)
        else:
            x = rng.integers(0, 256, size=(case.n, h, w, cin), dtype=np.uint8)
            wdeq, bias, packed = deblock_layer(rng, cin, cout, s)
        want = oracle_codes(x, wdeq, bias, s, case.relu, da, case.zp, DX, case.zx)
        norelu = oracle_codes(x, wdeq, bias, s, 0, da, case.zp, DX, case.zx) if case.relu and case.zp > 0 else None
        live(want, case.relu, case.zp, norelu)
        _LAYERS[key] = (x, packed, bias, (want.astype(np.int16) - 128).astype(np.int8))
    return _LAYERS[key]


class Operands:
    """what _deblock_layers.launch and check_outputs read of a Prepared, assembled from the shared layers"""

    def __init__(self, case):
        self.case, self.da = case, out_step(1.0, case.zp, case.relu)
        ndest = max(case.dests) + 1
        ctot = [FRONT + sum(l[1] for l, d in zip(case.layers, case.dests) if d == k) + BACK for k in range(ndest)]
        self.expect = [np.full((case.n, case.H + 2, case.W + 2, c), SENT, np.int8) for c in ctot]
        self.windows = [[] for _ in range(ndest)]
        self.x, self.packed, self.bias, self.c0 = [], [], [], []
        nxt = [FRONT] * ndest
        for layer, dst in zip(case.layers, case.dests):
            x, packed, bias, want = _layer(layer, case)
            c0, cout = nxt[dst], layer[1]
            nxt[dst] += cout
            self.expect[dst][:, 1:-1, 1:-1, c0:c0 + cout] = want
            self.windows[dst].append((c0, cout))
            self.x.append(x); self.packed.append(packed); self.bias.append(bias); self.c0.append(c0)


@pytest.mark.parametrize("name", list(CASES))
def test_woven_i8(name):
    case = CASES[name]
    assert_plan(case)
    prep = Operands(case)
    check_outputs(prep, launch(prep, "batch"), "qv2x_deconv_i8_batch")


@pytest.mark.parametrize("name", list(F32_CASES))
def test_woven_f32in(name):
    case = F32_CASES[name]
    assert_plan(case)
    prep = Operands(case)
    check_outputs(prep, launch(prep, "f32in"), "qv2x_deconv_f32in")
