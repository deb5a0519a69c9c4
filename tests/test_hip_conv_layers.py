"""The dense 3x3 W8A8 convolution kernels (csrc/conv_i8.hip, conv_i8_wide.hip, conv_i8_ws.hip, conv_i8_ws2.hip, conv_i8_chain.hip) at their
edges, through qv2x_conv3x3_i8, qv2x_conv3x3_i8_wide and qv2x_conv3x3_i8_chain64, bit for bit against orc_conv3x3 (itself pinned against
float64 numpy in tests/test_conv_layers_cpu.py).  tests/test_hip_conv_wide.py and tests/test_hip_conv_chain.py run the workload's own sizes
with relu = 1, out_c0 = 0 and groups that fill the tensor; here (cases, operands and checks in tests/_conv_layers.py):

  * relu = 0 (the two-sided quantizer, zp 120 and 64) beside relu = 1 with zp 7 and 0, in every epilogue -- the chain entry included;
  * the output channel window: out_c0 = 16 in a destination with 16 spare channels in front and 32 behind, allocated full of a sentinel
    that the pad ring and the spare channels must still hold;
  * input groups anywhere in cin_total -- a non-zero offset of the one group (cin_off of the weights-stationary forms), groups out of channel
    order with gaps -- and random bytes in every channel outside the groups, border included;
  * every form of the three launch rules, aimed at by name through the restated rule (launch_plan), both sides of the thresholds
    wgs64 <= 256, M >= 16384, M >= 262144, patches >= 1024 and patches * cout / 256 >= 192, and for the persistent forms the items per
    workgroup: one, one or two, exactly two, two or three, idle padded items;
  * codes, zero points and K at their extremes: |T| beyond 2^24, the widest operands of __mul24.

Every case asserts ``live`` on the oracle's codes (in Prepared) before the kernel's result is looked at.  Every wide case is also compared
with the regular entry on the same descriptor.  Each case takes well under a second on the GPU; the two m192 cases (68 MB in, 10 GMAC in the
oracle) and the 512- / 1024-image weights-stationary cases are the only ones that move tens of megabytes.  Needs an MI355X."""
import numpy as np
import pytest

from _conv_layers import (CHAIN_CASES, EXTRA_CASES, EXTREME_SHAPES, EXTRA_VARIANTS, REGULAR_CASES, WIDE_CASES, Case, Prepared, PreparedChain,
                          assert_extreme_reference, check_outputs, expect_from, extreme_input, extreme_layer, launch, launch_chain,
                          launch_plan, oracle_conv, padded_input)

pytestmark = pytest.mark.gpu


def _run(case, variant):
    case.assert_plan()
    prep = Prepared(case, variant)
    xpad = padded_input(prep.rng, prep.x, prep.layer)
    regular = launch("regular", prep.layer, prep.x, xpad)
    check_outputs(regular, prep.expect, f"qv2x_conv3x3_i8 ({launch_plan('regular', case).form})")
    if case.entry == "wide":
        wide = launch("wide", prep.layer, prep.x, xpad)
        check_outputs(wide, prep.expect, f"qv2x_conv3x3_i8_wide ({case.form})")
        np.testing.assert_array_equal(wide, regular, err_msg="the wide entry vs the regular one")


def _ids(cases, extra=False):
    return [(name, v) for name, c in cases.items() for v in (EXTRA_VARIANTS if extra else c.variants)]


@pytest.mark.parametrize("name,variant", _ids(REGULAR_CASES), ids=lambda v: v if isinstance(v, str) else f"relu{v[0]}_zp{v[1]}")
def test_regular_entry(name, variant):
    _run(REGULAR_CASES[name], variant)


@pytest.mark.parametrize("name,variant", _ids(WIDE_CASES), ids=lambda v: v if isinstance(v, str) else f"relu{v[0]}_zp{v[1]}")
def test_wide_entry(name, variant):
    _run(WIDE_CASES[name], variant)


@pytest.mark.parametrize("name,variant", _ids(EXTRA_CASES, True), ids=lambda v: v if isinstance(v, str) else f"relu{v[0]}_zp{v[1]}")
def test_zero_and_off_centre_zero_points(name, variant):
    _run(EXTRA_CASES[name], variant)


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chain_entry(name):
    """the chain against the oracle layer by layer and against layer-wise qv2x_conv3x3_i8 launches; cases 1-4 without ReLU, which the entry
    had never run, with per-layer out_zp as the pad codes of the intermediate maps"""
    case = CHAIN_CASES[name]
    case.assert_plan()
    prep = PreparedChain(case)
    xpad = padded_input(np.random.default_rng(case.seed), prep.x, prep.layers[0])
    got, layerwise = launch_chain(prep.layers, prep.x, xpad, case.relu)
    for l, (m, want) in enumerate(zip(layerwise, prep.wants)):
        np.testing.assert_array_equal(m[:, 1:-1, 1:-1], expect_from(want, window=False)[:, 1:-1, 1:-1],
                                      err_msg=f"layer {l}: layer-wise qv2x_conv3x3_i8 against the oracle")
    check_outputs(got, prep.expect, "qv2x_conv3x3_i8_chain64", window=False)


@pytest.mark.parametrize("relu,zp", [(1, 7), (0, 120)])
@pytest.mark.parametrize("zx", [0, 255])
def test_extreme_codes_and_zero_points(zx, relu, zp):
    """inputs constant per image at code 0 or 255, weight codes constant per output channel at 0 or 255 with zw at the other end, zx 0 or
    255: |T| up to 9 x 1536 x 255^2 = 8.99e8, aw = 128 | -127 times window sums of up to 1.77e6.  The conditions under which the kernels are
    specified are asserted on the int64 reference (assert_extreme_reference); then every entry equals the oracle bit for bit."""
    for entry, form, c, cout, stride, (n, h, w) in EXTREME_SHAPES:
        layer = extreme_layer(c, cout, stride, relu, zp, zx)
        x = extreme_input(n, h, w, c)
        if entry == "chain":
            assert launch_plan("chain", (n, h, w, 1, stride)).form == form
        else:
            assert launch_plan(entry, Case(entry, form, (n, h, w), stride, [(0, c)], cout)).form == form
        want = oracle_conv(layer, x)
        assert_extreme_reference(layer, x, want)
        xpad = padded_input(np.random.default_rng(0), x, layer)
        what = f"{entry} {form} c {c} cout {cout} stride {stride}"
        if entry == "chain":
            got, layerwise = launch_chain([layer], x, xpad, relu)
            check_outputs(got, expect_from(want, window=False), what, window=False)
            np.testing.assert_array_equal(layerwise[0][:, 1:-1, 1:-1], got[:, 1:-1, 1:-1], err_msg=what + ": layer-wise")
            continue
        check_outputs(launch("regular", layer, x, xpad), expect_from(want), what + ": qv2x_conv3x3_i8")
        if entry == "wide":
            check_outputs(launch("wide", layer, x, xpad), expect_from(want), what + ": qv2x_conv3x3_i8_wide")
