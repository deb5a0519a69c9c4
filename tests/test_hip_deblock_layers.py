"""The deblock kernels of csrc/deconv_f32.hip at their edges, through all three entries, bit for bit against orc_deconv / orc_deconv_f32in
(themselves pinned against numpy in tests/test_deblock_layers_cpu.py).  tests/test_hip_deconv_batch.py runs the workload's own shapes;
here (cases, operands and the checks in tests/_deblock_layers.py):

  * column pairs that straddle two sub-positions (Cout an odd multiple of 32) with one and with two pairs per item, s = 3 and s = 8; two cases
    whose items step from one row of sub-positions into the next (dj carries into di inside an item);
  * pixel tails: M = 1, M < 32, a map one pixel wide, a last item whose second pixel tile is entirely past the end (Cin 64, and the
    64 x 64 wave tiles);
  * the wave form's K loop at Cin 16, 48 and 80;
  * four layers in one batch whose order the host's sort changes, into one and into two destinations; a batch that mixes a
    pixel-stationary shape with one that is not;
  * quantizers that make both clamps decide codes: ReLU with zp 0 / 7 / 64 and no ReLU with zp 128, input zero points 0 and 255.

Every int8 case runs through qv2x_deconv_i8 (32 x 32 wave tiles) AND qv2x_deconv_i8_batch; both must equal the oracle, so also each other.
Destinations are allocated full of a sentinel, with spare channels in front of and behind the windows: after every launch the pad ring and
the spare channels must still hold it.  Every case asserts, through the restated launch rule, the form and the pairs per item it was written
for, and (in Prepared) ``live`` on the oracle's codes.  Needs an MI355X."""
import numpy as np
import pytest

from _deblock_layers import F32_CASES, I8_CASES, QUANT_GRID, Prepared, assert_plan, check_outputs, launch, quant_case

pytestmark = pytest.mark.gpu


def _run_i8(case):
    assert_plan(case)
    prep = Prepared(case)
    batch = launch(prep, "batch")
    check_outputs(prep, batch, "qv2x_deconv_i8_batch")
    single = launch(prep, "single")
    check_outputs(prep, single, "qv2x_deconv_i8")
    for b, s in zip(batch, single):
        np.testing.assert_array_equal(b, s, err_msg="batch entry vs one launch per layer")


@pytest.mark.parametrize("name", list(I8_CASES))
def test_deblock_i8(name):
    _run_i8(I8_CASES[name])


@pytest.mark.parametrize("relu,zp,zx", QUANT_GRID)
@pytest.mark.parametrize("shape", ["ps", "wave"])
def test_deblock_i8_quantizers(shape, relu, zp, zx):
    _run_i8(quant_case(shape, relu, zp, zx))


@pytest.mark.parametrize("name", list(F32_CASES))
def test_deblock_f32in(name):
    case = F32_CASES[name]
    assert_plan(case)
    prep = Prepared(case)
    check_outputs(prep, launch(prep, "f32in"), "qv2x_deconv_f32in")
