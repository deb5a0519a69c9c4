"""The three entries of csrc/pyramid_fuse.hip -- qv2x_pyramid_weighted_fuse_f32, _f32p and _i8 -- at their edges against
``oracle.geometry.weighted_fuse`` within FUSE_TOL (cases, operands and checks in tests/_weighted_fuse_cases.py; what each case is aimed at is
asserted on the reference by tests/test_weighted_fuse_cases_cpu.py).  tests/test_pyramid_fuse.py runs the reference project's own vectors
through the unpadded entry with ego = 0; here:

  * every case runs through ALL THREE entries; _f32 and _f32p must be bit-equal to each other;
  * identity (1 x 1, 16 x 1, 4 x 8): the output equals the input, for _i8 the dequantized codes, bit for bit;
  * whole-cell, half-cell and out-of-view translations; 90 and 180 degrees on a non-square map with h_metres != w_metres and
    discrete_ratio != 1;
  * 1, 2, 5 and 8 agents with max_cav 5 and 8, ego = 1 and ego = agents - 1;
  * 1 x 1, 3 x 7 (a tail of 5 cells), 16 x 1 and 5 x 16 maps; 64, 128, 192, 256, 320 and 512 channels (192: the count whose lane mapping
    ran past the per-cell records before it was fixed);
  * score maps with exact zeros (masked although visible; cells masked for every agent come back as exactly 0, not untouched), scores
    1.0001 against 1e-4;
  * _i8: in_zx 0, 128 and 255 with the bytes -128 and 127 present.

Every destination is allocated full of a sentinel; the padded entry's ring must keep it, and its input ring holds NaN.  Needs an MI355X."""
import numpy as np
import pytest

from _weighted_fuse_cases import CASES, SENT, Prepared, check, launch, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_weighted_fuse_all_entries(name):
    prep = Prepared(CASES[name])
    c = prep.case
    plain = launch(prep, "f32")
    check(prep, plain, prep.want, f"{name}: qv2x_pyramid_weighted_fuse_f32")
    padded = launch(prep, "f32p")
    ring = np.ones(padded.shape[:2], bool)
    ring[1:-1, 1:-1] = False
    assert (padded[ring] == SENT).all(), f"{name}: qv2x_pyramid_weighted_fuse_f32p wrote its pad ring"
    check(prep, padded[1:-1, 1:-1], prep.want, f"{name}: qv2x_pyramid_weighted_fuse_f32p")
    same_bits(padded[1:-1, 1:-1], plain, f"{name}: the padded entry against the unpadded one")
    codes = launch(prep, "i8")
    check(prep, codes, prep.want_i8, f"{name}: qv2x_pyramid_weighted_fuse_i8")
    if c.identity:
        same_bits(plain, prep.x[0], f"{name}: identity, fp32 features")
        same_bits(codes, prep.xdq[0], f"{name}: identity, dequantized codes")
