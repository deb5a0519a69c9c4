"""The entries of csrc/fp32_path.hip and qv2x_codebook_decode_f32 called directly at their edges (cases, operands, references and checks in
tests/_fp32_kernels.py; the references are pinned and every case's aim is asserted by tests/test_fp32_kernels_cpu.py).
tests/test_hip_fp32.py and tests/test_hip_pyramid_fp32.py reach these kernels only through whole models.

  * qv2x_conv3x3_f32 / qv2x_deconv_f32: bit for bit against ``orc_gemm_f32``.  M = 1, 15, 32, 33, a row tile over two images, tile counts that
    leave waves idle; stride 2 on 4 x 6, 5 x 7, 1 x 1 and 2 x 1 maps; cin 8, 24, 64; an input window at cin0 = 12 of 40 channels with NaN
    around it; 64, 128 and 192 columns; out_c0 = 0, 4 and 5; the centre-tap shortcut and the grouped slabs of the Pyramid engine;
    deconvolutions with s = 1, 2, 3, 4, 8 whose 32-column spans hold one, two, eight and thirty-two sub-positions, two layers into one
    destination.  Destinations are full of a sentinel: the pad ring and the spare channels must keep it.
  * qv2x_pfn_scatter_f32: bit for bit against ``orc_pfn_f32`` + the scatter, into a zero-filled canvas as the engine allocates it and into
    one full of a sentinel; M = 1, 5, 9, P = 1, 5, 32, np > P, z = 1, the last agent's corners, pillars outside the canvas on every side.
  * qv2x_add_relu_f32 at 4, 1020, 1024, 1028 floats with cancellation, signed zeros, infinities and overflow; equal to
    ``np.maximum(a + b, 0)`` by value.  No engine passes ``out`` aliased to an operand (engine_pyramid_fp32 alternates two buffers and the
    block's input is never its output), so no aliased case is run.
  * qv2x_occ_sigmoid_f32 on both sides of expf's overflow; qv2x_codebook_decode_f32 for d 4 .. 256, 1 .. 16 levels, both layouts.

Needs an MI355X."""
import numpy as np
import pytest

from _fp32_kernels import (ADD_RELU_COUNTS, CONV_CASES, DECODE_CASES, DECONV_CASES, OCC_SHAPES, PFN_CASES, SENT, DecodePrepared, GemmPrepared,
                           PfnPrepared, add_relu_launch, add_relu_operands, decode_launch, gemm_check, gemm_launch, occ_launch, occ_operands,
                           occ_score64, pfn_launch, same_bits)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv3x3_f32(name):
    prep = GemmPrepared(CONV_CASES[name])
    gemm_check(prep, gemm_launch(prep), f"qv2x_conv3x3_f32, {name}")


@pytest.mark.parametrize("name", list(DECONV_CASES))
def test_deconv_f32(name):
    prep = GemmPrepared(DECONV_CASES[name])
    gemm_check(prep, gemm_launch(prep), f"qv2x_deconv_f32, {name}")


@pytest.mark.parametrize("name", list(PFN_CASES))
def test_pfn_scatter_f32(name):
    prep = PfnPrepared(PFN_CASES[name])
    same_bits(pfn_launch(prep, 0.0), prep.canvas(0.0), f"qv2x_pfn_scatter_f32, {name}: the zero-filled canvas")
    same_bits(pfn_launch(prep, SENT), prep.canvas(SENT), f"qv2x_pfn_scatter_f32, {name}: the canvas full of the sentinel")


@pytest.mark.parametrize("count", ADD_RELU_COUNTS)
def test_add_relu_f32(count):
    a, b = add_relu_operands(count)
    got, tail = add_relu_launch(a, b)
    with np.errstate(over="ignore"):
        want = np.maximum(a + b, np.float32(0))
    assert (tail == SENT).all(), "written behind the end"
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", list(OCC_SHAPES))
def test_occ_sigmoid_f32(name):
    n, h, w, ct = OCC_SHAPES[name]
    x, v = occ_operands(n, h, w, ct)
    occ, score = occ_launch(x, n, h, w, ct)
    m = n * h * w
    assert (occ[m:] == SENT).all() and (score[m:] == SENT).all(), "written behind the end"
    same_bits(occ[:m], v, "occ: a copy of channel 0")
    assert np.isfinite(score[:m]).all() and (score[:m] >= np.float32(1e-4)).all()
    np.testing.assert_allclose(score[:m], occ_score64(v), rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_codebook_decode_f32(name):
    prep = DecodePrepared(DECODE_CASES[name])
    got, tail = decode_launch(prep)
    assert (tail == SENT).all(), "written behind the end"
    same_bits(got, prep.want(), f"qv2x_codebook_decode_f32, {name}")
