"""``qv2x_bev_entry_f32`` (csrc/bev_entry.hip) against ``camera_bev.bev_entry_statement`` (itself pinned against float64 numpy in
tests/test_camera_pyramid_cpu.py): conv1's codes equal on every element, the shortcut rows equal by value, the destination's pad ring
untouched.  The shapes (tests/_bev_entry.py) cover a map smaller than a 32-pixel tile, odd sizes under stride 2, tile seams (33 and 17
columns) and K = 720; the output zero point is 7, so the ReLU is a clamp of its own; the maps hold whole channels and a region of exact zeros
and a row whose sums clamp at both ends.  Both shortcut kinds run: the 1x1 downsample on every shape, the identity copy on the stride-1
shapes with cin == cout = 64 | 128 (two 64-channel groups per pixel tile).  Needs an MI355X."""
import numpy as np
import pytest

from _bev_entry import BLOCK, COUT, SENT, SHAPES, ZP, bev_map, block_state, padded_i8

pytestmark = pytest.mark.gpu


def _run(n, cin, h, w, stride, cout, downsample, seed):
    import torch
    from quantv2x_amd.camera_bev import BevEntry, bev_entry_statement, entry_shapes
    state, x = block_state(cin, cout, downsample, seed), bev_map(n, cin, h, w, seed + 1)
    codes, (da, za), short = bev_entry_statement(x, state, BLOCK, stride)
    assert za == ZP and (codes == ZP).any() and (codes > ZP).mean() > 0.2, "the ReLU's clamp and live codes"
    assert codes.size < 4096 or codes.max() == 255, "the upper clamp"
    dev = torch.device("cuda", 0)
    ho, wo = entry_shapes(h, w, stride)
    out = torch.full((n, ho + 2, wo + 2, cout), SENT, dtype=torch.int8, device=dev)
    rows = torch.full((n * ho * wo, cout), float("nan"), dtype=torch.float32, device=dev)
    BevEntry(state, BLOCK, stride, dev)(torch.from_numpy(x).to(dev), out, rows)
    torch.cuda.synchronize()
    got, got_rows = out.cpu().numpy(), rows.cpu().numpy().reshape(short.shape)
    for name, part in (("top", got[:, 0]), ("bottom", got[:, -1]), ("left", got[:, :, 0]), ("right", got[:, :, -1])):
        assert (part == SENT).all(), f"pad ring written ({name})"
    np.testing.assert_array_equal(got, padded_i8(codes), err_msg="conv1 codes")
    assert not np.isnan(got_rows).any(), "shortcut rows left unwritten"
    np.testing.assert_array_equal(got_rows, short, err_msg="shortcut rows")


@pytest.mark.parametrize("n,cin,h,w,stride", SHAPES)
def test_bev_entry_downsample(n, cin, h, w, stride):
    _run(n, cin, h, w, stride, COUT, True, 100 + cin + h)


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 1, 1), (1, 64, 20, 20), (2, 128, 17, 33)])
def test_bev_entry_identity(n, c, h, w):
    _run(n, c, h, w, 1, c, False, 200 + c + h)
