"""The row bands of the sharded post stage (``AgentShardedModel(ego_only=True, shard_post=True)``) as pure Python: which rows a rank
computes, the fixed slab layout of the second all-gather, the plain-torch assembly, and the argument errors of the mode."""
import numpy as np
import pytest
import torch

from quantv2x_amd.dist import (AgentShardedModel, assemble_bands_reference, band_cells_cap, band_payload_layout, band_rows)


@pytest.mark.parametrize("h", [16, 100, 256])
def test_band_rows_cover_the_map(h):
    for world in list(range(1, 9)) + [h + 3, 3 * h]:                        # (world > h: some bands are empty)
        w = 7
        bands = [band_rows(h, world, r) for r in range(world)]
        assert bands[0][0] == 0 and bands[-1][1] == h
        for r, (y0, y1) in enumerate(bands):
            assert (y0, y1) == (r * h // world, (r + 1) * h // world) and 0 <= y0 <= y1 <= h
            if r:
                assert y0 == bands[r - 1][1]                                # contiguous, ordered, disjoint
            assert (y1 - y0) * w <= band_cells_cap(h, w, world)
        assert sum(y1 - y0 for y0, y1 in bands) == h
        assert band_cells_cap(h, w, world) == -(-h // world) * w
        if world > h:
            assert any(y0 == y1 for y0, y1 in bands) and band_cells_cap(h, w, world) == w


def test_slab_layout_sizes():
    # V2X-Real feature map 100 x 352, multi-class heads (72 channels), 32 frames, two ranks
    assert band_payload_layout(32, 72, 100, 352, 2, "f32") == (50 * 352, 32 * 72 * 50 * 352 * 4)
    assert band_payload_layout(32, 72, 100, 352, 2, "u8") == (50 * 352, 32 * 72 * 50 * 352)
    assert band_payload_layout(32, 72, 100, 352, 2) == band_payload_layout(32, 72, 100, 352, 2, "f32")
    # the capacity is the LARGEST band's (100 rows over 8 ranks: 12 or 13), every rank sends the same bytes
    assert band_payload_layout(1, 20, 100, 352, 8, "u8") == (13 * 352, 20 * 13 * 352)
    # padded up to a multiple of 16
    cap, nbytes = band_payload_layout(1, 3, 5, 3, 2, "u8")
    assert cap == 9 and nbytes == 32 and band_payload_layout(1, 3, 5, 3, 2, "f32") == (9, 112)
    with pytest.raises(ValueError):
        band_payload_layout(1, 3, 5, 3, 2, "f16")


def _cut(full, world, wire, da=None, za=None):
    """a map [frames, cout, h, w] cut into the ranks' slabs (numpy), codes for the u8 wire"""
    frames, cout, h, w = full.shape
    _, nbytes = band_payload_layout(frames, cout, h, w, world, wire)
    slabs = np.full((world, nbytes), 0xA5, np.uint8)                           # (padding is never read)
    for r in range(world):
        y0, y1 = band_rows(h, world, r)
        band = np.ascontiguousarray(full[:, :, y0:y1])
        raw = band.astype(np.uint8).tobytes() if wire == "u8" else band.astype(np.float32).tobytes()
        slabs[r, :len(raw)] = np.frombuffer(raw, np.uint8)
    return torch.from_numpy(slabs)


@pytest.mark.parametrize("world", [1, 2, 3, 8, 11])
@pytest.mark.parametrize("shape", [(2, 5, 9, 6), (1, 20, 16, 12)])
def test_reference_assembly(world, shape):
    g = np.random.default_rng(world)
    frames, cout, h, w = shape
    full = g.standard_normal(shape).astype(np.float32)
    got = assemble_bands_reference(_cut(full, world, "f32"), frames, cout, h, w, world, "f32")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), full)
    codes = g.integers(0, 256, shape).astype(np.uint8)
    da = g.uniform(0.01, 0.3, cout).astype(np.float32)
    za = g.integers(0, 256, cout).astype(np.float32)
    want = (codes.astype(np.float32) - za[None, :, None, None]) * da[None, :, None, None]      # one fp32 subtract, one fp32 multiply
    got = assemble_bands_reference(_cut(codes, world, "u8"), frames, cout, h, w, world, "u8", torch.from_numpy(da), torch.from_numpy(za))
    assert np.array_equal(got.numpy(), want)
    with pytest.raises(ValueError):
        assemble_bands_reference(_cut(full, world, "f32")[:, :-16], frames, cout, h, w, world, "f32")


class _Eng:
    has_codebook = True

    def __init__(self, u8):
        self.u8 = u8

    def wire_shape(self):
        return 3, 12

    def head_wire_supported(self, wire):
        return wire == "f32" or self.u8


def test_mode_argument_errors():
    with pytest.raises(ValueError, match="ego_only"):
        AgentShardedModel(_Eng(True), shard_post=True)
    with pytest.raises(ValueError, match="band_wire"):
        AgentShardedModel(_Eng(True), ego_only=True, shard_post=True, band_wire="f16")
    with pytest.raises(ValueError, match="cannot serve"):
        AgentShardedModel(_Eng(False), ego_only=True, shard_post=True, band_wire="u8")
    for wire in ("f32", "u8"):
        m = AgentShardedModel(_Eng(True), ego_only=True, shard_post=True, band_wire=wire)
        assert m.shard_post and m.band_wire == wire
    m = AgentShardedModel(_Eng(False), ego_only=True, shard_post=True)
    assert m.band_wire == "f32"
    assert not AgentShardedModel(_Eng(True), ego_only=True).shard_post          # opt-in
