"""The cases of tests/_weighted_fuse_cases.py checked on the reference alone, and the phase-2 lane mapping of
``pyramid_weighted_fuse_kernel`` restated in Python.  No GPU.

  * the mapping: for every accepted channel count up to 576 each (cell < 16, channel) of a workgroup is stored exactly once and no cell index
    reaches 16 (``rec[16][MAXA][PREC]``).  The rule the kernel had before -- ``lpc = min(c >> 2, 64)`` -- is restated beside it and shown to
    break exactly at 192 channels (lpc = 48 does not divide 64): 16 float4 stores past cell 15 and 240 float4 (960 float) duplicate stores;
  * identity cases: the oracle returns its input bit for bit (fp32 features and dequantized codes);
  * partial-view cases: cells with no / exactly one / two or more visible agents each make up at least 10 %;
  * ``ego != 0``: fusing into agent 0's frame instead moves more than half of the outputs by more than FUSE_TOL; with ``max_cav > agents`` the
    same for a pairwise tensor indexed with stride ``agents``;
  * the out-of-view agent contributes nothing; fully masked cells are exactly 0; the stored bytes hold -128 and 127; in_zx covers 0, 128, 255;
  * the case table holds every shape, channel count and agent count the GPU file is meant to run.
"""
from collections import Counter

import numpy as np
import pytest

from _common import FUSE_TOL
from _weighted_fuse_cases import CASES, CHANNELS, Prepared, lanes_per_cell, phase2_stores, same_bits

_PREP = {}


def prepared(name):
    if name not in _PREP:
        _PREP[name] = Prepared(CASES[name])
    return _PREP[name]


def _moved(a, b):
    """share of the outputs that differ by more than FUSE_TOL"""
    return float((np.abs(a - b) > FUSE_TOL["atol"] + FUSE_TOL["rtol"] * np.abs(b)).mean())


@pytest.mark.parametrize("c", CHANNELS)
def test_phase2_mapping_covers_every_cell_and_channel_once(c):
    assert c % 64 == 0 and 64 % lanes_per_cell(c) == 0
    stores = phase2_stores(c)
    assert max(ci for ci, _ in stores) == 15, "a cell index outside rec[16]"
    count = Counter(stores)
    assert set(count) == {(ci, ch) for ci in range(16) for ch in range(0, c, 4)}
    assert set(count.values()) == {1}, "a (cell, channel) stored twice"


def test_the_former_rule_breaks_at_192_channels_only():
    """lpc = min(c >> 2, 64), as the kernel computed it: what the fix removes"""
    def stores(c):
        lpc = min(c >> 2, 64)
        cps = 64 // lpc
        out = []
        for wave in range(4):
            for lane in range(64):
                sub = lane // lpc
                l4 = (lane - sub * lpc) * 4
                for step in range(4 // cps):
                    for cb in range(0, c, 256):
                        if cb + l4 < c:
                            out.append((wave * 4 + step * cps + sub, cb + l4))
        return out
    for c in CHANNELS:
        old = stores(c)
        past = sum(ci >= 16 for ci, _ in old)
        dup = sum(v - 1 for v in Counter(old).values())
        if c == 192:
            assert (past, dup) == (16, 240)                      # float4 stores: 64 floats past cell 15, 960 floats stored twice
        else:
            assert (past, dup) == (0, 0) and sorted(old) == sorted(phase2_stores(c))      # the fix changes no other mapping


def test_case_table_holds_what_the_gpu_file_is_meant_to_run():
    cs = CASES.values()
    assert {c.c for c in cs} >= {64, 128, 192, 256, 320, 512}
    assert {c.agents for c in cs} >= {1, 2, 5, 8}
    assert {(c.h, c.w) for c in cs} >= {(1, 1), (3, 7), (16, 1), (5, 16)}
    assert {c.zx for c in cs} == {0, 128, 255}
    assert {c.max_cav for c in cs} == {5, 8} and any(c.max_cav > c.agents and c.ego > 0 for c in cs) and any(c.max_cav == c.agents for c in cs)
    assert any(c.ego == 1 for c in cs) and any(c.ego == c.agents - 1 and c.ego > 1 for c in cs)
    assert any(c.ratio != 1.0 and c.hm != c.wm and (c.h, c.w) != (c.w, c.h) for c in cs)
    assert any((c.h * c.w) % 16 == 5 for c in cs) and any(c.h * c.w == 16 for c in cs)
    assert all(c.aim for c in cs)


@pytest.mark.parametrize("name", list(CASES))
def test_case_aims_hold_on_the_reference(name):
    p = prepared(name)
    c = p.case
    vis = p.visible()
    b = p.bytes
    assert (b == -128).any() and (b == 127).any()
    assert np.isfinite(p.want).all() and np.isfinite(p.want_i8).all()
    assert (p.want[vis == 0] == 0).all() and (p.want_i8[vis == 0] == 0).all()
    if vis.all():
        assert (np.abs(p.want).max(axis=-1) > 0).all()
    if c.identity:
        same_bits(p.want, p.x[0], "oracle at the identity, fp32 features")
        same_bits(p.want_i8, p.xdq[0], "oracle at the identity, dequantized codes")
    if c.partial:
        share = [float((vis == 0).mean()), float((vis == 1).mean()), float((vis >= 2).mean())]
        print(f"{name}: no / one / two or more visible agents: {share}")
        assert min(share) >= 0.10, share
    if c.out_of_view is not None:
        assert c.out_of_view == c.agents - 1
        same_bits(p.want, p.oracle(p.x, n=c.agents - 1), "the out-of-view agent contributes nothing")
        assert (vis == c.agents - 1).all()
    if c.ego != 0:
        moved = _moved(p.oracle(p.x, ego=0), p.want)
        print(f"{name}: fused into agent 0's frame instead: {moved:.3f} of the outputs move")
        assert moved > 0.5
        if c.max_cav > c.agents:
            moved = _moved(p.oracle(p.x, affine=p.affine_with_stride_agents()), p.want)
            print(f"{name}: pairwise indexed with stride agents: {moved:.3f} of the outputs move")
            assert moved > 0.5
    if c.score == "zeros":
        inside = p.s[..., 0] == 0
        assert 0.2 < inside.mean() < 0.45 and (vis == 0).any()                         # masked although visible; some cells masked for both
    if c.score == "extremes":
        assert set(np.unique(p.s)) == {np.float32(1e-4), np.float32(1.0001)}
        # the weaker agent keeps exp(1e-4 - 1.0001) / (1 + ..) = 0.269 of the weight: both agents decide every output
        assert _moved(p.oracle(p.x, n=1), p.want) > 0.5
    if name == "half_cell_c256":
        assert (vis[:-1, :-1] == 2).all() and (vis[-1, :] >= 1).all()
