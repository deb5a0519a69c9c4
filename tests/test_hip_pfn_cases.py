"""qv2x_pfn_scatter_i8 and qv2x_pfn_unscatter_i8 called directly at their edges (cases, operands, references and checks in
tests/_pfn_cases.py; the reference is pinned and every case's aim is asserted by tests/test_pfn_cases_cpu.py).  tests/test_hip_parity.py and
tests/test_hip_fullsize.py reach these kernels only through whole models: max_points 32, z = 0, one calibrated pair of quantizers.

Every case: the canvas after the scatter equals the expected one byte for byte -- ``orc_pfn``'s codes in the pillars' cells, the fill
``z2 - 128`` in every other interior cell, the ring byte in the pad ring, the guard planes in front of and behind the canvas untouched --
and the un-scatter with ``z2 - 128`` gives back the canvas as it was before the scatter, ring included.

  * max_points 1, 2, 3, 5, 32 with 1, P - 1, P and np > P points; a channel only a masked slot can win, a dead channel
  * M = 1, 15, 16, 17, 33 (16 pillars per round) and 63, 64, 65 (64 pillars per un-scatter workgroup)
  * z = 1, 2, -1, the last agent's corners, eight pillars outside the canvas (one per side of each axis), the voxelizer's tail rows
  * one-point pillars on the first quantizer's rounding boundaries (exact ties with d1 a power of two, the boundary's fp32 neighbours
    otherwise) and on every entry of the second quantizer's table, at both quantizer settings
  * 2 and 8 rounds per workgroup with a ragged last workgroup, sized from this GPU's CU count
  * the un-scatter alone on a canvas full of another byte, with value -128, 0, 127; a case launched twice

Needs an MI355X."""
import numpy as np
import pytest

from _pfn_cases import (CASES, GUARD, MULTI_ROUND, REPEATED, UNSCATTER_ALONE, UNSCATTER_VALUES, DeviceCanvas, build, coords_to_device, device_cus,
                        multi_round_m, rounds_rule, same_bytes, scatter_launch, unscatter_launch)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_scatter_then_unscatter(name):
    cus = device_cus()
    prep = build(name, cus)
    if name in MULTI_ROUND:
        rounds = prep.facts["rounds"]
        assert prep.M == multi_round_m(rounds, cus) and rounds_rule(prep.M, cus) == rounds and rounds in (2, 8)
        assert 0 < prep.M % (16 * rounds) < 16 * (rounds - 1) + 1, "the last workgroup has empty rounds"
        print(f"{name}: {cus} CUs, M = {prep.M}, {rounds} rounds, grid {prep.N} x {prep.ny} x {prep.nx}, {int((~prep.inside).sum())} rows outside")
    else:
        assert rounds_rule(prep.M, cus) == 1
    before = prep.before()
    dc, co = DeviceCanvas(before), coords_to_device(prep)
    scatter_launch(prep, dc, co)
    same_bytes(dc.read(f"qv2x_pfn_scatter_i8, {name}"), prep.after(), f"qv2x_pfn_scatter_i8, {name}")
    unscatter_launch(prep, dc, int(prep.q.z2) - 128, co)
    same_bytes(dc.read(f"qv2x_pfn_unscatter_i8, {name}"), before, f"qv2x_pfn_unscatter_i8 after the scatter, {name}")


@pytest.mark.parametrize("value", UNSCATTER_VALUES)
@pytest.mark.parametrize("name", UNSCATTER_ALONE)
def test_unscatter_alone(name, value):
    prep = build(name)
    want = prep.unscattered(value)
    dc = DeviceCanvas(np.full_like(want, GUARD))
    unscatter_launch(prep, dc, value)
    same_bytes(dc.read(f"qv2x_pfn_unscatter_i8, {name}, value {value}"), want, f"qv2x_pfn_unscatter_i8 alone, {name}, value {value}")


def test_scatter_twice_gives_equal_bytes():
    prep = build(REPEATED)
    got = []
    for _ in range(2):
        dc = DeviceCanvas(prep.before())
        scatter_launch(prep, dc)
        got.append(dc.read(f"qv2x_pfn_scatter_i8, {REPEATED}"))
    same_bytes(got[0], got[1], f"qv2x_pfn_scatter_i8, {REPEATED}: the second launch against the first")
    same_bytes(got[0], prep.after(), f"qv2x_pfn_scatter_i8, {REPEATED}")
