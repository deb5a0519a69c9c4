"""The reference of tests/test_hip_pfn_cases.py pinned, and what every case of tests/_pfn_cases.py is aimed at asserted on the reference
alone.  No GPU.

  * ``orc_pfn`` against PillarVFE + QuantPFNLayer restated in float64 (``ref64``): wherever the float64 value in front of the first quantizer
    lies farther from every rounding boundary of that quantizer than ``pfn_ref64``'s bound, the final codes are equal.  The share of elements
    inside the bound is printed and, on the random-weight cases, capped at 1 % (bound ~4e-6 against d1 of a few 1e-2: a few 1e-4 expected).
    The tie cases sit on the boundaries on purpose and are exempt from the cap.
  * the two quantizer settings are what the cases need; the second quantizer's table is the same in fp32 and in float64, no entry near a
    boundary; the ring byte is a byte no pillar can write.
  * per case: distinct cells (asserted when the case is built), the expected canvas differs from the clean one in the pillars' cells only,
    masked-slot winners exactly where a slot is masked, the dead channel, np > P, the placement rows, the tie band and both roundings, the
    table's coverage, the rounds and the ragged last workgroup of the multi-round cases at 256 CUs.
  * the host's argument checks of both entries, which return before any launch.
"""
import ctypes as C

import numpy as np
import pytest

from _pfn_cases import (CASES, CH_DEAD, CH_MASKED, GRID, GUARD, MULTI_ROUND, PLACEMENT_P, QA, QB, QUANTS, REPEATED, UNSCATTER_ALONE, UNSCATTER_VALUES,
                        build, multi_round_m, placement_rows, q_code32, ref64, ring_byte, rounds_rule, slot_counts, table32, table64,
                        table_values, tap_operand, tap_rotations, tie_values)

RANDOM = [n for n in CASES if not n.startswith(("ties_", "table_"))]
CAP = 0.01


def test_quantizer_settings():
    assert QA.z2 == 0 and np.log2(float(QA.d1)) % 1 == 0 and np.float32(1) / QA.d1 * QA.d1 == 1
    assert QB.z2 > 0 and 64 <= QB.z1 <= 192 and np.log2(float(QB.d1)) % 1 != 0 and np.log2(float(QB.d2)) % 1 != 0
    for q in QUANTS.values():
        t32, (t64, margin) = table32(q), table64(q)
        assert (t32 == t64).all() and margin.min() > 1e-3, "the second quantizer must not depend on fp32 against float64"
        assert (t32[:int(q.z1) + 1] == int(q.z2)).all() and (np.diff(t32.astype(int)) >= 0).all() and t32[-1] > int(q.z2) + 100
        ring = int(ring_byte(q)) + 128
        assert ring not in t32 and ring != int(q.z2) and np.int8(ring - 128) != GUARD
    assert table32(QA)[-1] == 255 and table32(QB)[-1] < 255                                    # one table saturates, the other does not
    assert {build(n).q.name for n in CASES} == {"qa", "qb"}
    for v in UNSCATTER_VALUES:
        assert np.int8(v) != GUARD


@pytest.mark.parametrize("name", list(CASES))
def test_orc_pfn_against_float64(name):
    p = build(name)
    rows = None
    if name in MULTI_ROUND:                                                                     # a sample: the ends, the out-of-canvas rows' neighbours, 4096 at random
        rng = np.random.default_rng(5)
        rows = np.unique(np.concatenate([np.arange(64), np.arange(p.M - 64, p.M), rng.integers(0, p.M, 4096)]))
    rows, code64, y, bound, near = ref64(p, rows)
    assert len(rows) and np.isfinite(y).all() and (bound >= 0).all()
    share = float(near.mean())
    differ = p.codes[rows] != code64
    print(f"{name}: {near.sum()} of {near.size} elements within the bound of a boundary (share {share:.2e}); {int(differ.sum())} codes differ, "
          f"all among them: {bool((differ <= near).all())}; largest bound / d1 = {float(bound.max() / p.q.d1):.2e}")
    assert (differ <= near).all(), f"{int((differ & ~near).sum())} codes differ from float64 away from every boundary"
    if p.kind == "random":
        assert share < CAP
        assert (y / float(p.q.d1) + float(p.q.z1) > 255.5).mean() < 0.3                                              # the codes are spread, not saturated
        assert len(np.unique(p.codes[rows])) > 40 or len(rows) < 5
    elif name.startswith("table_"):
        assert not near.any()


@pytest.mark.parametrize("name", list(CASES))
def test_expected_canvas(name):
    p = build(name)
    assert p.aim
    before, after = p.before(), p.after()
    ring, fill = ring_byte(p.q), np.int8(int(p.q.z2) - 128)
    assert ring != fill and (before[:, 1:-1, 1:-1] == fill).all()
    for part in (before[:, 0], before[:, -1], before[:, :, 0], before[:, :, -1], after[:, 0], after[:, -1], after[:, :, 0], after[:, :, -1]):
        assert (part == ring).all()
    assert not (after == ring)[:, 1:-1, 1:-1].any(), "a pillar writes the ring byte"
    changed = (after != before).any(axis=-1)
    assert int(changed.sum()) <= int(p.inside.sum()) == len(p.cell)
    assert set(np.flatnonzero(changed.reshape(-1)).tolist()) <= set(p.cell.tolist())
    live = p.codes[p.inside]
    assert ((live != int(p.q.z2)).mean(axis=1) > 0.2).all(), "every in-canvas pillar has live channels: a skipped pillar would show"
    for v in UNSCATTER_VALUES:
        u = p.unscattered(v)
        assert int((u != GUARD).any(axis=-1).sum()) == len(p.cell) and (u[u != GUARD] == v).all()


@pytest.mark.parametrize("name", RANDOM)
def test_masked_slot_winners(name):
    p = build(name)
    q = p.q
    bias_code = table32(q)[int(q_code32(p.b[CH_MASKED], q.d1, q.z1))]
    masked = p.npts < p.P
    ok = p.npts >= 1
    print(f"{name}: masked-slot winner in pillars {np.flatnonzero(masked & ok).tolist()[:40]}")
    assert (p.codes[masked & ok, CH_MASKED] == bias_code).all(), "a masked slot contributes the bias alone, and here it wins"
    assert (p.codes[~masked, CH_MASKED] < bias_code).all(), "np >= P: no masked slot exists, the bias alone must not win"
    assert (p.codes[ok, CH_DEAD] == int(q.z2)).all()
    if p.P > 1:
        assert masked[p.inside].any()
    assert (~masked)[p.inside].any() or p.M == 1


def test_slot_and_pillar_count_cases():
    slots = [build(n) for n in CASES if n.startswith("slots_")]
    assert {(p.P, p.q.name) for p in slots} == {(P, q) for P in (1, 2, 3, 5, 32) for q in ("qa", "qb")}
    for p in slots:
        assert set(p.npts.tolist()) == set(slot_counts(p.P)) >= {1, max(p.P - 1, 1), p.P} and p.npts.max() > p.P and p.inside.all()
        # np > P: the mean divides by the reported count.  With np clamped to P the mean features differ, and so do the codes
        over = p.npts > p.P
        clamped = type(p)(p.name, p.aim, p.kind, p.q, p.P, (p.N, p.ny, p.nx), p.coords, np.minimum(p.npts, p.P), p.vf, p.w, p.b, p.vox, p.off)
        assert ((clamped.codes != p.codes).mean(axis=1)[over] > 0.1).all() and (clamped.codes[~over] == p.codes[~over]).all()
    counts = [build(n) for n in CASES if n.startswith("m")]
    assert [p.M for p in counts] == [1, 15, 16, 17, 33, 63, 64, 65] and all(p.inside.all() for p in counts)
    assert {p.q.name for p in counts} == {"qa", "qb"} and all(set(p.npts.tolist()) <= {1, 2, 3, 4, 5} and p.P == 3 for p in counts)
    assert set(UNSCATTER_ALONE) >= {"m63", "m64", "m65"} and REPEATED in CASES


@pytest.mark.parametrize("name", ["placement_qa", "placement_qb"])
def test_placement_case(name):
    p = build(name)
    n, ny, nx = GRID
    live, outside, tail = placement_rows()
    rows = [tuple(int(v) for v in r) + (int(k),) for r, k in zip(p.coords, p.npts)]
    assert sorted(rows) == sorted(live + outside + tail) and p.P == PLACEMENT_P
    assert int(p.inside.sum()) == len(live) == 8 and len(outside) == 8
    at = {(b, y, z + x) for (b, z, y, x, _k) in live}
    assert at >= {(n - 1, 0, 0), (n - 1, 0, nx - 1), (n - 1, ny - 1, 0), (n - 1, ny - 1, nx - 1)}
    assert {z for (_b, z, _y, _x, _k) in live} >= {1, 2, -1} and (0, -1, 3, 1, 2) in live                                   # z = -1, x = 1: column 0
    assert all(x >= 0 for (_b, _z, _y, x, _k) in live) and {k for r in live for k in r[4:]} >= {1, PLACEMENT_P, 9}
    out = [r[:4] for r in outside]
    assert {r[0] for r in out} >= {-1, n} and {r[2] for r in out} >= {-1, ny} and {r[1] + r[3] for r in out} >= {-1, nx}
    assert all(sum([not 0 <= r[0] < n, not 0 <= r[2] < ny, not 0 <= r[1] + r[3] < nx]) == 1 for r in out)                    # one side each
    assert sum(r[1] != 0 for r in out) == 2                                                                                   # two leave through z
    is_out = np.array([r in outside for r in rows])
    assert (np.abs(p.vf[is_out]).sum(axis=(1, 2)) > 0).all() and (p.codes[is_out] != int(p.q.z2)).any(axis=1).all(), "their features are real points"
    is_tail = p.npts == 0
    assert is_tail.sum() == 5 and (p.coords[is_tail] == -1).all() and (p.vf[is_tail] == 0).all() and is_tail[0] and is_tail[-1]
    assert not is_tail[1:-1].all() and np.diff(np.flatnonzero(is_tail)).min() > 1, "tail rows lie between live rows"


@pytest.mark.parametrize("name", ["ties_qa", "ties_qb"])
def test_tie_case(name):
    p = build(name)
    q = p.q
    values, k = tie_values(q)
    assert p.P == 1 and (p.npts == 1).all() and p.inside.all() and (p.vf[:, 0, 3] == values).all()
    assert set(k.tolist()) == set(range(-int(q.z1), 256 - int(q.z1)))
    y = tap_operand(p)
    assert set(y.view(np.uint32).ravel().tolist()) == set(values.view(np.uint32).tolist())
    for j in range(4):
        assert set(p.vf[:, 0, j].view(np.uint32).tolist()) == set(values.view(np.uint32).tolist()), "every byte of a lane's dword sees every value"
    t = y / q.d1                                                                                   # fp32 division, as the quantizer's
    assert t.dtype == np.float32 and (np.abs(t - np.rint(t)) > 0.4997).all(), "every element lies in the kernel's doubtful band"
    assert (p.codes == table32(q)[q_code32(y, q.d1, q.z1).astype(np.int64)]).all(), "orc_pfn against the numpy restatement of q_code"
    # both roundings: where the table tells code k + z1 from k + 1 + z1 apart, the oracle's final code says which way the element went
    tab = table32(q)
    kk = np.stack([k[(np.arange(len(k)) + r) % len(k)] for r in tap_rotations(len(k))], axis=1)[:, np.arange(64) % 4]
    lo, hi = np.clip(kk + int(q.z1), 0, 255), np.clip(kk + 1 + int(q.z1), 0, 255)
    tells = tab[lo] != tab[hi]
    down, up = tells & (p.codes == tab[lo]), tells & (p.codes == tab[hi])
    print(f"{name}: {int(tells.sum())} telling elements, {int(down.sum())} rounded down, {int(up.sum())} up")
    assert (down | up)[tells].all() and down.sum() > 1000 and up.sum() > 1000
    if q is QA:
        assert (values.astype(np.float64) == (k + 0.5) * float(q.d1)).all(), "exact ties"
        even = kk % 2 == 0
        assert (down[tells] == even[tells]).all(), "round half to even"
    else:
        # the reciprocal product rounds some of these the other way: a kernel that trusted it would write other bytes
        other = np.clip(np.rint(y * (np.float32(1) / q.d1)).astype(np.float32) + q.z1, 0, 255).astype(np.int64)
        wrong = tab[other] != p.codes
        print(f"{name}: rint(y * fl(1 / d1)) gives another final code on {int(wrong.sum())} elements")
        assert wrong.sum() >= 8


@pytest.mark.parametrize("name", ["table_qa", "table_qb"])
def test_table_case(name):
    p = build(name)
    q = p.q
    values = table_values(q)
    assert p.P == 1 and p.M == 258 and (p.npts == 1).all() and p.inside.all() and (p.vf[:, 0, 3] == values).all()
    first = q_code32(tap_operand(p), q.d1, q.z1).astype(np.int64)
    for j in range(4):
        assert set(first[:, j].tolist()) == set(range(256)), "every first-quantizer code in every byte of a lane's dword"
    assert (q_code32(values[:256], q.d1, q.z1) == np.arange(256)).all() and q_code32(values[256], q.d1, q.z1) == 255 and q_code32(values[257], q.d1, q.z1) == 0
    tab = table32(q)
    assert (p.codes == tab[first]).all(), "orc_pfn against the numpy restatement of q_code and the table"
    final = set(p.codes.ravel().tolist())
    assert int(q.z2) in final and (p.codes[first < int(q.z1)] == int(q.z2)).all(), "the ReLU clamps every code below z1 to z2"
    if (255 - float(q.z1)) * float(q.d1) / float(q.d2) + float(q.z2) >= 255:
        assert 255 in final
    assert final == set(tab.tolist())
    # without the ReLU the second quantizer would see negative values: with z2 > 0 other codes, with z2 = 0 the clamp hides it
    c = np.arange(256, dtype=np.float32)
    no_relu = q_code32((c - q.z1) * q.d1, q.d2, q.z2)
    assert (no_relu != tab).any() == (q.z2 > 0)


@pytest.mark.parametrize("name", MULTI_ROUND)
def test_multi_round_case_at_256_cus(name):
    p = build(name, 256)
    rounds = p.facts["rounds"]
    assert p.M == multi_round_m(rounds, 256) and rounds_rule(p.M, 256) == rounds and (rounds, p.P) in ((2, 2), (8, 1))
    assert rounds_rule(65535, 256) == 1 and rounds_rule(65536, 256) == 2 and rounds_rule(10 ** 7, 256) == 8 and rounds_rule(1, 256) == 1
    per_wg = 16 * rounds
    tail = p.M % per_wg
    assert 0 < tail < per_wg and tail % 16 != 0, "the last workgroup is ragged"
    assert rounds - -(-tail // 16) >= 1, "some of its rounds are empty, and the header fetched one round ahead falls past M"
    assert 30 <= int((~p.inside).sum()) <= 60 and p.inside[-1] and p.inside[0]
    assert p.N * p.ny * p.nx >= p.inside.sum() > 0.97 * p.N * p.ny * p.nx and p.before().nbytes < 20e6
    assert set(p.coords[p.inside][:, 1].tolist()) == {-1, 0, 1} and (p.coords[p.inside][:, 3] >= 0).all()
    assert p.npts.min() == 1 and p.npts.max() > p.P


def test_argument_checks_without_gpu():
    """both entries refuse bad arguments on the host, before any launch"""
    from quantv2x_amd import build as B, lib
    B.build()
    l = lib.load()
    buf = np.zeros(4096 + 64, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    prm, err = C.byref(lib.PfnParams()), l.qv2x_last_error
    OK, EINVAL, EALIGN = 0, -1, -2
    sc = l.qv2x_pfn_scatter_i8
    assert sc(None, None, None, 0, 32, None, None, 1, 4, 4, None) == OK                          # M = 0: nothing to do
    for args in ((None, p, p, 1, 32, prm, p), (p, None, p, 1, 32, prm, p), (p, p, None, 1, 32, prm, p), (p, p, p, 1, 32, None, p), (p, p, p, 1, 32, prm, None)):
        assert sc(*args, 1, 4, 4, None) == EINVAL and b"null" in err()
    assert sc(p, p, p, -1, 32, prm, p, 1, 4, 4, None) == EINVAL and b"bad sizes" in err()
    for mp in (0, -1):
        assert sc(p, p, p, 1, mp, prm, p, 1, 4, 4, None) == EINVAL
    for dims in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert sc(p, p, p, 1, 32, prm, p, *dims, None) == EINVAL and b"bad sizes" in err()
    assert sc(odd, p, p, 1, 32, prm, p, 1, 4, 4, None) == EALIGN and b"aligned" in err()
    assert sc(p, odd, p, 1, 32, prm, p, 1, 4, 4, None) == EALIGN
    un = l.qv2x_pfn_unscatter_i8
    assert un(None, 0, 0, None, 1, 4, 4, None) == OK
    assert un(None, 1, 0, p, 1, 4, 4, None) == EINVAL and un(p, 1, 0, None, 1, 4, 4, None) == EINVAL and b"null" in err()
    for v in (-129, 128):
        assert un(p, 1, v, p, 1, 4, 4, None) == EINVAL and b"value" in err()
    assert un(p, -1, 0, p, 1, 4, 4, None) == EINVAL and un(p, 1, 0, p, 0, 4, 4, None) == EINVAL and un(p, 1, 0, p, 1, 4, 0, None) == EINVAL
    assert un(odd, 1, 0, p, 1, 4, 4, None) == EALIGN and b"aligned" in err()
    assert un(p, 1, 0, odd, 1, 4, 4, None) == EALIGN
