"""CPU side of the direct post-processing tests (tests/_postprocess_cases.py): the polygon IoU of oracle/postprocess.py held against a
reference that shares nothing with clipping, the score family whose bits no device library can move, and -- for EVERY case of the GPU
suite, by the oracle alone -- the conditions that case's GPU comparison rests on: that it is the case it claims to be."""
import numpy as np
import pytest

import _postprocess_cases as K
from oracle import postprocess as P

F32 = np.float32


# ---- the IoU reference -------------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    return abs(a - b) <= 1e-9 * max(abs(a), abs(b)) + 1e-12


def test_clipping_equals_the_vertex_method_on_seeded_rectangles():
    """oracle.postprocess.quad_intersection_area (the clipping quad_iou.h restates) against inter_area_by_vertices on 2000 seeded pairs of
    rotated rectangles, both vertex orientations of either operand: 1e-9 relative + 1e-12"""
    pairs = K.random_rect_pairs(2000)
    overlapping = 0
    for p, q in pairs:
        want = K.inter_area_by_vertices(p, q)
        overlapping += want > 0
        for pp in (p, p[::-1]):
            for qq in (q, q[::-1]):
                got = P.quad_intersection_area(pp, qq)
                assert _close(got, want), (p, q, got, want)
                assert _close(K.inter_area_by_vertices(pp, qq), want)
                assert _close(P.quad_intersection_area(qq, pp), want)            # and with the operands' roles swapped
    assert 1500 < overlapping < 2000                                               # both kinds occur


@pytest.mark.parametrize("name", list(K.HAND_PAIRS))
def test_clipping_on_hand_made_pairs(name):
    p, q, area = K.HAND_PAIRS[name]
    for pp in (p, p[::-1]):
        for qq in (q, q[::-1]):
            got, ref = P.quad_intersection_area(pp, qq), K.inter_area_by_vertices(pp, qq)
            if area is None:
                assert got == pytest.approx(8 * (np.sqrt(2) - 1), rel=1e-6)       # the octagon of test_polygon_intersection
            else:
                assert got == area and ref == area                                 # dyadic: exact
            assert _close(got, ref)


def test_clipping_is_exact_on_axis_aligned_dyadic_rectangles():
    g = np.random.default_rng(8)
    zero = 0
    for _ in range(400):
        x0, y0, x1, y1 = g.integers(-16, 17, 4) / 4.0
        a = (x0, y0, x0 + g.integers(0, 17) / 4.0, y0 + g.integers(0, 17) / 4.0)
        b = (x1, y1, x1 + g.integers(0, 17) / 4.0, y1 + g.integers(0, 17) / 4.0)
        want = K.aligned_closed_form(a, b)
        zero += want == 0
        for pa in (K.aligned_quad(a), K.aligned_quad(a)[::-1]):
            for pb in (K.aligned_quad(b), K.aligned_quad(b)[::-1]):
                assert P.quad_intersection_area(pa, pb) == want
                assert K.inter_area_by_vertices(pa, pb) == want
    assert 50 < zero < 350


# ---- the score family ----------------------------------------------------------------------------------------------------------------------------
def _sigmoid_with_exp_moved(x, ulps):
    e = np.exp(-np.asarray(x, F32), dtype=F32)
    for _ in range(abs(ulps)):
        e = np.nextafter(e, F32(np.inf if ulps > 0 else 0.0))
    return (F32(1.0) / (F32(1.0) + e)).astype(F32)


def test_score_family_bits_hold_under_any_expf():
    ks = np.arange(1, 121)
    x = K.family_logit(ks)
    want = K.family_bits(ks)
    assert x.dtype == F32 and len(set(want.tolist())) == 120 and set((want >> 8).tolist()) == {0x3F7FFF}
    assert (P.sigmoid(x).view(np.uint32) == want).all()
    assert P.sigmoid(np.array([K.ONE_LOGIT])).view(np.uint32)[0] == 0x3F800000
    for ulps in range(-4, 5):                                                      # the device library's expf, wherever it rounds
        assert (_sigmoid_with_exp_moved(x, ulps).view(np.uint32) == want).all(), ulps
        assert _sigmoid_with_exp_moved([K.ONE_LOGIT], ulps).view(np.uint32)[0] == 0x3F800000
    # a logit of 0 against a threshold of 0.5: exp(-0) is 1 by definition, nothing to move
    assert np.exp(F32(-0.0), dtype=F32) == F32(1.0) and P.sigmoid(np.zeros(1, F32))[0] == F32(0.5) and not (P.sigmoid(np.zeros(1, F32))[0] > F32(0.5))


# ---- every case is what it claims ------------------------------------------------------------------------------------------------------------------
def _centres(corners):
    return corners.astype(np.float64).mean(axis=1)


def _over(ious, thr):
    return {k for k, v in ious.items() if v > thr}


def _check_sweep(case, sc, ref):
    """the pairs above the threshold are the ``overlaps`` the builder names, the oracle keeps all but ``removed``"""
    info = case.info
    n = len(sc["scores"])
    ious = K.pair_ious(sc["corners"][:case.topk])
    assert _over(ious, case.nms_thr) == info["overlaps"]
    assert all(v == 0.0 or v > case.nms_thr + 0.05 for v in ious.values())         # touching or far above
    kept = [p for p in range(min(n, case.topk)) if p not in info["removed"]]
    assert K.greedy(min(n, case.topk), ious, case.nms_thr) == kept
    assert np.array_equal(ref[0], sc["corners"][kept]) and np.array_equal(ref[1], sc["scores"][kept])


def _check_disjoint(case, sc, ref):
    n = len(sc["scores"])
    assert K.pair_ious(sc["corners"]) == {}                                        # not even touching: the NMS removes nothing
    assert len(ref[1]) == min(n, case.topk)                                        # and the range mask nothing
    assert np.array_equal(ref[0], sc["corners"][:case.topk]) and np.array_equal(ref[1], sc["scores"][:case.topk])
    assert np.array_equal(ref[2], sc["labels"][:case.topk])


def _family_a(case, sc, ref):
    info, name = case.info, case.name
    n = info["n"]
    assert len(case.cavs) == 1 and case.ncls == 1 and case.nbins == 0 and np.array_equal(case.cavs[0][4], np.eye(4))
    assert len(sc["scores"]) == n == sc["flagged"]
    if name != "identical_equal":
        assert (np.diff(info["logits"]) <= -0.01 + 1e-9).all()                     # sorted position p is the p-th logit
    else:
        assert len(set(sc["scores"].tolist())) == 1 and (np.diff(info["slots"]) > 0).all()
    assert np.array_equal(sc["slots"], info["slots"])
    if n:
        assert (case.cavs[0][3].reshape(-1, 7)[info["slots"], 6] == 0).all()      # yaw 0
    if case.disjoint:
        _check_disjoint(case, sc, ref)
    else:
        _check_sweep(case, sc, ref)
    if name == "chain":
        assert n == 200 and {70, 150, 64} == info["removed"] and len(ref[1]) == 197
    if name == "bit63":
        assert {a for a, _ in info["overlaps"]} == {63} and len(ref[1]) == 128
    if name == "silent":
        assert len(ref[1]) == 128
    if name.startswith("identical"):
        assert len(ref[1]) == 1 and ref[0][0, 0, 2] == F32(-1.5)                   # sorted position 0 (equal scores: the lowest slot), z = -1
    if name.startswith("nvalid"):
        assert len(ref[1]) == n == int(name[6:]) and case.topk == case.na > n
    if name.startswith("topk"):
        assert len(ref[1]) == case.max_boxes == case.topk == int(name[4:]) < n
    if name.startswith("tiny"):
        assert len(ref[1]) == n == case.na == case.topk < case.max_boxes
    if name == "nothing":
        assert len(ref[1]) == 0


def _family_b(case, sc, ref):
    info = case.info
    bits = sc["scores"].view(np.uint32)
    assert case.h == 1 and case.a == 1 and case.w % 256 != 0 and case.max_boxes == 64
    assert set(bits.tolist()) <= set(K.family_bits(np.arange(1, 121)).tolist()) | {0x3F800000}
    _check_disjoint(case, sc, ref)
    n = len(bits)
    if "survivors" in info:
        cut = int(bits[63])
        thr24 = cut >> 8
        assert int((bits >> 8 >= thr24).sum()) == info["survivors"] == n           # one 24-bit prefix holds the cut: everything survives
        assert (n > K.SEL_CAP) == (case.name != "sel_cap2048") and (case.name != "sel_cap2048" or n == K.SEL_CAP)
        assert (case.name != "sel_cap2049" or n == K.SEL_CAP + 1)
        assert cut == K.family_bits(info["cut_k"]) and int((bits == cut).sum()) >= 30 - 0 and int((bits[:64] == cut).sum()) == info["ties_in"] >= 5
        assert int((bits > 0x3F7FFFFF).sum()) == 10                                 # ten in the prefix above
        above = {int(b) & 0xFF for b in bits if (int(b) >> 8) == thr24 and b > cut}
        assert len(above) >= 3                                                      # low-byte bins above the cut bin
        tied = sc["slots"][:64][bits[:64] == cut]
        assert np.array_equal(tied, info["tie_slots"][:14]) and (np.diff(tied) > 0).all()
        c = np.searchsorted(np.sort(sc["slots"]), sc["slots"][bits == cut])        # the ties' candidate numbers (rank among the flagged slots)
        assert np.array_equal(c[:14], np.sort(c)[:14]) and (c < 1024).sum() == 6 and 1024 <= c[13] < 2048      # the last to enter: 8th of group 1
        top = int((c >= 2048).sum())
        assert top == {"sel_lowbyte": 12, "sel_cap2048": 0, "sel_cap2049": 1}[case.name] and top != 6      # (from the top group down: another 14th tie)
        if case.name == "sel_cap2049":                                              # same top 64 as with one slot fewer
            other = K.reference("sel_cap2048")
            assert all(np.array_equal(a, b) for a, b in zip(ref, other))
    else:
        bad = info["bad"]
        assert sc["flagged"] == info["n"] and n == info["n"] - len(bad)
        assert len(ref[1]) == min(n, 64)
        if case.name == "sel_fewer":
            assert n == 40
        if case.name == "sel_exact":
            assert n == 64
        if case.name == "sel_plus1":
            assert n == 65 and bits[63] == bits[64] and sc["slots"][63] < sc["slots"][64] and bits[62] > bits[63]
        if bad:
            want_bits = K.family_bits(np.array([r + 1 for r in range(info["n"]) if r not in bad]))
            assert np.array_equal(bits, want_bits)                                  # the filtered ranks are gone, among them the best
            assert 0 in bad and (len(ref[1]) == 61 if case.name == "sel_bad61" else len(ref[1]) == 64 and n == 65)


def _family_c(case, sc, ref):
    info, name = case.info, case.name
    cls, reg, dirp, anchors, t = case.cavs[0]
    a = anchors.reshape(-1, 7)
    raw = P._candidates(cls, reg, dirp, anchors, t, case.thr, 0.0, 0, 1)[0]       # before the filters, slot order
    assert np.array_equal(_centres(ref[0])[:, :2], a[info["expect"], :2].astype(np.float64)), "the boxes that come out"
    quads = raw[:, :4, :2].astype(np.float64)
    if name.startswith("iou_eq"):
        assert P.quad_intersection_area(quads[0], quads[1]) == 2.0 and K.iou(quads[0], quads[1]) == 0.5
        assert K.iou(quads[0], quads[1], K.inter_area_by_vertices) == 0.5
    if name.startswith("extent_eq"):
        ax = 0 if name == "extent_eq" else 1
        ext = raw[:, :, ax].max(1) - raw[:, :, ax].min(1)
        assert ext[0] == F32(6.0) and ext[1] == np.nextafter(F32(6.0), F32(7.0))
    if name == "w_zero":
        assert (raw[0, :, 1].max() - raw[0, :, 1].min()) == 0 and (raw[0, :, 0].max() - raw[0, :, 0].min()) == 4
    if name == "z_eq":
        assert raw[0, :, 2].min() == F32(-3.0) and raw[0, :, 2].max() == F32(1.0)
    if name == "z_below":
        assert raw[0, :, 2].min() == np.nextafter(F32(-3.0), F32(-4.0))
    if name == "z_above":
        assert raw[0, :, 2].max() == np.nextafter(F32(1.0), F32(2.0)) and raw[0, :, 2].min() >= F32(-3.0)
    if name.startswith("range_") and "_xy" not in name:
        f = name[6:]
        ax, top = "xy".index(f[0]), f[1:] == "hi"
        face = F32(case.rng[ax + 3] if top else case.rng[ax])
        edge = raw[:, :, ax].max(1) if top else raw[:, :, ax].min(1)
        assert edge[0] == face and edge[1] == np.nextafter(face, F32(np.inf if top else -np.inf))
        assert len(sc["scores"]) == 2                                               # both pass the filters: the range mask decides
    if "_xy" in name:
        zlo, zhi = raw[0, :, 2].min(), raw[0, :, 2].max()
        f = name[6:9]
        assert len(sc["scores"]) == 1
        if f == "zon":
            assert (zlo, zhi) == (F32(-4.0), F32(2.0))
        elif f == "zhi":
            assert zhi == np.nextafter(F32(2.0), F32(3)) and zlo >= F32(-4.0)
        else:
            assert zlo == np.nextafter(F32(-4.0), F32(-5)) and zhi <= F32(2.0)
    if name == "score_eq":
        assert P.sigmoid(np.zeros(1, F32))[0] == F32(case.thr) and sc["flagged"] == 1 and cls.reshape(-1)[0] == 0


def _expected_late(case):
    """from the builder's plan alone: rows (cav, slot, x, y, logit) minus ``removed``, by descending logit, then CAV, then slot"""
    rows = [r for r in case.info["rows"] if (r[0], r[2], r[3]) not in case.info["removed"]]
    rows.sort(key=lambda r: (-r[4], r[0], r[1]))
    return np.array([[r[2], r[3]] for r in rows])


def _family_d(case, sc, ref):
    if case.batch:
        assert [len(r[1]) for r in ref] == case.info["counts"] and case.na1 == 111
        for f in (0, 1):
            assert K.sorted_candidates(case, [case.cavs[f]])["flagged"] == f
        sc2 = K.sorted_candidates(case, [case.cavs[2]])
        _check_sweep(case, sc2, ref[2])
        assert all(c[3] is case.cavs[0][3] for c in case.cavs)                     # shared anchors
        return
    ncav = len(case.cavs)
    assert (ncav, case.na1) in ((8, 111), (3, 257))
    ious = K.pair_ious(sc["corners"])
    assert len(_over(ious, case.nms_thr)) == len(case.info["removed"]) and all(v == 0 or v > 0.3 for v in ious.values())
    want = _expected_late(case)
    assert len(ref[1]) == len(want) == len(case.info["rows"]) - len(case.info["removed"])
    assert np.array_equal(_centres(ref[0])[:, :2], want)
    cav_of = sc["slots"] // case.na1
    assert set(cav_of.tolist()) == set(range(ncav))                                 # every CAV contributes
    if ncav == 3:
        assert {0, 255, 256} <= set((sc["slots"] % case.na1).tolist()) and (case.na1 + 255) // 256 == 2
    else:
        tied = sc["scores"] == P.sigmoid(np.array([1.0], F32))[0]
        assert tied.sum() == 8 and (np.diff(cav_of[tied]) > 0).all()               # eight tied across the CAVs: CAV order


def _dir_fixed_yaw(case, dtype):
    cls, reg, dirp, anchors, t = case.cavs[0]
    slots = case.info["slots"]
    yaw = anchors.reshape(-1, 7)[slots, 6].astype(dtype)
    lab = np.transpose(dirp, (0, 2, 3, 1)).reshape(-1, case.nbins)[slots].argmax(axis=1)
    period = dtype(2 * np.pi / case.nbins)
    lp = lambda v, off, per: v - np.floor(v / dtype(per) + dtype(off)) * dtype(per)
    rot = lp(yaw - dtype(F32(case.dir_offset)), 0.0, period)
    return lp(rot + dtype(F32(case.dir_offset)) + period * lab.astype(dtype), 0.5, 2 * np.pi), lab


def _family_e(case, sc, ref):
    if case.nbins == 0:
        lg = case.info["logits"]
        assert case.h * case.w % 2 == 1 and case.ncls in (2, 8) and case.a in (1, 16)
        _check_disjoint(case, sc, ref)
        best = lg.max(axis=1)
        order = np.argsort(-best, kind="stable")
        assert len(ref[1]) == case.na and np.array_equal(sc["slots"], order)
        assert np.array_equal(ref[2], lg.argmax(axis=1)[order] + 1)                 # first maximum
        by_slot = dict(zip(sc["slots"].tolist(), ref[2].tolist()))
        assert [by_slot[s] for s in range(4)] == [1, case.ncls, 1, case.ncls // 2 + 1]
        assert len(set(lg[0].tolist())) == 1 and lg[2, 0] == lg[2, -1] == lg[2].max()
        assert (np.diff(np.sort(best)) >= 2.0 ** -10).all()
        return
    n, nb = case.info["n"], case.nbins
    y32, lab = _dir_fixed_yaw(case, np.float32)
    y64, _ = _dir_fixed_yaw(case, np.float64)
    assert np.abs(y32 - y64).max() < 1e-5                                           # no floor falls the other way in fp32
    assert np.array_equal(lab, case.info["labels"]) and set(lab.tolist()) == set(range(nb))
    d = np.transpose(case.cavs[0][2], (0, 2, 3, 1)).reshape(-1, nb)[case.info["slots"]]
    tied = int(((d == d.max(axis=1, keepdims=True)).sum(axis=1) == 2).sum())
    assert tied == sum(l + 2 < nb for l in case.info["labels"]) and (nb < 4 or tied >= n // 2)      # tied maxima wherever a later bin exists
    assert np.abs(sc["corners"][:, :, 0]).max() < 64
    ious = K.pair_ious(sc["corners"])
    assert all(abs(v - case.nms_thr) > K.MARGIN for v in ious.values())
    extras = case.info["extras"]
    assert len(_over(ious, case.nms_thr)) == extras == len(ious) and len(sc["scores"]) == n + extras and len(ref[1]) == n


def _family_f(case, sc, ref):
    n = len(sc["scores"])
    assert n == 40 == case.na
    a = K.pair_ious(sc["corners"])
    b = K.pair_ious(sc["corners"], K.inter_area_by_vertices)
    assert a.keys() == b.keys()
    for k in a:
        assert abs(a[k] - case.nms_thr) > K.MARGIN and abs(b[k] - case.nms_thr) > K.MARGIN, k
        assert abs(a[k] - b[k]) < 1e-9
    kept = K.greedy(n, a, case.nms_thr)
    assert kept == K.greedy(n, b, case.nms_thr) and 20 <= len(kept) <= 32
    assert np.array_equal(ref[0], sc["corners"][kept])
    vals = sorted(a.values())
    assert vals[0] == 0.0 and vals[-1] > 0.999 and sum(0 < v < case.nms_thr for v in vals) >= 3
    yaw = case.cavs[0][3].reshape(-1, 7)[:, 6]
    assert {F32(0), F32(np.pi / 4), F32(np.pi / 2)} <= set(yaw.tolist())


_FAMILY = {"A": _family_a, "B": _family_b, "C": _family_c, "D": _family_d, "E": _family_e, "F": _family_f}


@pytest.mark.parametrize("name", K.CASES)
def test_case_is_what_it_claims(name):
    case = K.build(name)
    ref = K.reference(name)
    assert case.na <= 2600 and 1 <= case.max_boxes <= 1024
    sc = None if case.batch else K.sorted_candidates(case)
    _FAMILY[case.family](case, sc, ref)


def test_every_family_is_listed():
    fam = {K.build(n).family for n in K.CASES}
    assert fam == set("ABCDEF") and len(K.CASES) == len(set(K.CASES))
    assert {1, 2, 63, 65} == {K.build(n).na for n in K.CASES if n.startswith("tiny")}
