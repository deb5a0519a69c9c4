"""Case builders, the case list and an independent polygon-intersection reference for the direct tests of csrc/postprocess.hip (no tests
here, numpy only).  tests/test_postprocess_cases_cpu.py pins the references and checks, for every case, the conditions its GPU comparison
rests on; tests/test_hip_postprocess_cases.py runs the C entries on the same cases against oracle/postprocess.py.

What makes a case direct: ``anchors`` is an input array.  With ``reg == 0`` and no direction head a decoded box IS its anchor
(``exp(0) = 1``, ``0 * diag + a = a``), so ``plant`` puts any box with any score at any slot.  With dyadic box parameters, ``yaw = 0`` and
a matrix that is the identity or a dyadic translation every corner is exact in fp32, on the GPU and in the oracle, under any order of the
sums: those cases compare corners for equality (``Case.exact``).  Unless a case says otherwise the range is +-2^14 m, so nothing is masked
by accident, and boxes sit at z = -1 with height 1, inside the z limits.

A case's sorted position p (its rank in the stable descending score order) is decoupled from its slot: positions are dealt to the slots by
a seeded permutation, so the selection and the sort do real work in every case.
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import postprocess as P

F32 = np.float32
WIDE = [-2.0 ** 14, -2.0 ** 14, -2.0 ** 14, 2.0 ** 14, 2.0 ** 14, 2.0 ** 14]
FAR = np.array([2.0 ** 15, 2.0 ** 15, -1.0, 1.0, 1.0, 1.0, 0.0], F32)      # an unplanted slot's anchor: outside every range used here
EYE = np.eye(4, dtype=F32)
DIR_OFFSET = 0.7853


def translation(tx, ty, tz=0.0):
    t = np.eye(4, dtype=F32)
    t[:3, 3] = (tx, ty, tz)
    return t


def box(x, y, l=4.0, w=2.0, z=-1.0, h=1.0, yaw=0.0):
    """an 'hwl' anchor row (x, y, z, h, w, l, yaw): ``l`` along x, ``w`` along y at yaw 0"""
    return (x, y, z, h, w, l, yaw)


def plant(boxes, logits, slots, h, w, a, ncls=1, background=-20.0):
    """-> cls f32 [1, a * ncls, h, w], reg f32 [1, 7 a, h, w] (zeros), anchors f32 [h, w, a, 7]: slot s = (y * w + x) * a + anchor holds
    ``boxes[i]`` with class logits ``logits[i]`` (a scalar, or ``ncls`` values); every other slot ``background`` and the FAR anchor"""
    na = h * w * a
    slots = np.asarray(slots, np.int64).reshape(-1)
    assert len(set(slots.tolist())) == len(slots) and (len(slots) == 0 or (0 <= slots.min() and slots.max() < na))
    anchors = np.tile(FAR, (na, 1))
    lg = np.full((na, ncls), background, F32)
    if len(slots):
        anchors[slots] = np.asarray(boxes, F32).reshape(len(slots), 7)
        lg[slots] = np.asarray(logits, F32).reshape(len(slots), -1)
    cls = np.ascontiguousarray(lg.reshape(h, w, a * ncls).transpose(2, 0, 1)[None])
    return cls, np.zeros((1, 7 * a, h, w), F32), anchors.reshape(h, w, a, 7)


@dataclasses.dataclass
class Case:
    name: str
    family: str
    h: int
    w: int
    a: int
    cavs: list                       # [(cls, reg, dirp or None, anchors [h, w, a, 7], t 4x4)]: one per CAV -- or, ``batch``: one per frame
    ncls: int = 1
    nbins: int = 0
    thr: float = 0.2
    nms_thr: float = 0.25
    dir_offset: float = 0.0
    rng: tuple = tuple(WIDE)
    xy_only: bool = False
    max_extent: float = 6.0
    z_lim: tuple = (-3.0, 1.0)
    max_boxes: int = 1000
    batch: bool = False              # the cavs are the frames of one qv2x_postprocess_batch_f32 call (shared anchors)
    disjoint: bool = False           # the candidates' bounding boxes are pairwise disjoint: the reference is the oracle without its NMS
    exact: bool = True               # corners compare for equality (else to 1e-5)
    score_bits: bool = False         # scores compare bit for bit (else to 1e-5)
    info: dict = dataclasses.field(default_factory=dict)

    @property
    def na1(self):
        return self.h * self.w * self.a

    @property
    def na(self):
        return self.na1 * (1 if self.batch else len(self.cavs))

    @property
    def topk(self):
        return min(self.max_boxes, self.na)


# ---- the oracle on a case --------------------------------------------------------------------------------------------------------------------
def _kw(case):
    return dict(score_threshold=case.thr, nms_thresh=case.nms_thr, dir_offset=case.dir_offset, num_bins=case.nbins, num_classes=case.ncls,
                max_extent=case.max_extent, z_lim=case.z_lim, range_xy_only=case.xy_only, return_labels=True, top=case.topk)


def _reference(case, cavs):
    if case.disjoint:
        c, s, l = P.post_process_late(cavs, list(case.rng), nms=False, **_kw(case))
        return c[:case.topk], s[:case.topk], l[:case.topk]
    return P.post_process_late(cavs, list(case.rng), nms=True, **_kw(case))


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle/postprocess.py on the case -> (corners f32 [K, 8, 3], scores f32 [K], labels i64 [K]); a batch: a list of these, one per
    frame.  Computed once per process and shared: treat it as read-only."""
    case = build(name)
    if case.batch:
        return [_reference(case, [f]) for f in case.cavs]
    return _reference(case, case.cavs)


def sorted_candidates(case, cavs=None):
    """what enters the top-k cut, by the oracle alone: the thresholded candidates of every CAV in (CAV, slot) order, size / z filters, stable
    descending sort.  -> dict: corners f32 [N, 8, 3], scores, labels, slots (global: cav * na1 + local), in sorted order; ``flagged``: the
    number above the threshold before the filters"""
    cavs = case.cavs if cavs is None else cavs
    parts, slots = [], []
    for ci, (cls, reg, dirp, anchors, t) in enumerate(cavs):
        parts.append(P._candidates(cls, reg, dirp, anchors, t, case.thr, case.dir_offset, case.nbins, case.ncls))
        pk = P.sigmoid(np.transpose(cls, (0, 2, 3, 1))).reshape(-1, case.ncls).max(axis=-1)
        slots.append(ci * case.na1 + np.nonzero(pk > F32(case.thr))[0])
    corners, scores, labels = (np.concatenate([p[i] for p in parts]) for i in range(3))
    slots = np.concatenate(slots)
    assert len(slots) == len(scores)
    flagged = len(scores)
    if flagged:
        xl = corners[:, :, 0].max(1) - corners[:, :, 0].min(1)
        yl = corners[:, :, 1].max(1) - corners[:, :, 1].min(1)
        keep = (xl <= case.max_extent) & (yl <= case.max_extent) & (yl != 0)
        keep &= (corners[:, :, 2].min(1) >= case.z_lim[0]) & (corners[:, :, 2].max(1) <= case.z_lim[1])
        corners, scores, labels, slots = corners[keep], scores[keep], labels[keep], slots[keep]
    order = np.argsort(-scores, kind="stable")
    return dict(corners=corners[order], scores=scores[order], labels=labels[order], slots=slots[order], flagged=flagged)


# ---- polygon intersection without clipping -----------------------------------------------------------------------------------------------------
def _cross(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _shoelace(pts):
    s = 0.0
    for i in range(len(pts)):
        x0, y0 = pts[i]
        x1, y1 = pts[(i + 1) % len(pts)]
        s += x0 * y1 - x1 * y0
    return 0.5 * s


def _inside_or_on(pt, poly, sign):
    return all(sign * _cross(*poly[i], *poly[(i + 1) % len(poly)], *pt) >= 0.0 for i in range(len(poly)))


def inter_area_by_vertices(p, q):
    """Area of the intersection of two convex polygons in float64 by its vertex set -- no clipping: the vertices of ``p`` inside or on ``q``,
    those of ``q`` inside or on ``p``, every proper edge-edge crossing; de-duplicated, sorted by angle about their centroid, shoelace.
    (An improper crossing -- a vertex on the other polygon's edge, collinear edges -- adds nothing: that vertex is already 'on'.)"""
    p = [tuple(map(float, v)) for v in p]
    q = [tuple(map(float, v)) for v in q]
    sp, sq = _shoelace(p), _shoelace(q)
    if sp == 0.0 or sq == 0.0:
        return 0.0
    sp, sq = math.copysign(1.0, sp), math.copysign(1.0, sq)
    pts = [v for v in p if _inside_or_on(v, q, sq)] + [v for v in q if _inside_or_on(v, p, sp)]
    for i in range(len(p)):
        a, b = p[i], p[(i + 1) % len(p)]
        for j in range(len(q)):
            c, d = q[j], q[(j + 1) % len(q)]
            d1, d2 = _cross(*a, *b, *c), _cross(*a, *b, *d)
            d3, d4 = _cross(*c, *d, *a), _cross(*c, *d, *b)
            if d1 * d2 < 0.0 and d3 * d4 < 0.0:
                s = d3 / (d3 - d4)
                pts.append((a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1])))
    scale = max(max(abs(x), abs(y)) for x, y in p + q)
    uniq = []
    for v in pts:
        if all(max(abs(v[0] - u[0]), abs(v[1] - u[1])) > 1e-12 * scale for u in uniq):
            uniq.append(v)
    if len(uniq) < 3:
        return 0.0
    gx, gy = sum(v[0] for v in uniq) / len(uniq), sum(v[1] for v in uniq) / len(uniq)
    uniq.sort(key=lambda v: math.atan2(v[1] - gy, v[0] - gx))
    return abs(_shoelace(uniq))


def rect(cx, cy, l, w, yaw):
    """float64 [4, 2]: a rectangle's vertices, counter-clockwise for positive sizes"""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[cx + c * dx * l / 2 - s * dy * w / 2, cy + s * dx * l / 2 + c * dy * w / 2] for dx, dy in ((1, -1), (1, 1), (-1, 1), (-1, -1))])


def random_rect_pairs(n, seed=3):
    """seeded pairs of rotated rectangles of 0.5 .. 5 m whose centres lie within 3 m: most overlap, some do not"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = rect(*g.uniform(-1.5, 1.5, 2), *g.uniform(0.5, 5.0, 2), g.uniform(-math.pi, math.pi))
        q = rect(*g.uniform(-1.5, 1.5, 2), *g.uniform(0.5, 5.0, 2), g.uniform(-math.pi, math.pi))
        out.append((p, q))
    return out


SQ = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], float)
HAND_PAIRS = {   # name: (p, q, area)
    "identical": (rect(1, 2, 4, 2, 0), rect(1, 2, 4, 2, 0), 8.0),
    "inside": (rect(0, 0, 8, 4, 0), rect(0.5, -0.25, 2, 1, 0), 2.0),
    "shared_edge": (rect(0, 0, 4, 2, 0), rect(4, 0, 4, 2, 0), 0.0),
    "shared_edge_part": (rect(0, 0, 4, 2, 0), rect(4, 1, 4, 2, 0), 0.0),
    "shared_vertex": (rect(0, 0, 4, 2, 0), rect(4, 2, 4, 2, 0), 0.0),
    "cross": (rect(0, 0, 6, 1, 0), rect(0, 0, 1, 6, 0), 1.0),
    "square_45": (SQ, np.array([[1, -0.41421356], [2.41421356, 1], [1, 2.41421356], [-0.41421356, 1]]), None),    # regular octagon, 1e-6
    "zero_width": (rect(0, 0, 4, 2, 0), rect(0, 0, 4, 0, 0), 0.0),
    "zero_width_first": (rect(0, 0, 4, 0, 0), rect(0, 0, 4, 2, 0), 0.0),
    "t_junction": (rect(0, 0, 4, 2, 0), rect(1, 1.5, 2, 3, 0), 2.0),                  # vertices of q on an edge of p
    "edge_through_vertex": (SQ, np.array([[2, 0], [4, 2], [2, 4], [0, 2]], float), 2.0),     # an edge of q through two vertices of p
}


def aligned_closed_form(a, b):
    """(x0, y0, x1, y1) rectangles -> intersection area"""
    return max(0.0, min(a[2], b[2]) - max(a[0], b[0])) * max(0.0, min(a[3], b[3]) - max(a[1], b[1]))


def aligned_quad(r):
    return np.array([[r[2], r[1]], [r[2], r[3]], [r[0], r[3]], [r[0], r[1]]], float)


def iou(p, q, inter_fn=P.quad_intersection_area):
    inter = inter_fn(p, q)
    union = P.quad_area(p) + P.quad_area(q) - inter
    return inter / union if union > 0 else 0.0


def pair_ious(corners, inter_fn=P.quad_intersection_area):
    """{(i, j): IoU} over the pairs i < j of bottom faces whose bounding boxes touch or overlap (every other pair: 0 by any method)"""
    quads = corners[:, :4, :2].astype(np.float64)
    lo, hi = quads.min(axis=1), quads.max(axis=1)
    near = ((lo[:, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[:, None, :])).all(axis=2)
    return {(int(i), int(j)): iou(quads[i], quads[j], inter_fn) for i, j in zip(*np.nonzero(np.triu(near, 1)))}


def greedy(n, ious, thr):
    """the greedy NMS over sorted candidates 0..n-1 from a ``pair_ious`` table -> kept positions"""
    removed, kept = set(), []
    for i in range(n):
        if i in removed:
            continue
        kept.append(i)
        removed.update(j for (a, j), v in ious.items() if a == i and v > thr)
    return kept


# ---- family A: sweep and chunk geometry ------------------------------------------------------------------------------------------------------
def _grid(p):
    """position p's own place: 4 x 2 boxes on a 16 x 8 grid, none at a zero coordinate"""
    return 16.0 + 16.0 * (p % 32), 16.0 + 8.0 * (p // 32)


def _sweep(name, n, h, w, a, place=None, overlaps=(), removed=(), max_boxes=1000, disjoint=False, logits=None, seed=1, z_of=None):
    """``n`` candidates; sorted position p sits on its grid place, or ``place[p] = (q, dx)``: on q's place shifted by dx along x (boxes are
    4 long: |dx| = 2 is an IoU of 1/3 > 0.25, |dx| = 4 only touches).  ``overlaps``: the pairs of positions meant to exceed the threshold --
    the CPU file asserts that these and no others do; ``removed``: the positions the greedy sweep drops."""
    place = place or {}
    na = h * w * a
    step = 0.02 if n <= 300 else 0.01
    lg = (6.0 - step * np.arange(n)) if logits is None else np.asarray(logits, np.float64)
    slots = np.random.default_rng(seed).permutation(na)[:n] if logits is None else np.sort(np.random.default_rng(seed).permutation(na)[:n])
    boxes = []
    for p in range(n):
        q, dx = place.get(p, (p, 0.0))
        x, y = _grid(q)
        boxes.append(box(x + dx, y, z=-1.0 if z_of is None else z_of(p)))
    cls, reg, anchors = plant(boxes, lg, slots, h, w, a)
    return Case(name, "A", h, w, a, [(cls, reg, None, anchors, EYE)], thr=2.0 ** -10, max_boxes=max_boxes, disjoint=disjoint,
                info=dict(n=n, overlaps=set(overlaps), removed=set(removed), logits=lg, slots=slots))


def _all_pairs(n):
    return {(i, j) for i in range(n) for j in range(i + 1, n)}


A_CASES = {
    # box 0 removes 70 (one chunk on), 70 would remove 140 but is removed itself; 1 removes 150 two chunk boundaries on; 63 (bit 63 of
    # chunk 0) removes 64 (bit 0 of chunk 1), which would remove 128
    "chain": lambda: _sweep("chain", 200, 3, 71, 2, {70: (0, 2.0), 140: (0, 4.0), 150: (1, 2.0), 64: (63, 2.0), 128: (63, 4.0)},
                            [(0, 70), (70, 140), (1, 150), (63, 64), (64, 128)], [70, 150, 64]),
    "bit63": lambda: _sweep("bit63", 130, 3, 59, 2, {64: (63, 2.0), 127: (63, -2.0)}, [(63, 64), (63, 127)], [64, 127]),
    # inside one chunk (0 -> 5 -> 10: the kept row's own-chunk word) and across (3 -> 40 -> 100: the OR over the kept rows only)
    "silent": lambda: _sweep("silent", 130, 3, 59, 2, {5: (0, 2.0), 10: (0, 4.0), 40: (3, 2.0), 100: (3, 4.0)},
                             [(0, 5), (5, 10), (3, 40), (40, 100)], [5, 40]),
    # 130 copies of one bottom face (their z tells them apart: the NMS is on the bottom faces alone)
    "identical": lambda: _sweep("identical", 130, 3, 59, 2, {p: (0, 0.0) for p in range(130)}, _all_pairs(130), range(1, 130),
                                z_of=lambda p: -1.0 - p / 128.0),
    "identical_equal": lambda: _sweep("identical_equal", 130, 3, 59, 2, {p: (0, 0.0) for p in range(130)}, _all_pairs(130), range(1, 130),
                                      logits=np.full(130, 1.5), z_of=lambda p: -1.0 - p / 128.0),
    **{f"nvalid{n}": (lambda n=n: _sweep(f"nvalid{n}", n, 3, 59, 2, disjoint=True)) for n in (63, 64, 65, 128)},
    **{f"topk{k}": (lambda k=k: _sweep(f"topk{k}", 300, 3, 59, 2, max_boxes=k, disjoint=True)) for k in (1, 63, 64, 65)},
    "topk1024": lambda: _sweep("topk1024", 1100, 5, 121, 2, max_boxes=1024, disjoint=True),
    **{f"tiny{h * w * a}": (lambda h=h, w=w, a=a: _sweep(f"tiny{h * w * a}", h * w * a, h, w, a, disjoint=True))
       for h, w, a in ((1, 1, 1), (1, 1, 2), (3, 7, 3), (5, 13, 1))},
    "nothing": lambda: _sweep("nothing", 0, 3, 59, 2, disjoint=True),
}


# ---- family B: selection ---------------------------------------------------------------------------------------------------------------------
SEL_W, SEL_TOPK, SEL_CAP = 2597, 64, 2048


def family_logit(k):
    """the logit whose fp32 sigmoid has the bits 0x3F800000 - 2 k (k = 1 .. 120): exp(-x) = k 2^-23 to a relative 1e-7, 1 + k 2^-23 is an
    fp32 number and swallows that error whole, and 1 / (1 + k 2^-23) = 1 - k 2^-23 + k^2 2^-46 rounds to 1 - 2 k 2^-24"""
    return F32(-np.log(np.asarray(k, np.float64) * 2.0 ** -23))


def family_bits(k):
    return (0x3F800000 - 2 * np.asarray(k, np.int64)).astype(np.uint32)


ONE_LOGIT = F32(20.0)            # sigmoid = 1.0 exactly: the next 24-bit prefix


def _sel_box(slot, **kw):
    return box(16.0 + 4.0 * (slot % 64), 16.0 + 4.0 * (slot // 64), **{**dict(l=2.0, w=2.0), **kw})


def _sel(name, slots, logits, boxes=None, **info):
    slots = np.asarray(slots, np.int64)
    boxes = [_sel_box(int(s)) for s in slots] if boxes is None else boxes
    cls, reg, anchors = plant(boxes, logits, slots, 1, SEL_W, 1)
    return Case(name, "B", 1, SEL_W, 1, [(cls, reg, None, anchors, EYE)], max_boxes=SEL_TOPK, disjoint=True, score_bits=True,
                info=dict(slots=slots, logits=np.asarray(logits, F32), **info))


def _sel_crowd(name, n_family, extra_tie=False, seed=7):
    """10 slots at 1.0 and ``n_family`` from the score family, all sharing one 24-bit prefix: more than SEL_CAP survivors when n_family >
    2038.  k = 1, 2, 3, 4 hold 7 + 11 + 13 + 9 = 40 slots (four low-byte bins above the cut); k = 5 holds 30, of which 14 enter;
    everything else is spread over k = 6 .. 120.  The selection numbers a candidate by its rank c among the flagged slots (the scan's order)
    and settles ties by c >> 10, then c & 1023: of the 30 ties 6 have c < 1024, and 12 each 1024 <= c < 2048 and c >= 2048 -- or, where
    there is no third group, 24 the former -- so the 14th tie is the 8th of the second group; counted from the top group down it would not be.
    ``extra_tie``: one candidate more with k = 5, the last of all (c = 2048, alone in the third group)."""
    g = np.random.default_rng(seed)
    n = 10 + n_family + int(extra_tie)
    body = n - int(extra_tie)
    used = np.sort(g.permutation(SEL_W - 1)[:body])                # the planted slots: candidate c sits at used[c]
    if extra_tie:
        used = np.append(used, SEL_W - 1)                          # (the last slot: everything else as without it)
    groups = [(0, 1024, 6), (1024, 2048, 12), (2048, body, 12)] if body >= 2048 + 12 else [(0, 1024, 6), (1024, 2048, 24)]
    tie_c = np.sort(np.concatenate([lo + g.permutation(hi - lo)[:m] for lo, hi, m in groups]))
    rest = np.setdiff1d(np.arange(body), tie_c)
    rest = rest[g.permutation(len(rest))]
    ks = np.concatenate([np.full(7, 1), np.full(11, 2), np.full(13, 3), np.full(9, 4)])
    ks = np.concatenate([ks, 6 + np.arange(n_family - 30 - len(ks)) % 115])
    assert len(rest) == 10 + len(ks)
    cand = np.concatenate([rest[:10], tie_c, rest[10:]])
    logits = np.concatenate([np.full(10, ONE_LOGIT), np.full(30, family_logit(5)), family_logit(ks)])
    if extra_tie:
        cand, logits = np.append(cand, n - 1), np.append(logits, family_logit(5))
    return _sel(name, used[cand], logits, survivors=n, tie_slots=used[tie_c], cut_k=5, ties_in=14)


def _sel_small(name, n, tied_tail=False, bad=()):
    """``n`` candidates at scattered slots with the scores k = 1 .. n of the family (``tied_tail``: the last two share a score); ``bad``:
    (rank, kind) -- the candidate of that rank fails a size / z filter"""
    slots = np.random.default_rng(11).permutation(SEL_W)[:n]
    ks = np.arange(1, n + 1)
    if tied_tail:
        ks[-1] = ks[-2]
        slots[-2:] = np.sort(slots[-2:])
    kinds = dict(bad)
    mk = {None: {}, "long": dict(l=8.0), "flat": dict(w=0.0), "low": dict(z=-3.0), "high": dict(z=1.0)}
    boxes = [_sel_box(int(s), **mk[kinds.get(r)]) for r, s in enumerate(slots)]
    return _sel(name, slots, family_logit(ks), boxes, n=n, bad=sorted(kinds))


B_CASES = {
    "sel_lowbyte": lambda: _sel_crowd("sel_lowbyte", 2500),
    "sel_cap2048": lambda: _sel_crowd("sel_cap2048", 2038),
    "sel_cap2049": lambda: _sel_crowd("sel_cap2049", 2038, extra_tie=True),
    "sel_fewer": lambda: _sel_small("sel_fewer", 40),
    "sel_exact": lambda: _sel_small("sel_exact", 64),
    "sel_plus1": lambda: _sel_small("sel_plus1", 65, tied_tail=True),
    "sel_bad61": lambda: _sel_small("sel_bad61", 66, bad=[(0, "long"), (3, "flat"), (10, "low"), (11, "high"), (40, "long")]),
    "sel_bad_cut": lambda: _sel_small("sel_bad_cut", 70, bad=[(0, "flat"), (1, "long"), (30, "low"), (62, "high"), (63, "long")]),
}


# ---- family C: comparisons at equality -------------------------------------------------------------------------------------------------------
def _up(x, steps=1):
    x = F32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf if steps > 0 else -np.inf))
    return float(x)


def _few(name, boxes, logits, expect, **kw):
    """boxes at the first slots of a 1 x 3 x 1 map; ``expect``: which of them come out, in output order"""
    cls, reg, anchors = plant(boxes, logits, range(len(boxes)), 1, 3, 1)
    return Case(name, "C", 1, 3, 1, [(cls, reg, None, anchors, EYE)], info=dict(expect=list(expect)), **kw)


C_RANGE = (-32.0, -16.0, -4.0, 32.0, 16.0, 2.0)
# a 4 x 2 box whose corner lies on a range face, and one fp32 step beyond it (the centres are fp32 numbers, so are the corners)
_FACES = {"xhi": (30.0, 0.5, 30.0 + 2.0 ** -18, 0.5), "xlo": (-30.0, 0.5, -30.0 - 2.0 ** -18, 0.5),
          "yhi": (0.5, 15.0, 0.5, 15.0 + 2.0 ** -19), "ylo": (0.5, -15.0, 0.5, -15.0 - 2.0 ** -19)}
# a box of height 6 about z = -1 fills the z range [-4, 2] exactly; moved by one step of the face it leaves it
_ZFACES = {"zon": -1.0, "zhi": -1.0 + 2.0 ** -22, "zlo": -1.0 - 2.0 ** -21}

C_CASES = {
    # two 3 x 1 boxes shifted by 1: intersection 2, union 4
    "iou_eq_kept": lambda: _few("iou_eq_kept", [box(16.5, 8.0, 3.0, 1.0), box(17.5, 8.0, 3.0, 1.0)], [2.0, 1.0], [0, 1], nms_thr=0.5),
    "iou_eq_above": lambda: _few("iou_eq_above", [box(16.5, 8.0, 3.0, 1.0), box(17.5, 8.0, 3.0, 1.0)], [2.0, 1.0], [0], nms_thr=0.25),
    # centre x = 0: the x extent is l itself
    "extent_eq": lambda: _few("extent_eq", [box(0.0, 16.0, 6.0, 2.0), box(0.0, 32.0, _up(6.0), 2.0)], [2.0, 1.0], [0]),
    "extent_eq_y": lambda: _few("extent_eq_y", [box(16.0, 0.0, 2.0, 6.0), box(32.0, 0.0, 2.0, _up(6.0))], [2.0, 1.0], [0]),
    "w_zero": lambda: _few("w_zero", [box(16.0, 8.0, 4.0, 0.0), box(32.0, 8.0)], [2.0, 1.0], [1]),
    "z_eq": lambda: _few("z_eq", [box(16.0, 8.0, z=-1.0, h=4.0)], [2.0], [0]),
    "z_below": lambda: _few("z_below", [box(16.0, 8.0, z=-1.0, h=_up(4.0)), box(32.0, 8.0)], [2.0, 1.0], [1]),
    "z_above": lambda: _few("z_above", [box(16.0, 8.0, z=-1.0 + 2.0 ** -23, h=4.0), box(32.0, 8.0)], [2.0, 1.0], [1]),
    **{f"range_{f}": (lambda f=f: _few(f"range_{f}", [box(*_FACES[f][:2]), box(*_FACES[f][2:])], [2.0, 1.0], [0], rng=C_RANGE)) for f in _FACES},
    **{f"range_{f}_xy{xy}": (lambda f=f, xy=xy: _few(f"range_{f}_xy{xy}", [box(8.0, 4.0, z=_ZFACES[f], h=6.0)], [2.0],
                                                    [0] if (f == "zon" or xy) else [], rng=C_RANGE, z_lim=(-100.0, 100.0), xy_only=bool(xy)))
       for f in _ZFACES for xy in (0, 1)},
    # sigmoid(0) = 1 / (1 + exp(-0)) = 0.5 exactly: not above a threshold of 0.5
    "score_eq": lambda: _few("score_eq", [box(16.0, 8.0), box(32.0, 8.0)], [0.0, 0.5], [1], thr=0.5),
}


# ---- family D: late fusion and batches -------------------------------------------------------------------------------------------------------
def _late(name, h, w, a, plan, seed=5):
    """``plan``: per CAV a list of (ego x, ego y, logit, slot or None); CAV c's matrix is the translation by (8 c, -4 c, c / 4), its
    anchors hold ego - translation: all dyadic, the projected corners exact.  A slot of None: dealt by a seeded permutation."""
    cavs, rows = [], []
    na1 = h * w * a
    for c, items in enumerate(plan):
        tx, ty, tz = 8.0 * c, -4.0 * c, c / 4.0
        given = [s for *_, s in items if s is not None]
        spare = [int(s) for s in np.random.default_rng(seed + c).permutation(na1) if int(s) not in given]
        slots = [s if s is not None else spare.pop() for *_, s in items]
        boxes = [box(x - tx, y - ty, z=-1.0 - tz) for x, y, _, _ in items]
        cls, reg, anchors = plant(boxes, [lg for _, _, lg, _ in items], slots, h, w, a)
        cavs.append((cls, reg, None, anchors, translation(tx, ty, tz)))
        rows += [(c, s, x, y, lg) for (x, y, lg, _), s in zip(items, slots)]
    return Case(name, "D", h, w, a, cavs, info=dict(rows=rows))


def _late8():
    plan = []
    for c in range(8):
        y = 16.0 + 8.0 * c
        plan.append([(16.0, y, 3.0 - 0.1 * c, None),             # its own box, a score of its own
                     (48.0, y, 1.0, None),                       # eight boxes tied across the CAVs: CAV order
                     (80.0, y, 0.5, 7), (112.0, y, 0.5, 90)])    # two tied inside the CAV: slot order
    plan[5].append((16.0, 128.0, 4.0, None)); plan[2].append((18.0, 128.0, 3.5, None))        # CAV 5's box removes CAV 2's
    plan[1].append((48.0, 128.0, 2.0, 100)); plan[6].append((50.0, 128.0, 2.0, 3))            # tied and overlapping: CAV 1's stays
    c = _late("late8", 1, 37, 3, plan)
    c.info.update(removed=[(2, 18.0, 128.0), (6, 50.0, 128.0)])
    return c


def _late3():
    """na1 = 257: two workgroups per CAV, the second with one anchor -- boxes at slots 0, 255 and 256 of every CAV"""
    plan = [[(16.0 + 16.0 * j, 16.0 + 8.0 * c, 3.0 - 0.3 * j - 0.05 * c, s) for j, s in enumerate((0, 255, 256))] for c in range(3)]
    plan[0].append((18.0, 32.0, 1.0, 128))                       # overlaps CAV 2's slot-0 box (16, 32), which scores higher
    c = _late("late3_257", 1, 257, 1, plan)
    c.info.update(removed=[(0, 18.0, 32.0)])
    return c


def _batch3():
    """three frames of 111 anchors over shared anchors: nothing | one box | a chain over two chunk boundaries (0 -> 40 -> 80 inside and
    across chunks, 63 -> 64 -> 100), each frame with its own dyadic translation"""
    h, w, a, n = 1, 37, 3, 105
    place = {40: (0, 2.0), 80: (0, 4.0), 64: (63, 2.0), 100: (63, 4.0)}
    slots = np.random.default_rng(2).permutation(h * w * a)[:n]
    boxes = []
    for p in range(n):
        q, dx = place.get(p, (p, 0.0))
        x, y = _grid(q)
        boxes.append(box(x + dx, y))
    lg = 6.0 - 0.02 * np.arange(n)
    cls2, reg, anchors = plant(boxes, lg, slots, h, w, a)
    cls0, _, _ = plant([], [], [], h, w, a)
    cls1, _, _ = plant(boxes[17:18], lg[17:18], slots[17:18], h, w, a)
    # (the frames share the anchors: frame 1's one box is the chain's box 17)
    frames = [(cls0, reg, None, anchors, translation(1.0, 2.0)), (cls1, reg, None, anchors, translation(-4.0, 0.5, 0.25)),
              (cls2, reg, None, anchors, translation(0.0, -8.0))]
    return Case("batch3", "D", h, w, a, frames, thr=2.0 ** -10, batch=True,
                info=dict(counts=[0, 1, n - 2], overlaps={(0, 40), (40, 80), (63, 64), (64, 100)}, removed={40, 64}))


D_CASES = {"late8": _late8, "late3_257": _late3, "batch3": _batch3}


# ---- family E: heads the descriptor allows -----------------------------------------------------------------------------------------------------
def _classes(name, ncls, h, w, a, seed=3):
    """every slot planted (h w a boxes on the grid, pairwise disjoint) with ``ncls`` dyadic class logits: slot 0 -- all classes equal
    (label 1); slot 1 -- the last class largest; slot 2 -- the first and the last tied at the top (label 1); slot 3 -- two tied in the
    middle below the winner; the rest seeded, ties allowed (integers / 4 in [-1, 3])"""
    na = h * w * a
    g = np.random.default_rng(seed)
    lg = g.integers(-4, 13, size=(na, ncls)).astype(np.float64) / 4.0
    lg[0] = 1.0
    lg[1] = np.linspace(-1.0, 2.5, ncls)
    lg[2] = 0.25; lg[2, 0] = lg[2, -1] = 2.0
    lg[3] = -0.5; lg[3, ncls // 2] = 3.0
    # a slot's own dyadic offset below 1/4 on all its classes: ties inside the slot stay ties, the best logits of two slots differ by at
    # least 2^-10 (a score step of 3e-5 or more at these logits: the output order cannot hang on an ulp of expf)
    lg += g.permutation(na)[:, None] / 1024.0
    boxes = [box(*_grid(s)) for s in range(na)]
    cls, reg, anchors = plant(boxes, lg, range(na), h, w, a, ncls=ncls)
    return Case(name, "E", h, w, a, [(cls, reg, None, anchors, EYE)], ncls=ncls, thr=0.2, disjoint=True, xy_only=True, max_extent=100.0,
                z_lim=(-100.0, 100.0), info=dict(logits=lg))


def _bins(name, nbins):
    """3 x 7 x 2 slots; boxes of 3 x 1.5 on an 8 m grid inside |x| < 64; anchor yaws 0.05 rad on either side of every period boundary
    dir_offset + m period; direction logits that tie between the wanted bin and a later one (the first maximum wins); up to four more boxes
    half a metre from one of the first, same yaw and direction logits: an IoU far above the threshold"""
    h, w, a = 3, 7, 2
    period = 2 * math.pi / nbins
    yaws = [DIR_OFFSET + m * period + e for m in range(nbins) for e in (-0.05, 0.05)]
    n = len(yaws)
    slots = np.random.default_rng(4).permutation(h * w * a)[:n + min(4, n)]
    boxes = [box(-24.0 + 8.0 * (p % 7), -8.0 + 8.0 * (p // 7), 3.0, 1.5, yaw=yaws[p]) for p in range(n)]
    labels = [p % nbins for p in range(n)]
    extras = min(4, n)
    for p in range(extras):
        base = p * (n // extras)
        b = list(boxes[base]); b[0] += 0.5
        boxes.append(tuple(b)); labels.append(labels[base])
    lg = 3.0 - 0.1 * np.arange(n + extras)
    cls, reg, anchors = plant(boxes, lg, slots, h, w, a)
    d = np.zeros((h * w * a, nbins), F32)
    for p, s in enumerate(slots):
        d[s, :] = [(-1.0) ** b for b in range(nbins)]
        d[s, labels[p]] = 2.0
        if labels[p] + 2 < nbins:
            d[s, labels[p] + 2] = 2.0
    dirp = np.ascontiguousarray(d.reshape(h, w, a * nbins).transpose(2, 0, 1)[None])
    return Case(name, "E", h, w, a, [(cls, reg, dirp, anchors, EYE)], nbins=nbins, dir_offset=DIR_OFFSET, exact=False,
                info=dict(labels=labels, slots=slots, n=n, extras=extras))


E_CASES = {
    "classes2_a1": lambda: _classes("classes2_a1", 2, 3, 5, 1),
    "classes8_a16": lambda: _classes("classes8_a16", 8, 3, 5, 16),
    **{f"bins{b}": (lambda b=b: _bins(f"bins{b}", b)) for b in (1, 4, 8)},
}


# ---- family F: rotated NMS ---------------------------------------------------------------------------------------------------------------------
def _rotated(seed=12):
    """40 boxes, every slot of a 5 x 4 x 2 map, in clusters 16 m apart: the hand-made overlaps of the IoU cross-check turned into boxes, and
    eight seeded clusters of three boxes with arbitrary yaws"""
    g = np.random.default_rng(seed)
    q = math.pi / 4
    clusters = [
        [box(0, 0, 4, 2, yaw=0.3), box(0, 0, 4, 2, yaw=0.3)],                          # identical
        [box(0, 0, 4, 4, yaw=q), box(0, 0, 1, 1, yaw=0.2)],                            # one inside the other: 1/16
        [box(0, 0, 4, 2), box(4, 0, 4, 2)],                                            # shared edge
        [box(0, 0, 4, 2), box(4, 2, 4, 2)],                                            # shared vertex
        [box(0, 0, 4, 2), box(0, 0, 4, 2, yaw=2 * q)],                                 # a cross: 4 / 12
        [box(0, 0, 2, 2), box(0, 0, 2, 2, yaw=q)],                                     # the 45 degree square: 0.707
        [box(0, 0, 4, 2, yaw=-q), box(0.25, 0.25, 4, 0, yaw=q)],                       # a zero-width box across a box
    ]
    while sum(len(c) for c in clusters) < 38:
        clusters.append([box(*g.uniform(-1.5, 1.5, 2), g.uniform(2.0, 4.5), g.uniform(1.0, 2.5), yaw=g.uniform(-math.pi, math.pi)) for _ in range(3)])
    clusters += [[box(0, 0, 3, 1.5, yaw=1.0)], [box(0, 0, 3, 1.5, yaw=-2.0)]]
    boxes = []
    for c, cl in enumerate(clusters):
        ox, oy = -40.0 + 16.0 * (c % 6), -24.0 + 16.0 * (c // 6)
        boxes += [(b[0] + ox, b[1] + oy) + tuple(b[2:]) for b in cl]
    assert len(boxes) == 40
    lg = 3.0 - 0.05 * g.permutation(40)
    cls, reg, anchors = plant(boxes, lg, g.permutation(40), 5, 4, 2)
    return Case("rotated40", "F", 5, 4, 2, [(cls, reg, None, anchors, EYE)], exact=False)


F_CASES = {"rotated40": _rotated}

BUILDERS = {**A_CASES, **B_CASES, **C_CASES, **D_CASES, **E_CASES, **F_CASES}
CASES = list(BUILDERS)
# inexact corners (1e-5 on boxes of 1 - 4 m) move an IoU by about perimeter * 1e-5 / area = 1e-4: no IoU of such a case is this close to the threshold
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def build(name):
    case = BUILDERS[name]()
    assert case.name == name
    return case
