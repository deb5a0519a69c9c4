"""qv2x_postprocess_batch_f32 (through ``gpu_post_process_batch``) against a loop of qv2x_postprocess_f32 calls: bit for bit per frame.
Head maps of 48 x 88 cells with 2 anchors (8 448 slots: the selection's SEL_CAP = 2048 fallback is within reach), 64 boxes at most.
oracle/postprocess.py says on the CPU which case a frame is, and pins the few-dozen-candidates frame (1e-5: the tolerance of
tests/test_hip_postprocess.py).  Needs an MI355X."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from oracle import postprocess as P

pytestmark = pytest.mark.gpu
H, W, A, MAX_BOXES = 48, 88, 2, 64
LIDAR = [-35.2, -19.2, -3.0, 35.2, 19.2, 1.0]
THR, NMS, DIR_OFFSET = 0.2, 0.15, 0.7853
CONFIGS = {   # name: (num_classes, num_bins, range_xy_only, max_extent, z_lim)
    "one_class": (1, 0, False, 6.0, (-3.0, 1.0)),
    "three_heads": (3, 0, True, 100.0, (-100.0, 100.0)),
    "direction": (1, 2, False, 6.0, (-3.0, 1.0)),
}


def _rot(yaw, tx, ty, tz=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]], np.float32)


TRANSFORMS = np.stack([np.eye(4, dtype=np.float32), _rot(0.3, 1.5, -0.7), _rot(0.0, -2.0, 1.0, 0.1), _rot(-1.0, 0.5, 0.25), _rot(0.3, 1.5, -0.7)])


def _frames(ncls, nbins, seed=5):
    """five frames: nothing above the threshold | a few dozen candidates | far more than max_boxes | 3 000 equal top scores | frame 1 again"""
    g = np.random.default_rng(seed)
    ch = A * ncls
    cls = np.empty((5, ch, H, W), np.float32)
    reg = g.normal(0.0, 0.05, size=(5, 7 * A, H, W)).astype(np.float32)
    dirp = g.normal(0.0, 1.0, size=(5, nbins * A, H, W)).astype(np.float32) if nbins else None
    cls[0] = -9.0
    cls[1] = g.normal(-6.0, 0.8, size=(ch, H, W))
    for _ in range(5):                                                   # planted objects: 3 x 3 overlapping detections each
        y, x, c = int(g.integers(2, H - 2)), int(g.integers(2, W - 2)), int(g.integers(0, ch))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cls[1, c, y + dy, x + dx] = abs(g.normal(1.5, 1.0))
                reg[1, (c // ncls) * 7 + 0, y + dy, x + dx] = -dx * 0.8 / 4.2 + g.normal(0, 0.02)
                reg[1, (c // ncls) * 7 + 1, y + dy, x + dx] = -dy * 0.8 / 4.2 + g.normal(0, 0.02)
    cls[2] = g.normal(-1.0, 1.0, size=(ch, H, W))
    cls[3] = g.normal(-1.0, 0.1, size=(ch, H, W))                        # above the threshold of 0.2, below the ties
    cls[3].reshape(ch, H * W)[0, g.choice(H * W, size=3000, replace=False)] = 2.5
    cls[4], reg[4] = cls[1], reg[1]
    if nbins:
        dirp[4] = dirp[1]
    return cls, reg, dirp


def _candidates(cfg, cls, reg, dirp, anchors, f):
    ncls, nbins = CONFIGS[cfg][:2]
    return P._candidates(cls[f:f + 1], reg[f:f + 1], None if dirp is None else dirp[f:f + 1], anchors, TRANSFORMS[f], THR, DIR_OFFSET, nbins, ncls)


def _owner():
    return types.SimpleNamespace(params={"target_args": {"score_threshold": THR}, "nms_thresh": NMS}, _ws=None)


def _kw(cfg):
    ncls, nbins, xy, ext, zl = CONFIGS[cfg]
    return dict(anchors_per_cell=A, num_classes=ncls, num_bins=nbins, dir_offset=DIR_OFFSET if nbins else 0.0, rng=LIDAR, range_xy_only=xy,
                max_extent=ext, z_lim=zl, max_boxes=MAX_BOXES)


def _single(cfg, cls, reg, dirp, anchors, t):
    """one qv2x_postprocess_f32 call on one frame's maps (device tensors [C, H, W]); t: numpy 4x4 -> (corners, scores, labels, count)"""
    from quantv2x_amd import lib as L
    lib = L.load()
    ncls, nbins, xy, ext, zl = CONFIGS[cfg]
    d = L.PostprocessDesc()
    d.h, d.w, d.anchors_per_cell, d.num_bins = H, W, A, nbins
    d.score_threshold, d.nms_threshold, d.dir_offset = THR, NMS, DIR_OFFSET if nbins else 0.0
    for i, v in enumerate(LIDAR):
        d.range[i] = v
    for i, v in enumerate(np.asarray(t, np.float32).reshape(16)):
        d.transform[i] = float(v)
    d.max_boxes, d.num_classes, d.range_xy_only, d.max_extent, d.z_min, d.z_max = MAX_BOXES, ncls, int(xy), ext, zl[0], zl[1]
    need = lib.qv2x_postprocess_workspace_bytes(C.byref(d))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    corners = torch.empty((MAX_BOXES, 8, 3), dtype=torch.float32, device="cuda")
    scores = torch.empty((MAX_BOXES,), dtype=torch.float32, device="cuda")
    labels = torch.empty((MAX_BOXES,), dtype=torch.int32, device="cuda")
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    assert cls.is_contiguous() and reg.is_contiguous()
    L.check(lib.qv2x_postprocess_f32(C.byref(d), L.ptr(cls), L.ptr(reg), L.ptr(dirp if nbins else None), L.ptr(anchors), L.ptr(ws), need,
                                     L.ptr(corners), L.ptr(scores), L.ptr(labels), L.ptr(count), L.current_stream()), "qv2x_postprocess_f32")
    torch.cuda.synchronize()
    return corners, scores, labels, count


def _assert_frames_equal(cfg, got, cls, reg, dirp, anchors, transforms):
    """every frame of the batch result == the single entry on that frame, on the rows the count covers (the rows past it are not written
    by either entry)"""
    corners, scores, labels, counts = got
    torch.cuda.synchronize()
    ks = []
    for f in range(cls.shape[0]):
        sc, ss, sl, sn = _single(cfg, cls[f].contiguous(), reg[f].contiguous(), None if dirp is None else dirp[f].contiguous(), anchors, transforms[f])
        k = int(sn)
        assert int(counts[f]) == k, (f, int(counts[f]), k)
        assert torch.equal(corners[f, :k], sc[:k]) and torch.equal(scores[f, :k], ss[:k]) and torch.equal(labels[f, :k], sl[:k]), f
        ks.append(k)
    return ks


@pytest.fixture(scope="module")
def anchors():
    return P.generate_anchor_box(LIDAR, 2 * W, 2 * H, 0.4, 0.4).astype(np.float32)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_five_frames_equal_the_single_entry(cfg, anchors):
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process_batch
    ncls, nbins = CONFIGS[cfg][:2]
    assert anchors.shape == (H, W, A, 7)
    cls, reg, dirp = _frames(ncls, nbins)
    # on the CPU: every frame is the case it is meant to be
    cand = [_candidates(cfg, cls, reg, dirp, anchors, f) for f in range(5)]
    n = [len(c[1]) for c in cand]
    assert n[0] == 0 and 24 <= n[1] <= MAX_BOXES and n[2] > 10 * MAX_BOXES and n[4] == n[1]
    top = cand[3][1].max()
    assert (cand[3][1] == top).sum() == 3000 and n[3] > 3000            # more equal scores at the cut than the selection's LDS sort holds (2048)
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    dcls, dreg, ddir, danc = dev(cls), dev(reg), dev(dirp), dev(anchors.reshape(-1, 7))
    got = gpu_post_process_batch(_owner(), dcls, dreg, ddir, danc, torch.from_numpy(TRANSFORMS).cuda(), **_kw(cfg))
    ks = _assert_frames_equal(cfg, got, dcls, dreg, ddir, danc, TRANSFORMS)
    assert ks[0] == 0 and 0 < ks[1] <= n[1] and ks[2] > 0 and ks[3] > 0
    # the copy of frame 1 (same maps, same matrix) gives frame 1's boxes
    k = ks[1]
    assert ks[4] == k and torch.equal(got[0][4, :k], got[0][1, :k]) and torch.equal(got[1][4, :k], got[1][1, :k])
    # frame 1 against the oracle's whole post-process (fewer candidates than max_boxes: the top-k cut plays no part)
    _, _, xy, ext, zl = CONFIGS[cfg]
    want = P.post_process(cls[1:2], reg[1:2], None if dirp is None else dirp[1:2], anchors, TRANSFORMS[1], LIDAR, THR, NMS, DIR_OFFSET, nbins, True,
                          ncls, ext, zl, xy, True)
    assert len(want[1]) == k and 0 < k < n[1]                            # the NMS removed something
    np.testing.assert_allclose(got[1][1, :k].cpu().numpy(), want[1], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got[0][1, :k].cpu().numpy(), want[0], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(got[2][1, :k].cpu().numpy(), want[2])


def test_one_frame_equals_the_single_entry(anchors):
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process_batch
    cls, reg, _ = _frames(1, 0)
    danc = torch.from_numpy(anchors.reshape(-1, 7)).cuda()
    for f in (2, 3):
        dcls, dreg, t = torch.from_numpy(cls[f:f + 1]).cuda(), torch.from_numpy(reg[f:f + 1]).cuda(), TRANSFORMS[f:f + 1]
        got = gpu_post_process_batch(_owner(), dcls, dreg, None, danc, torch.from_numpy(t).cuda(), **_kw("one_class"))
        assert got[0].shape == (1, MAX_BOXES, 8, 3) and got[3].shape == (1,)
        assert _assert_frames_equal("one_class", got, dcls, dreg, None, danc, t)[0] > 0


@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_single_entry_equals_the_oracle_on_the_crowded_frames(cfg, f, anchors):
    """qv2x_postprocess_f32 pinned to the CPU oracle directly (the batch-vs-single comparisons above run both sides through the same
    kernels): frame 2 -- far more candidates than max_boxes, the top-k selection cuts -- and frame 3 -- 3 000 tied top scores, the
    selection's tie-breaking by slot -- against oracle.postprocess.post_process with the NMS looking at the MAX_BOXES best scores: same
    boxes in the same order, labels equal, scores and corners to 1e-5 (the tolerance of tests/test_hip_postprocess.py)."""
    ncls, nbins, xy, ext, zl = CONFIGS[cfg]
    cls, reg, dirp = _frames(ncls, nbins)
    fdir = None if dirp is None else dirp[f:f + 1]
    want = P.post_process(cls[f:f + 1], reg[f:f + 1], fdir, anchors, TRANSFORMS[f], LIDAR, THR, NMS, DIR_OFFSET, nbins, True, ncls, ext, zl, xy,
                          True, top=MAX_BOXES)
    assert 1 <= len(want[1]) <= MAX_BOXES                                # on the CPU: the oracle keeps something
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    corners, scores, labels, count = _single(cfg, dev(cls[f]), dev(reg[f]), None if dirp is None else dev(dirp[f]), dev(anchors.reshape(-1, 7)),
                                             TRANSFORMS[f])
    k = int(count)
    print(f"{cfg} frame {f}: oracle keeps {len(want[1])}, the entry {k}")
    assert k == len(want[1])
    np.testing.assert_array_equal(labels[:k].cpu().numpy(), want[2])
    np.testing.assert_allclose(scores[:k].cpu().numpy(), want[1], rtol=0, atol=1e-5)
    np.testing.assert_allclose(corners[:k].cpu().numpy(), want[0], rtol=0, atol=1e-5)


def test_frames_at_a_stride(anchors):
    """head maps that are a slice of a larger tensor (the model's stacked cls | reg | dir predictions): taken where they are"""
    from quantv2x_amd.plugin.data_utils.post_processor import voxel_postprocessor as V
    cls, reg, dirp = _frames(1, 2)
    stacked = torch.from_numpy(np.concatenate([cls, reg, dirp], 1)).cuda()                # [5, 2 + 14 + 4, H, W]
    dcls, dreg, ddir = stacked[:, :2], stacked[:, 2:16], stacked[:, 16:]
    assert not dcls.is_contiguous() and V._frame_maps(dreg, 5)[0].data_ptr() == dreg.data_ptr() and V._frame_maps(dreg, 5)[1] == 20 * H * W
    danc = torch.from_numpy(anchors.reshape(-1, 7)).cuda()
    got = V.gpu_post_process_batch(_owner(), dcls, dreg, ddir, danc, torch.from_numpy(TRANSFORMS).cuda(), **_kw("direction"))
    ks = _assert_frames_equal("direction", got, dcls, dreg, ddir, danc, TRANSFORMS)
    assert ks[1] > 0 and ks[2] > 0


def test_batch_inside_a_hip_graph(anchors):
    """capture the call, change the maps and the matrices in place, replay: the new frames' boxes (nothing is copied from the host inside
    the call: the matrices are read from the device)"""
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process_batch
    cls, reg, _ = _frames(1, 0)
    order = [3, 1, 2, 0, 4]
    dcls, dreg = torch.from_numpy(cls).cuda(), torch.from_numpy(reg).cuda()
    dt = torch.from_numpy(TRANSFORMS).cuda()
    danc = torch.from_numpy(anchors.reshape(-1, 7)).cuda()
    owner = _owner()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            gpu_post_process_batch(owner, dcls, dreg, None, danc, dt, **_kw("one_class"))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = gpu_post_process_batch(owner, dcls, dreg, None, danc, dt, **_kw("one_class"))
    graph.replay()
    first = _assert_frames_equal("one_class", got, dcls, dreg, None, danc, TRANSFORMS)
    dcls.copy_(torch.from_numpy(cls[order])); dreg.copy_(torch.from_numpy(reg[order])); dt.copy_(torch.from_numpy(TRANSFORMS[order]))
    graph.replay()
    second = _assert_frames_equal("one_class", got, dcls, dreg, None, danc, TRANSFORMS[order])
    assert second == [first[i] for i in order] and first[0] == 0 and min(first[1:]) > 0
