"""Camera agents in the Pyramid model, the CPU side: the three statements of ``quantv2x_amd/camera_bev.py``, the mirror's crop mask against
the reference's own ``PyramidFusion`` (tests/golden/cam_pyramid.npz), the mirror model with a camera modality, and the host-side descriptor
checks of ``qv2x_bev_entry_f32``."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from _bev_entry import BLOCK, COUT, SHAPES, bev_map, block_state
from _camera_pyramid import calibrated_camera_model as build_calibrated, camera_hypes, camera_inputs, camera_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)                  # tests/test_pyramid_model.py: the mirror's fp32 maps against the reference's
LEVELS = [(16, 32), (8, 16), (4, 8)]


def info_of(rh, rw, m="m2"):
    return {m: {f"crop_ratio_W_{m}": float(rw), f"crop_ratio_H_{m}": float(rh)}}


# ---- the mask --------------------------------------------------------------------------------------------------------------------------------

def _rect(h, w, rows, cols):
    m = np.zeros((h, w), np.float32)
    if rows is not None:
        m[rows, cols] = 1
    return m.reshape(-1)


TABLE = {
    (0.8, 1.6): [(slice(0, 16), slice(8, 24)), (slice(1, 7), slice(5, 11)), (None, None)],
    (6.4 / 9.6, 12.8 / 9.6): [(slice(15, 16), slice(7, 25)), (slice(1, 7), slice(5, 11)), (None, None)],      # rows -1:17 = row 15 only
}


@pytest.mark.parametrize("ratios", list(TABLE))
def test_crop_mask_table(ratios):
    from quantv2x_amd.camera_bev import crop_mask_rect, crop_mask_statement
    info = info_of(*ratios)
    if ratios == (6.4 / 9.6, 12.8 / 9.6):
        assert crop_mask_rect(info, "m2", 16, 32) == (-1, 17, 7, 25)
    for (h, w), (rows, cols) in zip(LEVELS, TABLE[ratios]):
        got = crop_mask_statement(["m1", "m2"], info, h, w)
        assert got.shape == (2, h * w) and got.dtype == np.float32
        assert (got[0] == 1).all(), "a LiDAR agent keeps every score"
        np.testing.assert_array_equal(got[1], _rect(h, w, rows, cols))
    assert (crop_mask_statement(["m1", "m1"], {}, 4, 8) == 1).all()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_crop_mask_is_the_goldens_zero_pattern(golden, tag):
    from quantv2x_amd.camera_bev import crop_mask_statement
    g = golden["cam_pyramid"]
    mods, info = [str(m) for m in g[f"{tag}/modalities"]], info_of(g[f"{tag}/ratio_H"], g[f"{tag}/ratio_W"])
    for i, (h, w) in enumerate(LEVELS):
        score = g[f"{tag}/score{i}"].reshape(3, h * w)
        np.testing.assert_array_equal(score != 0, crop_mask_statement(mods, info, h, w) == 1, err_msg=f"level {i}")
    assert (g[f"{tag}/score2"][[j for j, m in enumerate(mods) if m == "m2"]] == 0).all(), "level 2: the camera agents are masked everywhere"


# ---- the mirror's fusion ---------------------------------------------------------------------------------------------------------------------

def _golden_inputs(g):
    x = torch.from_numpy(g["x_q"].astype(np.float32) / np.float32(64.0))
    return x, torch.tensor([3]), torch.from_numpy(g["affine"])


def _recorded(module_with_fuse, monkeypatch):
    """wraps ``weighted_fuse`` as seen by ``module_with_fuse`` and returns the list that receives each level's score"""
    scores, inner = [], module_with_fuse.weighted_fuse

    def recording(x, score, *a, **k):
        scores.append(score.detach().clone().numpy())
        return inner(x, score, *a, **k)
    monkeypatch.setattr(module_with_fuse, "weighted_fuse", recording)
    return scores


@pytest.fixture(scope="module")
def mirror_fusion(golden):
    torch.set_num_threads(1)           # the golden's recipe (make_golden_cam_pyramid.py), as tests/test_pyramid_model.py does for its own
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.models.fuse_modules.pyramid_fuse import PyramidFusion
    cfg = copy.deepcopy(synth.make_pyramid_hypes("tiny")["model"]["args"]["fusion_backbone"])
    model = PyramidFusion(cfg).eval()
    synth.load_state_dict_numpy(model, synth.make_state_dict(model.state_dict(), seed=int(golden["cam_pyramid"]["seed_w"])))
    return model


@pytest.mark.parametrize("tag", ["a", "b"])
def test_mirror_pyramid_fusion_masks_as_the_reference(golden, mirror_fusion, monkeypatch, tag):
    from quantv2x_amd.plugin.models.fuse_modules import pyramid_fuse
    g = golden["cam_pyramid"]
    x, rl, aff = _golden_inputs(g)
    mods, info = [str(m) for m in g[f"{tag}/modalities"]], info_of(g[f"{tag}/ratio_H"], g[f"{tag}/ratio_W"])
    scores = _recorded(pyramid_fuse, monkeypatch)
    with torch.no_grad():
        fused, occ = mirror_fusion(x, rl, aff, mods, info)
    assert len(scores) == 3
    for i in range(3):
        want = g[f"{tag}/score{i}"]
        np.testing.assert_array_equal(scores[i] == 0, want == 0, err_msg=f"level {i}: masked cells")
        np.testing.assert_array_equal(scores[i][want == 0], want[want == 0])
        np.testing.assert_allclose(scores[i], want, **TOL)
        np.testing.assert_allclose(occ[i].numpy(), g[f"{tag}/occ{i}"], **TOL)
    np.testing.assert_allclose(fused.numpy()[:, ::4], g[f"{tag}/fused"], **TOL)


def test_mirror_pyramid_fusion_training_mode_and_empty_info(golden, mirror_fusion, monkeypatch):
    """no mask in training mode (pyramid_fuse.py:147), none with an empty ``cam_crop_info``: the scores then hold no zero"""
    from quantv2x_amd.plugin.models.fuse_modules import pyramid_fuse
    g = golden["cam_pyramid"]
    x, rl, aff = _golden_inputs(g)
    scores = _recorded(pyramid_fuse, monkeypatch)
    with torch.no_grad():
        plain, _ = mirror_fusion(x, rl, aff, ["m1", "m2", "m2"], {})
        none, _ = mirror_fusion(x, rl, aff, ["m1", "m2", "m2"], None)
    assert torch.equal(plain, none) and all((s != 0).all() for s in scores)
    del scores[:]
    pyramid_fuse.level_score(torch.zeros(3, 1, 16, 32), ["m1", "m2", "m2"], info_of(0.8, 1.6), training=True)
    assert (pyramid_fuse.level_score(torch.zeros(3, 1, 16, 32), ["m1", "m2", "m2"], info_of(0.8, 1.6), training=True) != 0).all()
    assert (pyramid_fuse.level_score(torch.zeros(3, 1, 16, 32), ["m1", "m2", "m2"], info_of(0.8, 1.6), training=False)[1:, :, :, :8] == 0).all()


def test_quant_pyramid_fusion_applies_the_same_mask(golden, monkeypatch):
    from _common import calibrated_pyramid_plugin
    from quantv2x_amd.camera_bev import crop_mask_statement
    from quantv2x_amd.plugin.quant import quant_block
    g = golden["cam_pyramid"]
    x, rl, aff = _golden_inputs(g)
    qpf = calibrated_pyramid_plugin("tiny", n_agents=2, codebook=False).model.pyramid_backbone
    assert type(qpf).__name__ == "QuantPyramidFusion" and not qpf.training
    mods, info = ["m2", "m1", "m2"], info_of(6.4 / 9.6, 12.8 / 9.6)
    scores = _recorded(quant_block, monkeypatch)
    with torch.no_grad():
        today, occ_today = qpf(x, rl, aff)                                  # the call a LiDAR-only model makes
        empty, occ_empty = qpf(x, rl, aff, mods, {})
        plain = [s.copy() for s in scores]
        del scores[:]
        masked, _ = qpf(x, rl, aff, mods, info)
    assert torch.equal(today, empty) and all(torch.equal(a, b) for a, b in zip(occ_today, occ_empty))
    assert len(scores) == 3 and len(plain) == 6
    for i, (h, w) in enumerate(LEVELS):
        mask = crop_mask_statement(mods, info, h, w).reshape(3, 1, h, w)
        np.testing.assert_array_equal(scores[i], plain[i] * mask, err_msg=f"level {i}")
    assert not torch.equal(masked, today)


# ---- the crop --------------------------------------------------------------------------------------------------------------------------------

def test_center_crop_pad_statement():
    from quantv2x_amd.camera_bev import center_crop_pad_statement, center_crop_window, crop_target
    from quantv2x_amd.plugin.models.heter_pyramid_collab_mc import center_crop
    x = np.arange(2 * 20 * 20, dtype=np.float32).reshape(2, 20, 20) + 1
    # a crop in H (20 -> 16: rows 2..17) and a pad in W (20 -> 32: six zero columns on each side) at once
    y = center_crop_pad_statement(x, 16, 32)
    assert y.shape == (2, 16, 32)
    np.testing.assert_array_equal(y[:, :, 6:26], x[:, 2:18])
    assert (y[:, :, :6] == 0).all() and (y[:, :, 26:] == 0).all()
    # odd differences: Python's round is half-to-even -- a difference of 1 crops at 0 (round(0.5) = 0), of 3 at 2 (round(1.5) = 2)
    assert center_crop_window(20, 20, 19, 17) == ((0, 0, 0, 0), (0, 2))
    np.testing.assert_array_equal(center_crop_pad_statement(x, 19, 17), x[:, 0:19, 2:19])
    # odd pads: the extra cell goes right / below ((d + 1) // 2)
    assert center_crop_window(20, 20, 21, 23) == ((0, 1, 1, 2), (0, 0))
    z = center_crop_pad_statement(x, 21, 23, fill=7)
    np.testing.assert_array_equal(z[:, :20, 1:21], x)
    assert (z[:, 20] == 7).all() and (z[:, :, 0] == 7).all() and (z[:, :, 21:] == 7).all()
    np.testing.assert_array_equal(center_crop_pad_statement(x, 20, 20), x)
    for th, tw in ((16, 32), (19, 17), (21, 23), (20, 20)):
        np.testing.assert_array_equal(center_crop(torch.from_numpy(x), th, tw).numpy(), center_crop_pad_statement(x, th, tw))
    assert crop_target(20, 6.4 / 8.0) == 16 and crop_target(20, 12.8 / 8.0) == 32


# ---- the mirror model with a camera modality -------------------------------------------------------------------------------------------------

def test_mirror_model_with_a_camera_modality():
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.tools import train_utils
    model = train_utils.create_model(copy.deepcopy(camera_hypes(depth_supervision=True))).eval()
    assert model.sensor_type_dict == {"m1": "lidar", "m2": "camera"}
    assert type(model.encoder_m2).__name__ == "LiftSplatShoot"
    assert model.crop_ratio_W_m2 == 12.8 / 8.0 and model.crop_ratio_H_m2 == 6.4 / 8.0 and model.xdist_m2 == 16.0 and model.ydist_m2 == 16.0
    assert model.cam_crop_info == {"m2": {"crop_ratio_W_m2": 12.8 / 8.0, "crop_ratio_H_m2": 6.4 / 8.0}}
    assert not hasattr(model, "crop_ratio_W_m1")
    dd = camera_scene(["m1", "m2", "m2"])                                  # agents 1 and 2 are cameras
    with torch.no_grad():
        cam = model.backbone_m2(model.encoder_m2(dd, "m2"))
        assert tuple(cam.shape) == (2, 64, 20, 20)                         # 40 x 40 cells, stride 2
        feats = model.encode_agents(dd)
        assert tuple(feats.shape) == (3, 64, 16, 32)                       # cropped in H, padded in W
        np.testing.assert_array_equal(feats[1:, :, :, 6:26].numpy(), cam[:, :, 2:18].numpy())
        assert (feats[1:, :, :, :6] == 0).all() and (feats[1:, :, :, 26:] == 0).all()
        out = model(dd)
    assert tuple(out["preds_tensor"].shape[-2:]) == (16, 32) and "depth_items_m2" in out
    assert [tuple(o.shape) for o in out["occ_single_list"]] == [(3, 1, 16, 32), (3, 1, 8, 16), (3, 1, 4, 8)]
    with pytest.raises(NotImplementedError, match="sensor_type"):
        hy = camera_hypes()
        hy["model"]["args"]["m2"]["sensor_type"] = "radar"
        train_utils.create_model(hy)


# ---- the PTQ state of a camera modality ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def calibrated_camera_model():
    return build_calibrated()


def test_export_ptq_state_of_a_camera_modality(calibrated_camera_model):
    from quantv2x_amd.ptq_state import CAMERA_PREFIX, export_camera_state, export_ptq_state
    qt = calibrated_camera_model
    state = export_ptq_state(qt, modality="m2")
    assert str(state["meta/sensor_type"]) == "camera" and str(state["meta/modality"]) == "m2" and str(state["meta/encoder"]) == "lift_splat_shoot"
    cam = {k[len(CAMERA_PREFIX):]: v for k, v in state.items() if k.startswith(CAMERA_PREFIX)}
    want = export_camera_state(qt.model.encoder_m2)
    assert sorted(cam) == sorted(want) and "conv1/w_code" in cam and "layer2.3/a_delta" in cam
    for k in want:
        np.testing.assert_array_equal(cam[k], want[k], err_msg=k)
    assert not [k for k in state if k.startswith("encoder_m")] and "pfn/a2_delta" not in state
    assert state["backbone_m1.resnet.layer0.0.conv1/w_code"].shape == (64, 16, 3, 3)         # the camera's backbone under the _m1 names
    assert state["backbone_m1.resnet.layer0.0.downsample/w_code"].shape == (64, 16, 1, 1)
    assert int(state["meta/inplanes"]) == 16 and list(state["meta/grid"]) == [40, 40, 1] and int(state["meta/canvas_channels"]) == 16
    assert float(state["meta/crop_ratio_H"]) == 6.4 / 8.0 and float(state["meta/crop_ratio_W"]) == 12.8 / 8.0
    assert list(state["meta/layer_strides"]) == [2] and list(state["meta/layer_nums"]) == [2]
    lidar = export_ptq_state(qt, modality="m1")
    assert "meta/sensor_type" not in lidar and not [k for k in lidar if k.startswith(CAMERA_PREFIX)] and "pfn/a2_delta" in lidar
    assert lidar["backbone_m1.resnet.layer0.0.conv1/w_code"].shape == (64, 64, 3, 3)


def test_export_refusals_with_a_camera_modality(calibrated_camera_model, monkeypatch):
    from quantv2x_amd.ptq_state import export_ptq_state
    qt = calibrated_camera_model
    enc = qt.model.encoder_m2
    with monkeypatch.context() as mp:
        mp.setattr(enc, "camera_encoder_type", "EfficientNet")
        with pytest.raises(NotImplementedError, match="EfficientNet"):
            export_ptq_state(qt, modality="m2")
    with monkeypatch.context() as mp:
        mp.setattr(enc.camencode, "use_gt_depth", True)
        with pytest.raises(NotImplementedError, match="use_gt_depth"):
            export_ptq_state(qt, modality="m2")
    with monkeypatch.context() as mp:
        mp.setattr(enc, "__class__", type("QuantLiftSplatShootVoxel", (type(enc),), {}))
        with pytest.raises(NotImplementedError, match="Voxel"):
            export_ptq_state(qt, modality="m2")
    with monkeypatch.context() as mp:
        mp.setattr(qt.model.aligner_m2, "channel_align", torch.nn.Conv2d(64, 64, 1))
        with pytest.raises(NotImplementedError, match="aligner"):
            export_ptq_state(qt, modality="m2")
    export_ptq_state(qt, modality="m2")                                    # and the model itself still exports


# ---- the entry's statement -------------------------------------------------------------------------------------------------------------------

def _conv64(x, w_kc, stride):
    """float64 3x3 convolution (zero padding 1) of an NCHW map with [9 cin, cout] weights, and sum |x w|: ([n, ho, wo, cout], same)"""
    from quantv2x_amd.camera_bev import im2col_rows
    rows = im2col_rows(x, stride).astype(np.float64)
    w = w_kc.astype(np.float64)
    return rows @ w, np.abs(rows) @ np.abs(w)


@pytest.mark.parametrize("n,cin,h,w,stride", SHAPES)
def test_bev_entry_statement_against_float64(n, cin, h, w, stride):
    """An ascending fmaf chain of K terms from +0 plus one rounded add: each fma rounds once, so |fl - exact| <= (K + 1) u sum|x w| to first
    order, u = 2^-24; (K + 2) u covers the second-order terms (K u << 1)."""
    from quantv2x_amd.camera_bev import bev_entry_statement, chain_rows, entry_constants, im2col_rows
    from quantv2x_amd.camera_encoder import q_code_mul
    state, x = block_state(cin, COUT, True, 100 + cin + h), bev_map(n, cin, h, w, 101 + cin + h)
    codes, (da, za), short = bev_entry_statement(x, state, BLOCK, stride)
    w1, b1, q, wd, bd = entry_constants(state, BLOCK)
    assert q == (da, za) and codes.dtype == np.uint8 and short.dtype == np.float32
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert codes.shape == short.shape == (n, ho, wo, COUT)
    pre = chain_rows(im2col_rows(x, stride), w1)                           # the chain the codes were made of
    exact, mag = _conv64(x, w1, stride)
    K = 9 * cin
    y = (pre + b1[None, :]).astype(np.float32)
    assert (np.abs(y.astype(np.float64) - (exact + b1)) <= (K + 2) * 2.0 ** -24 * (mag + np.abs(b1))).all()
    np.testing.assert_array_equal(codes.reshape(-1, COUT), q_code_mul(np.maximum(y, 0), da, za).astype(np.uint8))
    centre = x[:, :, ::stride, ::stride].transpose(0, 2, 3, 1).reshape(-1, cin).astype(np.float64)
    sexact, smag = centre @ wd.astype(np.float64) + bd, np.abs(centre) @ np.abs(wd.astype(np.float64)) + np.abs(bd)
    assert (np.abs(short.reshape(-1, COUT).astype(np.float64) - sexact) <= (cin + 2) * 2.0 ** -24 * smag).all()


def test_bev_entry_statement_identity():
    from quantv2x_amd.camera_bev import bev_entry_statement
    state, x = block_state(64, 64, False, 5), bev_map(2, 64, 5, 7, 6)
    _, _, short = bev_entry_statement(x, state, BLOCK, 1)
    np.testing.assert_array_equal(short, x.transpose(0, 2, 3, 1))
    with pytest.raises(ValueError, match="no downsample"):
        bev_entry_statement(x, state, BLOCK, 2)


def test_pack_entry_weights():
    from quantv2x_amd.camera_bev import pack_entry_weights
    w = np.arange(16 * 3, dtype=np.float32).reshape(16, 3)
    p = pack_entry_weights(w)
    assert p.shape == (2, 3, 2, 4)
    for k in range(16):
        for co in range(3):
            assert p[k // 8, co, k % 2, (k % 8) // 2] == w[k, co]


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------

def test_cabi_of_the_bev_entry():
    from quantv2x_amd import build, lib
    header = open(os.path.join(ROOT, "include", "qv2x.h")).read()
    assert re.search(r"\bint qv2x_bev_entry_f32\(", header) and "qv2x_bev_entry_f32" in lib.SYMBOLS
    assert C.sizeof(lib.BevEntryDesc) == 8 * 4 + 2 * 4
    body = re.search(r"typedef struct \{([^}]*)\} qv2x_bev_entry_desc;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in lib.BevEntryDesc._fields_]
    build.build()
    l = lib.load()
    buf = np.zeros(256, np.float32)
    p, off = lib.ptr(buf), C.c_void_p(buf.ctypes.data + 4)

    def desc(**kw):
        d = lib.BevEntryDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.stride, d.downsample, d.out_delta, d.out_zp = 1, 4, 4, 16, 64, 2, 1, 0.1, 3.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    call = lambda d, *a: l.qv2x_bev_entry_f32(C.byref(d), *(a or (p, p, p, p, p, p, p)), None)     # noqa: E731
    for i in (0, 1, 2, 5, 6):                                               # in, w1, b1, out, shortcut
        args = [p] * 7
        args[i] = None
        assert call(desc(), *args) == -1 and b"null" in l.qv2x_last_error(), i
    assert call(desc(), p, p, p, None, p, p, p) == -1 and b"null" in l.qv2x_last_error()            # the downsample's weights when it has one
    for field, bad, code, word in (("n", 0, -1, b"positive"), ("h", 0, -1, b"positive"), ("w", -1, -1, b"positive"), ("stride", 3, -1, b"stride"),
                                   ("stride", 0, -1, b"stride"), ("out_delta", 0.0, -1, b"out_delta"), ("out_delta", float("nan"), -1, b"out_delta"),
                                   ("out_zp", 256.0, -1, b"out_zp"), ("downsample", 2, -1, b"downsample"), ("cin", 24, -2, b"cin"),
                                   ("cout", 96, -2, b"cout"), ("cin", 0, -1, b"cin"), ("cin", 256, -1, b"LDS")):
        assert call(desc(**{field: bad})) == code and word in l.qv2x_last_error(), (field, bad, l.qv2x_last_error())
    # the identity shortcut: stride 1 and cin == cout, and then no downsample weights are needed
    assert call(desc(downsample=0)) == -1 and b"identity" in l.qv2x_last_error()
    assert call(desc(downsample=0, stride=1, cin=64, cout=128)) == -1 and b"identity" in l.qv2x_last_error()
    for i in range(7):
        args = [p] * 7
        args[i] = off
        assert call(desc(), *args) == -2 and b"aligned" in l.qv2x_last_error(), i
