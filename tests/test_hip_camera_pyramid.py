"""Camera agents in the deployed Pyramid engines against the CPU statements, at the tiny shape of tests/_camera_pyramid.py (camera map 20 x 20,
LiDAR map 16 x 32: a crop in H and a pad in W).

The lift-splat's BEV agrees with its statement within DESIGN.md section 13's bound and not bit for bit, so the chain behind it is teacher-forced
on the ENGINE's own BEV: ``bev_entry_statement`` -> the oracle's conv2 / block end / BasicBlocks -> ``center_crop_pad_statement`` must then
equal the engine's taps on every code, ``enc_in``'s fill included.  On the ego side the per-level scores must equal the oracle's scores times
``crop_mask_statement`` exactly -- the level whose camera mask is all zero included -- and everything behind the fusion is compared as
tests/test_hip_pyramid.py compares it, with an oracle whose ``occupancy`` applies the same mask.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from _camera import codes_of, statement_chain
from _camera_pyramid import calibrated_camera_model, camera_scene
from _common import FUSE_TOL, interior_u8
from test_hip_pyramid import check_after_fuse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B0 = "backbone_m1.resnet.layer0.0"
MATRICES = ("rots", "trans", "intrins", "post_rots", "post_trans")


def masked_oracle(state, masks):
    """the CPU oracle with the camera crop mask on its scores (``masks``: per level f32 [n, h * w], or None)"""
    from oracle.spec_pyramid import OraclePyramid

    class Masked(OraclePyramid):
        def occupancy(self, lvl, x, xq):
            code, occ, score = super().occupancy(lvl, x, xq)
            if masks is not None:
                score = (score * masks[lvl].reshape(score.shape)).astype(np.float32)
            return code, occ, score
    return Masked(state)


def agent_chain(eng, state, taps, n):
    """the camera agent's side behind the BEV, teacher-forced on the engine's own BEV: every tap against the statements; returns the cropped
    codes u8 [n, fh, fw, 64] and their quantizer"""
    from quantv2x_amd.camera_bev import bev_entry_statement, center_crop_pad_statement
    orc = masked_oracle(state, None)
    bev = taps["bev"].cpu().numpy()
    codes, q, short = bev_entry_statement(bev, state, B0, eng.agent_stride)
    np.testing.assert_array_equal(codes_of(taps[B0 + ".conv1"]), codes, err_msg="conv1 of the first block")
    np.testing.assert_array_equal(taps[B0 + ".shortcut"].cpu().numpy().reshape(short.shape), short, err_msg="shortcut rows")
    y = orc.convg(B0 + ".conv2", codes, (np.float32(q[0]), int(q[1])), f32_out=True)
    x, xq = orc.finish(B0, y, short)
    np.testing.assert_array_equal(codes_of(taps[B0]), x, err_msg=B0)
    for i in range(1, len(eng.agent_blocks)):
        name = f"backbone_m1.resnet.layer0.{i}"
        x, xq = orc.residual_block(name, x, xq, 1, ["conv1", "conv2"])
        np.testing.assert_array_equal(codes_of(taps[name]), x, err_msg=name)
    want = center_crop_pad_statement(x.transpose(0, 3, 1, 2), eng.fh, eng.fw, fill=int(xq[1])).transpose(0, 2, 3, 1)
    assert want.shape == (n, 16, 32, 64) and (want[:, :, :6] == int(xq[1])).all()
    np.testing.assert_array_equal(codes_of(taps["enc_in"])[..., :64], want, err_msg="enc_in: the cropped map and its fill")
    return np.ascontiguousarray(want), xq


def check_bev(eng, inputs, taps, n):
    """the image encoder inside the Pyramid engine -- built from the ``camera/`` sub-state, one per (n, views), fed the 4-channel images --
    against the camera ``statement_chain`` on the same images: depth logits and features bit for bit; then the BEV within the splat's derived
    bound of its statement on those tensors"""
    from quantv2x_amd import lift_splat as ls
    views = int(inputs["imgs"].shape[1])
    assert list(eng.cam_encoders) == [(n, views)]
    enc = eng.cam_encoders[(n, views)]
    depth, feats, st = enc.depth.cpu().numpy(), enc.feats.cpu().numpy(), enc.splat
    imgs = inputs["imgs"].cpu().numpy().reshape(n * views, *inputs["imgs"].shape[2:])
    want_depth, want_feats = statement_chain(eng.cam_state, imgs)
    assert np.array_equal(depth.view(np.int32), want_depth.view(np.int32)), "depth logits against the camera statement chain"
    assert np.array_equal(feats.view(np.int32), want_feats.view(np.int32)), "image features against the camera statement chain"
    cells = ls.cells_statement(ls.geometry_statement(st.frustum, *(inputs[k].cpu().numpy() for k in MATRICES)), st.dx, st.bx, st.nx)
    want, mag, count = ls.splat_terms_statement(cells, depth, feats, "logits", nx=st.nx)
    diff = np.abs(taps["bev"].cpu().numpy().astype(np.float64) - want)
    assert (want != 0).any() and (diff <= ls.splat_bound(count, mag, feats.shape[1], float(np.abs(feats).max()))).all()


def check_ego(orc, state, sc, x, xq, masks, gtaps, got):
    """the pyramid on the agents' codes ``x``: scores = oracle scores x mask exactly, fused maps within FUSE_TOL, the rest as test_hip_pyramid"""
    otaps = {}
    orc.pyramid(None, sc["pairwise_t_matrix"].cpu().numpy(), [int(v) for v in sc["record_len"]], otaps, codes_in=(x, xq))
    plain = {}
    masked_oracle(state, None).pyramid(None, sc["pairwise_t_matrix"].cpu().numpy(), [int(v) for v in sc["record_len"]], plain, codes_in=(x, xq))
    for lvl in range(3):
        sco = plain[f"score{lvl}"]
        want = sco if masks is None else (sco * masks[lvl].reshape(sco.shape)).astype(np.float32)
        np.testing.assert_array_equal(gtaps[f"score{lvl}"].cpu().numpy().reshape(sco.shape), want, err_msg=f"score {lvl}")
        np.testing.assert_array_equal(gtaps[f"occ_code{lvl}"].cpu().numpy().reshape(otaps[f"occ_code{lvl}"].shape), otaps[f"occ_code{lvl}"])
        fu = otaps[f"fused{lvl}"]
        np.testing.assert_allclose(gtaps[f"fused{lvl}"].cpu().numpy().reshape(fu.shape), fu, **FUSE_TOL)
    check_after_fuse(orc, state, gtaps, got, otaps)


def test_camera_only_model_without_codebook():
    from quantv2x_amd.camera_bev import crop_mask_statement
    from quantv2x_amd.engine_pyramid import DeployedPyramidModel
    from quantv2x_amd.ptq_state import export_ptq_state
    qt = calibrated_camera_model(codebook=False, modalities=("m2",), agents=("m2", "m2"))
    state = export_ptq_state(qt, modality="m2")
    assert not bool(state["meta/has_codebook"])
    eng = DeployedPyramidModel(state, device=DEV)
    sc = camera_scene(["m2", "m2"], device=DEV)
    taps = {}
    got = eng(sc, taps)
    torch.cuda.synchronize()
    check_bev(eng, sc["inputs_m2"], taps, 2)
    x, xq = agent_chain(eng, state, taps, 2)
    info = {"m2": {"crop_ratio_W_m2": float(state["meta/crop_ratio_W"]), "crop_ratio_H_m2": float(state["meta/crop_ratio_H"])}}
    masks = [crop_mask_statement(["m2", "m2"], info, h, w) for h, w in ((16, 32), (8, 16), (4, 8))]
    assert (masks[2] == 0).all() and (masks[0] == 1).any()
    check_ego(masked_oracle(state, masks), state, sc, x, xq, masks, taps, got)


@pytest.fixture(scope="module")
def heter():
    from quantv2x_amd.engine_pyramid import deploy_heter_pyramid
    from quantv2x_amd.ptq_state import export_ptq_state
    qt = calibrated_camera_model(codebook=True)
    qt.model.ego_modality = "m1"
    return qt, {m: export_ptq_state(qt, modality=m) for m in ("m1", "m2")}, deploy_heter_pyramid(qt, device=DEV)


@pytest.mark.parametrize("agents", [["m1", "m2", "m2"], ["m2", "m1"]])
def test_heterogeneous_codebook_model(heter, agents):
    from quantv2x_amd.camera_bev import crop_mask_statement
    qt, states, eng = heter
    sc = camera_scene(agents, device=DEV)
    taps = {}
    got = eng(sc, taps)
    torch.cuda.synchronize()
    n_cam = sum(a == "m2" for a in agents)
    cam_eng, cam_taps = eng.engines["m2"], taps["modality/m2"]
    if n_cam == 1:                                                   # (one case: the statement chain of the image encoder is the slow part)
        cam_eng.cam_encoders = {k: v for k, v in cam_eng.cam_encoders.items() if k[0] == 1}
        check_bev(cam_eng, sc["inputs_m2"], cam_taps, 1)
    x, xq = agent_chain(cam_eng, states["m2"], cam_taps, n_cam)
    orc_cam = masked_oracle(states["m2"], None)
    want_codes = orc_cam.encode(x, xq).reshape(-1, n_cam, 16 * 32)
    slots = [i for i, a in enumerate(agents) if a == "m2"]
    wire = taps["codes"].cpu().numpy()
    np.testing.assert_array_equal(wire[:, slots], want_codes, err_msg="the camera agents' wire codes")
    # the ego side on the wire codes: decoded map, scores x mask, fusion, heads -- with the ego modality's state (shared layers are equal)
    main_state = states["m1"]
    info = {"m2": {"crop_ratio_W_m2": float(states["m2"]["meta/crop_ratio_W"]), "crop_ratio_H_m2": float(states["m2"]["meta/crop_ratio_H"])}}
    masks = [crop_mask_statement(agents, info, h, w) for h, w in ((16, 32), (8, 16), (4, 8))]
    orc = masked_oracle(main_state, masks)
    n = len(agents)
    feats = orc.decode(wire.reshape(-1, n * 16 * 32)).reshape(n, 16, 32, orc.D)
    np.testing.assert_array_equal(taps["features"].cpu().numpy().reshape(feats.shape), feats, err_msg="decoded map")
    otaps, plain = {}, {}
    pw, lens = sc["pairwise_t_matrix"].cpu().numpy(), [int(v) for v in sc["record_len"]]
    orc.pyramid(feats, pw, lens, otaps)
    masked_oracle(main_state, None).pyramid(feats, pw, lens, plain)
    for lvl in range(3):
        sco = plain[f"score{lvl}"]
        want = (sco * masks[lvl].reshape(sco.shape)).astype(np.float32)
        np.testing.assert_array_equal(taps[f"score{lvl}"].cpu().numpy().reshape(sco.shape), want, err_msg=f"score {lvl}")
        fu = otaps[f"fused{lvl}"]
        np.testing.assert_allclose(taps[f"fused{lvl}"].cpu().numpy().reshape(fu.shape), fu, **FUSE_TOL)
    cam_rows = [i for i, a in enumerate(agents) if a == "m2"]
    assert (taps["score2"].cpu().numpy()[cam_rows] == 0).all(), "level 2: the camera agents' scores are masked everywhere"
    check_after_fuse(orc, main_state, taps, got, otaps)


def test_lidar_only_scene_runs_without_masks(heter):
    """the same engine objects on a scene without a camera agent: no mask is built, so the ego runs the launches it ran before; and the mask
    is the ONLY thing ``score_masks`` adds -- masks of all ones (a multiply by 1.0) leave every tap and the predictions bit-equal"""
    from quantv2x_amd.engine import scene_layout
    _, _, eng = heter
    sc = camera_scene(["m1", "m1"], device=DEV)
    assert eng.main.crop_masks(["m1", "m1"]) is None
    taps = {}
    got = eng(sc, taps)["preds_tensor"].clone()
    pairwise, lens = scene_layout(sc, 2)
    hw = eng.main.fh * eng.main.fw
    ones = [torch.ones((2, h * w), dtype=torch.float32, device=DEV) for h, w in ((16, 32), (8, 16), (4, 8))]
    t2 = {}
    again = eng.main.decode_features(taps["codes"].contiguous(), hw, 2 * hw, lens, pairwise, 0, t2, score_masks=ones)["preds_tensor"]
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    for lvl in range(3):
        assert torch.equal(taps[f"score{lvl}"], t2[f"score{lvl}"]) and torch.equal(taps[f"fused{lvl}"], t2[f"fused{lvl}"])


def test_capture_and_replay_of_encode_features(heter):
    from quantv2x_amd.engine import capture_call
    _, _, eng = heter
    cam = eng.engines["m2"]
    inputs = camera_scene(["m1", "m2", "m2"], device=DEV)["inputs_m2"]
    other = camera_scene(["m1", "m2", "m2"], seed=9, device=DEV)["inputs_m2"]["imgs"]
    first = inputs["imgs"].clone()
    eager = cam.encode_features(inputs, 2).clone()
    replay = capture_call(lambda: cam.encode_features(inputs, 2))
    inputs["imgs"].copy_(other)
    moved = replay().clone()
    inputs["imgs"].copy_(first)
    again = replay().clone()
    torch.cuda.synchronize()
    assert not torch.equal(moved, eager) and torch.equal(again, eager)
