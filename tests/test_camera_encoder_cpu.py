"""The camera encoder without a GPU: the plugin mirror (``CamEncode_Resnet101``, ``QuantCamEncode_Resnet101``, ``LiftSplatShoot``,
``bin_depths``) and the host statements (``stem_statement``, the oracle's ``residual_block``, ``cam_heads_statement``) against
tests/golden/cam_encode.npz -- the reference's own quantized encoder, written by tests/golden/make_golden_cam.py, which runs
``check_mirror`` and ``check_statements`` below on what it is about to write -- plus the state round trip, the engine's refusals and the
C ABI of the two new entries.

The golden rule is the project's (tests/test_oracle_golden.py): teacher-forced on the reference's own layer inputs, at most 1 LSB off on
less than 5e-4 of the elements; the reference sums its fp32 convolutions in an unspecified order, the mirror in another, the statements
exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cam_encode.npz")
GRID = {"xbound": [-16, 16, 1], "ybound": [-16, 16, 1], "zbound": [-3, 3, 6], "ddiscr": [2, 24, 8], "mode": "LID"}
SHARE = 5e-4


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def lss_args(final_dim=(32, 48), features=64, encoder="Resnet101", use_depth_gt=False):
    return {"grid_conf": dict(GRID), "data_aug_conf": {"final_dim": final_dim}, "img_downsample": 8, "img_features": features,
            "camera_encoder": encoder, "use_depth_gt": use_depth_gt, "depth_supervision": False}


class Rule:
    """the golden rule over a run of comparisons: every difference at most 1 LSB, the share of differing elements below 5e-4"""

    def __init__(self):
        self.flips = self.total = 0

    def codes(self, name, got, want):
        diff = np.asarray(got).astype(np.int32) - np.asarray(want).astype(np.int32)
        assert diff.shape == np.asarray(want).shape and np.abs(diff).max() <= 1, f"{name}: more than 1 LSB off"
        self.flips += int((diff != 0).sum())
        self.total += diff.size

    def values(self, name, got, want, delta):
        """f32 values on a quantizer grid, in units of its delta"""
        self.codes(name, np.rint(np.asarray(got, np.float64) / float(delta)), np.rint(np.asarray(want, np.float64) / float(delta)))

    def share(self):
        share = self.flips / max(self.total, 1)
        assert share < SHARE, f"{self.flips} of {self.total} elements differ: {share:.2e} >= {SHARE}"
        return share


def mirror_model(g):
    """the plugin's QuantLiftSplatShoot with the fixture's weights (regenerated from its seed), BN folded, weight quantizers set, activation
    quantizers initialised layer by layer on the reference's own inputs (``calibrate_teacher_forced``)"""
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.models.heter_encoders import LiftSplatShoot
    from quantv2x_amd.plugin.quant import BaseQuantBlock, QuantModule, UniformAffineQuantizer, set_weight_quantize_params
    from quantv2x_amd.plugin.quant.fold_bn import search_fold_and_remove_bn
    from quantv2x_amd.plugin.quant.quant_block import QuantLiftSplatShoot
    lss = LiftSplatShoot(lss_args())
    enc = lss.camencode
    assert list(enc.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    assert [n for n, _ in enc.named_modules()] == [str(k) for k in g["float_module_names"]]
    synth.load_state_dict_numpy(enc, synth.make_state_dict(enc.state_dict(), int(g["seed"])))
    lss.eval()
    search_fold_and_remove_bn(lss)
    qt = QuantLiftSplatShoot(lss, dict(n_bits=8, channel_wise=True, scale_method="minmax"),
                             dict(n_bits=8, channel_wise=False, scale_method="minmax", leaf_param=True, prob=0.5)).eval()
    set_weight_quantize_params(qt)
    for m in qt.modules():                                           # as QuantModel.set_quant_state walks its tree
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.set_quant_state(True, True)
    calibrate_teacher_forced(g, qt.camencode)
    for m in qt.modules():
        if isinstance(m, UniformAffineQuantizer):
            m.set_inited(True)
    return qt


def calibrate_teacher_forced(g, enc):
    """Initialise every activation quantizer of the mirror from the reference's own input to its layer (min-max, as the reference's pass did),
    assert that it lands on the reference's (delta, zp), then pin the reference's values.  Teacher-forced, because a calibration pass down the
    mirror's own chain inherits every code its fp32 convolutions round the other way on another CPU: one flip upstream moves a min or a max
    downstream, and with it a whole layer's grid."""
    mods = dict(enc.named_modules())

    def init(owner, run, x, name):
        q = owner.act_quantizer
        q.set_inited(False)
        with torch.no_grad():
            run(x)
        q.set_inited(True)
        np.testing.assert_allclose(float(q.delta), g[name + "/a_delta"], rtol=1e-6, err_msg=name)
        assert float(q.zero_point) == float(g[name + "/a_zp"]), name
        q.delta, q.zero_point = torch.tensor(g[name + "/a_delta"]), torch.tensor(g[name + "/a_zp"])

    init(enc.conv1, enc.conv1, torch.from_numpy(g["images"]), "conv1")
    x = _deq(g, "maxpool", "conv1")
    for b in (str(k) for k in g["block_names"]):
        blk = mods[b]
        init(blk.conv1, blk.conv1, x, b + ".conv1")
        init(blk.conv2, blk.conv2, _deq(g, b + ".conv1"), b + ".conv2")
        init(blk, blk, x, b)
        x = _deq(g, b)
    init(enc.depth_head, enc.depth_head, x, "depth_head")
    init(enc.image_head, enc.image_head, x, "image_head")


def _checksum(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1).astype(np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * np.arange(1, a.size + 1)).sum()], np.float64)


def _deq(g, name, qname=None):
    """the reference's fake-quant tensor of a stored code map, f32 [V, C, H, W]"""
    qname = qname or name
    return torch.from_numpy((g[name + "/out_code"].astype(np.float32) - g[qname + "/a_zp"]) * g[qname + "/a_delta"])


def _code(t, delta, zp):
    return torch.round(t / float(delta)) + float(zp)


def check_mirror(g, qt=None):
    from quantv2x_amd.camera_encoder import maxpool_codes
    from quantv2x_amd.ptq_state import weight_codes
    qt = qt or mirror_model(g)
    enc = qt.camencode
    assert [n for n, _ in enc.named_modules()] == [str(k) for k in g["module_names"]]
    mods = dict(enc.named_modules())
    for n in (str(k) for k in g["quant_module_names"]):
        m = mods[n]
        np.testing.assert_array_equal(m.weight_quantizer.delta.detach().numpy().reshape(-1), g[n + "/w_delta"], err_msg=n)
        np.testing.assert_array_equal(m.weight_quantizer.zero_point.detach().numpy().reshape(-1), g[n + "/w_zp"], err_msg=n)
        assert bool(m.disable_act_quant) == bool(g[n + "/a_off"]) and weight_codes(m).dtype == np.uint8
        np.testing.assert_allclose(_checksum(m.weight.detach().numpy()), g[n + "/w_checksum"], rtol=1e-6, err_msg=n)      # the folded weights, from the seed
        if m.bias is not None:
            np.testing.assert_allclose(_checksum(m.bias.detach().numpy()), g[n + "/bias_checksum"], rtol=1e-6, atol=1e-9, err_msg=n)
        if not m.disable_act_quant:
            np.testing.assert_allclose(float(m.act_quantizer.delta), g[n + "/a_delta"], rtol=1e-6, err_msg=n)
            assert float(m.act_quantizer.zero_point) == float(g[n + "/a_zp"]), n
    rule = Rule()
    q = lambda n: (g[n + "/a_delta"], g[n + "/a_zp"])                # noqa: E731
    with torch.no_grad():
        rule.codes("conv1", _code(enc.conv1(torch.from_numpy(g["images"])), *q("conv1")), g["conv1/out_code"])
        pooled = enc.maxpool(_deq(g, "conv1"))
        np.testing.assert_array_equal(_code(pooled, *q("conv1")).numpy(), g["maxpool/out_code"])       # a max of grid values: exact
        np.testing.assert_array_equal(maxpool_codes(g["conv1/out_code"].transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2), g["maxpool/out_code"])
        x = _deq(g, "maxpool", "conv1")
        for b in (str(k) for k in g["block_names"]):
            np.testing.assert_allclose(float(mods[b].act_quantizer.delta), g[b + "/a_delta"], rtol=1e-6, err_msg=b)
            assert float(mods[b].act_quantizer.zero_point) == float(g[b + "/a_zp"]), b
            rule.codes(b + ".conv1", _code(mods[b].conv1(x), *q(b + ".conv1")), g[b + ".conv1/out_code"])
            rule.codes(b + ".conv2", _code(mods[b].conv2(_deq(g, b + ".conv1")), *q(b + ".conv2")), g[b + ".conv2/out_code"])
            rule.codes(b, _code(mods[b](x), *q(b)), g[b + "/out_code"])
            x = _deq(g, b)                                           # teacher forcing
        rule.values("depth_head", enc.depth_head(x), g["depth_logits"], g["depth_head/a_delta"])
        rule.values("image_head", enc.image_head(x), g["features"], g["image_head/a_delta"])
    return rule.share()


def check_statements(g, qt=None):
    from _camera import TRUNK, oracle
    from quantv2x_amd import camera_encoder as ce
    from quantv2x_amd.ptq_state import export_camera_state
    state = export_camera_state(qt or mirror_model(g))
    nhwc = lambda n: np.ascontiguousarray(g[n + "/out_code"].transpose(0, 2, 3, 1))          # noqa: E731
    rule = Rule()
    wdeq, bias, q = ce.stem_constants(state)
    pooled, conv = ce.stem_statement(g["images"], wdeq, bias, *q, want_conv=True)
    rule.codes("conv1", conv, nhwc("conv1"))
    rule.codes("maxpool", pooled, nhwc("maxpool"))
    orc = oracle(state)
    x, xq = nhwc("maxpool"), (np.float32(q[0]), int(q[1]))
    for layer, count, _, stride in TRUNK:
        for i in range(count):
            b, taps = f"{layer}.{i}", {}
            _, oq = orc.residual_block(b, x, xq, stride if i == 0 else 1, ["conv1", "conv2", "conv3"], taps)
            for n in (b + ".conv1", b + ".conv2", b):
                rule.codes(n, taps[n], nhwc(n))
            x, xq = nhwc(b), oq
    depth, feats = ce.cam_heads_statement(x, xq, state)
    rule.values("depth_head", depth, g["depth_logits"], g["depth_head/a_delta"])
    rule.values("image_head", feats, g["features"], g["image_head/a_delta"])
    return rule.share()


@pytest.fixture(scope="module")
def mirror(golden):
    return mirror_model(golden)


def test_mirror_against_the_reference(golden, mirror):
    print("mirror: share of elements 1 LSB off", check_mirror(golden, mirror))


def test_statements_against_the_reference(golden, mirror):
    print("statements: share of elements 1 LSB off", check_statements(golden, mirror))


def test_trunk_keeps_its_width_after_a_pyramid_model_was_built(monkeypatch):
    """PyramidFusion sets ``Bottleneck.expansion = 1`` on the shared class; the camera trunk is torchvision's (expansion 4) whatever ran before"""
    from quantv2x_amd.plugin.models.sub_modules import resblock
    from quantv2x_amd.plugin.models.sub_modules.lss_submodule import CamEncode_Resnet101
    monkeypatch.setattr(resblock.Bottleneck, "expansion", 1)
    enc = CamEncode_Resnet101(8, 64, 8, [2, 24, 8], "LID", False, False).eval()
    assert enc.layer1[0].conv3.out_channels == 256 and enc.layer2[3].conv3.out_channels == 512
    with torch.no_grad():
        assert enc.get_resnet_features(torch.zeros(1, 3, 32, 48)).shape == (1, 512, 4, 6)


def test_bin_depths_equals_the_reference(golden):
    from quantv2x_amd.plugin.utils.camera_utils import bin_depths
    lo, hi, bins = (float(v) for v in golden["bin/ddiscr"])
    for mode in ("UD", "LID", "SID"):
        for target in (True, False):
            with np.errstate(all="ignore"):
                idx, mask = bin_depths(torch.from_numpy(golden["bin/depths"].copy()), mode, int(lo), int(hi), int(bins), target=target)
            assert idx.dtype == torch.int64
            np.testing.assert_array_equal(idx.numpy(), golden[f"bin/{mode}/{int(target)}/indices"], err_msg=f"{mode} target={target}")
            if target:
                assert mask is None
            else:
                np.testing.assert_array_equal(mask.numpy(), golden[f"bin/{mode}/0/mask"], err_msg=mode)
    with pytest.raises(NotImplementedError):
        bin_depths(torch.zeros(3), "XYZ", 2, 24, 8)


def test_mirror_forward_on_the_cpu_pools_without_the_product(golden, mirror):
    """QuantLiftSplatShoot.forward on the CPU: the BEV of the statements' torch form equals splat_statement on the same factors"""
    from _lift_splat import MATRICES, rig
    from quantv2x_amd import lift_splat as ls
    m = rig(1, 2, (32, 48), seed=4)
    imgs = torch.from_numpy(golden["images"])[None]
    with torch.no_grad():
        bev = mirror({"inputs_m4": dict({k: torch.from_numpy(v) for k, v in m.items()}, imgs=imgs)}, "m4").numpy()
        _, depth, mode, feats = mirror.get_cam_feats(imgs)
    cells = ls.cells_statement(ls.geometry_statement(mirror.frustum, *(m[k] for k in MATRICES)), mirror.dx, mirror.bx, mirror.nx)
    want = ls.splat_statement(cells, depth.numpy(), feats.numpy(), mode, nx=mirror.nx)
    assert mode == "logits" and bev.shape == want.shape == (1, 64, 32, 32) and (want != 0).any()
    np.testing.assert_allclose(bev, want, rtol=1e-4, atol=1e-5)


def test_camera_state_round_trip(golden, mirror, tmp_path):
    from quantv2x_amd.ptq_state import export_camera_state, load_ptq_state, save_ptq_state
    state = export_camera_state(mirror)
    assert [str(n) for n in state["meta/block_names"]] == [str(n) for n in golden["block_names"]]
    assert [str(n) for n in state["meta/module_names"]] == [str(n) for n in golden["quant_module_names"]]
    assert state["conv1/w_code"].shape == (64, 3, 7, 7) and state["depth_head/w_code"].shape == (8, 512, 1, 1)
    path = str(tmp_path / "cam.npz")
    save_ptq_state(path, state)
    back = load_ptq_state(path)
    assert sorted(back) == sorted(state)
    for k, v in state.items():
        assert np.array_equal(np.asarray(v), back[k]) and np.asarray(v).dtype == back[k].dtype, k


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def _engine(state):
    """the engine's constructor with the GPU taken out: the state checks run before anything touches the device"""
    from quantv2x_amd import engine_camera as ec
    return ec.DeployedCameraEncoder(state, views=2, samples=1, device="cpu")


@pytest.fixture()
def no_gpu_needed(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)


def test_engine_refusals(no_gpu_needed):
    from _camera import camera_state
    good = camera_state(3)
    with pytest.raises(NotImplementedError, match="Resnet101"):
        _engine(dict(good, **{"meta/camera_encoder": np.array("EfficientNet")}))
    with pytest.raises(NotImplementedError, match="use_gt_depth"):
        _engine(dict(good, **{"meta/use_gt_depth": np.bool_(True)}))
    for name in ("conv1", "layer1.1.conv2", "layer2.0", "image_head"):
        with pytest.raises(ValueError, match="disabled"):
            _engine(dict(good, **{name + "/a_off": np.bool_(True)}))
    with pytest.raises(ValueError, match="downsample"):                # 40 -> 20 -> 10 -> 5 rows, but 40 // 8 = 5 and 52 -> 26 -> 13 -> 7 != 52 // 8
        _engine(dict(good, **{"meta/final_dim": np.array([40, 52])}))


def test_export_refusals(golden):
    from quantv2x_amd.plugin.models.heter_encoders import LiftSplatShoot
    from quantv2x_amd.plugin.quant.quant_block import QuantLiftSplatShoot
    from quantv2x_amd.ptq_state import export_camera_state
    with pytest.raises(NotImplementedError, match="EfficientNet"):
        LiftSplatShoot(lss_args(encoder="EfficientNet"))
    wq, aq = dict(n_bits=8, channel_wise=True, scale_method="minmax"), dict(n_bits=8, channel_wise=False, scale_method="minmax", leaf_param=True, prob=0.5)
    unfolded = QuantLiftSplatShoot(LiftSplatShoot(lss_args()).eval(), wq, aq)
    for m in unfolded.modules():
        if hasattr(m, "set_inited"):
            m.set_inited(True)
    with pytest.raises(ValueError, match="not folded"):
        export_camera_state(unfolded)
    voxel = type("LiftSplatShootVoxel", (), {})()
    with pytest.raises(NotImplementedError, match="Voxel"):
        export_camera_state(voxel)
    other = type("QuantLiftSplatShoot", (), {"camera_encoder_type": "EfficientNet"})()
    with pytest.raises(NotImplementedError, match="EfficientNet"):
        export_camera_state(other)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------

def test_cabi_of_the_camera_entries():
    from quantv2x_amd import build, lib
    header = open(os.path.join(ROOT, "include", "qv2x.h")).read()
    for name in ("qv2x_cam_stem_f32", "qv2x_cam_heads_i8"):
        assert re.search(r"\bint " + name + r"\(", header) and name in lib.SYMBOLS
    assert C.sizeof(lib.CamStemDesc) == 4 * 4 + 8 + 2 * 4 and C.sizeof(lib.CamHeadsDesc) == 6 * 4 + 4 * 4
    for struct, cname in ((lib.CamStemDesc, "qv2x_cam_stem_desc"), (lib.CamHeadsDesc, "qv2x_cam_heads_desc")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in struct._fields_], cname
    build.build()
    l = lib.load()
    buf = np.zeros(256, np.float32)
    p = lib.ptr(buf)
    d = lib.CamStemDesc()
    d.views, d.h, d.w, d.view_stride, d.out_delta, d.out_zp = 1, 8, 8, 3 * 64, 0.1, 0.0
    assert l.qv2x_cam_stem_f32(C.byref(d), None, p, p, p, None) == -1 and b"null" in l.qv2x_last_error()
    d.view_stride = 3 * 64 - 1
    assert l.qv2x_cam_stem_f32(C.byref(d), p, p, p, p, None) == -1 and b"view_stride" in l.qv2x_last_error()
    d.view_stride, d.h = 3 * 64, 0
    assert l.qv2x_cam_stem_f32(C.byref(d), p, p, p, p, None) == -1 and b"positive" in l.qv2x_last_error()
    d.h, d.out_delta = 8, 0.0
    assert l.qv2x_cam_stem_f32(C.byref(d), p, p, p, p, None) == -1 and b"out_delta" in l.qv2x_last_error()
    d.out_delta = 0.1
    assert l.qv2x_cam_stem_f32(C.byref(d), p, C.c_void_p(buf.ctypes.data + 4), p, p, None) == -2 and b"aligned" in l.qv2x_last_error()
    e = lib.CamHeadsDesc()
    e.views, e.h, e.w, e.cin, e.depth_bins, e.features = 1, 2, 2, 32, 8, 4
    e.depth_delta, e.depth_zp, e.feat_delta, e.feat_zp = 0.1, 0.0, 0.1, 255.0
    args = lambda: (C.byref(e), p, p, p, p, p, p, p, p, None)        # noqa: E731
    assert l.qv2x_cam_heads_i8(C.byref(e), p, p, p, p, p, p, None, p, None) == -1 and b"null" in l.qv2x_last_error()
    for field, bad, code, word in (("w", 0, -1, b"positive"), ("cin", 48, -2, b"cin"), ("depth_bins", 257, -1, b"depth_bins"), ("depth_bins", 0, -1, b"depth_bins"),
                                   ("features", 6, -2, b"features"), ("features", 0, -1, b"features"), ("feat_zp", 256.0, -1, b"zero point"),
                                   ("depth_delta", -1.0, -1, b"positive")):
        keep = getattr(e, field)
        setattr(e, field, bad)
        assert l.qv2x_cam_heads_i8(*args()) == code and word in l.qv2x_last_error(), (field, l.qv2x_last_error())
        setattr(e, field, keep)
    assert l.qv2x_cam_heads_i8(C.byref(e), C.c_void_p(buf.ctypes.data + 4), p, p, p, p, p, p, p, None) == -2 and b"aligned" in l.qv2x_last_error()
