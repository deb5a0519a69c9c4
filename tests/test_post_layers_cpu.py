"""The references of tests/test_hip_post_layers.py (tests/_post_layers.py) pinned against the CPU oracle, and the conditions its GPU
comparisons rest on checked for every case of that file:

  * ``ref_heads64`` + ``ref_quant`` against ``orc_heads`` on the golden tiny state under ``_common.compare_frame``'s rule for predictions,
    ``ref_decode`` against ``Oracle.decode`` and ``ref_fuse`` against ``Oracle.fuse`` bit for bit;
  * ``dyadic`` operands are order-free: every row's 256 products summed in three random orders in fp32 give the float64 sum;
  * the doubtful set of every ``real`` head / table case (float64 ``y / d`` within ``E / d`` of a rounding boundary) holds at most 1 % of the
    quantized outputs;
  * ``ref_fuse`` (fp32) stays within half of ``FUSE_TOL`` of ``ref_fuse64`` on every fuse case, so the GPU keeps the other half.  The fuse
    operands are N(0, 1/16) per channel, not unit scale: at N(0, 1) the ego's score on itself (|f|^2 / 16 ~ 16) would make the softmax the
    identity and a kernel that mis-weighted the other agents would pass (``_post_layers.FUSE_SCALE``)."""
import numpy as np
import pytest

import _post_layers as P
from _common import FUSE_TOL, calibrated_plugin, ego_view, head_lsb, scene_np


def _oracle(**fields):
    from oracle.spec import Oracle
    orc = Oracle.__new__(Oracle)
    for k, v in fields.items():
        setattr(orc, k, v)
    return orc


def test_heads_reference_against_the_oracle_on_the_golden_tiny_state():
    from oracle.spec import Oracle
    from quantv2x_amd.ptq_state import export_ptq_state
    state = export_ptq_state(calibrated_plugin())
    orc = Oracle(state)
    taps = {}
    want = orc.forward(scene_np(2), taps)
    fused = taps["fused"]
    rows = fused.reshape(-1, 256)
    lsb = head_lsb(state)
    got = []
    for head in ("cls_head", "reg_head", "dir_head"):
        p = orc.q(head)
        w = orc.dequant_weight(p).reshape(p["code"].shape[0], -1)
        y = P.ref_heads64(rows, w, p["bias"]).astype(np.float32)
        cout = w.shape[0]
        o = y if p["a_off"] else P.ref_quant(y, np.full(cout, p["da"], np.float32), np.full(cout, p["za"], np.float32))
        got.append(o.reshape(fused.shape[0], fused.shape[1], fused.shape[2], cout).transpose(0, 3, 1, 2))
    d = np.abs(np.concatenate(got, axis=1) - want["preds_tensor"])
    assert d.max() <= lsb * 1.001 and (d > 1e-5).mean() < 1e-3, (d.max(), (d > 1e-5).mean())


@pytest.mark.parametrize("planes,kc,R", [(3, 128, 77), (6, 256, 40), (1, 1, 5), (16, 32, 33)])
def test_decode_reference_equals_the_oracle(planes, kc, R):
    rng = np.random.default_rng(planes * 1000 + kc)
    for mode in ("real", "dyadic"):
        lut, bias = P.make_lut(rng, planes, kc, mode)
        codes = P.make_codes(rng, planes, R, kc)
        np.testing.assert_array_equal(P.ref_decode(codes, lut, bias), _oracle(lut=lut, lut_bias=bias).decode(codes))


@pytest.mark.parametrize("name", ["transforms_att", "transforms_max_negative", "ego2_of6_7x33", "ragged_batch_ego1", "feats_att"])
def test_fuse_reference_equals_the_oracle(name):
    c = P.fuse_case(name)
    orc = _oracle(s={"meta/HW_metres": np.array([P.HM, P.WM]), "meta/discrete_ratio": P.RATIO, "meta/fusion_method": "max" if c["fusion"] else "att"})
    for s, n in enumerate(c["scenes"]):
        feats, pw = ego_view(c["dec"][s], c["pairwise"][s], n, c["ego"])
        want = orc.fuse(feats, pw, [n])[0]
        np.testing.assert_array_equal(c["ref"][s], want.reshape(c["hw"], 256))


# ---- the conditions of the GPU file, case by case -----------------------------------------------------------------------------------------
def _order_free(rows, w, bias, seed):
    """EVERY row: each output's 257 terms (exact products and the bias) summed in three random orders in fp32, one running sum each,
    equal the float64 sum"""
    rng = np.random.default_rng(seed)
    w64, b64 = w.astype(np.float64), bias.astype(np.float64)
    for r0 in range(0, rows.shape[0], 64):
        x = rows[r0:r0 + 64]
        t64 = np.concatenate([x.astype(np.float64)[:, None, :] * w64[None], np.broadcast_to(b64[None, :, None], (x.shape[0], w.shape[0], 1))], axis=2)
        terms = t64.astype(np.float32)                                   # [rows][cout][257]
        assert np.array_equal(terms.astype(np.float64), t64)
        y64 = P.ref_heads64(x, w, bias)
        for _ in range(3):
            s = np.cumsum(terms[:, :, rng.permutation(257)], axis=2, dtype=np.float32)[:, :, -1]
            np.testing.assert_array_equal(s.astype(np.float64), y64)


def _dyadic_steps(*heads):
    for hd in heads:
        on = hd["da"] > 0
        assert np.all(np.log2(hd["da"][on]) == np.rint(np.log2(hd["da"][on])))


def _decode_order_free(c):
    np.testing.assert_array_equal(P.ref_decode(c["codes"], c["lut"], c["lut_bias"]).astype(np.float64),
                                  P.table_sum64(c["codes"], c["lut"].astype(np.float64), c["lut_bias"].astype(np.float64)))


@pytest.mark.parametrize("name", list(P.PAIR_CASES))
def test_dyadic_pair_cases_are_order_free(name):
    c = P.pair_case(name)
    _order_free(c["rows"], c["h0"]["w"], c["h0"]["bias"], 2)
    _order_free(c["drows"], c["h1"]["w"], c["h1"]["bias"], 3)
    _dyadic_steps(c["h0"], c["h1"])
    _decode_order_free(c)


@pytest.mark.parametrize("every_quantized", [False, True])
@pytest.mark.parametrize("name", list(P.IDENTITY_CASES))
def test_dyadic_identity_cases_are_order_free_and_the_warp_is_the_identity(name, every_quantized):
    c = P.identity_case(name, every_quantized)
    _order_free(c["drows"], c["heads"]["w"], c["heads"]["bias"], 4)
    _dyadic_steps(c["heads"])
    _decode_order_free(c)
    hw = c["hw"]
    for s in range(c["scenes"]):
        dec = c["drows"][s * hw:(s + 1) * hw]
        np.testing.assert_array_equal(P.ref_fuse(dec.reshape(1, c["h"], c["w"], 256), c["pairwise"][s], 1, 0, P.HM, P.WM, P.RATIO, 0).reshape(hw, 256), dec)


@pytest.mark.parametrize("R,planes,kc", P.DECODE_CASES)
def test_dyadic_decode_cases_are_order_free(R, planes, kc):
    _decode_order_free(P.decode_case(R, planes, kc, "dyadic"))


@pytest.mark.parametrize("name", [k for k, v in P.HEAD_CASES.items() if v[2] == "dyadic"])
def test_dyadic_head_cases_are_order_free(name):
    c = P.head_case(name)
    for rows in (c["rows"], c["drows"]):
        _order_free(rows, c["heads"]["w"], c["heads"]["bias"], 1)
    _dyadic_steps(c["heads"], c["heads_q"])
    _decode_order_free(c)               # the decoded rows themselves: bias + planes terms, any order


def test_quantizer_case_holds_clamps_and_ties():
    """the dyadic head cases reach both clamps, |y / d| >= 1100 and exact half-integer ties next to clean values"""
    c = P.head_case("dyadic_c72")
    hd = c["heads_q"]
    t = c["y64"] / hd["da"].astype(np.float64)
    code, dist = P.code64(c["y64"], hd["da"], hd["za"])
    assert (t >= 1100).any() and (t <= -1100).any() and (code == 0).any() and (code == 255).any()
    assert (dist == 0).any() and ((dist > 0.4) & (dist < 0.5)).any() or (dist == 0).any() and (dist == 0.5).any()
    assert ((code > 0) & (code < 255)).mean() > 0.1
    assert set(np.unique(hd["za"])) >= {0.0, 37.0, 255.0}


@pytest.mark.parametrize("name", P.REAL_HEAD_CASES)
def test_real_head_cases_keep_the_doubtful_set_small(name):
    c = P.head_case(name)
    for hd in (c["heads"], c["heads_q"]):
        for y64, E in ((c["y64"], c["E"]), (c["y64d"], c["Ed"])):
            on = hd["da"] > 0
            share = P.doubtful(y64, E, hd["da"])[:, on].mean()
            assert share <= 0.01, f"{name}: {share:.4f} of the quantized outputs are doubtful: another seed or step"
            code, _ = P.code64(y64, hd["da"], hd["za"])
            assert ((code[:, on] > 0) & (code[:, on] < 255)).mean() > 1 / 3


@pytest.mark.parametrize("name", list(P.LUT_CASES) + list(P.TABLE_CASES))
def test_table_cases(name):
    d = P.table_case(name, "dyadic")
    y64 = P.table_sum64(d["codes"], d["t64"], d["b64"])
    rng = np.random.default_rng(3)
    pick = rng.choice(d["R"], size=min(d["R"], 64), replace=False)
    terms = np.stack([np.broadcast_to(d["bias"], (d["R"], d["ct"]))] + [d["tables"][p][d["codes"][p].astype(np.int64)] for p in range(d["planes"])])
    for _ in range(3):
        perm = rng.permutation(d["planes"] + 1)
        s = np.cumsum(terms[perm][:, pick], axis=0, dtype=np.float32)[-1]
        np.testing.assert_array_equal(s.astype(np.float64), y64[pick])
    if name == "groups2":
        return
    r = P.table_case(name, "real")
    y64 = P.table_sum64(r["codes"], r["t64"], r["b64"])
    on = r["da"] > 0
    if on.any():
        share = P.doubtful(y64, P.table_error_bound(r["codes"], r["t64"], r["b64"]), r["da"])[:, on].mean()
        assert share <= 0.01, f"{name}: {share:.4f} doubtful"


@pytest.mark.parametrize("name", list(P.FUSE_CASES))
def test_fuse_reference_within_half_the_tolerance_of_float64(name):
    c = P.fuse_case(name)
    half = dict(rtol=FUSE_TOL["rtol"] / 2, atol=FUSE_TOL["atol"] / 2)
    for s in range(len(c["scenes"])):
        assert np.isfinite(c["ref"][s]).all()
        np.testing.assert_allclose(c["ref"][s], c["ref64"][s], **half)
    if not c["feats"]:
        codes = c["codes_buf"]
        assert c["level_stride"] > c["hw"] and c["agent_stride"] > c["planes"] * c["level_stride"] and (codes == P.POISON_CODE).any()


def test_fuse_cases_hold_what_their_names_say():
    from oracle import geometry
    # saturated softmax: the ego's score on agent 1 is at least 100 above every other one, the result is agent 1's warped feature
    c = P.fuse_case("saturated_softmax")
    warped = P._warp(c["dec"][0], c["pairwise"][0], 3, 0, P.HM, P.WM, P.RATIO)
    score = np.einsum("hwc,nhwc->hwn", warped[0].astype(np.float64), warped.astype(np.float64)) / 16.0
    assert (score[..., 1] - np.maximum(score[..., 0], score[..., 2])).min() >= 100
    np.testing.assert_allclose(c["ref"][0], warped[1].reshape(-1, 256), **FUSE_TOL)
    # the out-of-view agent: a map of zeros that wins MaxFusion on all-negative features ...
    c = P.fuse_case("transforms_max_negative")
    assert (c["dec"][0] < 0).all() and (c["ref"][0] == 0).all()
    # ... and takes part in the softmax with score 0
    c = P.fuse_case("transforms_att")
    warped = P._warp(c["dec"][0], c["pairwise"][0], 8, 0, P.HM, P.WM, P.RATIO)
    assert (warped[6] == 0).all() and (warped[7] == 0).all() and (warped[1:6] != 0).any(axis=(1, 2, 3)).all()
    without = geometry.att_fuse(warped[:6])
    assert np.abs(without.reshape(-1, 256) - c["ref"][0]).max() > 1e-3
    # code planes: 0 and kc - 1 in every plane, bytes >= 128 at kc = 256
    for name in ("planes4_kc256", "planes16_kc256", "planes3_kc256"):
        c = P.fuse_case(name)
        wire = c["codes_buf"]
        for l in range(c["planes"]):
            vals = np.concatenate([wire[a * c["agent_stride"] + l * c["level_stride"]:][:c["hw"]] for a in range(3)])
            assert vals.min() == 0 and vals.max() == 255 and (vals >= 128).any()
