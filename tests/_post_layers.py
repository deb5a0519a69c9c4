"""Operands, references and the case lists of the post stage's direct tests (a7-a11: decode, warp, attention / max fusion, heads; no tests
here, numpy only).  tests/test_post_layers_cpu.py pins the references and checks the conditions the GPU comparisons rest on;
tests/test_hip_post_layers.py runs the C entries on the same cases.

Two value modes:

  dyadic  rows, tables, weights and biases are integers in [-8, 8] times a fixed power of two, every output step ``da`` is a power of two.
          A decoded row is a sum of at most 17 such integers (|.| <= 136), a product with a weight at most 1088, so every partial sum of a
          256-term dot product is an integer below 2^19 < 2^24 times a fixed power of two: the fp32 result is the same under ANY order of
          addition and equals the float64 one, and ``y / da`` is exact, half-integer ties included.  Comparisons are bit for bit.
  real    N(0, 1) rows, N(0, 1/16) weights, steps that are no powers of two.  The error of the kernel's fp32 dot product is bounded by
          ``heads_error_bound`` (any order of addition), an output whose float64 ``y / da`` lies within that bound of a rounding boundary is
          ``doubtful`` and may differ by one code.

Fuse cases are NOT unit scale: a decoded feature is N(0, 1/16) per channel (FUSE_SCALE below says why).  The smaller values only make the
fp32 reference's distance to its float64 form smaller; it is checked against half of FUSE_TOL as it stands.
"""
import functools

import numpy as np

U = 2.0 ** -24
NAN_ROWS = 256                  # rows of NaN behind a device table: a code byte read from a poisoned gap (0xEE) lands there, not outside
POISON_CODE = 0xEE


def ceil32(c):
    return (c + 31) // 32 * 32


# ---- operand builders --------------------------------------------------------------------------------------------------------------------
def dyadic_ints(rng, shape, exp=0):
    return (rng.integers(-8, 9, size=shape).astype(np.float64) * 2.0 ** exp).astype(np.float32)


def make_lut(rng, planes, kc, mode, width=256):
    """decode tables ``lut [planes][kc][width]`` and ``lut_bias [width]``; ``real``: a decoded row is N(0, 1)"""
    if mode == "dyadic":
        return dyadic_ints(rng, (planes, kc, width), -1), dyadic_ints(rng, width, -1)
    s = 1.0 / np.sqrt(planes + 1.0)
    return (rng.normal(0, s, (planes, kc, width)).astype(np.float32), rng.normal(0, s, width).astype(np.float32))


def make_rows(rng, R, mode):
    return dyadic_ints(rng, (R, 256), -1) if mode == "dyadic" else rng.normal(0, 1, (R, 256)).astype(np.float32)


def make_codes(rng, planes, R, kc):
    """code planes u8 [planes][R]; 0 and kc - 1 occur in every plane that has room for both (for kc = 256: bytes >= 128)"""
    c = rng.integers(0, kc, size=(planes, R)).astype(np.uint8)
    if R >= 2:
        for p in range(planes):
            i, j = rng.choice(R, size=2, replace=False)
            c[p, i], c[p, j] = 0, kc - 1
    return c


def make_heads(rng, cout, cout_pad, mode, za_set=(0, 37, 255), every_quantized=False):
    """``w [cout][256]``, ``bias``, ``da``, ``za`` per channel (every third channel without a quantizer unless ``every_quantized``) and the
    device operands: the weights packed by the engine's own ``_pack_k4p`` and padded to ``cout_pad`` as ``_Heads`` pads, padding da = -1."""
    from quantv2x_amd.engine import _pack_k4p
    if mode == "dyadic":
        w, b = dyadic_ints(rng, (cout, 256)), dyadic_ints(rng, cout, -1)
        da = (2.0 ** rng.integers(-2, 7, size=cout)).astype(np.float32)
    else:
        w, b = rng.normal(0, 0.25, (cout, 256)).astype(np.float32), rng.normal(0, 1, cout).astype(np.float32)
        da = rng.uniform(0.2, 0.4, size=cout).astype(np.float32)
    za = np.asarray(za_set, np.float32)[(np.arange(cout) // 2) % len(za_set)]
    if not every_quantized:
        da[2::3] = -1.0
        za[2::3] = 0.0
    pad = cout_pad - cout
    return dict(cout=cout, cout_pad=cout_pad, w=w, bias=b, da=da, za=za,
                w_packed=_pack_k4p(np.concatenate([w, np.zeros((pad, 256), np.float32)])),
                bias_pad=np.concatenate([b, np.zeros(pad, np.float32)]), da_pad=np.concatenate([da, np.full(pad, -1.0, np.float32)]),
                za_pad=np.concatenate([za, np.zeros(pad, np.float32)]))


def collapse_tables(lut, lut_bias, w, bias):
    """head(decode(codes)) = b' + sum_l T'_l[code_l]  (``_Heads.collapse_over_decode``): float64 ``(T' [planes][kc][cout], b' [cout])``"""
    t = np.einsum("lkd,cd->lkc", lut.astype(np.float64), w.astype(np.float64))
    return t, lut_bias.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)


def make_pairwise(poses_per_scene, max_cav):
    """pairwise blocks f64 [scenes][L][L][4][4] from the agents' world poses (x, y, yaw)"""
    from oracle.geometry import pairwise_from_poses
    from quantv2x_amd.synth import pose_matrix
    return np.stack([pairwise_from_poses([pose_matrix(*p) for p in poses], max_cav) for poses in poses_per_scene])


# ---- references --------------------------------------------------------------------------------------------------------------------------
def ref_decode(codes, lut, lut_bias):
    """codes u8 [planes][R] -> f32 [R][width], fp32 adds in plane order: ((bias + T0[c0]) + T1[c1]) + ... (the order the kernels state)"""
    v = np.broadcast_to(lut_bias.astype(np.float32), (codes.shape[1], lut.shape[2])).copy()
    for p in range(codes.shape[0]):
        v = (v + lut[p][codes[p].astype(np.int64)]).astype(np.float32)
    return v


def ref_heads64(rows, w, bias):
    return rows.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)


def ref_quant(y, da, za, codes=False):
    """``clamp(rint(y / d) + z, 0, 255)`` on fp32 y with an fp32 division (common.h:q_code's promise), per channel (last axis); the code, or
    the dequantized value ``(code - z) * d``; channels with ``da <= 0`` pass through (code: -1)."""
    y = np.asarray(y, np.float32)
    on = da > 0
    d = np.where(on, da, np.float32(1)).astype(np.float32)
    code = np.clip(np.rint(y / d) + za.astype(np.float32), np.float32(0), np.float32(255)).astype(np.float32)
    if codes:
        return np.where(on, code, np.float32(-1))
    return np.where(on, ((code - za.astype(np.float32)) * d).astype(np.float32), y)


def ref_dequant(code_u8, zp, delta):
    """``(code + 128 - zp) * delta`` in fp32 on the i8 tensor's values ``code`` = u8 code - 128"""
    return ((code_u8.astype(np.int32) + (128 - int(zp))).astype(np.float32) * np.float32(delta)).astype(np.float32)


def _warp(feats, pairwise_b, n, ego, hm, wm, ratio):
    from _common import ego_view
    from oracle import geometry
    fv, pw = ego_view(np.ascontiguousarray(feats, dtype=np.float32), pairwise_b, n, ego)
    affine = geometry.normalize_pairwise_tfm(pw, hm, wm, ratio)[0]
    return geometry.warp_to_ego(fv, affine, n)


def ref_fuse(feats, pairwise_b, n, ego, hm, wm, ratio, fusion):
    """feats f32 [n][h][w][256], pairwise_b f64 [L][L][4][4] -> [h][w][256]: the oracle's own path (``Oracle.fuse``) seen from agent ``ego``"""
    from oracle import geometry
    warped = _warp(feats, pairwise_b, n, ego, hm, wm, ratio)
    return geometry.max_fuse(warped) if fusion == 1 else geometry.att_fuse(warped)


def ref_fuse64(feats, pairwise_b, n, ego, hm, wm, ratio, fusion):
    """the same warp (fp32 grid and bilinear sums), the softmax and the weighted sum in float64"""
    warped = _warp(feats, pairwise_b, n, ego, hm, wm, ratio).astype(np.float64)
    if fusion == 1:
        return warped.max(axis=0)
    score = np.einsum("hwc,nhwc->hwn", warped[0], warped) / 16.0
    p = np.exp(score - score.max(axis=-1, keepdims=True))
    return np.einsum("hwn,nhwc->hwc", p / p.sum(axis=-1, keepdims=True), warped)


def ref_assemble(slabs_u8, frames, cout, h, w, world, wire, da=None, za=None):
    """numpy slabs u8 [world][slab_bytes] (any slack past the layout's size is cut off first) -> f32 [frames][cout][h][w]"""
    import torch
    from quantv2x_amd.dist import assemble_bands_reference, band_payload_layout
    _, nbytes = band_payload_layout(frames, cout, h, w, world, wire)
    t = torch.from_numpy(np.ascontiguousarray(slabs_u8[:, :nbytes]))
    return assemble_bands_reference(t, frames, cout, h, w, world, wire, None if da is None else torch.from_numpy(da),
                                    None if za is None else torch.from_numpy(za)).numpy()


# ---- error bounds of the ``real`` cases -----------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


def heads_error_bound(rows, w, bias):
    """E = g (|b| + sum_k |x_k| |w_k|), g = 257 u / (1 - 257 u): the forward error of a 256-term fp32 dot product plus bias in any order"""
    return gamma(257) * (np.abs(bias.astype(np.float64)) + np.abs(rows.astype(np.float64)) @ np.abs(w.astype(np.float64)).T)


def table_error_bound(codes, t64, b64):
    """E of the table forms: the fp32 sum of ``planes + 1`` fp32 terms that are float64 values rounded once"""
    planes = codes.shape[0]
    terms = np.stack([np.broadcast_to(np.abs(b64), (codes.shape[1], b64.size))] + [np.abs(t64[p][codes[p].astype(np.int64)]) for p in range(planes)])
    return gamma(planes + 1) * terms.sum(axis=0) + U * (planes + 1) * terms.max(axis=0)


def table_sum64(codes, t64, b64):
    y = np.broadcast_to(b64, (codes.shape[1], b64.size)).copy()
    for p in range(codes.shape[0]):
        y += t64[p][codes[p].astype(np.int64)]
    return y


def code64(y64, da, za):
    """the float64 code and the distance of ``y / d`` to the nearest rounding boundary, per channel (only where da > 0)"""
    d = np.where(da > 0, da, np.float32(1)).astype(np.float64)
    t = y64 / d
    return np.clip(np.rint(t) + za.astype(np.float64), 0, 255), np.abs(t - np.floor(t) - 0.5)


def doubtful(y64, E, da):
    d = np.where(da > 0, da, np.float32(1)).astype(np.float64)
    t = y64 / d
    return (np.abs(t - np.floor(t) - 0.5) <= E / d) & (da > 0)


# ---- head cases ----------------------------------------------------------------------------------------------------------------------------
# name -> (cout, cout_pad, mode, n images, hw, decode planes, kc)
HEAD_CASES = {}
for _c in (1, 16, 17, 20, 32, 33, 48, 49, 64, 72, 80, 81, 96):
    HEAD_CASES[f"dyadic_c{_c}"] = (_c, ceil32(_c), "dyadic", 1, 70, 3, 32)
HEAD_CASES["dyadic_c20_pad64"] = (20, 64, "dyadic", 1, 70, 3, 32)
HEAD_CASES["dyadic_c40_pad96"] = (40, 96, "dyadic", 1, 70, 3, 32)
for _c in (20, 48, 72, 81, 96):
    HEAD_CASES[f"real_c{_c}"] = (_c, ceil32(_c), "real", 1, 70, 3, 32)
for _n, _hw in ((1, 1), (1, 31), (1, 32), (1, 33), (3, 45), (40, 1), (2, 257)):
    HEAD_CASES[f"rows_n{_n}_hw{_hw}"] = (72, 96, "dyadic", _n, _hw, 3, 256)
for _p in (1, 3, 4, 6):
    HEAD_CASES[f"decode_planes{_p}"] = (72, 96, "dyadic", 3, 45, _p, 256)
    HEAD_CASES[f"decode_planes{_p}_real"] = (20, 32, "real", 3, 45, _p, 32)
HEAD_CASES["decode_planes4_kc1"] = (72, 96, "dyadic", 3, 45, 4, 1)
REAL_HEAD_CASES = [k for k, v in HEAD_CASES.items() if v[2] == "real"]


@functools.lru_cache(maxsize=None)
def head_case(name):
    """Operands and references of one head case.  ``rows`` feed the rows-from-memory entries, ``codes`` + ``lut`` the decoding ones
    (``drows`` = ref_decode of them); ``heads`` carries every-third-channel-unquantized steps, ``heads_q`` (the u8 wire) a quantizer on every
    channel.  y64 / y64d: the float64 outputs [R][cout] on rows / drows."""
    cout, cout_pad, mode, n, hw, planes, kc = HEAD_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + cout)
    R = n * hw
    c = dict(name=name, mode=mode, n=n, hw=hw, R=R, planes=planes, kc=kc, cout=cout, cout_pad=cout_pad)
    c["rows"] = make_rows(rng, R, mode)
    c["lut"], c["lut_bias"] = make_lut(rng, planes, kc, mode)
    c["codes"] = make_codes(rng, planes, R, kc)
    c["drows"] = ref_decode(c["codes"], c["lut"], c["lut_bias"])
    c["heads"] = make_heads(rng, cout, cout_pad, mode)
    hq = dict(c["heads"])
    da = hq["da"].copy()
    za = hq["za"].copy()
    off = da <= 0
    da[off] = (2.0 ** rng.integers(-2, 7, size=int(off.sum()))) if mode == "dyadic" else rng.uniform(0.2, 0.4, size=int(off.sum()))
    za[off] = 37.0
    hq["da"], hq["za"] = da.astype(np.float32), za
    hq["da_pad"] = np.concatenate([hq["da"], np.full(cout_pad - cout, -1.0, np.float32)])
    hq["za_pad"] = np.concatenate([za, np.zeros(cout_pad - cout, np.float32)])
    c["heads_q"] = hq
    for key, rows in (("y64", c["rows"]), ("y64d", c["drows"])):
        c[key] = ref_heads64(rows, c["heads"]["w"], c["heads"]["bias"])
        c["E" + key[3:]] = heads_error_bound(rows, c["heads"]["w"], c["heads"]["bias"]) if mode == "real" else None
    return c


# ---- fuse cases ----------------------------------------------------------------------------------------------------------------------------
HM, WM, RATIO = 40.0, 100.0, 0.4            # hm / wm is no map's h / w; the ratio is no power of two
# a decoded feature is N(0, 1/16) per channel: the ego's score on itself is |f|^2 / 16 ~ 1 and its scores on the others N(0, 1/16), so every
# agent carries weight in the softmax (at N(0, 1) the ego's own e^16 would make attention the identity and hide the other agents)
FUSE_SCALE = 0.25
# world poses (x, y, yaw) of up to eight agents; one map is RATIO * WM = 40 m wide and RATIO * HM = 16 m high
POSES = [(0.0, 0.0, 0.0),                    # the ego: identity
         (4.0, 0.0, 0.0),                    # whole cells on a 20-wide map (2 m per cell)
         (0.7, -0.45, 0.0),                  # a fraction of a cell
         (0.3, 0.2, np.pi / 2),              # yaw 90
         (-1.1, 0.4, np.pi),                 # yaw 180
         (1.3, -0.7, np.deg2rad(37.0)),      # yaw 37
         (400.0, 160.0, 0.0),                # wholly out of view
         (1.0e9, -1.0e9, 0.0)]               # the bounds test before the float-to-int conversion


def _fc(h=3, w=5, scenes=(3,), planes=3, kc=32, ego=0, max_cav=8, fusion=0, feats=False, poses=None, special=None, seed=0):
    return dict(h=h, w=w, scenes=list(scenes), planes=planes, kc=kc, ego=ego, max_cav=max_cav, fusion=fusion, feats=feats, poses=poses,
                special=special, seed=seed)


FUSE_CASES = {}
for _a in range(1, 9):
    FUSE_CASES[f"agents{_a}_att"] = _fc(h=5, w=4, scenes=(_a,), seed=_a)
    FUSE_CASES[f"agents{_a}_max"] = _fc(h=5, w=4, scenes=(_a,), fusion=1, seed=20 + _a)
FUSE_CASES["ragged_batch"] = _fc(scenes=(1, 5, 8, 2, 7), seed=40)
FUSE_CASES["ragged_batch_ego1"] = _fc(scenes=(2, 5, 8, 2, 7), ego=1, seed=41)
for _p, _k in ((1, 1), (1, 256), (2, 32), (4, 256), (6, 32), (16, 1), (16, 256), (3, 256)):
    FUSE_CASES[f"planes{_p}_kc{_k}"] = _fc(scenes=(3,), planes=_p, kc=_k, seed=50 + _p + _k)
for _h, _w in ((1, 1), (1, 7), (3, 5), (5, 4), (12, 20), (7, 33)):
    FUSE_CASES[f"map_{_h}x{_w}"] = _fc(h=_h, w=_w, scenes=(6,), seed=60 + _h)
FUSE_CASES["transforms_att"] = _fc(h=12, w=20, scenes=(8,), seed=70)
FUSE_CASES["transforms_max_negative"] = _fc(h=12, w=20, scenes=(4,), fusion=1, poses=[[POSES[0], POSES[2], POSES[6], POSES[7]]], special="negative", seed=71)
for _n in (3, 6):
    for _r in range(_n):
        FUSE_CASES[f"ego{_r}_of{_n}"] = _fc(scenes=(_n,), ego=_r, seed=80 + _n)
FUSE_CASES["ego2_of6_7x33"] = _fc(h=7, w=33, scenes=(6,), ego=2, seed=88)
FUSE_CASES["saturated_softmax"] = _fc(h=5, w=4, scenes=(3,), kc=32, special="saturated", poses=[[POSES[0], POSES[0], POSES[2]]], seed=90)
FUSE_CASES["feats_att"] = _fc(scenes=(3, 1, 2), feats=True, seed=91)
FUSE_CASES["feats_max"] = _fc(scenes=(3, 1, 2), feats=True, fusion=1, seed=92)
BAND_RANGES = [(0, 7 * 33), (7 * 33 - 1, 1), (7, 45), (33, 0)]          # on map_7x33
ONE_LAUNCH_CASES = ["agents5_att", "ragged_batch", "map_7x33"]           # the last one over the band (7, 45)


@functools.lru_cache(maxsize=None)
def fuse_case(name):
    """Operands and the reference of one fuse case.  The code planes lie in the gathered-wire layout [agent][plane][cells] with gaps behind
    every plane and every agent (``code_level_stride`` > cells, ``code_agent_stride`` > planes * level stride), the gaps full of POISON_CODE;
    scene s starts ``offsets[s]`` bytes in.  ``feats`` cases: fp32 maps [agent][cells][256], NaN between the scenes, offsets in floats.
    ``dec[s]``: the scene's decoded maps f32 [n][h][w][256];  ``ref[s]`` / ``ref64[s]``: [cells][256]."""
    p = FUSE_CASES[name]
    rng = np.random.default_rng(1000 + p["seed"])
    h, w, planes, kc, scenes = p["h"], p["w"], p["planes"], p["kc"], p["scenes"]
    hw, total = h * w, sum(p["scenes"])
    c = dict(p, name=name, hw=hw, hm=HM, wm=WM, ratio=RATIO)
    poses = p["poses"] or [POSES[:n] for n in scenes]
    c["pairwise"] = make_pairwise(poses, p["max_cav"])
    starts = np.concatenate([[0], np.cumsum(scenes)[:-1]]).astype(np.int64)
    if p["feats"]:
        gap = 8                                                        # floats between two scenes (offsets stay multiples of 4)
        per = [rng.normal(0, FUSE_SCALE, (n, hw, 256)).astype(np.float32) for n in scenes]
        buf, offs = [], []
        for f in per:
            offs.append(sum(b.size for b in buf))
            buf += [f.reshape(-1), np.full(gap, np.nan, np.float32)]
        c["feats_buf"], c["offsets"] = np.concatenate(buf), np.asarray(offs, np.int64)
        c["dec"] = [f.reshape(-1, h, w, 256) for f in per]
        c["codes_buf"] = c["lut"] = c["lut_bias"] = None
        c["level_stride"] = c["agent_stride"] = 0
    else:
        lut, bias = make_lut(rng, planes, kc, "real")
        lut, bias = lut * np.float32(FUSE_SCALE), bias * np.float32(FUSE_SCALE)
        codes = make_codes(rng, planes, total * hw, kc)               # [planes][agents * cells]
        if p["special"] == "negative":
            lut, bias = -np.abs(lut), -np.abs(bias)
        if p["special"] == "saturated":
            # agent 1 = 8 x the ego's feature (plane 0 rows k + kc/2 = 8 x row k, the other planes and the bias two orders below): the ego's
            # score on agent 1 is 8 |f|^2 / 16 ~ 200 against |f|^2 / 16 ~ 25 on itself
            lut[0, kc // 2:] = 8.0 * lut[0, :kc // 2]
            lut[0] *= np.float32(10.0)
            lut[1:] *= np.float32(0.01)
            bias = bias * np.float32(0.01)
            cp = codes.reshape(planes, total, hw)
            cp[0, 0] = rng.integers(0, kc // 2, size=hw)
            cp[0, 1] = cp[0, 0] + kc // 2
            cp[1:, 1] = cp[1:, 0]
            cp[0, 2] = rng.integers(0, kc // 2, size=hw)
        level_stride = hw + 5
        agent_stride = planes * level_stride + 3
        wire = np.full(total * agent_stride + 16, POISON_CODE, np.uint8)
        for a in range(total):
            for l in range(planes):
                o = a * agent_stride + l * level_stride
                wire[o:o + hw] = codes[l, a * hw:(a + 1) * hw]
        c["codes_buf"], c["offsets"] = wire, starts * agent_stride
        c["level_stride"], c["agent_stride"] = level_stride, agent_stride
        c["lut"], c["lut_bias"], c["feats_buf"] = lut, bias, None
        dec = ref_decode(codes, lut, bias).reshape(total, h, w, 256)
        c["dec"] = [dec[s0:s0 + n] for s0, n in zip(starts, scenes)]
    args = (p["ego"], HM, WM, RATIO, p["fusion"])
    c["ref"] = [ref_fuse(c["dec"][s], c["pairwise"][s], n, *args).reshape(hw, 256) for s, n in enumerate(scenes)]
    c["ref64"] = [ref_fuse64(c["dec"][s], c["pairwise"][s], n, *args).reshape(hw, 256) for s, n in enumerate(scenes)]
    return c


# ---- table-form cases ----------------------------------------------------------------------------------------------------------------------
# qv2x_single_heads_lut_f32: (levels, kc, cout, agents, hw)
LUT_CASES = {}
for _l in (1, 2, 3, 4):
    for (_k, _c), (_a, _hw) in zip(((128, 20), (32, 96), (256, 1)), ((3, 45), (1, 64), (2, 100))):
        LUT_CASES[f"l{_l}_kc{_k}_c{_c}"] = (_l, _k, _c, _a, _hw)
LUT_CASES["groups2"] = (3, 128, 20, 5, 13123)                          # 65 615 cells = 1026 runs of 64: two runs per workgroup
# qv2x_table_heads_f32: (planes, kc, c0, c1, R, hw)
TABLE_CASES = {}
for _c0, _c1 in ((72, 20), (0, 8), (7, 0), (70, 21)):
    TABLE_CASES[f"lds_{_c0}_{_c1}"] = (3, 32, _c0, _c1, 3 * 45, 45)
for _p, _k in ((6, 256), (16, 32)):
    for (_c0, _c1), (_R, _hw) in zip(((0, 4), (72, 20), (128, 0)), ((1, 1), (33, 33), (3 * 45, 45))):
        TABLE_CASES[f"global_p{_p}_kc{_k}_{_c0}_{_c1}"] = (_p, _k, _c0, _c1, _R, _hw)
TABLE_CASES["global_p3_kc256_128_0"] = (3, 256, 128, 0, 33, 33)
TABLE_CASES["global_p3_kc256_72_56"] = (3, 256, 72, 56, 3 * 45, 45)


@functools.lru_cache(maxsize=None)
def table_case(name, mode):
    """(codes [planes][R], tables f32 [planes][kc][CT], bias f32, da, za, float64 tables and bias) of a LUT_CASES / TABLE_CASES entry"""
    if name in LUT_CASES:
        planes, kc, ct, a, hw = LUT_CASES[name]
        R = a * hw
    else:
        planes, kc, c0, c1, R, hw = TABLE_CASES[name]
        ct = c0 + c1
    rng = np.random.default_rng(sum(name.encode()) * 31 + (mode == "real"))
    codes = make_codes(rng, planes, R, kc)
    if mode == "dyadic":
        t64, b64 = dyadic_ints(rng, (planes, kc, ct), -1).astype(np.float64), dyadic_ints(rng, ct, -1).astype(np.float64)
        da = (2.0 ** rng.integers(-5, 3, size=ct)).astype(np.float32)
    else:
        lut, lb = make_lut(rng, planes, kc, "real")
        t64, b64 = collapse_tables(lut, lb, rng.normal(0, 0.25, (ct, 256)).astype(np.float32), rng.normal(0, 1, ct).astype(np.float32))
        da = rng.uniform(0.2, 0.4, size=ct).astype(np.float32)
    za = np.asarray((0, 37, 255), np.float32)[(np.arange(ct) // 2) % 3]
    da[2::3] = -1.0
    return dict(planes=planes, kc=kc, ct=ct, R=R, hw=hw, codes=codes, t64=t64, b64=b64, tables=t64.astype(np.float32), bias=b64.astype(np.float32),
                da=da, za=za, mode=mode)


# ---- qv2x_heads_pair_f32: name -> (hw, images of job 0, agents of job 1, (cout, cout_pad) of job 0, of job 1, planes); dyadic, kc = 256 ------
PAIR_CASES = {
    "r293_r879": (293, 1, 3, (72, 96), (20, 32), 3),
    "r300_r60": (60, 5, 1, (96, 96), (17, 32), 3),
    "r879_r293_rowwise": (293, 3, 1, (20, 32), (81, 96), 6),
    "tail16_and_pad64": (60, 5, 1, (16, 32), (20, 64), 3),
    "pad96_and_c1": (293, 1, 3, (40, 96), (1, 32), 4),
}


@functools.lru_cache(maxsize=None)
def pair_case(name):
    hw, n0, n1, (c0, p0), (c1, p1), planes = PAIR_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 13 + hw)
    kc = 256
    c = dict(hw=hw, n0=n0, n1=n1, planes=planes, kc=kc, rows=make_rows(rng, n0 * hw, "dyadic"), codes=make_codes(rng, planes, n1 * hw, kc))
    c["lut"], c["lut_bias"] = make_lut(rng, planes, kc, "dyadic")
    c["drows"] = ref_decode(c["codes"], c["lut"], c["lut_bias"])
    c["h0"], c["h1"] = make_heads(rng, c0, p0, "dyadic"), make_heads(rng, c1, p1, "dyadic")
    return c


# ---- the one-launch entries on one agent per scene and T = I: name -> (h, w, scenes, cout, cout_pad); dyadic, three planes of 32 -------------
IDENTITY_CASES = {f"{_h}x{_w}_s{_s}_c{_c}_pad{_p}": (_h, _w, _s, _c, _p) for _h, _w, _s, _c, _p in (
    (2, 16, 1, 72, 96), (4, 32, 3, 72, 96), (1, 64, 2, 72, 96), (4, 32, 3, 16, 32), (2, 16, 1, 1, 32), (4, 32, 3, 17, 32), (1, 64, 2, 49, 64),
    (2, 16, 1, 81, 96), (4, 32, 3, 96, 96), (4, 32, 3, 20, 64), (1, 64, 2, 40, 96))}


@functools.lru_cache(maxsize=None)
def identity_case(name, every_quantized):
    from oracle.geometry import pairwise_from_poses
    h, w, scenes, cout, cout_pad = IDENTITY_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 17 + every_quantized)
    hw, planes, kc = h * w, 3, 32
    c = dict(h=h, w=w, hw=hw, scenes=scenes, planes=planes, kc=kc)
    c["lut"], c["lut_bias"] = make_lut(rng, planes, kc, "dyadic")
    c["codes"] = make_codes(rng, planes, scenes * hw, kc)
    c["drows"] = ref_decode(c["codes"], c["lut"], c["lut_bias"])
    c["pairwise"] = np.stack([pairwise_from_poses([np.eye(4)], 2)] * scenes)
    c["heads"] = make_heads(rng, cout, cout_pad, "dyadic", every_quantized=every_quantized)
    c["level_stride"], c["agent_stride"] = hw + 3, planes * (hw + 3) + 1
    wire = np.full(scenes * c["agent_stride"], POISON_CODE, np.uint8)
    for s in range(scenes):
        for l in range(planes):
            o = s * c["agent_stride"] + l * c["level_stride"]
            wire[o:o + hw] = c["codes"][l, s * hw:(s + 1) * hw]
    c["codes_buf"] = wire
    return c


# ---- qv2x_decode_lut_f32: (R, planes, kc) ------------------------------------------------------------------------------------------------------
DECODE_CASES = [(R, p, k) for R in (1, 3, 4, 5, 130) for p in (1, 3, 6, 16) for k in (1, 256)]


@functools.lru_cache(maxsize=None)
def decode_case(R, planes, kc, mode):
    rng = np.random.default_rng(R * 100 + planes + kc + (mode == "real"))
    lut, lb = make_lut(rng, planes, kc, mode)
    return dict(lut=lut, lut_bias=lb, codes=make_codes(rng, planes, R, kc))
