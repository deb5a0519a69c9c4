"""The two ends of the int8 ResNet image encoder of camera agents (``QuantCamEncode_Resnet101``, reference ``quant_block.py:744-860``): host
statements in numpy, host-side packing, and the device wrappers of ``qv2x_cam_stem_f32`` / ``qv2x_cam_heads_i8`` (include/qv2x.h,
DESIGN.md section 14).

STEM   f32 image -> conv1 7x7 / 2 (BN folded, dequantized weights) -> ReLU -> activation quantizer -> 3x3 / 2 max-pool, codes out
HEADS  codes -> depth_head (cin -> D) and image_head (cin -> C), each fake-quantized with its own (delta, zp), f32 out

Activation codes travel as in the rest of the project: uint8 ``[N, H, W, C]`` in the statements, padded int8 ``[N, H + 2, W + 2, C]``
(code - 128) on the device.  A PTQ state is the flat dict of ``ptq_state`` (``<module>/w_code`` ...)."""
from __future__ import annotations

import ctypes as C

import numpy as np

_LD = np.longdouble
STEM_COUT, STEM_K, STEM_CIN = 64, 7, 3


def fma32(a, b, c) -> np.ndarray:
    """float32 fused multiply-add in numpy: ``a * b + c`` evaluated in ``np.longdouble`` and rounded once to float32.  With a 64-bit
    significand (x86) the 48-bit product of two float32 is exact and so is the sum unless the addends lie more than 16 binades apart; there the
    sum is rounded to 64 bits first, and the second rounding to 24 bits differs from a true fma only when the 64-bit value lands exactly on a
    float32 tie that the exact value misses -- 40 given bits, never seen, and impossible to hit by accident.  On a platform whose
    long double is a plain double (53 bits) the statement refuses instead of returning near-misses."""
    if np.finfo(_LD).nmant < 63:
        raise RuntimeError("camera_encoder.fma32: np.longdouble with a 64-bit significand expected (x86 extended precision)")
    return (np.asarray(a, np.float32).astype(_LD) * np.asarray(b, np.float32).astype(_LD) + np.asarray(c, np.float32).astype(_LD)).astype(np.float32)


def q_code_mul(y, delta, zp) -> np.ndarray:
    """common.h's epilogue quantizer: clamp(rint(fma(y, fl(1 / delta), zp)), 0, 255) as float32 (rint = round half to even)"""
    rd = np.float32(1.0) / np.float32(delta)
    return np.clip(np.rint(fma32(y, rd, np.float32(zp))), 0.0, 255.0).astype(np.float32)


def dequant_weight(state, name) -> np.ndarray:
    """fl((code - zp[co]) * delta[co]) of a module whose scales run along dim 0, as ``_DenseF32In`` builds its own"""
    code = state[name + "/w_code"].astype(np.float32)
    shape = (-1,) + (1,) * (code.ndim - 1)
    return ((code - state[name + "/w_zp"].astype(np.float32).reshape(shape)) * state[name + "/w_delta"].astype(np.float32).reshape(shape)).astype(np.float32)


def stem_constants(state, name="conv1"):
    """(wdeq f32 [7, 7, 3, 64] = [ky][kx][ci][co], bias f32 [64], (delta, zp)) of the stem convolution of a camera state"""
    code = state[name + "/w_code"]
    if code.shape != (STEM_COUT, STEM_CIN, STEM_K, STEM_K):
        raise NotImplementedError(f"{name}: the stem is a 7x7 convolution 3 -> 64 (got a weight of shape {tuple(code.shape)})")
    if bool(state[name + "/a_off"]):
        raise ValueError(f"{name}: the stem's activation quantizer is disabled; the trunk runs on its codes")
    wdeq = np.ascontiguousarray(dequant_weight(state, name).transpose(2, 3, 1, 0))
    bias = state[name + "/bias"].astype(np.float32)
    if bias.size != STEM_COUT:
        bias = np.zeros(STEM_COUT, np.float32)
    return wdeq, bias, (float(np.float32(state[name + "/a_delta"])), int(state[name + "/a_zp"]))


def stem_shapes(h: int, w: int):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return hc, wc, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1


def stem_conv_statement(imgs, wdeq, bias) -> np.ndarray:
    """f32 [V, Hc, Wc, 64]: the pre-activation of the stem, the ascending (ky, kx, ci) fmaf chain from +0 plus the bias, bit for bit what
    ``qv2x_cam_stem_f32`` accumulates (``fma32`` says how a float32 fma is had in numpy).  ``imgs`` f32 [V, >= 3, H, W]: channels 0..2."""
    imgs = np.asarray(imgs, np.float32)
    v, _, h, w = imgs.shape
    hc, wc, _, _ = stem_shapes(h, w)
    pad = np.zeros((v, 3, 2 * hc + 5, 2 * wc + 5), np.float32)            # rows 2i + ky - 3 for i < hc, ky < 7: -3 .. 2 hc + 1
    pad[:, :, 3:3 + h, 3:3 + w] = imgs[:, :3]
    acc = np.zeros((v, hc, wc, STEM_COUT), np.float32)
    for ky in range(STEM_K):
        for kx in range(STEM_K):
            for ci in range(STEM_CIN):
                x = pad[:, ci, ky:ky + 2 * hc:2, kx:kx + 2 * wc:2]
                acc = fma32(x[..., None], wdeq[ky, kx, ci][None, None, None, :], acc)
    return (acc + np.asarray(bias, np.float32)).astype(np.float32)


def maxpool_codes(codes) -> np.ndarray:
    """3x3 stride-2 pad-1 max-pool of uint8 codes [V, Hc, Wc, C]; outside the map counts as -inf (here: code 0, the lowest)"""
    v, hc, wc, c = codes.shape
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    pad = np.zeros((v, 2 * hp + 1, 2 * wp + 1, c), codes.dtype)
    pad[:, 1:1 + hc, 1:1 + wc] = codes
    out = np.zeros((v, hp, wp, c), codes.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, pad[:, dy:dy + 2 * hp:2, dx:dx + 2 * wp:2])
    return out


def stem_statement(imgs, wdeq, bias, delta, zp, want_conv=False):
    """uint8 codes [V, Hp, Wp, 64] of the stem: conv chain -> ReLU -> quantizer -> max-pool of the codes (the quantizer is monotone, so the max
    of the codes is the code of the max).  ``want_conv``: also the conv-resolution codes [V, Hc, Wc, 64], what ``QuantModule`` conv1 returns."""
    y = np.maximum(stem_conv_statement(imgs, wdeq, bias), np.float32(0.0))
    conv = q_code_mul(y, delta, zp).astype(np.uint8)
    pooled = maxpool_codes(conv)
    return (pooled, conv) if want_conv else pooled


def head_statement(x, in_q, state, name) -> np.ndarray:
    """One head of ``cam_heads_statement``: x uint8 [V, h, w, cin] with quantizer ``in_q`` -> f32 [V, cout, h, w]"""
    code = state[name + "/w_code"]
    cout, cin = code.shape[:2]
    if code.shape[2:] != (1, 1) or cin != x.shape[-1]:
        raise ValueError(f"{name}: a 1x1 convolution on {x.shape[-1]} channels expected, the weight is {tuple(code.shape)}")
    wz = code.reshape(cout, cin).astype(np.int64) - np.rint(state[name + "/w_zp"]).astype(np.int64)[:, None]
    T = (x.astype(np.int64) - int(in_q[1])) @ wz.T                                            # exact
    scale = (np.float32(in_q[0]) * state[name + "/w_delta"].astype(np.float32)).astype(np.float32)
    bias = state[name + "/bias"].astype(np.float32) if state[name + "/bias"].size else np.zeros(cout, np.float32)
    y = (bias + (T.astype(np.float32) * scale).astype(np.float32)).astype(np.float32)
    delta, zp = np.float32(state[name + "/a_delta"]), np.float32(state[name + "/a_zp"])
    out = ((q_code_mul(y, delta, zp).astype(np.int32) - int(zp)).astype(np.float32) * delta).astype(np.float32)     # integer codes: never -0
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def cam_heads_statement(x, in_q, state, depth_name="depth_head", feat_name="image_head"):
    """(depth f32 [V, D, h, w], feats f32 [V, C, h, w]): per head T = sum (x - zx)(w - zw) in int64, y = bias + float32(T) * scale,
    code = clamp(rint(fma(y, fl(1 / delta), zp)), 0, 255), value = fl(float32(code - zp) * delta) -- no ReLU in front of the quantizer."""
    return head_statement(x, in_q, state, depth_name), head_statement(x, in_q, state, feat_name)


def heads_constants(state, in_q, depth_name="depth_head", feat_name="image_head") -> dict:
    """The joint row list of both heads as ``qv2x_cam_heads_i8`` takes it: each head's rows padded to a multiple of 32 with zero rows."""
    parts = {k: [] for k in ("ws", "scale", "aw", "bias")}
    dims, qs, cin = [], [], None
    for name in (depth_name, feat_name):
        code = state[name + "/w_code"]
        cout = code.shape[0]
        if code.shape[2:] != (1, 1) or code.shape[1] % 32:
            raise NotImplementedError(f"{name}: a 1x1 convolution with cin % 32 == 0")
        if cin not in (None, code.shape[1]):
            raise ValueError("the two heads read the same map: equal cin expected")
        if bool(state[name + "/a_off"]):
            raise ValueError(f"{name}: its activation quantizer is disabled; the deployed heads write fake-quantized values")
        cin = code.shape[1]
        padn = -cout % 32
        parts["ws"].append(np.concatenate([code.reshape(cout, cin).astype(np.int64) - 128, np.zeros((padn, cin), np.int64)]))
        parts["aw"].append(np.concatenate([128 - np.rint(state[name + "/w_zp"]).astype(np.int64), np.zeros(padn, np.int64)]))
        parts["scale"].append(np.concatenate([(np.float32(in_q[0]) * state[name + "/w_delta"].astype(np.float32)).astype(np.float32), np.zeros(padn, np.float32)]))
        b = state[name + "/bias"].astype(np.float32) if state[name + "/bias"].size else np.zeros(cout, np.float32)
        parts["bias"].append(np.concatenate([b, np.zeros(padn, np.float32)]))
        dims.append(cout)
        qs.append((float(np.float32(state[name + "/a_delta"])), int(state[name + "/a_zp"])))
    ws, aw = np.concatenate(parts["ws"]), np.concatenate(parts["aw"])
    ax = 128 - int(in_q[1])
    corr = ax * ws.sum(axis=1) + cin * ax * aw
    assert np.abs(corr).max() < 2 ** 31
    rows = ws.shape[0]
    frag = ws.astype(np.int8).reshape(rows // 32, 32, cin // 32, 2, 16).transpose(0, 2, 3, 1, 4)      # [row/32][ci/32][half][row%32][16]
    return {"w": np.ascontiguousarray(frag), "scale": np.concatenate(parts["scale"]), "corr": corr.astype(np.int32), "aw": aw.astype(np.int32),
            "bias": np.concatenate(parts["bias"]), "cin": cin, "depth_bins": dims[0], "features": dims[1], "depth_q": qs[0], "feat_q": qs[1]}


class GpuCamStem:
    """``qv2x_cam_stem_f32`` with its constants on the device.  ``__call__(imgs, out)``: imgs f32 [V, 3 | 4, H, W] on the device (a 4-channel
    RGB-D tensor passes as it is), out padded int8 [V, Hp + 2, Wp + 2, 64] whose interior is written."""

    def __init__(self, state, name="conv1", device="cuda"):
        import torch
        from . import lib as L
        self.lib = L.load()
        wdeq, bias, self.out_q = stem_constants(state, name)
        self.w, self.bias = torch.from_numpy(wdeq).to(device), torch.from_numpy(bias).to(device)
        self.name = name

    def __call__(self, imgs, out):
        import torch
        from . import lib as L
        v, ch, h, w = imgs.shape
        _, _, hp, wp = stem_shapes(h, w)
        if imgs.dtype != torch.float32 or not imgs.is_contiguous() or ch < 3:
            raise ValueError("GpuCamStem: a contiguous float32 tensor [V, >= 3, H, W] expected")
        if tuple(out.shape) != (v, hp + 2, wp + 2, STEM_COUT) or not out.is_contiguous():
            raise ValueError(f"GpuCamStem: out {tuple(out.shape)}: {(v, hp + 2, wp + 2, STEM_COUT)} expected")
        d = L.CamStemDesc()
        d.views, d.h, d.w, d.view_stride = v, h, w, ch * h * w
        d.out_delta, d.out_zp = self.out_q[0], float(self.out_q[1])
        L.check(self.lib.qv2x_cam_stem_f32(C.byref(d), L.ptr(imgs), L.ptr(self.w), L.ptr(self.bias), L.ptr(out), L.current_stream()), self.name)
        return out


class GpuCamHeads:
    """``qv2x_cam_heads_i8`` with its constants on the device.  ``__call__(x, depth, feats)``: x padded int8 [V, h + 2, w + 2, cin]."""

    def __init__(self, state, in_q, depth_name="depth_head", feat_name="image_head", device="cuda"):
        import torch
        from . import lib as L
        self.lib = L.load()
        k = heads_constants(state, in_q, depth_name, feat_name)
        for key in ("w", "scale", "corr", "aw", "bias"):
            setattr(self, key, torch.from_numpy(k[key]).to(device))
        self.cin, self.depth_bins, self.features, self.depth_q, self.feat_q = k["cin"], k["depth_bins"], k["features"], k["depth_q"], k["feat_q"]

    def __call__(self, x, depth, feats):
        from . import lib as L
        v, h, w = x.shape[0], x.shape[1] - 2, x.shape[2] - 2
        if x.shape[-1] != self.cin or not x.is_contiguous():
            raise ValueError(f"GpuCamHeads: a contiguous padded map with {self.cin} channels expected")
        if tuple(depth.shape) != (v, self.depth_bins, h, w) or tuple(feats.shape) != (v, self.features, h, w) or not depth.is_contiguous() or not feats.is_contiguous():
            raise ValueError(f"GpuCamHeads: depth {(v, self.depth_bins, h, w)} and feats {(v, self.features, h, w)} expected")
        d = L.CamHeadsDesc()
        d.views, d.h, d.w, d.cin, d.depth_bins, d.features = v, h, w, self.cin, self.depth_bins, self.features
        d.depth_delta, d.depth_zp = self.depth_q[0], float(self.depth_q[1])
        d.feat_delta, d.feat_zp = self.feat_q[0], float(self.feat_q[1])
        L.check(self.lib.qv2x_cam_heads_i8(C.byref(d), L.ptr(x), L.ptr(self.w), L.ptr(self.scale), L.ptr(self.corr), L.ptr(self.aw), L.ptr(self.bias),
                                           L.ptr(depth), L.ptr(feats), L.current_stream()), "qv2x_cam_heads_i8")
        return depth, feats
