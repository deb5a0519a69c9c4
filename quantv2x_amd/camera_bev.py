"""Camera agents in the Pyramid model, between the lift-splat's BEV and the fusion: host statements in numpy over the CPU checker, host-side
packing, and the device wrapper of ``qv2x_bev_entry_f32`` (include/qv2x.h).

ENTRY  f32 BEV [n, cin, H, W] -> conv1 of the first ``QuantBasicBlock`` (3x3, stride, pad 1, dequantized weights) -> ReLU -> activation
       quantizer -> codes, and the block's shortcut (strided 1x1 ``downsample`` or the input itself) as fp32
CROP   the centre crop / zero pad of a camera map to the LiDAR range (reference ``heter_pyramid_collab.py:173-190``)
MASK   the camera agents' score mask of every pyramid level (reference ``fuse_modules/pyramid_fuse.py:147-160``)

Activation codes travel as in the rest of the project: uint8 ``[N, H, W, C]`` in the statements, padded int8 ``[N, H + 2, W + 2, C]``
(code - 128) on the device.  A PTQ state is the flat dict of ``ptq_state`` (``<module>/w_code`` ...)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .camera_encoder import dequant_weight


# ---- ENTRY -----------------------------------------------------------------------------------------------------------------------------------

def entry_shapes(h: int, w: int, stride: int):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def entry_constants(state, block_name):
    """(w1 f32 [9 cin, cout] with k = (ky*3 + kx)*cin + ci, b1 [cout], (delta, zp) of conv1, wd f32 [cin, cout] | None, bd [cout] | None) of
    the block ``block_name`` of a PTQ state: dequantized weights fl((code - zw[co]) * dw[co])"""
    c1, ds = block_name + ".conv1", block_name + ".downsample"
    code = state[c1 + "/w_code"]
    if code.ndim != 4 or code.shape[2:] != (3, 3):
        raise NotImplementedError(f"{c1}: a 3x3 convolution expected (weight of shape {tuple(code.shape)})")
    if bool(state[c1 + "/a_off"]):
        raise ValueError(f"{c1}: conv1's activation quantizer is disabled; conv2 runs on its codes")
    cout, cin = code.shape[:2]
    w1 = np.ascontiguousarray(dequant_weight(state, c1).transpose(2, 3, 1, 0).reshape(9 * cin, cout))
    b1 = _bias(state, c1, cout)
    q = (float(np.float32(state[c1 + "/a_delta"])), int(state[c1 + "/a_zp"]))
    if ds + "/w_code" not in state:
        return w1, b1, q, None, None
    dcode = state[ds + "/w_code"]
    if dcode.shape != (cout, cin, 1, 1):
        raise NotImplementedError(f"{ds}: a 1x1 convolution {cin} -> {cout} expected (weight of shape {tuple(dcode.shape)})")
    if not bool(state[ds + "/a_off"]):
        raise ValueError(f"{ds}: the shortcut feeds the block's fp32 add (disable_act_quant); this one has an activation quantizer")
    wd = np.ascontiguousarray(dequant_weight(state, ds).reshape(cout, cin).T)
    return w1, b1, q, wd, _bias(state, ds, cout)


def _bias(state, name, cout):
    b = np.asarray(state[name + "/bias"], np.float32)
    return b if b.size == cout else np.zeros(cout, np.float32)


def im2col_rows(x_nchw, stride: int) -> np.ndarray:
    """f32 [n * ho * wo, 9 cin]: the zero-padded 3x3 windows of an NCHW map in the chain's k order (ky*3 + kx)*cin + ci"""
    x = np.asarray(x_nchw, np.float32)
    n, cin, h, w = x.shape
    ho, wo = entry_shapes(h, w, stride)
    pad = np.zeros((n, cin, stride * (ho - 1) + 3, stride * (wo - 1) + 3), np.float32)     # rows s yo + ky - 1: -1 .. s (ho - 1) + 1
    pad[:, :, 1:1 + h, 1:1 + w] = x
    rows = np.empty((n, ho, wo, 9, cin), np.float32)
    for ky in range(3):
        for kx in range(3):
            rows[:, :, :, ky * 3 + kx] = pad[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride].transpose(0, 2, 3, 1)
    return rows.reshape(n * ho * wo, 9 * cin)


def chain_rows(rows, w_kc) -> np.ndarray:
    """f32 [R, cout]: per output ONE ascending-k fmaf chain from +0 (the checker's ``orc_linear`` without a bias); rows [R, K], w [K, cout]"""
    from oracle.spec import _f32, _p, lib as olib
    rows, wt = _f32(rows), _f32(np.asarray(w_kc, np.float32).T)
    out = np.zeros((rows.shape[0], wt.shape[0]), np.float32)
    olib().orc_linear(_p(rows), rows.shape[0], rows.shape[1], _p(wt), None, wt.shape[0], _p(out))
    return out


def bev_entry_statement(x_nchw, state, block_name, stride: int):
    """(conv1 codes u8 [n, ho, wo, cout], its (delta, zp), shortcut f32 [n, ho, wo, cout]): what ``qv2x_bev_entry_f32`` computes, bit for bit.
    conv1 is the checker's ``orc_deconv_f32in`` with s = 1 on the im2col rows (the ascending chain, + bias, ReLU, the epilogue quantizer);
    the shortcut the same chain over the centre pixels, + bias, fp32 -- or the input itself when the block has no ``downsample``."""
    from oracle.spec import _cf, _f32, _p, lib as olib
    if stride not in (1, 2):
        raise ValueError(f"stride {stride}: 1 or 2")
    x = np.asarray(x_nchw, np.float32)
    n, cin, h, w = x.shape
    w1, b1, (da, za), wd, bd = entry_constants(state, block_name)
    if w1.shape[0] != 9 * cin:
        raise ValueError(f"{block_name}.conv1 takes {w1.shape[0] // 9} channels, the map has {cin}")
    cout = w1.shape[1]
    ho, wo = entry_shapes(h, w, stride)
    rows = im2col_rows(x, stride)
    codes = np.zeros((n, ho, wo, cout), np.uint8)
    w4 = _f32(w1.reshape(9 * cin, cout, 1, 1))
    olib().orc_deconv_f32in(_p(rows), n, ho, wo, 9 * cin, _p(w4), _p(_f32(b1)), cout, 1, 1, _cf(da), _cf(za), _p(codes), cout, 0)
    centre = np.ascontiguousarray(x[:, :, ::stride, ::stride].transpose(0, 2, 3, 1))
    if wd is None:
        if stride != 1 or cin != cout:
            raise ValueError(f"{block_name}: no downsample module, but stride {stride} and {cin} -> {cout} channels")
        return codes, (da, za), centre
    short = (chain_rows(centre.reshape(-1, cin), wd) + bd[None, :]).astype(np.float32).reshape(n, ho, wo, cout)
    return codes, (da, za), short


def pack_entry_weights(w_kc) -> np.ndarray:
    """[K, cout] -> f32 [K / 8, cout, 2, 4]: element [g][co][p][j] = w[8 g + 2 j + p][co] (MFMA k-step j of group g, k parity p)"""
    w = np.asarray(w_kc, np.float32)
    k, cout = w.shape
    assert k % 8 == 0
    return np.ascontiguousarray(w.reshape(k // 8, 4, 2, cout).transpose(0, 3, 2, 1))


class BevEntry:
    """Device constants of one block's input side and the launch of ``qv2x_bev_entry_f32``."""

    def __init__(self, state, block_name, stride, device):
        import torch
        w1, b1, (self.delta, self.zp), wd, bd = entry_constants(state, block_name)
        self.cin, self.cout, self.stride = w1.shape[0] // 9, w1.shape[1], int(stride)
        dev = torch.device(device)
        self.w1 = torch.from_numpy(pack_entry_weights(w1)).to(dev)
        self.b1 = torch.from_numpy(b1.copy()).to(dev)
        self.wd = torch.from_numpy(pack_entry_weights(wd)).to(dev) if wd is not None else None
        self.bd = torch.from_numpy(bd.copy()).to(dev) if wd is not None else None

    def __call__(self, x, out, shortcut):
        """x f32 [n, cin, H, W] (contiguous); out i8 [n, ho + 2, wo + 2, cout]; shortcut f32 [n * ho * wo, cout]"""
        from . import lib as L
        n, cin, h, w = x.shape
        ho, wo = entry_shapes(h, w, self.stride)
        assert cin == self.cin and x.is_contiguous() and out.is_contiguous() and shortcut.is_contiguous()
        assert tuple(out.shape) == (n, ho + 2, wo + 2, self.cout) and shortcut.numel() == n * ho * wo * self.cout
        d = L.BevEntryDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.stride, d.downsample = n, h, w, cin, self.cout, self.stride, int(self.wd is not None)
        d.out_delta, d.out_zp = self.delta, float(self.zp)
        L.check(L.load().qv2x_bev_entry_f32(C.byref(d), L.ptr(x), L.ptr(self.w1), L.ptr(self.b1), L.ptr(self.wd), L.ptr(self.bd), L.ptr(out),
                                            L.ptr(shortcut), L.current_stream()), "qv2x_bev_entry_f32")


# ---- CROP ------------------------------------------------------------------------------------------------------------------------------------

def crop_target(size: int, ratio: float) -> int:
    """``int(H * crop_ratio)`` (heter_pyramid_collab.py:181-182) in Python floats"""
    return int(size * float(ratio))


def center_crop_window(h: int, w: int, th: int, tw: int):
    """torchvision ``CenterCrop`` arithmetic, restated from its source (functional.center_crop) and NOT pinned against it (torchvision is not
    installed where this project is tested): ((pad top, bottom, left, right), (crop top, crop left) in the padded map)"""
    top = (th - h) // 2 if th > h else 0
    bottom = (th - h + 1) // 2 if th > h else 0
    left = (tw - w) // 2 if tw > w else 0
    right = (tw - w + 1) // 2 if tw > w else 0
    ph, pw = h + top + bottom, w + left + right
    return (top, bottom, left, right), (int(round((ph - th) / 2.0)), int(round((pw - tw) / 2.0)))


def center_crop_pad_statement(x, target_h: int, target_w: int, fill=0):
    """``CenterCrop((target_h, target_w))`` on the last two axes of ``x``: pad with ``fill`` where the target is larger, then crop"""
    x = np.asarray(x)
    h, w = x.shape[-2:]
    (top, bottom, left, right), (ct, cl) = center_crop_window(h, w, target_h, target_w)
    if top or bottom or left or right:
        x = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(top, bottom), (left, right)], constant_values=fill)
    return np.ascontiguousarray(x[..., ct:ct + target_h, cl:cl + target_w])


# ---- MASK ------------------------------------------------------------------------------------------------------------------------------------

def crop_mask_rect(cam_crop_info, modality, h: int, w: int):
    """(start_h, end_h, start_w, end_w) of pyramid_fuse.py:151-157, literally, in Python floats"""
    H, W = h, w
    crop_H = H / cam_crop_info[modality][f"crop_ratio_H_{modality}"] - 4
    crop_W = W / cam_crop_info[modality][f"crop_ratio_W_{modality}"] - 4
    return int(H // 2 - crop_H // 2), int(H // 2 + crop_H // 2), int(W // 2 - crop_W // 2), int(W // 2 + crop_W // 2)


def crop_mask_statement(agent_modalities, cam_crop_info, h: int, w: int) -> np.ndarray:
    """f32 [n, h * w] of 0 / 1: what multiplies the scores of a level of h x w cells (pyramid_fuse.py:147-160, eval mode).  Ones for every agent
    whose modality is not in ``cam_crop_info``; for a camera agent ones inside its rectangle, taken with Python slice semantics as the reference's
    indexing does: a negative start wraps, start >= end is empty (the agent's scores are then zero everywhere)."""
    mask = np.ones((len(agent_modalities), h, w), np.float32)
    for m in (cam_crop_info or {}):
        sh, eh, sw, ew = crop_mask_rect(cam_crop_info, m, h, w)
        sel = np.array([a == m for a in agent_modalities], bool)
        sub = mask[sel]
        sub[:, sh:eh, sw:ew] = 0
        mask[sel] = 1 - sub
    return mask.reshape(len(agent_modalities), h * w)
