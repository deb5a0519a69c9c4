"""Deployed W8A8 hot path on MI355X: host side of ``libqv2x.so``.

``deploy(qt_model)`` takes a calibrated ``QuantModel`` (the reference's ``opencood.quant.QuantModel`` or this
build's mirror -- only attribute names are read) of the network shape this engine hard-wires -- PointPillar
encoder, BaseBEVBackbone, shrinker, optional codebook or NaiveCompressor, AttFusion or MaxFusion, 1x1 heads, BN folded, ReLU on every
conv / deconv (the HEAL Pyramid model has its own engine, ``engine_pyramid.py``);
``ptq_state.export_ptq_state`` raises ``NotImplementedError`` for anything else (other fusions, a post-fusion
``shrink_header``, unfolded BN, ``disable_act_quant`` off the heads) -- freezes its PTQ state and
returns a ``DeployedModel``: an ``nn.Module`` with the reference's model contract

    out = model(data_dict)      # data_dict = batch['ego'];  out: cls_preds / reg_preds / dir_preds / preds_tensor

whose forward is the chain of HIP kernels declared in ``include/qv2x.h`` (PyTorch only provides device memory
and the stream).  The codebook runs the deterministic ``encode -> decode`` pair (the wire format); see
DESIGN.md for why the reference's Gumbel ``forward`` is not used at inference.

There is no CPU / eager fallback here: if ``libqv2x.so`` is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import lib as L
from .ptq_state import export_ptq_state, load_ptq_state

_HEADS = ("cls_head", "reg_head", "dir_head")


def _dev(a: np.ndarray, dev) -> torch.Tensor:
    """numpy -> device tensor, always C-contiguous (the kernels take raw pointers)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous()


def _pack_k4(w: np.ndarray) -> np.ndarray:
    """[J, K] row-major (out = W x) -> [K/4][J][4] float32: four consecutive k innermost, J coalesced per wave."""
    j, k = w.shape
    assert k % 4 == 0
    return np.ascontiguousarray(w.T.reshape(k // 4, 4, j).transpose(0, 2, 1), dtype=np.float32)


def decode_tables(state: Dict[str, np.ndarray], levels: int, width: int = 256):
    """UMGMQuantizer.decode (codebook.py:339-343, 263-269) collapsed: every head is affine, so
    decode(c_0..c_{L-1}) = bias + sum_l T_l[c_l].  float64 algebra, fp32 tables ``[L][kc][width]``."""
    g = lambda l, n: state[f"codebook/{l}/{n}"].astype(np.float64)
    tables, const, chain = [], np.zeros(width), np.eye(width)
    for l in range(levels):
        front = chain @ g(l, "restore_w")
        tables.append((front @ g(l, "dqhead_w") @ g(l, "codebook").T).T)
        const = const + front @ g(l, "dqhead_b") + chain @ g(l, "restore_b")
        if l < levels - 1:
            const = const + front @ g(l, "side_b")
            chain = front @ g(l, "side_w")
    return np.ascontiguousarray(np.stack(tables), dtype=np.float32), np.ascontiguousarray(const, dtype=np.float32)


def collapse_encoder_f64(state: Dict[str, np.ndarray], levels: int):
    """The float64 algebra of ``collapse_encoder``: (G [levels*kc, 256], g [levels*kc], {(l, j): T_lj [kc_j][kc_l]}) with
    ``dist_l[k] - |q_l|^2 = G_l[k] . x_1 + g_l[k] + sum_{j<l} T_lj[code_j][k]`` on the shared feature x_1 (also the candidate stage of the
    two-stage exact encode, encode_two_stage.py)."""
    g = lambda l, n: state[f"codebook/{l}/{n}"].astype(np.float64)
    kc = int(state["codebook/0/codebook"].shape[0])
    front, shift = np.eye(256), np.zeros(256)          # x_l = front @ x_1 + shift - sum_j back[j] @ C_j[code_j]
    back = []                                          # per earlier level j: the matrix that carries its subtracted codeword to x_l
    G, gb, tables = [], [], {}
    for l in range(levels):
        Ws, bs, Wq, bq, Cb = g(l, "stage_w"), g(l, "stage_b"), g(l, "qhead_w"), g(l, "qhead_b"), g(l, "codebook")
        Gp = -2.0 * Cb @ Wq @ Ws                       # on x_l
        gp = (Cb * Cb).sum(1) - 2.0 * Cb @ (Wq @ bs + bq)
        G.append(Gp @ front)
        gb.append(Gp @ shift + gp)
        for j, Bj in enumerate(back):
            tables[(l, j)] = -(Gp @ Bj @ g(j, "codebook").T).T          # [kc_j][kc_l]
        if l < levels - 1:
            A = g(l, "lhead_w") @ Ws
            d = g(l, "lhead_w") @ bs + g(l, "lhead_b")
            front, shift = A @ front, A @ shift + d
            back = [A @ Bj for Bj in back] + [np.eye(256)]
    return np.concatenate(G), np.concatenate(gb), tables                # [L*kc, 256], [L*kc]


def collapse_encoder(state: Dict[str, np.ndarray], levels: int, in_delta: float, in_zx: int):
    """UMGMQuantizer.encode (codebook.py:330-337 -> :231-239 -> :106-131) with its affine heads multiplied out in float64 -- the operands
    of the OPT-IN ``qv2x_codebook_encode_collapsed_f32`` (not the parity path: the argmin may differ where the two best distances are
    within fp32 rounding error of each other).  With z = stage(x), q = qhead(z), x' = lhead(z) - C[code]:

        dist_l[k] - |q_l|^2 = |C_l[k]|^2 - 2 C_l[k] . q_l = G_l[k] . x_1 + g_l[k] + sum_{j<l} T_lj[code_j][k]

    Returns (g_packed f32 [L*kc/32][128][64], bias f32 [L*kc], tables f32 [L(L-1)/2][kc][kc]); the input dequantization
    x_1 = in_delta * (code - in_zx) is folded in: the kernel multiplies by the uint8 code itself."""
    Gall, gall, tables = collapse_encoder_f64(state, levels)
    kc = Gall.shape[0] // levels
    bias = gall + in_delta * (0.0 - in_zx) * Gall.sum(1)
    Gs = in_delta * Gall
    nct = levels * kc // 32
    lane = np.arange(64)
    col = (np.arange(nct)[:, None, None] * 32 + (lane & 31)[None, None, :])             # [nct, 1, 64]
    k = (2 * np.arange(128)[None, :, None] + (lane >> 5)[None, None, :])               # [1, 128, 64]
    packed = Gs[col, k]
    tab = np.stack([tables[(l, j)] for l in range(levels) for j in range(l)]) if levels > 1 else np.zeros((1, kc, kc))
    return (np.ascontiguousarray(packed, dtype=np.float32), np.ascontiguousarray(bias, dtype=np.float32), np.ascontiguousarray(tab, dtype=np.float32))


def _pack_k4p(w: np.ndarray) -> np.ndarray:
    """As ``_pack_k4`` but the four k of a group are stored (k0, k2, k1, k3): the half-wave feeding MFMA k-parity p
    reads one contiguous float2 = (k_p, k_{p+2}) (codebook_encode.hip)."""
    return np.ascontiguousarray(_pack_k4(w)[:, :, [0, 2, 1, 3]])


def _pack_wave(w: np.ndarray) -> np.ndarray:
    """[J, 256] row-major -> [J/64 tile pairs][32 groups][2 tiles][64 lanes][4] float32 (J zero-padded to a multiple of 64), the A-operand
    order of codebook_encode_wave.hip: lane ``32 h + c`` of group ``g`` of tile ``t`` of pair ``P`` holds ``w[64 P + 32 t + c, 8 g + 2 s + h]``
    for the four MFMA steps s."""
    j, k = w.shape
    assert k == 256
    if j % 64:
        w = np.concatenate([w, np.zeros((64 - j % 64, k), w.dtype)])
    return np.ascontiguousarray(w.reshape(-1, 2, 32, 32, 4, 2).transpose(0, 3, 1, 5, 2, 4), dtype=np.float32)


ENC_WAVE_PAD = 16 * 256          # floats behind a level blob's wave section (codebook_encode.h)


def _pack_wave_seg(cb: np.ndarray, segs: int) -> np.ndarray:
    """The codebook stream of the wave form for seg_num = 2 | 4 (codebook_encode_wave.hip, SEGS > 1): only the DIAGONAL blocks of the extended
    codebook [segs * kc][256] -- a tile pair is code tile ``P`` (32 codes) of two segments, ``32 / segs`` groups of eight dims long:
    [segment pair][kc / 32 tiles][32 / segs groups][2 segments][64 lanes][4], lane ``32 h + c`` of group ``g`` of segment ``seg`` of tile ``P`` holding
    ``cb[seg * kc + 32 P + c, (256 / segs) * seg + 8 g + 2 s + h]`` for the four MFMA steps s."""
    ke, k = cb.shape
    kc, d = ke // segs, 256 // segs
    assert k == 256 and segs in (2, 4) and kc % 32 == 0
    blocks = np.stack([cb[sg * kc:(sg + 1) * kc, sg * d:(sg + 1) * d] for sg in range(segs)])          # [seg][kc][d]
    b = blocks.reshape(segs // 2, 2, kc // 32, 32, d // 8, 4, 2)                                        # [pair][t][P][c][g][s][h]
    return np.ascontiguousarray(b.transpose(0, 2, 4, 1, 6, 3, 5), dtype=np.float32)                     # [pair][P][g][t][h][c][s]


def wave_section(stage_w, qhead_w, lhead_w, cb, segs: int = 1) -> np.ndarray:
    """The second half of a level blob (include/qv2x.h): stage | qhead | codebook | lhead in A-operand order -- one linear stream.  With
    ``segs`` > 1 the codebook part holds the diagonal blocks only (1 / segs of the dense stream); the section keeps its stated size."""
    cbs = _pack_wave(cb) if segs == 1 else _pack_wave_seg(cb, segs)
    sec = np.concatenate([_pack_wave(stage_w).reshape(-1), _pack_wave(qhead_w).reshape(-1), cbs.reshape(-1), _pack_wave(lhead_w).reshape(-1)])
    full = 3 * 65536 + (cb.shape[0] + 63) // 64 * 64 * 256
    return np.concatenate([sec, np.zeros(full - sec.size + ENC_WAVE_PAD, np.float32)])


class _ConvLayer:
    """Device-side constants of one 3x3 QuantModule convolution."""

    def __init__(self, state, name, in_groups, stride, dev, pad_cin=0, pad_cout=0):
        """``pad_cin`` / ``pad_cout``: widen a narrow layer (the 16-channel NaiveCompressor bottleneck) to the kernels' 64-channel
        granularity.  Extra input channels get the weight code zw[co] (so (w - zw) = 0 whatever they hold), extra output channels
        a zero filter with zero bias (they quantize to the code of 0.0 and are never read with a non-zero weight)."""
        code = state[name + "/w_code"]                              # [Cout, Cin, 3, 3] uint8
        dw = state[name + "/w_delta"].astype(np.float32)
        zw = state[name + "/w_zp"].astype(np.int64)
        bias_np = state[name + "/bias"].astype(np.float32)
        if pad_cin > code.shape[1]:
            fill = np.broadcast_to(np.clip(zw, 0, 255).astype(np.uint8)[:, None, None, None], (code.shape[0], pad_cin - code.shape[1], 3, 3))
            code = np.concatenate([code, fill], axis=1)
        if pad_cout > code.shape[0]:
            extra = pad_cout - code.shape[0]
            code = np.concatenate([code, np.full((extra,) + code.shape[1:], 128, np.uint8)])
            dw, zw = np.concatenate([dw, np.ones(extra, np.float32)]), np.concatenate([zw, np.full(extra, 128, np.int64)])
            bias_np = np.concatenate([bias_np, np.zeros(extra, np.float32)])
        cout = code.shape[0]
        ws = code.astype(np.int64) - 128
        aw = 128 - zw
        parts, corr, scale = [], [], []
        for (c0, c, dx, zx) in in_groups:
            blk = ws[:, c0:c0 + c].transpose(0, 2, 3, 1).reshape(cout, -1)      # [Cout][3][3][c]
            parts.append(blk)
            ax = 128 - int(zx)
            corr.append(ax * blk.sum(axis=1) + blk.shape[1] * ax * aw)
            scale.append(np.float32(dx) * dw)
        self.name, self.stride, self.cout = name, stride, cout
        self.groups = [(int(c0), int(c), int(zx)) for (c0, c, _, zx) in in_groups]
        self.w = _dev(np.concatenate(parts, axis=1).astype(np.int8), dev)
        self.w_wide = None                                              # tiled copy for qv2x_conv3x3_i8_wide, made on first use
        self.scale = _dev(np.stack(scale).astype(np.float32), dev)
        self.corr = _dev(np.stack(corr).astype(np.int32), dev)
        self.aw = _dev(aw.astype(np.int32), dev)
        self.bias = _dev(bias_np, dev)
        self.out_q = (float(np.float32(state[name + "/a_delta"])), int(state[name + "/a_zp"]))
        assert np.abs(np.stack(corr)).max() < 2 ** 31


def launch_conv3x3(lib, layer: _ConvLayer, x, n, h, w, out, out_q=None, res_mode=0, res=None, res_q=(0.0, 128), out_ctotal=None, out_c0=0,
                   wide=True):
    """One 3x3 QuantModule convolution on codes: ``qv2x_conv3x3_i8``, its wide form where ``wide`` and the shape allow it, or ``_res`` with a
    fused residual end.  ``out_q``: the output quantizer (the layer's own by default); ``out_ctotal`` / ``out_c0``: the channel window of
    ``out`` the layer writes (all of it by default).  Shared by every engine."""
    out_q = layer.out_q if out_q is None else out_q
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin_total, d.stride, d.cout = n, h, w, x.shape[-1], layer.stride, layer.cout
    d.ngroups = len(layer.groups)
    for i, (c0, c, zx) in enumerate(layer.groups):
        d.group_c0[i], d.group_c[i], d.group_zx[i] = c0, c, zx
    d.out_ctotal = out.shape[-1] if out_ctotal is None else out_ctotal
    d.out_c0, d.relu = out_c0, 1
    d.out_delta, d.out_zp = out_q[0], float(out_q[1])
    st = L.current_stream()
    if res_mode:
        L.check(lib.qv2x_conv3x3_i8_res(C.byref(d), L.ptr(x), L.ptr(layer.w), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw),
                                        L.ptr(layer.bias), res_mode, L.ptr(res), int(res_q[1]), float(res_q[0]), L.ptr(out), st), layer.name)
        return
    if wide and lib.qv2x_conv3x3_i8_wide_ok(C.byref(d)):
        if layer.w_wide is None:                                        # one-off re-tiling of the weights (not capturable)
            layer.w_wide = torch.empty_like(layer.w)
            L.check(lib.qv2x_conv3x3_i8_pack_wide(C.byref(d), L.ptr(layer.w), L.ptr(layer.w_wide), st), layer.name)
        L.check(lib.qv2x_conv3x3_i8_wide(C.byref(d), L.ptr(x), L.ptr(layer.w_wide), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw),
                                         L.ptr(layer.bias), L.ptr(out), st), layer.name)
        return
    L.check(lib.qv2x_conv3x3_i8(C.byref(d), L.ptr(x), L.ptr(layer.w), L.ptr(layer.scale), L.ptr(layer.corr), L.ptr(layer.aw),
                                L.ptr(layer.bias), L.ptr(out), st), layer.name)


class _ChainLayers:
    """Consecutive 64 -> 64 channel conv layers of one backbone level as ONE launch (qv2x_conv3x3_i8_chain64): the B
    fragments of v_mfma_i32_32x32x32_i8 in load order ``[layer][cout/32][tap][cin/32][lane][16]`` and the per-layer
    epilogue constants stacked ``[layer][64]``."""
    MAX_DEPTH = 4

    @staticmethod
    def eligible(convs) -> bool:
        return (1 <= len(convs) <= _ChainLayers.MAX_DEPTH and all(c.cout == 64 and len(c.groups) == 1 and c.groups[0][1] == 64 for c in convs)
                and all(c.stride == 1 for c in convs[1:]))

    def __init__(self, convs, dev):
        self.convs = convs
        self.name = convs[-1].name                                    # the tensor it produces is the last layer's output
        packed = []
        for c in convs:
            w = c.w.cpu().numpy().reshape(2, 32, 9, 2, 2, 16)          # [cout/32][n][tap][ks][half][16]
            packed.append(w.transpose(0, 2, 3, 4, 1, 5))               # [cout/32][tap][ks][half][n][16]: lane = 32 * half + n
        self.w = _dev(np.stack(packed).astype(np.int8), dev)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).contiguous()
        self.scale, self.corr = cat([c.scale for c in convs]), cat([c.corr for c in convs])
        self.aw, self.bias = cat([c.aw for c in convs]), cat([c.bias for c in convs])
        self.stride0 = convs[0].stride
        self.out_q = convs[-1].out_q


class _DeconvLayer:
    def __init__(self, state, name, in_q, dev):
        code = state[name + "/w_code"].astype(np.float32)            # [Cin, Cout, s, s]; scales per C_in (dim 0)
        dw = state[name + "/w_delta"].astype(np.float32).reshape(-1, 1, 1, 1)
        zw = state[name + "/w_zp"].astype(np.float32).reshape(-1, 1, 1, 1)
        wdeq = ((code - zw) * dw).astype(np.float32)
        cin, cout, s, _ = wdeq.shape
        cols = wdeq.transpose(0, 2, 3, 1).reshape(cin, s * s * cout)              # col = (i*s + j)*Cout + co
        self.w = _dev(_pack_k4p(cols.T), dev)
        self.bias = _dev(state[name + "/bias"].astype(np.float32), dev)
        self.name, self.cin, self.cout, self.s, self.in_q = name, cin, cout, s, in_q
        self.out_q = (float(np.float32(state[name + "/a_delta"])), int(state[name + "/a_zp"]))


class _Heads:
    """cls | reg | dir stacked on the channel axis, each with its own output quantizer."""

    def __init__(self, state, suffix, dev):
        ws, bs, das, zas = [], [], [], []
        for h in _HEADS:
            n = h + suffix
            code = state[n + "/w_code"].astype(np.float32).reshape(state[n + "/w_code"].shape[0], -1)
            w = ((code - state[n + "/w_zp"].astype(np.float32)[:, None]) * state[n + "/w_delta"].astype(np.float32)[:, None])
            ws.append(w.astype(np.float32))
            bs.append(state[n + "/bias"].astype(np.float32))
            off = bool(state[n + "/a_off"])
            das.append(np.full(w.shape[0], -1.0 if off else float(np.float32(state[n + "/a_delta"])), np.float32))
            zas.append(np.full(w.shape[0], 0.0 if off else float(state[n + "/a_zp"]), np.float32))   # (a disabled quantizer's parameters are never read)
        self._stack(ws, bs, das, zas, dev)

    @classmethod
    def folded_fp32(cls, state, suffix, dev):
        """the heads of an un-quantized model (``<head>/w`` [C, 256], ``<head>/bias``): every output quantizer off"""
        hd = cls.__new__(cls)
        ws = [state[h + suffix + "/w"] for h in _HEADS]
        hd._stack(ws, [state[h + suffix + "/bias"] for h in _HEADS], [np.full(w.shape[0], -1.0, np.float32) for w in ws],
                  [np.zeros(w.shape[0], np.float32) for w in ws], dev)
        return hd

    def _stack(self, ws, bs, das, zas, dev):
        self.splits = [w.shape[0] for w in ws]
        self.cout = sum(self.splits)
        self.cout_pad = (self.cout + 31) // 32 * 32
        if self.cout_pad > 96:
            raise NotImplementedError("heads: at most 96 stacked output channels")
        pad = self.cout_pad - self.cout
        w = np.concatenate(ws + [np.zeros((pad, 256), np.float32)])
        self.w = _dev(_pack_k4p(w), dev)
        self.bias = _dev(np.concatenate(bs + [np.zeros(pad, np.float32)]), dev)
        self.da = _dev(np.concatenate(das + [np.full(pad, -1.0, np.float32)]), dev)
        self.za = _dev(np.concatenate(zas + [np.zeros(pad, np.float32)]), dev)
        self._w_np, self._b_np = np.concatenate(ws).astype(np.float64), np.concatenate(bs).astype(np.float64)
        self.da_np = np.ascontiguousarray(np.concatenate(das))         # host copy: which channels have an output quantizer (the u8 band wire)
        self.lut_tables = None

    def collapse_over_decode(self, lut: np.ndarray, lut_bias: np.ndarray, dev):
        """head(decode(codes)) = b' + sum_l T'_l[code_l]: decode is a sum of table rows (``decode_tables``), the head is linear.
        float64 on the host -> ``(tables f32 [L][kc][cout], bias f32 [cout])`` on the device (qv2x_single_heads_lut_f32)."""
        t = np.einsum("lkd,cd->lkc", lut.astype(np.float64), self._w_np)
        b = lut_bias.astype(np.float64) @ self._w_np.T + self._b_np
        self.lut_tables = (_dev(t.astype(np.float32), dev), _dev(b.astype(np.float32), dev))


# ---- shared by every deployed engine ------------------------------------------------------------------------------------------------
def scene_layout(data_dict: dict, n_total: int):
    """``(pairwise f64 contiguous, agents per scene)`` of one model call: ``record_len`` is read on the host (its values shape the launch
    list), so a device ``record_len`` is refused during HIP-graph capture (``capture_forward`` hands the forward a CPU copy)."""
    pairwise = data_dict["pairwise_t_matrix"]
    if pairwise.dtype != torch.float64 or not pairwise.is_contiguous():
        pairwise = pairwise.to(torch.float64).contiguous()
    if pairwise.shape[0] == 1:
        return pairwise, [n_total]
    rl = data_dict["record_len"]
    if isinstance(rl, torch.Tensor) and rl.is_cuda and torch.cuda.is_current_stream_capturing():
        raise ValueError("record_len on the GPU cannot be read during HIP-graph capture: pass a CPU tensor")
    return pairwise, [int(v) for v in (rl.tolist() if isinstance(rl, torch.Tensor) else rl)]


def split_heads(preds: torch.Tensor, splits, suffix: str = "") -> dict:
    """cls | reg | dir as views of the stacked predictions ``preds`` [n, C, H, W] (plus ``preds_tensor`` itself without a suffix)."""
    c, r, _ = splits
    out = {"cls_preds" + suffix: preds[:, :c], "reg_preds" + suffix: preds[:, c:c + r], "dir_preds" + suffix: preds[:, c + r:]}
    if not suffix:
        out["preds_tensor"] = preds
    return out


def capture_call(call):
    """Capture one ``call()`` (no arguments) into a HIP graph (torch.cuda.CUDAGraph on ROCm) after two warm-up calls on a side stream.
    The returned callable replays it and returns what ``call`` returned; ``replay.graph`` is the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()

    def replay():
        graph.replay()
        return out
    replay.graph = graph
    return replay


def capture_forward(module: nn.Module, data_dict: dict):
    """Capture one ``module.forward(data_dict)`` into a HIP graph (``capture_call``).  The returned callable replays it on the same input
    tensors (refresh their contents in place between replays) and returns the same output dict; ``replay.graph`` is the graph.  A device
    ``record_len`` is replaced by a CPU copy: its values shape the launch list."""
    rl = data_dict.get("record_len")
    if data_dict["pairwise_t_matrix"].shape[0] > 1 and isinstance(rl, torch.Tensor) and rl.is_cuda:
        data_dict = dict(data_dict, record_len=rl.cpu())
    return capture_call(lambda: module.forward(data_dict))


def assemble_heter_codes(owner: str, engines: dict, slot_cache: dict, agents: list, data_dict: dict, encode, taps: Optional[dict]) -> torch.Tensor:
    """The code planes u8 [levels, n * H*W] of a heterogeneous scene in agent order: every modality's engine encodes its own agents
    (``encode(engine, inputs, k, taps)``) and ``index_copy_`` puts them in their slots.  The slot indices are an H2D copy: built once per
    agent layout in ``slot_cache``, refused during HIP-graph capture (``capture_forward`` runs eager forwards first)."""
    unknown = sorted(set(agents) - set(engines))
    if unknown:
        raise NotImplementedError(f"{owner}: no engine for modality {unknown}")
    slots = slot_cache.get(tuple(agents))
    if slots is None:
        if torch.cuda.is_current_stream_capturing():
            raise L.Qv2xError(f"{owner}: agent layout {agents} is new and the stream is capturing -- its slot indices are an H2D copy; "
                              "run one eager forward of this layout first (capture does)")
        slots = {m: torch.as_tensor([i for i, a in enumerate(agents) if a == m], dtype=torch.int64, device=e.dev) for m, e in engines.items()}
        slot_cache[tuple(agents)] = slots
    e = next(iter(engines.values()))                                 # (every modality's feature map and code planes are the same size)
    n_total, hw, lv = len(agents), e.fh * e.fw, e.levels
    enc = torch.empty((lv, n_total * hw), dtype=torch.uint8, device=e.dev)
    for m, eng in engines.items():
        k = int(slots[m].numel())
        if not k:
            continue
        mt = {} if taps is not None else None
        codes = encode(eng, data_dict["inputs_" + m], k, mt).view(lv, k, hw)
        enc.view(lv, n_total, hw).index_copy_(1, slots[m], codes)                                # agent order (a copy, no arithmetic)
        if taps is not None:
            taps["modality/" + m] = mt
    return enc


def pillar_inputs(inputs: dict, pfn: bool = True):
    """``(voxel_features, voxel_coords i32, voxel_num_points i32)`` of one ``inputs_m1`` dict, contiguous, as the PFN kernels take them
    (``pfn=False``: the SECOND encoder, which states its own voxel shape)."""
    vf = inputs["voxel_features"].contiguous()
    co = inputs["voxel_coords"].to(torch.int32).contiguous()
    npnt = inputs["voxel_num_points"].to(torch.int32).contiguous()
    if pfn and (vf.dtype != torch.float32 or vf.dim() != 3 or tuple(vf.shape[1:]) != (32, 4)):
        raise ValueError("voxel_features must be float32 [M, 32, 4]")
    return vf, co, npnt


def pfn_params(state: Dict[str, np.ndarray]):
    """a1 of a W8A8 state: ``(L.PfnParams, (delta, zero point) of the canvas)`` -- the host struct qv2x_pfn_scatter_i8 takes by value."""
    s, n = state, "encoder_m1.pillar_vfe.pfn_layers.0.linear"
    wq = ((s[n + "/w_code"].astype(np.float32) - s[n + "/w_zp"].astype(np.float32)[:, None])
          * s[n + "/w_delta"].astype(np.float32)[:, None]).astype(np.float32)
    if wq.shape != (64, 10):
        raise NotImplementedError("deployed PFN expects Linear(10 -> 64)")
    p = L.PfnParams()
    p.w[:] = wq.reshape(-1).tolist()
    p.b[:] = s[n + "/bias"].astype(np.float32).tolist()
    p.d1, p.z1 = float(np.float32(s[n + "/a_delta"])), float(s[n + "/a_zp"])
    p.d2, p.z2 = float(np.float32(s["pfn/a2_delta"])), float(s["pfn/a2_zp"])
    p.vox[:] = [float(np.float32(v)) for v in s["meta/voxel"]]
    p.off[:] = [float(np.float32(v)) for v in s["meta/offset"]]
    return p, (p.d2, int(p.z2))


def level_blob_host(state: Dict[str, np.ndarray], l: int, ke: int, D: int, segs: int):
    """One codebook level's heads as the flat fp32 blob the encode kernels read (codebook_encode.h, include/qv2x.h) ->
    ``(flat, cb_off, c2_off)``: the offsets, in floats, of the row-major codebook and of its ``c2`` slot (``ke`` zeros; filled on the device).
    ``D == 64`` is the native 64-wide layout (qv2x_codebook_encode64_f32); every other ``D <= 256`` is zero-padded to the 256-wide one, which
    carries the wave form's section too (every extra term of every fma chain is 0 * 0 and the padded |.|^2 chains are exactly 0, so the
    codes equal a native evaluation bit for bit).  The last level (no ``lhead_w``) has an all-zero lhead."""
    W = 64 if D == 64 else 256
    last = f"codebook/{l}/lhead_w" not in state

    def padded(n, *shape):
        out = np.zeros(shape, np.float32)
        if not (last and n.startswith("lhead")):
            a = state[f"codebook/{l}/{n}"]
            out[tuple(slice(0, k) for k in a.shape)] = a
        return out
    stage, qhead, lhead, cb = padded("stage_w", W, W), padded("qhead_w", W, W), padded("lhead_w", W, W), padded("codebook", ke, W)
    parts = [_pack_k4p(stage), padded("stage_b", W), _pack_k4p(qhead), padded("qhead_b", W), _pack_k4p(lhead), padded("lhead_b", W),
             _pack_k4p(cb), cb, np.zeros(ke, np.float32)]
    flat = np.concatenate([p.reshape(-1) for p in parts])
    c2_off = flat.size - ke                                          # the workgroup form's section ends with c2
    if W == 256:
        flat = np.concatenate([flat, wave_section(stage, qhead, lhead, cb, segs)])
    return flat, c2_off - ke * W, c2_off


def level_blob(lib, state: Dict[str, np.ndarray], l: int, ke: int, D: int, segs: int, dev) -> torch.Tensor:
    """``level_blob_host`` on the device, its ``c2`` slot filled by the matching qv2x_codebook[64]_c2_f32"""
    flat, cb_off, c2_off = level_blob_host(state, l, ke, D, segs)
    floats, c2fn, name = ((lib.qv2x_codebook64_level_floats, lib.qv2x_codebook64_c2_f32, "qv2x_codebook64_c2_f32") if D == 64
                          else (lib.qv2x_codebook_level_floats, lib.qv2x_codebook_c2_f32, "qv2x_codebook_c2_f32"))
    assert flat.size == floats(ke)
    blob = _dev(flat, dev)
    L.check(c2fn(C.c_void_p(blob.data_ptr() + 4 * cb_off), ke, C.c_void_p(blob.data_ptr() + 4 * c2_off), L.current_stream()), name)
    return blob


class CodebookConstants(NamedTuple):
    enc_levels: int                     # residual levels: what the encode kernels count
    segs: int
    levels: int                         # code planes = enc_levels * segs: what everything downstream of the encode counts
    ke: int                             # rows of the extended codebook = segs * kc
    kc: int
    D: int
    lut_host: np.ndarray                # the decode table [levels][kc][D] and its bias [D]
    lut_bias_host: np.ndarray
    lut: torch.Tensor
    lut_bias: torch.Tensor
    level_blobs: List[torch.Tensor]
    level_ptrs: object                  # (C.c_void_p * enc_levels) of the blobs


def codebook_constants(lib, state: Dict[str, np.ndarray], dev, refuse) -> CodebookConstants:
    """a6 / a7 of every engine.  seg_num (m) > 1: the state holds the EXTENDED codebook [m * kc][D] (ptq_state.extended_codebook).  Downstream
    of the encode everything counts code PLANES: ``levels`` = residual levels * m (the wire's [levels][agents][H*W] planes and the decode
    table [levels][kc][D], which is the per-level table over the extended rows read plane by plane); the encode kernels get the true level
    count ``enc_levels`` and ``segs``.  ``refuse(ke, kc, D, segs)`` raises for what the calling engine's kernels do not take, before any upload."""
    s = state
    enc_levels, segs = int(s["meta/codebook_levels"]), int(s.get("meta/codebook_segs", 1))
    ke, D = (int(v) for v in s["codebook/0/codebook"].shape)
    kc, levels = ke // segs, enc_levels * segs
    refuse(ke, kc, D, segs)
    lut, lut_bias = decode_tables(s, enc_levels, D)
    lut = lut.reshape(levels, kc, D)
    blobs = [level_blob(lib, s, l, ke, D, segs, dev) for l in range(enc_levels)]
    return CodebookConstants(enc_levels, segs, levels, ke, kc, D, lut, lut_bias, _dev(lut, dev), _dev(lut_bias, dev), blobs,
                             (C.c_void_p * enc_levels)(*[b.data_ptr() for b in blobs]))


def _pairwise_from_poses(self, gathered: torch.Tensor, world: int, agent_stride: int, pose_offset: int, max_cav: int, out: torch.Tensor):
    """pairwise f64 [max_cav, max_cav, 4, 4] from the poses inside the gathered payloads (qv2x_pairwise_from_poses_f64): the method of that
    name of every engine with the multi-GPU stage interface (it reads ``self.lib`` only)."""
    L.check(self.lib.qv2x_pairwise_from_poses_f64(L.ptr(gathered), world, agent_stride, pose_offset, max_cav, L.ptr(out),
                                                  L.current_stream()), "qv2x_pairwise_from_poses_f64")


class DeployedPostStage(nn.Module):
    """What every engine of the AttFusion / MaxFusion network shares: the codebook constants and the POST stage a7-a11 on the agents' wire
    data (decode + warp + fusion, the heads, the ``*_single`` heads), the reference's model contract around it (``forward`` = ``encode_agents``
    + ``finish``), HIP-graph capture and the multi-GPU stage interface (dist.py).  The code planes are the boundary (``DeployedHeterModel``).

    An agent stage (a1-a6: ``DeployedModel`` in W8A8, ``DeployedFp32Model`` in fp32) derives from it, calls ``_set_heads`` and provides
      ``_workspace(n)``               the buffers of ``n`` agents; the first one sets the feature map's size ``fh``, ``fw``
      ``heads``, ``heads_single``     (through ``_set_heads``)
      ``encode_agents(inputs, n, taps)``  the wire data of ``n`` agents: code planes u8 [levels, n, H*W], or the shrinker output without a codebook
      ``encode_into(inputs, frames, codes_out)``  the same for ``frames`` frames of one agent, into the caller's payload
      ``_shared_features(enc, n)``    without a codebook: that shrinker output as fp32 rows [n, H*W, 256]"""
    # a7-a11 as ONE launch (qv2x_fuse_heads_batch_f32: the fused map stays in LDS) from this many 32-cell tiles on -- four rounds of the
    # chip's 1280 resident workgroups; below it (one frame: a single round) the two launches are faster.  Measured at a batch of 32
    # V2X-Real frames: round 4 (the agent-by-agent walk inside the tile kernel, profiles/r04_fuse_heads_times.log): single-agent scenes 1160
    # against 1224 us, scenes of four agents 780 against 632 us -- only scenes of ONE agent took it.  Round 5 (the batched round trips of
    # fuse_att.h:fuse_cell_b3 inside it, tools/bench_fuse.py 32 ring): scenes of two agents 1421 against 877 + 635 us, of four 2010 against
    # 1428 + 629; of five / eight (the eight-agent instantiation: 140 registers) 2889 against 2450 / 3790 against 3156 -- up to FOUR agents.
    fuse_heads_min_tiles = 4 * 1280
    fuse_heads_max_agents = 4           # (with three code planes: the batched form needs them; otherwise scenes of one agent -- _one_launch_agents)
    # scenes of ONE agent: every head by table look-up on the agent's own codes (qv2x_table_heads_f32; see _set_heads)
    single_agent_tables = True
    band_one_launch = None              # the band path's form: None = by the agent count (as _post_form); True / False force it (tests, tools/bench_band_post.py)
    _band_rows = None

    def __init__(self, state: Dict[str, np.ndarray], device, emit_single_preds: Optional[bool]):
        super().__init__()
        self.lib = L.load()                      # raises if libqv2x.so is absent: no fallback
        if not torch.cuda.is_available():
            raise L.Qv2xError(f"{type(self).__name__} needs an MI355X (torch.cuda.is_available() is False)")
        self.state, self.dev = state, torch.device(device)
        s, dev = state, self.dev
        if str(s.get("meta/fusion_method", "att")) not in ("att", "max"):
            raise NotImplementedError(f"deployed path: fusion_method {s['meta/fusion_method']!r} ('att' = AttFusion and 'max' = MaxFusion are built here)")
        self.fusion = 1 if str(s.get("meta/fusion_method", "att")) == "max" else 0
        self.nx, self.ny, _ = (int(v) for v in s["meta/grid"])
        self.hm, self.wm = (float(v) for v in s["meta/HW_metres"])
        self.ratio = float(s["meta/discrete_ratio"])
        self.layer_nums = [int(v) for v in s["meta/layer_nums"]]
        self.strides = [int(v) for v in s["meta/layer_strides"]]
        self.ups = [int(v) for v in s["meta/upsample_strides"]]
        self.has_codebook = bool(s["meta/has_codebook"])
        self.emit_single = bool(s["meta/supervise_single"]) if emit_single_preds is None else bool(emit_single_preds)
        # ---- a6 / a7: codebook -----------------------------------------------------------------------------
        self._lut_host = (None, None)
        if self.has_codebook:
            c = codebook_constants(self.lib, s, dev, self._refuse_codebook)
            self.enc_levels, self.segs, self.levels, self.ke, self.kc = c.enc_levels, c.segs, c.levels, c.ke, c.kc
            self.lut, self.lut_bias, self.level_blobs, self.level_ptrs = c.lut, c.lut_bias, c.level_blobs, c.level_ptrs
            self._lut_host = (c.lut_host, c.lut_bias_host)             # (for the head tables of ``_set_heads``)

    @staticmethod
    def _refuse_codebook(ke, kc, D, segs):
        if ke > 512 or kc > 256:
            raise NotImplementedError(f"deployed codebook path: seg_num * dict_size <= 512, dict_size <= 256 (got {segs} x {kc}): "
                                      "the encode kernels' tile budget (qv2x_codebook_encode_f32)")
        if D != 256:
            raise NotImplementedError(f"deployed codebook path: a codebook as wide as the 256-channel shared feature (got {D})")

    def _set_heads(self, heads: _Heads, heads_single: Optional[_Heads], tables: bool):
        """``heads`` / ``heads_single`` and how they run.  ``tables``: heads by table look-up where a table fits (the W8A8 engine).  The
        fp32 engine passes False: no head tables, ``table_heads`` None and ``single_by_tables`` / ``single_by_global_tables`` False -- its
        ``*_single`` heads keep the GEMM forms (qv2x_heads_pair_f32 / qv2x_decode_heads_f32) and single-agent scenes the general path."""
        self.heads, self.heads_single = heads, heads_single
        self.table_heads, self.single_by_tables, self.single_by_global_tables = None, False, False
        if not (tables and self.has_codebook):
            return
        (lut, lut_bias), dev = self._lut_host, self.dev
        # the *_single heads see one agent's own decoded feature: with the codebook that is three table rows per cell -- no GEMM
        self.single_by_tables = (self.heads_single is not None and self.levels <= 4
                                 and self.levels * self.kc * self.heads_single.cout * 4 <= 60 * 1024)
        # (round 5: tables past that kernel's LDS -- six planes x 256 rows -- through qv2x_table_heads_f32's global-memory form)
        # (the C entry's global-memory form: c0 + c1 a multiple of 4 and <= 128, 16-byte aligned arrays -- torch allocations are 256-byte
        #  aligned; a wider single head keeps qv2x_decode_heads_f32, which handles it: ADVICE r5)
        self.single_by_global_tables = (not self.single_by_tables and self.heads_single is not None and self.levels <= 16
                                        and self.heads_single.cout % 4 == 0 and self.heads_single.cout <= 128)
        if self.single_by_tables or self.single_by_global_tables:
            self.heads_single.collapse_over_decode(lut, lut_bias, dev)
        # single-agent scenes (round 4): AttFusion over one agent is the identity, so EVERY head is a table look-up on the agent's own codes
        # (qv2x_table_heads_f32): cls | reg | dir [+ the *_single heads] stacked, tables = decode table x head weights in float64
        # (AttFusion or MaxFusion: either is the identity on one agent)
        sets = [self.heads] + ([self.heads_single] if self.heads_single is not None else [])
        ct = sum(h.cout for h in sets)
        ct4 = (ct + 3) // 4 * 4
        st = ct4 if (ct4 // 4) % 2 else ct4 + 4
        in_lds = self.levels <= 4 and (self.levels * self.kc * st + 4 * ct4) * 4 <= 160 * 1024
        # (round 5: tables past the LDS -- seg_num 2 x dict_size 256: six planes, 565 KB -- stay in global memory, qv2x.h)
        if in_lds or (self.levels <= 16 and ct % 4 == 0 and ct <= 128):
            t = np.concatenate([np.einsum("lkd,cd->lkc", lut.astype(np.float64), h._w_np) for h in sets], axis=2)
            b = np.concatenate([lut_bias.astype(np.float64) @ h._w_np.T + h._b_np for h in sets])
            cat = lambda name: torch.cat([getattr(h, name)[:h.cout] for h in sets]).contiguous()
            self.table_heads = (_dev(t.astype(np.float32), dev), _dev(b.astype(np.float32), dev), cat("da"), cat("za"),
                                self.heads.cout, self.heads_single.cout if self.heads_single is not None else 0)

    def _run_heads(self, hd: _Heads, rows, nb, hw):
        out = torch.empty((nb, hd.cout, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        L.check(self.lib.qv2x_heads_f32(L.ptr(rows), nb * hw, hw, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias),
                                        L.ptr(hd.da), L.ptr(hd.za), L.ptr(out), L.current_stream()), "qv2x_heads_f32")
        return out

    # ---- stage interface of the multi-GPU driver (quantv2x_amd/dist.py) -----------------------------------------------------
    def wire_shape(self):
        """(levels, H*W) of one agent-frame's code planes -- the payload of the V2X link."""
        self._workspace(1)
        return self.levels, self.fh * self.fw

    pairwise_from_poses = _pairwise_from_poses

    def pairwise_frames_from_poses(self, gathered: torch.Tensor, world: int, agent_stride: int, pose_offset: int, frames: int, frame_stride: int,
                                   max_cav: int, out: torch.Tensor):
        """the same for ``frames`` scenes in one launch; ``out`` f64 [frames, max_cav, max_cav, 4, 4]"""
        L.check(self.lib.qv2x_pairwise_from_poses_batch_f64(L.ptr(gathered), world, agent_stride, pose_offset, frames, frame_stride, max_cav,
                                                            L.ptr(out), L.current_stream()), "qv2x_pairwise_from_poses_batch_f64")

    def fuse_frames_and_heads(self, gathered: torch.Tensor, agent_stride: int, level_stride: int, frame_stride: int, pairwise: torch.Tensor,
                              n_agents: int, ego: int, own_codes: Optional[torch.Tensor], frames: int) -> dict:
        """a7-a11 for ``frames`` scenes whose agents' code planes lie ``agent_stride`` bytes apart in ``gathered`` (frame f at
        ``+ f * frame_stride``); ``pairwise`` f64 [frames, L, L, 4, 4].  With ``own_codes`` (u8 [levels, frames, H*W]) the
        ``*_single`` heads of this rank's own agent run in the same launch as the heads on the fused maps."""
        # a world of one agent: the own code planes ARE the scene (pairwise here comes from qv2x_pairwise_from_poses_*: T[0][0] of a world of
        # one is the identity by construction, so the table look-up's contract holds without a read-back)
        lens = [n_agents] * frames
        form = self._post_form(lens, None, own_codes is not None and frame_stride == self.fh * self.fw)
        return self._post(form, L.ptr(gathered), agent_stride, level_stride, None, pairwise, [f * frame_stride for f in range(frames)], lens, ego,
                          own_codes, frames)

    # ---- the ego's post stage in row bands (dist.py: shard_post) -----------------------------------------------------------------
    def band_shape(self):
        """(cout, H, W) of the stacked cls | reg | dir predictions a band is cut from"""
        self._workspace(1)
        return self.heads.cout, self.fh, self.fw

    def head_wire_supported(self, wire: str) -> bool:
        """Can a band's predictions travel as ``wire``?  "f32" always; "u8" (the output quantizer's codes) iff every channel of the heads
        has an output quantizer."""
        if wire not in L.WIRES:
            raise ValueError(f"wire: one of {sorted(L.WIRES)}, got {wire!r}")
        return wire == "f32" or bool((self.heads.da_np > 0).all())

    def fuse_frames_and_heads_band(self, gathered: torch.Tensor, agent_stride: int, level_stride: int, frame_stride: int, pairwise: torch.Tensor,
                                   n_agents: int, ego: int, frames: int, y0: int, y1: int, out_slab: torch.Tensor, wire: str = "f32"):
        """a7-a11 of ``fuse_frames_and_heads`` for the rows ``[y0, y1)`` of the ego's map only, straight into ``out_slab`` (u8 bytes): the
        compact band ``[frames][cout][(y1 - y0) * W]`` as fp32 values (``wire="f32"``) or output-quantizer codes (``"u8"``).  Bit for bit the
        same cells as the whole-map call.  Never the single-agent table look-up (another fp32 association) and no ``*_single`` heads (they are
        not a function of the ego's map: ``single_preds``).  One launch per 64 frames up to ``_one_launch_agents()`` agents, else the fused
        rows of the band (a buffer kept per shape: nothing is allocated once warm) and the heads on them -- the whole-map selector's rule."""
        if not self.head_wire_supported(wire):
            raise L.Qv2xError("band wire 'u8': a head without an output quantizer has no codes to send")
        hd, n_cells, esz = self.heads, (y1 - y0) * self.fw, (1 if wire == "u8" else 4)
        if not 0 <= y0 <= y1 <= self.fh:
            raise ValueError(f"band rows [{y0}, {y1}) outside the map's {self.fh} rows")
        if out_slab.dtype != torch.uint8 or out_slab.numel() < frames * hd.cout * n_cells * esz:
            raise ValueError("out_slab: u8, at least frames * cout * band cells * element size bytes")
        if n_cells == 0:
            return
        one_launch = self.band_one_launch
        if one_launch is None:
            one_launch = frames * n_cells // 32 >= self.fuse_heads_min_tiles and n_agents <= self._one_launch_agents()
        rows = None
        if not one_launch:
            key = (frames, n_cells)
            if self._band_rows is None or self._band_rows[0] != key:
                self._band_rows = (key, torch.empty((frames, n_cells, 256), dtype=torch.float32, device=self.dev))
            rows = self._band_rows[1]
        base, st = out_slab.data_ptr(), L.current_stream()
        for s0, n, d, offs, cnts, lut, lb in self._scene_chunks(agent_stride, level_stride, pairwise, [f * frame_stride for f in range(frames)],
                                                                [n_agents] * frames, ego):
            out = C.c_void_p(base + s0 * hd.cout * n_cells * esz)
            if one_launch:
                L.check(self.lib.qv2x_fuse_heads_band(C.byref(d), n, offs, cnts, L.ptr(gathered), lut, lb, None, L.ptr(pairwise[s0]),
                                                      y0 * self.fw, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da),
                                                      L.ptr(hd.za), L.WIRES[wire], L.ptr(hd.da_np), out, None, st), "qv2x_fuse_heads_band")
            else:
                L.check(self.lib.qv2x_fuse_att_band_f32(C.byref(d), n, offs, cnts, L.ptr(gathered), lut, lb, None, L.ptr(pairwise[s0]),
                                                        y0 * self.fw, n_cells, L.ptr(rows[s0]), st), "qv2x_fuse_att_band_f32")
                L.check(self.lib.qv2x_heads_band(L.ptr(rows[s0]), n, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias),
                                                 L.ptr(hd.da), L.ptr(hd.za), L.WIRES[wire], L.ptr(hd.da_np), out, st), "qv2x_heads_band")

    def assemble_bands(self, gathered_slabs: torch.Tensor, world: int, frames: int, wire: str, out: torch.Tensor):
        """The gathered band slabs u8 ``[world, slab_bytes]`` -> ``out`` f32 ``[frames, cout, H, W]`` in one launch (qv2x_assemble_bands)."""
        hd = self.heads
        L.check(self.lib.qv2x_assemble_bands(L.ptr(gathered_slabs), world, gathered_slabs.shape[1], frames, hd.cout, self.fh, self.fw, L.WIRES[wire],
                                             L.ptr(hd.da), L.ptr(hd.za), L.ptr(out), L.current_stream()), "qv2x_assemble_bands")

    def band_output(self, preds: torch.Tensor, own_codes: Optional[torch.Tensor], frames: int) -> dict:
        """The model's output dict from the assembled predictions ``[frames, cout, H, W]``, plus the ``*_single`` heads of this rank's own
        agent on ``own_codes`` (u8 [levels, frames, H*W]) -- the keys of ``fuse_frames_and_heads``."""
        out = split_heads(preds, self.heads.splits)
        if own_codes is not None:
            out.update(self.single_preds(own_codes, frames))
        return out

    def decode_rows(self, codes, n_rows_total):
        """codes u8 [levels, R] -> fp32 [R, 256] (only needed for the *_single heads)."""
        out = torch.empty((n_rows_total, 256), dtype=torch.float32, device=self.dev)
        L.check(self.lib.qv2x_decode_lut_f32(L.ptr(codes), n_rows_total, self.levels, self.kc, L.ptr(self.lut),
                                             L.ptr(self.lut_bias), L.ptr(out), L.current_stream()), "qv2x_decode_lut_f32")
        return out

    def _fuse_desc(self, agent_stride, level_stride, pairwise_b, n, ego):
        d = L.FuseDesc()
        d.agents, d.h, d.w = n, self.fh, self.fw
        d.levels, d.kc = (self.levels, self.kc) if self.has_codebook else (1, 1)
        d.max_cav, d.ego = pairwise_b.shape[0], ego
        d.code_agent_stride, d.code_level_stride = agent_stride, level_stride
        d.h_metres, d.w_metres, d.discrete_ratio = self.hm, self.wm, self.ratio
        d.fusion = self.fusion
        return d

    def fuse(self, codes_ptr, agent_stride, level_stride, feats, pairwise_b, n, out, ego=0):
        """a7-a10 alone: the fused fp32 map [H*W, 256] into ``out`` (parity tests, benchmarks)."""
        d = self._fuse_desc(agent_stride, level_stride, pairwise_b, n, ego)
        lut, lb = self._lut_ptrs()
        L.check(self.lib.qv2x_fuse_att_f32(C.byref(d), codes_ptr, lut, lb, L.ptr(feats) if feats is not None else None,
                                           L.ptr(pairwise_b), L.ptr(out), L.current_stream()), "qv2x_fuse_att_f32")

    def _lut_ptrs(self):
        return (L.ptr(self.lut), L.ptr(self.lut_bias)) if self.has_codebook else (None, None)

    def _scene_chunks(self, agent_stride, level_stride, pairwise, offsets, counts, ego):
        """The scenes of a batched a7-a10 launch in chunks of 64 (the kernels' scene tables): per chunk ``(first scene, scenes, FuseDesc,
        offsets i64[], agent counts i32[], decode table, its bias)``."""
        lut, lb = self._lut_ptrs()
        for s0 in range(0, len(counts), 64):
            s1 = min(len(counts), s0 + 64)
            d = self._fuse_desc(agent_stride, level_stride, pairwise[s0], max(counts[s0:s1]), ego)
            yield s0, s1 - s0, d, (C.c_int64 * (s1 - s0))(*offsets[s0:s1]), (C.c_int32 * (s1 - s0))(*counts[s0:s1]), lut, lb

    def fuse_scenes(self, codes_ptr, agent_stride, level_stride, feats, pairwise, offsets, counts, out, ego=0):
        """a7-a10 for several scenes in ONE launch: scene s = ``counts[s]`` agents starting ``offsets[s]`` bytes into the codes (floats into
        ``feats``); ``pairwise`` f64 [scenes, L, L, 4, 4], ``out`` f32 [scenes, H*W, 256].  Chunks of 64 scenes."""
        for s0, n, d, offs, cnts, lut, lb in self._scene_chunks(agent_stride, level_stride, pairwise, offsets, counts, ego):
            L.check(self.lib.qv2x_fuse_att_batch_f32(C.byref(d), n, offs, cnts, codes_ptr, lut, lb,
                                                     L.ptr(feats) if feats is not None else None, L.ptr(pairwise[s0]), L.ptr(out[s0]),
                                                     L.current_stream()), "qv2x_fuse_att_batch_f32")

    def _self_transforms_are_identity(self, pairwise: torch.Tensor) -> bool:
        """The table look-up for single-agent scenes skips the warp: it is only the model's result when ``pairwise[b, 0, 0] = I`` (what
        ``get_pairwise_transformation`` produces, transformation_utils.py:21-66).  The reference warps with whatever it is handed
        (AttFusion -> warp_affine_simple, fusion_in_one.py:142-143), so a non-identity self-transform (pose-noise experiments, a caller's
        bug) must take the general path.  Checked on the host whenever the matrix can be read: a CPU tensor always; a device tensor unless
        the stream is capturing (the verdict is remembered per tensor OBJECT and version, so a replayed input costs one read-back).  During capture of a
        device tensor the contract cannot be verified and is assumed -- ``capture()`` runs an eager forward first, which does check."""
        if pairwise.is_cuda:
            if torch.cuda.is_current_stream_capturing():
                return True
            # The verdict is remembered for the tensor OBJECT (a weak reference) at its version -- never for an address: a fresh tensor that
            # reuses a freed block has the same data_ptr and version 0 but other contents (GPU suite of round 6 hit exactly that).
            ref = getattr(self, "_ident_ref", None)
            if ref is not None and ref[0]() is pairwise and ref[1] == pairwise._version:
                return ref[2]
            t00 = pairwise[:, 0, 0].cpu()
        else:
            t00 = pairwise[:, 0, 0]
        ok = bool((t00 == torch.eye(4, dtype=t00.dtype)).all())
        if pairwise.is_cuda:
            import weakref
            self._ident_ref = (weakref.ref(pairwise), pairwise._version, ok)
        return ok

    def _one_launch_agents(self) -> int:
        """most agents per scene for which a7-a11 run as one launch (see ``fuse_heads_max_agents``)"""
        batched = self.has_codebook and self.levels == 3
        return self.fuse_heads_max_agents if batched else min(self.fuse_heads_max_agents, 1)

    def _table_heads_out(self, codes, n: int) -> dict:
        """The model's output dict for ``n`` single-agent scenes from their code planes u8 [levels, n * H*W] (qv2x_table_heads_f32).
        Relies on the contract ``pairwise_t_matrix[b, 0, 0] = I`` (``T[i, j] = T_j^-1 T_i``, transformation_utils.py:21-66)."""
        tab, tb, da, za, c0, c1 = self.table_heads
        hw = self.fh * self.fw
        preds = torch.empty((n, c0, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        sp = torch.empty((n, c1, self.fh, self.fw), dtype=torch.float32, device=self.dev) if c1 else None
        L.check(self.lib.qv2x_table_heads_f32(L.ptr(codes), n * hw, hw, self.levels, self.kc, c0, c1, L.ptr(tab), L.ptr(tb), L.ptr(da), L.ptr(za),
                                              L.ptr(preds), L.ptr(sp) if sp is not None else None, L.current_stream()), "qv2x_table_heads_f32")
        out = split_heads(preds, self.heads.splits)
        if sp is not None:
            out.update(split_heads(sp, self.heads_single.splits, "_single"))
        return out

    def fuse_heads_scenes(self, codes_ptr, agent_stride, level_stride, feats, pairwise, offsets, counts, ego=0, fused_tap=None):
        """a7-a11 for several scenes in ONE launch per 64 scenes (qv2x_fuse_heads_batch_f32): predictions f32 [scenes, cout, H, W]; the
        fused map only exists tile by tile in LDS (``fused_tap`` f32 [scenes, H*W, 256], optional, receives a copy)."""
        hd, hw = self.heads, self.fh * self.fw
        out = torch.empty((len(counts), hd.cout, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        for s0, n, d, offs, cnts, lut, lb in self._scene_chunks(agent_stride, level_stride, pairwise, offsets, counts, ego):
            L.check(self.lib.qv2x_fuse_heads_batch_f32(C.byref(d), n, offs, cnts, codes_ptr, lut, lb,
                                                       L.ptr(feats) if feats is not None else None, L.ptr(pairwise[s0]),
                                                       hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za), L.ptr(out[s0]),
                                                       L.ptr(fused_tap[s0]) if fused_tap is not None else None, L.current_stream()),
                    "qv2x_fuse_heads_batch_f32")
        return out

    def _post_form(self, lens: List[int], taps: Optional[dict], identity) -> str:
        """How a7-a11 run on scenes of ``lens`` agents: "tables" -- every scene one agent, all heads by table look-up on its code planes, only
        where the contract ``pairwise[b, 0, 0] = I`` holds (``identity``: a bool, or a callable asked last that may read the matrix back);
        "one_launch" -- qv2x_fuse_heads_batch_f32, no fused map in HBM; or "fused" -- the fused map, then the heads (what ``taps`` need)."""
        if (taps is None and self.table_heads is not None and self.single_agent_tables and all(n == 1 for n in lens)
                and (identity() if callable(identity) else identity)):
            return "tables"
        if taps is None and len(lens) * self.fh * self.fw // 32 >= self.fuse_heads_min_tiles and max(lens) <= self._one_launch_agents():
            return "one_launch"
        return "fused"

    def _post(self, form: str, codes_ptr, agent_stride, level_stride, feats, pairwise, offsets, lens: List[int], ego: int,
              own: Optional[torch.Tensor], n_own: int, taps: Optional[dict] = None) -> dict:
        """a7-a11 in ``form`` (``_post_form``) on the scenes ``lens`` -- the agents' code planes at ``codes_ptr`` (``offsets`` in bytes) or
        their fp32 shared features ``feats`` (``offsets`` in floats), ``pairwise`` f64 [scenes, L, L, 4, 4] -- and the ``*_single`` heads on
        ``own``, the code planes u8 [levels, n_own * H*W] of the agents that want them (the scenes themselves in the table form; without a
        codebook the ``*_single`` heads run on ``feats``).  Returns the model's output dict."""
        if form == "tables":
            return self._table_heads_out(own, len(lens))
        hw, nb = self.fh * self.fw, len(lens)
        single = self.heads_single is not None and own is not None
        sp = None
        if form == "one_launch":                                         # decode + warp + fusion + heads, tile by tile: no fused map in HBM
            preds = self.fuse_heads_scenes(codes_ptr, agent_stride, level_stride, feats, pairwise, offsets, lens, ego)
            if single:
                sp = self._decode_heads_single(own, n_own)
        else:                                                            # every scene of the call in one launch, then the heads
            fused = torch.empty((nb, hw, 256), dtype=torch.float32, device=self.dev)
            self.fuse_scenes(codes_ptr, agent_stride, level_stride, feats, pairwise, offsets, lens, fused, ego)
            if single:                                                   # the heads on the fused map + the *_single heads on the own codes
                preds, sp = self._heads_pair(fused, nb, own, n_own)
            else:
                preds = self._run_heads(self.heads, fused, nb, hw)
            if taps is not None:
                taps["fused"] = fused
        if self.heads_single is not None and sp is None and feats is not None:
            sp = self._run_heads(self.heads_single, feats, sum(lens), hw)
        out = split_heads(preds, self.heads.splits)
        if sp is not None:
            out.update(split_heads(sp, self.heads_single.splits, "_single"))
        return out

    def fuse_and_heads(self, codes, agent_stride, level_stride, pairwise_b, n_agents, ego=0) -> dict:
        """a7-a11 on an (all-gathered) code tensor for one scene; ``pairwise_b`` f64 [L, L, 4, 4] on the device."""
        return self.fuse_heads_and_single(codes, agent_stride, level_stride, pairwise_b, n_agents, ego, None, 0)

    def _decode_heads_single(self, codes, n_agents: int):
        hw = self.fh * self.fw
        hd = self.heads_single
        sp = torch.empty((n_agents, hd.cout, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        if self.single_by_tables:
            tab, tb = hd.lut_tables
            L.check(self.lib.qv2x_single_heads_lut_f32(L.ptr(codes), n_agents * hw, hw, self.levels, self.kc, hd.cout, L.ptr(tab), L.ptr(tb),
                                                       L.ptr(hd.da), L.ptr(hd.za), L.ptr(sp), L.current_stream()), "qv2x_single_heads_lut_f32")
            return sp
        if self.single_by_global_tables:
            tab, tb = hd.lut_tables
            L.check(self.lib.qv2x_table_heads_f32(L.ptr(codes), n_agents * hw, hw, self.levels, self.kc, hd.cout, 0, L.ptr(tab), L.ptr(tb),
                                                  L.ptr(hd.da), L.ptr(hd.za), L.ptr(sp), None, L.current_stream()), "qv2x_table_heads_f32")
            return sp
        L.check(self.lib.qv2x_decode_heads_f32(L.ptr(codes), n_agents * hw, hw, self.levels, self.kc, L.ptr(self.lut), L.ptr(self.lut_bias),
                                               hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za),
                                               L.ptr(sp), L.current_stream()), "qv2x_decode_heads_f32")
        return sp

    def _heads_pair(self, fused, nb, codes, n_agents):
        """heads on the fused rows [nb*hw, 256] + *_single heads on the agents' own codes [levels, n_agents*hw]"""
        hw = self.fh * self.fw
        hd, hs = self.heads, self.heads_single
        if self.single_by_tables or self.single_by_global_tables:        # the single heads are a table look-up: their own launch
            return self._run_heads(hd, fused, nb, hw), self._decode_heads_single(codes, n_agents)
        preds = torch.empty((nb, hd.cout, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        sp = torch.empty((n_agents, hs.cout, self.fh, self.fw), dtype=torch.float32, device=self.dev)
        L.check(self.lib.qv2x_heads_pair_f32(L.ptr(fused), nb * hw, hw, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da),
                                             L.ptr(hd.za), L.ptr(preds), L.ptr(codes), n_agents * hw, self.levels, self.kc,
                                             L.ptr(self.lut), L.ptr(self.lut_bias), hs.cout, hs.cout_pad, L.ptr(hs.w), L.ptr(hs.bias),
                                             L.ptr(hs.da), L.ptr(hs.za), L.ptr(sp), L.current_stream()), "qv2x_heads_pair_f32")
        return preds, sp

    def fuse_heads_and_single(self, codes, agent_stride, level_stride, pairwise_b, n_agents, ego, own_codes, n_own: int = 1) -> dict:
        """``fuse_and_heads`` on the gathered codes plus ``single_preds`` on this rank's own codes, the two head passes in one
        launch (what one rank of the multi-GPU driver does after the all-gather)."""
        pairwise = pairwise_b.to(torch.float64).contiguous()[None]      # (one scene of the batched fuse: the same device code, qv2x.h)
        return self._post("fused", L.ptr(codes), agent_stride, level_stride, None, pairwise, [0], [n_agents], ego, own_codes, n_own)

    def single_preds(self, codes, n_agents: int) -> dict:
        """``*_preds_single`` (heter_model_baseline.py:224-230): the per-agent heads on each agent's own decoded feature."""
        if self.heads_single is None:
            return {}
        return split_heads(self._decode_heads_single(codes, n_agents), self.heads_single.splits, "_single")

    # ---- the reference's model contract ----------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, data_dict: dict, taps: Optional[dict] = None) -> dict:
        agents = data_dict["agent_modality_list"]
        n_total = len(agents)
        if any(a != "m1" for a in agents):
            raise NotImplementedError("deployed path: every agent is the LiDAR modality 'm1' (a heterogeneous model deploys as DeployedHeterModel)")
        enc = self.encode_agents(data_dict["inputs_m1"], n_total, taps)
        return self.finish(enc, n_total, data_dict, taps)

    @torch.no_grad()
    def finish(self, enc, n_total: int, data_dict: dict, taps: Optional[dict] = None) -> dict:
        """a7-a11 on the agents' wire data ``enc`` (code planes u8 [levels, n_total * H*W] in agent order, or the i8 shrinker output of a
        model without a codebook): decode + warp + fusion per scene, the heads, the ``*_single`` heads."""
        pairwise, lens = scene_layout(data_dict, n_total)
        hw = self.fh * self.fw
        # (no workspace of n_total agents here: a codebook model's post stage only needs the code planes it is handed -- the ego engine of a
        #  heterogeneous scene never encodes n_total agents itself)
        feats = None if self.has_codebook else self._shared_features(enc, n_total)
        form = self._post_form(lens, taps, lambda: self._self_transforms_are_identity(data_dict["pairwise_t_matrix"]))   # (the caller's own tensor object: see there)
        if form != "tables" and not pairwise.is_cuda:                   # a host tensor (the reference's collate output before to_device): copied here
            if torch.cuda.is_current_stream_capturing():
                raise ValueError("pairwise_t_matrix on the host cannot be uploaded during HIP-graph capture: pass a device tensor")
            pairwise = pairwise.to(self.dev)
        starts = [sum(lens[:bi]) for bi in range(len(lens))]
        if self.has_codebook:
            out = self._post(form, L.ptr(enc), hw, n_total * hw, None, pairwise, [st * hw for st in starts], lens, 0, enc, n_total, taps)
        else:
            out = self._post(form, None, 0, 0, feats, pairwise, [st * hw * 256 for st in starts], lens, 0, None, n_total, taps)
        if taps is not None:
            taps["codes"] = enc if self.has_codebook else None
            taps["features"] = feats
        return out

    # ---- HIP-graph replay of a fixed-shape frame ---------------------------------------------------------------
    def capture(self, data_dict: dict):
        """Capture one frame into a HIP graph (``capture_forward``): the returned callable replays it on the same input tensors.

        The graph relies on the resident canvas being clean between calls (``DeployedModel.pillars_to_canvas``): every path of that class leaves it
        so; ``pillars_to_canvas(resident=False)`` refuses to run on a workspace that has such graphs.
        The pillar count M = ``voxel_features.shape[0]`` is baked into the graph: keep M fixed across replays and pad
        unused rows with an out-of-range agent index (``voxel_coords[:, 0] = -1``), which ``pfn_scatter_kernel`` drops.
        ``record_len`` (several scenes per call) must be a CPU tensor: its values shape the launch list."""
        return capture_forward(self, data_dict)


class DeployedModel(DeployedPostStage):
    """The hot path as HIP kernels.  Same call contract as the reference's model: the W8A8 agent stage a1-a6 (PFN or
    SECOND, backbone plan, shrinker, compressor, the three encode modes, the resident canvas) in front of ``DeployedPostStage``."""

    def __init__(self, state: Dict[str, np.ndarray], device="cuda", emit_single_preds: Optional[bool] = None):
        super().__init__(state, device, emit_single_preds)
        s, dev = state, self.dev

        # ---- a1: PFN parameters (host struct, passed by value to the kernel) -- or a13, the SECOND encoder ------------
        self.encoder_kind = str(s["meta/encoder"]) if "meta/encoder" in s else "point_pillar"
        if self.encoder_kind == "second":
            last = int(s["second/n_layers"]) - 1
            q = (float(np.float32(s[f"second/{last}/a_delta"])), int(s[f"second/{last}/a_zp"]))
            self.canvas_c, self.canvas_q, self.pfn = int(s["meta/canvas_channels"]), q, None
            self.second: Dict[int, object] = {}                        # per agent count: a DeployedSecondEncoder (it owns the canvas)
            self.second_max_voxels, self.second_max_points = 70000, 5
        else:
            self.pfn, q = pfn_params(s)
            self.canvas_c, self.canvas_q = 64, q

        # ---- a3: backbone ----------------------------------------------------------------------------------
        self.blocks: List[List[_ConvLayer]] = []
        self.chains: List[Optional[_ChainLayers]] = []                 # per level: its conv layers as one launch, where built
        self.deblocks: List[_DeconvLayer] = []
        cat_groups, c0 = [], 0
        cin = self.canvas_c
        for lvl in range(len(self.layer_nums)):
            convs = []
            for i in range(self.layer_nums[lvl] + 1):
                layer = _ConvLayer(s, f"backbone_m1.blocks.{lvl}.{i + 1}", [(0, cin, q[0], q[1])],
                                   self.strides[lvl] if i == 0 else 1, dev)
                convs.append(layer)
                q, cin = layer.out_q, layer.cout
            self.blocks.append(convs)
            self.chains.append(_ChainLayers(convs, dev) if _ChainLayers.eligible(convs) else None)
            de = _DeconvLayer(s, f"backbone_m1.deblocks.{lvl}.0", q, dev)
            self.deblocks.append(de)
            cat_groups.append((c0, de.cout, de.out_q[0], de.out_q[1]))
            c0 += de.cout
        self.cat_channels = c0
        # ---- a4: shrinker ----------------------------------------------------------------------------------
        self.shrink0 = _ConvLayer(s, "shrinker_m1.layers.0.double_conv.0", cat_groups, 1, dev)
        self.shrink1 = _ConvLayer(s, "shrinker_m1.layers.0.double_conv.1",
                                  [(0, self.shrink0.cout, *self.shrink0.out_q)], 1, dev)
        if self.shrink1.cout != 256:
            raise NotImplementedError("deployed path expects a 256-channel shared feature")
        # ---- NaiveCompressor (models without the codebook): 256 -> 256 / r -> 256 -> 256, the bottleneck padded to 64 channels ----
        self.compress = bool(s.get("meta/compress", False))
        self.final = self.shrink1                                      # the layer whose output is the shared feature
        if self.compress:
            if self.has_codebook:
                raise NotImplementedError("deployed path: compressor and codebook together")
            narrow = int(s["compressor.encoder.0/w_code"].shape[0])
            pad = (narrow + 63) // 64 * 64
            self.comp = [_ConvLayer(s, "compressor.encoder.0", [(0, 256, *self.shrink1.out_q)], 1, dev, pad_cout=pad)]
            self.comp.append(_ConvLayer(s, "compressor.decoder.0", [(0, pad, *self.comp[0].out_q)], 1, dev, pad_cin=pad))
            self.comp.append(_ConvLayer(s, "compressor.decoder.1", [(0, 256, *self.comp[1].out_q)], 1, dev))
            self.comp_channels = narrow                                # what would travel: narrow x H x W bytes per agent
            self.final = self.comp[-1]
        # ---- a11: heads ------------------------------------------------------------------------------------
        self._set_heads(_Heads(s, "", dev), _Heads(s, "_single", dev) if (self.emit_single and "cls_head_single/w_code" in s) else None,
                        tables=True)
        self._bufs: Dict[int, dict] = {}
        # launch-plan switches for the ablation tools (tools/bench_*_abl.py); the defaults are the shipped configuration
        self.use_wide_conv, self.batch_deconvs, self.use_chains = True, True, True
        self.chain_max_agents = 1
        # "exact": every cell through the reference's eleven chained GEMMs.  "two_stage" (round 6, the default wherever its contract holds):
        # the SAME indices by construction -- exact integer candidates, the chain only for the cells a proven bound cannot decide
        # (encode_two_stage.py; its operands are built with the first workspace).  "collapsed": opt-in and approximate, see collapse_encoder.
        self._collapsed, self._two_stage, self.two_stage_refused = None, None, None
        self.encode_form = "auto"                                      # "wave": force the wave-per-32-cells encode kernel on every cell (same codes)
        self.encode_mode = "two_stage" if self.two_stage_supported() else "exact"
        # the pair of entries behind "two_stage".  True: the span pair (qv2x_codebook_encode_candidates_span_i8 + qv2x_codebook_encode_span_f32:
        # six lists by (first, last) undecided level, stage 2 ends a tile at its last undecided level -- DESIGN.md 3.1); False: the
        # first pair (three lists by first undecided level, every listed cell through all later levels).  The same indices either way.
        self.encode_span = True

    def _padded(self, n, h, w, c, q):
        """Padded i8 BEV tensor with the border (and interior) preset to the code of 0.0."""
        t = torch.empty((n, h + 2, w + 2, c), dtype=torch.int8, device=self.dev)
        t.fill_(int(q[1]) - 128)
        return t

    def _workspace(self, n: int) -> dict:
        if n in self._bufs:
            return self._bufs[n]
        b = {}
        h, w = self.ny, self.nx
        if self.encoder_kind == "second":
            from .engine_second import DeployedSecondEncoder
            self.second[n] = DeployedSecondEncoder(self.state, self.dev, agents=n, max_voxels=self.second_max_voxels, max_points=self.second_max_points)
            b["canvas"] = self.second[n].bev
        else:
            b["canvas"] = self._padded(n, h, w, 64, self.canvas_q)
        b["lvl"] = []
        for lvl, convs in enumerate(self.blocks):
            h, w = (h + 2 - 3) // self.strides[lvl] + 1, (w + 2 - 3) // self.strides[lvl] + 1
            # ping-pong pair per level.  The border stores the consumer's input zero point; post-ReLU quantizers all
            # have zero point 0, and a shared buffer needs them equal.
            zps = {c.out_q[1] for c in convs}
            if len(zps) != 1:
                raise NotImplementedError("conv outputs of one backbone level must share a zero point (post-ReLU: 0)")
            pair = [self._padded(n, h, w, convs[0].cout, convs[0].out_q) for _ in range(2)]
            b["lvl"].append((pair, h, w))
        (_, h0, w0) = b["lvl"][0]
        self.fh, self.fw = h0 * self.ups[0], w0 * self.ups[0]
        for lvl, (_, hl, wl) in enumerate(b["lvl"]):
            # the reference's torch.cat raises on mismatched deblock outputs (base_bev_backbone.py:116); the deconv kernel
            # derives its row pitch from (h*s + 2, w*s + 2), so a mismatch would write out of bounds in the concat tensor
            if (hl * self.ups[lvl], wl * self.ups[lvl]) != (self.fh, self.fw):
                raise ValueError(f"deblock {lvl} upsamples {hl}x{wl} by {self.ups[lvl]} to {hl * self.ups[lvl]}x{wl * self.ups[lvl]}, "
                                 f"level 0 gives {self.fh}x{self.fw}: the grid does not line up across backbone levels")
        cat = torch.empty((n, self.fh + 2, self.fw + 2, self.cat_channels), dtype=torch.int8, device=self.dev)
        c0 = 0
        for de in self.deblocks:
            cat[..., c0:c0 + de.cout] = int(de.out_q[1]) - 128
            c0 += de.cout
        b["cat"] = cat
        b["s0"] = self._padded(n, self.fh, self.fw, self.shrink0.cout, self.shrink0.out_q)
        b["s1"] = self._padded(n, self.fh, self.fw, self.shrink1.cout, self.shrink1.out_q)
        if self.compress:
            b["comp"] = [self._padded(n, self.fh, self.fw, c.cout, c.out_q) for c in self.comp]
        hw = self.fh * self.fw
        if self.has_codebook:
            b["codes"] = torch.empty((self.levels, n, hw), dtype=torch.uint8, device=self.dev)
        if self.two_stage_supported():
            if self._two_stage is None and self.encode_mode == "two_stage":
                self._build_two_stage()                                 # (a6's operands exist before a6 first runs)
            b["enc_list"] = torch.zeros(3 * n * hw, dtype=torch.int32, device=self.dev)     # three lists (by first undecided level)
            b["enc_counters"] = torch.zeros(4, dtype=torch.int32, device=self.dev)
            b["enc_span_list"] = torch.zeros(6 * n * hw, dtype=torch.int32, device=self.dev)     # the span pair's own: six lists by (first, last)
            b["enc_span_counters"] = torch.zeros(8, dtype=torch.int32, device=self.dev)
        if not self.has_codebook or self.heads_single is not None:
            b["feats"] = torch.empty((n, hw, 256), dtype=torch.float32, device=self.dev)
        self._bufs[n] = b
        return b

    # ---- kernel launch helpers -----------------------------------------------------------------------------
    def _conv(self, layer: _ConvLayer, x, n, h, w, out, out_ctotal=None, out_c0=0):
        launch_conv3x3(self.lib, layer, x, n, h, w, out, out_ctotal=out_ctotal, out_c0=out_c0, wide=self.use_wide_conv)

    def _chain(self, ch: _ChainLayers, x, n, h, w, out):
        """``x``: padded input [n][h+2][w+2][64] of the first layer; ``out``: padded output of the last one."""
        d = L.ChainDesc()
        d.n, d.in_h, d.in_w = n, h, w
        d.h, d.w = out.shape[1] - 2, out.shape[2] - 2
        d.depth, d.stride0, d.relu = len(ch.convs), ch.stride0, 1
        for i, c in enumerate(ch.convs):
            d.out_delta[i], d.out_zp[i] = c.out_q[0], float(c.out_q[1])
        L.check(self.lib.qv2x_conv3x3_i8_chain64(C.byref(d), L.ptr(x), L.ptr(ch.w), L.ptr(ch.scale), L.ptr(ch.corr), L.ptr(ch.aw),
                                                 L.ptr(ch.bias), L.ptr(out), L.current_stream()), ch.name)

    def _deconv_desc(self, de: _DeconvLayer, n, h, w, out, out_c0):
        d = L.DeconvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.s = n, h, w, de.cin, de.cout, de.s
        d.in_zx, d.in_delta = int(de.in_q[1]), float(de.in_q[0])
        d.out_ctotal, d.out_c0, d.relu = out.shape[-1], out_c0, 1
        d.out_delta, d.out_zp = de.out_q[0], float(de.out_q[1])
        d.out_h, d.out_w = out.shape[1] - 2, out.shape[2] - 2
        return d

    def _deconv(self, de: _DeconvLayer, x, n, h, w, out, out_c0):
        d = self._deconv_desc(de, n, h, w, out, out_c0)
        L.check(self.lib.qv2x_deconv_i8(C.byref(d), L.ptr(x), L.ptr(de.w), L.ptr(de.bias), L.ptr(out), L.current_stream()), de.name)

    def _deconv_batch(self, items, n):
        """items: [(layer, x, h, w, out, out_c0)] -> one launch"""
        k = len(items)
        descs = (L.DeconvDesc * k)(*[self._deconv_desc(de, n, h, w, out, c0) for (de, x, h, w, out, c0) in items])
        arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
        L.check(self.lib.qv2x_deconv_i8_batch(descs, k, arr([it[1] for it in items]), arr([it[0].w for it in items]),
                                              arr([it[0].bias for it in items]), arr([it[4] for it in items]), L.current_stream()),
                "qv2x_deconv_i8_batch")

    # ---- stages (also used one by one by the parity tests and the multi-GPU driver) --------------------------
    def conv_plan(self, n_agents: int):
        """Static launch list of a3 + a4 for ``n_agents`` agents: ``(kind, layer, x, h, w, out, out_c0, macs)``."""
        b = self._workspace(n_agents)
        # one launch per backbone level (conv3x3_i8_chain64) pays while launches are latency-bound, i.e. for ONE agent-frame (29.6 us
        # against four launches of ~10); from two on the per-layer kernels are as fast or faster (V2X-Real level 0: 2 agent-frames
        # 509 vs 501 us for the whole stack, 8: 203 us fused against 144 us in four launches)
        use_chains = self.use_chains and n_agents <= self.chain_max_agents
        key = ("plan", use_chains)
        if key in b:
            return b[key]
        plan = []
        x, h, w, c0 = b["canvas"], self.ny, self.nx, 0
        for lvl, convs in enumerate(self.blocks):
            pair, ho, wo = b["lvl"][lvl]
            macs = [n_agents * ho * wo * layer.cout * layer.w.shape[1] for layer in convs]
            if use_chains and self.chains[lvl] is not None:
                out = pair[(len(convs) - 1) % 2]
                plan.append(("chain", self.chains[lvl], x, h, w, out, 0, sum(macs)))
                x, h, w = out, ho, wo
            else:
                for i, layer in enumerate(convs):
                    out = pair[i % 2]
                    plan.append(("conv", layer, x, h, w, out, 0, macs[i]))
                    x, h, w = out, ho, wo
            de = self.deblocks[lvl]
            plan.append(("deconv", de, x, h, w, b["cat"], c0, n_agents * h * w * de.cin * de.cout * de.s * de.s))
            c0 += de.cout
        hw = n_agents * self.fh * self.fw
        plan.append(("conv", self.shrink0, b["cat"], self.fh, self.fw, b["s0"], 0, hw * self.shrink0.cout * self.shrink0.w.shape[1]))
        plan.append(("conv", self.shrink1, b["s0"], self.fh, self.fw, b["s1"], 0, hw * self.shrink1.cout * self.shrink1.w.shape[1]))
        if self.compress:
            x = b["s1"]
            for c, out in zip(self.comp, b["comp"]):
                plan.append(("conv", c, x, self.fh, self.fw, out, 0, hw * c.cout * c.w.shape[1]))
                x = out
        b[key] = plan
        return plan

    def run_plan(self, n_agents: int, only=None, taps: Optional[dict] = None):
        pending = []                                  # the deblocks only feed the concat: they run as ONE launch before the shrinker

        def flush():
            if len(pending) == 1:
                de, x, h, w, out, c0 = pending[0]
                self._deconv(de, x, n_agents, h, w, out, c0)
            elif pending:
                self._deconv_batch(pending, n_agents)
            pending.clear()

        for (kind, layer, x, h, w, out, c0, _) in self.conv_plan(n_agents):
            if only is not None and not only(kind, layer):
                continue
            if kind == "chain":
                self._chain(layer, x, n_agents, h, w, out)
                if taps is not None:
                    taps[layer.name] = out.clone()
            elif kind == "conv":
                if layer is self.shrink0:
                    flush()
                self._conv(layer, x, n_agents, h, w, out)
                if taps is not None:
                    taps[layer.name] = out.clone()
            else:
                pending.append((layer, x, h, w, out, c0))
                if not self.batch_deconvs:
                    flush()
        flush()

    def pillars_to_canvas(self, inputs: dict, n_agents: int, resident: bool = False):
        """a1 + a2: clear the canvas, run the PFN and scatter.  ``resident``: the caller will hand the canvas back clean with
        ``clear_pillars`` once the first convolution has read it, so the 9 MB-per-frame fill is skipped while the canvas is known clean."""
        b = self._workspace(n_agents)
        st = L.current_stream()
        vf, co, npnt = pillar_inputs(inputs, pfn=self.encoder_kind != "second")
        if self.encoder_kind == "second":                             # a13: MeanVFE + sparse convolutions + height compression
            return self.second[n_agents]({"voxel_features": vf, "voxel_coords": co, "voxel_num_points": npnt})
        canvas = b["canvas"]
        # INVARIANT of the resident canvas: between calls it holds the code of 0.0 everywhere (`canvas_clean`), so a resident call needs
        # no fill -- and a HIP graph captured in that state contains none.  Such a graph cannot see this host flag: once one exists
        # (`fill_less_graphs`), nothing may leave the canvas dirty behind its back -- the non-resident form (which returns a canvas the
        # caller is going to read) is refused on that workspace, and `forward` refills at once if it fails between scatter and clear.
        capturing = torch.cuda.is_current_stream_capturing()
        if not resident and b.get("fill_less_graphs", False):
            raise L.Qv2xError("pillars_to_canvas(resident=False) on a workspace whose captured graphs rely on the clean resident canvas: "
                              "use resident=True + clear_pillars, or another DeployedModel")
        if not (resident and b.get("canvas_clean", False)):
            L.check(self.lib.qv2x_fill_i8(L.ptr(canvas), canvas.numel(), int(self.pfn.z2) - 128, st), "qv2x_fill_i8")
        elif capturing:
            b["fill_less_graphs"] = True
        b["canvas_clean"] = False
        L.check(self.lib.qv2x_pfn_scatter_i8(L.ptr(vf), L.ptr(co), L.ptr(npnt), vf.shape[0], 32, C.byref(self.pfn),
                                             L.ptr(canvas), n_agents, self.ny, self.nx, st), "qv2x_pfn_scatter_i8")
        return canvas

    def _restore_canvas(self, n_agents: int):
        """After a failure between scatter and clear: put the whole canvas back to the code of 0.0 (outside any capture)."""
        b = self._workspace(n_agents)
        if self.encoder_kind != "second" and not torch.cuda.is_current_stream_capturing():
            L.check(self.lib.qv2x_fill_i8(L.ptr(b["canvas"]), b["canvas"].numel(), int(self.pfn.z2) - 128, L.current_stream()), "qv2x_fill_i8")
            b["canvas_clean"] = True

    def clear_pillars(self, inputs: dict, n_agents: int):
        """Sets the cells ``pillars_to_canvas(..., resident=True)`` wrote back to the code of 0.0: the canvas is clean for the next frame."""
        if self.encoder_kind == "second":
            return
        b = self._workspace(n_agents)
        co = inputs["voxel_coords"].to(torch.int32).contiguous()
        L.check(self.lib.qv2x_pfn_unscatter_i8(L.ptr(co), co.shape[0], int(self.pfn.z2) - 128, L.ptr(b["canvas"]), n_agents, self.ny, self.nx,
                                               L.current_stream()), "qv2x_pfn_unscatter_i8")
        b["canvas_clean"] = True

    def encode_codes(self, n_agents: int, out: Optional[torch.Tensor] = None):
        """a6 on the shrinker output already in the workspace; ``out``: u8 [levels, n_agents, H*W] (default: the workspace's)."""
        b = self._workspace(n_agents)
        codes = b["codes"] if out is None else out
        if codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.numel() != self.levels * n_agents * self.fh * self.fw:
            raise ValueError("encode_codes: out must be a contiguous uint8 tensor [levels, n_agents, H*W]")
        d = L.EncodeDesc()
        d.n, d.h, d.w, d.levels, d.kc, d.segs = n_agents, self.fh, self.fw, self.enc_levels, self.kc, self.segs
        d.in_zx, d.in_delta = int(self.shrink1.out_q[1]), float(self.shrink1.out_q[0])
        two_stage = self.encode_mode == "two_stage" and self.encode_form == "auto"
        if two_stage and self._two_stage is None:                      # (switched on after the first workspace; may refuse -> "exact")
            self._refuse_during_capture("encode_mode 'two_stage'")
            self._build_two_stage()
            two_stage = self.encode_mode == "two_stage"
        if self.encode_mode == "collapsed":                           # opt-in: one GEMM + argmin chain, indices may differ at near-ties
            if self.segs != 1 or self.kc > 128:
                raise NotImplementedError("encode_mode 'collapsed': seg_num 1 and dict_size <= 128 (the exact encode takes the rest)")
            if self._collapsed is None:
                self._refuse_during_capture("encode_mode 'collapsed'")
                self._collapsed = tuple(_dev(t, self.dev) for t in collapse_encoder(self.state, self.enc_levels, d.in_delta, d.in_zx))
            gp, bias, tab = self._collapsed
            L.check(self.lib.qv2x_codebook_encode_collapsed_f32(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), L.ptr(codes),
                                                                L.current_stream()), "qv2x_codebook_encode_collapsed_f32")
            return codes
        if two_stage:                                                  # exact by construction: candidates on the integer grid + the chain on the undecided
            return self._encode_two_stage(d, b, codes)
        if self.encode_mode not in ("exact", "two_stage"):
            raise ValueError(f"encode_mode {self.encode_mode!r}: 'exact' (every cell through the reference's op order), 'two_stage' (the same "
                             "indices: exact integer candidates, the chain only where the bound cannot decide) or 'collapsed' (opt-in, approximate)")
        if self.encode_form == "wave":                                # tests: the many-frames form at any size (the library picks by launch size)
            L.check(self.lib.qv2x_codebook_encode_wave_f32(C.byref(d), L.ptr(b["s1"]), None, self.level_ptrs, L.ptr(codes),
                                                           L.current_stream()), "qv2x_codebook_encode_wave_f32")
            return codes
        L.check(self.lib.qv2x_codebook_encode_f32(C.byref(d), L.ptr(b["s1"]), self.level_ptrs, L.ptr(codes),
                                                  L.current_stream()), "qv2x_codebook_encode_f32")
        return codes

    def two_stage_supported(self) -> bool:
        """seg_num 1 with dict_size 32 | 64 | ... | 256, or seg_num 2 with dict_size 64 | 128 | 192 | 256, up to three levels: the contracts
        of qv2x_codebook_encode_candidates_i8 (seg_num 1, dict_size <= 128) and qv2x_codebook_encode_candidates_seg_i8 (the rest) on i8 rows"""
        if not self.has_codebook or self.enc_levels > 3 or self.kc > 256:
            return False
        return bool(self.kc % 32 == 0 if self.segs == 1 else self.segs == 2 and self.kc % 64 == 0)

    def _refuse_during_capture(self, what: str):
        if torch.cuda.is_current_stream_capturing():
            raise L.Qv2xError(f"{what}: its operands are built on the host and uploaded -- not inside a HIP-graph capture; encode once "
                              "in this mode before capturing")

    def _build_two_stage(self):
        """The operands of the two-stage encode (encode_two_stage.py) as ``self._two_stage = (gpack, bias, tables, tau, t)``.  A codebook
        outside the candidate stage's fixed-point contract (or ANY failure of the host algebra or the upload) leaves ``encode_mode = "exact"`` -- every cell through the
        chain, the same indices -- and says why in ``two_stage_refused``."""
        if not self.two_stage_supported():
            raise NotImplementedError("encode_mode 'two_stage': seg_num 1 | 2, dict_size <= 256, up to three levels (encode_mode 'exact' takes the rest)")
        from .encode_two_stage import candidate_tables
        try:
            t = candidate_tables(self.state, self.enc_levels, float(self.shrink1.out_q[0]), int(self.shrink1.out_q[1]), self.segs)
            k = np.arange(t["bias"].shape[0], dtype=np.int64) % self.kc               # the index inside the segment
            pf = int(t["pack"])                                          # 128 | 256: encode_two_stage.pack_factor, the entry's in candidate_entry
            packed = (pf * t["bias"] + k).astype(np.float64)
            if not np.array_equal(packed.astype(np.int64), pf * t["bias"] + k):
                raise ValueError("two-stage encode: packed scores not exact in float64")                  # (below 2^53 by construction)
            self._two_stage = (_dev(t["gpack"], self.dev), _dev(packed, self.dev), _dev(t["tables"], self.dev),
                               (C.c_float * (3 * self.enc_levels))(*[float(v) for v in t["tau"].reshape(-1)]), t)
        except Exception as e:                                          # whatever the host algebra raises (LinAlgError, FloatingPointError, ...)
            self.encode_mode, self.two_stage_refused = "exact", str(e) or type(e).__name__

    def candidate_entry(self) -> str:
        """the stage-1 entry for this codebook: the one that takes bias packed with ``encode_two_stage.pack_factor`` (128: seg_num 1,
        dict_size <= 128; 256: the rest), which is what ``_build_two_stage`` packed"""
        from .encode_two_stage import CANDIDATE_ENTRY, pack_factor
        return CANDIDATE_ENTRY[pack_factor(self.segs, self.kc)]

    def _encode_two_stage(self, d, b, codes):
        """a6 as two launches (encode_two_stage.py): the candidate stage (``candidate_entry``) decides every cell it can PROVE, the listed
        rest goes through the reference-order kernel (qv2x_codebook_encode_listed_f32) -- identical indices, a fraction of the fp32 work."""
        gp, bias, tab, tau, _ = self._two_stage
        if self.encode_span:                                           # the same operands: the span entry packs as candidate_entry() does
            L.check(self.lib.qv2x_codebook_encode_candidates_span_i8(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), tau, L.ptr(codes),
                                                                     L.ptr(b["enc_span_list"]), L.ptr(b["enc_span_counters"]), L.current_stream()),
                    "qv2x_codebook_encode_candidates_span_i8")
            L.check(self.lib.qv2x_codebook_encode_span_f32(C.byref(d), L.ptr(b["s1"]), self.level_ptrs, L.ptr(b["enc_span_list"]),
                                                           L.ptr(b["enc_span_counters"]), L.ptr(codes), L.current_stream()), "qv2x_codebook_encode_span_f32")
            return codes
        name = self.candidate_entry()
        L.check(getattr(self.lib, name)(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), tau, L.ptr(codes),
                                        L.ptr(b["enc_list"]), L.ptr(b["enc_counters"]), L.current_stream()), name)
        L.check(self.lib.qv2x_codebook_encode_listed_f32(C.byref(d), L.ptr(b["s1"]), self.level_ptrs, L.ptr(b["enc_list"]), L.ptr(b["enc_counters"]),
                                                         L.ptr(codes), L.current_stream()), "qv2x_codebook_encode_listed_f32")
        return codes

    def encode_refine_stats(self, n_agents: int) -> dict:
        """after a two-stage encode of ``n_agents`` frames: how many cells stage 2 recomputed (counters the candidate stage left on the device)"""
        if not (self.encode_mode == "two_stage" and self.encode_form == "auto") or "enc_counters" not in self._bufs.get(n_agents, {}):
            raise L.Qv2xError(f"encode_refine_stats({n_agents}): no two-stage encode of {n_agents} frames here (encode_mode "
                              f"{self.encode_mode!r}, encode_form {self.encode_form!r}, workspaces {sorted(self._bufs)})")
        cells = n_agents * self.fh * self.fw
        if self.encode_span:                                           # six classes (first, last), in the lists' order (encode_two_stage.SPAN_CLASSES)
            from .encode_two_stage import SPAN_CLASSES
            c = self._bufs[n_agents]["enc_span_counters"].cpu().numpy().astype(np.int64)
            first = [int(sum(c[1 + k] for k, (f, _) in enumerate(SPAN_CLASSES) if f == l)) for l in range(self.enc_levels)]
            return {"cells": cells, "refined": int(c[0]), "refined_fraction": float(c[0]) / cells, "first_flagged_at_level": first,
                    "undecided_span": {f"{f}-{e}": int(c[1 + k]) for k, (f, e) in enumerate(SPAN_CLASSES)}}
        c = self._bufs[n_agents]["enc_counters"].cpu().numpy().astype(np.int64)
        return {"cells": cells, "refined": int(c[0]), "refined_fraction": float(c[0]) / cells, "first_flagged_at_level": [int(v) for v in c[1:1 + self.enc_levels]]}

    def encode_into(self, inputs: dict, frames: int, codes_out: torch.Tensor):
        """a1-a6 for ``frames`` frames of ONE agent (batch index = frame); codes u8 [levels, frames, H*W] written to ``codes_out``."""
        self.pillars_to_canvas(inputs, frames, resident=True)
        try:
            self.run_plan(frames)
            self.clear_pillars(inputs, frames)
        except BaseException:                                          # (KeyboardInterrupt too: a fill-less graph cannot see `canvas_clean`)
            self._restore_canvas(frames)
            raise
        return self.encode_codes(frames, out=codes_out)

    def encode_agents(self, inputs: dict, n_agents: int, taps: Optional[dict] = None):
        """a1-a6 for ``n_agents`` agents.  Returns codes u8 [levels, n, H*W] (or the i8 shrinker output without a codebook)."""
        b = self._workspace(n_agents)
        canvas = self.pillars_to_canvas(inputs, n_agents, resident=True)
        try:
            self.run_plan(n_agents, taps=taps)
            if taps is not None:
                taps["canvas"], taps["cat"] = canvas.clone(), b["cat"]     # (a copy: the canvas itself is handed back clean just below)
            self.clear_pillars(inputs, n_agents)
        except BaseException:
            self._restore_canvas(n_agents)                             # never leave pillars behind (see pillars_to_canvas)
            raise
        if taps is not None:
            taps[self.shrink0.name], taps[self.shrink1.name] = b["s0"], b["s1"]
        if taps is not None and self.compress:
            for c, out in zip(self.comp, b["comp"]):
                taps[c.name] = out
        return self.encode_codes(n_agents) if self.has_codebook else (b["comp"][-1] if self.compress else b["s1"])

    def _shared_features(self, shrinker_out, n_total: int):
        """no codebook: the fp32 shared feature [n, H*W, 256] is the dequantized shrinker output"""
        q = self.final.out_q
        feats = self._workspace(n_total)["feats"]
        L.check(self.lib.qv2x_dequant_i8_f32(L.ptr(shrinker_out), n_total, self.fh, self.fw, 256, int(q[1]), float(q[0]), L.ptr(feats),
                                             L.current_stream()), "qv2x_dequant_i8_f32")
        return feats


class DeployedHeterModel(nn.Module):
    """A heterogeneous scene (heter_model_baseline.py:169-216): every modality has its own encoder / backbone / shrinker, the agents'
    features are assembled in ``agent_modality_list`` order, fusion and heads are shared.  One ``DeployedModel`` per modality runs a1-a6
    on that modality's agents (each from its own PTQ state, ``export_ptq_state(qt, modality=m)``: own weights, own quantizers -- the
    encoder's input scale differs per modality); the code planes go into one buffer in agent order; the ego modality's engine runs
    a7-a11 on it.  The code planes ARE the interface, so nothing else is shared.  Codebook models only."""

    def __init__(self, states: Dict[str, Dict[str, np.ndarray]], ego_modality: Optional[str] = None, device="cuda", **kw):
        super().__init__()
        if not states:
            raise ValueError("DeployedHeterModel: no modality")
        self.engines = {m: DeployedModel(st, device=device, **kw) for m, st in states.items()}
        self.main = self.engines[ego_modality if ego_modality in self.engines else next(iter(self.engines))]
        for m, e in self.engines.items():
            e._workspace(1)                                            # (the feature-map size is known once a workspace exists)
            if not e.has_codebook:
                raise NotImplementedError("deployed heterogeneous path: codebook models (the code planes are what the modalities share)")
            if (e.fh, e.fw, e.levels, e.kc) != (self.main.fh, self.main.fw, self.main.levels, self.main.kc):
                raise ValueError(f"modality {m}: feature map {e.fh} x {e.fw} / codebook {e.levels} x {e.kc} differs from the ego modality's")
        self.dev = self.main.dev
        self._slots: Dict[tuple, Dict[str, torch.Tensor]] = {}         # agent layout -> per modality, the agent slots as a device index

    @torch.no_grad()
    def forward(self, data_dict: dict, taps: Optional[dict] = None) -> dict:
        agents = list(data_dict["agent_modality_list"])
        enc = assemble_heter_codes("DeployedHeterModel", self.engines, self._slots, agents, data_dict,
                                   lambda eng, inputs, k, mt: eng.encode_agents(inputs, k, mt), taps)
        return self.main.finish(enc, len(agents), data_dict, taps)

    def capture(self, data_dict: dict):
        """One heterogeneous frame as a HIP graph (see ``DeployedModel.capture``: fixed pillar counts, resident canvases, CPU ``record_len``)."""
        return capture_forward(self, data_dict)


def deploy_heter(qt_model, device="cuda", **kw) -> DeployedHeterModel:
    """Freeze every modality of a calibrated heterogeneous ``QuantModel`` (``export_ptq_state(qt, modality=m)``) into its own engine."""
    model = qt_model.model if hasattr(qt_model, "model") else qt_model
    states = {m: export_ptq_state(qt_model, modality=m) for m in model.modality_name_list}
    return DeployedHeterModel(states, ego_modality=getattr(model, "ego_modality", None), device=device, **kw)


def deploy(qt_model=None, state: Optional[Dict[str, np.ndarray]] = None, path: Optional[str] = None,
           device="cuda", **kw) -> DeployedModel:
    """Freeze a calibrated ``QuantModel`` (or load a saved PTQ state) into the HIP int8 path.  A plain, un-quantized model (what
    ``create_model`` + ``load_saved_model`` give the reference's ``inference.py``) deploys on the fp32 HIP path instead."""
    if state is None:
        if path is not None:
            state = load_ptq_state(path)
        elif any(hasattr(m, "weight_quantizer") for m in qt_model.modules()):
            inner = qt_model.model if hasattr(qt_model, "model") else qt_model
            if len(getattr(inner, "modality_name_list", ["m1"])) > 1:        # heter_model_baseline.py:41-75: one stack per modality
                if hasattr(inner, "pyramid_backbone"):                        # HEAL: one agent-side stack per modality in front of PyramidFusion
                    from .engine_pyramid import deploy_heter_pyramid
                    return deploy_heter_pyramid(qt_model, device=device)
                return deploy_heter(qt_model, device=device, **kw)
            state = export_ptq_state(qt_model)
        elif hasattr(qt_model, "pyramid_backbone"):
            from .engine_pyramid_fp32 import export_fp32_pyramid_state
            state = export_fp32_pyramid_state(qt_model)
        else:
            from .engine_fp32 import export_fp32_state
            state = export_fp32_state(qt_model)
    if str(state.get("meta/mode", "w8a8")) == "fp32":
        if str(state.get("meta/fusion_method", "att")) == "pyramid":
            from .engine_pyramid_fp32 import DeployedPyramidFp32Model
            return DeployedPyramidFp32Model(state, device=device, **kw)
        from .engine_fp32 import DeployedFp32Model
        return DeployedFp32Model(state, device=device, **kw)
    if str(state.get("meta/fusion_method", "att")) == "pyramid":
        from .engine_pyramid import DeployedPyramidModel
        return DeployedPyramidModel(state, device=device, **kw)
    return DeployedModel(state, device=device, **kw)
