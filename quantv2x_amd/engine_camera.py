"""Deployed W8A8 image encoder of camera agents on MI355X: ``QuantLiftSplatShoot`` over ``QuantCamEncode_Resnet101`` (reference
``quant_block.py:744-985``) from images to the BEV tensor, host side of ``libqv2x.so``.

    imgs f32 -> stem (conv1 7x7/2 + ReLU + quantizer + max-pool: qv2x_cam_stem_f32)
             -> layer1: 3 bottlenecks 64 -> 256, layer2: 4 bottlenecks 128 -> 512, the first with stride 2 (qv2x_conv1x1_i8 /
                qv2x_conv3x3_i8, the per-layer path ``engine_pyramid.bottleneck_layers`` shares with the Pyramid engine)
             -> depth_head + image_head (qv2x_cam_heads_i8) -> f32 depth logits [V, D, fH, fW] and features [V, C, fH, fW]
             -> GpuLiftSplat (qv2x_lss_splat_f32) -> BEV f32 [B, C * Z, Y, X]

Every buffer is allocated at construction, the ring of every padded map holds that map's own zero point, nothing is read back in a call,
and a call is a fixed launch list: capturable as one HIP graph.  There is no CPU / eager fallback.  DESIGN.md section 14."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import lib as L
from .camera_encoder import GpuCamHeads, GpuCamStem, stem_shapes
from .engine import _ConvLayer, capture_call, launch_conv3x3
from .engine_pyramid import _Conv1x1, _q, bottleneck_layers
from .lift_splat import GpuLiftSplat
from .ptq_state import CAMERA_TRUNK, check_finite, export_camera_state

TRUNK_STRIDES = {"layer1": 1, "layer2": 2}


def _needs_codes(state, name):
    if bool(state.get(name + "/a_off", False)):
        raise ValueError(f"{name}: its activation quantizer is disabled, and the next layer of the deployed chain reads its codes")


class _CamBlock:
    """One QuantBottleneck of the camera trunk: 1x1 -> dense 3x3 (carries the stride) -> 1x1, optional 1x1 shortcut, block quantizer."""

    def __init__(self, state, name, in_q, stride, dev):
        for c in ("conv1", "conv2", "conv3"):
            if (f"{name}.{c}/w_code") not in state:
                raise NotImplementedError(f"{name}: a bottleneck (conv1, conv2, conv3) expected; {name}.{c} is missing from the state")
        _needs_codes(state, name + ".conv1")
        _needs_codes(state, name + ".conv2")
        _needs_codes(state, name)
        self.conv1 = _Conv1x1(state, name + ".conv1", in_q, 1, dev)
        width = self.conv1.cout
        if state[name + ".conv2/w_code"].shape[1] != width:
            raise NotImplementedError(f"{name}.conv2: a dense 3x3 convolution (groups = 1) expected")
        self.conv2 = _ConvLayer(state, name + ".conv2", [(0, width, *self.conv1.out_q)], stride, dev)
        self.conv3 = _Conv1x1(state, name + ".conv3", self.conv2.out_q, 1, dev)
        self.down = None
        if (name + ".downsample/w_code") in state:
            self.down = _Conv1x1(state, name + ".downsample", in_q, stride, dev)
        for m in (self.conv3, self.down):
            if m is not None and not m.a_off:
                raise NotImplementedError(f"{m.name}: the sum of a block's branches is formed in fp32 (disable_act_quant, quant_block.py:109-116)")
        if self.down is None and (stride != 1 or self.conv3.cout != self.conv1.cin):
            raise NotImplementedError(f"{name}: an identity shortcut needs stride 1 and as many output as input channels")
        self.name, self.stride, self.cout = name, stride, self.conv3.cout
        self.in_q, self.out_q = in_q, _q(state, name)


class DeployedCameraEncoder:
    """``DeployedCameraEncoder(state, views, samples)`` with ``state`` from ``ptq_state.export_camera_state``; ``deploy_camera_encoder`` builds
    one from a calibrated ``QuantLiftSplatShoot``.

        enc.plan(rots, trans, intrins, post_rots, post_trans)        once per camera rig
        bev = enc(imgs)                                              f32 [samples, C * Z, Y, X], the same tensor every call
        depth, feats = enc.features(imgs, taps)                      the heads' outputs; ``taps`` receives clones of every layer's codes
        replay = enc.capture(imgs)                                   one HIP graph; refresh ``imgs`` in place between replays

    ``imgs`` f32 on the device, ``[samples, views, 3 | 4, H, W]`` or ``[samples * views, 3 | 4, H, W]``; a fourth (depth) channel is never read."""

    def __init__(self, state: Dict[str, np.ndarray], views: int, samples: int = 1, device="cuda"):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.Qv2xError("DeployedCameraEncoder needs an MI355X (torch.cuda.is_available() is False)")
        check_finite(state)
        kind = str(state.get("meta/camera_encoder", ""))
        if kind != "Resnet101":
            raise NotImplementedError(f"DeployedCameraEncoder: camera_encoder {kind!r}; only 'Resnet101' has a quantized form")
        if bool(state.get("meta/use_gt_depth", False)):
            raise NotImplementedError("DeployedCameraEncoder: use_gt_depth replaces the depth head by a one-hot of the measured depth; that path "
                                      "stays on the plugin's QuantLiftSplatShoot")
        self.state, self.dev = state, torch.device(device)
        self.views, self.samples, self.n = int(views), int(samples), int(views) * int(samples)
        self.h, self.w = (int(v) for v in state["meta/final_dim"])
        self.downsample = int(state["meta/downsample"])
        dev, s = self.dev, state
        # ---- layers ----------------------------------------------------------------------------------------------------------------------
        self.stem = GpuCamStem(s, "conv1", dev)
        q = self.stem.out_q
        self.blocks: List[_CamBlock] = []
        for layer, count in CAMERA_TRUNK:
            for i in range(count):
                blk = _CamBlock(s, f"{layer}.{i}", q, TRUNK_STRIDES[layer] if i == 0 else 1, dev)
                self.blocks.append(blk)
                q = blk.out_q
        self.heads = GpuCamHeads(s, q, "depth_head", "image_head", dev)
        if self.heads.cin != self.blocks[-1].cout:
            raise ValueError(f"the heads read {self.heads.cin} channels, the trunk ends with {self.blocks[-1].cout}")
        # ---- shapes: the reference's .view(B, N, C, D, H // downsample, W // downsample) must hold ---------------------------------------
        _, _, hp, wp = stem_shapes(self.h, self.w)
        fh, fw = hp, wp
        for blk in self.blocks:
            fh, fw = (fh - 1) // blk.stride + 1, (fw - 1) // blk.stride + 1
        if (fh, fw) != (self.h // self.downsample, self.w // self.downsample):
            raise ValueError(f"images of {self.h} x {self.w} leave the encoder as {fh} x {fw}, not (H // downsample, W // downsample) = "
                             f"{self.h // self.downsample} x {self.w // self.downsample}: the reference's .view in get_cam_feats fails on this size")
        self.fh, self.fw = fh, fw
        grid_conf = {k: [float(v) for v in s["meta/grid/" + k]] for k in ("xbound", "ybound", "zbound", "ddiscr")}
        grid_conf["mode"] = str(s["meta/grid/mode"])
        self.splat = GpuLiftSplat(grid_conf, (self.h, self.w), self.downsample, self.heads.features, self.views, self.samples, dev)
        if (self.splat.depth_bins, self.splat.fh, self.splat.fw) != (self.heads.depth_bins, fh, fw):
            raise ValueError(f"the frustum is {self.splat.depth_bins} x {self.splat.fh} x {self.splat.fw}, the depth head gives "
                             f"{self.heads.depth_bins} x {fh} x {fw}")
        if int(s.get("meta/features", self.heads.features)) != self.heads.features:
            raise ValueError(f"img_features {int(s['meta/features'])} but the image head has {self.heads.features} rows")
        # ---- buffers ---------------------------------------------------------------------------------------------------------------------
        n = self.n
        self._pool: Dict[tuple, list] = {}
        self._rows: Dict[tuple, torch.Tensor] = {}
        self.x0 = self._map(hp, wp, 64, self.stem.out_q[1])
        self.plan_: List[dict] = []
        x, h, w = self.x0, hp, wp
        for blk in self.blocks:
            ho, wo = (h - 1) // blk.stride + 1, (w - 1) // blk.stride + 1
            t1 = self._map(h, w, blk.conv1.cout, blk.conv1.out_q[1], avoid=(x,))
            t2 = self._map(ho, wo, blk.conv2.cout, blk.conv2.out_q[1], avoid=(x, t1))
            out = self._map(ho, wo, blk.cout, blk.out_q[1], avoid=(x, t1, t2))
            ds = None
            if blk.down is not None:
                ds = self._rows.setdefault((n * ho * wo, blk.cout), torch.empty((n * ho * wo, blk.cout), dtype=torch.float32, device=dev))
            self.plan_.append({"x": x, "h": h, "w": w, "ho": ho, "wo": wo, "t1": t1, "t2": t2, "ds": ds, "out": out})
            x, h, w = out, ho, wo
        self.depth = torch.empty((n, self.heads.depth_bins, fh, fw), dtype=torch.float32, device=dev)
        self.feats = torch.empty((n, self.heads.features, fh, fw), dtype=torch.float32, device=dev)

    def _map(self, h, w, c, zp, avoid=()):
        """a padded i8 map [n, h + 2, w + 2, c] whose ring holds ``zp``: one that exists with this shape and zero point and is not live, or a new one"""
        key = (h, w, c, int(zp))
        for t in self._pool.setdefault(key, []):
            if all(t is not a for a in avoid):
                return t
        t = torch.empty((self.n, h + 2, w + 2, c), dtype=torch.int8, device=self.dev)
        t.fill_(int(zp) - 128)
        self._pool[key].append(t)
        return t

    def _conv2(self, layer, x, n, h, w, out):
        launch_conv3x3(self.lib, layer, x, n, h, w, out, layer.out_q)

    def _images(self, imgs):
        if imgs.dim() == 5:
            if tuple(imgs.shape[:2]) != (self.samples, self.views):
                raise ValueError(f"imgs {tuple(imgs.shape)}: [{self.samples}, {self.views}, C, H, W] expected")
            imgs = imgs.view(self.n, *imgs.shape[2:]) if imgs.is_contiguous() else imgs
        if imgs.dim() != 4 or imgs.shape[0] != self.n or imgs.shape[1] < 3 or tuple(imgs.shape[2:]) != (self.h, self.w):
            raise ValueError(f"imgs {tuple(imgs.shape)}: [{self.n}, 3 | 4, {self.h}, {self.w}] expected")
        if imgs.device.type != "cuda" or imgs.dtype != torch.float32 or not imgs.is_contiguous():
            raise ValueError("imgs: a contiguous float32 tensor on the device expected (nothing is copied or converted in a call)")
        return imgs

    # ---- the call ------------------------------------------------------------------------------------------------------------------------
    def plan(self, rots, trans, intrins, post_rots, post_trans):
        self.splat.plan(rots, trans, intrins, post_rots, post_trans)
        return self

    @torch.no_grad()
    def features(self, imgs, taps: Optional[dict] = None):
        """(depth logits f32 [V, D, fH, fW], features f32 [V, C, fH, fW]): the tensors ``GpuLiftSplat`` takes.  ``taps``: padded i8 clones of
        the stem's pooled map (``maxpool``) and of every layer's / block's output under its module name."""
        imgs = self._images(imgs)
        self.stem(imgs, self.x0)
        if taps is not None:
            taps["maxpool"] = self.x0.clone()
        xq = self.stem.out_q
        for blk, p in zip(self.blocks, self.plan_):
            bottleneck_layers(self.lib, blk, self._conv2, p["x"], xq, self.n, p["h"], p["w"], p["ho"], p["wo"], p["t1"], p["t2"], p["ds"], p["out"])
            if taps is not None:
                taps[blk.name + ".conv1"], taps[blk.name + ".conv2"], taps[blk.name] = p["t1"].clone(), p["t2"].clone(), p["out"].clone()
            xq = blk.out_q
        self.heads(self.plan_[-1]["out"], self.depth, self.feats)
        return self.depth, self.feats

    @torch.no_grad()
    def __call__(self, imgs):
        depth, feats = self.features(imgs)
        return self.splat(depth, feats, "logits")

    def capture(self, imgs):
        """one call as a replayable HIP graph on ``imgs`` (refresh its contents in place); ``plan`` first"""
        imgs = self._images(imgs)
        return capture_call(lambda: self(imgs))

    def work_inventory(self) -> dict:
        """Launches and algorithmic work of one call, stage by stage: multiply-accumulates = output pixels x the weight tensor's elements,
        bytes = what a stage must read and write once (codes 1 byte, fp32 maps 4)."""
        s, n = self.state, self.n
        wsize = lambda name: int(np.prod(s[name + "/w_code"].shape))
        hc, wc, hp, wp = stem_shapes(self.h, self.w)
        inv = {"stem": {"launches": 1, "f32_macs": n * hc * wc * wsize("conv1"), "bytes": n * (3 * self.h * self.w * 4 + hp * wp * 64)}}
        for layer, _ in CAMERA_TRUNK:
            macs = nbytes = launches = 0
            for blk, p in zip(self.blocks, self.plan_):
                if not blk.name.startswith(layer + "."):
                    continue
                pin, pout = n * p["h"] * p["w"], n * p["ho"] * p["wo"]
                macs += pin * wsize(blk.name + ".conv1") + pout * (wsize(blk.name + ".conv2") + wsize(blk.name + ".conv3"))
                nbytes += pin * (blk.conv1.cin + blk.conv1.cout) + pin * blk.conv1.cout + pout * blk.conv2.cout * 2 + pout * blk.cout * 2
                launches += 3
                if blk.down is not None:
                    macs += pout * wsize(blk.name + ".downsample")
                    nbytes += pin * blk.conv1.cin + 2 * pout * blk.cout * 4
                    launches += 1
            inv[layer] = {"launches": launches, "int8_macs": macs, "bytes": nbytes}
        pix = n * self.fh * self.fw
        rows = self.heads.depth_bins + self.heads.features
        inv["heads"] = {"launches": 1, "int8_macs": pix * self.heads.cin * rows, "bytes": pix * (self.heads.cin + 4 * rows)}
        inv["splat"] = {"launches": None, "bytes": pix * 4 * rows + int(self.splat.out.numel()) * 4}       # (its own kernels: profiles/lift_splat.json)
        return inv


def deploy_camera_encoder(qt_encoder, views: int, samples: int = 1, device="cuda") -> DeployedCameraEncoder:
    """A calibrated ``QuantLiftSplatShoot`` (the reference's or the plugin's) -> its deployed form for ``samples`` x ``views`` images."""
    return DeployedCameraEncoder(export_camera_state(qt_encoder), views, samples, device)
