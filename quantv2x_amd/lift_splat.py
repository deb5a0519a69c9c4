"""Lift-splat BEV pooling of camera agents: the float64 statements of ``qv2x_lss_plan_f32`` / ``qv2x_lss_splat_f32`` and ``GpuLiftSplat``,
the device stage that stands in for ``get_geometry`` + ``voxel_pooling`` of the reference's ``LiftSplatShoot``
(opencood/models/lift_splat_shoot.py:89-181).  include/qv2x.h has the C contract, DESIGN.md section 13 the reasoning.

What is the reference's and what is this project's:
  * ``create_frustum``, the chain of ``geometry_statement`` (un-augment, ``(u d, v d, d)``, ``rots * intrins^-1``, ``+ trans``), the cell
    expression of ``cells_statement`` with its truncation toward zero, the channel order ``z * C + c`` and the ``[Y, X]`` map are the
    reference's.
  * Evaluating the chain in fp64 from the f32 inputs in one stated order with closed-form inverses and rounding once, dropping points with
    a non-finite coordinate, the flat cell index ``(iz * nx[1] + iy) * nx[0] + ix``, and summing a cell in ascending point index are this
    project's: the reference's f32 ``torch.inverse`` / ``matmul`` depend on the BLAS build and its cumsum differences on the point count.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .plugin.utils.camera_utils import depth_discretization, gen_dx_bx

MAX_VIEWS, MAX_DEPTH_BINS, MAX_FEATURES = 64, 128, 256
MODES = {"logits": 0, "probs": 1}       # QV2X_LSS_LOGITS, QV2X_LSS_PROBS


def _np(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t), dtype=dtype)


def create_frustum(final_dim, downsample, ddiscr, mode) -> torch.Tensor:
    """f32 [D, fH, fW, 3]: per depth bin and feature-map pixel the image coordinates (u, v) of the pixel's sample and the bin's depth.
    ``final_dim`` (H, W) of the network's input image, ``ddiscr`` (min, max, bins), ``mode`` 'UD' or 'LID'."""
    height, width = (int(v) for v in final_dim)
    fh, fw = height // downsample, width // downsample
    bins = torch.tensor(depth_discretization(*ddiscr, mode), dtype=torch.float32)
    out = torch.empty((bins.numel(), fh, fw, 3), dtype=torch.float32)
    out[..., 0] = torch.linspace(0, width - 1, fw, dtype=torch.float32)[None, None, :]          # u: first to last pixel column, both ends included
    out[..., 1] = torch.linspace(0, height - 1, fh, dtype=torch.float32)[None, :, None]         # v: the same over the rows
    out[..., 2] = bins[:, None, None]
    return out


def inv3_statement(a: np.ndarray) -> np.ndarray:
    """float64 [..., 3, 3] -> its inverse as adjugate / determinant, every product, difference and quotient a separate fp64 operation
    (csrc/lift_splat.hip: inv3 has the same lines)."""
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (a[..., i, j] for i in range(3) for j in range(3))
    c00, c01, c02 = a11 * a22 - a12 * a21, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11
    c10, c11, c12 = a12 * a20 - a10 * a22, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12
    c20, c21, c22 = a10 * a21 - a11 * a20, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10
    det = (a00 * c00 + a01 * c10) + a02 * c20
    with np.errstate(all="ignore"):
        rows = [np.stack([c / det for c in r], -1) for r in ((c00, c01, c02), (c10, c11, c12), (c20, c21, c22))]
    return np.stack(rows, -2)


def geometry64_statement(frustum, rots, trans, intrins, post_rots, post_trans) -> np.ndarray:
    """the chain of ``geometry_statement`` before its one rounding: float64 [B, N, D, fH, fW, 3]"""
    f = _np(frustum, np.float32).astype(np.float64)
    r, k, p = (_np(t, np.float32).astype(np.float64) for t in (rots, intrins, post_rots))
    tr, pt = (_np(t, np.float32).astype(np.float64) for t in (trans, post_trans))
    pinv, kinv = inv3_statement(p), inv3_statement(k)
    with np.errstate(all="ignore"):
        m = np.stack([np.stack([(r[..., i, 0] * kinv[..., 0, j] + r[..., i, 1] * kinv[..., 1, j]) + r[..., i, 2] * kinv[..., 2, j]
                                for j in range(3)], -1) for i in range(3)], -2)
        ex = lambda t: t[:, :, None, None, None]                                    # noqa: E731  [B, N] -> [B, N, 1, 1, 1]
        q = [f[None, None, ..., i] - ex(pt[..., i]) for i in range(3)]
        u = [(ex(pinv[..., i, 0]) * q[0] + ex(pinv[..., i, 1]) * q[1]) + ex(pinv[..., i, 2]) * q[2] for i in range(3)]
        w = [u[0] * u[2], u[1] * u[2], u[2]]
        g = [((ex(m[..., i, 0]) * w[0] + ex(m[..., i, 1]) * w[1]) + ex(m[..., i, 2]) * w[2]) + ex(tr[..., i]) for i in range(3)]
    return np.stack(g, -1)


def geometry_statement(frustum, rots, trans, intrins, post_rots, post_trans) -> np.ndarray:
    """f32 [B, N, D, fH, fW, 3]: where every frustum point lies in the ego frame.  ``frustum`` f32 [D, fH, fW, 3]; ``rots``, ``intrins``,
    ``post_rots`` f32 [B, N, 3, 3]; ``trans``, ``post_trans`` f32 [B, N, 3].  Evaluated in fp64 from the f32 inputs, in the order
    include/qv2x.h writes out, and rounded to f32 once."""
    with np.errstate(all="ignore"):
        return geometry64_statement(frustum, rots, trans, intrins, post_rots, post_trans).astype(np.float32)


def cells_statement(geom, dx, bx, nx) -> np.ndarray:
    """i32 [B, N, D, fH, fW]: the flat cell ``(iz * nx[1] + iy) * nx[0] + ix`` of every point, or -1.  ``((g - (bx - dx/2)) / dx)`` in f32
    with gen_dx_bx's f32 ``dx`` / ``bx``, truncated toward zero as ``.long()`` does -- so a coordinate up to one cell below the lower bound
    lands in cell 0 and is kept -- then ``0 <= i < nx`` on all three axes.  A point with a non-finite coordinate is dropped."""
    g = _np(geom, np.float32)
    dx, bx, nx = _np(dx, np.float32), _np(bx, np.float32), _np(nx, np.int64)
    lo = bx - dx / np.float32(2.0)
    with np.errstate(all="ignore"):
        t = np.trunc((g - lo) / dx)                                                 # f32 throughout
        kept = np.isfinite(g).all(-1) & ((t >= 0) & (t < nx.astype(np.float64))).all(-1)
    i = np.where(kept[..., None], t, 0).astype(np.int64)
    cell = (i[..., 2] * nx[1] + i[..., 1]) * nx[0] + i[..., 0]
    return np.where(kept, cell, -1).astype(np.int32)


def depth_probs_statement(depth, mode="logits") -> np.ndarray:
    """float64 [B*N, D, fH, fW]: softmax over D of the f32 logits (the per-pixel maximum subtracted), or the given probabilities"""
    x = _np(depth, np.float32).astype(np.float64)
    if mode == "probs":
        return x
    if mode != "logits":
        raise ValueError(f"mode {mode!r}: 'logits' or 'probs'")
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def splat_terms_statement(cells, depth, feats, mode="logits", *, nx):
    """-> (sum float64 [B, C*Z, Y, X], S float64 of the same shape: the sum of ``|p * f|`` over the cell, n i64 [B, Z, Y, X]: its points).
    The error bound of the fp32 splat is stated in ``S`` and ``n``."""
    cells = _np(cells, np.int64)
    b, n_views, d, fh, fw = cells.shape
    prob = depth_probs_statement(depth, mode).reshape(b, n_views, d, fh, fw)
    f = _np(feats, np.float32).astype(np.float64)
    c = f.shape[1]
    f = f.reshape(b, n_views, c, fh, fw)
    x, y, z = (int(v) for v in _np(nx, np.int64))
    ncell = x * y * z
    total, mag = np.zeros((b, z, c, y * x)), np.zeros((b, z, c, y * x))
    count = np.zeros((b, ncell), np.int64)
    for s in range(b):
        flat = cells[s].reshape(-1)
        kept = flat >= 0
        idx = flat[kept]
        count[s] = np.bincount(idx, minlength=ncell)
        for ch in range(c):
            term = (prob[s] * f[s, :, ch][:, None]).reshape(-1)[kept]               # in ascending point index; fp64 makes the order moot
            total[s, :, ch] = np.bincount(idx, weights=term, minlength=ncell).reshape(z, y * x)
            mag[s, :, ch] = np.bincount(idx, weights=np.abs(term), minlength=ncell).reshape(z, y * x)
    shape = (b, z * c, y, x)
    return total.reshape(shape), mag.reshape(shape), count.reshape(b, z, y, x)


def splat_statement(cells, depth, feats, mode="logits", *, nx) -> np.ndarray:
    """float64 [B, C*Z, Y, X]: per cell the sum of ``prob[p] * feat[pixel(p), c]`` over its points.  ``cells`` i32 [B, N, D, fH, fW] from
    ``cells_statement``; ``depth`` [B*N, D, fH, fW]: logits with ``mode='logits'`` (softmax over D, as ``get_depth_dist``) or probabilities
    with ``mode='probs'`` (``use_gt_depth``'s one-hot); ``feats`` [B*N, C, fH, fW].  Output channel ``z * C + c``, map ``[Y, X]``."""
    return splat_terms_statement(cells, depth, feats, mode, nx=nx)[0]


def splat_bound(count, mag, features, feats_absmax=0.0) -> np.ndarray:
    """the fp32 splat's derived error bound against ``splat_statement``, per element: ``(n + 2) * 2^-24 * S`` plus the
    underflow floor ``n * 2^-126 * (1 + max|f|)`` (a probability below the normal range may be flushed)"""
    n = np.repeat(count, features, axis=1).astype(np.float64)
    return (n + 2.0) * 2.0 ** -24 * mag + n * 2.0 ** -126 * (1.0 + float(feats_absmax))


class GpuLiftSplat:
    """The lift-splat stage on the device for ``samples`` samples of ``views`` cameras each.  The workspace, the cell tensor and the BEV
    output are allocated once; ``plan`` is run when the camera matrices change (per rig, not per frame), a call per frame.

    ``grid_conf`` is the reference's: ``xbound``, ``ybound``, ``zbound``, ``ddiscr``, ``mode``."""

    def __init__(self, grid_conf, final_dim, downsample, features, views, samples=1, device="cuda"):
        from .lib import LssDesc, Qv2xError, load
        lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GpuLiftSplat: a GPU device expected (the CPU statements are geometry_statement / cells_statement / splat_statement)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dx, self.bx, self.nx = gen_dx_bx(grid_conf["xbound"], grid_conf["ybound"], grid_conf["zbound"])
        self.frustum = create_frustum(final_dim, downsample, grid_conf["ddiscr"], grid_conf["mode"]).to(self.device)
        self.samples, self.views, self.features = int(samples), int(views), int(features)
        self.depth_bins, self.fh, self.fw = (int(v) for v in self.frustum.shape[:3])
        d = LssDesc()
        d.samples, d.views, d.depth_bins, d.fh, d.fw, d.features = self.samples, self.views, self.depth_bins, self.fh, self.fw, self.features
        for i in range(3):
            d.nx[i], d.dx[i], d.bx[i] = int(self.nx[i]), float(self.dx[i]), float(self.bx[i])
        self.desc = d
        nbytes = lib.qv2x_lss_workspace_bytes(C.byref(d))
        if nbytes < 0:
            raise Qv2xError("GpuLiftSplat: " + lib.qv2x_last_error().decode(errors="replace"))
        x, y, z = (int(v) for v in self.nx)
        self.workspace = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.int32, device=self.device)
        self.cells = torch.full((self.samples, self.views, self.depth_bins, self.fh, self.fw), -1, dtype=torch.int32, device=self.device)
        self.out = torch.zeros((self.samples, z * self.features, y, x), dtype=torch.float32, device=self.device)
        self.planned = False

    def _arg(self, t, shape, name):
        t = torch.as_tensor(t)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} {tuple(t.shape)}: {shape} expected")
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            if torch.cuda.is_current_stream_capturing():
                raise ValueError(f"{name}: a contiguous float32 tensor on {self.device} expected while the stream is capturing")
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t

    def plan(self, rots, trans, intrins, post_rots, post_trans):
        """camera matrices [samples, views, 3, 3] / [samples, views, 3] -> self; ``self.cells`` then holds every frustum point's cell"""
        from .lib import check, current_stream, load, ptr
        b, n = self.samples, self.views
        rots, intrins, post_rots = (self._arg(t, (b, n, 3, 3), k) for t, k in ((rots, "rots"), (intrins, "intrins"), (post_rots, "post_rots")))
        trans, post_trans = (self._arg(t, (b, n, 3), k) for t, k in ((trans, "trans"), (post_trans, "post_trans")))
        check(load().qv2x_lss_plan_f32(C.byref(self.desc), ptr(self.frustum), ptr(rots), ptr(trans), ptr(intrins), ptr(post_rots), ptr(post_trans),
                                       ptr(self.cells), ptr(self.workspace), current_stream()), "qv2x_lss_plan_f32")
        self.planned = True
        return self

    def __call__(self, depth, feats, mode="logits"):
        """``depth`` f32 [samples * views, D, fH, fW] (the depth head's logits, or probabilities with ``mode='probs'``), ``feats`` f32
        [samples * views, C, fH, fW] -> the BEV tensor f32 [samples, C * Z, Y, X] on the device (the same tensor every call).  Nothing is
        read back: capturable with ``engine.capture_call``."""
        from .lib import Qv2xError, check, current_stream, load, ptr
        if not self.planned:
            raise Qv2xError("GpuLiftSplat: call plan(rots, trans, intrins, post_rots, post_trans) first")
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: 'logits' or 'probs'")
        v = self.samples * self.views
        depth = self._arg(depth, (v, self.depth_bins, self.fh, self.fw), "depth")
        feats = self._arg(feats, (v, self.features, self.fh, self.fw), "feats")
        check(load().qv2x_lss_splat_f32(C.byref(self.desc), ptr(depth), ptr(feats), MODES[mode], ptr(self.workspace), ptr(self.out),
                                        current_stream()), "qv2x_lss_splat_f32")
        return self.out
