"""The MSE range search of the PTQ observers on the device: ``qv2x_range_search_f32`` (``csrc/range_search.hip``) behind the table of
candidates the reference's loops walk, and the opt-in that sends ``UniformAffineQuantizer``'s searches through it.

``perform_2D_search`` / ``perform_1D_search`` (reference ``opencood/quant/quant_layer.py:201-254``) try ``num`` range widths -- times
``2^n`` zero points in the 2-D case -- one after the other: quantize the tensor, take the mean of ``|x - q|^2.4``, keep the range when the
score is strictly lower than the best so far.  Nothing in a step depends on the step before it, so

* ``candidate_table`` builds all K ranges at once, with the loop's own fp32 expressions (bit-equal to what the loop would walk);
* ``gpu_range_search`` scores them in one kernel call and returns the range of the FIRST least loss -- the loop's result;
* ``range_search_statement`` states the kernel's contract in float64 (the CPU checker).

The losses are summed in fp64 (the loop's are fp32 means): on near-ties the kernel's choice can differ from the loop's, and is then the
better one by the float64 statement.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

MODES = ("2d", "pos", "neg", "sym")
BACKENDS = ("torch", "hip")
_EPS = 1e-8                 # UniformAffineQuantizer.eps


def _observed_range(x, channel_wise, include_zero):
    """``UniformAffineQuantizer._observed_range``"""
    if channel_wise:
        lo, hi = torch.aminmax(torch.flatten(x, 1), dim=1)
        if include_zero:
            hi = torch.max(hi, torch.zeros_like(hi))
            lo = torch.min(lo, torch.zeros_like(lo))
        return lo, hi
    return tuple(torch.aminmax(x))


def _divisor(value, like):
    """``value`` as a one-element f32 tensor next to ``like``.  ``tensor / python_number`` is an IEEE division on the CPU, but on the GPU
    torch multiplies by the number's reciprocal, which differs in the last bit for most operands; a division by a TENSOR is IEEE on both.
    The table is the CPU loop's -- the one the reference's recorded results (tests/golden/uaq_units.npz) come from -- on either device."""
    return torch.full((1,), float(value), dtype=torch.float32, device=like.device)


def _qparams(min_val, max_val, n_levels):
    """``UniformAffineQuantizer.calculate_qparams``, expression for expression (divisions: see ``_divisor``)"""
    eps = torch.tensor(_EPS, dtype=torch.float32)
    lo = torch.min(min_val, torch.zeros_like(min_val))
    hi = torch.max(max_val, torch.zeros_like(max_val))
    scale = torch.max((hi - lo) / _divisor(n_levels - 1, lo), eps)
    zero_point = torch.clamp(0 - torch.round(lo / scale), 0, n_levels - 1)
    return scale, zero_point


def _table(x, n_bits, channel_wise, mode, num):
    if mode not in MODES:
        raise ValueError(f"candidate_table: mode {mode!r}, one of {MODES}")
    if not (2 <= int(n_bits) <= 8) or int(num) < 1:
        raise ValueError("candidate_table: 2 <= n_bits <= 8 and num >= 1")
    x = x.detach().float()
    n_levels = 2 ** int(n_bits)
    x_min, x_max = _observed_range(x, channel_wise, include_zero=(mode == "2d"))
    lo0, hi0 = x_min.reshape(1, -1), x_max.reshape(1, -1)                                  # [1, C]
    i = torch.arange(1, num + 1, dtype=torch.float32, device=x.device).reshape(-1, 1)     # [num, 1]
    zero = torch.zeros_like(lo0)
    if mode == "2d":
        top = (hi0 - lo0) / _divisor(num, x) * i                                           # span / num * i          [num, C]
        step = (top - zero) / _divisor(2 ** int(n_bits) - 1, x)                            # (top - 0) / (2^n - 1)
        zp = torch.arange(0, n_levels, dtype=torch.float32, device=x.device).reshape(1, -1, 1)
        shift = zp * step.unsqueeze(1)                                                     # zp * step               [num, 2^n, C]
        lo = (zero.unsqueeze(1) - shift).reshape(num * n_levels, -1)                       # 0 - zp * step
        hi = (top.unsqueeze(1) - shift).reshape(num * n_levels, -1)                        # top - zp * step
    else:
        thr = torch.max(lo0.abs(), hi0) / _divisor(num, x) * i                             # reach / num * i         [num, C]
        lo = zero.expand_as(thr) if mode == "pos" else -thr
        hi = zero.expand_as(thr) if mode == "neg" else thr
    delta, zpt = _qparams(lo, hi, n_levels)
    return x_min, x_max, lo.contiguous(), hi.contiguous(), delta.contiguous(), zpt.contiguous()


def candidate_table(x, n_bits, channel_wise, mode, num=100):
    """Every range the reference's search would try on ``x``, in its order (``i`` outer, zero point inner), as four f32 ``[K, C]`` tensors
    on ``x``'s device: ``(lo, hi, delta, zp)`` -- the range handed to ``quantize`` and what ``calculate_qparams`` makes of it.  The same
    bits on the CPU and on the GPU: those of the loop on the CPU.  ``mode``:
    ``'2d'`` (``perform_2D_search``, K = num * 2^n_bits) or ``'pos'`` / ``'neg'`` / ``'sym'`` (the branches of ``perform_1D_search``,
    K = num).  C = ``x.shape[0]`` when ``channel_wise`` else 1.  Built by broadcasting, with the loop's fp32 expressions."""
    return _table(x, n_bits, channel_wise, mode, num)[2:]


def range_search_statement(x, delta, zp, n_levels, block=1 << 22):
    """The contract of ``qv2x_range_search_f32`` in float64: ``x`` ``[C, N]`` f32, ``delta`` / ``zp`` ``[K, C]`` f32 ->
    ``(loss [K, C] float64, best [C] int64)``.  ``rint(x / delta)`` is the fp32 division ``torch.round(x / delta)`` rounds; everything after
    it is float64: ``q = (clamp(r + zp, 0, n_levels - 1) - zp) * delta``, ``loss = mean |x - q|^2.4``, ``best`` the first least loss.
    Runs on the tensors' device (any), ``block`` elements at a time."""
    x = torch.as_tensor(x).detach().float()
    delta, zp = torch.as_tensor(delta).detach().float().to(x.device), torch.as_tensor(zp).detach().float().to(x.device)
    if x.dim() != 2 or delta.dim() != 2 or delta.shape != zp.shape or delta.shape[1] != x.shape[0]:
        raise ValueError("range_search_statement: x [C, N], delta and zp [K, C]")
    K, ch = delta.shape
    n = x.shape[1]
    x64 = x.double()
    loss = torch.zeros((K, ch), dtype=torch.float64, device=x.device)
    kb = max(1, int(block // max(1, min(n, block))))               # candidates per step
    nb = min(n, block)                                             # elements per step
    for c in range(ch):
        for k0 in range(0, K, kb):
            d32, z32 = delta[k0:k0 + kb, c].reshape(-1, 1), zp[k0:k0 + kb, c].reshape(-1, 1)
            d64, z64 = d32.double(), z32.double()
            acc = torch.zeros(d32.shape[0], dtype=torch.float64, device=x.device)
            for e0 in range(0, n, nb):
                r = torch.round(x[c, e0:e0 + nb].reshape(1, -1) / d32).double()
                q = (torch.clamp(r + z64, 0, n_levels - 1) - z64) * d64
                acc += (x64[c, e0:e0 + nb].reshape(1, -1) - q).abs().pow(2.4).sum(1)
            loss[k0:k0 + kb, c] = acc / n
    best = torch.from_numpy(np.argmin(loss.cpu().numpy(), axis=0).astype(np.int64).reshape(-1))       # numpy: the first least entry
    return loss, best


_buffers = {}               # (device, channels, candidates, per_channel) -> (workspace u8, loss f64 [K, C], best i32 [C])


def _buffers_for(lib, desc, device):
    key = (str(device), desc.channels, desc.candidates, desc.per_channel)
    hit = _buffers.get(key)
    if hit is None:
        from .lib import Qv2xError
        need = lib.qv2x_range_search_workspace_bytes(C.byref(desc))
        if need < 0:
            raise Qv2xError("qv2x_range_search_workspace_bytes: " + lib.qv2x_last_error().decode(errors="replace"))
        if len(_buffers) >= 64:                                     # a calibration meets a few dozen shapes; do not grow without bound
            _buffers.clear()
        hit = (torch.empty(need, dtype=torch.uint8, device=device),
               torch.empty((desc.candidates, desc.channels), dtype=torch.float64, device=device),
               torch.empty(desc.channels, dtype=torch.int32, device=device))
        _buffers[key] = hit
    return hit


def run_range_search(x2d, delta, zp, n_levels, want_loss=True):
    """One ``qv2x_range_search_f32`` call on ``x2d`` f32 ``[C, N]`` and a table ``delta`` / ``zp`` f32 ``[K, C]`` (all on the GPU, contiguous)
    -> ``(loss f64 [K, C] or None, best i32 [C])``.  The outputs are buffers cached per shape: the next call of that shape overwrites them."""
    from .lib import RangeSearchDesc, check, current_stream, load, ptr
    if not (x2d.is_cuda and delta.is_cuda and zp.is_cuda):
        raise ValueError("run_range_search: tensors on the GPU expected (the CPU statement is range_search_statement)")
    if x2d.dtype != torch.float32 or delta.dtype != torch.float32 or zp.dtype != torch.float32:
        raise ValueError("run_range_search: f32 tensors expected")
    if x2d.dim() != 2 or delta.dim() != 2 or delta.shape != zp.shape or delta.shape[1] != x2d.shape[0]:
        raise ValueError("run_range_search: x [C, N], delta and zp [K, C]")
    if not (x2d.is_contiguous() and delta.is_contiguous() and zp.is_contiguous()):
        raise ValueError("run_range_search: contiguous tensors expected")
    lib = load()
    d = RangeSearchDesc()
    d.channels, d.per_channel, d.candidates, d.n_levels = int(x2d.shape[0]), int(x2d.shape[1]), int(delta.shape[0]), int(n_levels)
    ws, loss, best = _buffers_for(lib, d, x2d.device)
    with torch.cuda.device(x2d.device):
        check(lib.qv2x_range_search_f32(C.byref(d), ptr(x2d), ptr(delta), ptr(zp), ptr(loss if want_loss else None), ptr(best), ptr(ws),
                                        current_stream()), "qv2x_range_search_f32")
    return (loss if want_loss else None), best


def gpu_range_search(x, n_bits, channel_wise, mode, num=100, return_losses=False):
    """``perform_2D_search`` (``mode='2d'``) / ``perform_1D_search`` (``'pos' | 'neg' | 'sym'``) of a ``scale_method='mse'`` quantizer on a
    GPU tensor: ``(best_min, best_max)``, entries of the table's ``lo`` / ``hi``, shaped like the observed minimum (``[C]`` channel-wise, a
    scalar tensor otherwise).  A channel whose least loss is not below 1e10 keeps the observed ``(x_min, x_max)``, the loop's initial
    values.  ``return_losses``: ``(best_min, best_max, loss f64 [K, C], best i64 [C])`` as well."""
    if not x.is_cuda:
        raise ValueError("gpu_range_search: a tensor on the GPU expected (the torch loop of UniformAffineQuantizer serves CPU tensors)")
    x = x.detach().float()
    x_min, x_max, lo, hi, delta, zp = _table(x, n_bits, channel_wise, mode, num)
    x2d = (torch.flatten(x, 1) if channel_wise else x.reshape(1, -1)).contiguous()
    loss, best = run_range_search(x2d, delta, zp, 2 ** int(n_bits))
    pick = best.long().reshape(1, -1)
    found = (loss.gather(0, pick) < 1e10).reshape(x_min.shape)
    best_min = torch.where(found, lo.gather(0, pick).reshape(x_min.shape), x_min)
    best_max = torch.where(found, hi.gather(0, pick).reshape(x_max.shape), x_max)
    if return_losses:
        return best_min, best_max, loss.clone(), best.long()
    return best_min, best_max


def set_search_backend(module, backend):
    """``search_backend`` of every ``UniformAffineQuantizer`` under ``module`` (itself included): ``'hip'`` sends the MSE searches of GPU
    tensors through ``gpu_range_search``, ``'torch'`` (the default) walks the loops.  Returns the number of quantizers set."""
    from .plugin.quant.quant_layer import UniformAffineQuantizer
    if backend not in BACKENDS:
        raise ValueError(f"set_search_backend: {backend!r}, one of {BACKENDS}")
    n = 0
    for m in module.modules():
        if isinstance(m, UniformAffineQuantizer):
            m.search_backend = backend
            n += 1
    return n
