"""Shared by tests/test_range_search_cpu.py and tests/test_hip_range_search.py: the five ``mse`` searches pinned in
tests/golden/uaq_units.npz, and the table of candidates collected from the torch loops of ``UniformAffineQuantizer`` themselves."""
import torch

from quantv2x_amd.plugin.quant import UniformAffineQuantizer

# tensor -> (channel_wise, mode): what the first observation of a fresh quantizer takes (get_x_min_x_max); the bit width is the fixture's
FIXTURE_CASES = {"conv": (True, "2d"), "deconv": (True, "2d"), "linear": (True, "2d"), "act_pos": (False, "pos"), "act_signed": (False, "2d")}


def fixture_case(g, tname):
    """(x f32 tensor, n_bits, channel_wise, mode, delta [C], zp [C]) of one pinned search"""
    cw, mode = FIXTURE_CASES[tname]
    k = f"{tname}/mse"
    return torch.from_numpy(g["in/" + tname]), int(g[k + "/n_bits"]), cw, mode, g[k + "/delta"], g[k + "/zp"]


def rows(x, channel_wise):
    """the tensor as the kernel reads it: [C, N]"""
    return (torch.flatten(x, 1) if channel_wise else x.reshape(1, -1)).contiguous()


class _Recorder(UniformAffineQuantizer):
    """the quantizer with ``quantize`` replaced by a note of the range it was handed (and an error-free answer: the walk is all we want)"""

    def quantize(self, x, x_max, x_min):
        delta, zp = self.calculate_qparams(x_min, x_max)
        self.seen.append([t.detach().clone().reshape(-1) for t in (x_min, x_max, delta, zp)])
        return x


def loop_table(x, n_bits, channel_wise, mode, num=100):
    """(lo, hi, delta, zp) [K, C] as ``perform_2D_search`` / ``perform_1D_search`` hand them to ``quantize``, in the order they do"""
    q = _Recorder(n_bits=n_bits, channel_wise=channel_wise, scale_method="mse", leaf_param=not channel_wise)
    q.num, q.seen = num, []
    if mode == "2d":
        q.perform_2D_search(x)
    else:
        q.one_side_dist = mode if mode in ("pos", "neg") else "no"
        q.perform_1D_search(x)
    return tuple(torch.stack([s[j] for s in q.seen]) for j in range(4))


def torch_loop_search(x, n_bits, channel_wise, num):
    """(lo, hi, mode) of the untouched torch loops on ``x``, the way ``get_x_min_x_max`` picks the search on a first observation"""
    q = UniformAffineQuantizer(n_bits=n_bits, channel_wise=channel_wise, scale_method="mse", leaf_param=False)
    q.num = num
    q.one_side_dist = 'pos' if x.min() >= 0.0 else 'neg' if x.max() <= 0.0 else 'no'
    if q.one_side_dist != 'no':
        return (*q.perform_1D_search(x), q.one_side_dist)
    return (*q.perform_2D_search(x), "2d")
