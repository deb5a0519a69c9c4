"""``qv2x_range_search_f32`` (csrc/range_search.hip) on the GPU: the reference's own ``mse`` results (tests/golden/uaq_units.npz), the
float64 statement (``quantv2x_amd.calibration.range_search_statement``) at every boundary of the kernel's tiling, determinism, the torch
loops on the tiny model's real tensors, and the full search grid end to end through ``deploy``."""
import time

import numpy as np
import pytest
import torch

from _range_search import FIXTURE_CASES, fixture_case, rows, torch_loop_search

pytestmark = pytest.mark.gpu

# Allowed relative deviation of a loss from the float64 statement: 4 x the largest deviation measured on the five fixture searches
# (MEASURED_LOSS_DEVIATION: profiles/range_search.json "loss_accuracy"), for other tensors and another compiler's
# exp2 / log2.  It has to stay below 1.2e-3, half the smallest top-2 gap of the fixture, or equality with the fixture would mean nothing.
MEASURED_LOSS_DEVIATION = 4.05e-7
LOSS_RTOL = 4 * MEASURED_LOSS_DEVIATION
TILE, CHUNK = 256, 1024                    # candidates per workgroup, floats per staging round (csrc/range_search.hip)

_tally = {"channels": 0, "differing": 0}  # over the edge-shape cases of this file: at most 1 % of the channels may pick another candidate


def _check_against_statement(x, delta, zp, n_levels, name):
    """kernel vs statement on one problem (CPU tensors in): losses within LOSS_RTOL, best equal -- or no worse within LOSS_RTOL"""
    from quantv2x_amd.calibration import range_search_statement, run_range_search
    loss, best = run_range_search(x.cuda(), delta.cuda().contiguous(), zp.cuda().contiguous(), n_levels)
    loss, best = loss.cpu(), best.cpu().long()
    want_loss, want_best = range_search_statement(x, delta, zp, n_levels)
    dev = float(((loss - want_loss).abs() / want_loss.clamp_min(1e-300)).max())
    print(f"{name}: largest relative loss deviation {dev:.3e}")
    assert torch.equal(loss == 0, want_loss == 0), name
    assert dev <= LOSS_RTOL, (name, dev)
    assert int(best.min()) >= 0 and int(best.max()) < delta.shape[0], name
    differ = (best != want_best).nonzero().reshape(-1).tolist()
    for c in differ:
        assert float(want_loss[best[c], c]) <= float(want_loss[want_best[c], c]) * (1 + LOSS_RTOL), (name, c)
    _tally["channels"] += x.shape[0]
    _tally["differing"] += len(differ)
    return loss, best


@pytest.mark.parametrize("tname", list(FIXTURE_CASES))
def test_fixture_ranges_exactly(golden, tname):
    from quantv2x_amd.calibration import candidate_table, gpu_range_search
    from quantv2x_amd.plugin.quant import UniformAffineQuantizer
    x, n_bits, cw, mode, want_delta, want_zp = fixture_case(golden["uaq_units"], tname)
    table_gpu, table_cpu = candidate_table(x.cuda(), n_bits, cw, mode), candidate_table(x, n_bits, cw, mode)
    for g, c in zip(table_gpu, table_cpu):                               # the table does not depend on the device it is built on
        np.testing.assert_array_equal(g.cpu().numpy(), c.numpy())
    lo, hi, loss, best = gpu_range_search(x.cuda(), n_bits, cw, mode, return_losses=True)
    assert lo.is_cuda and tuple(lo.shape) == ((x.shape[0],) if cw else ()) and tuple(loss.shape) == tuple(table_cpu[0].shape)
    # the (delta, zp) the kernel scored lowest ...
    pick = best.reshape(1, -1)
    np.testing.assert_array_equal(table_gpu[2].gather(0, pick).cpu().numpy().reshape(-1), want_delta)
    np.testing.assert_array_equal(table_gpu[3].gather(0, pick).cpu().numpy().reshape(-1), want_zp)
    # ... and what calculate_qparams makes of the returned range where the fixture was recorded, on the CPU (on the GPU torch divides by
    # n_levels - 1 through a reciprocal: the last bit of delta may differ there, for the torch loop's ranges just as for these)
    delta, zp = UniformAffineQuantizer(n_bits=n_bits, channel_wise=cw).calculate_qparams(lo.cpu(), hi.cpu())
    np.testing.assert_array_equal(delta.numpy().reshape(-1), want_delta)
    np.testing.assert_array_equal(zp.numpy().reshape(-1), want_zp)


@pytest.mark.parametrize("tname", list(FIXTURE_CASES))
def test_fixture_through_the_quantizer(golden, tname):
    """the opt-in: a fresh quantizer with search_backend='hip' observing a GPU tensor takes its range from gpu_range_search (the search
    get_x_min_x_max picks on a first observation) and everything after it -- calculate_qparams, the fake quantization -- is its own"""
    from quantv2x_amd.calibration import gpu_range_search
    from quantv2x_amd.plugin.quant import UniformAffineQuantizer
    x, n_bits, cw, mode, want_delta, want_zp = fixture_case(golden["uaq_units"], tname)
    x = x.cuda()
    q = UniformAffineQuantizer(n_bits=n_bits, channel_wise=cw, scale_method="mse", leaf_param=not cw, search_backend="hip")
    q.set_inited(False)
    y = q(x)
    lo, hi = gpu_range_search(x, n_bits, cw, mode)
    if not cw:                                                           # leaf_param: the first observation passes through the EMA
        lo, hi = 0.1 * lo + 0.9 * lo, 0.1 * hi + 0.9 * hi
    delta, zp = q.calculate_qparams(lo, hi)
    assert torch.equal(torch.as_tensor(q.delta).reshape(-1), delta.reshape(-1)) and torch.equal(torch.as_tensor(q.zero_point).reshape(-1), zp.reshape(-1))
    np.testing.assert_allclose(delta.cpu().numpy().reshape(-1), want_delta, rtol=3e-7)       # the last bit: see test_fixture_ranges_exactly
    np.testing.assert_array_equal(zp.cpu().numpy().reshape(-1), want_zp)
    q.set_inited(True)
    assert torch.equal(q(x), y)


def test_loss_accuracy_on_the_fixture(golden):
    """every candidate of the five searches against the float64 statement"""
    from quantv2x_amd.calibration import candidate_table, range_search_statement, run_range_search
    assert 0 < LOSS_RTOL < 1.2e-3
    worst = 0.0
    for tname in FIXTURE_CASES:
        x, n_bits, cw, mode, _, _ = fixture_case(golden["uaq_units"], tname)
        _, _, delta, zp = candidate_table(x, n_bits, cw, mode)
        want, want_best = range_search_statement(rows(x, cw), delta, zp, 2 ** n_bits)
        got, best = run_range_search(rows(x, cw).cuda(), delta.cuda(), zp.cuda(), 2 ** n_bits)
        dev = float(((got.cpu() - want).abs() / want).max())
        print(f"{tname}: largest relative loss deviation {dev:.3e} over {want.numel()} losses")
        assert torch.equal(best.cpu().long(), want_best), tname
        worst = max(worst, dev)
    print(f"largest relative loss deviation on the fixture: {worst:.3e}")
    assert worst <= LOSS_RTOL


def _random_problem(channels, per_channel, candidates, n_levels, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(channels, per_channel, generator=g) * (0.2 + torch.rand(channels, 1, generator=g))
    reach = x.abs().amax(1).clamp_min(0.05).reshape(1, -1)
    delta = reach * (0.3 + 1.7 * torch.rand(candidates, channels, generator=g)) / (n_levels - 1)
    zp = torch.randint(0, n_levels, (candidates, channels), generator=g).float()
    return x.contiguous(), delta.contiguous(), zp.contiguous()


@pytest.mark.parametrize("per_channel", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_edge_row_lengths(per_channel):
    x, delta, zp = _random_problem(3, per_channel, 70, 256, seed=per_channel)
    _check_against_statement(x, delta, zp, 256, f"per_channel={per_channel}")


@pytest.mark.parametrize("candidates", [1, 63, 65, TILE, TILE + 1])
def test_edge_candidate_counts(candidates):
    x, delta, zp = _random_problem(2, 200, candidates, 256, seed=1000 + candidates)
    _, best = _check_against_statement(x, delta, zp, 256, f"candidates={candidates}")
    if candidates == 1:
        assert best.tolist() == [0, 0]


@pytest.mark.parametrize("channels,n_levels", [(1, 4), (300, 16)])
def test_edge_channels_and_levels(channels, n_levels):
    x, delta, zp = _random_problem(channels, 37, 40, n_levels, seed=channels)
    _check_against_statement(x, delta, zp, n_levels, f"channels={channels}, n_levels={n_levels}")


def test_long_row_in_ragged_slices():
    """a per-tensor row over three data slices, the last one ragged: 320 candidates (two tiles), 64 levels"""
    import ctypes as C
    from quantv2x_amd import lib
    from quantv2x_amd.calibration import candidate_table
    n = 2 * CHUNK + 500
    x = torch.randn(1, n, generator=torch.Generator().manual_seed(9))
    _, _, delta, zp = candidate_table(x, 6, False, "2d", num=5)
    d = lib.RangeSearchDesc()
    d.channels, d.candidates, d.n_levels, d.per_channel = 1, 320, 64, n
    assert delta.shape[0] == 320 and lib.load().qv2x_range_search_workspace_bytes(C.byref(d)) == 3 * 320 * 8
    _check_against_statement(x, delta, zp, 64, "three slices")
    # and a longer one, whose slices hold several staging rounds each (139 rounds over 128 slices at most: two per slice, 70 slices)
    n = 138 * CHUNK + 77
    x = torch.randn(1, n, generator=torch.Generator().manual_seed(10)).abs()
    _, _, delta, zp = candidate_table(x, 6, False, "pos", num=5)
    _check_against_statement(x, delta, zp, 64, "seventy slices")


def test_clamped_step_and_all_clipped_channel():
    from quantv2x_amd.calibration import candidate_table
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 50, generator=g)
    x[0] = 0.0                                       # span 0: calculate_qparams clamps every step to 1e-8; every loss is 0
    x[1] *= 1e-9                                     # steps of 1e-11 clamp to 1e-8 too: every candidate is (1e-8, 0), the first one wins
    _, _, delta, zp = candidate_table(x, 4, True, "2d", num=3)
    assert float(delta[:, :2].max()) == np.float32(1e-8) and float(delta[:, 2:].min()) > 1e-8
    loss, best = _check_against_statement(x, delta, zp, 16, "clamped step")
    assert best[:2].tolist() == [0, 0] and float(loss[:, 0].abs().max()) == 0.0
    # a channel every candidate clips entirely: all elements far above every range (codes all 255), and one far below (codes all 0)
    x = torch.cat([10.0 + torch.rand(1, 90, generator=g), -10.0 - torch.rand(1, 90, generator=g)])
    delta = (0.001 + 0.004 * torch.rand(30, 2, generator=g)).contiguous()
    zp = torch.randint(64, 192, (30, 2), generator=g).float()
    _check_against_statement(x, delta, zp, 256, "all clipped")


def test_first_minimum_on_duplicated_rows():
    x, delta, zp = _random_problem(5, 130, 300, 256, seed=77)
    delta, zp = torch.cat([delta, delta, delta[:40]]), torch.cat([zp, zp, zp[:40]])      # 640 rows: every candidate two or three times
    _, best = _check_against_statement(x, delta, zp, 256, "duplicated rows")
    assert int(best.max()) < 300


def test_bit_equal_repeats_and_null_loss():
    from quantv2x_amd.calibration import run_range_search
    x, delta, zp = (t.cuda() for t in _random_problem(7, 3 * CHUNK + 11, 300, 256, seed=123))
    loss0, best0 = (t.clone() for t in run_range_search(x, delta, zp, 256))
    loss1, best1 = (t.clone() for t in run_range_search(x, delta, zp, 256))
    assert torch.equal(loss0.view(torch.int64), loss1.view(torch.int64)) and torch.equal(best0, best1)
    none, best2 = run_range_search(x, delta, zp, 256, want_loss=False)
    assert none is None and torch.equal(best2, best0)


def test_differing_channels_are_rare():
    """over the edge-shape cases above, which pytest runs first (each has asserted that a differing choice is no worse by the statement)"""
    print(f"{_tally['differing']} of {_tally['channels']} channels picked another candidate than the statement")
    assert _tally["differing"] <= 0.01 * _tally["channels"]


_real = []                                  # (name, tensor on the GPU, channel_wise) of the tiny model, collected once


def _real_tensors():
    """every activation quantizer's first input (forward pre-hooks, one scene of two agents on the GPU) and every layer's weight"""
    from _common import act_quantizers, calibrated_plugin, scene
    from quantv2x_amd.plugin.quant import QuantModule
    if not _real:
        qt = calibrated_plugin().cuda()
        seen, hooks = {}, []
        for i, q in enumerate(act_quantizers(qt)):
            hooks.append(q.register_forward_pre_hook(lambda m, args, i=i: seen.setdefault(i, args[0].detach().clone())))
        with torch.no_grad():
            torch.manual_seed(0)
            qt(scene(2, device="cuda"))
        for h in hooks:
            h.remove()
        assert len(seen) >= 10
        _real.extend((f"act{i}", t, False) for i, t in sorted(seen.items()))
        _real.extend((name, m.org_weight.detach().cuda(), True) for name, m in qt.named_modules() if isinstance(m, QuantModule))
        assert len(_real) > len(seen) + 10
    return _real


REAL_PARTS = 8


def _real_part(part):
    """the tensors dealt into REAL_PARTS cases of about equal cost for the torch loop (largest first, each to the lightest case so far)"""
    bins, load = [[] for _ in range(REAL_PARTS)], [0.0] * REAL_PARTS
    for item in sorted(_real_tensors(), key=lambda it: -it[1].numel()):
        j = load.index(min(load))
        bins[j].append(item)
        load[j] += 0.3 + 2e-6 * item[1].numel()
    return bins[part]


@pytest.mark.parametrize("part", range(REAL_PARTS))
def test_real_tensors_both_backends(part):
    """the tiny model's real tensors, an eighth of them per case: the torch loop and the kernel at three range widths return the same
    range, or the float64 statement rates the kernel's no worse than the loop's.
    The loop runs on a CPU copy of the tensor, where it walks the table the kernel scores.  On the GPU torch divides by ``num`` and by
    ``2^n - 1`` through a reciprocal, so the loop there walks neighbouring floats -- of the reference's recorded ranges
    (tests/golden/uaq_units.npz) just as of ``candidate_table``'s -- and two different tables are not what this test compares."""
    from quantv2x_amd.calibration import gpu_range_search, range_search_statement
    from quantv2x_amd.plugin.quant import UniformAffineQuantizer
    tensors = _real_part(part)
    differing = 0
    for name, t, cw in tensors:
        lo_t, hi_t, mode = torch_loop_search(t.cpu(), 8, cw, num=3)
        lo_g, hi_g = (r.cpu() for r in gpu_range_search(t, 8, cw, mode, num=3))
        assert lo_g.shape == lo_t.shape and hi_g.shape == hi_t.shape, name
        same = (lo_g == lo_t) & (hi_g == hi_t)
        if bool(same.all()):
            continue
        differing += 1
        q = UniformAffineQuantizer(n_bits=8, channel_wise=cw)
        pairs = [q.calculate_qparams(lo.reshape(1, -1), hi.reshape(1, -1)) for lo, hi in ((lo_g, hi_g), (lo_t, hi_t))]
        loss, _ = range_search_statement(rows(t, cw), torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs]), 256)
        excess = float((loss[0] / loss[1].clamp_min(1e-300)).max()) - 1.0
        print(f"{name}: {int((~same).sum())} of {same.numel()} ranges differ; the kernel's loss over the loop's, worst channel: 1 {excess:+.3e}")
        assert bool((loss[0] <= loss[1] * (1 + LOSS_RTOL)).all()), (name, excess)
    print(f"{differing} of {len(tensors)} tensors: the kernel and the torch loop returned different ranges")


def test_full_grid_end_to_end():
    """the reference's own grid (100 widths x 256 zero points) on the tiny model: weights, one calibration scene, deploy, one frame
    against the oracle -- the bar of tests/test_hip_deploy_states.py::test_mse_calibrated_state"""
    from _common import build_plugin, compare_frame, scene, scene_np
    from oracle.spec import Oracle
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.plugin.quant import QuantModel, UniformAffineQuantizer, set_weight_quantize_params
    from quantv2x_amd.plugin.tools.inference_quant import calibrate_minmax, quant_params
    from quantv2x_amd.ptq_state import export_ptq_state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wq, aq = quant_params(scale_method="mse", search_backend="hip")
    qt = QuantModel(build_plugin("tiny"), wq, aq).eval().cuda()
    quantizers = [m for m in qt.modules() if isinstance(m, UniformAffineQuantizer)]
    assert all(q.num == 100 and q.search_backend == "hip" for q in quantizers)
    set_weight_quantize_params(qt)
    calibrate_minmax(qt, [scene(2, device="cuda")])
    torch.cuda.synchronize()
    print(f"full-grid mse calibration of the tiny model ({len(quantizers)} quantizers): {time.perf_counter() - t0:.2f} s")
    state = export_ptq_state(qt)
    compare_frame(Oracle(state), deploy(state=state), scene_np(2), state)
