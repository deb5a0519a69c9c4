"""The MSE range search without a GPU: the vectorised candidate table against the table the torch loops walk, the float64 statement of
``qv2x_range_search_f32`` against the reference's own results (tests/golden/uaq_units.npz), the first-minimum rule, and the C entry's
argument checks (answered on the host)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _range_search import FIXTURE_CASES, fixture_case, loop_table, rows

torch.set_num_threads(4)


@pytest.mark.parametrize("tname", list(FIXTURE_CASES))
def test_candidate_table_is_the_loops_table(golden, tname):
    from quantv2x_amd.calibration import candidate_table
    x, n_bits, cw, mode, _, _ = fixture_case(golden["uaq_units"], tname)
    got = candidate_table(x, n_bits, cw, mode)
    want = loop_table(x, n_bits, cw, mode)
    k = 100 * (2 ** n_bits if mode == "2d" else 1)
    for name, g, w in zip(("lo", "hi", "delta", "zp"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == (k, x.shape[0] if cw else 1), name
        np.testing.assert_array_equal(g.numpy(), w.numpy(), err_msg=f"{tname}/{name}")


@pytest.mark.parametrize("mode", ["neg", "sym"])
def test_candidate_table_one_dimensional_branches(mode):
    """the two branches of perform_1D_search the fixture does not take"""
    from quantv2x_amd.calibration import candidate_table
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 40, generator=g)
    if mode == "neg":
        x = -x.abs()
    for cw in (True, False):
        got, want = candidate_table(x, 6, cw, mode, num=7), loop_table(x, 6, cw, mode, num=7)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.numpy(), b.numpy())
    with pytest.raises(ValueError):
        candidate_table(x, 8, True, "3d")


@pytest.mark.parametrize("tname", list(FIXTURE_CASES))
def test_statement_picks_the_references_range(golden, tname):
    from quantv2x_amd.calibration import candidate_table, range_search_statement
    x, n_bits, cw, mode, want_delta, want_zp = fixture_case(golden["uaq_units"], tname)
    _, _, delta, zp = candidate_table(x, n_bits, cw, mode)
    loss, best = range_search_statement(rows(x, cw), delta, zp, 2 ** n_bits)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == tuple(delta.shape) and best.dtype == torch.int64
    pick = best.reshape(1, -1)
    np.testing.assert_array_equal(delta.gather(0, pick).numpy().reshape(-1), want_delta)
    np.testing.assert_array_equal(zp.gather(0, pick).numpy().reshape(-1), want_zp)


def test_statement_first_minimum_and_all_zero():
    from quantv2x_amd.calibration import range_search_statement
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 50, generator=g)
    delta = torch.tensor([[0.5, 0.5], [0.02, 0.03], [0.02, 0.03], [0.5, 0.5], [0.02, 0.03]])
    zp = torch.tensor([[128.0, 128.0], [120.0, 130.0], [120.0, 130.0], [128.0, 128.0], [120.0, 130.0]])
    loss, best = range_search_statement(x, delta, zp, 256)
    assert best.tolist() == [1, 1]                                   # rows 1, 2 and 4 are the same candidate: the lowest index
    assert torch.equal(loss[1], loss[2]) and torch.equal(loss[1], loss[4]) and bool((loss[0] > loss[1]).all())
    loss, best = range_search_statement(torch.zeros(2, 9), delta, zp, 256)
    assert best.tolist() == [0, 0] and float(loss.abs().max()) == 0.0
    # by hand: x = 0.26, delta = 0.1, zp = 1, four levels: round(2.6) = 3, code clamp(4, 0, 3) = 3, q = 0.2, |x - q| = 0.06
    loss, _ = range_search_statement(torch.tensor([[0.26]]), torch.tensor([[0.1]]), torch.tensor([[1.0]]), 4)
    want = abs(float(np.float32(0.26)) - 2.0 * float(np.float32(0.1))) ** 2.4
    assert abs(float(loss) - want) <= 1e-15


def _lib():
    from quantv2x_amd import build, lib
    build.build()
    return lib.load()


def _desc(channels=1, candidates=320, n_levels=64, per_channel=1024):
    from quantv2x_amd import lib
    d = lib.RangeSearchDesc()
    d.channels, d.candidates, d.n_levels, d.per_channel = channels, candidates, n_levels, per_channel
    return d


def test_argument_errors_without_gpu():
    from quantv2x_amd import lib
    l = _lib()
    assert C.sizeof(lib.RangeSearchDesc) == 4 * 4 + 8
    buf = np.zeros(4096, np.uint8)
    p = lib.ptr(buf)

    def call(d, x=p, delta=p, zp=p, loss=p, best=p, ws=p):
        return l.qv2x_range_search_f32(C.byref(d) if d is not None else None, x, delta, zp, loss, best, ws, None)
    for bad, word in ((_desc(channels=0), b"channels"), (_desc(candidates=65537), b"candidates"), (_desc(candidates=0), b"candidates"),
                      (_desc(n_levels=3), b"n_levels"), (_desc(n_levels=257), b"n_levels"), (_desc(per_channel=0), b"per_channel")):
        assert call(bad) == -1 and word in l.qv2x_last_error(), word
        assert l.qv2x_range_search_workspace_bytes(C.byref(bad)) == -1
    assert call(None) == -1 and l.qv2x_range_search_workspace_bytes(None) == -1
    for name in ("x", "delta", "zp", "best", "ws"):
        assert call(_desc(), **{name: None}) == -1 and b"null" in l.qv2x_last_error(), name


def test_workspace_grows_with_the_slices():
    """one row of 320 candidates: a slice per staging chunk of 1024 elements while the row is short, 8 bytes per (slice, candidate)"""
    l = _lib()
    sizes = [l.qv2x_range_search_workspace_bytes(C.byref(_desc(per_channel=n))) for n in (1, 1024, 1025, 2 * 1024 + 500, 64 * 1024)]
    assert sizes == [320 * 8, 320 * 8, 2 * 320 * 8, 3 * 320 * 8, 64 * 320 * 8]
    # many rows fill the GPU by themselves: one slice each
    assert l.qv2x_range_search_workspace_bytes(C.byref(_desc(channels=600, per_channel=64 * 1024))) == 600 * 320 * 8
    # and the cut depends on the descriptor alone: the same answer every time
    assert l.qv2x_range_search_workspace_bytes(C.byref(_desc(per_channel=36044800, candidates=25600, n_levels=256))) == \
        l.qv2x_range_search_workspace_bytes(C.byref(_desc(per_channel=36044800, candidates=25600, n_levels=256))) > 25600 * 8


def test_backend_switch_is_opt_in():
    """nothing changes unless asked: the class default is the torch loop, CPU tensors always take it, the helpers pass the choice on"""
    from quantv2x_amd.calibration import set_search_backend
    from quantv2x_amd.plugin.quant import UniformAffineQuantizer
    from quantv2x_amd.plugin.tools.inference_quant import quant_params
    assert UniformAffineQuantizer.search_backend == "torch" and UniformAffineQuantizer().search_backend == "torch"
    assert quant_params(scale_method="mse") == ({"n_bits": 8, "channel_wise": True, "scale_method": "mse"},
                                                 {"n_bits": 8, "channel_wise": False, "scale_method": "mse", "leaf_param": True, "prob": 0.5})
    wq, aq = quant_params(scale_method="mse", search_backend="hip")
    box = torch.nn.Sequential(UniformAffineQuantizer(**wq), torch.nn.Sequential(UniformAffineQuantizer(**aq)))
    assert [m.search_backend for m in box.modules() if isinstance(m, UniformAffineQuantizer)] == ["hip", "hip"]
    assert set_search_backend(box, "torch") == 2 and box[0].search_backend == "torch"
    with pytest.raises(ValueError):
        set_search_backend(box, "cuda")
    # 'hip' on a CPU tensor: the loop, and the loop's answer
    x = torch.randn(4, 30, generator=torch.Generator().manual_seed(0))
    a, b = UniformAffineQuantizer(n_bits=4, channel_wise=True, scale_method="mse"), UniformAffineQuantizer(n_bits=4, channel_wise=True, scale_method="mse", search_backend="hip")
    for q in (a, b):
        q.num = 3
        q.set_inited(False)
        q(x)
    assert torch.equal(a.delta, b.delta) and torch.equal(a.zero_point, b.zero_point)
