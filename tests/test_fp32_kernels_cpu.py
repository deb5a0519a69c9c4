"""The references of tests/test_hip_fp32_kernels.py pinned, and what every case of tests/_fp32_kernels.py is aimed at asserted on the
reference alone.  No GPU.

  * ``orc_gemm_f32`` against a float64 ``torch.nn.functional.conv2d`` / ``conv_transpose2d`` of the same operands, every case, every output:
    ``|got - ref64| <= (K + 2) 2^-24 (sum_k |x_k w_k| + |bias|)`` with the bracket in float64 -- K roundings of the fma chain, one of the bias
    add, one to spare; ReLU does not widen it.  Nothing here is measured.
  * ``pack_k8`` against its stated layout ``packed[g, col, half, e] == wmat[col, 8 g + 4 half + e]``; ``grouped_slabs`` against a float64
    grouped convolution; ``centre_tap3x3`` against a float64 strided 1x1 convolution.
  * per case: the row count, tile count, column spans and early-returning waves it was written for (``facts`` against ``gemm_facts``); with
    ReLU 20-80 % of the oracle's outputs are exactly 0 and the same layer without ReLU has negative outputs; walking K in natural order changes
    outputs bit-wise, so the bit comparison of the GPU file means something; no output is NaN although every channel outside the window is.
  * ``orc_pfn_f32`` against PillarVFE restated in float64 with a derived bound (``pfn_ref64``), and the constructed pillars: the masked slot
    wins channel CH_MASKED exactly where a slot is masked, channel CH_DEAD is exactly 0, np > P divides by np, no two pillars share a cell.
  * add_relu / occ_sigmoid operands hold the special values; the decode tables are such that another summation order changes outputs.
"""
import numpy as np
import pytest

from _fp32_kernels import (ADD_RELU_COUNTS, CH_DEAD, CH_MASKED, CONV_CASES, DECODE_CASES, DECONV_CASES, GROUP_CG, OCC_SHAPES, OCC_VALUES, PFN_CASES,
                           PFN_N, PFN_NX, PFN_NY, DecodePrepared, GemmPrepared, PfnPrepared, add_relu_operands, gemm_facts, natural_order,
                           occ_operands, occ_score64, pfn_inside, pfn_ref64, ref64)

GEMM = [("conv", k) for k in CONV_CASES] + [("deconv", k) for k in DECONV_CASES]
_PREP = {}


def prepared(kind, name):
    if (kind, name) not in _PREP:
        _PREP[kind, name] = GemmPrepared((CONV_CASES if kind == "conv" else DECONV_CASES)[name])
    return _PREP[kind, name]


@pytest.mark.parametrize("kind,name", GEMM)
def test_orc_gemm_f32_against_float64_torch(kind, name):
    p = prepared(kind, name)
    case = p.case
    for i, l in enumerate(case.layers):
        y, bound = ref64(p.x[i], l, case.deconv, p.wmat[i], p.bias[i], case.relu)
        err = np.abs(p.want[i].astype(np.float64) - y)
        assert np.isfinite(err).all()
        worst = float((err / bound).max())
        print(f"{kind} {name} layer {i}: largest error / bound = {worst:.3f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("kind,name", GEMM)
def test_gemm_case_aims_hold_on_the_oracle(kind, name):
    p = prepared(kind, name)
    case = p.case
    assert case.aim
    got = gemm_facts(case)
    for k, v in case.facts.items():
        assert got[k] == v, f"{k}: the case was written for {v}, the shapes give {got[k]}"
    assert all(nc % 64 == 0 for nc in got["ncols"]) and all(l.cin % 8 == 0 and l.cin0 % 4 == 0 for l in case.layers)
    changed = 0.0
    for i, l in enumerate(case.layers):
        want, norelu = p.want[i], p.want_norelu[i]
        assert np.isfinite(want).all() and np.isfinite(norelu).all()
        if case.relu:
            zeros = float((want == 0).mean())
            assert 0.2 <= zeros <= 0.8, f"layer {i}: {zeros:.3f} of the oracle's outputs are exactly 0"
        assert (norelu < 0).mean() >= 0.2, f"layer {i}: the layer without ReLU has too few negative outputs"
        nat = natural_order(p.x[i], l, case.deconv, p.wmat[i], p.bias[i], 0)
        np.testing.assert_allclose(nat, norelu, rtol=0, atol=float(2.0 ** -20 * (np.abs(norelu).max() + 8)))      # the same sums
        changed = max(changed, float((nat.view(np.uint32) != norelu.view(np.uint32)).mean()))
    print(f"{kind} {name}: K in natural order changes {changed:.3f} of the outputs bit-wise")
    assert changed >= 0.02
    # the expected destination: windows finite, everything else the sentinel
    inner = p.expect[:, 1:-1, 1:-1, case.front:p.expect.shape[-1] - case.back]
    assert np.isfinite(inner).all() and (inner != p.expect[0, 0, 0, 0]).all()


def test_gemm_case_lists_hold_what_the_gpu_file_is_meant_to_run():
    conv, dec = list(CONV_CASES.values()), list(DECONV_CASES.values())
    f = [gemm_facts(c) for c in conv]
    assert {m for x in f for m in x["M"]} >= {1, 15, 32, 33, 42}
    assert any(x["spans_images"] for x in f) and any(x["early_return"] and max(x["tiles"]) > 4 for x in f)
    assert {(l.h, l.w) for c in conv for l in c.layers if l.stride == 2} >= {(4, 6), (5, 7), (1, 1), (2, 1)}
    assert {l.cin for c in conv for l in c.layers} >= {8, 24, 64} and {l.cout for c in conv for l in c.layers} >= {64, 128, 192}
    assert any((l.cin_total, l.cin0, l.cin) == (40, 12, 24) for c in conv for l in c.layers)
    assert any(c.front % 4 for c in conv) and any(c.front == 0 for c in conv) and {c.relu for c in conv} == {0, 1}
    assert any(l.form == "centre" and l.stride == 2 for c in conv for l in c.layers) and any(l.form == "slab" for c in conv for l in c.layers)
    assert {(l.stride, l.cout) for c in dec for l in c.layers} >= {(1, 64), (1, 128), (2, 16), (2, 32), (2, 48), (3, 64), (4, 4), (4, 20), (8, 1)}
    g = [gemm_facts(c) for c in dec]
    assert {m for x in g for m in x["M"]} >= {1, 15, 32, 33, 42} and any(x["spans_images"] for x in g)
    assert any(len(c.layers) == 2 and c.layers[0].stride != c.layers[1].stride for c in dec)
    assert any(l.cin0 % 8 == 4 for c in dec for l in c.layers) and {c.relu for c in dec} == {0, 1}


def test_pack_k8_layout():
    from quantv2x_amd.engine_fp32 import pack_k8
    rng = np.random.default_rng(5)
    for cols, k in ((64, 8), (192, 72), (64, 216)):
        wmat = rng.standard_normal((cols, k)).astype(np.float32)
        packed = pack_k8(wmat)
        assert packed.shape == (k // 8, cols, 2, 4) and packed.dtype == np.float32 and packed.flags["C_CONTIGUOUS"]
        g, col, half, e = np.meshgrid(np.arange(k // 8), np.arange(cols), np.arange(2), np.arange(4), indexing="ij")
        np.testing.assert_array_equal(packed, wmat[col, 8 * g + 4 * half + e])


def test_grouped_slabs_and_centre_tap_against_float64_torch():
    import torch
    import torch.nn.functional as F
    p = prepared("conv", "grouped_slabs")
    x = torch.from_numpy(p.x[0].astype(np.float64)).permute(0, 3, 1, 2)
    c = p.x[0].shape[-1]
    bias = torch.from_numpy(np.concatenate(p.bias).astype(np.float64))
    y = F.conv2d(x, torch.from_numpy(p.wgroup.astype(np.float64)), bias, padding=1, groups=c // GROUP_CG).clamp_min(0).permute(0, 2, 3, 1).numpy()
    got = np.concatenate(p.want, axis=-1)
    mag = F.conv2d(x.abs(), torch.from_numpy(np.abs(p.wgroup).astype(np.float64)), bias.abs(), padding=1, groups=c // GROUP_CG).permute(0, 2, 3, 1).numpy()
    assert (np.abs(got - y) <= (9 * 64 + 2) * 2.0 ** -24 * mag).all()          # the dense chain walks all 576 k; the zeros add nothing to mag
    p = prepared("conv", "centre_tap_s2")
    l = p.case.layers[0]
    x = torch.from_numpy(p.x[0].astype(np.float64)).permute(0, 3, 1, 2)
    w, b = torch.from_numpy(p.wtorch[0].astype(np.float64)), torch.from_numpy(p.bias[0].astype(np.float64))
    y = F.conv2d(x, w, b, stride=2).permute(0, 2, 3, 1).numpy()
    mag = F.conv2d(x.abs(), w.abs(), b.abs(), stride=2).permute(0, 2, 3, 1).numpy()
    assert y.shape == p.want[0].shape and (np.abs(p.want[0] - y) <= (9 * l.cin + 2) * 2.0 ** -24 * mag).all()


# ---- PFN ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PFN_CASES))
def test_orc_pfn_f32_against_float64_pillar_vfe(name):
    p = PfnPrepared(PFN_CASES[name])
    y, bound = pfn_ref64(p)
    err = np.abs(p.feats.astype(np.float64) - y)
    print(f"{name}: largest error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    P = p.case.P
    for i, pil in enumerate(p.case.pillars):
        masked = pil[4] < P
        assert p.feats[i, CH_DEAD] == 0.0
        if masked:
            assert p.feats[i, CH_MASKED] == p.b[CH_MASKED], "the masked slot must win this channel"
        else:
            assert 0.0 <= p.feats[i, CH_MASKED] < p.b[CH_MASKED]
    assert ((p.feats > 0).mean(axis=1) > 0.3).all()                       # every pillar has live channels: a skipped pillar would show


def test_pfn_cases_are_what_they_say():
    assert {(len(c.pillars), c.P) for c in PFN_CASES.values()} >= {(1, 1), (5, 5), (9, 32)}
    assert {len(c.pillars) % 4 for c in PFN_CASES.values()} >= {1, 0}
    e = PFN_CASES["edges_p5"]
    assert e.pillars[0][4] == 1 and e.pillars[1][4] == e.P and e.pillars[2][4] > e.P and e.pillars[3][1] == 1
    inside = [p for p in e.pillars if pfn_inside(p)]
    outside = [p[:4] for p in e.pillars if not pfn_inside(p)]
    last = PFN_N - 1
    assert {(b, y, z + x) for (b, z, y, x, _n) in inside} >= {(last, 0, 0), (last, 0, PFN_NX - 1), (last, PFN_NY - 1, 0), (last, PFN_NY - 1, PFN_NX - 1)}
    assert {p[0] for p in outside} >= {-1, PFN_N} and {p[2] for p in outside} >= {-1, PFN_NY} and {p[1] + p[3] for p in outside} >= {-1, PFN_NX}
    assert all(sum([not 0 <= p[0] < PFN_N, not 0 <= p[2] < PFN_NY, not 0 <= p[1] + p[3] < PFN_NX]) == 1 for p in outside)    # one side each
    prep = PfnPrepared(e)
    assert len(prep.cells) == len(inside) == 8
    # np > P: the mean divides by the reported count.  With np clamped to P the mean features differ, and so do the outputs
    clamped = PfnPrepared(e)
    from oracle.spec import _p, lib as olib
    npts = np.minimum(clamped.npts, e.P).astype(np.int32)
    other = np.zeros_like(clamped.feats)
    olib().orc_pfn_f32(_p(clamped.vf), _p(clamped.coords), _p(npts), len(e.pillars), e.P, _p(clamped.w), _p(clamped.b),
                       _p(np.array([0.4, 0.4, 4.0], np.float32)), _p(np.array([-1.0, -0.6, -1.0], np.float32)), _p(other))
    assert (other[2] != prep.feats[2]).mean() > 0.3 and (np.delete(other, 2, axis=0) == np.delete(prep.feats, 2, axis=0)).all()
    # the expected canvas: exactly the eight cells differ from the fill, ring included
    canvas = prep.canvas(-5.0)
    assert int((canvas != -5.0).any(axis=-1).sum()) == 8 and (canvas[:, 0] == -5.0).all() and (canvas[:, :, -1] == -5.0).all()


# ---- add_relu, occ_sigmoid, decode ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", ADD_RELU_COUNTS)
def test_add_relu_operands(count):
    a, b = add_relu_operands(count)
    assert a.size == b.size == count and count % 4 == 0
    with np.errstate(over="ignore"):
        s = a + b
    assert not np.isnan(s).any()
    assert ((a != 0) & (s == 0)).any(), "exact cancellation"
    assert (np.signbit(a) & np.signbit(b) & (a == 0) & (b == 0)).any(), "-0.0 + -0.0"
    assert np.isposinf(a).any() and np.isneginf(a).any()
    if count > 16:
        assert np.isposinf(s[np.isfinite(a) & np.isfinite(b)]).any() and np.isneginf(s[np.isfinite(a) & np.isfinite(b)]).any(), "overflowing sums"
        assert 0.3 < (s < 0).mean() < 0.7


@pytest.mark.parametrize("name", list(OCC_SHAPES))
def test_occ_operands(name):
    n, h, w, ct = OCC_SHAPES[name]
    x, v = occ_operands(n, h, w, ct)
    assert np.isnan(x[:, 0]).all() and np.isnan(x[:, -1]).all() and np.isnan(x[:, :, 0]).all() and np.isnan(x[:, :, -1]).all()
    assert np.isnan(x[..., 1:]).all() and not np.isnan(x[:, 1:-1, 1:-1, 0]).any()
    bits = set(v.view(np.uint32).tolist())
    assert bits >= set(np.array(OCC_VALUES, np.float32).view(np.uint32).tolist())
    s = occ_score64(v)
    assert np.isfinite(s).all() and (s >= np.float32(1e-4)).all() and (s <= np.float32(1.0001)).all()
    assert s[v == np.float32(-1e30)][0] == np.float32(1e-4) and s[v == np.float32(1e30)][0] == np.float32(1.0001)
    if name == "n1_1x257_c4":
        assert n * h * w == 257


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_decode_cases(name):
    p = DecodePrepared(DECODE_CASES[name])
    c = p.case
    assert c.aim and c.d % 4 == 0 and c.work % 256 != 0
    assert p.idx.min() == 0 and p.idx.max() == c.kc - 1
    for l in range(c.levels):
        assert set(p.idx[:, :, l].ravel().tolist()) & {0, c.kc - 1}
    want = p.want()
    assert np.isfinite(want).all()
    if c.levels > 1:
        other = p.want(order=list(range(c.levels))[::-1])
        changed = float((other.view(np.uint32) != want.view(np.uint32)).mean())
        print(f"{name}: summing the levels in reverse changes {changed:.3f} of the outputs bit-wise")
        assert changed > 0.1
    if c.layout == "agent_major":
        assert c.agent_stride > c.levels * c.level_stride > c.levels * c.hw


def test_decode_case_list():
    cs = DECODE_CASES.values()
    assert {c.d for c in cs} >= {4, 64, 68, 256} and {c.levels for c in cs} >= {1, 3, 16} and {c.kc for c in cs} >= {1, 128, 256}
    assert {c.layout for c in cs} == {"engine", "agent_major"}
