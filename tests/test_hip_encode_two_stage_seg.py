"""The two-stage EXACT encode for segmented and 256-entry codebooks on the GPU: ``(seg_num, dict_size)`` = (2, 256) -- six of the reference's
ten codebook yamls -- and (1, 256).  Stage 1 is the kernel of csrc/codebook_encode_cand.hip through its second entry, packed score
256 S + k (qv2x_codebook_encode_candidates_seg_i8), stage 2 the widened qv2x_codebook_encode_listed_f32; theory and operands: quantv2x_amd/encode_two_stage.py, pinned on the CPU by
tests/test_encode_two_stage_seg_cpu.py.  Every count here is zero: exactness has no tolerance.

  * the default mode of such an engine is ``"two_stage"``, and ``two_stage == exact == Oracle.encode_rows`` on all ``levels * seg_num`` planes
    of the reference's 35 200 golden rows;
  * stage 1 alone equals ``candidate_emulate`` bit for bit: every candidate index of every cell, the listed set, the three per-level counts
    (``assert_stage1_is_the_emulation`` of tests/test_hip_encode_two_stage.py, on the entry the engine calls);
  * both cell-tile forms of the kernel on a ragged launch, tiny frames through the model call, replay from a HIP graph on fresh rows;
  * stage 2 alone on constructed lists; a full bench batch of 32 frames; the refusals of the new entry."""
import copy

import numpy as np
import pytest
import torch

from test_codebook_full_golden import golden_rows
from test_hip_encode_two_stage import assert_stage1_is_the_emulation, put_rows, run_modes, v2xreal_engine

pytestmark = pytest.mark.gpu

SHAPES = [(2, 256), (1, 256)]
_STATES = {}


def seg_state(m, k):
    from _common import calibrated_plugin
    from quantv2x_amd.ptq_state import export_ptq_state
    if (m, k) not in _STATES:
        _STATES[(m, k)] = export_ptq_state(calibrated_plugin("tiny", dict_size=k, seg_num=m))
    return _STATES[(m, k)]


@pytest.mark.parametrize("m,k", SHAPES)
def test_golden_rows_default_mode_two_stage_equals_exact_and_oracle(golden, m, k):
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(seg_state(m, k), g)
    assert (eng.segs, eng.kc, eng.levels) == (m, k, 3 * m)
    assert eng.encode_mode == "two_stage" and eng.two_stage_refused is None, (eng.encode_mode, eng.two_stage_refused)
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert got["exact"].shape == want.shape == (3 * m, 35200)
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"({m}, {k}) two-stage encode: {mism} indices differ from the oracle"
    e_flag, first = assert_stage1_is_the_emulation(eng, 1, codes_u8, g["in_delta"], g["in_zp"])
    stats = eng.encode_refine_stats(1)
    print(f"two-stage encode ({m}, {k}) on the golden rows:", stats)
    assert stats["refined"] == int(e_flag.sum()) and stats["first_flagged_at_level"] == [int(f.sum()) for f in first]
    assert 0.01 < stats["refined_fraction"] <= (0.25 if m == 2 else 0.15)


@pytest.mark.parametrize("m,k", [(2, 128), (1, 192)])
def test_other_shapes_the_same_code_takes(golden, m, k):
    """shapes that fall out of the same code (kc is a run-time argument of both stages): default mode, two_stage == exact == oracle on the
    golden rows, stage 1 == the emulation"""
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(seg_state(m, k), g)
    assert (eng.segs, eng.kc) == (m, k) and eng.encode_mode == "two_stage" and eng.two_stage_refused is None
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"({m}, {k}) two-stage encode: {mism} indices differ from the oracle"
    e_flag, _ = assert_stage1_is_the_emulation(eng, 1, codes_u8, g["in_delta"], g["in_zp"])
    assert 0 < e_flag.sum() < len(e_flag)


def _big_launches(ct_big):
    """100 x 348 = 34 800 cells per frame: no launch is a whole number of workgroups; the frame counts on both sides of the switch to the
    large cell tile (M >= 4 * CUs * 32 * ct_big * 2)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cells = 100 * 348
    switch = 4 * cus * 32 * ct_big * 2
    return cells, switch, -(-switch // cells)


@pytest.mark.parametrize("m,k,ct_big", [(2, 256, 3), (1, 256, 4)])
@pytest.mark.parametrize("side", ["large_tile", "two_tiles_just_below"])
def test_candidate_seg_kernel_both_tile_forms_at_a_ragged_launch(golden, side, m, k, ct_big):
    """Every cell-tile form of the kernel at 256 S + k: ``encode_candidates_kernel<3, 2, 256>`` (the bench batch's form) and ``<4, 1, 256>`` (a
    batch of a (1, 256) engine, eight frames or more) at the switch, ``<2, 2, 256>`` and ``<2, 1, 256>`` just below it, on launches whose last workgroup is
    partial: stage 1 == the emulation on EVERY cell, two_stage == exact."""
    import _encode_families as F
    from quantv2x_amd.engine import deploy
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    fam = F.family("base", seg_state(m, k), g)
    cells, switch, n_hi = _big_launches(ct_big)
    n = n_hi if side == "large_tile" else n_hi - 1
    assert n >= 1 and (n * cells >= switch) == (side == "large_tile")
    assert (n * cells) % (128 * ct_big if side == "large_tile" else 256) != 0   # (a partial last workgroup: 32 ct_big | 64 cells per wave)
    eng = deploy(state=F.deployable(fam, (696, 200, 1)))
    eng._workspace(n)
    assert (eng.fh, eng.fw) == (100, 348) and eng.encode_mode == "two_stage" and (eng.segs, eng.kc) == (m, k)
    rows = F.frame_rows(codes_u8, eng._two_stage[4], fam.in_zx, n * cells)
    put_rows(eng, n, rows)
    got = run_modes(eng, n)
    mism = int((got["two_stage"] != got["exact"]).sum())
    assert mism == 0, f"{mism} indices of {n} frames differ between the two-stage and the exact encode"
    assert_stage1_is_the_emulation(eng, n, rows, fam.in_delta, fam.in_zx)


@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("n_agents", [1, 2, 3])
def test_tiny_frames_through_the_model_call(m, k, n_agents):
    """whole frames at tiny shape through the model call: the two-stage engine's output dict equals the exact engine's bit for bit"""
    from _common import calibrated_plugin, scene_np
    from oracle.spec import Oracle
    from quantv2x_amd import synth
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.ptq_state import export_ptq_state
    state = export_ptq_state(calibrated_plugin("tiny", n_agents=2, dict_size=k, seg_num=m))
    eng = deploy(state=state)
    sc = scene_np(n_agents, seed=13)
    dd = synth.scene_to_torch(sc, "cuda")
    eng.encode_mode = "exact"
    te = {}
    want = {key: v.clone() for key, v in eng(dd, te).items()}
    exact_codes = te["codes"].clone()
    eng.encode_mode = "two_stage"
    tt = {}
    got = eng(dd, tt)
    torch.cuda.synchronize()
    assert eng.encode_mode == "two_stage" and eng.two_stage_refused is None
    assert torch.equal(tt["codes"], exact_codes)
    for key in want:
        assert torch.equal(got[key], want[key]), key
    ot = {}
    Oracle(state).forward(sc, ot)
    assert np.array_equal(tt["codes"].cpu().numpy().reshape(ot["codes"].shape), ot["codes"])


def test_graph_replay_on_fresh_rows(golden):
    """both launches (and the counter reset) inside ONE HIP graph: replayed on rows written after the capture, the indices follow the rows"""
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(seg_state(2, 256), g)
    assert eng.encode_mode == "two_stage"
    put_rows(eng, 1, codes_u8)
    eng.encode_codes(1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        eng.encode_codes(1)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = eng.encode_codes(1)
    torch.cuda.synchronize()
    orc = Oracle(st)
    for shift in (0, 17):
        fresh = np.roll(codes_u8, shift, axis=1)
        put_rows(eng, 1, fresh)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = orc.encode_rows((fresh.astype(np.float32) - np.float32(g["in_zp"])) * np.float32(g["in_delta"]))
        assert np.array_equal(out.cpu().numpy().reshape(6, -1), want), shift
        assert eng.encode_refine_stats(1)["refined"] > 0


@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("counts", [(31, 0, 0), (1000, 12000, 19730), (40, 511 * 32, 1024 * 32 - 7), (70400, 0, 0), (5, 7, 70388)])
def test_stage2_alone_on_constructed_lists(golden, m, k, counts):
    """qv2x_codebook_encode_listed_f32 by itself for two segments / 256 codes on lists of chosen lengths (the workgroup form alone, whole
    rounds of persistent waves + a remainder, every cell of two frames in one list).  The listed cells' planes from their list's LEVEL on are
    overwritten with garbage first: stage 2 must restore the every-cell kernel's indices using the ``seg_num`` STORED codes of every level
    below, and leave every other cell untouched."""
    import ctypes as C
    from quantv2x_amd import lib as L
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    st, eng = v2xreal_engine(seg_state(m, k), g)
    n = 2
    rng = np.random.default_rng(5)
    rows = np.concatenate([codes_u8, np.roll(codes_u8, 7, axis=0)[:, rng.permutation(256)]])
    b = put_rows(eng, n, rows)
    eng.encode_mode = "exact"
    ref = eng.encode_codes(n).clone()
    torch.cuda.synchronize()
    m_cells = n * eng.fh * eng.fw
    assert sum(counts) <= m_cells
    eng.encode_mode = "two_stage"
    eng.encode_codes(n)                                                 # (allocates the list buffers)
    cells = torch.from_numpy(rng.permutation(m_cells)[:sum(counts)].astype(np.int32)).cuda()
    work = ref.clone().reshape(eng.levels, m_cells)
    lst, cnt, at = b["enc_list"], b["enc_counters"], 0
    lst.fill_(-1)
    for c, kk in enumerate(counts):
        mine = cells[at:at + kk]
        lst[c * m_cells:c * m_cells + kk] = mine
        for p in range(c * m, eng.levels):
            work[p, mine.long()] = 255 - p
        at += kk
    untouched = torch.ones(m_cells, dtype=torch.bool, device="cuda")
    untouched[cells.long()] = False
    before = work[:, untouched].clone()
    cnt.copy_(torch.tensor([sum(counts), *counts], dtype=torch.int32))
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = n, eng.fh, eng.fw, eng.enc_levels, eng.kc, eng.segs
    d.in_zx, d.in_delta = int(eng.shrink1.out_q[1]), float(eng.shrink1.out_q[0])
    L.check(eng.lib.qv2x_codebook_encode_listed_f32(C.byref(d), L.ptr(b["s1"]), eng.level_ptrs, L.ptr(lst), L.ptr(cnt), L.ptr(work), L.current_stream()), "listed")
    torch.cuda.synchronize()
    bad = (work != ref.reshape(eng.levels, m_cells)).sum().item()
    assert bad == 0, f"({m}, {k}): {bad} indices differ after stage 2 on lists of {counts} cells"
    assert torch.equal(work[:, untouched], before)


def test_full_bench_batch_two_stage_equals_exact():
    """32 V2X-Real frames of a (2, 256) engine on a synthetic scene, ``two_stage`` against ``exact``: 0 of 6 x 32 x 35 200 indices differ"""
    from quantv2x_amd import synth
    from quantv2x_amd.engine import deploy
    st = copy.copy(seg_state(2, 256))
    st["meta/grid"] = np.array(synth.grid_size(*synth.SHAPES["v2xreal"][:2]), dtype=np.int64)
    eng = deploy(state=st)
    n = 32
    eng(synth.scene_to_torch(synth.make_scene("v2xreal", n_agents=1, seed=3), "cuda"), {})      # one frame through the model call
    torch.cuda.synchronize()
    b1 = eng._workspace(1)
    assert (eng.fh, eng.fw) == (100, 352) and int((b1["s1"][0, 1:-1, 1:-1] != b1["s1"][0, 1, 1]).sum()) > 0
    b = eng._workspace(n)
    rng = np.random.default_rng(2)
    for i in range(n):                                                   # the frame's real shrinker output, its channels rotated per frame
        b["s1"][i] = torch.roll(b1["s1"][0], int(rng.integers(0, 256)), dims=-1)
    assert eng.encode_mode == "two_stage" and eng.two_stage_refused is None
    got = {}
    for mode in ("exact", "two_stage"):
        eng.encode_mode = mode
        got[mode] = eng.encode_codes(n).clone()
    torch.cuda.synchronize()
    assert got["exact"].numel() == 6 * 32 * 35200
    mism = int((got["exact"] != got["two_stage"]).sum().item())
    stats = eng.encode_refine_stats(n)
    print("two-stage encode (2, 256), 32 frames:", stats)
    assert mism == 0, f"{mism} of {got['exact'].numel()} indices differ"
    assert 0 < stats["refined"] < stats["cells"]


def test_refusals_of_the_segment_entry():
    import ctypes as C
    from quantv2x_amd import lib as L
    lib = L.load()
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = 1, 4, 4, 3, 256, 2
    d.in_zx, d.in_delta = 0, 1.0
    assert lib.qv2x_codebook_encode_candidates_seg_i8(C.byref(d), None, None, None, None, None, None, None, None, None) != 0
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    tau = (C.c_float * 9)()
    p = buf.data_ptr()                                                   # (a plain integer: p + 8 is a misaligned address)
    call = lambda *ptrs: lib.qv2x_codebook_encode_candidates_seg_i8(C.byref(d), *ptrs, None)
    ok = (p, p, p, p, tau, p, p, p)
    # (seg_num * dict_size > 512 cannot be reached past "seg_num <= 2" and "dict_size <= 256": (384, 2) and (256, 4) are refused by those)
    for kc, segs in ((288, 1), (256, 3), (256, 4), (384, 2), (96, 2), (16, 1)):
        d.kc, d.segs = kc, segs
        assert call(*ok) != 0, (kc, segs)
    d.kc, d.segs = 256, 2
    assert call(p, p, p, None, tau, p, p, p) != 0                          # three levels need their tables
    assert call(p + 8, p, p, p, tau, p, p, p) != 0 and call(p, p + 4, p, p, tau, p, p, p) != 0      # misaligned map / limbs
    assert call(p, p, p + 4, p, tau, p, p, p) != 0 and call(p, p, p, p + 8, tau, p, p, p) != 0      # misaligned bias / tables
    d.in_zx = 256
    assert call(*ok) != 0
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0                                    # nothing was launched on the buffer


def test_a_failing_operand_build_ends_in_the_exact_encode(golden, monkeypatch):
    import quantv2x_amd.encode_two_stage as E
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)

    def refuse(*a, **kw):
        raise ValueError("two-stage encode: table / bias entries leave the fixed-point range of the candidate stage")

    monkeypatch.setattr(E, "candidate_tables", refuse)
    st, eng = v2xreal_engine(seg_state(2, 256), g)
    assert eng.encode_mode == "exact" and "fixed-point range" in eng.two_stage_refused and eng._two_stage is None
    put_rows(eng, 1, codes_u8)
    got = eng.encode_codes(1).cpu().numpy().reshape(6, -1)
    assert np.array_equal(got, Oracle(st).encode_rows(rows))
