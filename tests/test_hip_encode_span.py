"""The span pair of the two-stage exact encode on the GPU (qv2x_codebook_encode_candidates_span_i8 + qv2x_codebook_encode_span_f32; the rule
and its host statement: quantv2x_amd/encode_two_stage.py ``span_classes`` / ``span_rule``, pinned on the CPU by tests/test_encode_span_cpu.py).

  * stage 2 alone on constructed lists: one tile, a partial tile, tiles that straddle two classes, empty classes, every cell listed (both
    kernels: persistent waves and the workgroup remainder) -- expected indices from ``encode_mode = "exact"``, 0 mismatches.  A listed cell
    holds the true codes below its first level; a BAD cell holds wrong candidates from its first to its last undecided level and garbage behind them (its
    tile must continue and restore everything), the others the true codes.  A tile whose candidates are all right must write NOTHING behind
    its exit level: sentinels stored there are still there afterwards;
  * stage 1 alone files every listed cell under the class the host rule gives it, with the same counts, and computes the emulation's codes;
  * end to end two_stage == exact == oracle on the golden rows, the adversarial model and every family; replayed from a HIP graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_codebook_full_golden import _state, golden_rows
from test_encode_two_stage_cpu import adversarial_state
from test_hip_encode_two_stage import put_rows, run_modes, v2xreal_engine

pytestmark = pytest.mark.gpu


def _desc(eng, n):
    from quantv2x_amd import lib as L
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = n, eng.fh, eng.fw, eng.enc_levels, eng.kc, eng.segs
    d.in_zx, d.in_delta = int(eng.shrink1.out_q[1]), float(eng.shrink1.out_q[0])
    return d


@pytest.fixture(scope="module", params=[3, 2, 1], ids=lambda v: f"levels{v}")
def two_frames(request, golden):
    """an engine of `levels` levels with two frames of rows in its workspace and the every-cell kernel's indices for them (computed once)"""
    import _encode_families as F
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    levels = request.param
    state = _state() if levels == 3 else F.family(f"levels_{levels}", _state(), g).state
    st, eng = v2xreal_engine(state, g)
    assert eng.enc_levels == levels and eng.encode_span
    n = 2
    rng = np.random.default_rng(5)
    rows = np.concatenate([codes_u8, np.roll(codes_u8, 7, axis=0)[:, rng.permutation(256)]])
    b = put_rows(eng, n, rows)
    eng.encode_mode = "exact"
    ref = eng.encode_codes(n).clone().reshape(levels, -1)
    eng.encode_mode = "two_stage"
    eng.encode_codes(n)                                                 # (builds the operands)
    torch.cuda.synchronize()
    ref.requires_grad_(False)
    yield eng, b, n, ref
    del eng
    torch.cuda.empty_cache()


def run_stage2(eng, b, n, ref, counts, bad_every=0, bad_at=(), sentinel=()):
    """Lists of ``counts[k]`` cells for class k (SPAN_CLASSES order) out of a fixed permutation of the cells.  Entry i of the whole sequence
    is BAD if ``bad_every`` and i % bad_every == 0, or if i is in ``bad_at``: wrong candidates at every level of its class's span, garbage behind it.
    Entries in ``sentinel`` keep true candidates and get a sentinel behind their class's last level, which must SURVIVE (their tile exits).
    Returns (planes after stage 2, expected planes)."""
    from quantv2x_amd import lib as L
    from quantv2x_amd.encode_two_stage import SPAN_CLASSES
    levels, m_cells = ref.shape
    total = sum(counts)
    assert total <= m_cells and len(counts) == 6
    cells = np.random.default_rng(9).permutation(m_cells)[:total]
    work, want = ref.clone(), ref.clone()
    lst, cnt = b["enc_span_list"], b["enc_span_counters"]
    assert lst.numel() == 6 * m_cells and cnt.numel() == 8
    lst.fill_(-1)
    at = 0
    for k, ((f, e), c) in enumerate(zip(SPAN_CLASSES, counts)):
        if c == 0:
            continue
        assert e < levels, "a class beyond the model's levels must be empty"
        mine = cells[at:at + c]
        lst[k * m_cells:k * m_cells + c] = torch.from_numpy(mine.astype(np.int32)).cuda()
        seq = np.arange(at, at + c)
        bad = np.isin(seq, bad_at) | ((seq % bad_every == 0) if bad_every else False)
        bad_cells = torch.from_numpy(mine[bad]).cuda()
        for l in range(f, e + 1):
            work[l, bad_cells] = (ref[l, bad_cells] + 1) % eng.kc         # wrong candidates from the first to the last undecided level
        for l in range(e + 1, levels):
            work[l, bad_cells] = 255 - l                                  # ... and nothing usable behind it
        keep = torch.from_numpy(mine[np.isin(seq, sentinel)]).cuda()
        for l in range(e + 1, levels):
            work[l, keep] = 200 + l
            want[l, keep] = 200 + l
        at += c
    cnt.copy_(torch.tensor([total, *counts, 0], dtype=torch.int32))
    d = _desc(eng, n)
    L.check(eng.lib.qv2x_codebook_encode_span_f32(C.byref(d), L.ptr(b["s1"]), eng.level_ptrs, L.ptr(lst), L.ptr(cnt), L.ptr(work), L.current_stream()), "span")
    torch.cuda.synchronize()
    return work, want


def by_class(levels, **kw):
    """counts for the classes named f_l (e.g. c0_2=20), zero where the class needs a level the model does not have"""
    from quantv2x_amd.encode_two_stage import SPAN_CLASSES
    return [kw.get(f"c{f}_{e}", 0) if e < levels else 0 for f, e in SPAN_CLASSES]


CASES = {
    "one_tile_0_0": dict(c0_0=32),
    "partial_tile_33_cells": dict(c0_0=33),
    "straddle_0_2_and_0_0": dict(c0_2=20, c0_0=20),                      # tile 0: 20 cells of (0, 2) + 12 of (0, 0)
    "straddle_2_2_and_1_1": dict(c2_2=40, c1_1=40),                      # tile 1: 8 cells of (2, 2) + 24 of (1, 1)
    "all_six_small": dict(c0_2=5, c1_2=70, c2_2=1, c0_1=33, c1_1=64, c0_0=31),
    "nothing_listed": dict(),
    "one_round_of_waves": dict(c0_2=3000, c1_2=5000, c2_2=9000, c0_1=2000, c1_1=7000, c0_0=6001),      # 1001 tiles: the remainder is too long for the workgroups
    "workgroups_only": dict(c0_2=300, c1_2=500, c2_2=4000, c0_1=20, c1_1=3000, c0_0=1000),             # 276 tiles
    "every_cell_listed": dict(c0_2=10000, c1_2=11000, c2_2=20000, c0_1=3000, c1_1=12000, c0_0=14400),  # 2200 tiles: two rounds + 152 in workgroups
}


@pytest.mark.parametrize("case", list(CASES))
def test_stage2_alone_on_constructed_spans(two_frames, case):
    eng, b, n, ref = two_frames
    levels = ref.shape[0]
    counts = by_class(levels, **CASES[case])
    if case == "every_cell_listed":                                      # whatever classes the model has: all 70 400 cells
        counts[5] += ref.shape[1] - sum(counts)
    for bad_every in (0, 97):                                            # every candidate right | one wrong in about a quarter of the tiles
        work, want = run_stage2(eng, b, n, ref, counts, bad_every=bad_every)
        bad = int((work != want).sum())
        assert bad == 0, f"{case}, levels {levels}, bad_every {bad_every}: {bad} indices differ after stage 2 on lists of {counts} cells"


def test_a_tile_continues_on_one_wrong_candidate_and_an_exited_tile_writes_nothing(two_frames):
    """Three tiles of class (0, 0).  Tile 0: ONE cell's stored candidate at level 0 is wrong and every cell's later codes are garbage -- the
    whole tile continues and restores all of them.  Tile 1: every candidate right, the true later codes -- left as they are.  Tile 2: every
    candidate right and SENTINELS behind level 0 -- still there afterwards: an exited tile computes and writes nothing behind its exit level.
    (A one-level model has nothing behind level 0: the wrong candidate is restored, that is all.)"""
    eng, b, n, ref = two_frames
    levels = ref.shape[0]
    counts = by_class(levels, c0_0=96)
    # first with the true later codes in tile 0's other 31 cells (entry 7 alone is bad), the sentinels in tile 2
    work, want = run_stage2(eng, b, n, ref, counts, bad_at=(7,), sentinel=tuple(range(64, 96)))
    assert int((work != want).sum()) == 0
    if levels > 1:
        cells = np.random.default_rng(9).permutation(ref.shape[1])[64:96]
        assert (work[1:, torch.from_numpy(cells).cuda()] >= 200).all()   # the sentinels, not the chain's codes
    # the same with garbage behind level 0 in ALL of tile 0 (true candidates but for entry 7): the tile that continues restores every cell
    from quantv2x_amd import lib as L
    lst, cnt = b["enc_span_list"], b["enc_span_counters"]
    cells = lst[5 * ref.shape[1]:5 * ref.shape[1] + 32].long()
    work2 = ref.clone()
    for l in range(1, levels):
        work2[l, cells] = 255 - l
    work2[0, cells[7]] = (ref[0, cells[7]] + 1) % eng.kc
    d = _desc(eng, n)
    L.check(eng.lib.qv2x_codebook_encode_span_f32(C.byref(d), L.ptr(b["s1"]), eng.level_ptrs, L.ptr(lst), L.ptr(cnt), L.ptr(work2), L.current_stream()), "span")
    torch.cuda.synchronize()
    assert int((work2 != ref).sum()) == 0


def span_stage1_alone(eng, n):
    """qv2x_codebook_encode_candidates_span_i8 by itself: (codes [levels * segs, M], counters [7], the six lists)"""
    from quantv2x_amd import lib as L
    b = eng._workspace(n)
    eng.encode_mode = "two_stage"
    eng.encode_codes(n)
    gp, bias, tab, tau, _ = eng._two_stage
    d = _desc(eng, n)
    m_cells = n * eng.fh * eng.fw
    codes = torch.zeros((eng.levels, m_cells), dtype=torch.uint8, device="cuda")
    b["enc_span_list"].fill_(-1)
    L.check(eng.lib.qv2x_codebook_encode_candidates_span_i8(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), tau, L.ptr(codes),
                                                            L.ptr(b["enc_span_list"]), L.ptr(b["enc_span_counters"]), L.current_stream()), "span stage 1")
    torch.cuda.synchronize()
    cnt = b["enc_span_counters"].cpu().numpy().astype(np.int64)[:7]
    lists = [b["enc_span_list"][k * m_cells:k * m_cells + cnt[1 + k]].cpu().numpy().astype(np.int64) for k in range(6)]
    return codes.cpu().numpy(), cnt, lists


def assert_span_stage1_is_the_host_rule(eng, n, codes_u8, in_delta, in_zx):
    """every listed cell in the list of the class ``span_classes`` gives it (the order inside a list is free), the same counts, the
    emulation's codes"""
    from quantv2x_amd.encode_two_stage import candidate_emulate, span_classes
    cand, cnt, lists = span_stage1_alone(eng, n)
    e_cand, e_flag, e_flags, _ = candidate_emulate(codes_u8, eng._two_stage[4], float(in_delta), int(in_zx))
    assert np.array_equal(cand, e_cand), f"{int((cand != e_cand).sum())} candidate indices differ from the emulation"
    _, _, cls = span_classes(e_flags, eng.segs)
    assert cnt[0] == e_flag.sum() and list(cnt[1:7]) == [int((cls == k).sum()) for k in range(6)], (cnt, np.bincount(cls[cls >= 0], minlength=6))
    for k in range(6):
        assert len(np.unique(lists[k])) == len(lists[k]) and np.array_equal(np.sort(lists[k]), np.flatnonzero(cls == k)), k
    return cls


@pytest.mark.parametrize("adversarial", [False, True])
def test_golden_rows_stage1_classes_and_end_to_end(golden, adversarial):
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(adversarial_state(_state()) if adversarial else _state(), g)
    assert eng.encode_span
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"span pair: {mism} indices differ from the oracle"
    stats = eng.encode_refine_stats(1)
    cls = assert_span_stage1_is_the_host_rule(eng, 1, codes_u8, g["in_delta"], g["in_zp"])
    print("span pair on the golden rows:", stats, "adversarial" if adversarial else "")
    assert stats["refined"] == int((cls >= 0).sum()) == sum(stats["undecided_span"].values()) == sum(stats["first_flagged_at_level"])
    # the other pair of entries, switched to by the deploy option: the same indices
    eng.encode_span = False
    assert np.array_equal(eng.encode_codes(1).cpu().numpy().reshape(3, -1), want)
    assert eng.encode_refine_stats(1)["first_flagged_at_level"] == stats["first_flagged_at_level"]


@pytest.mark.parametrize("m,k", [(2, 256), (1, 256)])
def test_segmented_and_256_entry_codebooks(golden, m, k):
    """the span pair takes these shapes through the same templates (a level is undecided if any of its segments is): stage 1's classes are
    the host rule's, two_stage == exact == oracle on every plane, and the first pair of entries gives the same planes"""
    from oracle.spec import Oracle
    from test_hip_encode_two_stage_seg import seg_state
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(seg_state(m, k), g)
    assert (eng.segs, eng.kc) == (m, k) and eng.encode_mode == "two_stage" and eng.encode_span
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"({m}, {k}) span pair: {mism} indices differ from the oracle"
    cls = assert_span_stage1_is_the_host_rule(eng, 1, codes_u8, g["in_delta"], g["in_zp"])
    print(f"span classes ({m}, {k}):", np.bincount(cls[cls >= 0], minlength=6).tolist())
    eng.encode_span = False
    assert np.array_equal(eng.encode_codes(1).cpu().numpy().reshape(eng.levels, -1), want)


def _family_names():
    import _encode_families as F
    return F.FAMILY_NAMES + tuple(F.FLAG_EVERYTHING)


@pytest.mark.parametrize("name", _family_names())
def test_every_family_end_to_end_and_stage1_classes(golden, name):
    import _encode_families as F
    from oracle.spec import Oracle
    fam = F.family(name, _state(), golden["codebook_full"])
    st, eng = v2xreal_engine(fam.state, {"in_delta": fam.in_delta, "in_zp": fam.in_zx})
    assert eng.encode_mode == "two_stage" and eng.encode_span and eng.enc_levels == fam.levels
    codes_u8, _ = golden_rows(golden["codebook_full"])
    rows = F.frame_rows(codes_u8, eng._two_stage[4], fam.in_zx, eng.fh * eng.fw)
    put_rows(eng, 1, rows)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(F.dequantized(rows, fam.in_delta, fam.in_zx))
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"[{fam.name}] span pair: {mism} indices differ from the oracle"
    assert_span_stage1_is_the_host_rule(eng, 1, rows, fam.in_delta, fam.in_zx)
    del eng
    torch.cuda.empty_cache()


def test_graph_replay_on_fresh_rows(golden):
    """the counter reset and the three launches of the span pair inside ONE HIP graph, replayed on rows written after the capture"""
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(_state(), g)
    assert eng.encode_mode == "two_stage" and eng.encode_span
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
    for shift in (0, 17, 101):
        fresh = np.roll(codes_u8, shift, axis=1)
        put_rows(eng, 1, fresh)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = orc.encode_rows((fresh.astype(np.float32) - np.float32(g["in_zp"])) * np.float32(g["in_delta"]))
        assert np.array_equal(out.cpu().numpy().reshape(3, -1), want), shift
        assert eng.encode_refine_stats(1)["refined"] > 0


def test_refusals():
    from quantv2x_amd import lib as L
    lib = L.load()
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = 1, 4, 4, 3, 128, 1
    assert lib.qv2x_codebook_encode_candidates_span_i8(C.byref(d), None, None, None, None, None, None, None, None, None) != 0
    assert lib.qv2x_codebook_encode_span_f32(C.byref(d), None, None, None, None, None, None) != 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 4)(*([buf.data_ptr()] * 4))
    d.levels = 4                                                         # the span lists have no class for a fourth level
    assert lib.qv2x_codebook_encode_span_f32(C.byref(d), L.ptr(buf), ptrs, L.ptr(buf), L.ptr(buf), L.ptr(buf), None) != 0
    d.levels, d.segs = 3, 4
    tau = (C.c_float * 9)()
    assert lib.qv2x_codebook_encode_candidates_span_i8(C.byref(d), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), tau, L.ptr(buf), L.ptr(buf), L.ptr(buf), None) != 0
