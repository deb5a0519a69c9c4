"""The two-stage EXACT encode on the GPU (csrc/codebook_encode_cand.hip + the LIST form of codebook_encode_wave_kernel; theory and operands:
quantv2x_amd/encode_two_stage.py, pinned on the CPU by tests/test_encode_two_stage_cpu.py).  Gates:

  * ``encode_mode = "two_stage"`` gives the indices of the reference-order kernel AND of the oracle, bit for bit -- on the reference's own
    35 200 golden rows (also against ``UMGMQuantizer.encode``'s indices themselves, codebook.py:106-131, 231-239, 330-337), on a codebook
    with duplicated / nearly duplicated codewords (exact ties: the first index, as ``argmin`` at codebook.py:110), on ragged launches,
    other dictionary sizes, several frames, and replayed from a HIP graph on fresh input;
  * stage 1 alone equals its numpy emulation bit for bit: the candidate indices of EVERY cell and the set of listed cells (so the CPU
    proof obligations are statements about what runs here);
  * the two C entries of stage 1 are ONE kernel that differs in the packing factor of the score (128 S + k | 256 S + k): the same rows
    through both give the same codes, counters and lists;
  * the refine fraction is the CPU's.

``stage1_alone`` and ``assert_stage1_is_the_emulation`` serve tests/test_hip_encode_two_stage_seg.py (two segments, 256 codes) as well."""
import copy

import numpy as np
import pytest
import torch

from test_codebook_full_golden import _state, golden_rows
from test_encode_two_stage_cpu import adversarial_state

pytestmark = pytest.mark.gpu


def v2xreal_engine(state, g):
    """an engine of V2X-Real map size (100 x 352 = 35 200 cells) around the seeded weights; the encoder's input quantizer is the file's"""
    from quantv2x_amd import synth
    from quantv2x_amd.engine import deploy
    st = copy.copy(state)
    st["meta/grid"] = np.array(synth.grid_size(*synth.SHAPES["v2xreal"][:2]), dtype=np.int64)
    st["shrinker_m1.layers.0.double_conv.1/a_delta"] = np.float32(g["in_delta"])
    st["shrinker_m1.layers.0.double_conv.1/a_zp"] = np.float32(g["in_zp"])
    eng = deploy(state=st)
    eng._workspace(1)
    assert (eng.fh, eng.fw) == (100, 352)
    return st, eng


def put_rows(eng, n, codes_u8):
    b = eng._workspace(n)
    b["s1"][:, 1:-1, 1:-1, :] = torch.from_numpy((codes_u8.astype(np.int16) - 128).astype(np.int8).reshape(n, eng.fh, eng.fw, 256)).cuda()
    return b


def run_modes(eng, n):
    out = {}
    for mode in ("exact", "two_stage"):
        eng.encode_mode = mode
        out[mode] = eng.encode_codes(n).cpu().numpy().reshape(eng.levels, -1).copy()
    torch.cuda.synchronize()
    return out


def stage1_alone(eng, n):
    """the candidate entry the engine would call (``eng.candidate_entry()``) by itself: (codes [levels * segs, M], sorted listed cells,
    counters, the three lists by first undecided level)"""
    import ctypes as C
    from quantv2x_amd import lib as L
    b = eng._workspace(n)
    eng.encode_mode = "two_stage"
    eng.encode_codes(n)                                                  # builds the operands and the buffers
    gp, bias, tab, tau, _ = eng._two_stage
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = n, eng.fh, eng.fw, eng.enc_levels, eng.kc, eng.segs
    d.in_zx, d.in_delta = int(eng.shrink1.out_q[1]), float(eng.shrink1.out_q[0])
    m_cells = n * eng.fh * eng.fw
    codes = torch.zeros((eng.levels, m_cells), dtype=torch.uint8, device="cuda")
    name = eng.candidate_entry()
    L.check(getattr(eng.lib, name)(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), tau, L.ptr(codes),
                                   L.ptr(b["enc_list"]), L.ptr(b["enc_counters"]), L.current_stream()), name)
    torch.cuda.synchronize()
    cnt = b["enc_counters"].cpu().numpy().astype(np.int64)
    lists = [b["enc_list"][c * m_cells:c * m_cells + cnt[1 + c]].cpu().numpy().astype(np.int64) for c in range(3)]
    assert cnt[0] == sum(len(v) for v in lists)
    return codes.cpu().numpy(), np.sort(np.concatenate(lists)), cnt, lists


def assert_stage1_is_the_emulation(eng, n, codes_u8, in_delta, in_zx):
    """stage 1 alone = ``candidate_emulate`` bit for bit: every candidate index of every cell (a listed cell's later levels follow a
    candidate the kernel and the emulation both computed: equal as well), the listed set, the four counters, the three lists as sets (n0,
    n1 and the in_zx arithmetic of the kernel are visible only through the listed set).  Returns (listed flags, the cells first undecided
    at each level)."""
    from quantv2x_amd.encode_two_stage import candidate_emulate
    levels, m = eng.enc_levels, eng.segs
    cand, listed, cnt, lists = stage1_alone(eng, n)
    e_cand, e_flag, e_flags, _ = candidate_emulate(codes_u8, eng._two_stage[4], float(in_delta), int(in_zx))
    assert e_cand.shape == cand.shape == (levels * m, len(codes_u8))
    assert np.array_equal(cand, e_cand), f"{int((cand != e_cand).sum())} candidate indices differ from the emulation"
    assert np.array_equal(listed, np.flatnonzero(e_flag)), (len(listed), int(e_flag.sum()))
    lvl = [e_flags[l * m:(l + 1) * m].any(0) for l in range(levels)]               # a level is undecided if any of its segments is
    first = [lvl[l] & ~np.any(lvl[:l], axis=0) if l else lvl[0] for l in range(levels)] + [np.zeros_like(e_flag)] * (3 - levels)
    assert cnt[0] == e_flag.sum() and list(cnt[1:4]) == [int(f.sum()) for f in first], (cnt, [int(f.sum()) for f in first])
    for c in range(3):                                               # list c = exactly the cells first undecided at level c
        assert np.array_equal(np.sort(lists[c]), np.flatnonzero(first[c])), c
    return e_flag, first


@pytest.mark.parametrize("adversarial", [False, True])
def test_golden_rows_two_stage_equals_exact_oracle_and_reference(golden, adversarial):
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    base = adversarial_state(_state()) if adversarial else _state()
    st, eng = v2xreal_engine(base, g)
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert np.array_equal(got["exact"], want)
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"two-stage encode: {mism} indices differ from the oracle"
    if not adversarial:
        assert np.array_equal(got["two_stage"], g["codes"]) or int((got["two_stage"] != g["codes"]).sum()) == int((want != g["codes"]).sum())
    # stage 1 alone = the CPU emulation, bit for bit: every candidate index, and exactly the same cells listed
    assert_stage1_is_the_emulation(eng, 1, codes_u8, g["in_delta"], g["in_zp"])
    stats = eng.encode_refine_stats(1)
    print("two-stage encode on the golden rows:", stats, "adversarial" if adversarial else "")
    assert 0.01 < stats["refined_fraction"] < 0.5
    if adversarial:
        ties = np.isin(want, [3, 9, 2, 1, 0]).any(0)
        assert ties.sum() > 100


@pytest.mark.parametrize("kc", [64, 32, 96])
def test_other_dictionary_sizes(golden, kc):
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    base = copy.copy(_state())
    for l in range(3):
        base[f"codebook/{l}/codebook"] = np.ascontiguousarray(base[f"codebook/{l}/codebook"][:kc])
    st, eng = v2xreal_engine(base, g)
    put_rows(eng, 1, codes_u8)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(rows)
    assert np.array_equal(got["exact"], want) and np.array_equal(got["two_stage"], want)


@pytest.mark.parametrize("n_agents", [1, 2, 3])
def test_tiny_frames_ragged_launches(n_agents):
    """whole frames at tiny shape (512 cells per agent: less than one wave's 128 cells x 4 per workgroup in the last block, one to three
    frames) through the model call: the two-stage engine's output dict equals the exact engine's bit for bit, indices equal the oracle's"""
    from _common import calibrated_plugin, scene_np
    from oracle.spec import Oracle
    from quantv2x_amd import synth
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.ptq_state import export_ptq_state
    state = export_ptq_state(calibrated_plugin("tiny", n_agents=2))
    eng = deploy(state=state)
    sc = scene_np(n_agents, seed=13)
    dd = synth.scene_to_torch(sc, "cuda")
    eng.encode_mode = "exact"
    te = {}
    want = {k: v.clone() for k, v in eng(dd, te).items()}
    exact_codes = te["codes"].clone()
    eng.encode_mode = "two_stage"
    tt = {}
    got = eng(dd, tt)
    torch.cuda.synchronize()
    assert torch.equal(tt["codes"], exact_codes)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    ot = {}
    Oracle(state).forward(sc, ot)
    assert np.array_equal(tt["codes"].cpu().numpy().reshape(ot["codes"].shape), ot["codes"])


def test_graph_replay_on_fresh_rows(golden):
    """both launches (and the counter reset) inside ONE HIP graph: replayed on rows written after the capture, the indices follow the rows"""
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st, eng = v2xreal_engine(_state(), g)
    eng.encode_mode = "two_stage"
    b = put_rows(eng, 1, codes_u8)
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
    import ctypes as C
    from quantv2x_amd import lib as L
    lib = L.load()
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = 1, 4, 4, 3, 128, 1
    assert lib.qv2x_codebook_encode_candidates_i8(C.byref(d), None, None, None, None, None, None, None, None, None) != 0
    assert lib.qv2x_codebook_encode_listed_f32(C.byref(d), None, None, None, None, None, None) != 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    tau = (C.c_float * 9)()
    d.kc = 256
    assert lib.qv2x_codebook_encode_candidates_i8(C.byref(d), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), tau, L.ptr(buf), L.ptr(buf), L.ptr(buf), None) != 0
    d.kc, d.segs = 128, 2
    assert lib.qv2x_codebook_encode_candidates_i8(C.byref(d), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), tau, L.ptr(buf), L.ptr(buf), L.ptr(buf), None) != 0


@pytest.mark.parametrize("counts", [(31, 0, 0), (1000, 12000, 19730), (1024 * 32 - 40, 0, 33), (20000, 20000, 9152), (300, 49000, 137),
                                    (0, 0, 1536 * 32), (0, 0, 1536 * 32 + 1), (40, 511 * 32, 1024 * 32 - 7), (70400, 0, 0), (5, 7, 70388)])
def test_stage2_alone_on_constructed_lists(golden, counts):
    """qv2x_codebook_encode_listed_f32 by itself on lists of chosen lengths: the device-side split (whole rounds of persistent waves, every second
    round backwards; the remainder as workgroups; more than `list_tail_max` remainder tiles = one more round of waves) at its boundaries --
    1 tile; 2 x 1024 tiles - 1 (+ a second list); a remainder of exactly 512 and of 513 tiles; every cell of two frames listed -- with partial
    tiles in every list.  The listed cells' codes from their list's level on are overwritten with garbage first: stage 2 must restore the
    every-cell kernel's indices, using the STORED codes below that level."""
    import ctypes as C
    from quantv2x_amd import lib as L
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    st, eng = v2xreal_engine(_state(), g)
    n = 2
    rng = np.random.default_rng(5)
    rows = np.concatenate([codes_u8, np.roll(codes_u8, 7, axis=0)[:, rng.permutation(256)]])
    b = put_rows(eng, n, rows)
    eng.encode_mode = "exact"
    ref = eng.encode_codes(n).clone()                                   # [levels, M]
    torch.cuda.synchronize()
    m_cells = n * eng.fh * eng.fw
    assert sum(counts) <= m_cells
    eng.encode_mode = "two_stage"
    eng.encode_codes(n)                                                 # (allocates the list buffers)
    cells = torch.from_numpy(rng.permutation(m_cells)[:sum(counts)].astype(np.int32)).cuda()
    work = ref.clone().reshape(eng.levels, m_cells)
    lst, cnt, at = b["enc_list"], b["enc_counters"], 0
    lst.fill_(-1)
    for c, k in enumerate(counts):
        mine = cells[at:at + k]
        lst[c * m_cells:c * m_cells + k] = mine
        for l in range(c, eng.levels):
            work[l, mine.long()] = 255 - l
        at += k
    cnt.copy_(torch.tensor([sum(counts), *counts], dtype=torch.int32))
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = n, eng.fh, eng.fw, eng.enc_levels, eng.kc, 1
    d.in_zx, d.in_delta = int(eng.shrink1.out_q[1]), float(eng.shrink1.out_q[0])
    L.check(eng.lib.qv2x_codebook_encode_listed_f32(C.byref(d), L.ptr(b["s1"]), eng.level_ptrs, L.ptr(lst), L.ptr(cnt), L.ptr(work), L.current_stream()), "listed")
    torch.cuda.synchronize()
    bad = (work != ref.reshape(eng.levels, m_cells)).sum().item()
    assert bad == 0, f"{bad} indices differ after stage 2 on lists of {counts} cells"


# ---- the hostile families of tests/_encode_families.py: the kernels held to the statements tests/test_encode_two_stage_cpu.py proves ------------
def _family_names():
    import _encode_families as F
    return F.FAMILY_NAMES + tuple(F.FLAG_EVERYTHING)


@pytest.fixture(scope="module", params=_family_names())
def deployed_family(request, golden):
    """one deploy per family (the expensive part), alive for that family's tests only"""
    import _encode_families as F
    fam = F.family(request.param, _state(), golden["codebook_full"])
    st, eng = v2xreal_engine(fam.state, {"in_delta": fam.in_delta, "in_zp": fam.in_zx})
    yield fam, st, eng
    del eng
    torch.cuda.empty_cache()


def test_every_family_two_stage_equals_exact_and_oracle_and_stage1_is_the_emulation(deployed_family, golden):
    """The hostile rows in front of the golden rows, one V2X-Real frame of 35 200 cells: ``two_stage == exact == Oracle.encode_rows`` with 0
    mismatches, and stage 1 alone is the numpy emulation the CPU proof is about.  Covers the grid step decided by a table entry and by a
    bias entry, limbs of -128 against stored bytes of -128 (the kernel's i32 bracket at 2^30 + 2^22), one and two levels, in_zx 255 / 128,
    in_delta / 16 and x 8, and the families the bound cannot decide (every cell listed)."""
    import _encode_families as F
    from oracle.spec import Oracle
    fam, st, eng = deployed_family
    assert eng.encode_mode == "two_stage" and eng.two_stage_refused is None and eng.enc_levels == fam.levels
    assert (float(eng.shrink1.out_q[0]), int(eng.shrink1.out_q[1])) == (fam.in_delta, fam.in_zx)
    codes_u8, _ = golden_rows(golden["codebook_full"])
    rows = F.frame_rows(codes_u8, eng._two_stage[4], fam.in_zx, eng.fh * eng.fw)
    put_rows(eng, 1, rows)
    got = run_modes(eng, 1)
    want = Oracle(st).encode_rows(F.dequantized(rows, fam.in_delta, fam.in_zx))
    assert got["exact"].shape == want.shape == (fam.levels, len(rows))
    assert np.array_equal(got["exact"], want), f"[{fam.name}] exact kernel: {int((got['exact'] != want).sum())} indices differ from the oracle"
    mism = int((got["two_stage"] != want).sum())
    assert mism == 0, f"[{fam.name}] two-stage encode: {mism} indices differ from the oracle"
    e_flag, _ = assert_stage1_is_the_emulation(eng, 1, rows, fam.in_delta, fam.in_zx)
    stats = eng.encode_refine_stats(1)
    print(f"two-stage encode [{fam.name}]:", stats)
    assert stats["refined"] == int(e_flag.sum())
    if fam.name in F.FLAG_EVERYTHING:                                  # (the golden rows behind the hostile ones are all listed)
        assert e_flag[-30000:].all()


def _big_launches():
    """an engine whose cell count per frame (100 x 348 = 34 800 = 2^4 * 2175) makes neither kernel's launch a whole number of workgroups,
    and the frame counts on both sides of the candidate kernel's switch to four cell tiles per wave (M >= 4 * CUs * 256)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cells = 100 * 348
    n_hi = -(-4 * cus * 256 // cells)
    return cus, cells, n_hi


@pytest.mark.parametrize("side", ["four_tiles", "two_tiles_just_below"])
def test_candidate_kernel_both_tile_forms_at_a_large_ragged_launch(golden, side):
    """``encode_candidates_kernel<4, 1, 128>`` (the bench batch's form, reached elsewhere only end to end) and ``<2, 1, 128>`` just below the
    switch, on a launch whose last workgroup is partial: stage 1 == the emulation on EVERY cell, two_stage == exact."""
    import _encode_families as F
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    fam = F.family("base", _state(), g)
    cus, cells, n_hi = _big_launches()
    n = n_hi if side == "four_tiles" else n_hi - 1
    assert n >= 1 and (n * cells >= 4 * cus * 256) == (side == "four_tiles")
    assert (n * cells) % (512 if side == "four_tiles" else 256) != 0   # (a partial last workgroup: 128 | 64 cells per wave, four waves)
    from quantv2x_amd.engine import deploy
    eng = deploy(state=F.deployable(fam, (696, 200, 1)))
    eng._workspace(n)
    assert (eng.fh, eng.fw) == (100, 348) and eng.encode_mode == "two_stage"
    rows = F.frame_rows(codes_u8, eng._two_stage[4], fam.in_zx, n * cells)
    put_rows(eng, n, rows)
    got = run_modes(eng, n)
    mism = int((got["two_stage"] != got["exact"]).sum())
    assert mism == 0, f"{mism} indices of {n} frames differ between the two-stage and the exact encode"
    assert_stage1_is_the_emulation(eng, n, rows, fam.in_delta, fam.in_zx)


@pytest.fixture(scope="module", params=[128, 64])
def one_segment_engine(request, golden):
    """one deploy per dict_size on the ragged map -- the (1, kc) operands of ``candidate_tables`` are built once, inside it -- for both
    launch sizes"""
    import _encode_families as F
    from quantv2x_amd.engine import deploy
    kc = request.param
    base = copy.copy(_state())
    for l in range(3):
        base[f"codebook/{l}/codebook"] = np.ascontiguousarray(base[f"codebook/{l}/codebook"][:kc])
    fam = F.family("base", base, golden["codebook_full"])
    eng = deploy(state=F.deployable(fam, (696, 200, 1)))
    yield kc, fam, eng
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side", ["one_frame", "four_tiles"])
def test_the_packing_factor_is_the_only_difference_between_the_entries(golden, side, one_segment_engine):
    """A (1, kc <= 128) codebook through BOTH entries on the same rows: ``encode_candidates_kernel<CT, 1, 128>`` on bias packed as 128 b + k
    against ``<CT, 1, 256>`` on 256 b + k, CT = 2 (one frame) and CT = 4 (the frame count at the large-tile switch), three levels, a partial
    last workgroup.  With the integer score gap D and T = ceil(t) a cell is listed iff D <= T, or D = T + 1 with the second index below the
    first -- for either P -- so the code planes, the four counters and the three lists (as sets) are equal."""
    import ctypes as C
    import _encode_families as F
    from quantv2x_amd import lib as L
    from quantv2x_amd.encode_two_stage import CANDIDATE_ENTRY
    kc, fam, eng = one_segment_engine
    cus, cells, n_hi = _big_launches()
    n = 1 if side == "one_frame" else n_hi
    m_cells = n * cells
    assert (m_cells >= 4 * cus * 256) == (side == "four_tiles") and m_cells % (512 if side == "four_tiles" else 256) != 0
    b = eng._workspace(n)
    assert (eng.fh, eng.fw, eng.segs, eng.kc, eng.enc_levels) == (100, 348, 1, kc, 3) and eng.encode_mode == "two_stage"
    gp, _, tab, tau, t = eng._two_stage
    assert t["pack"] == 128 and int(np.abs(t["bias"]).max()) < 2 ** 43 - 2 ** 32      # the same grid is inside the 256 contract
    codes_u8, _ = golden_rows(golden["codebook_full"])
    put_rows(eng, n, F.frame_rows(codes_u8, t, fam.in_zx, m_cells))
    eng.encode_codes(n)                                                  # (allocates the list buffers)
    d = L.EncodeDesc()
    d.n, d.h, d.w, d.levels, d.kc, d.segs = n, eng.fh, eng.fw, 3, kc, 1
    d.in_zx, d.in_delta = int(eng.shrink1.out_q[1]), float(eng.shrink1.out_q[0])
    k = np.arange(3 * kc, dtype=np.int64) % kc
    got = {}
    for pf in (128, 256):
        packed = pf * t["bias"] + k
        assert np.array_equal(packed.astype(np.float64).astype(np.int64), packed)
        bias = torch.from_numpy(packed.astype(np.float64)).cuda()
        codes = torch.full((3, m_cells), 255, dtype=torch.uint8, device="cuda")
        b["enc_list"].fill_(-1)
        L.check(getattr(eng.lib, CANDIDATE_ENTRY[pf])(C.byref(d), L.ptr(b["s1"]), L.ptr(gp), L.ptr(bias), L.ptr(tab), tau, L.ptr(codes),
                                                      L.ptr(b["enc_list"]), L.ptr(b["enc_counters"]), L.current_stream()), CANDIDATE_ENTRY[pf])
        torch.cuda.synchronize()
        cnt = b["enc_counters"].cpu().numpy().astype(np.int64)
        lists = [np.sort(b["enc_list"][c * m_cells:c * m_cells + cnt[1 + c]].cpu().numpy().astype(np.int64)) for c in range(3)]
        got[pf] = (codes.cpu().numpy(), cnt, lists)
    assert int(got[128][0].max()) < kc and 0 < got[128][1][0] < m_cells and got[128][1][0] == got[128][1][1:4].sum()
    assert np.array_equal(got[128][0], got[256][0]), f"{int((got[128][0] != got[256][0]).sum())} candidate indices differ between the entries"
    assert np.array_equal(got[128][1][:4], got[256][1][:4]), (got[128][1], got[256][1])
    for c in range(3):
        assert len(np.unique(got[128][2][c])) == len(got[128][2][c]) and np.array_equal(got[128][2][c], got[256][2][c]), c


def test_a_failing_operand_build_ends_in_the_exact_encode(golden, monkeypatch):
    """Whatever ``candidate_tables`` raises -- not only the ValueError of its documented refusals -- the engine falls back to
    ``encode_mode = "exact"`` with the reason in ``two_stage_refused``, and still encodes: no dead forward."""
    import quantv2x_amd.encode_two_stage as E
    from oracle.spec import Oracle
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)

    def singular(*a, **k):
        raise np.linalg.LinAlgError("SVD did not converge")

    def arithmetic(*a, **k):
        raise FloatingPointError("invalid value encountered in divide")

    for boom in (singular, arithmetic):
        monkeypatch.setattr(E, "candidate_tables", boom)
        st, eng = v2xreal_engine(_state(), g)
        assert eng.encode_mode == "exact" and eng.two_stage_refused and eng._two_stage is None, (eng.encode_mode, eng.two_stage_refused)
        put_rows(eng, 1, codes_u8)
        got = eng.encode_codes(1).cpu().numpy().reshape(3, -1)
        assert np.array_equal(got, Oracle(st).encode_rows(rows))
        del eng
