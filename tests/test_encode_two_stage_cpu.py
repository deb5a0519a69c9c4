"""The two-stage exact encode's THEORY on the CPU (quantv2x_amd/encode_two_stage.py): stage 1 -- the collapsed scores in exact integer
arithmetic, emulated in numpy -- accepts a cell only when its gap at every level exceeds a bound that provably covers the fp32 chain's
rounding; every accepted cell must then carry the oracle's indices (the reference-order fp32 chain, oracle/qv2x_oracle.c) at every level.
Checked on the reference's own 35 200 golden rows (tests/golden/codebook_full.npz: against the oracle AND against the indices
``UMGMQuantizer.encode`` itself produced, codebook.py:106-131, 231-239, 330-337), on a codebook with DUPLICATED and NEARLY duplicated
codewords (exact ties -- first index wins in the reference, codebook.py:110 ``argmin`` -- and gaps spread around the bound), and on other
dictionary sizes; then, on the hostile models and rows of tests/_encode_families.py, the proof's inequalities one by one (the bound on every
cell, every collapsed score against a float64 chain, the kernel's integer ranges).  The HIP kernels are held to the same statements in
tests/test_hip_encode_two_stage.py."""
import copy

import numpy as np
import pytest

from test_codebook_full_golden import _state, golden_rows


def _levels_kc(state):
    levels = sum(1 for l in range(4) if f"codebook/{l}/codebook" in state)
    return levels, int(state["codebook/0/codebook"].shape[0])


DUPLICATES = {5: 3, 70: 9, 40: 2, 41: 1, 90: 0, 100: 50, 101: 60, 110: 30, 111: 31, 120: 64}


def adversarial_state(state):
    """Duplicated codewords (exact ties in every kernel: c_5 = c_3, c_70 = c_9, ... at every level) and near-duplicates at distances that put
    the two best scores 1e-4 .. 1 apart (below, around and above the bound)."""
    st = copy.copy(state)
    rng = np.random.default_rng(5)
    for l in range(3):
        cb = np.array(st[f"codebook/{l}/codebook"], dtype=np.float32, copy=True)
        for dup, src in DUPLICATES.items():
            cb[dup] = cb[src]
        for k, src, eps in ((20, 11, 1e-5), (21, 12, 1e-3), (22, 13, 1e-2), (23, 14, 3e-2), (24, 15, 0.1), (25, 16, 0.3)):
            v = rng.standard_normal(256).astype(np.float32)
            cb[k] = cb[src] + np.float32(eps) * v / np.float32(np.linalg.norm(v))
        st[f"codebook/{l}/codebook"] = cb
    return st


def check_theory(state, codes_u8, in_delta, in_zp, ref_codes=None, name=""):
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import candidate_emulate, candidate_tables
    levels, kc = _levels_kc(state)
    tabs = candidate_tables(state, levels, float(in_delta), int(in_zp))
    cand, flagged, flags, gaps = candidate_emulate(codes_u8, tabs, float(in_delta), int(in_zp))
    rows = (codes_u8.astype(np.float32) - np.float32(in_zp)) * np.float32(in_delta)
    want, ogaps = Oracle(state).encode_rows(rows, want_gaps=True)
    ok = ~flagged
    wrong = (cand != want).any(0)
    print(f"two-stage theory [{name}]: {len(ok)} rows, flagged {flagged.mean():.4f} (per level {flags.mean(1).round(4).tolist()}), "
          f"candidate != oracle on {int(wrong.sum())} rows, of them accepted {int((wrong & ok).sum())}; "
          f"tau at |x| = 134: {[float(t[0] + 134 * t[1] + 134 * 134 * t[2]) * tabs['h'] for t in tabs['tau']]}")
    assert not (wrong & ok).any(), "an ACCEPTED cell differs from the fp32 chain: the bound does not hold"
    # accepted cells have a strict minimum in the fp32 chain too: no exact tie among them
    assert (ogaps[:, ok] > 0).all()
    if ref_codes is not None:
        assert not ((cand != ref_codes).any(0) & ok).any(), "an accepted cell differs from the reference's own index"
    return flagged, cand, want, ogaps


def test_golden_rows_accepted_cells_equal_the_oracle_and_the_reference(golden):
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    flagged, cand, want, _ = check_theory(_state(), codes_u8, g["in_delta"], g["in_zp"], ref_codes=g["codes"], name="reference golden rows")
    assert 0.01 < flagged.mean() < 0.35                                  # the bound is neither vacuous nor useless
    assert ((cand != want).any(0)).sum() >= 1                           # the sample has cells where real arithmetic and the fp32 chain disagree


def test_duplicated_and_nearly_duplicated_codewords(golden):
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    codes_u8 = codes_u8[::4]
    st = adversarial_state(_state())
    flagged, cand, want, ogaps = check_theory(st, codes_u8, g["in_delta"], g["in_zp"], name="duplicated / nearly duplicated codewords")
    # exact ties exist, the fp32 chain resolves them to the FIRST index, and every one of them is sent to stage 2
    ties = (ogaps == 0).any(0)
    assert ties.sum() > 100 and flagged[ties].all()
    assert np.isin(want, list(DUPLICATES)).sum() == 0 and np.isin(want, list(DUPLICATES.values())).sum() > 100
    # gaps on both sides of the bound occur: some near-duplicates are accepted, some flagged
    near = np.isin(want, [11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24, 25]).any(0)
    assert (flagged & near).sum() > 10 and (~flagged & near).sum() > 10


@pytest.mark.parametrize("kc", [64, 32, 96])
def test_other_dictionary_sizes(golden, kc):
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    st = copy.copy(_state())
    for l in range(3):
        st[f"codebook/{l}/codebook"] = np.ascontiguousarray(st[f"codebook/{l}/codebook"][:kc])
    check_theory(st, codes_u8[::8], g["in_delta"], g["in_zp"], name=f"dict {kc}")


def test_refusals_and_the_grid():
    from quantv2x_amd.encode_two_stage import G_MAX_INT, candidate_tables
    st = _state()
    tabs = candidate_tables(st, 3, 0.387, 0)
    gi = tabs["g_int"]
    assert np.abs(gi).max() == G_MAX_INT and tabs["gpack"].shape == (3, 4, 3, 8, 64, 16)
    # the three limbs put back together are the grid values, in the fragment order the kernel reads
    p = tabs["gpack"].astype(np.int64)
    lane, byte = 37, 9                                                  # half 1, score 5 of its tile
    for lv, t, s in ((0, 0, 0), (2, 3, 7), (1, 2, 4)):
        v = p[lv, t, 0, s, lane, byte] + 256 * p[lv, t, 1, s, lane, byte] + 65536 * p[lv, t, 2, s, lane, byte]
        assert v == gi[lv * 128 + 32 * t + (lane & 31), 32 * s + 16 * (lane >> 5) + byte]
    big = copy.copy(st)
    big["codebook/0/codebook"] = np.concatenate([st["codebook/0/codebook"], st["codebook/0/codebook"]])
    with pytest.raises(ValueError):
        candidate_tables(big, 3, 0.387, 0)
    # the bias past 2^44 AFTER the grid choice: the grid keeps rint(g / h) below 2^44 - 2^32, but the folded input offset
    # (128 - zx) * rowsum(G_int) comes on top -- up to 128 * 256 * 2^23 = 2^38.  A state built for it: level 0 with identity heads, one
    # codeword -1 in every channel (a G row of +2 everywhere) and a quantization bias just large enough that g decides the grid.
    import _encode_families as F
    one = F.fewer_levels(st, 1)
    one["codebook/0/stage_w"] = one["codebook/0/qhead_w"] = np.eye(256, dtype=np.float32)
    cb = np.zeros((128, 256), np.float32)
    cb[0] = -1.0
    one["codebook/0/codebook"] = cb
    one["codebook/0/stage_b"] = np.zeros(256, np.float32)
    one["codebook/0/qhead_b"] = np.full(256, 4096.0, np.float32)
    terms = F.h_terms(one, 1, 0.387)
    assert max(terms, key=terms.get) == "bias" and terms["g"] > 0.5 * terms["bias"], terms
    with pytest.raises(ValueError, match="fixed-point range"):
        candidate_tables(one, 1, 0.387, 0)
    assert candidate_tables(one, 1, 0.387, 128)["bias"].max() == 2 ** 44 - 2 ** 32     # (no folded offset at zx = 128: exactly the limit)
    # (the table refusal, an entry >= 2^28 after the grid choice, cannot be reached with finite weights: h >= tmax / (2^28 - 2) puts the
    #  largest entry ON 2^28 - 2 -- test_proof_inequalities_on_every_family asserts that on the two families whose tables decide)


# ---- the proof's inequalities, stated directly, on hostile models and rows (tests/_encode_families.py) --------------------------------------
# (a) an accepted cell equals the oracle; (b) |oracle gap - stage-1 gap| <= tau_l(N0) h on EVERY cell whose codes agree so far;
# (c) every integer score against a float64 evaluation of the layered chain; (d) the kernel's integer ranges; (e) cells on both sides.
_BASE, _FAMILIES = [], {}


def _family(name, golden):
    """(family, its candidate tables): built once per module -- candidate_tables is hundreds of 256 x 256 SVDs"""
    import _encode_families as F
    from quantv2x_amd.encode_two_stage import candidate_tables
    if name not in _FAMILIES:
        if not _BASE:
            _BASE.append(_state())
        fam = F.family(name, _BASE[0], golden["codebook_full"])
        _FAMILIES[name] = (fam, candidate_tables(fam.state, fam.levels, fam.in_delta, fam.in_zx))
    return _FAMILIES[name]


def check_proof(fam, tabs, golden_u8):
    import _encode_families as F
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import candidate_emulate
    rows, n_gold = F.hostile_rows(golden_u8, tabs, fam.in_zx)
    h, levels = tabs["h"], fam.levels
    cand, flagged, flags, gaps = candidate_emulate(rows, tabs, fam.in_delta, fam.in_zx)
    want, ogaps = Oracle(fam.state).encode_rows(F.dequantized(rows, fam.in_delta, fam.in_zx), want_gaps=True)
    assert cand.shape == want.shape == (levels, len(rows))
    # (a) accepted == oracle, and an accepted cell is the fp32 chain's STRICT minimum
    ok = ~flagged
    wrong = (cand != want).any(0)
    assert not (wrong & ok).any(), f"[{fam.name}] an ACCEPTED cell differs from the fp32 chain: rows {np.flatnonzero(wrong & ok)[:8]}"
    assert (ogaps[:, ok] > 0).all()
    # (b) both gaps are minima over b of quantities that differ by at most E_l + 2 e2 = tau_l h (module docstring of encode_two_stage.py);
    # the oracle's gap is ONE more fp32 subtraction (second - best, oracle/qv2x_oracle.c): 2^-24 of it on top
    tau = F.tau_units(tabs, rows, fam.in_delta, fam.in_zx)
    slack = []
    for l in range(levels):
        same = (cand[:l + 1] == want[:l + 1]).all(0)
        lhs = np.abs(ogaps[l].astype(np.float64) - gaps[l])
        rhs = tau[l] * h + 2.0 ** -24 * ogaps[l].astype(np.float64)
        bad = same & ~(lhs <= rhs)
        assert not bad.any(), (f"[{fam.name}] level {l}: the bound does not cover the fp32 chain on rows {np.flatnonzero(bad)[:8]}: "
                               f"|gap difference| {lhs[bad][:4]} > tau h {rhs[bad][:4]}")
        slack.append(float((lhs[same] / (tau[l][same] * h)).max()) if same.any() else float("nan"))
    # (c) stage 1's own error: h S_l[k] against the float64 chain with the oracle's codes forced.  e2 = 0.5 sum |code - zx| (G on the grid)
    # + 0.5 (1 + l) (bias and l table entries) units; eps64 = the float64 chain's bound (F.chain_f64) TWICE -- the collapsed form is the same
    # sum of the same products grouped differently, each passing through as many roundings -- plus the one rounding of h * S
    x0 = (rows.astype(np.float64) - fam.in_zx) * fam.in_delta
    n1 = np.abs(rows.astype(np.int64) - fam.in_zx).sum(1).astype(np.float64)
    grid = []
    for l, (sc, (val, err)) in enumerate(zip(F.integer_scores(tabs, rows, want), F.chain_f64(fam.state, levels, x0, want))):
        e2 = (0.5 * n1 + 0.5 * (1 + l))[:, None] * h
        lhs = np.abs(h * sc - val)
        eps64 = 2.0 * err + F.U64 * np.abs(h * sc)
        bad = ~(lhs <= e2 + eps64)
        assert not bad.any(), (f"[{fam.name}] level {l}: {int(bad.sum())} collapsed scores leave the grid error: worst {float((lhs / (e2 + eps64)).max()):.3g} "
                               f"of the bound at (row, k) {np.argwhere(bad)[:4].tolist()}")
        grid.append(float((lhs / e2).max()))
    # (d) the conditions of the kernel's comments (csrc/codebook_encode_cand.hip): i32 accumulators and bracket, fp64 packed scores
    r = F.integer_ranges(tabs, rows, cand)
    assert r["acc_analytic"] < 2 ** 31 and r["bracket_analytic"] < 2 ** 31 and r["packed_analytic"] < 2 ** 53, r
    assert r["acc_attained"] <= r["acc_analytic"] and r["bracket_attained"] <= r["bracket_analytic"] and r["packed_attained"] <= r["packed_analytic"], r
    stats = {"family": fam.name, "rows": len(rows), "decided_by": F.decided_by(fam.state, levels, fam.in_delta), "h": h,
             "flagged_golden": float(flagged[:n_gold].mean()), "flagged_all": float(flagged.mean()),
             "flagged_per_level": flags.mean(1).round(4).tolist(), "slack_ratio": [round(s, 5) for s in slack],
             "grid_ratio": [round(s, 4) for s in grid], "bracket_bits": round(float(np.log2(max(1, r["bracket_attained"]))), 2),
             "bracket_bits_analytic": round(float(np.log2(r["bracket_analytic"])), 2),
             "packed_bits_analytic": round(float(np.log2(r["packed_analytic"])), 2)}
    print("two-stage proof:", stats)
    return stats, (rows, cand, want, flagged)


def _families():
    import _encode_families as F
    return F.FAMILY_NAMES


@pytest.mark.parametrize("name", _families())
def test_proof_inequalities_on_every_family(golden, name):
    import _encode_families as F
    codes_u8, _ = golden_rows(golden["codebook_full"])
    fam, tabs = _family(name, golden)
    stats, (rows, cand, want, flagged) = check_proof(fam, tabs, codes_u8)
    # (e) not vacuous: at least 5 % of the golden sample accepted (otherwise (a) says nothing), at least one cell flagged
    assert stats["flagged_golden"] <= 0.95 and flagged.any(), stats
    # the variants that exist to reach a branch of the grid choice must reach it
    if name == "base":
        assert fam.in_zx == 0                                            # (the (0, g) point of the issue's input quantizers)
    if name in ("tables_decide_h", "delta_div16"):                       # (a small in_delta shrinks delta G: the tables decide there too)
        terms = F.h_terms(fam.state, fam.levels, fam.in_delta)
        assert max(terms, key=terms.get) == "tables" and tabs["h"] == terms["tables"], terms
        assert np.abs(tabs["tables"]).max() == 2 ** 28 - 2               # the grid choice puts the largest table entry exactly on the limit
    if name == "limb_extremes":
        limbs = F.balanced_limbs(tabs["g_int"])
        assert stats["decided_by"] == "g"
        assert (limbs[0, :F.LIMB_ROWS] == -128).all() and (limbs[1, :F.LIMB_ROWS] == -128).all()
        assert (limbs[:, F.LIMB_ROWS] == 127).all() and (limbs[:, F.LIMB_ROWS + 1] == -127).all()
        # the all-zero row (stored bytes -128) against those rows: both low accumulators at 256 * 128 * 128, the bracket at 2^30 + 2^22
        assert stats["bracket_bits"] >= 30.0 and F.integer_ranges(tabs, rows[:1] * 0, cand[:, :1])["acc_attained"] == 2 ** 22
    if name in ("levels_1", "levels_2"):
        assert tabs["tau"].shape == (fam.levels, 3) and tabs["gpack"].shape[0] == fam.levels and cand.shape[0] == fam.levels


@pytest.mark.parametrize("name", ["heads_x0.05", "heads_x20", "bias_decides_h"])
def test_families_that_must_flag_every_row(golden, name):
    """Models the candidate stage can represent but not decide.  heads_x0.05 / heads_x20: the collapsed matrix of level l grows as
    f^(4 l + 4), a factor f^8 between levels 0 and 2 on ONE 24-bit grid, so the small level's scores are all grid error.  bias_decides_h:
    a bias entry 2^21 times the largest G entry decides the grid (asserted), the distances are that large and one fp32 ulp of them exceeds
    the gaps.  Every golden row must be FLAGGED (stage 2 then decides: still exact) -- and (a)-(d) hold as everywhere."""
    import _encode_families as F
    codes_u8, _ = golden_rows(golden["codebook_full"])
    fam, tabs = _family(name, golden)
    stats, _ = check_proof(fam, tabs, codes_u8)
    assert stats["flagged_golden"] == 1.0, stats
    if name == "bias_decides_h":
        terms = F.h_terms(fam.state, fam.levels, fam.in_delta)
        assert max(terms, key=terms.get) == "bias" and tabs["h"] == terms["bias"], terms
