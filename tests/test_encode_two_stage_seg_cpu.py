"""The two-stage exact encode for segmented and 256-entry codebooks, host side (quantv2x_amd/encode_two_stage.py with ``segs``): the theory
pinned on the CPU for ``(seg_num, dict_size)`` = (2, 256) and (1, 256), as tests/test_encode_two_stage_cpu.py pins it for (1, <= 128).

  (a) every cell the emulation does NOT list has, on every plane, the index of ``Oracle.encode_rows`` -- zero exceptions -- and is the fp32
      chain's strict minimum there;
  (b) the proof's inequality itself, per plane: ``|(D_hat[a] - D_hat[b]) - (s[a] - s[b])| <= E_l(N0)`` with a the oracle's index and b
      stage 1's runner-up, D_hat the oracle's fp32 distances and s a float64 evaluation of the layered chain (its own rounding bound added);
      and both top-2 gaps within ``tau_l h`` of each other on every cell whose codes agree so far;
  (c) stage 1's integer scores against that float64 chain: the grid error 0.5 sum |code - zx| + 0.5 (1 + seg_num * l) units;
  (d) the kernel's integer ranges on the actual operands: i32 accumulators, the i32 bracket with ``seg_num * l`` table entries, packed
      scores ``256 S + k`` and their differences below 2^53;
  (e) the listed fraction on the 35 200 golden rows is capped, so the file cannot pass by listing everything: the measured values below
      + 0.05 absolute (what a coarser grid step or another fp32 evaluation of tau may cost); a bound that lists more has lost something
      against the derivation in encode_two_stage.py.

Measured on the golden rows (state of ``calibrated_plugin("tiny", dict_size, seg_num)``, the input quantizer of codebook_full.npz):
(2, 256): listed 0.1973, per plane 0.017 / 0.017 / 0.031 / 0.039 / 0.061 / 0.050, tau at |x| = 134: 0.084 / 0.180 / 0.294;
(1, 256): listed 0.0944, per plane 0.014 / 0.027 / 0.056, tau 0.105 / 0.222 / 0.368."""
import copy

import numpy as np
import pytest

import _encode_families as F
from test_codebook_full_golden import TAU, golden_rows

SHAPES = [(2, 256), (1, 256)]
CAP = {(2, 256): 0.25, (1, 256): 0.15}       # measured 0.197 / 0.094 (module docstring) + 0.05 absolute
_STATES, _TABS = {}, {}


def seg_state(m, k):
    from _common import calibrated_plugin
    from quantv2x_amd.ptq_state import export_ptq_state
    if (m, k) not in _STATES:
        st = export_ptq_state(calibrated_plugin("tiny", dict_size=k, seg_num=m))
        assert int(st["meta/codebook_segs"]) == m and st["codebook/0/codebook"].shape == (m * k, 256)
        _STATES[(m, k)] = st
    return _STATES[(m, k)]


def tables_of(key, state, levels, in_delta, in_zx, m):
    from quantv2x_amd.encode_two_stage import candidate_tables
    if key not in _TABS:
        _TABS[key] = candidate_tables(state, levels, float(in_delta), int(in_zx), m)
    return _TABS[key]


def integer_scores(tabs, rows_u8, codes):
    """stage 1's scores (exact integers in f64, [levels][R, ke]) with the earlier levels' codes FORCED to ``codes`` [levels * m, R]"""
    gi, bias, tables, m, kc = tabs["g_int"], tabs["bias"], tabs["tables"], tabs["segs"], tabs["kc"]
    levels, ke = tabs["tau"].shape[0], m * kc
    s = (rows_u8.astype(np.float64) - 128.0) @ gi.astype(np.float64).T + bias.astype(np.float64)[None]
    out = []
    for l in range(levels):
        sc = s[:, l * ke:(l + 1) * ke].copy()
        for j in range(l):
            for sp in range(m):
                sc += tables[l * (l - 1) // 2 + j][sp * kc + codes[j * m + sp].astype(np.int64)].astype(np.float64)
        out.append(sc)
    return out


def chain_f64(state, levels, m, x0, codes):
    """``F.chain_f64`` for the extended codebook: the codeword an earlier level subtracts is the sum of one extended row per segment.  A
    score's own dot product runs over 256 dims of which 256 / m are non-zero: the bound of 258 roundings covers it."""
    g = lambda l, n: state[f"codebook/{l}/{n}"].astype(np.float64)
    gam = 258.0 * F.U64 / (1.0 - 258.0 * F.U64)

    def layer(W, b, v, E):
        out = v @ W.T + b
        loc = gam * (np.abs(v) @ np.abs(W).T + np.abs(b))
        return out, float(np.linalg.norm(W, 2)) * E + np.linalg.norm(loc, axis=1)

    x, E, res = x0.astype(np.float64), np.zeros(len(x0)), []
    for l in range(levels):
        Cb = g(l, "codebook")
        kc = Cb.shape[0] // m
        z, Ez = layer(g(l, "stage_w"), g(l, "stage_b"), x, E)
        q, Eq = layer(g(l, "qhead_w"), g(l, "qhead_b"), z, Ez)
        c2 = (Cb * Cb).sum(1)
        val = c2[None] - 2.0 * (q @ Cb.T)
        err = 2.0 * np.linalg.norm(Cb, axis=1)[None] * Eq[:, None] + gam * (2.0 * (np.abs(q) @ np.abs(Cb).T) + c2[None])
        res.append((val, err))
        if l < levels - 1:
            lz, El = layer(g(l, "lhead_w"), g(l, "lhead_b"), z, Ez)
            x = lz - sum(Cb[sp * kc + codes[l * m + sp].astype(np.int64)] for sp in range(m))
            E = El + (m + 1) * F.U64 * (np.linalg.norm(x, axis=1) + np.linalg.norm(lz, axis=1))
    return res


def integer_ranges(tabs, rows_u8, cand):
    """The largest values the candidate kernel holds at two segments / 256 codes (csrc/codebook_encode_cand.hip): analytically -- every stored byte at -128 against the
    limbs' absolute values, ``seg_num * l`` table entries of the largest magnitude -- and as attained on the rows with stage 1's own codes."""
    gi, bias, tables = tabs["g_int"], tabs["bias"].astype(np.int64), tabs["tables"].astype(np.int64)
    m, kc, P = tabs["segs"], tabs["kc"], int(tabs["pack"])
    levels, ke = tabs["tau"].shape[0], m * kc
    limbs = F.balanced_limbs(gi)
    acc_max = np.abs(limbs).sum(2) * 128
    tab_max = [m * sum(int(np.abs(tables[l * (l - 1) // 2 + j]).max()) for j in range(l)) for l in range(levels)]
    lvl = np.arange(levels * ke) // ke
    bracket_max = 256 * acc_max[1] + acc_max[0] + np.array(tab_max, dtype=np.int64)[lvl]
    packed_max = P * (65536 * acc_max[2] + bracket_max + np.abs(bias)) + (P - 1)
    b = rows_u8.astype(np.int64) - 128
    acc = np.stack([b @ limbs[i].T for i in range(3)])
    bracket = 256 * acc[1] + acc[0]
    for l in range(1, levels):
        for j in range(l):
            for sp in range(m):
                bracket[:, l * ke:(l + 1) * ke] += tables[l * (l - 1) // 2 + j][sp * kc + cand[j * m + sp].astype(np.int64)]
    packed = P * (65536 * acc[2] + bracket + bias[None]) + (np.arange(levels * ke) % kc)[None]
    return {"acc_analytic": int(acc_max.max()), "bracket_analytic": int(bracket_max.max()), "packed_analytic": int(packed_max.max()),
            "acc_attained": int(np.abs(acc).max()), "bracket_attained": int(np.abs(bracket).max()), "packed_attained": int(np.abs(packed).max())}


def check_proof(name, state, m, tabs, rows, in_delta, in_zx):
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import candidate_emulate
    levels, kc, h = tabs["tau"].shape[0], tabs["kc"], tabs["h"]
    cand, flagged, flags, gaps = candidate_emulate(rows, tabs, in_delta, in_zx)
    want, ogaps = Oracle(state).encode_rows(F.dequantized(rows, in_delta, in_zx), want_gaps=True)
    assert cand.shape == want.shape == ogaps.shape == (levels * m, len(rows))
    # (a) accepted == oracle on every plane, and an accepted cell is the fp32 chain's STRICT minimum
    ok = ~flagged
    wrong = (cand != want).any(0)
    assert not (wrong & ok).any(), f"[{name}] an ACCEPTED cell differs from the fp32 chain: rows {np.flatnonzero(wrong & ok)[:8]}"
    assert (ogaps[:, ok] > 0).all()
    # (b) the top-2 gaps of the two evaluations differ by at most tau_l h on every cell whose codes agree so far (both are minima over b of
    # quantities that differ by at most E_l + 2 e2); the oracle's gap is one more fp32 subtraction: 2^-24 of it on top
    tau = F.tau_units(tabs, rows, in_delta, in_zx)                       # [levels, R], in units of h
    slack = []
    for l in range(levels):
        for sg in range(m):
            p = l * m + sg
            same = (cand[:p + 1] == want[:p + 1]).all(0) if m == 1 else (cand[:l * m] == want[:l * m]).all(0) & (cand[p] == want[p])
            lhs = np.abs(ogaps[p].astype(np.float64) - gaps[p])
            rhs = tau[l] * h + 2.0 ** -24 * ogaps[p].astype(np.float64)
            bad = same & ~(lhs <= rhs)
            assert not bad.any(), f"[{name}] plane {p}: the bound does not cover the fp32 chain on rows {np.flatnonzero(bad)[:8]}: {lhs[bad][:4]} > {rhs[bad][:4]}"
            slack.append(float((lhs[same] / (tau[l][same] * h)).max()) if same.any() else float("nan"))
    # (c) stage 1's own error against the float64 chain with the oracle's codes forced: e2 = 0.5 sum |code - zx| + 0.5 (1 + m l) units
    x0 = (rows.astype(np.float64) - in_zx) * in_delta
    n1 = np.abs(rows.astype(np.int64) - in_zx).sum(1).astype(np.float64)
    ea, eb, ec = tabs["bound"]
    n0 = np.linalg.norm(x0, axis=1)
    scores = integer_scores(tabs, rows, want)
    chain = chain_f64(state, levels, m, x0, want)
    for l, (sc, (val, err)) in enumerate(zip(scores, chain)):
        e2 = (0.5 * n1 + 0.5 * (1 + m * l))[:, None] * h
        lhs = np.abs(h * sc - val)
        eps64 = 2.0 * err + F.U64 * np.abs(h * sc)
        bad = ~(lhs <= e2 + eps64)
        assert not bad.any(), f"[{name}] level {l}: {int(bad.sum())} collapsed scores leave the grid error: worst {float((lhs / (e2 + eps64)).max()):.3g} of the bound"
        # the inequality of the proof, per segment, for the pair (a = the oracle's index, b = stage 1's runner-up among the others):
        # |(D_hat[a] - D_hat[b]) - (s[a] - s[b])| <= E_l(N0), s from the float64 chain (its own error bound on both scores added).  The
        # oracle reports D_hat[b'] - D_hat[a] for ITS runner-up b'; where b' == b that is the left side; elsewhere the minimum property
        # gives the one-sided statement ogap <= s[b] - s[a] + E.
        E = ea[l] + eb[l] * n0 + ec[l] * n0 * n0
        for sg in range(m):
            p = l * m + sg
            v = val[:, sg * kc:(sg + 1) * kc]
            er = err[:, sg * kc:(sg + 1) * kc]
            a = want[p].astype(np.int64)
            masked = sc[:, sg * kc:(sg + 1) * kc].copy()
            r = np.arange(len(rows))
            masked[r, a] = np.inf
            b = masked.argmin(1)
            ds = v[r, b] - v[r, a]
            de = er[r, b] + er[r, a]
            og = ogaps[p].astype(np.float64)
            bad = ~(og <= ds + E + de + 2.0 ** -24 * og)
            assert not bad.any(), f"[{name}] plane {p}: D_hat[b] - D_hat[a] exceeds s[b] - s[a] + E_l on rows {np.flatnonzero(bad)[:8]}"
            # and where the float64 gap itself exceeds E_l (+ its own error) the fp32 chain's minimum is a: a strict positive oracle gap
            sure = ds - de > E
            assert (og[sure] > 0).all()
    # (d) the kernel's integer ranges
    rg = integer_ranges(tabs, rows, cand)
    assert rg["acc_analytic"] < 2 ** 31 and rg["bracket_analytic"] < 2 ** 31 and 2 * rg["packed_analytic"] < 2 ** 53, rg
    assert rg["acc_attained"] <= rg["acc_analytic"] and rg["bracket_attained"] <= rg["bracket_analytic"] and rg["packed_attained"] <= rg["packed_analytic"], rg
    stats = {"name": name, "rows": len(rows), "h": h, "listed": float(flagged.mean()), "per_plane": flags.mean(1).round(4).tolist(),
             "slack_ratio": [round(s, 5) for s in slack], "bracket_bits": round(float(np.log2(rg["bracket_analytic"])), 2),
             "packed_bits": round(float(np.log2(rg["packed_analytic"])), 2)}
    print("two-stage proof (segments):", stats)
    return stats, (cand, want, flagged, flags, ogaps)


@pytest.mark.parametrize("m,k", SHAPES)
def test_golden_rows_unlisted_cells_equal_the_oracle_and_the_listed_fraction_is_capped(golden, m, k):
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import candidate_emulate
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    st = seg_state(m, k)
    tabs = tables_of((m, k), st, 3, g["in_delta"], g["in_zp"], m)
    assert tabs["pack"] == 256 and tabs["gpack"].shape == (3, m * k // 32, 3, 8, 64, 16) and tabs["tables"].shape == (3, m * k, m * k)
    cand, flagged, flags, _ = candidate_emulate(codes_u8, tabs, float(g["in_delta"]), int(g["in_zp"]))
    want, ogaps = Oracle(st).encode_rows(rows, want_gaps=True)
    assert cand.shape == want.shape == (3 * m, 35200)
    ok = ~flagged
    assert int((cand[:, ok] != want[:, ok]).sum()) == 0                  # zero exceptions, every plane
    assert (ogaps[:, ok] > 0).all()
    lvl = [flags[l * m:(l + 1) * m].any(0) for l in range(3)]
    first = [float((lvl[l] & ~np.any(lvl[:l], axis=0)).mean()) if l else float(lvl[0].mean()) for l in range(3)]
    print(f"two-stage theory ({m}, {k}): listed {flagged.mean():.4f}, first undecided at level {np.round(first, 4).tolist()}, per plane "
          f"{flags.mean(1).round(4).tolist()}, tau at |x| = 134: {[float(t[0] + 134 * t[1] + 134 * 134 * t[2]) * tabs['h'] for t in tabs['tau']]}")
    assert 0.01 < flagged.mean() <= CAP[(m, k)], flagged.mean()


@pytest.mark.parametrize("m,k", SHAPES + [(2, 128), (1, 192)])        # (the last two: other shapes the same code takes)
def test_proof_inequalities_on_hostile_rows(golden, m, k):
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    st = seg_state(m, k)
    in_delta, in_zx = float(np.float32(g["in_delta"])), int(g["in_zp"])
    tabs = tables_of((m, k), st, 3, in_delta, in_zx, m)
    rows, n_gold = F.hostile_rows(codes_u8, tabs, in_zx)
    stats, (_, _, flagged, _, _) = check_proof(f"({m}, {k}) base", st, m, tabs, rows, in_delta, in_zx)
    assert flagged.any() and not flagged[:n_gold].all()


def duplicated_state(state, m, kc, tie_segments):
    """Duplicated codewords INSIDE the given segments (exact ties in every kernel: the first index wins, codebook.py:110) and near-duplicates
    at distances on both sides of the bound; the other segments keep their wide gaps."""
    st = copy.copy(state)
    rng = np.random.default_rng(5)
    d = 256 // m
    for l in range(3):
        cb = np.array(st[f"codebook/{l}/codebook"], dtype=np.float32, copy=True)
        for sg in tie_segments:
            blk = cb[sg * kc:(sg + 1) * kc]
            for dup, src in ((5, 3), (70, 9), (200, 2), (41, 1), (255, 0), (130, 50)):
                blk[dup] = blk[src]
            for kk, src, eps in ((20, 11, 1e-5), (21, 12, 1e-3), (22, 13, 1e-2), (23, 14, 3e-2), (24, 15, 0.1), (25, 16, 0.3)):
                v = np.zeros(256, np.float32)
                v[sg * d:(sg + 1) * d] = rng.standard_normal(d).astype(np.float32)
                blk[kk] = blk[src] + np.float32(eps) * v / np.float32(np.linalg.norm(v))
        st[f"codebook/{l}/codebook"] = cb
    return st


@pytest.mark.parametrize("tie_segments", [(0, 1), (1,)])
def test_duplicated_codewords_inside_a_segment(golden, tie_segments):
    """exact ties in both segments, and a tie in ONE segment with a wide gap in the other: every tied cell is listed, the oracle resolves
    the tie to the FIRST index, the accepted cells equal the oracle on all six planes"""
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    m, k = 2, 256
    st = duplicated_state(seg_state(m, k), m, k, tie_segments)
    in_delta, in_zx = float(np.float32(g["in_delta"])), int(g["in_zp"])
    tabs = tables_of(("dup", tie_segments), st, 3, in_delta, in_zx, m)
    rows = codes_u8[::8]
    stats, (cand, want, flagged, flags, ogaps) = check_proof(f"duplicates in segments {tie_segments}", st, m, tabs, rows, in_delta, in_zx)
    planes = [l * m + sg for l in range(3) for sg in tie_segments]
    others = [p for p in range(3 * m) if p not in planes]
    ties = (ogaps[planes] == 0).any(0)
    assert ties.sum() > 50 and flagged[ties].all()
    assert np.isin(want[planes], [5, 70, 200, 41, 255, 130]).sum() == 0 and np.isin(want[planes], [3, 9, 2, 1, 0, 50]).sum() > 50
    if others:                                                          # a tie in one segment beside a WIDE gap in the other: still listed
        wide = (ogaps[others] > 1.0).all(0)
        assert (ties & wide).sum() > 10 and flagged[ties & wide].all() and not flags[others][:, ties & wide].any()
    assert (~flagged).sum() > 100


@pytest.mark.parametrize("in_zx", [255, 128])
def test_other_input_zero_points(golden, in_zx):
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    m, k = 2, 256
    st = seg_state(m, k)
    in_delta = float(np.float32(g["in_delta"]))
    tabs = tables_of(("zx", in_zx), st, 3, in_delta, in_zx, m)
    rows, _ = F.hostile_rows(codes_u8, tabs, in_zx, stride=64)
    check_proof(f"(2, 256) in_zx {in_zx}", st, m, tabs, rows, in_delta, in_zx)


def test_a_table_entry_decides_the_grid_step(golden):
    """codebook, qhead_w and qhead_b times a power of two until a table entry decides ``h``: the largest entry then sits on the segment
    kernel's limit 2^27 - 2 (four entries beside 256 a1 + a0 in an i32), and everything above still holds on the coarser grid"""
    from quantv2x_amd.encode_two_stage import G_MAX_INT
    from quantv2x_amd.engine import collapse_encoder_f64
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    m, k = 2, 256
    base = seg_state(m, k)
    in_delta, in_zx = float(np.float32(g["in_delta"])), int(g["in_zp"])
    beta, st = 1.0, None
    while beta <= 2.0 ** 24:
        st = copy.copy(base)
        for l in range(3):
            for n in ("codebook", "qhead_w", "qhead_b"):
                st[f"codebook/{l}/{n}"] = np.ascontiguousarray(base[f"codebook/{l}/{n}"] * np.float32(beta), dtype=np.float32)
        G, gb, tt = collapse_encoder_f64(st, 3)
        terms = {"g": float(np.abs(in_delta * G).max()) / G_MAX_INT, "tables": max(float(np.abs(t).max()) for t in tt.values()) / (2.0 ** 27 - 2.0),
                 "bias": float(np.abs(gb).max()) / (2.0 ** 43 - 2.0 ** 32)}
        if max(terms, key=terms.get) == "tables":
            break
        beta *= 2.0
    assert max(terms, key=terms.get) == "tables", terms
    tabs = tables_of("tables_decide", st, 3, in_delta, in_zx, m)
    assert tabs["h"] == terms["tables"] and np.abs(tabs["tables"]).max() == 2 ** 27 - 2
    rows, _ = F.hostile_rows(codes_u8, tabs, in_zx, stride=64)
    stats, _ = check_proof("(2, 256) tables decide h", st, m, tabs, rows, in_delta, in_zx)
    assert stats["bracket_bits"] < 31.0


def test_refusals_and_one_segment_128_is_unchanged(golden):
    """what does not fit is refused with a ValueError (the engine then stays on ``"exact"``); (1, 128) through the generalised functions
    gives the arrays it gave: the 128-wide packing, the 2^28 / 2^44 limits, the same tau"""
    from quantv2x_amd.encode_two_stage import candidate_emulate, candidate_tables, encode_error_bound
    from test_codebook_full_golden import _state
    g = golden["codebook_full"]
    st = _state()
    a = candidate_tables(st, 3, 0.387, 0)
    b = candidate_tables(st, 3, 0.387, 0, 1)
    for key in ("gpack", "bias", "tables", "tau", "h"):
        assert np.array_equal(a[key], b[key]), key
    assert a["pack"] == 128 and a["tau"].dtype == np.float32 and a["bias"].dtype == np.int64 and a["tables"].dtype == np.int32
    assert all(np.array_equal(x, y) for x, y in zip(encode_error_bound(st, 3, 0.387)[:3], encode_error_bound(st, 3, 0.387, 1)[:3]))
    codes_u8, _ = golden_rows(g)
    out = candidate_emulate(codes_u8[::16], a, 0.387, 0)
    assert out[0].shape == (3, len(codes_u8[::16])) and out[2].shape == out[0].shape
    seg = seg_state(2, 256)
    with pytest.raises(ValueError):
        candidate_tables(seg, 3, 0.387, 0, 4)                             # four segments: not taken
    with pytest.raises(ValueError):
        candidate_tables(seg, 3, 0.387, 0, 1)                             # 512 rows as ONE segment: dict_size > 256


@pytest.mark.parametrize("m,k", SHAPES)
def test_reference_fixture_oracle_and_unlisted_cells(golden, m, k):
    """tests/golden/codebook_seg_i8grid.npz: ``UMGMQuantizer.encode`` of the reference itself (one BLAS thread) at (2, 256) and (1, 256) on
    the int8-grid rows of codebook_full.npz.  Wherever the reference's own top-2 gap exceeds 1e-4 the oracle's planes equal the reference's,
    and so do the emulation's unlisted cells; the planes left out are fewer than 5e-3 of all."""
    import os
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import candidate_emulate
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebook_seg_i8grid.npz")
    f = np.load(path)
    g = golden["codebook_full"]
    codes_u8, rows = golden_rows(g)
    ref, gaps = f[f"codes_m{m}_k{k}"], f[f"gaps_m{m}_k{k}"].astype(np.float32)
    assert ref.shape == gaps.shape == (3 * m, 35200)
    st = seg_state(m, k)
    solid = gaps > TAU
    assert (~solid).mean() < 5e-3
    want = Oracle(st).encode_rows(rows)
    assert int(((want != ref) & solid).sum()) == 0
    tabs = tables_of((m, k), st, 3, g["in_delta"], g["in_zp"], m)
    cand, flagged, _, _ = candidate_emulate(codes_u8, tabs, float(g["in_delta"]), int(g["in_zp"]))
    assert int(((cand != ref) & solid)[:, ~flagged].sum()) == 0
