"""Hostile models and rows for the two-stage exact encode (quantv2x_amd/encode_two_stage.py), shared by tests/test_encode_two_stage_cpu.py and
tests/test_hip_encode_two_stage.py.  Everything is derived from the seeded state of test_codebook_full_golden.py, the input quantizer and the
rows of tests/golden/codebook_full.npz, and seeds: only ``codebook/*`` keys, ``meta/codebook_levels`` (with the levels removed) and the
encoder's input quantizer differ from the seeded model, so every variant is a complete state the engine can deploy.

A family is ``Family(name, state, levels, in_delta, in_zx)``; ``family(name, state, g)`` builds one.  ``hostile_rows`` builds the rows
u8 [R, 256] (the golden sample first); the other functions compute what the CPU statements (a)-(e) are about."""
import copy
from collections import namedtuple

import numpy as np

Family = namedtuple("Family", "name state levels in_delta in_zx")

U64 = 2.0 ** -53
# Per-matrix factors of the scaled families.  Level l's collapsed matrix grows as f^(4 l + 4) -- f^8 between levels 0 and 2, on ONE 24-bit
# grid -- so at 0.05 and 20 one level's scores are all grid error and the unmodified bound flags every golden row: (a) would say nothing.
# 0.25 and 4 are the most extreme factors of the ladder 0.2, 0.25, 0.3, 0.5 / 2, 3, 4, 5 that flag at most 95 % of the golden sample
# (measured: 1.00, 0.71, 0.27, 0.08 / 0.07, 0.14, 0.60, 1.00).  0.05 and 20 stay as families that must flag everything.
SCALED = {"heads_x0.25": 0.25, "heads_x4": 4.0}
FLAG_EVERYTHING = {"heads_x0.05": 0.05, "heads_x20": 20.0, "bias_decides_h": None}
# (the golden quantizer's zero point IS 0 -- asserted in the CPU test -- so ``base`` is the (0, g) point of the input-side list)
QUANTIZERS = ("zx255", "zx128", "delta_div16", "delta_x8")


def levels_kc(state):
    levels = sum(1 for l in range(4) if f"codebook/{l}/codebook" in state)
    return levels, int(state["codebook/0/codebook"].shape[0])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def h_terms(state, levels, in_delta):
    """the three candidates of the grid step ``h`` (encode_two_stage.candidate_tables), recomputed from the collapsed form"""
    from quantv2x_amd.encode_two_stage import G_MAX_INT
    from quantv2x_amd.engine import collapse_encoder_f64
    G, gb, tabs = collapse_encoder_f64(state, levels)
    tmax = max([float(np.abs(t).max()) for t in tabs.values()] + [0.0])
    return {"g": float(np.abs(float(in_delta) * G).max()) / G_MAX_INT, "tables": tmax / (2.0 ** 28 - 2.0),
            "bias": float(np.abs(gb).max()) / (2.0 ** 44 - 2.0 ** 32)}


def decided_by(state, levels, in_delta):
    t = h_terms(state, levels, in_delta)
    return max(t, key=t.get)


def scaled_heads(state, f):
    """stage_w / qhead_w / lhead_w of every level times f, the biases and codebooks by the power of f their layer's input has picked up by
    then (level l: z by f^(2l+1), q and the residual by f^(2l+2)): in real arithmetic the same indices, distances times f^(4l+4)"""
    st = copy.copy(state)
    levels, _ = levels_kc(state)
    for l in range(levels):
        p = f"codebook/{l}/"
        zf, qf = f ** (2 * l + 1), f ** (2 * l + 2)
        for tag, wf, bf in (("stage", f, zf), ("qhead", f, qf), ("lhead", f, qf)):
            if p + tag + "_w" in st:
                st[p + tag + "_w"] = _f32(st[p + tag + "_w"].astype(np.float64) * wf)
                st[p + tag + "_b"] = _f32(st[p + tag + "_b"].astype(np.float64) * bf)
        st[p + "codebook"] = _f32(st[p + "codebook"].astype(np.float64) * qf)
    return st


def tables_decide_h(state, in_delta):
    """Codebook, qhead_w and qhead_b of every level times beta (a power of two: level 0's fp32 chain is the seeded one, scaled exactly).
    G_l = -2 C_l Q_l S_l front_l and g_l grow as beta^2, T_lj = -(G'_l B_j C_j^T)^T as beta^3: the first beta at which a table entry
    decides the grid.  (Enlarging lhead as well enlarges front_l: G would grow FASTER than the tables.)"""
    levels, _ = levels_kc(state)
    beta = 1.0
    while beta <= 2.0 ** 24:
        st = copy.copy(state)
        for l in range(levels):
            for n in ("codebook", "qhead_w", "qhead_b"):
                st[f"codebook/{l}/{n}"] = _f32(state[f"codebook/{l}/{n}"] * np.float32(beta))
        if decided_by(st, levels, in_delta) == "tables":
            return st
        beta *= 2.0
    raise AssertionError("tables_decide_h: no beta up to 2^24 makes a table entry decide the grid")


def bias_decides_h(state, in_delta):
    """qhead_b and stage_b of every level times gamma (a power of two): g_l = G'_l shift_l + |c|^2 - 2 C_l (Q_l bs_l + bq_l) grows as gamma,
    G does not: the first gamma at which a bias entry decides the grid"""
    levels, _ = levels_kc(state)
    gamma = 1.0
    while gamma <= 2.0 ** 40:
        st = copy.copy(state)
        for l in range(levels):
            for n in ("stage_b", "qhead_b"):
                st[f"codebook/{l}/{n}"] = _f32(state[f"codebook/{l}/{n}"] * np.float32(gamma))
        if decided_by(st, levels, in_delta) == "bias":
            return st
        gamma *= 2.0
    raise AssertionError("bias_decides_h: no gamma up to 2^40 makes a bias entry decide the grid")


def ill_conditioned(state):
    """level 1's stage matrix with its singular values replaced by a geometric spread over 1e4 (the largest kept)"""
    st = copy.copy(state)
    u, s, vt = np.linalg.svd(state["codebook/1/stage_w"].astype(np.float64))
    st["codebook/1/stage_w"] = _f32((u * (s[0] * np.logspace(0.0, -4.0, len(s)))) @ vt)
    return st


LIMB_ROWS = 8           # rows 0..7 of level 0's G: both low digits -128 in every channel; row 8: digits (127, 127, 127); row 9: all -127


def limb_extremes(state, in_delta):
    """Level 0 with stage_w = qhead_w = I, so G_0 = -2 C_0 EXACTLY, and codewords that are integers times a power of two: rows 0..7 of G_0
    on the grid are ``d2 * 65536 - 128 * 256 - 128`` (balanced digits (-128, -128, d2)) in every channel, row 8 is G_MAX_INT (which fixes
    the grid: the scale is chosen so that no other level's entry is larger), row 9 its negative.  A cell of stored bytes -128 (code 0)
    then drives both low limb accumulators of those scores to 256 * 128 * 128 = 2^22 -- the largest value the kernel's i32 bracket
    ``(a1 << 8) + a0`` can take."""
    from quantv2x_amd.encode_two_stage import G_MAX_INT
    from quantv2x_amd.engine import collapse_encoder_f64
    st = copy.copy(state)
    levels, kc = levels_kc(state)
    st["codebook/0/stage_w"] = np.eye(256, dtype=np.float32)
    st["codebook/0/qhead_w"] = np.eye(256, dtype=np.float32)
    G, _, _ = collapse_encoder_f64(st, levels)                       # (the later levels' G do not depend on level 0's codebook)
    other = float(np.abs(G[kc:]).max()) if levels > 1 else 1.0
    scale = 2.0 ** int(np.ceil(np.log2(other / G_MAX_INT)))           # G_MAX_INT * scale >= every other entry of G
    rng = np.random.default_rng(23)
    v = np.zeros((kc, 256), np.int64)
    v[:LIMB_ROWS] = rng.integers(-120, 121, (LIMB_ROWS, 256)) * 65536 - 128 * 256 - 128
    v[LIMB_ROWS] = G_MAX_INT
    v[LIMB_ROWS + 1] = -G_MAX_INT
    # the rest: the seeded codewords, rescaled to half the range and put on the same integers (|v| < 2^24: exact in fp32)
    rest = state["codebook/0/codebook"][LIMB_ROWS + 2:].astype(np.float64)
    v[LIMB_ROWS + 2:] = np.rint(rest / np.abs(rest).max() * (G_MAX_INT // 2))
    st["codebook/0/codebook"] = _f32(-0.5 * v.astype(np.float64) * scale)
    assert np.array_equal(-2.0 * st["codebook/0/codebook"].astype(np.float64) / scale, v)
    return st


def fewer_levels(state, levels):
    st = {k: v for k, v in state.items() if not (k.startswith("codebook/") and int(k.split("/")[1]) >= levels)}
    st["meta/codebook_levels"] = np.int64(levels)
    return st


def quantizer(name, g):
    gd, gz = float(g["in_delta"]), int(g["in_zp"])
    return {"zx255": (gd, 255), "zx128": (gd, 128), "delta_div16": (gd / 16.0, gz), "delta_x8": (gd * 8.0, gz)}[name]


FAMILY_NAMES = ("base",) + tuple(SCALED) + ("tables_decide_h", "ill_conditioned", "limb_extremes", "levels_1", "levels_2") + QUANTIZERS


def family(name, state, g):
    """one named variant of ``state`` (the seeded model)"""
    gd, gz = float(np.float32(g["in_delta"])), int(g["in_zp"])
    levels, _ = levels_kc(state)
    if name == "base":
        return Family(name, state, levels, gd, gz)
    if name.startswith("heads_x"):
        return Family(name, scaled_heads(state, {**SCALED, **FLAG_EVERYTHING}[name]), levels, gd, gz)
    if name == "tables_decide_h":
        return Family(name, tables_decide_h(state, gd), levels, gd, gz)
    if name == "bias_decides_h":
        return Family(name, bias_decides_h(state, gd), levels, gd, gz)
    if name == "ill_conditioned":
        return Family(name, ill_conditioned(state), levels, gd, gz)
    if name == "limb_extremes":
        return Family(name, limb_extremes(state, gd), levels, gd, gz)
    if name in ("levels_1", "levels_2"):
        n = int(name[-1])
        return Family(name, fewer_levels(state, n), n, gd, gz)
    d, z = quantizer(name, g)
    return Family(name, state, levels, float(np.float32(d)), z)


def deployable(fam, grid):
    """the family's state with the map size and the encoder's input quantizer written where the engine and the oracle read them"""
    st = copy.copy(fam.state)
    st["meta/grid"] = np.array(grid, dtype=np.int64)
    st["shrinker_m1.layers.0.double_conv.1/a_delta"] = np.float32(fam.in_delta)
    st["shrinker_m1.layers.0.double_conv.1/a_zp"] = np.float32(fam.in_zx)
    return st


def balanced_limbs(gi):
    """the three balanced base-256 digits of the grid values, as candidate_tables packs them: int64 [3][scores][256]"""
    limbs, rest = [], gi.astype(np.int64).copy()
    for _ in range(3):
        d = ((rest + 128) % 256) - 128
        limbs.append(d)
        rest = (rest - d) // 256
    assert not rest.any()
    return np.stack(limbs)


def hostile_rows(golden_u8, tabs, in_zx, seed=11, stride=32):
    """u8 [R, 256] and the number of leading rows that are the strided golden sample"""
    gi = tabs["g_int"]
    sample = golden_u8[::stride]
    rng = np.random.default_rng(seed)
    alt = np.tile(np.array([0, 255], np.uint8), 128)
    special = [np.zeros(256, np.uint8), np.full(256, 255, np.uint8), np.full(256, in_zx, np.uint8), alt, alt[::-1].copy()]
    onehot = (255 * np.eye(256, dtype=np.int64)).astype(np.uint8)
    # the rows that maximise one score's limb sums: 255 where its G is positive (and the complement) -- a handful of scores of every level
    ks = np.unique(np.linspace(0, gi.shape[0] - 1, 6).astype(np.int64))
    limb = [(255 * (gi[k] > 0)).astype(np.uint8) for k in ks] + [(255 * (gi[k] <= 0)).astype(np.uint8) for k in ks]
    uniform = rng.integers(0, 256, (256, 256), dtype=np.uint8)
    few = golden_u8[::4 * stride]
    cleared = [few & np.uint8((0xFF << b) & 0xFF) for b in (1, 2, 3)]
    rows = np.concatenate([sample, np.stack(special), onehot, np.stack(limb), uniform] + cleared)
    return np.ascontiguousarray(rows), len(sample)


def frame_rows(golden_u8, tabs, in_zx, cells):
    """``cells`` rows for one launch: the hostile rows (without their golden sample) in front, golden rows behind"""
    rows, n_gold = hostile_rows(golden_u8, tabs, in_zx)
    extra = rows[n_gold:]
    reps = -(-(cells - len(extra)) // len(golden_u8))
    out = np.concatenate([extra] + [np.roll(golden_u8, 3 * r, axis=1) for r in range(reps)])[:cells]
    assert out.shape == (cells, 256)
    return np.ascontiguousarray(out)


def dequantized(rows_u8, in_delta, in_zx):
    """the fp32 rows the chain sees: (code - zx) * delta, as the kernels and the oracle's callers compute them"""
    return (rows_u8.astype(np.float32) - np.float32(in_zx)) * np.float32(in_delta)


def tau_units(tabs, rows_u8, in_delta, in_zx):
    """tau_l / h of every row, f64 [levels, R], evaluated in fp32 exactly as candidate_emulate (and the kernel) does"""
    tau = tabs["tau"]
    n = rows_u8.astype(np.int64) - int(in_zx)
    n1, n2 = np.abs(n).sum(1), (n * n).sum(1)
    n0 = (np.float32(in_delta) * np.sqrt(n2.astype(np.float32))).astype(np.float32)
    out = np.zeros((tau.shape[0], len(rows_u8)))
    for l in range(tau.shape[0]):
        t = (((tau[l, 0] + tau[l, 1] * n0) + (tau[l, 2] * n0) * n0) + n1.astype(np.float32)).astype(np.float32)
        assert t.dtype == np.float32
        out[l] = t
    return out


def integer_scores(tabs, rows_u8, codes):
    """stage 1's scores S_l[k] (exact integers in f64 [levels][R, kc]) with the earlier levels' codes FORCED to ``codes`` [levels, R]"""
    gi, bias, tables = tabs["g_int"], tabs["bias"], tabs["tables"]
    levels = tabs["tau"].shape[0]
    kc = gi.shape[0] // levels
    s = (rows_u8.astype(np.float64) - 128.0) @ gi.astype(np.float64).T + bias.astype(np.float64)[None]
    out = []
    for l in range(levels):
        sc = s[:, l * kc:(l + 1) * kc].copy()
        for j in range(l):
            sc += tables[l * (l - 1) // 2 + j][codes[j]].astype(np.float64)
        out.append(sc)
    return out


def chain_f64(state, levels, x0, codes):
    """The layered encode (stage -> qhead -> |c|^2 - 2 q . c; lhead - codeword) in float64 with the codes forced: per level
    (dist - |q|^2 as f64 [R, kc], a bound on this evaluation's own rounding error [R, kc]).

    The error bound, u = 2^-53, gamma = 258 u / (1 - 258 u) (a dot product of 256 terms plus its bias, ANY summation order -- Higham,
    Accuracy and Stability of Numerical Algorithms, (3.5) -- so it covers the BLAS):
      * one layer out = W v + b computed from an input that is already off by a vector of norm <= E: the output is off by a vector of
        norm <= ||W||_2 E + || gamma (|W| |v| + |b|) ||_2, the second term from the magnitudes actually computed;
      * the residual lhead(z) - c: one more rounding, u ||x||;
      * the score c2_k - 2 q . c_k: 2 ||c_k|| E_q for the input, gamma (2 |c_k| . |q| + c2_k) for the dot product, the sum of squares and
        the final subtraction (each of at most 258 roundings).
    Nothing here is tuned: every number is a count of roundings or a computed magnitude."""
    g = lambda l, n: state[f"codebook/{l}/{n}"].astype(np.float64)
    gam = 258.0 * U64 / (1.0 - 258.0 * U64)

    def layer(W, b, v, E):
        out = v @ W.T + b
        loc = gam * (np.abs(v) @ np.abs(W).T + np.abs(b))
        return out, float(np.linalg.norm(W, 2)) * E + np.linalg.norm(loc, axis=1)

    x, E, res = x0.astype(np.float64), np.zeros(len(x0)), []
    for l in range(levels):
        Cb = g(l, "codebook")
        z, Ez = layer(g(l, "stage_w"), g(l, "stage_b"), x, E)
        q, Eq = layer(g(l, "qhead_w"), g(l, "qhead_b"), z, Ez)
        c2 = (Cb * Cb).sum(1)
        val = c2[None] - 2.0 * (q @ Cb.T)
        err = 2.0 * np.linalg.norm(Cb, axis=1)[None] * Eq[:, None] + gam * (2.0 * (np.abs(q) @ np.abs(Cb).T) + c2[None])
        res.append((val, err))
        if l < levels - 1:
            lz, El = layer(g(l, "lhead_w"), g(l, "lhead_b"), z, Ez)
            x = lz - Cb[codes[l]]
            E = El + U64 * np.linalg.norm(x, axis=1)
    return res


def integer_ranges(tabs, rows_u8, cand):
    """The largest values the candidate kernel holds (csrc/codebook_encode_cand.hip: i32 limb accumulators, the i32 bracket
    ``256 a1 + a0 + T0 + T1``, the packed fp64 score ``128 S + k``): analytically -- every stored byte at -128 against the limbs' absolute
    values, the largest table entries -- and as attained on the rows with stage 1's own codes."""
    gi, bias, tables = tabs["g_int"], tabs["bias"].astype(np.int64), tabs["tables"].astype(np.int64)
    levels = tabs["tau"].shape[0]
    kc = gi.shape[0] // levels
    limbs = balanced_limbs(gi)                                              # [3][levels * kc][256]
    acc_max = np.abs(limbs).sum(2) * 128                                    # [3][levels * kc]
    tab_max = [sum(int(np.abs(tables[l * (l - 1) // 2 + j]).max()) for j in range(l)) for l in range(levels)]
    lvl = np.arange(levels * kc) // kc
    bracket_max = 256 * acc_max[1] + acc_max[0] + np.array(tab_max, dtype=np.int64)[lvl]
    packed_max = 128 * (65536 * acc_max[2] + bracket_max + np.abs(bias)) + 127
    b = rows_u8.astype(np.int64) - 128
    acc = np.stack([b @ limbs[i].T for i in range(3)])                      # [3][R][levels * kc]
    bracket = 256 * acc[1] + acc[0]
    for l in range(1, levels):
        for j in range(l):
            bracket[:, l * kc:(l + 1) * kc] += tables[l * (l - 1) // 2 + j][cand[j]]
    packed = 128 * (65536 * acc[2] + bracket + bias[None]) + (np.arange(levels * kc) % kc)[None]
    return {"acc_analytic": int(acc_max.max()), "bracket_analytic": int(bracket_max.max()), "packed_analytic": int(packed_max.max()),
            "acc_attained": int(np.abs(acc).max()), "bracket_attained": int(np.abs(bracket).max()), "packed_attained": int(np.abs(packed).max())}
