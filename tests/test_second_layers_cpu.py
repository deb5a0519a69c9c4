"""The reference of tests/test_hip_second_layers.py -- ``oracle/spec_second.py`` on the synthetic states and site sets of
tests/_second_layers.py -- pinned on the CPU at the corners the calibrated-model tests never reach: odd volumes, sites on every face, corner
and agent seam, every geometry ``check_geom`` admits that the GPU tests run, zero points that are not 0 on both sides of a layer, real
channel counts that pad upward, and the row-capacity truncation.

  * sites and rulebook: against ``F.conv3d`` of the occupancy and a padded dense index volume, equal element for element;
  * arithmetic: T from a float64 dense convolution of (x - zx) with (w - zw) (exact), then ``* scale * g + h``, ReLU and the quantizer in
    float64.  The oracle rounds after every fp32 operation, so a code may differ where the float64 value y / a_delta lies within 1e-3 of a
    half-integer: those elements are excluded, and they may be at most 0.1 % of a case (the cap of tests/test_pyramid_blocks_cpu.py).  The
    cap is a condition on the float64 side alone: a seed that misses it is replaced, the cap stays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _second_layers import (CHAIN_FILLS, KINDS, STRIDED, SUBM3, SUBM_Z3, chain_layers, chain_scene, codes_like, f32_features, index_volume,
                            input_quantizer, layer_state, second_state, sites, uniform_stats)

VOLUMES = {"5x7x9": (2, (5, 7, 9)), "13x30x37": (3, (13, 30, 37))}
GEOMS = dict(STRIDED, subm3=SUBM3, subm_z3=SUBM_Z3)


def _oracle(state):
    from oracle.spec_second import OracleSecond
    return OracleSecond(state)


def _occupancy(idx, agents, shape):
    occ = torch.zeros((agents, 1, *shape), dtype=torch.float64)
    occ[idx[:, 0], 0, idx[:, 1], idx[:, 2], idx[:, 3]] = 1.0
    return occ


def _dense_rulebook(oidx, iidx, agents, ishape, geom):
    """nbr [K, N_out] read off a dense index volume with a one-cell-per-padding border of -1"""
    k, s, p = geom[1:4], geom[4:7], geom[7:10]
    vol = index_volume(iidx, agents, ishape).reshape(agents, *ishape)
    big = np.full((agents, ishape[0] + 4, ishape[1] + 4, ishape[2] + 4), -1, np.int64)        # window 3, padding 1: two cells suffice
    big[:, 2:-2, 2:-2, 2:-2] = vol
    o = oidx.astype(np.int64)
    out = np.empty((k[0] * k[1] * k[2], len(o)), np.int64)
    kk = 0
    for kz in range(k[0]):
        for ky in range(k[1]):
            for kx in range(k[2]):
                z, y, x = (o[:, 1] * s[0] - p[0] + kz, o[:, 2] * s[1] - p[1] + ky, o[:, 3] * s[2] - p[2] + kx)
                out[kk] = big[o[:, 0], z + 2, y + 2, x + 2]
                kk += 1
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("volume", list(VOLUMES))
@pytest.mark.parametrize("gname", list(GEOMS))
def test_sites_and_rulebook_are_the_dense_convolution_of_the_occupancy(gname, volume, kind):
    from oracle.spec_second import out_shape, out_sites, rulebook
    geom = GEOMS[gname]
    agents, shape = VOLUMES[volume]
    rng = np.random.default_rng(sum(map(ord, gname + volume + kind)))
    idx = sites(rng, agents, shape, kind, density=0.15)
    k, s, p = geom[1:4], geom[4:7], geom[7:10]
    occ = _occupancy(idx, agents, shape)
    if geom[0]:
        act, oidx = occ[:, 0] > 0, idx
    else:
        act = F.conv3d(occ, torch.ones((1, 1, *k), dtype=torch.float64), stride=s, padding=p)[:, 0] > 0
        oidx = out_sites(idx, shape, geom)
        np.testing.assert_array_equal(oidx, act.nonzero().numpy().astype(np.int32))             # nonzero(): raster order of (agent, z, y, x)
        assert oidx.dtype == np.int32
    assert out_shape(shape, geom) == list(act.shape[1:])
    np.testing.assert_array_equal(rulebook(oidx, idx, shape, geom), _dense_rulebook(oidx, idx, agents, shape, geom))


def test_site_kinds():
    rng = np.random.default_rng(0)
    shape = (5, 7, 9)
    for kind in KINDS:
        idx = sites(rng, 3, shape, kind)
        assert idx.dtype == np.int32 and len(np.unique(idx, axis=0)) == len(idx) and (idx >= 0).all() and (idx < [3, *shape]).all()
    c = sites(rng, 2, shape, "corners")
    for b in range(2):
        for z in (0, 4):
            for y in (0, 6):
                for x in (0, 8):
                    assert (c == [b, z, y, x]).all(axis=1).any()
    s = sites(rng, 3, shape, "seam")
    for b in range(2):
        assert (s == [b, 4, 6, 8]).all(axis=1).any() and (s == [b + 1, 0, 0, 0]).all(axis=1).any()
    assert len(sites(rng, 3, shape, "single")) == 1 and 1 not in sites(rng, 3, shape, "empty_agent", density=0.5)[:, 0]
    d = sites(rng, 2, (13, 30, 37), "dense")
    assert len(d) == 7 * 30 * 37 and not (np.diff(d[:, 3]) >= 0).all()                           # shuffled


# ---- arithmetic against float64 --------------------------------------------------------------------------------------------------------

def _f64_codes(state, i, x_minus_zx, idx, agents, shape, oidx, scale):
    """codes and the near-a-boundary mask of layer ``i`` from a float64 dense convolution; ``x_minus_zx`` f64 [N_in, C_in]"""
    p = f"second/{i}/"
    geom = [int(v) for v in state[p + "geom"]]
    k, s, pad = geom[1:4], geom[4:7], geom[7:10]
    wz = state[p + "w_code"].astype(np.float64) - state[p + "w_zp"].astype(np.float64)[None, None, :]      # [K, Cin, Cout]
    cin, cout = wz.shape[1], wz.shape[2]
    dense = torch.zeros((agents, cin, *shape), dtype=torch.float64)
    dense[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(x_minus_zx)
    w = torch.from_numpy(wz.reshape(*k, cin, cout)).permute(4, 3, 0, 1, 2).contiguous()
    T = F.conv3d(dense, w, stride=s, padding=pad).numpy()                                                   # products and sums of integers: exact
    T = T[oidx[:, 0], :, oidx[:, 1], oidx[:, 2], oidx[:, 3]]
    y = T * scale.astype(np.float64)[None, :] * state[p + "bn_g"].astype(np.float64)[None, :] + state[p + "bn_h"].astype(np.float64)[None, :]
    q = np.maximum(y, 0.0) / float(state[p + "a_delta"])
    near = np.abs(q - np.floor(q) - 0.5) < 1e-3
    return np.clip(np.rint(q) + float(state[p + "a_zp"]), 0, 255).astype(np.uint8), near


def _compare(got, want, near, a_zp):
    share = float(near.mean())
    print(f"excluded (within 1e-3 of a rounding boundary): {near.sum()} of {near.size} = {100 * share:.3f} %")
    assert share <= 1e-3, f"{near.sum()} of {near.size} elements sit on a rounding boundary: pick another seed"
    at255, above = float((want == 255).mean()), float((want > a_zp).mean())
    assert at255 < 0.01 and above >= 1 / 3, f"reference output saturated: {at255:.3f} at 255, {above:.3f} above a_zp"
    np.testing.assert_array_equal(got[~near], want[~near])


# (K, padded cin, padded cout) form <- real channels, geometry, input zp, output zp.  Seeds: the first for which the float64 side alone
# keeps the excluded share under its cap (about 0.2 % of the elements strictly inside the code range fall in the 1e-3 band).
I8_CASES = {
    "27_32_32_c16_c16_subm": dict(cin=16, cout=16, geom=SUBM3, zx=3, zp=7, seed=4),
    "27_32_64_c20_c48_s2": dict(cin=20, cout=48, geom=STRIDED["k3_s2_p1"], zx=11, zp=7, seed=8),
    "27_64_64_c64_c64_s2_p011": dict(cin=64, cout=64, geom=STRIDED["k3_s2_p011"], zx=3, zp=5, seed=2),
    "27_64_64_c48_c48_s1": dict(cin=48, cout=48, geom=STRIDED["k3_s1_p1"], zx=11, zp=0, seed=1),
    "3_64_64_c48_c64_subm_z": dict(cin=48, cout=64, geom=SUBM_Z3, zx=7, zp=3, seed=3),
    "3_64_128_c64_c128_k311": dict(cin=64, cout=128, geom=STRIDED["k311_s211_p0"], zx=3, zp=7, seed=1),
    "8_32_32_k2_s2": dict(cin=32, cout=32, geom=STRIDED["k2_s2_p0"], zx=5, zp=9, seed=0),
    "9_32_64_k133": dict(cin=32, cout=64, geom=STRIDED["k133_s122_p011"], zx=9, zp=2, seed=1),
}


def _i8_case(p):
    rng = np.random.default_rng(p["seed"])
    agents, shape = 2, (5, 7, 9)
    dx = np.float32(0.05)
    K = p["geom"][1] * p["geom"][2] * p["geom"][3]
    state = input_quantizer(0, dx, p["zx"])
    state.update(layer_state(rng, 1, p["cin"], p["cout"], p["geom"], (dx, p["zx"]), uniform_stats(p["zx"]), p["zp"], fill=0.35 if K > 8 else 0.6))
    state["second/0/geom"] = np.array(SUBM3, dtype=np.int64)
    state["second/n_layers"], state["second/sparse_shape"] = np.int64(2), np.asarray(shape, dtype=np.int64)
    idx = sites(rng, agents, shape, "random", density=0.3)
    x = codes_like(rng, len(idx), p["cin"])
    return state, idx, x, agents, shape, dx


@pytest.mark.parametrize("case", list(I8_CASES))
def test_integer_layer_matches_float64(case):
    p = I8_CASES[case]
    state, idx, x, agents, shape, dx = _i8_case(p)
    got, oidx, _ = _oracle(state).layer(1, x, idx, list(shape))
    scale = (state["second/1/w_delta"].astype(np.float32) * dx).astype(np.float32)
    want, near = _f64_codes(state, 1, x.astype(np.float64) - p["zx"], idx, agents, shape, oidx, scale)
    assert got.shape == want.shape == (len(oidx), p["cout"]) and got.dtype == np.uint8
    _compare(got, want, near, p["zp"])


F32_CASES = {"k27_zp0": dict(geom=SUBM3, zp=0, seed=1), "k27_zp7": dict(geom=SUBM3, zp=7, seed=1), "k3_zp7": dict(geom=SUBM_Z3, zp=7, seed=1)}


@pytest.mark.parametrize("case", list(F32_CASES))
def test_layer0_matches_float64(case):
    p = F32_CASES[case]
    rng = np.random.default_rng(p["seed"])
    agents, shape = 2, (7, 9, 11)
    K = p["geom"][1] * p["geom"][2] * p["geom"][3]
    state = second_state(rng, shape, [(4, 16, p["geom"])], [p["zp"]], fill=0.35 if K > 8 else 0.6)
    idx = sites(rng, agents, shape, "random", density=0.3)
    x = f32_features(rng, len(idx))
    got, oidx, _ = _oracle(state).layer(0, x, idx, list(shape))
    # the fp32 weight (code - zp_w) * delta_w is itself rounded: the float64 side starts from the same fp32 weights, as the deployed layer does
    wd = ((state["second/0/w_code"].astype(np.float32) - state["second/0/w_zp"][None, None, :]) * state["second/0/w_delta"][None, None, :]).astype(np.float32)
    st64 = dict(state)
    st64["second/0/w_code"], st64["second/0/w_zp"] = wd.astype(np.float64), np.zeros(16)
    want, near = _f64_codes(st64, 0, x.astype(np.float64), idx, agents, shape, oidx, np.ones(16))
    _compare(got, want, near, p["zp"])


# ---- the row-capacity truncation -------------------------------------------------------------------------------------------------------

def test_site_caps_keep_the_first_rows_in_raster_order():
    from oracle.spec_second import out_sites
    rng = np.random.default_rng(4)
    shape = (21, 30, 37)
    state = second_state(rng, shape, chain_layers(), [3, 7, 5, 11, 2], fill=CHAIN_FILLS)
    sc = chain_scene(rng, 2, shape)
    orc = _oracle(state)
    full, capped = {}, {}
    orc.forward(sc, full, batch_size=2)
    n1, n2, n3 = (len(full[f"second/{i}"][1]) for i in (1, 2, 4))
    caps = [n1 // 2, n2 // 3, 10 ** 9]
    bev = orc.forward(sc, capped, batch_size=2, site_caps=caps)
    # level 1: the first cap rows of the uncapped level, codes unchanged (an output's value does not depend on which others are kept)
    c1, i1, _ = capped["second/1"]
    np.testing.assert_array_equal(i1, full["second/1"][1][: caps[0]])
    np.testing.assert_array_equal(c1, full["second/1"][0][: caps[0]])
    key = lambda c: ((c[:, 0].astype(np.int64) * 64 + c[:, 1]) * 64 + c[:, 2]) * 64 + c[:, 3]
    assert (np.diff(key(i1)) > 0).all()
    # level 2: out_sites of the TRUNCATED level 1, truncated again
    c2, i2, s2 = capped["second/2"]
    np.testing.assert_array_equal(i2, out_sites(i1, full["second/1"][2], [int(v) for v in state["second/2/geom"]])[: caps[1]])
    assert len(i2) == caps[1] and len(capped["second/3"][1]) == caps[1] and len(capped["second/4"][1]) <= n3
    # the map: the kept rows of the last level at their cells, the output zero point everywhere else
    c4, i4, s4 = capped["second/4"]
    want = np.full((2, 128, *s4), 2, np.uint8)
    want[i4[:, 0], :, i4[:, 1], i4[:, 2], i4[:, 3]] = c4
    np.testing.assert_array_equal(bev, want.reshape(2, 128 * s4[0], s4[1], s4[2]))
    assert orc.level_of(0) == 0 and orc.level_of(1) == 1 and orc.level_of(3) == 2 and orc.level_of(4) == 3


def test_chain_states_stay_inside_the_code_range():
    """the builder's claim, on the chain the GPU test runs: every layer under 1 % at 255 and a third of the codes above its zero point"""
    rng = np.random.default_rng(4)
    shape = (21, 30, 37)
    zps = [3, 7, 5, 11, 2]
    state = second_state(rng, shape, chain_layers((16, 20, 48, 48, 100)), zps, fill=CHAIN_FILLS)
    taps = {}
    _oracle(state).forward(chain_scene(rng, 2, shape), taps, batch_size=2)
    for i, zp in enumerate(zps):
        c = taps[f"second/{i}"][0]
        print(f"layer {i}: {100 * (c == 255).mean():.2f} % at 255, {100 * (c > zp).mean():.1f} % above a_zp, {len(c)} rows")
        assert (c == 255).mean() < 0.01 and (c > zp).mean() >= 1 / 3 and c.min() >= zp
