"""The SECOND encoder's kernels (csrc/sparse_conv.hip) one entry at a time against the CPU restatement, bit for bit: qv2x_mean_vfe_f32,
qv2x_sp_index_scatter, qv2x_sp_out_sites, qv2x_sp_rulebook, qv2x_sp_conv_f32in, qv2x_sp_conv_i8, qv2x_sp_to_bev_i8, and whole synthetic
five-layer encoders through ``DeployedSecondEncoder``.

The whole-frame tests (test_hip_second.py, test_hip_fullsize.py, test_heter.py) run one calibrated VoxelBackBone8x: every zero point is 0,
the volumes are multiples of 1024 cells, no level overflows, no loop takes a second trip.  Here: zero points that are not 0 on both sides
of a layer, real channel counts that pad upward, odd volumes, sites on every corner, face and agent seam, every geometry the argument
check admits that a layer could have, row counts at and around every tile size, capacities below the true count, and one case past each
grid-stride / persistent-loop threshold.  States and site sets come from tests/_second_layers.py, weights go through the engine's own
``_SpLayer``, every output buffer starts full of a sentinel, and tests/test_second_layers_cpu.py pins the reference itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from _second_layers import (CHAIN_FILLS, KINDS, STRIDED, SUBM3, SUBM_Z3, chain_layers, chain_scene, codes_like, f32_features, index_volume,
                            input_quantizer, layer_state, linear, second_state, sites, uniform_stats)

pytestmark = pytest.mark.gpu

SENT, SENT32, SENTF = -77, -7777, -7777.0
VOLUMES = {"5x7x9": (2, (5, 7, 9)), "13x30x37": (3, (13, 30, 37))}


def _dev():
    return torch.device("cuda")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _count(n):
    return torch.tensor([int(n)], dtype=torch.int32, device=_dev())


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=_dev())


def _desc(geom, in_shape, agents, cin=32, cout=32, cap_in=1, cap_out=1, out_q=(1.0, 0.0)):
    from oracle.spec_second import out_shape
    from quantv2x_amd import lib as L
    d, osh = L.SpconvDesc(), out_shape(in_shape, geom)
    d.subm = int(geom[0])
    for a in range(3):
        d.k[a], d.s[a], d.p[a] = int(geom[1 + a]), int(geom[4 + a]), int(geom[7 + a])
        d.in_shape[a], d.out_shape[a] = int(in_shape[a]), int(osh[a])
    d.agents, d.cin, d.cout, d.cap_in, d.cap_out = int(agents), int(cin), int(cout), int(cap_in), int(cap_out)
    d.out_delta, d.out_zp = float(out_q[0]), float(out_q[1])
    return d, osh


def _rows(idx, cap):
    """int32 [cap][4] on the device: ``idx`` in front, rows behind it at the (valid) coordinate 0"""
    c = np.zeros((cap, 4), np.int32)
    c[: len(idx)] = idx
    return _t(c)


# ---- qv2x_mean_vfe_f32 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_points", [1, 5, 7])
def test_mean_vfe(max_points):
    from oracle.spec_second import mean_vfe
    from quantv2x_amd import lib as L
    cap, pad = 300, 8
    rng = np.random.default_rng(max_points)
    vox = rng.normal(0.0, 3.0, size=(cap, max_points, 4)).astype(np.float32)
    nump = rng.integers(0, max_points + 1, size=cap).astype(np.int32)
    assert (nump == 0).any()
    want = mean_vfe(vox, nump)
    vd, nd = _t(vox), _t(nump)
    for n in (0, 1, 257, cap, cap + 5):                               # cap + 5: the count is clamped to the buffers' rows
        out, cnt = _full((cap + pad, 4), SENTF, torch.float32), _count(n)
        L.check(L.load().qv2x_mean_vfe_f32(L.ptr(vd), L.ptr(nd), L.ptr(cnt), cap, max_points, L.ptr(out), L.current_stream()), "qv2x_mean_vfe_f32")
        torch.cuda.synchronize()
        o, m = out.cpu().numpy(), min(n, cap)
        np.testing.assert_array_equal(o[:m].view(np.int32), want[:m].view(np.int32), err_msg=f"count {n}")
        assert (o[m:] == SENTF).all(), f"count {n}: rows at or beyond it were written"


# ---- qv2x_sp_index_scatter -------------------------------------------------------------------------------------------------------------

def _scatter(coords, cnt, cap, agents, shape, vol, set_):
    from quantv2x_amd import lib as L
    L.check(L.load().qv2x_sp_index_scatter(L.ptr(coords), L.ptr(cnt), cap, agents, *[int(v) for v in shape], L.ptr(vol), set_, L.current_stream()),
            "qv2x_sp_index_scatter")
    torch.cuda.synchronize()


def test_index_scatter_set_and_undo():
    agents, shape = 3, (5, 7, 9)
    rng = np.random.default_rng(11)
    idx = sites(rng, agents, shape, "empty_agent", density=0.3)
    n, cells = len(idx), agents * 5 * 7 * 9
    cap = n + 10
    coords = _rows(idx, cap)
    for count in (n, n // 2, 1, 0):                                   # n // 2: fewer than the rows present
        vol = _full((cells + 8,), -1, torch.int32)
        vol[cells:] = SENT32
        cnt = _count(count)
        _scatter(coords, cnt, cap, agents, shape, vol, 1)
        v = vol.cpu().numpy()
        np.testing.assert_array_equal(v[:cells], index_volume(idx[:count], agents, shape), err_msg=f"count {count}")
        assert (v[cells:] == SENT32).all()
        _scatter(coords, cnt, cap, agents, shape, vol, 0)
        v = vol.cpu().numpy()
        assert (v[:cells] == -1).all() and (v[cells:] == SENT32).all(), f"count {count}: the undo left cells behind"


# ---- qv2x_sp_out_sites -----------------------------------------------------------------------------------------------------------------

def _out_sites(geom, shape, agents, idx, cap_out=None):
    """two calls (the second after the undo) against ``out_sites`` cut to the first ``cap_out`` rows; returns (kept rows, all rows)"""
    from oracle.spec_second import out_sites
    from quantv2x_amd import lib as L
    lib = L.load()
    allrows = out_sites(idx, shape, geom)
    cap_out = len(allrows) + 5 if cap_out is None else cap_out
    kept = allrows[:cap_out]
    cap_in = len(idx) + 3
    d, osh = _desc(geom, shape, agents, cap_in=cap_in, cap_out=cap_out)
    cells = agents * osh[0] * osh[1] * osh[2]
    in_c, n_in = _rows(idx, cap_in), _count(len(idx))
    vol = _full((cells + 8,), -1, torch.int32)
    vol[cells:] = SENT32
    out_c, n_out = _full((cap_out + 4, 4), SENT32, torch.int32), _count(SENT32)
    ws_bytes = int(lib.qv2x_sp_out_sites_workspace_bytes(C.byref(d)))
    assert ws_bytes == (cells + 1023) // 1024 * 4 + 16
    ws = _full((ws_bytes,), 0x55, torch.uint8)
    want_vol = np.full(cells, -1, np.int32)
    want_vol[linear(kept, osh)] = np.arange(len(kept), dtype=np.int32)
    for rep in range(2):
        out_c.fill_(SENT32), n_out.fill_(SENT32)
        L.check(lib.qv2x_sp_out_sites(C.byref(d), L.ptr(in_c), L.ptr(n_in), L.ptr(vol), L.ptr(out_c), L.ptr(n_out), L.ptr(ws), ws_bytes,
                                      L.current_stream()), "qv2x_sp_out_sites")
        torch.cuda.synchronize()
        n, oc, v = int(n_out.item()), out_c.cpu().numpy(), vol.cpu().numpy()
        assert n == len(kept), f"call {rep}: *n_out = {n}, expected {len(kept)} (of {len(allrows)} active, capacity {cap_out})"
        np.testing.assert_array_equal(oc[:n], kept, err_msg=f"call {rep}: out_coords")
        assert (oc[n:] == SENT32).all(), f"call {rep}: out_coords rows at or beyond *n_out were written"
        assert (v[:cells] != -2).all(), f"call {rep}: marks left in the volume"
        np.testing.assert_array_equal(v[:cells], want_vol, err_msg=f"call {rep}: out_volume")
        assert (v[cells:] == SENT32).all(), f"call {rep}: cells past the volume were written"
        _scatter(out_c, n_out, cap_out, agents, osh, vol, 0)          # how a frame leaves the volume: dropped cells are already -1
        assert int((vol[:cells] != -1).sum().item()) == 0, f"call {rep}: the undo left cells behind"
    return kept, allrows, osh


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("volume", list(VOLUMES))
@pytest.mark.parametrize("gname", list(STRIDED))
def test_out_sites(gname, volume, kind):
    """5x7x9 x 2: every output volume under 1024 cells (one count block, ragged).  13x30x37 x 3: several blocks, and cell counts that are no
    multiple of 4 (5985 for k3_s2_p1, 43 290 for k3_s1_p1), so the scalar tail of the count runs."""
    agents, shape = VOLUMES[volume]
    rng = np.random.default_rng(sum(map(ord, gname + volume + kind)))
    _out_sites(STRIDED[gname], shape, agents, sites(rng, agents, shape, kind, density=0.15))


def test_out_sites_full_and_empty_count_blocks():
    agents, shape = 3, (13, 30, 37)
    rng = np.random.default_rng(5)
    for gname in ("k3_s2_p1", "k3_s1_p1"):
        kept, _, osh = _out_sites(STRIDED[gname], shape, agents, sites(rng, agents, shape, "dense"))
        cells = agents * osh[0] * osh[1] * osh[2]
        per_block = np.bincount(linear(kept, osh) // 1024, minlength=(cells + 1023) // 1024)
        assert per_block[0] == 1024 and (per_block == 0).any() and cells % 4, (gname, per_block)


def test_out_sites_empty_input():
    kept, _, _ = _out_sites(STRIDED["k3_s2_p1"], (13, 30, 37), 3, np.zeros((0, 4), np.int32))
    assert len(kept) == 0


# two agents whose OUTPUT volume is 9 x 249 x 251: 1 124 982 cells = 1099 count blocks (the scan's second pass of 1024 and its carry),
# and no multiple of 4.  The sites reach the last blocks.
BIG_OUT = dict(agents=2, shape=(17, 497, 501), density=0.002)
_big = {}


def _big_sites():
    if not _big:
        rng = np.random.default_rng(2)
        _big["idx"] = sites(rng, BIG_OUT["agents"], BIG_OUT["shape"], "random", density=BIG_OUT["density"])
    return _big["idx"]


@pytest.mark.parametrize("cap", ["roomy", "half"])
def test_out_sites_scan_second_pass(cap):
    from oracle.spec_second import out_sites
    geom = STRIDED["k3_s2_p1"]
    idx = _big_sites()
    if "all" not in _big:
        _big["all"] = out_sites(idx, BIG_OUT["shape"], geom)
    n = len(_big["all"])
    kept, allrows, osh = _out_sites(geom, BIG_OUT["shape"], BIG_OUT["agents"], idx, cap_out=None if cap == "roomy" else n // 2)
    cells = BIG_OUT["agents"] * osh[0] * osh[1] * osh[2]
    assert osh == [9, 249, 251] and cells > 1024 * 1024 and cells % 4 == 2
    assert (linear(allrows, osh) // 1024 > 1024).sum() > 100          # rows whose offset needs the carry


@pytest.mark.parametrize("cap", ["true", "true-1", "half", "one"])
def test_out_sites_over_capacity(cap):
    """raster order, the first cap_out kept, the rest dropped: *n_out == cap_out, dropped cells back at -1"""
    from oracle.spec_second import out_sites
    agents, shape = 3, (13, 30, 37)
    geom = STRIDED["k3_s2_p1"]
    idx = sites(np.random.default_rng(9), agents, shape, "random", density=0.1)
    n = len(out_sites(idx, shape, geom))
    assert n > 2048
    cap_out = {"true": n, "true-1": n - 1, "half": n // 2, "one": 1}[cap]
    kept, _, _ = _out_sites(geom, shape, agents, idx, cap_out=cap_out)
    assert len(kept) == cap_out


# ---- qv2x_sp_rulebook ------------------------------------------------------------------------------------------------------------------

def _rulebook(geom, shape, agents, idx, slack=37):
    from oracle.spec_second import out_sites, rulebook
    from quantv2x_amd import lib as L
    oidx = idx if geom[0] else out_sites(idx, shape, geom)
    n, cap_in = len(oidx), len(idx) + 3
    cap_out = n + slack
    if cap_out % 256 == 0:
        cap_out += 1
    K = geom[1] * geom[2] * geom[3]
    d, osh = _desc(geom, shape, agents, cap_in=cap_in, cap_out=cap_out)
    in_vol = _t(index_volume(idx, agents, shape))                     # built on the host: the rulebook alone is under test
    out_c, n_out = _rows(oidx, cap_out), _count(n)
    nbr = _full((K, cap_out), SENT32, torch.int32)
    L.check(L.load().qv2x_sp_rulebook(C.byref(d), L.ptr(out_c), L.ptr(n_out), L.ptr(in_vol), L.ptr(nbr), L.current_stream()), "qv2x_sp_rulebook")
    torch.cuda.synchronize()
    want = rulebook(oidx, idx, shape, geom)
    want[want < 0] = cap_in                                           # absent neighbours read the fill row
    got = nbr.cpu().numpy()
    np.testing.assert_array_equal(got[:, :n], want)
    assert (got[:, n:] == SENT32).all(), "columns at or beyond the row count were written"
    return want


@pytest.mark.parametrize("kind", ["random", "corners", "seam", "dense", "empty_agent", "single"])
@pytest.mark.parametrize("volume", list(VOLUMES))
@pytest.mark.parametrize("gname", ["subm3", "subm_z3"] + list(STRIDED))
def test_rulebook(gname, volume, kind):
    geom = dict(STRIDED, subm3=SUBM3, subm_z3=SUBM_Z3)[gname]
    agents, shape = VOLUMES[volume]
    rng = np.random.default_rng(sum(map(ord, gname + volume + kind)) + 1)
    _rulebook(geom, shape, agents, sites(rng, agents, shape, kind, density=0.2))


def test_rulebook_grid_stride():
    """512 workgroups of 256 per window offset: above 131 072 rows a thread takes a second row"""
    agents, shape = 2, (11, 128, 128)
    idx = sites(np.random.default_rng(3), agents, shape, "random", density=0.4)
    assert len(idx) > 131072 + 256
    want = _rulebook(SUBM3, shape, agents, idx)
    assert (want[13] == np.arange(len(idx))).all()                    # the centre offset of a sub-manifold layer is the site itself


# ---- the two gather-GEMM entries -------------------------------------------------------------------------------------------------------

def _conv_sites(rng, n):
    """``n`` sites of two agents: a solid block (rows with all 27 neighbours), a lattice of step 3 (rows with none but themselves), the
    rest at random clear of the block"""
    shape = (8, 16, 16) if n <= 1000 else (8, 32, 32)
    if n == 1:
        return sites(rng, 2, shape, "single"), shape
    b = (4, 5, 5) if n >= 200 else (3, 3, 3) if n >= 28 else (0, 0, 0)
    g = np.stack(np.meshgrid(np.arange(b[0]), np.arange(b[1]), np.arange(b[2]), indexing="ij"), -1).reshape(-1, 3)
    block = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)
    g = np.stack(np.meshgrid(np.arange(0, shape[0], 3), np.arange(0, shape[1], 3), np.arange(0, shape[2], 3), indexing="ij"), -1).reshape(-1, 3)
    lattice = np.concatenate([np.ones((len(g), 1), np.int64), g], 1)
    lattice = lattice[rng.permutation(len(lattice))[: max(0, min(60, n - len(block)))]]
    rest = n - len(block) - len(lattice)
    g = np.stack(np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij"), -1).reshape(-1, 3)
    g = g[(g[:, 0] > b[0]) | (g[:, 1] > b[1]) | (g[:, 2] > b[2])]
    pool = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)
    c = np.concatenate([block, lattice, pool[rng.permutation(len(pool))[:rest]]])
    assert len(c) == n and len(np.unique(c, axis=0)) == n
    return np.ascontiguousarray(c[rng.permutation(n)].astype(np.int32)), shape


def _launch_conv(state, i, x, idx, shape, cap_out_slack, agents=2):
    """layer ``i`` of ``state`` through its C entry with the ORACLE's rulebook; checks rows, padded channels and sentinels"""
    from oracle.spec_second import OracleSecond, rulebook
    from quantv2x_amd import lib as L
    from quantv2x_amd.engine_second import _SpLayer
    lib = L.load()
    geom = [int(v) for v in state[f"second/{i}/geom"]]
    want, oidx, _ = OracleSecond(state).layer(i, x, idx, list(shape))
    nbr = rulebook(oidx, idx, shape, geom)
    n_in, n = len(idx), len(oidx)
    cap_in, cap_out = n_in + 2, n + cap_out_slack
    in_q = None if i == 0 else (float(state[f"second/{i - 1}/a_delta"]), float(state[f"second/{i - 1}/a_zp"]))
    ly = _SpLayer(state, i, in_q, _dev())
    zp = int(ly.out_q[1])
    nb = np.full((ly.K, cap_out), cap_in, np.int32)                   # columns past the row count: the fill row (they are never read)
    nb[:, :n] = np.where(nbr < 0, cap_in, nbr)
    nb_d, cnt = _t(nb), _count(n)
    out = _full((cap_out + 1, ly.cop), SENT, torch.int8)
    d, _ = _desc(geom, shape, agents, cin=ly.cip, cout=ly.cop, cap_in=cap_in, cap_out=cap_out, out_q=ly.out_q)
    if i == 0:
        feat = np.full((cap_in, 4), np.float32(SENTF), np.float32)
        feat[:n_in] = x
        fd = _t(feat)
        L.check(lib.qv2x_sp_conv_f32in(C.byref(d), L.ptr(fd), L.ptr(nb_d), L.ptr(cnt), L.ptr(ly.w), L.ptr(ly.bn_g), L.ptr(ly.bn_h), L.ptr(out),
                                       L.current_stream()), "qv2x_sp_conv_f32in")
    else:
        zx = int(in_q[1])
        feat = np.full((cap_in + 1, ly.cip), SENT, np.int8)
        feat[:n_in, : ly.ci] = (x.astype(np.int16) - 128).astype(np.int8)
        feat[:n_in, ly.ci:] = zx - 128                                # padded channels and the fill row: the real value 0
        feat[cap_in] = zx - 128
        fd = _t(feat)
        L.check(lib.qv2x_sp_conv_i8(C.byref(d), L.ptr(fd), L.ptr(nb_d), L.ptr(cnt), L.ptr(ly.w), L.ptr(ly.scale), L.ptr(ly.corr), L.ptr(ly.aw),
                                    L.ptr(ly.bn_g), L.ptr(ly.bn_h), L.ptr(out), L.current_stream()), "qv2x_sp_conv_i8")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    got = (o[:n, : ly.co].astype(np.int16) + 128).astype(np.uint8)
    np.testing.assert_array_equal(got, want)
    assert (o[:n, ly.co:] == zp - 128).all(), "padded output channels must hold the zero point: the next layer reads them"
    assert (o[n:] == SENT).all(), "rows at or beyond the row count (the fill row among them) were written"
    return want, nbr, ly


@pytest.mark.parametrize("zp", [0, 7])
@pytest.mark.parametrize("n,slack", [(1, 40), (255, 40), (256, 40), (257, 40), (300, 0)])
@pytest.mark.parametrize("gname", ["subm3", "subm_z3"])
def test_conv_f32in(gname, n, slack, zp):
    geom = {"subm3": SUBM3, "subm_z3": SUBM_Z3}[gname]
    rng = np.random.default_rng(1000 * n + 10 * zp + len(gname))
    idx, shape = _conv_sites(rng, n)
    state = second_state(rng, shape, [(4, 16, geom)], [zp], fill=0.2 if gname == "subm3" else 0.5)
    x = f32_features(rng, n)
    assert (x == 0).any() or n == 1
    want, nbr, _ = _launch_conv(state, 0, x, idx, shape, slack)
    if n >= 255 and gname == "subm3":
        per_row = (nbr >= 0).sum(axis=0)
        assert per_row.max() == 27 and per_row.min() == 1
        assert ((want > zp) & (want < 255)).mean() >= 1 / 3


# (K, cin, cout) padded <- two pairs of real channel counts
I8_FORMS = {
    "27_32_32": (SUBM3, [(16, 16), (20, 32)]),
    "27_32_64": (SUBM3, [(32, 64), (20, 48)]),
    "27_64_64": (SUBM3, [(64, 64), (48, 48)]),
    "3_64_64": (SUBM_Z3, [(64, 64), (48, 64)]),
    "3_64_128": (SUBM_Z3, [(64, 128), (48, 100)]),
}
I8_ROWS = [1, 31, 32, 33, 255, 256, 257, 2049]
I8_Q = [(0, 0), (3, 7), (11, 0), (0, 7), (3, 0), (11, 7)]            # (input zp, output zp): every pair, one per row count in turn


def _i8_state(rng, geom, ci, co, zx, zp, fill, shape):
    dx = np.float32(0.05)
    state = input_quantizer(0, dx, zx)
    state.update(layer_state(rng, 1, ci, co, geom, (dx, zx), uniform_stats(zx), zp, fill=fill))
    state["second/0/geom"] = np.array(SUBM3, dtype=np.int64)
    state["second/n_layers"], state["second/sparse_shape"] = np.int64(2), np.asarray(shape, dtype=np.int64)
    return state


@pytest.mark.parametrize("n", I8_ROWS)
@pytest.mark.parametrize("form", list(I8_FORMS))
def test_conv_i8(form, n):
    """n == cap_out at 32, 256 and 2049; a single row in a capacity of 5001 (twenty workgroups, nineteen of which leave at once)"""
    geom, pairs = I8_FORMS[form]
    j = I8_ROWS.index(n)
    ci, co = pairs[j % 2]
    zx, zp = I8_Q[(j + list(I8_FORMS).index(form)) % 6]
    rng = np.random.default_rng(100 * n + list(I8_FORMS).index(form))
    idx, shape = _conv_sites(rng, n)
    state = _i8_state(rng, geom, ci, co, zx, zp, 0.2 if geom is SUBM3 else 0.5, shape)
    x = codes_like(rng, n, ci)
    slack = 0 if n in (32, 256, 2049) else 5000 if n == 1 else 777
    want, nbr, ly = _launch_conv(state, 1, x, idx, shape, slack)
    assert (ly.K, ly.cip, ly.cop) == tuple(int(v) for v in form.split("_"))
    if n >= 255:
        assert ((want > zp) & (want < 255)).mean() >= 1 / 3, "reference output mostly saturated"
        if geom is SUBM3:
            per_row = (nbr >= 0).sum(axis=0)
            assert per_row.max() == 27 and per_row.min() == 1


@pytest.mark.parametrize("form", list(I8_FORMS))
def test_conv_i8_saturating(form):
    """codes at 0 and 255 against weight zero points at 0 and 255: the largest |T| a layer can form (27 * 64 * 255 * 255 < 2^31), outputs
    at both ends of the range, fl(T) rounded above 2^24"""
    geom, pairs = I8_FORMS[form]
    ci, co = pairs[0]
    n = 257
    rng = np.random.default_rng(len(form) + ci + co)
    idx, shape = _conv_sites(rng, n)
    state = _i8_state(rng, geom, ci, co, 11, 7, 0.2, shape)
    state["second/1/w_zp"] = np.where(np.arange(co) % 2 == 0, 0.0, 255.0).astype(np.float32)
    state["second/1/w_code"] = np.where(rng.random(state["second/1/w_code"].shape) < 0.5, 0, 255).astype(np.uint8)
    x = np.where(rng.random((n, ci)) < 0.5, 0, 255).astype(np.uint8)
    want, _, _ = _launch_conv(state, 1, x, idx, shape, 40)
    assert (want == 255).mean() > 0.1 and (want == 7).mean() > 0.1


def test_conv_i8_persistent_tile_loop():
    """(27, 64, 64): 108 KB of weights, one workgroup per CU, 256 workgroups of 256 rows: above 65 536 rows a wave takes a second tile"""
    agents, shape = 2, (6, 128, 128)
    rng = np.random.default_rng(8)
    n = 65536 + 8 * 32 + 19                                           # one more round of tiles for the first workgroup, the last tile ragged
    idx = sites(rng, agents, shape, "random", count=n)
    state = _i8_state(rng, SUBM3, 64, 64, 3, 7, 0.35, shape)
    x = codes_like(rng, n, 64)
    want, _, ly = _launch_conv(state, 1, x, idx, shape, 5, agents=agents)
    assert (ly.K, ly.cip, ly.cop) == (27, 64, 64) and ((want > 7) & (want < 255)).mean() >= 1 / 3


# ---- qv2x_sp_to_bev_i8 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,cp,D,H,W,agents,n,fill", [
    (128, 128, 2, 5, 7, 2, 50, -128),
    (64, 64, 2, 75, 77, 1, 9000, -121),          # more than 8192 rows: a workgroup takes a second row
    (100, 128, 3, 5, 9, 3, 200, 5),              # c_padded > c
    (3, 32, 1, 5, 7, 1, 20, -125),               # 7 * 9 * 3 = 189 bytes: no multiple of 16, the byte tail of the fill
    (3, 32, 1, 5, 7, 1, 0, 17),                  # zero rows: the fill alone
    (64, 96, 2, 3, 3, 2, 36, 127),               # every cell active
])
def test_to_bev(c, cp, D, H, W, agents, n, fill):
    from quantv2x_amd import lib as L
    rng = np.random.default_rng(c + n)
    idx = sites(rng, agents, (D, H, W), "random", count=n)
    cap = n + 6
    feat = np.full((cap + 1, cp), SENT, np.int8)
    feat[:n, :c] = rng.integers(-128, 128, size=(n, c), dtype=np.int8)
    nbytes = agents * (H + 2) * (W + 2) * c * D
    bev = _full((nbytes + 32,), SENT, torch.int8)
    fd, cd, cnt = _t(feat), _rows(idx, cap), _count(n)
    L.check(L.load().qv2x_sp_to_bev_i8(L.ptr(fd), L.ptr(cd), L.ptr(cnt), cap, c, cp, agents, D, H, W, fill, L.ptr(bev), L.current_stream()),
            "qv2x_sp_to_bev_i8")
    torch.cuda.synchronize()
    want = np.full((agents, H + 2, W + 2, c, D), fill, np.int8)
    want[idx[:, 0], idx[:, 2] + 1, idx[:, 3] + 1, :, idx[:, 1]] = feat[:n, :c]
    got = bev.cpu().numpy()
    np.testing.assert_array_equal(got[:nbytes].reshape(want.shape), want)
    assert (got[nbytes:] == SENT).all(), "bytes past the map were written"


# ---- whole synthetic encoders ----------------------------------------------------------------------------------------------------------

CHAIN_SHAPE = (21, 30, 37)             # -> (11, 15, 19) -> (5, 8, 10) -> (2, 8, 10): odd at every level but the last
CHAIN_ZPS = [3, 7, 5, 11, 2]
BIG = 10 ** 9


def _chain(agents, empty, channels, caps_of):
    from oracle.spec_second import OracleSecond
    from quantv2x_amd.engine_second import DeployedSecondEncoder
    rng = np.random.default_rng(17 + agents)
    state = second_state(rng, CHAIN_SHAPE, chain_layers(channels), CHAIN_ZPS, fill=CHAIN_FILLS)
    sc = chain_scene(rng, agents, CHAIN_SHAPE, empty=empty)
    orc = OracleSecond(state)
    to, tg = {}, {}
    want = orc.forward(sc, to, batch_size=agents)
    true = [len(to[f"second/{i}"][1]) for i in (1, 2, 4)]
    caps = None
    if caps_of is not None:
        caps = caps_of(true)
        to = {}
        want = orc.forward(sc, to, batch_size=agents, site_caps=caps)
        for i, c in zip((1, 2, 4), caps):
            assert c == BIG or len(to[f"second/{i}"][1]) == c, f"layer {i}: the capacity {c} is not below the true count"
    m = len(sc["voxel_coords"])
    eng = DeployedSecondEncoder(state, "cuda:0", agents=agents, max_voxels=m, max_points=5, site_caps=caps)
    for lv, i in zip(eng.levels[1:], (1, 2, 4)):
        assert caps is not None or lv.cap >= len(to[f"second/{i}"][1])
    inp = {k: _t(v) for k, v in sc.items()}
    for rep in range(2):                                              # the second pass proves the index volumes were left clean
        tg.clear()
        bev = eng(inp, tg)
        torch.cuda.synchronize()
        for i in range(5):
            oc, oi, osh = to[f"second/{i}"]
            f, coords, count, co, gsh = tg[f"second/{i}"]
            n = int(count.item())
            assert n == len(oi) and list(gsh) == list(osh), f"pass {rep}, layer {i}: {n} rows, the oracle has {len(oi)}"
            np.testing.assert_array_equal(coords[:n].cpu().numpy(), oi, err_msg=f"pass {rep}, layer {i}: coordinates")
            rows = f[:n].cpu().numpy()
            np.testing.assert_array_equal((rows[:, :co].astype(np.int16) + 128).astype(np.uint8), oc, err_msg=f"pass {rep}, layer {i}: codes")
            assert (rows[:, co:] == CHAIN_ZPS[i] - 128).all(), f"pass {rep}, layer {i}: padded channels"
        np.testing.assert_array_equal(eng.dense_codes(bev).cpu().numpy(), want, err_msg=f"pass {rep}: dense codes")
        for l in eng.levels:
            assert int((l.volume != -1).sum().item()) == 0, f"pass {rep}: an index volume was not left clean"


@pytest.mark.parametrize("channels", [(16, 32, 64, 64, 128), (16, 20, 48, 48, 100)])
@pytest.mark.parametrize("agents,empty", [(1, None), (2, 1), (3, 1)])
def test_chain(agents, empty, channels):
    _chain(agents, empty, channels, None)


@pytest.mark.parametrize("which", ["one_level", "two_levels"])
def test_chain_over_capacity(which):
    """``site_caps`` below the true counts: both sides keep the first rows in raster order, and every later level follows from those"""
    caps_of = {"one_level": lambda t: [BIG, t[1] // 2, BIG], "two_levels": lambda t: [t[0] // 2, t[1] // 3, BIG]}[which]
    _chain(3, 1, (16, 32, 64, 64, 128), caps_of)
