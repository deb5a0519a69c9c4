"""Random SECOND-encoder states in the key format of ``ptq_state.export_second_state`` and site sets that sit where sparse kernels go
wrong (no tests here).  ``OracleSecond`` and the engine's ``_SpLayer`` / ``DeployedSecondEncoder`` read the same dict.

Steps, chosen so that the reference output of a layer is not mostly saturated:

  T = sum over the ACTIVE window offsets and the cin real channels of (x - zx)(w - zw):  n = max(1, fill * K) * cin  terms, ``fill`` the
  expected active share of a window.  Weight codes are uniform on 0..255 (std 73.9) and an ordinary channel's zw is the rounded mean of its
  own codes +- 1, so rms(w - zw) ~ 74 and |sum(w - zw)| <= 1.5 K cin: the offset  mean(x - zx) * sum(w - zw)  stays below the spread
  std(T) ~ sqrt(n) * rms(x - zx) * 74  whatever share of the window a site really has (a zw far from the mean -- up to 18 per term in
  tests/_pyramid_layers.py -- would move whole channels with the number of neighbours).  The weight step is set so that
  sigma = std(T) * dx * mean(dw) = 1, i.e.  dw ~ 1 / (dx * sqrt(K cin fill) * rms(x - zx) * 74):  the steps scale with sqrt(K * cin).
  BatchNorm:  |g| in [0.8, 1.25) with a random sign, h = N(0.3, 0.3) * |g| - g * (offset at the expected fill), never 0, so that
  y = T * scale * g + h ~ N(0.3, 1) * |g|.  The activation step puts 4 sigma at the end of the code range, a_delta = 4 / (255 - a_zp)
  (one more sigma than the 2-D builders: |g| * dw reaches 1.56 and a crowded site has up to 1 / fill times the expected terms).  About
  60 % of the outputs are then positive and under 1 % reach 255.
  Two channels per layer sit at the extremes zw = 0 and zw = 255, where (w - zw) has one sign: their step is cut so that a FULL window
  of average inputs lands at 2 sigma, and nothing is taken out of h.

A layer built here with ReLU has  code - zp = span * max(|g| (z + 0.3), 0) / 4,  z ~ N(0, 1):  mean 0.142 span, rms 0.222 span
(``relu_stats``), which is what the next layer's step is derived from.
"""
import numpy as np

W_RMS = 74.0            # rms of (w - zw): w uniform on 0..255, zw within 1.5 of the channel's mean code

# (subm, kz, ky, kx, sz, sy, sx, pz, py, px)
SUBM3 = [1, 3, 3, 3, 1, 1, 1, 1, 1, 1]
SUBM_Z3 = [1, 3, 1, 1, 1, 1, 1, 1, 0, 0]                   # three offsets, every row count reachable (the (3, *, *) forms of the GEMM)
STRIDED = {
    "k3_s2_p1": [0, 3, 3, 3, 2, 2, 2, 1, 1, 1],
    "k3_s2_p011": [0, 3, 3, 3, 2, 2, 2, 0, 1, 1],
    "k311_s211_p0": [0, 3, 1, 1, 2, 1, 1, 0, 0, 0],
    "k3_s1_p1": [0, 3, 3, 3, 1, 1, 1, 1, 1, 1],
    "k2_s2_p0": [0, 2, 2, 2, 2, 2, 2, 0, 0, 0],
    "k133_s122_p011": [0, 1, 3, 3, 1, 2, 2, 0, 1, 1],
}
# the five-layer chain of the issue: sub-manifold, stride 2, stride 2 with padding (0, 1, 1), sub-manifold, window (3, 1, 1)
CHAIN_GEOMS = [SUBM3, STRIDED["k3_s2_p1"], STRIDED["k3_s2_p011"], SUBM3, STRIDED["k311_s211_p0"]]
# expected active share of each layer's window for a scene of density 0.08: about three neighbours of 27 at the two sparse levels, then the
# strided levels fill up (85 % and 100 % of their cells are active)
CHAIN_FILLS = [0.12, 0.12, 0.8, 0.7, 1.0]


def uniform_stats(zx):
    """(mean, rms) of (x - zx) for codes uniform on 0..255"""
    m = 127.5 - zx
    return m, float(np.sqrt(73.9 ** 2 + m * m))


def relu_stats(zp):
    """(mean, rms) of (code - zp) of a layer built here (see the module docstring)"""
    span = 255.0 - zp
    return 0.142 * span, 0.222 * span


def layer_state(rng, i, cin, cout, geom, in_q, in_stats, a_zp, fill=0.3):
    """``second/<i>/...`` of one sparse layer.  ``in_q`` = (delta, zp) of the input codes, None for the fp32 layer 0 (``in_stats`` is then
    the (mean, rms) of the fp32 features themselves)."""
    K = int(geom[1] * geom[2] * geom[3])
    p = f"second/{i}/"
    code = rng.integers(0, 256, size=(K, cin, cout), dtype=np.uint8)
    zw = np.clip(np.rint(code.reshape(-1, cout).mean(axis=0)) + rng.integers(-1, 2, size=cout), 0, 255).astype(np.float32)
    lo, hi = rng.choice(cout, size=2, replace=False)
    zw[lo], zw[hi] = 0.0, 255.0
    dx = 1.0 if in_q is None else float(in_q[0])
    n = max(1.0, fill * K) * cin
    dw = rng.uniform(0.8, 1.25, size=cout) / (dx * np.sqrt(n) * in_stats[1] * W_RMS)
    full = abs(in_stats[0]) * 127.5 * K * cin + in_stats[1] * 147.0 * np.sqrt(K * cin)
    dw[[lo, hi]] = 2.0 / (dx * full)
    dw = dw.astype(np.float32)
    mag = rng.uniform(0.8, 1.25, size=cout)
    g = (mag * rng.choice([-1.0, 1.0], size=cout)).astype(np.float32)
    wsum = (code.reshape(-1, cout).astype(np.float64) - zw[None, :]).sum(axis=0)
    offset = in_stats[0] * wsum * min(1.0, max(fill, 1.0 / K)) * dx * dw
    offset[[lo, hi]] = 0.0
    h = rng.normal(0.3, 0.3, size=cout) * mag - g * offset
    h = np.where(np.abs(h) < 1e-3, 0.05, h).astype(np.float32)
    return {p + "w_code": code, p + "w_delta": dw, p + "w_zp": zw, p + "bn_g": g, p + "bn_h": h,
            p + "a_delta": np.float32(4.0 / (255.0 - a_zp)), p + "a_zp": np.float32(a_zp), p + "geom": np.array(geom, dtype=np.int64)}


def input_quantizer(i, delta, zp):
    """the two keys of layer ``i`` that the next layer reads: the quantizer of ITS input codes"""
    return {f"second/{i}/a_delta": np.float32(delta), f"second/{i}/a_zp": np.float32(zp)}


def second_state(rng, sparse_shape, layers, a_zps, fill=0.3, f32_stats=(0.0, 1.0)):
    """A whole encoder state.  ``layers``: [(cin, cout, geom), ...], layer 0 = (4, 16, geom) with fp32 input; ``a_zps``: one output zero
    point per layer; ``fill``: one value or one per layer.  Padded forms (K, cin, cout) the engine deploys after layer 0: (27,32,32), (27,32,64), (27,64,64), (3,64,64), (3,64,128);
    real channel counts pad upward to the next multiple of 32."""
    assert len(layers) == len(a_zps) and tuple(layers[0][:2]) == (4, 16)
    st = {"second/n_layers": np.int64(len(layers)), "second/sparse_shape": np.asarray(sparse_shape, dtype=np.int64)}
    in_q, stats = None, f32_stats
    for i, ((cin, cout, geom), zp) in enumerate(zip(layers, a_zps)):
        assert i == 0 or cin == layers[i - 1][1]
        st.update(layer_state(rng, i, cin, cout, geom, in_q, stats, zp, fill[i] if isinstance(fill, (list, tuple)) else fill))
        in_q, stats = (st[f"second/{i}/a_delta"], zp), relu_stats(zp)
    return st


def chain_layers(channels=(16, 32, 64, 64, 128)):
    """the issue's five layers with the given output channel counts"""
    cins = (4,) + tuple(channels[:-1])
    return [(ci, co, g) for ci, co, g in zip(cins, channels, CHAIN_GEOMS)]


# ---- site sets ---------------------------------------------------------------------------------------------------------------------------

KINDS = ("random", "corners", "dense", "single", "seam", "empty_agent")


def _unlin(lin, shape):
    d, h, w = shape
    lin = np.asarray(lin, dtype=np.int64)
    return np.stack([lin // (d * h * w), (lin // (h * w)) % d, (lin // w) % h, lin % w], 1)


def sites(rng, agents, shape, kind, density=0.1, count=None, empty=None):
    """int32 rows (agent, z, y, x), unique, shuffled.  Kinds:
      random        every cell with probability ``density`` (or exactly ``count`` cells)
      corners       all eight corners of every agent, four points inside each face and two along each edge
      dense         agent 0 full over its first ceil(D / 2) z-planes (whole 1024-cell blocks of marks), nothing behind them
      single        one site
      seam          the last cell of agent a and the first cell of agent a + 1, with their neighbours along every axis
      empty_agent   random, but agent ``empty`` (default: the middle one) has no site"""
    d, h, w = [int(v) for v in shape]
    cells = agents * d * h * w
    if kind in ("random", "empty_agent"):
        if count is not None:
            lin = rng.choice(cells, size=count, replace=False)
        else:
            lin = np.nonzero(rng.random(cells) < density)[0]
        c = _unlin(lin, shape)
        if kind == "empty_agent":
            c = c[c[:, 0] != (agents // 2 if empty is None else empty)]
    elif kind == "corners":
        rows = []
        ends = [(0, d - 1), (0, h - 1), (0, w - 1)]
        size = (d, h, w)
        for b in range(agents):
            for z in ends[0]:
                for y in ends[1]:
                    for x in ends[2]:
                        rows.append((b, z, y, x))
            for ax in range(3):                                       # faces: one axis at an end, the two others anywhere
                for e in ends[ax]:
                    for _ in range(4):
                        p = [int(rng.integers(0, s)) for s in size]
                        p[ax] = e
                        rows.append((b, *p))
            for ax in range(3):                                       # edges: two axes at their ends, the third anywhere
                o = [a for a in range(3) if a != ax]
                for e0 in ends[o[0]]:
                    for e1 in ends[o[1]]:
                        for _ in range(2):
                            p = [0, 0, 0]
                            p[ax], p[o[0]], p[o[1]] = int(rng.integers(0, size[ax])), e0, e1
                            rows.append((b, *p))
        c = np.unique(np.array(rows, dtype=np.int64), axis=0)
    elif kind == "dense":
        planes = (d + 1) // 2
        c = _unlin(np.arange(planes * h * w), shape)
    elif kind == "single":
        c = _unlin([int(rng.integers(0, cells))], shape)
    elif kind == "seam":
        rows = []
        for b in range(agents - 1):
            rows += [(b, d - 1, h - 1, w - 1), (b + 1, 0, 0, 0)]
            for ax in range(3):
                for step in (1, 2):
                    lo, hi = [0, 0, 0], [d - 1, h - 1, w - 1]
                    lo[ax] = min(step, hi[ax])
                    hi[ax] = max(hi[ax] - step, 0)
                    rows += [(b, *hi), (b + 1, *lo)]
        c = np.unique(np.array(rows, dtype=np.int64), axis=0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(c[rng.permutation(len(c))].astype(np.int32))


def linear(idx, shape):
    i = idx.astype(np.int64)
    return ((i[:, 0] * shape[0] + i[:, 1]) * shape[1] + i[:, 2]) * shape[2] + i[:, 3]


def index_volume(idx, agents, shape):
    """the dense volume ``qv2x_sp_index_scatter`` leaves: row at every site, -1 elsewhere (flat int32)"""
    vol = np.full(agents * int(shape[0]) * int(shape[1]) * int(shape[2]), -1, np.int32)
    vol[linear(idx, shape)] = np.arange(len(idx), dtype=np.int32)
    return vol


def codes_like(rng, n, c):
    """uint8 input codes of both signs around any zero point, with exact 0 and 255 among them"""
    x = rng.integers(0, 256, size=(n, c), dtype=np.uint8)
    m = rng.random((n, c))
    x[m < 0.02] = 0
    x[m > 0.98] = 255
    return x


def f32_features(rng, n):
    """fp32 voxel means of both signs with exact zeros"""
    x = rng.normal(0.0, 1.0, size=(n, 4)).astype(np.float32)
    x[rng.random((n, 4)) < 0.05] = 0.0
    return x


def chain_scene(rng, agents, shape, density=0.08, empty=None, max_points=5):
    """voxelizer output for ``OracleSecond.forward`` / ``DeployedSecondEncoder``: unused point slots are zero, some voxels claim 0 points"""
    idx = sites(rng, agents, shape, "empty_agent" if empty is not None else "random", density=density, empty=empty)
    n = len(idx)
    vf = rng.normal(0.0, 1.0, size=(n, max_points, 4)).astype(np.float32)
    npnt = rng.integers(0, max_points + 1, size=n).astype(np.int32)
    vf[np.arange(max_points)[None, :] >= np.maximum(npnt, 1)[:, None]] = 0.0
    return {"voxel_features": vf, "voxel_coords": idx, "voxel_num_points": npnt}
