"""Cases, operands, references, launches and checks for qv2x_pfn_scatter_i8 and qv2x_pfn_unscatter_i8 (csrc/pfn_scatter.hip); no tests here.

Used by tests/test_pfn_cases_cpu.py (no GPU: the references pinned, every case's aim asserted) and tests/test_hip_pfn_cases.py (GPU).

**Reference.**  The pillar codes are ``orc_pfn`` (oracle/qv2x_oracle.c): every slot through both quantizers with IEEE division, then the max.
The kernel takes the max first, quantizes once through the division-exact sandwich and reads the second quantizer from a 256-entry table:
equal bytes also test that reordering.  ``ref64`` restates PillarVFE + QuantPFNLayer in float64 with ``pfn_ref64``'s bound; the CPU file
holds ``orc_pfn`` against it wherever the float64 value is farther than the bound from every rounding boundary of the first quantizer.

**Canvas.**  ``Prepared.before()`` is the padded canvas ``[N][ny + 2][nx + 2][64]`` as the engines hand it over -- the interior full of
``z2 - 128`` -- except that the pad ring holds ``ring_byte(q)``, a byte no code of the second quantizer's table maps to and not the fill.
``after()`` has the 64 bytes ``code - 128`` of every pillar with ``0 <= b < N``, ``0 <= y < ny``, ``0 <= z + x < nx`` at ``(b, y + 1, z + x + 1)``
and nothing else changed.  On the GPU the canvas lies between two guard planes of one agent's size each, full of ``GUARD``: a pillar with
agent -1 or N that got through the bounds test would land there, not outside the allocation.

**Cases** (``CASES``; ``build(name, cus)``).  Random-weight cases draw Linear(10 -> 64) as ``_fp32_kernels.pfn_weights`` does (channel
CH_MASKED can only be won by a masked slot, channel CH_DEAD is dead).  Tap cases use one-point pillars with P = 1 and weights that copy one of
x, y, z, intensity into a channel (channel c taps feature c % 4, intensity for c % 4 == 3), bias 0: the value in front of the first quantizer
is the operand itself, bit for bit, and the four bytes of a lane's dword see four different values.
"""
import ctypes as C
import math

import numpy as np

CH_MASKED, CH_DEAD = 3, 7
GRID = (2, 4, 6)                                            # N, ny, nx of the fp32 section
VOX = np.array([0.4, 0.3, 4.0], np.float32)                 # three different sizes: an x / y swap changes the centre features
OFF = np.array([-1.0, -0.55, -1.0], np.float32)             # centre of voxel 0 (voxel / 2 + range minimum)
GUARD = np.int8(0x5A)                                       # guard planes around the device canvas; also the fill of the un-scatter-alone canvas
UNSCATTER_VALUES = (-128, 0, 127)
U = 2.0 ** -24


class Quant:
    """the two activation quantizers of the layer: (d1, z1) on the Linear's output, (d2, z2) after the ReLU"""

    def __init__(self, name, d1, z1, d2, z2):
        self.name, self.d1, self.z1, self.d2, self.z2 = name, np.float32(d1), np.float32(z1), np.float32(d2), np.float32(z2)


# QA: the post-ReLU setting of real states (z2 = 0); d1 a power of two, so (k + 1/2) d1 are exact ties and 1 / d1 is exact.
# QB: z2 > 0, z1 in the middle of the range, neither step a power of two.
# Both d2 keep (c - z1) d1 / d2 at least 8e-3 away from every half-integer for all 256 codes c: the table is the same in fp32 and in float64
# (0.0145 or 0.0172 would put an entry within 2e-6 of a boundary, where the two disagree).
QA = Quant("qa", 2.0 ** -5, 100, 0.014585, 0)
QB = Quant("qb", 0.0237, 131, 0.0171, 7)
QUANTS = {"qa": QA, "qb": QB}


def q_code32(y, d, z):
    """oracle/qv2x_oracle.c:q_code in numpy float32: clamp(rint(y / d) + z, 0, 255), the division and the sum rounded to fp32"""
    y = np.asarray(y, np.float32)
    t = np.rint(y / np.float32(d)).astype(np.float32) + np.float32(z)
    return np.clip(t, np.float32(0), np.float32(255))


def table32(q):
    """final code of every first-quantizer code 0..255, by the oracle's fp32 expressions: dequantize, ReLU, second quantizer"""
    c = np.arange(256, dtype=np.float32)
    y1 = np.maximum((c - q.z1) * q.d1, np.float32(0))
    return q_code32(y1, q.d2, q.z2).astype(np.uint8)


def table64(q):
    """(the same table in float64, the distance of (c - z1) d1 / d2 from the nearest half-integer)"""
    c = np.arange(256, dtype=np.float64)
    t = np.maximum((c - float(q.z1)) * float(q.d1), 0.0) / float(q.d2)
    return np.clip(np.rint(t) + float(q.z2), 0, 255).astype(np.uint8), np.abs(t - np.floor(t) - 0.5)


def ring_byte(q):
    """a byte no pillar can write under ``q`` (no entry of the table maps to it) that is not the fill either"""
    free = sorted(set(range(256)) - set(table32(q).tolist()) - {int(q.z2)})
    assert free, "every byte value is a code of this quantizer pair"
    return np.int8(free[0] - 128)


def rounds_rule(m, cus):
    """the host's launch rule of qv2x_pfn_scatter_i8: rounds of 16 pillars per workgroup"""
    return min(8, max(1, m // (128 * cus)))


def multi_round_m(rounds, cus):
    return {2: 2 * 128 * cus + 32 * 2 + 5, 8: 8 * 128 * cus + 128 * 3 + 21}[rounds]


def pfn_weights(rng):
    """as _fp32_kernels.pfn_weights: channel CH_MASKED = 0.5 - intensity (intensity >= 0.1: only a masked slot reaches the bias 0.5, five
    steps of either d1 above every real point); channel CH_DEAD has bias -100: first code 0, and the ReLU makes the final code z2"""
    w = (rng.standard_normal((64, 10)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(64) * 0.3).astype(np.float32)
    w[CH_MASKED] = 0.0
    w[CH_MASKED, 3] = -1.0
    b[CH_MASKED] = 0.5
    b[CH_DEAD] = -100.0
    return w, b


def tap_weights():
    w = np.zeros((64, 10), np.float32)
    w[np.arange(64), np.arange(64) % 4] = 1.0
    return w, np.zeros(64, np.float32)


def spread(count, n, ny, nx):
    """``count`` distinct cells (b, y, column), walked with a stride coprime to the cell count: neighbours in the list are far apart"""
    cells = n * ny * nx
    assert count <= cells
    stride = max(1, int(cells * 0.382))
    while math.gcd(stride, cells) != 1:
        stride += 1
    k = (np.arange(count, dtype=np.int64) * stride + cells // 3) % cells
    return k // (ny * nx), (k % (ny * nx)) // nx, k % nx


def outside_rows(n, ny, nx):
    """eight pillars (b, z, y, x) outside the canvas, one per side of each axis; the last two leave through z"""
    return [(-1, 0, 1, 1), (n, 0, 1, 1), (0, 0, -1, 2), (0, 0, ny, 2), (0, 0, 2, -1), (0, 0, 2, nx), (0, 1, 2, nx - 1), (0, -1, 2, 0)]


def random_features(rng, coords, npts, P, vox, off):
    """points around the pillar's own centre, intensity in [0.1, 1); the slots past min(np, P) hold zeros"""
    m = len(npts)
    centre = coords[:, [3, 2, 1]].astype(np.float64) * vox.astype(np.float64) + off.astype(np.float64)
    vf = np.empty((m, P, 4))
    vf[..., :3] = centre[:, None, :] + rng.uniform(-0.5, 0.5, (m, P, 3)) * vox.astype(np.float64)
    vf[..., 3] = rng.uniform(0.1, 1.0, (m, P))
    vf[np.arange(P)[None, :] >= np.minimum(npts, P)[:, None]] = 0.0
    return vf.astype(np.float32)


class Prepared:
    """operands of one case; ``codes`` (the oracle's, computed once), ``before()`` / ``after()`` the expected canvases"""

    def __init__(self, name, aim, kind, q, P, grid, coords, npts, vf, w, b, vox=VOX, off=OFF, **facts):
        self.name, self.aim, self.kind, self.q, self.P, self.facts = name, aim, kind, q, P, facts
        self.N, self.ny, self.nx = grid
        self.coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4)
        self.npts = np.ascontiguousarray(npts, dtype=np.int32)
        self.vf = np.ascontiguousarray(vf, dtype=np.float32)
        self.w, self.b, self.vox, self.off = (np.ascontiguousarray(a, dtype=np.float32) for a in (w, b, vox, off))
        self.M = len(self.npts)
        assert self.vf.shape == (self.M, P, 4) and self.coords.shape == (self.M, 4)
        assert np.abs(self.coords).max() < 2 ** 20, "z + x is a signed sum: keep the coordinates far from INT_MAX"
        bb, z, y, x = (self.coords[:, i].astype(np.int64) for i in range(4))
        col = z + x
        self.inside = (bb >= 0) & (bb < self.N) & (y >= 0) & (y < self.ny) & (col >= 0) & (col < self.nx)
        self.cell = ((bb * (self.ny + 2) + y + 1) * (self.nx + 2) + col + 1)[self.inside]
        assert len(np.unique(self.cell)) == len(self.cell), "two pillars share a cell: the kernel's order between waves is not defined"
        assert (self.npts[self.inside] >= 1).all(), "np = 0 inside the canvas: the reference's mean is 0 / 0, outside the contract"
        real = np.minimum(self.npts, P)
        assert (self.vf[np.arange(P)[None, :] >= real[:, None]] == 0).all(), "padding slots must hold zeros"
        self._codes = None

    @property
    def codes(self):
        """orc_pfn: u8 [M][64]"""
        if self._codes is None:
            from oracle.spec import _cf, _p, lib as olib
            q = self.q
            out = np.zeros((self.M, 64), np.uint8)
            with np.errstate(all="ignore"):
                olib().orc_pfn(_p(self.vf), _p(self.coords), _p(self.npts), self.M, self.P, _p(self.w), _p(self.b), _cf(q.d1), _cf(q.z1),
                               _cf(q.d2), _cf(q.z2), _p(self.vox), _p(self.off), _p(out))
            self._codes = out
        return self._codes

    def before(self):
        c = np.full((self.N, self.ny + 2, self.nx + 2, 64), ring_byte(self.q), np.int8)
        c[:, 1:-1, 1:-1] = np.int8(int(self.q.z2) - 128)
        return c

    def after(self):
        c = self.before()
        c.reshape(-1, 64)[self.cell] = (self.codes[self.inside].astype(np.int16) - 128).astype(np.int8)
        return c

    def unscattered(self, value, fill=GUARD):
        """the expected canvas after qv2x_pfn_unscatter_i8(value) alone on one full of ``fill``"""
        c = np.full((self.N, self.ny + 2, self.nx + 2, 64), fill, np.int8)
        c.reshape(-1, 64)[self.cell] = np.int8(value)
        return c


# ---- the float64 statement --------------------------------------------------------------------------------------------------------------------

def ref64(prep, rows=None):
    """PillarVFE + QuantPFNLayer in float64 on the rows ``rows`` (default: every row with np >= 1), as _fp32_kernels.pfn_ref64: ten features,
    the mean over all P slots divided by the reported count, Linear, zero-masked slots contribute the bias, max over the slots; then the first
    quantizer, dequantize, ReLU, the second quantizer.  Returns (rows, code [m][64], y [m][64] in front of the first quantizer,
    bound [m][64], near [m][64]): the bound is pfn_ref64's -- (10 + 2) 2^-24 (sum_k |f_k w_k| + |b|) for the fma chain, the bias add and the
    quantizer's division, plus sum_k |w_k| df_k for what the fp32 mean and centre features carry in -- and ``near`` marks the elements whose
    y lies within the bound of a rounding boundary (k + 1/2) d1 of the first quantizer: there fp32 may legitimately round the other way."""
    if rows is None:
        rows = np.flatnonzero(prep.npts >= 1)
    q, P = prep.q, prep.P
    vf, w, b = prep.vf[rows].astype(np.float64), prep.w.astype(np.float64), prep.b.astype(np.float64)
    vox, off = prep.vox.astype(np.float64), prep.off.astype(np.float64)
    npt = prep.npts[rows].astype(np.float64)[:, None]
    real = np.minimum(prep.npts[rows], P)
    xyz = vf[..., :3]
    mean = xyz.sum(axis=1) / npt
    dmean = U * (real[:, None] + 1) * np.abs(xyz).sum(axis=1) / npt
    cidx = prep.coords[rows][:, [3, 2, 1]].astype(np.float64)
    centre = cidx * vox + off
    dcentre = U * 2 * (np.abs(cidx * vox) + np.abs(off))
    dm, dc = xyz - mean[:, None, :], xyz - centre[:, None, :]
    f = np.concatenate([vf, dm, dc], axis=-1)                                                        # [m][P][10]
    df = np.concatenate([np.zeros_like(vf), dmean[:, None, :] + U * np.abs(dm), dcentre[:, None, :] + U * np.abs(dc)], axis=-1)
    val = f @ w.T + b
    vb = 12 * U * (np.abs(f) @ np.abs(w).T + np.abs(b)) + df @ np.abs(w).T
    masked = np.arange(P)[None, :] >= real[:, None]
    val[masked], vb[masked] = b, 0.0
    y, bound = val.max(axis=1), vb.max(axis=1)
    d1, z1 = float(q.d1), float(q.z1)
    t = y / d1
    c1 = np.clip(np.rint(t) + z1, 0, 255).astype(np.int64)
    near = np.abs(t - np.floor(t) - 0.5) * d1 <= bound
    return rows, table64(q)[0][c1], y, bound, near


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------

def _random_case(name, aim, q, P, grid, coords, npts, seed, vox=VOX, off=OFF, **facts):
    rng = np.random.default_rng(9000 + seed)
    w, b = pfn_weights(rng)
    coords, npts = np.asarray(coords, np.int32).reshape(-1, 4), np.asarray(npts, np.int32)
    return Prepared(name, aim, "random", q, P, grid, coords, npts, random_features(rng, coords, npts, P, vox, off), w, b, vox, off, **facts)


def _plain_coords(m, grid):
    bb, y, x = spread(m, *grid)
    return np.stack([bb, np.zeros_like(bb), y, x], axis=1)


def slot_counts(P):
    """point counts 1, P - 1, P and np > P"""
    return sorted({1, max(P - 1, 1), P, P + 4})


def _slots(name, q, P, seed):
    counts = slot_counts(P)
    npts = [counts[i % len(counts)] for i in range(3 * len(counts))]
    return _random_case(name, f"P = {P}: point counts {counts}, three pillars of each", q, P, GRID, _plain_coords(len(npts), GRID), npts, seed)


def _pillars(name, q, m, seed):
    grid = GRID if m <= GRID[0] * GRID[1] * GRID[2] else (2, 5, 7)
    npts = [1 + (i * 3) % 5 for i in range(m)]                                      # 1 4 2 5 3 with P = 3: masked, full and np > P
    return _random_case(name, f"M = {m}: 16 pillars per round (scatter), 64 per workgroup (un-scatter)", q, 3, grid, _plain_coords(m, grid), npts, seed)


PLACEMENT_P = 5


def placement_rows():
    """(live, outside, tail) rows (b, z, y, x, np) of the placement case on GRID"""
    n, ny, nx = GRID
    last = n - 1
    live = [(0, 1, 1, 2, 3), (0, 2, 2, 1, 5), (0, -1, 3, 1, 2), (0, 0, 0, 4, 1),                    # z = 1, 2 land at x + z; z = -1, x = 1: column 0
            (last, -1, 0, 1, 4), (last, 0, 0, nx - 1, 9), (last, 0, ny - 1, 0, 1), (last, 2, ny - 1, nx - 3, 5)]    # the last agent's corners
    outside = [r + (3,) for r in outside_rows(n, ny, nx)]
    tail = [(-1, -1, -1, -1, 0)] * 5                                                                  # the voxelizer's rows past its count
    return live, outside, tail


def _placement(name, q, seed):
    live, outside, tail = placement_rows()
    rows = [tail[0]]
    for i in range(8):
        rows += [live[i], outside[i]] + ([tail[1 + i // 2]] if i % 2 else [])
    rows = np.array(rows, np.int32)
    return _random_case(name, "z = 1, 2, -1; the last agent's corners; eight pillars outside, one per side; tail rows between live ones", q,
                        PLACEMENT_P, GRID, rows[:, :4], rows[:, 4], seed)


def tie_values(q):
    """(values, k): one-point intensities on the rounding boundaries (k + 1/2) d1 of the first quantizer, k over the code range.  d1 a power of
    two: the exact ties.  Otherwise fl((k + 1/2) d1) and its two fp32 neighbours."""
    k = np.arange(-int(q.z1), 256 - int(q.z1))
    centre = ((k.astype(np.float64) + 0.5) * float(q.d1)).astype(np.float32)
    if math.frexp(float(q.d1))[0] == 0.5:
        assert (centre.astype(np.float64) == (k + 0.5) * float(q.d1)).all()
        return centre, k
    lo, hi = np.nextafter(centre, np.float32(-np.inf)), np.nextafter(centre, np.float32(np.inf))
    return np.stack([lo, centre, hi], axis=1).reshape(-1), np.repeat(k, 3)


def table_values(q):
    """y = (c - z1) d1 for every first code c = 0..255, then one value far above and one far below the range"""
    c = np.arange(256, dtype=np.float32)
    return np.concatenate([(c - q.z1) * q.d1, np.array([1000.0, -1000.0], np.float32)]).astype(np.float32)


def tap_rotations(count):
    """feature j of pillar i holds values[(i + rot[j]) % count]; the intensity (j = 3) holds values[i]"""
    return [((j + 1) % 4) * (count // 4) for j in range(4)]


def _tap(name, aim, q, values):
    count = len(values)
    ny = max(2, int(math.sqrt(count / 2)))
    nx = -(-count // (2 * ny)) + 1
    grid = (2, ny, nx)
    vf = np.stack([values[(np.arange(count) + r) % count] for r in tap_rotations(count)], axis=1).reshape(count, 1, 4)
    w, b = tap_weights()
    return Prepared(name, aim, "tap", q, 1, grid, _plain_coords(count, grid), np.ones(count, np.int32), vf, w, b, values=values)


def tap_operand(prep):
    """[M][64]: what channel c of pillar i holds in front of the first quantizer"""
    return prep.vf[:, 0, np.arange(64) % 4]


def _multi(name, q, P, rounds, cus, seed):
    m = multi_round_m(rounds, cus)
    n_out = 40
    out_at = np.arange(n_out) * (m // n_out) + 7                                      # a few dozen out-of-canvas rows mixed in; the last row is live
    is_out = np.zeros(m, bool)
    is_out[out_at] = True
    live = m - n_out
    ny = int(math.sqrt(live / 2))
    nx = -(-live // (2 * ny)) + 1
    grid = (2, ny, nx)
    vox = np.array([4.0 / nx, 3.0 / ny, 4.0], np.float32)                            # the map spans 4 m x 3 m: the Linear's outputs stay inside the first quantizer's range
    off = (vox / 2 + np.array([-2.0, -1.5, -3.0], np.float32)).astype(np.float32)
    coords = np.zeros((m, 4), np.int32)
    bb, y, col = spread(live, *grid)
    z = np.arange(live) % 3 - 1                                                       # z = -1, 0, 1 where x = column - z stays on the map
    z[(col - z < 0) | (col - z >= nx)] = 0
    coords[~is_out] = np.stack([bb, z, y, col - z], axis=1)
    outs = outside_rows(*grid)
    coords[is_out] = [outs[i % 8] for i in range(n_out)]
    npts = (1 + (np.arange(m) * 7) % (P + 2)).astype(np.int32)                        # 1 .. P + 2: masked, full and np > P
    return _random_case(name, f"{rounds} rounds per workgroup at {cus} CUs: M = {m}, P = {P}, a ragged last workgroup", q, P, grid, coords, npts, seed,
                        vox, off, rounds=rounds, cus=cus)


CASES = {}
for _i, _P in enumerate((1, 2, 3, 5, 32)):
    for _j, _q in enumerate((QA, QB)):
        CASES[f"slots_p{_P}_{_q.name}"] = (lambda name, cus, P=_P, q=_q, s=10 + 2 * _i + _j: _slots(name, q, P, s))
for _i, _m in enumerate((1, 15, 16, 17, 33, 63, 64, 65)):
    CASES[f"m{_m}"] = (lambda name, cus, m=_m, q=(QA, QB)[_i % 2], s=30 + _i: _pillars(name, q, m, s))
for _q in (QA, QB):
    CASES[f"placement_{_q.name}"] = (lambda name, cus, q=_q, s=50 + int(_q.z2): _placement(name, q, s))
    CASES[f"ties_{_q.name}"] = (lambda name, cus, q=_q: _tap(name, "one-point pillars on the first quantizer's rounding boundaries", q, tie_values(q)[0]))
    CASES[f"table_{_q.name}"] = (lambda name, cus, q=_q: _tap(name, "every first code 0..255 and both saturations through the second quantizer's table",
                                                              q, table_values(q)))
CASES["rounds2"] = lambda name, cus: _multi(name, QB, 2, 2, cus, 61)
CASES["rounds8"] = lambda name, cus: _multi(name, QA, 1, 8, cus, 62)

MULTI_ROUND = ("rounds2", "rounds8")
UNSCATTER_ALONE = ("placement_qa", "m63", "m64", "m65")
REPEATED = "m33"
_PREP = {}


def build(name, cus=256):
    """the case ``name``, built once; ``cus`` sizes the multi-round cases"""
    key = (name, cus if name in MULTI_ROUND else 0)
    if key not in _PREP:
        _PREP[key] = CASES[name](name, cus)
    return _PREP[key]


# ---- launch and check (GPU) -------------------------------------------------------------------------------------------------------------------

def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def pfn_params(prep):
    from quantv2x_amd import lib as L
    p = L.PfnParams()
    p.w[:] = prep.w.reshape(-1).tolist()
    p.b[:] = prep.b.tolist()
    p.d1, p.z1, p.d2, p.z2 = float(prep.q.d1), float(prep.q.z1), float(prep.q.d2), float(prep.q.z2)
    p.vox[:] = prep.vox.tolist()
    p.off[:] = prep.off.tolist()
    return p


class DeviceCanvas:
    """a canvas on the GPU between two guard planes of one agent's size, full of GUARD"""

    def __init__(self, host):
        import torch
        self.shape = host.shape
        n = host.shape[0]
        dev = torch.device("cuda", 0)
        self.buf = torch.full((n + 2,) + tuple(host.shape[1:]), int(GUARD), dtype=torch.int8, device=dev)
        self.canvas = self.buf[1:n + 1]
        self.canvas.copy_(torch.from_numpy(host))
        assert self.canvas.is_contiguous() and self.canvas.data_ptr() % 16 == 0

    def read(self, what):
        """the canvas as numpy, after checking that both guard planes still hold GUARD"""
        import torch
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        assert (got[0] == GUARD).all(), f"{what}: written in front of the canvas (agent -1)"
        assert (got[-1] == GUARD).all(), f"{what}: written behind the canvas (agent N)"
        return got[1:-1]


def coords_to_device(prep):
    import torch
    return torch.from_numpy(prep.coords).to(torch.device("cuda", 0))


def scatter_launch(prep, dc, co=None):
    import torch
    from quantv2x_amd import lib as L
    dev = torch.device("cuda", 0)
    vf, npt = torch.from_numpy(prep.vf).to(dev), torch.from_numpy(prep.npts).to(dev)
    co = coords_to_device(prep) if co is None else co
    p = pfn_params(prep)
    L.check(L.load().qv2x_pfn_scatter_i8(L.ptr(vf), L.ptr(co), L.ptr(npt), prep.M, prep.P, C.byref(p), L.ptr(dc.canvas), prep.N, prep.ny, prep.nx,
                                         L.current_stream()), "qv2x_pfn_scatter_i8")
    torch.cuda.synchronize()


def unscatter_launch(prep, dc, value, co=None):
    import torch
    from quantv2x_amd import lib as L
    co = coords_to_device(prep) if co is None else co
    L.check(L.load().qv2x_pfn_unscatter_i8(L.ptr(co), prep.M, int(value), L.ptr(dc.canvas), prep.N, prep.ny, prep.nx, L.current_stream()),
            "qv2x_pfn_unscatter_i8")
    torch.cuda.synchronize()


def same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.int8, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    bad = got != want
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        cells = int(bad.any(axis=-1).sum())
        raise AssertionError(f"{what}: {int(bad.sum())} bytes in {cells} cells differ; first at (agent, row, column, channel) = {at} of the padded "
                             f"canvas: {int(got[at])} against {int(want[at])}")
