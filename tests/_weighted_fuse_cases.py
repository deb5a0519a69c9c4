"""Geometry, score and shape cases for the three entries of csrc/pyramid_fuse.hip, their operands, references, launches and checks (no tests).

Used by tests/test_weighted_fuse_cases_cpu.py (no GPU) and tests/test_hip_weighted_fuse_cases.py (GPU).

**Reference.**  ``oracle.geometry.weighted_fuse(.., ego=)``, pinned against the reference project's own vectors by tests/test_pyramid_fuse.py;
tolerance ``FUSE_TOL``.  For the i8 entry the reference's input is ``float32(code - zx) * dx``, the value the kernel forms at the taps.

**Pairwise matrices.**  ``pairwise [L][L][4][4]`` float64; the kernel reads row ``ego``.  A case names row ``ego`` (one planar motion per agent:
rotation, translation in CELLS of the ego map); every other row of the first ``agents`` rows holds drawn motions of its own, so reading the
wrong row changes the result, and entries past ``agents`` are the identity as ``get_pairwise_transformation`` pads them.  A translation by
(a, b) cells is ``T[0][3] = a ratio w_metres / w``, ``T[1][3] = b ratio h_metres / h``: output cell (y, x) samples input cell (y + b, x + a).

**Identity.**  The sampling position of cell i is ``((fl(fl((2 i + 1) / n - 1) + 1) n - 1) / 2`` in fp32, which equals i for every i only when n is
a power of two (n = 3, 5, 7 give -3e-8 at i = 0, so two taps with weights 1 - 3e-8 and 3e-8: torch's own behaviour).  The bit-equal identity
cases therefore run on 1 x 1, 16 x 1 and 4 x 8 maps; 3 x 7 and 5 x 16 carry the other geometries.

**Destinations** are allocated full of ``SENT``; the padded entry's ring must keep it, its input ring holds NaN (the i8 entry's ring: code 99).
"""
import ctypes as C

import numpy as np

SENT = np.float32(-777.25)
DX = np.float32(0.037)
CHANNELS = (64, 128, 192, 256, 320, 384, 448, 512, 576)     # every accepted count up to 576 (channels % 64 == 0)


# ---- the kernel's phase-2 mapping, restated ---------------------------------------------------------------------------------------------

def lanes_per_cell(c):
    """pyramid_weighted_fuse_kernel: 16 / 32 lanes per cell at 64 / 128 channels, a whole wave otherwise"""
    return 16 if c == 64 else 32 if c == 128 else 64


def phase2_stores(c):
    """every (cell index inside the workgroup, first channel of the float4) that the 256 threads of a workgroup store, in the kernel's
    loop order: wave, lane, step, 256-channel block"""
    lpc = lanes_per_cell(c)
    cps = 64 // lpc
    out = []
    for wave in range(4):
        for lane in range(64):
            sub = lane // lpc
            l4 = (lane - sub * lpc) * 4
            for step in range(4 // cps):
                ci = wave * 4 + step * cps + sub
                for cb in range(0, c, 256):
                    ch = cb + l4
                    if ch >= c:
                        break
                    out.append((ci, ch))
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

def motion(angle_deg=0.0, dx=0.0, dy=0.0):
    return (float(angle_deg), float(dx), float(dy))


I = motion()


class Fuse:
    """row: the ego's row of motions, one per agent.  score: "plain" (uniform in [0.05, 1]) | "zeros" (a third of every agent's cells exactly
    0, drawn independently) | "extremes" (agents 0 / 1 hold 1.0001 / 1e-4, swapped on odd cells) | "left_masked" (agent 0: columns < 6 are 0)"""

    def __init__(self, aim, h, w, c, row, max_cav, ego=0, hm=None, wm=None, ratio=1.0, score="plain", zx=128, seed=0,
                 partial=False, identity=False, out_of_view=None):
        self.aim, self.h, self.w, self.c, self.row, self.max_cav, self.ego = aim, h, w, c, row, max_cav, ego
        self.agents = len(row)
        self.hm, self.wm = (0.4 * h if hm is None else hm), (0.4 * w if wm is None else wm)
        self.ratio, self.score, self.zx, self.seed = ratio, score, zx, seed
        self.partial, self.identity, self.out_of_view = partial, identity, out_of_view
        assert 1 <= self.agents <= 8 and self.agents <= max_cav and 0 <= ego < self.agents


R = motion
CASES = {
    "identity_16x1": Fuse("identity, one agent, 16 x 1: out == in bit for bit", 16, 1, 64, [I], 5, zx=0, seed=1, identity=True),
    "identity_1x1_c128": Fuse("identity on a 1 x 1 map (one live cell of 16), 128 channels", 1, 1, 128, [I], 5, zx=255, seed=2, identity=True),
    "identity_4x8_c320": Fuse("identity, 320 channels: the second 256-chunk is partial", 4, 8, 320, [I], 8, zx=128, seed=3, identity=True),
    "shift_x3_partial": Fuse("agent 1 moved by (+3, 0) cells, agent 0 masked in columns >= 10: two / one / no visible agents", 5, 16, 64,
                             [I, R(0, 3, 0)], 5, score="right_masked", zx=0, seed=4, partial=True),
    "shift_y2_ego1": Fuse("ego = 1 = agents - 1 with max_cav 8 > agents: agent 0 moved by (0, -2) cells", 5, 16, 128, [R(0, 0, -2), I], 8, ego=1,
                          zx=255, seed=5),
    "shift_out_of_view": Fuse("agent 1 moved by (+w, 0): entirely out of view, the result is agent 0's own map", 3, 7, 64, [I, R(0, 7, 0)], 5,
                              seed=6, out_of_view=1),
    "half_cell_c256": Fuse("agent 1 moved by half a cell both ways: four equal taps; 21 cells = one group and a tail of 5; 256 channels", 3, 7, 256,
                           [I, R(0, 0.5, 0.5)], 5, zx=0, seed=7),
    "rot90_c320_partial": Fuse("90 and 180 degrees on a 5 x 16 map of 10 m x 32 m, discrete_ratio 2: the turned agent covers a 5 x 5 patch", 5, 16, 320,
                               [I, R(90, 0, 0), R(180, 2, 0)], 5, hm=10.0, wm=32.0, ratio=2.0, score="left_masked", zx=255, seed=8, partial=True),
    "rot180_c512": Fuse("180 degrees about the centre of a 3 x 7 map of 6 m x 21 m, discrete_ratio 0.5; 512 channels", 3, 7, 512, [I, R(180, 0, 0)], 5,
                        hm=6.0, wm=21.0, ratio=0.5, seed=9),
    "five_agents_ego1_c192": Fuse("5 agents of max_cav 8, ego = 1, 192 channels (lanes 48..63 idle), 21 cells", 3, 7, 192,
                                  [R(10, 1, 0), I, R(-15, -2, 1), R(0, 2.5, -1), R(5, 0, 0.5)], 8, ego=1, zx=0, seed=10),
    "eight_agents_ego7": Fuse("MAXA = 8 agents, ego = 7 = agents - 1, 16 x 1", 16, 1, 64,
                              [R(0, 0, 1), R(0, 0, -1), R(0, 0, 2.5), R(0, 0, -4), R(180, 0, 0), R(0, 0, 7), R(0, 0, -0.5), I], 8, ego=7, zx=255, seed=11),
    "two_agents_c192_16x1": Fuse("192 channels on exactly one group of 16 cells: wave 3's last cell is cell 15", 16, 1, 192, [I, R(0, 0, 3)], 5, seed=12),
    "score_zeros_partial": Fuse("identity for both agents, a third of each score map exactly 0: masked although visible; cells masked for both return 0",
                                5, 16, 128, [I, I], 5, score="zeros", seed=13, partial=True),
    "score_extremes": Fuse("scores 1.0001 against 1e-4", 3, 7, 64, [I, I], 8, score="extremes", zx=0, seed=14),
}


# ---- operands and references (CPU only) ----------------------------------------------------------------------------------------------------

def motion_matrix(case, m):
    ang, dx, dy = m
    q = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), -90.0: (0.0, -1.0)}.get(ang)
    cs, sn = q if q is not None else (np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang)))
    t = np.eye(4)
    t[0, 0], t[0, 1], t[1, 0], t[1, 1] = cs, -sn, sn, cs
    t[0, 3] = dx * case.ratio * case.wm / case.w
    t[1, 3] = dy * case.ratio * case.hm / case.h
    return t


class Prepared:
    def __init__(self, case):
        from oracle import geometry
        self.case = c = case
        rng = np.random.default_rng(9000 + c.seed)
        n, L = c.agents, c.max_cav
        self.pairwise = np.tile(np.eye(4), (L, L, 1, 1))
        for r in range(n):
            for a in range(n):
                m = c.row[a] if r == c.ego else motion(rng.uniform(-40, 40), rng.uniform(-0.3, 0.3) * c.w, rng.uniform(-0.3, 0.3) * c.h)
                self.pairwise[r, a] = motion_matrix(c, m)
        self.affine = geometry.normalize_pairwise_tfm(self.pairwise, c.hm, c.wm, c.ratio)
        self.x = rng.standard_normal((n, c.h, c.w, c.c)).astype(np.float32)
        self.bytes = rng.integers(-128, 128, size=(n, c.h, c.w, c.c)).astype(np.int8)                  # stored bytes: code - 128
        self.bytes[0, 0, 0, 0], self.bytes[-1, -1, -1, -1] = -128, 127
        self.bytes[0, 0, 0, 1 % c.c], self.bytes[-1, -1, -1, -2] = 127, -128
        self.xdq = ((self.bytes.astype(np.int32) + 128 - c.zx).astype(np.float32) * DX).astype(np.float32)
        s = rng.uniform(0.05, 1.0, (n, c.h, c.w, 1)).astype(np.float32)
        if c.score == "zeros":
            s[rng.uniform(size=s.shape) < 1.0 / 3.0] = 0.0
        elif c.score == "extremes":
            odd = (np.arange(c.h * c.w).reshape(c.h, c.w) % 2 == 1)[..., None]
            s[0], s[1] = np.where(odd, np.float32(1e-4), np.float32(1.0001)), np.where(odd, np.float32(1.0001), np.float32(1e-4))
        elif c.score == "left_masked":
            s[0, :, :6] = 0.0
        elif c.score == "right_masked":
            s[0, :, 10:] = 0.0
        else:
            assert c.score == "plain"
        self.s = s
        self.want = self.oracle(self.x)
        self.want_i8 = self.oracle(self.xdq)

    def oracle(self, x, ego=None, affine=None, n=None):
        from oracle import geometry
        n = self.case.agents if n is None else n
        return geometry.weighted_fuse(x[:n], self.s[:n], self.affine if affine is None else affine, n, ego=self.case.ego if ego is None else ego)

    def visible(self):
        """per cell, the number of agents whose warped score is not 0"""
        from oracle import geometry
        c = self.case
        grid = geometry.affine_grid(self.affine[c.ego, :c.agents], c.h, c.w).astype(np.float32)
        return (geometry.grid_sample_bilinear_zeros(self.s, grid)[..., 0] != 0).sum(axis=0)

    def affine_with_stride_agents(self):
        """the matrices a kernel would read that indexed the pairwise tensor [ego * agents + agent] instead of [ego * max_cav + agent]"""
        from oracle import geometry
        c = self.case
        flat = self.pairwise.reshape(-1, 4, 4)
        wrong = np.tile(np.eye(4), (c.max_cav, c.max_cav, 1, 1))
        wrong[c.ego, :c.agents] = flat[c.ego * c.agents:c.ego * c.agents + c.agents]
        return geometry.normalize_pairwise_tfm(wrong, c.hm, c.wm, c.ratio)


def pad_f32(x, fill):
    n, h, w, c = x.shape
    p = np.full((n, h + 2, w + 2, c), fill, np.float32)
    p[:, 1:-1, 1:-1] = x
    return p


def pad_i8(b, fill=99 - 128):
    n, h, w, c = b.shape
    p = np.full((n, h + 2, w + 2, c), fill, np.int8)
    p[:, 1:-1, 1:-1] = b
    return p


# ---- launches (GPU) ------------------------------------------------------------------------------------------------------------------------

def launch(prep, entry):
    """entry: "f32" | "f32p" | "i8"; returns the whole destination (for "f32p" the padded map [h+2][w+2][c]), allocated full of SENT"""
    import torch
    from quantv2x_amd import lib as L
    c = prep.case
    lib, dev = L.load(), torch.device("cuda", 0)
    d = L.FuseDesc()
    d.agents, d.h, d.w, d.levels, d.kc, d.max_cav, d.ego = c.agents, c.h, c.w, 1, 1, c.max_cav, c.ego
    d.h_metres, d.w_metres, d.discrete_ratio = c.hm, c.wm, c.ratio
    st = torch.from_numpy(np.ascontiguousarray(prep.s[..., 0])).to(dev)
    pw = torch.from_numpy(np.ascontiguousarray(prep.pairwise)).to(dev)
    shape = (c.h + 2, c.w + 2, c.c) if entry == "f32p" else (c.h, c.w, c.c)
    out = torch.full(shape, float(SENT), dtype=torch.float32, device=dev)
    if entry == "i8":
        ft = torch.from_numpy(pad_i8(prep.bytes)).to(dev)
        rc = lib.qv2x_pyramid_weighted_fuse_i8(C.byref(d), c.c, L.ptr(ft), c.zx, float(DX), L.ptr(st), L.ptr(pw), L.ptr(out), L.current_stream())
    elif entry == "f32p":
        ft = torch.from_numpy(pad_f32(prep.x, np.nan)).to(dev)
        rc = lib.qv2x_pyramid_weighted_fuse_f32p(C.byref(d), c.c, L.ptr(ft), L.ptr(st), L.ptr(pw), L.ptr(out), L.current_stream())
    else:
        assert entry == "f32"
        ft = torch.from_numpy(prep.x).to(dev)
        rc = lib.qv2x_pyramid_weighted_fuse_f32(C.byref(d), c.c, L.ptr(ft), L.ptr(st), L.ptr(pw), L.ptr(out), L.current_stream())
    L.check(rc, "qv2x_pyramid_weighted_fuse_" + entry)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits; first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]!r} against {want[bad][0]!r}")


def check(prep, got, want, what):
    """nothing left at the sentinel, no NaN, fully masked cells exactly 0, everything within FUSE_TOL of the oracle"""
    from _common import FUSE_TOL
    assert not np.isnan(got).any(), f"{what}: NaN (a tap outside the map was read)"
    assert not (got == SENT).any(), f"{what}: cells left untouched"
    dead = prep.visible() == 0
    assert (got[dead] == 0).all(), f"{what}: cells with every agent masked must be exactly 0"
    np.testing.assert_allclose(got, want, err_msg=what, **FUSE_TOL)
