"""The post stage's kernels (a7-a11: csrc/fuse_att.h, fuse_att.hip, heads_f32.hip) one entry at a time through the C ABI, on small synthetic
operands (tests/_post_layers.py) at the shapes the deployed tiny / small models never give them: 5-7 agents, 1-16 code planes with 1..256
entries, maps whose cell count is no multiple of 4, 32 or 64, every channel count around the 16- and 32-column tile boundaries, padded
channel counts, ragged batches, every ego, gapped code planes, bands, zero points 0 and 255, clamps and exact rounding ties.

Rules: decode, dequantization and band assembly are compared bit for bit.  ``dyadic`` head cases (order-free sums) are bit for bit against
the float64 reference on both wires; ``real`` head cases stay within the forward error bound E of an fp32 dot product on channels without a
quantizer and give the float64 code outside the doubtful set (at most one code off inside it).  Fused rows are within ``FUSE_TOL`` of the
numpy restatement and every form of a case (single scene, batch, band, the one-launch kernel's tap) agrees with the others bit for bit.
Every output is allocated full of NaN (0xA5 for bytes) with 64 guard elements on either side that must survive; code planes carry poisoned
gaps and the device tables a NaN tail, so a byte read from a gap shows as NaN instead of leaving the allocation.
(The four-cell table form stays with tests/test_hip_fuse_heads.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _post_layers as P
from _common import FUSE_TOL

pytestmark = pytest.mark.gpu

GUARD = 64


def _L():
    from quantv2x_amd import lib as L
    return L


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """an output of ``shape`` inside a sentinel-filled allocation; ``.t`` is the view the kernel writes, ``.np()`` its value after the guard check"""

    def __init__(self, shape, u8=False):
        self.n, self.u8 = int(np.prod(shape)), u8
        self.buf = (torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if u8 else
                    torch.full((self.n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda"))
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        """the output's address (a zero-size torch view has none of its own)"""
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def guards(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return bool((g == 0xA5).all()) if self.u8 else bool(torch.isnan(g).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all()) if self.u8 else bool(torch.isnan(self.buf).all())

    def np(self):
        torch.cuda.synchronize()
        assert self.guards(), "written outside the output"
        return self.t.cpu().numpy()


def lut_dev(lut):
    """[planes][kc][width] -> device rows with a NaN tail (a poisoned code byte reads NaN, never past the allocation)"""
    flat = lut.reshape(-1, lut.shape[-1])
    return dev(np.concatenate([flat, np.full((P.NAN_ROWS, lut.shape[-1]), np.nan, np.float32)]))


def heads_dev(hd):
    return dict(cout=hd["cout"], cout_pad=hd["cout_pad"], w=dev(hd["w_packed"]), bias=dev(hd["bias_pad"]), da=dev(hd["da_pad"]), za=dev(hd["za_pad"]),
                da_host=np.ascontiguousarray(hd["da"]))


def rows_dev(rows):
    """fp32 rows behind and in front of NaN (the ABI takes dense [R][256] rows)"""
    buf = torch.full((rows.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + rows.size] = dev(rows).reshape(-1)
    return buf, buf[GUARD:GUARD + rows.size]


def nchw(y, n, hw):
    """[n * hw][cout] -> [n][cout][hw]"""
    return np.ascontiguousarray(y.reshape(n, hw, -1).transpose(0, 2, 1))


# ---- the heads' launches ---------------------------------------------------------------------------------------------------------------------
def run_heads(x, n, hw, H, entry="heads_f32", wire="f32"):
    L = _L()
    out = Out((n, H["cout"], hw), u8=wire == "u8")
    hargs = (H["cout"], H["cout_pad"], L.ptr(H["w"]), L.ptr(H["bias"]), L.ptr(H["da"]), L.ptr(H["za"]))
    if entry == "heads_f32":
        L.check(L.load().qv2x_heads_f32(L.ptr(x), n * hw, hw, *hargs, L.ptr(out.t), L.current_stream()), entry)
    else:
        L.check(L.load().qv2x_heads_band(L.ptr(x), n, hw, *hargs, L.WIRES[wire], L.ptr(H["da_host"]), L.ptr(out.t), L.current_stream()), entry)
    return out.np()


def run_decode_heads(codes, n, hw, planes, kc, lut, bias, H):
    L = _L()
    out = Out((n, H["cout"], hw))
    L.check(L.load().qv2x_decode_heads_f32(L.ptr(codes), n * hw, hw, planes, kc, L.ptr(lut), L.ptr(bias), H["cout"], H["cout_pad"], L.ptr(H["w"]),
                                           L.ptr(H["bias"]), L.ptr(H["da"]), L.ptr(H["za"]), L.ptr(out.t), L.current_stream()), "decode heads")
    return out.np()


def check_dyadic(got, y64, hd, n, hw, wire):
    y = y64.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), y64)
    want = P.ref_quant(y, hd["da"], hd["za"], codes=wire == "u8")
    np.testing.assert_array_equal(got.astype(np.float32), nchw(want, n, hw))


def check_real(got, y64, E, hd, n, hw, wire):
    """channels without a quantizer within E; the float64 code outside the doubtful set, at most one off inside; f32 wire = (code - z) * d"""
    da, za = hd["da"], hd["za"]
    g = got.astype(np.float64).transpose(0, 2, 1).reshape(n * hw, -1)
    on = da > 0
    err = np.abs(g - y64)[:, ~on]
    print(f"unquantized channels: max |got - y64| / E = {float((err / E[:, ~on]).max()) if err.size else 0:.3f}")
    assert (err <= E[:, ~on]).all()
    d = np.where(on, da, np.float32(1))
    if wire == "u8":
        code = g
    else:
        code = np.rint(g / d.astype(np.float64) + za)
        back = ((code.astype(np.float32) - za) * d).astype(np.float32)
        assert np.array_equal(back[:, on], got.transpose(0, 2, 1).reshape(n * hw, -1)[:, on]), "an output is not (code - z) * d"
    want, _ = P.code64(y64, da, za)
    dbt = P.doubtful(y64, E, da)
    diff = np.abs(code - want)[:, on]
    print(f"doubtful {dbt[:, on].mean():.4f}, codes off {int((diff != 0).sum())}")
    assert diff.max() <= 1 and (diff[~dbt[:, on]] == 0).all()


@pytest.mark.parametrize("name", list(P.HEAD_CASES))
def test_heads(name):
    """qv2x_heads_f32, qv2x_heads_band on both wires and qv2x_decode_heads_f32 on one head case"""
    c = P.head_case(name)
    n, hw = c["n"], c["hw"]
    H, Hq = heads_dev(c["heads"]), heads_dev(c["heads_q"])
    keep, x = rows_dev(c["rows"])
    check = (lambda got, key, hd, wire: check_dyadic(got, c[key], hd, n, hw, wire)) if c["mode"] == "dyadic" else \
            (lambda got, key, hd, wire: check_real(got, c[key], c["E" + key[3:]], hd, n, hw, wire))
    check(run_heads(x, n, hw, H), "y64", c["heads"], "f32")
    check(run_heads(x, n, hw, H, "heads_band", "f32"), "y64", c["heads"], "f32")
    check(run_heads(x, n, hw, Hq, "heads_band", "u8"), "y64", c["heads_q"], "u8")
    check(run_heads(x, n, hw, Hq), "y64", c["heads_q"], "f32")
    lut, lb, codes = lut_dev(c["lut"]), dev(c["lut_bias"]), dev(c["codes"])
    check(run_decode_heads(codes, n, hw, c["planes"], c["kc"], lut, lb, H), "y64d", c["heads"], "f32")
    assert bool(torch.isnan(keep[:GUARD]).all())


@pytest.mark.parametrize("name", list(P.PAIR_CASES))
def test_heads_pair(name):
    """qv2x_heads_pair_f32 with R != R1 and more than eight tiles: the job with fewer tiles leaves the other's blocks alone; also a last
    column tile of at most 16 channels and ``cout_pad`` above ``ceil32(cout)`` in either job"""
    L = _L()
    c = P.pair_case(name)
    hw, n0, n1, planes, kc, h0, h1 = c["hw"], c["n0"], c["n1"], c["planes"], c["kc"], c["h0"], c["h1"]
    H0, H1 = heads_dev(h0), heads_dev(h1)
    keep, x = rows_dev(c["rows"])
    o0, o1 = Out((n0, h0["cout"], hw)), Out((n1, h1["cout"], hw))
    a = lambda H: (H["cout"], H["cout_pad"], L.ptr(H["w"]), L.ptr(H["bias"]), L.ptr(H["da"]), L.ptr(H["za"]))
    ld, lbd, cd = lut_dev(c["lut"]), dev(c["lut_bias"]), dev(c["codes"])
    L.check(L.load().qv2x_heads_pair_f32(L.ptr(x), n0 * hw, hw, *a(H0), L.ptr(o0.t), L.ptr(cd), n1 * hw, planes, kc, L.ptr(ld), L.ptr(lbd),
                                         *a(H1), L.ptr(o1.t), L.current_stream()), "heads pair")
    check_dyadic(o0.np(), P.ref_heads64(c["rows"], h0["w"], h0["bias"]), h0, n0, hw, "f32")
    check_dyadic(o1.np(), P.ref_heads64(c["drows"], h1["w"], h1["bias"]), h1, n1, hw, "f32")


# ---- fusion ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuse_dev(name):
    c = P.fuse_case(name)
    d = dict(pairwise=dev(c["pairwise"]))
    if c["feats"]:
        d.update(feats=dev(c["feats_buf"]), codes=None, lut=None, lut_bias=None)
    else:
        d.update(feats=None, codes=dev(c["codes_buf"]), lut=lut_dev(c["lut"]), lut_bias=dev(c["lut_bias"]))
    return d


def fuse_desc(c, agents):
    d = _L().FuseDesc()
    d.agents, d.h, d.w, d.levels, d.kc, d.max_cav, d.ego = agents, c["h"], c["w"], c["planes"], c["kc"], c["max_cav"], c["ego"]
    d.code_agent_stride, d.code_level_stride = c["agent_stride"], c["level_stride"]
    d.h_metres, d.w_metres, d.discrete_ratio, d.fusion = c["hm"], c["wm"], c["ratio"], c["fusion"]
    return d


def _scene_args(c, scenes):
    offs = (C.c_int64 * len(scenes))(*[int(c["offsets"][s]) for s in scenes])
    cnt = (C.c_int32 * len(scenes))(*[int(c["scenes"][s]) for s in scenes])
    return offs, cnt


def fuse_one(name, s):
    """qv2x_fuse_att_f32 on scene ``s`` alone"""
    L, c, D = _L(), P.fuse_case(name), fuse_dev(name)
    d = fuse_desc(c, c["scenes"][s])
    out = Out((c["hw"], 256))
    off = int(c["offsets"][s])
    codes, feats = (None, D["feats"][off:]) if c["feats"] else (D["codes"][off:], None)
    L.check(L.load().qv2x_fuse_att_f32(C.byref(d), L.ptr(codes), L.ptr(D["lut"]), L.ptr(D["lut_bias"]), L.ptr(feats), L.ptr(D["pairwise"][s]),
                                       L.ptr(out.t), L.current_stream()), "fuse")
    return out.np()


def fuse_batch(name, scenes=None, band=None):
    """qv2x_fuse_att_batch_f32, or qv2x_fuse_att_band_f32 over ``band`` = (cell0, n_cells); ``scenes``: consecutive scene numbers"""
    L, c, D = _L(), P.fuse_case(name), fuse_dev(name)
    scenes = list(range(len(c["scenes"]))) if scenes is None else scenes
    offs, cnt = _scene_args(c, scenes)
    d = fuse_desc(c, 1)
    cells = c["hw"] if band is None else band[1]
    out = Out((len(scenes), cells, 256))
    args = (C.byref(d), len(scenes), offs, cnt, L.ptr(D["codes"]), L.ptr(D["lut"]), L.ptr(D["lut_bias"]), L.ptr(D["feats"]), L.ptr(D["pairwise"][scenes[0]:]))
    if band is None:
        L.check(L.load().qv2x_fuse_att_batch_f32(*args, out.ptr(), L.current_stream()), "fuse batch")
    else:
        L.check(L.load().qv2x_fuse_att_band_f32(*args, band[0], band[1], out.ptr(), L.current_stream()), "fuse band")
    if cells == 0:
        torch.cuda.synchronize()
        assert out.untouched()
    return out.np()


def fuse_heads(name, H, band=None, wire="f32", entry="batch", tap=True):
    """the one-launch entries: (predictions [scenes][cout][cells], tapped fused rows [scenes][cells][256])"""
    L, c, D = _L(), P.fuse_case(name), fuse_dev(name)
    scenes = list(range(len(c["scenes"])))
    offs, cnt = _scene_args(c, scenes)
    d = fuse_desc(c, 1)
    cells = c["hw"] if band is None else band[1]
    out, tp = Out((len(scenes), H["cout"], cells), u8=wire == "u8"), Out((len(scenes), cells, 256))
    head = (H["cout"], H["cout_pad"], L.ptr(H["w"]), L.ptr(H["bias"]), L.ptr(H["da"]), L.ptr(H["za"]))
    args = (C.byref(d), len(scenes), offs, cnt, L.ptr(D["codes"]), L.ptr(D["lut"]), L.ptr(D["lut_bias"]), L.ptr(D["feats"]), L.ptr(D["pairwise"]))
    if entry == "batch":
        L.check(L.load().qv2x_fuse_heads_batch_f32(*args, *head, L.ptr(out.t), L.ptr(tp.t) if tap else None, L.current_stream()), "fuse heads")
    else:
        b = (0, c["hw"]) if band is None else band
        L.check(L.load().qv2x_fuse_heads_band(*args, b[0], b[1], *head, L.WIRES[wire], L.ptr(H["da_host"]), L.ptr(out.t), L.ptr(tp.t) if tap else None,
                                              L.current_stream()), "fuse heads band")
    return out.np(), (tp.np() if tap else None)


@functools.lru_cache(maxsize=None)
def small_head(cout=72, every_quantized=False, mode="real", cout_pad=None):
    rng = np.random.default_rng(cout + 5)
    return P.make_heads(rng, cout, cout_pad or P.ceil32(cout), mode, every_quantized=every_quantized)


@pytest.mark.parametrize("name", list(P.FUSE_CASES))
def test_fuse_forms(name):
    """every form of one fuse case: each scene alone (qv2x_fuse_att_f32), the batch, the whole-map band and the one-launch kernel's tap"""
    c = P.fuse_case(name)
    batch = fuse_batch(name)
    for s in range(len(c["scenes"])):
        got = fuse_one(name, s)
        err = np.abs(got - c["ref"][s]) - FUSE_TOL["rtol"] * np.abs(c["ref"][s])
        print(f"scene {s}: {c['scenes'][s]} agents, max excess over rtol {float(err.max()):.3g} of atol {FUSE_TOL['atol']}")
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, c["ref"][s], **FUSE_TOL)
        assert np.array_equal(batch[s], got), f"scene {s} of the batch differs from the scene alone"
        if len(c["scenes"]) > 1:
            assert np.array_equal(fuse_batch(name, [s])[0], got)
    assert np.array_equal(fuse_batch(name, band=(0, c["hw"])), batch)
    _, tap = fuse_heads(name, heads_dev(small_head(20)))
    assert np.array_equal(tap, batch)
    if c["special"] == "saturated":
        warped = P._warp(c["dec"][0], c["pairwise"][0], 3, 0, P.HM, P.WM, P.RATIO)
        np.testing.assert_allclose(batch[0], warped[1].reshape(-1, 256), **FUSE_TOL)
    if c["special"] == "negative":
        assert (batch == 0).all()


@pytest.mark.parametrize("band", P.BAND_RANGES)
@pytest.mark.parametrize("name", ["map_7x33", "ego2_of6_7x33"])
def test_fuse_band_ranges(name, band):
    c = P.fuse_case(name)
    whole = fuse_batch(name)
    got = fuse_batch(name, band=band)
    assert got.shape == (1, band[1], 256) and np.array_equal(got, whole[:, band[0]:band[0] + band[1]])
    np.testing.assert_allclose(got[0], c["ref"][0][band[0]:band[0] + band[1]], **FUSE_TOL)


@pytest.mark.parametrize("wire", ["f32", "u8"])
@pytest.mark.parametrize("cout,cout_pad", [(72, 96), (16, 32), (20, 64)])
@pytest.mark.parametrize("name", P.ONE_LAUNCH_CASES)
def test_one_launch_equals_two_launches(name, cout, cout_pad, wire):
    """qv2x_fuse_heads_batch_f32 / qv2x_fuse_heads_band against qv2x_fuse_att_band_f32 followed by qv2x_heads_band: a 72-channel head, a
    single 16-column tile and a head padded past ``ceil32(cout)``"""
    c = P.fuse_case(name)
    band = (7, 45) if name == "map_7x33" else (0, c["hw"])
    H = heads_dev(small_head(cout, every_quantized=wire == "u8", cout_pad=cout_pad))
    fused = fuse_batch(name, band=band)
    keep, x = rows_dev(fused.reshape(-1, 256))
    want = run_heads(x, len(c["scenes"]), band[1], H, "heads_band", wire)
    got, tap = fuse_heads(name, H, band=band, wire=wire, entry="band")
    assert np.array_equal(tap, fused) and np.array_equal(got, want)
    got, _ = fuse_heads(name, H, band=band, wire=wire, entry="band", tap=False)
    assert np.array_equal(got, want)
    if wire == "f32" and band == (0, c["hw"]):
        got, tap = fuse_heads(name, H)
        assert np.array_equal(tap, fused) and np.array_equal(got, want)
        assert np.array_equal(run_heads(x, len(c["scenes"]), band[1], H), want)


@pytest.mark.parametrize("wire", ["f32", "u8"])
@pytest.mark.parametrize("name", list(P.IDENTITY_CASES))
def test_one_launch_dyadic_identity(name, wire):
    """one agent per scene and T = I on maps whose cell centres are exact in fp32 (the numpy warp returns the decoded map itself:
    tests/test_post_layers_cpu.py): the one-launch entry equals the float64 head of the decoded rows bit for bit, at 72 channels, around
    the 16- and 32-column boundaries and with ``cout_pad`` above ``ceil32(cout)``"""
    L = _L()
    c = P.identity_case(name, wire == "u8")
    hw, scenes, hd = c["hw"], c["scenes"], c["heads"]
    H = heads_dev(hd)
    d = L.FuseDesc()
    d.agents, d.h, d.w, d.levels, d.kc, d.max_cav, d.ego = 1, c["h"], c["w"], c["planes"], c["kc"], 2, 0
    d.code_agent_stride, d.code_level_stride = c["agent_stride"], c["level_stride"]
    d.h_metres, d.w_metres, d.discrete_ratio, d.fusion = P.HM, P.WM, P.RATIO, 0
    offs = (C.c_int64 * scenes)(*[s * c["agent_stride"] for s in range(scenes)])
    cnt = (C.c_int32 * scenes)(*[1] * scenes)
    out, tap = Out((scenes, hd["cout"], hw), u8=wire == "u8"), Out((scenes, hw, 256))
    cd, ld, lbd, pwd = dev(c["codes_buf"]), lut_dev(c["lut"]), dev(c["lut_bias"]), dev(c["pairwise"])
    L.check(L.load().qv2x_fuse_heads_band(C.byref(d), scenes, offs, cnt, L.ptr(cd), L.ptr(ld), L.ptr(lbd), None, L.ptr(pwd), 0, hw, hd["cout"],
                                          hd["cout_pad"], L.ptr(H["w"]), L.ptr(H["bias"]), L.ptr(H["da"]), L.ptr(H["za"]), L.WIRES[wire],
                                          L.ptr(H["da_host"]), L.ptr(out.t), L.ptr(tap.t), L.current_stream()), "fuse heads band")
    np.testing.assert_array_equal(tap.np().reshape(-1, 256), c["drows"])
    check_dyadic(out.np(), P.ref_heads64(c["drows"], hd["w"], hd["bias"]), hd, scenes, hw, wire)


# ---- the table forms -----------------------------------------------------------------------------------------------------------------------
def check_table(got, t, n, hw, lo, hi):
    """channels [lo, hi) of a table case: got [n][hi - lo][hw]"""
    y64 = P.table_sum64(t["codes"], t["t64"], t["b64"])[:, lo:hi]
    da, za = t["da"][lo:hi], t["za"][lo:hi]
    hd = dict(da=da, za=za)
    if t["mode"] == "dyadic":
        check_dyadic(got, y64, hd, n, hw, "f32")
    else:
        check_real(got, y64, P.table_error_bound(t["codes"], t["t64"], t["b64"])[:, lo:hi], hd, n, hw, "f32")


# (the two-runs-per-workgroup case runs once, in the exact mode)
@pytest.mark.parametrize("name,mode", [(n, m) for n in P.LUT_CASES for m in ("dyadic", "real") if (n, m) != ("groups2", "real")])
def test_single_heads_lut(name, mode):
    L = _L()
    t = P.table_case(name, mode)
    n, hw = t["R"] // t["hw"], t["hw"]
    out = Out((n, t["ct"], hw))
    ops = [dev(t[k]) for k in ("codes", "tables", "bias", "da", "za")]
    L.check(L.load().qv2x_single_heads_lut_f32(L.ptr(ops[0]), t["R"], hw, t["planes"], t["kc"], t["ct"], *[L.ptr(o) for o in ops[1:]], L.ptr(out.t),
                                               L.current_stream()), "single heads lut")
    check_table(out.np(), t, n, hw, 0, t["ct"])


@pytest.mark.parametrize("mode", ["dyadic", "real"])
@pytest.mark.parametrize("name", list(P.TABLE_CASES))
def test_table_heads(name, mode):
    """qv2x_table_heads_f32: the one-cell LDS form at hw % 4 != 0 and the global-table form (more than four planes or tables past the LDS)"""
    L = _L()
    planes, kc, c0, c1, R, hw = P.TABLE_CASES[name]
    t = P.table_case(name, mode)
    n = R // hw
    # (a copy of qv2x_table_heads_f32's dispatch rule, heads_f32.hip: row stride ST with ST / 4 odd, more than four planes or more than
    #  160 KB of LDS -> the global-table form.  If that rule changes, change it here too: the case names promise a form.)
    ST = (c0 + c1 + 3) // 4 * 4
    ST = ST if (ST // 4) % 2 else ST + 4
    assert name.startswith("global") == (planes > 4 or (planes * kc * ST + 4 * ((c0 + c1 + 3) // 4 * 4)) * 4 > 160 * 1024)
    o0, o1 = (Out((n, c0, hw)) if c0 else None), (Out((n, c1, hw)) if c1 else None)
    ops = [dev(t[k]) for k in ("codes", "tables", "bias", "da", "za")]
    L.check(L.load().qv2x_table_heads_f32(L.ptr(ops[0]), R, hw, planes, kc, c0, c1, *[L.ptr(o) for o in ops[1:]], L.ptr(o0.t) if c0 else None,
                                          L.ptr(o1.t) if c1 else None, L.current_stream()), "table heads")
    if c0:
        check_table(o0.np(), t, n, hw, 0, c0)
    if c1:
        check_table(o1.np(), t, n, hw, c0, c0 + c1)


# ---- the small entries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,planes,kc", P.DECODE_CASES)
def test_decode_lut(R, planes, kc):
    L = _L()
    for mode in ("real", "dyadic"):
        c = P.decode_case(R, planes, kc, mode)
        out = Out((R, 256))
        cd, ld, lbd = dev(c["codes"]), lut_dev(c["lut"]), dev(c["lut_bias"])
        L.check(L.load().qv2x_decode_lut_f32(L.ptr(cd), R, planes, kc, L.ptr(ld), L.ptr(lbd), L.ptr(out.t), L.current_stream()), "decode")
        np.testing.assert_array_equal(out.np(), P.ref_decode(c["codes"], c["lut"], c["lut_bias"]))


@pytest.mark.parametrize("zp", [0, 128, 255])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 3, 5), (2, 7, 9)])
@pytest.mark.parametrize("c", [4, 64, 256])
def test_dequant_i8(c, n, h, w, zp):
    L = _L()
    rng = np.random.default_rng(c + h + zp)
    code = rng.integers(-128, 128, size=(n, h, w, c)).astype(np.int8)
    code.reshape(-1)[:2] = (-128, 127)
    padded = np.full((n, h + 2, w + 2, c), 0x55, np.int8)             # the border is poison: a value no interior element may pick up by position
    padded[:, 1:-1, 1:-1] = code
    delta = np.float32(0.0371)
    out = Out((n * h * w, c))
    pd = dev(padded)
    L.check(L.load().qv2x_dequant_i8_f32(L.ptr(pd), n, h, w, c, zp, C.c_float(float(delta)), L.ptr(out.t), L.current_stream()), "dequant")
    np.testing.assert_array_equal(out.np(), P.ref_dequant(code, zp, delta).reshape(n * h * w, c))


@pytest.mark.parametrize("wire", ["f32", "u8"])
@pytest.mark.parametrize("frames,cout", [(1, 3), (2, 20)])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("h,w", [(5, 7), (6, 9), (3, 33), (16, 32)])
def test_assemble_bands(h, w, world, frames, cout, wire):
    """odd widths: runs that start off a 16-byte boundary on either side (the element-wise head, tail and whole-run fallback); world > h: empty bands"""
    from quantv2x_amd.dist import band_payload_layout, band_rows
    L = _L()
    rng = np.random.default_rng(h * 100 + w + world)
    _, nbytes = band_payload_layout(frames, cout, h, w, world, wire)
    slab_bytes = nbytes + 32                                           # slack past the need, poisoned
    slabs = np.full((world, slab_bytes), 0xFF, np.uint8)
    for r in range(world):
        y0, y1 = band_rows(h, world, r)
        m = frames * cout * (y1 - y0) * w
        if wire == "u8":
            slabs[r, :m] = rng.integers(0, 256, size=m).astype(np.uint8)
        else:
            slabs[r, :4 * m] = rng.normal(0, 1, m).astype(np.float32).view(np.uint8)
    da = rng.uniform(0.01, 0.3, cout).astype(np.float32)
    za = np.asarray((0, 37, 255), np.float32)[np.arange(cout) % 3]
    want = P.ref_assemble(slabs, frames, cout, h, w, world, wire, da, za)
    out = Out((frames, cout, h * w))
    sd, dd, zd = dev(slabs), dev(da), dev(za)
    L.check(L.load().qv2x_assemble_bands(L.ptr(sd), world, slab_bytes, frames, cout, h, w, L.WIRES[wire], L.ptr(dd), L.ptr(zd), L.ptr(out.t),
                                         L.current_stream()), "assemble")
    np.testing.assert_array_equal(out.np(), want.reshape(frames, cout, h * w))
