"""``qv2x_bev_entry_f32`` -- the input side of a camera agent's first BasicBlock on the lift-splat's fp32 BEV -- against the form the
library's other entries compose, at the shape of CameraOnly/camera_pyramid.yaml (``img_features`` 128, grid 256 x 256 x 1, ``layer_strides``
[2], 64 filters) for 1 and for 8 agents per call, and the cost of the camera crop mask on the fusion scores of a scene.

  fused     one launch: conv1 codes into a padded i8 BEV + the shortcut's fp32 rows
  composed  the same two results from today's entries: a torch transpose and pad of the [n, C, Y, X] map into a zero-bordered NHWC tensor,
            ``qv2x_conv3x3_f32`` (ReLU in its epilogue), a quantizing pass (torch: multiply-add, round, clamp, cast into the padded i8 BEV),
            and the strided 1x1 as a strided gather of the centre pixels + ``qv2x_deconv_f32`` with s = 1.  Its sums walk K in the fp32
            path's own order (k0, k4, k1, ...), so its codes may differ from the fused form's by an LSB; the share is recorded.
  mask      ``score.mul_(mask)`` on the three levels' scores [n, h * w] of a scene of ``agents`` (128 x 128, 64 x 64, 32 x 32)

  agent     images to wire codes: ``DeployedPyramidModel.encode_features`` of a camera state (four 384 x 512 cameras, 48 depth bins, ResNet-101
            trunk, the entry, three BasicBlocks at 128 x 128, the crop copy, the 64-wide codebook encode) as one HIP graph, per call and per agent;
            the state is the plugin's own model at that shape with seeded weights, min-max calibrated on one scene on the CPU

Both forms alternate in one process inside HIP graphs (``engine.capture_call``): fused, composed, fused, composed, each run the median of five
windows of at least 0.25 s with its spread (highest minus lowest window).  Reported per form: the run with the LOWER median of its two (both runs
are kept in the file under ``*_runs``).  The composed form is the denominator.  Weights, quantizer and maps of the entry rows are seeded random,
made here.  Writes profiles/camera_pyramid.json.  No GPU: an error, not a fallback.

    python tools/bench_camera_pyramid.py [--out FILE] [--windows 5] [--agents 1 8] [--no-agent-row] [--git-head REV]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from bench_lift_splat import git_head, windows  # noqa: E402

CIN, COUT, H, W, STRIDE = 128, 64, 256, 256, 2
F32_MFMA_PEAK_TFLOPS = 157.3
BLOCK = "backbone_m2.resnet.layer0.0"
RANGE = [-51.2, -51.2, -3.0, 51.2, 51.2, 1.0]
GRID = {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10.0, 10.0, 20.0], "ddiscr": [2.0, 50.0, 48.0], "mode": "LID"}
FINAL_DIM, VIEWS = (384, 512), 4


def block_state(seed):
    """conv1 (3x3, CIN -> COUT, its quantizer with zero point 0 as calibration gives behind a ReLU) and the 1x1 downsample of one BasicBlock"""
    import numpy as np
    rng = np.random.default_rng(seed)
    s = {}
    for name, k, a_off in ((BLOCK + ".conv1", 3, False), (BLOCK + ".downsample", 1, True)):
        s[name + "/w_code"] = rng.integers(0, 256, size=(COUT, CIN, k, k), dtype=np.uint8)
        s[name + "/w_zp"] = rng.integers(110, 146, size=COUT).astype(np.float32)
        s[name + "/w_delta"] = (rng.uniform(0.5, 1.5, size=COUT) / (74.0 * np.sqrt(k * k * CIN))).astype(np.float32)
        s[name + "/bias"] = (rng.standard_normal(COUT) * 0.3).astype(np.float32)
        s[name + "/a_delta"], s[name + "/a_zp"], s[name + "/a_off"] = np.float32(5.0 / 255.0), np.float32(0.0), np.bool_(a_off)
    return s


def bev_map(n, seed):
    """f32 [n, CIN, H, W]: a third of the cells hold exact zeros, as a splat leaves the ones no frustum point reaches"""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, CIN, H, W)).astype(np.float32)
    x[:, :, : H // 2, : W // 3] = 0.0
    x[:, :, H - H // 4:, W - W // 3:] = 0.0
    return x


def camera_rig(n, seed):
    """images and matrices of ``n`` agents with four cameras each (front / left / back / right, 1.6 m up), f32 on the CPU"""
    import numpy as np
    import torch
    g = np.random.default_rng(seed)
    cam = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    rots, trans = np.zeros((n, VIEWS, 3, 3)), np.zeros((n, VIEWS, 3))
    intr, post = np.zeros((n, VIEWS, 3, 3)), np.tile(np.eye(3), (n, VIEWS, 1, 1))
    for a in range(n):
        for v in range(VIEWS):
            yaw = 2 * np.pi * v / VIEWS + g.uniform(-0.2, 0.2)
            rots[a, v] = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]) @ cam
            trans[a, v] = [g.uniform(-1.5, 1.5), g.uniform(-0.8, 0.8), 1.6]
            intr[a, v] = [[400.0, 0, 400.0], [0, 400.0, 300.0], [0, 0, 1]]
            post[a, v, :2, :2] *= 0.64                                # 600 x 800 resized to 384 x 512
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))          # noqa: E731
    return {"imgs": t(g.standard_normal((n, VIEWS, 3, *FINAL_DIM))), "rots": t(rots), "trans": t(trans), "intrins": t(intr),
            "post_rots": t(post), "post_trans": torch.zeros(n, VIEWS, 3)}


def camera_state():
    """PTQ state of the camera modality of the plugin's Pyramid codebook model at the camera_pyramid.yaml shape (Resnet101 encoder, the one that
    deploys): seeded weights, W8A8 min-max, one calibration pass of one agent on the CPU, frozen"""
    import copy
    import torch
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.tools import train_utils
    from quantv2x_amd.plugin.tools.inference_quant import calibrate_minmax, wrap
    from quantv2x_amd.ptq_state import export_ptq_state
    hy = synth.make_pyramid_hypes("tiny", codebook=True, modalities=("m2",))
    args = hy["model"]["args"]
    args["lidar_range"] = list(RANGE)
    args["m2"] = {"core_method": "lift_splat_shoot", "sensor_type": "camera",
                  "encoder_args": {"grid_conf": dict(GRID), "data_aug_conf": {"final_dim": FINAL_DIM}, "img_downsample": 8, "img_features": CIN,
                                   "camera_encoder": "Resnet101", "use_depth_gt": False, "depth_supervision": False},
                  "camera_mask_args": {"cav_lidar_range": list(RANGE), "grid_conf": dict(GRID)},
                  "backbone_args": {"layer_nums": [3], "layer_strides": [STRIDE], "num_filters": [COUT], "inplanes": CIN},
                  "aligner_args": {"core_method": "identity"}}
    model = train_utils.create_model(copy.deepcopy(hy)).eval()
    synth.load_state_dict_numpy(model, synth.make_state_dict(model.state_dict(), seed=1))
    dd = {"agent_modality_list": ["m2"], "record_len": torch.tensor([1]), "pairwise_t_matrix": torch.eye(4).repeat(1, 5, 5, 1, 1),
          "inputs_m2": camera_rig(1, 3)}
    return export_ptq_state(calibrate_minmax(wrap(model), [dd]), modality="m2")


def agent_rows(agents, n_windows, dev, sync):
    """images -> wire codes of ``n`` camera agents as one HIP graph: per call and per agent"""
    import torch
    from quantv2x_amd.engine import capture_call
    from quantv2x_amd.engine_pyramid import DeployedPyramidModel
    eng = DeployedPyramidModel(camera_state(), device=dev)
    rows = []
    for n in agents:
        inputs = {k: v.to(dev) for k, v in camera_rig(n, 5).items()}
        codes = eng.encode_features(inputs, n)
        sync()
        assert tuple(codes.shape) == (eng.levels, n, (H // STRIDE) * (W // STRIDE)) and int(codes.max()) < eng.kc
        t = windows(capture_call(lambda: eng.encode_features(inputs, n)), n_windows, sync)
        rows.append({"agents": n, "images_to_wire_codes": t, "per_agent_us": round(t["median_us"] / n, 2),
                     "map": [eng.mh, eng.mw], "wire": [eng.levels, eng.fh * eng.fw], "distinct_codes_level0": int(torch.unique(codes[0]).numel())})
        print(json.dumps({"agents": n, "images_to_wire_codes_us": t["median_us"], "spread_us": t["spread_us"]}), flush=True)
    return rows


def build(n, dev):
    import numpy as np
    import torch
    from quantv2x_amd import lib as L
    from quantv2x_amd.camera_bev import BevEntry, entry_constants, entry_shapes
    from quantv2x_amd.engine_fp32 import pack_k8
    lib = L.load()
    state = block_state(7)
    x = torch.from_numpy(bev_map(n, 8)).to(dev)
    ho, wo = entry_shapes(H, W, STRIDE)
    entry = BevEntry(state, BLOCK, STRIDE, dev)
    out_f = torch.full((n, ho + 2, wo + 2, COUT), entry.zp - 128, dtype=torch.int8, device=dev)
    rows_f = torch.empty((n * ho * wo, COUT), dtype=torch.float32, device=dev)
    fused = lambda: entry(x, out_f, rows_f)                                  # noqa: E731

    w1, b1, (da, za), wd, bd = entry_constants(state, BLOCK)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    w1p, wdp, b1t, bdt = t(pack_k8(w1.T)), t(pack_k8(wd.T)), t(b1), t(bd)
    xp = torch.zeros((n, H + 2, W + 2, CIN), dtype=torch.float32, device=dev)
    y = torch.zeros((n, ho + 2, wo + 2, COUT), dtype=torch.float32, device=dev)
    centre = torch.zeros((n, ho + 2, wo + 2, CIN), dtype=torch.float32, device=dev)
    short = torch.zeros((n, ho + 2, wo + 2, COUT), dtype=torch.float32, device=dev)
    out_c = torch.full((n, ho + 2, wo + 2, COUT), entry.zp - 128, dtype=torch.int8, device=dev)
    rd = float(np.float32(1.0) / np.float32(da))

    def gemm(fn, name, src, h, w, cin, stride, wt, bias, dst, relu):
        d = L.F32ConvDesc()
        d.n, d.h, d.w, d.cin_total, d.cin0, d.cin = n, h, w, cin, 0, cin
        d.stride, d.cout, d.out_ctotal, d.out_c0, d.relu = stride, COUT, COUT, 0, relu
        L.check(fn(C.byref(d), L.ptr(src), L.ptr(wt), L.ptr(bias), L.ptr(dst), L.current_stream()), name)

    def composed():
        xp[:, 1:-1, 1:-1].copy_(x.permute(0, 2, 3, 1))                                                   # transpose and pad
        gemm(lib.qv2x_conv3x3_f32, "qv2x_conv3x3_f32", xp, H, W, CIN, STRIDE, w1p, b1t, y, 1)
        out_c[:, 1:-1, 1:-1].copy_(torch.clamp(torch.round(y[:, 1:-1, 1:-1] * rd + za), 0, 255) - 128)   # the quantizing pass
        centre[:, 1:-1, 1:-1].copy_(xp[:, 1:-1:STRIDE, 1:-1:STRIDE])                                     # the strided 1x1
        gemm(lib.qv2x_deconv_f32, "qv2x_deconv_f32", centre, ho, wo, CIN, 1, wdp, bdt, short, 0)

    def compare():
        fused(); composed(); torch.cuda.synchronize()
        diff = (out_f.to(torch.int16) - out_c.to(torch.int16)).abs()
        sdiff = (rows_f.view(n, ho, wo, COUT) - short[:, 1:-1, 1:-1]).abs().max()
        return {"codes_differing_share": float((diff != 0).float().mean()), "codes_max_lsb": int(diff.max()), "shortcut_max_abs_diff": float(sdiff)}
    return fused, composed, compare


def main():
    import torch
    from quantv2x_amd.engine import capture_call
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_pyramid.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--git-head", default=None, help="the revision to record (a copy of the tree without .git cannot ask git)")
    ap.add_argument("--no-agent-row", action="store_true", help="skip images -> wire codes (its state takes a CPU calibration pass)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_pyramid: needs an MI355X (torch.cuda.is_available() is False)")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    rows = []
    for n in args.agents:
        fused, composed, compare = build(n, dev)
        agree = compare()
        gf, gc = capture_call(fused), capture_call(composed)
        tf, tc = [], []
        for _ in range(2):                                                   # alternating: fused, composed, fused, composed
            tf.append(windows(gf, args.windows, sync))
            tc.append(windows(gc, args.windows, sync))
        best = lambda ts: min(ts, key=lambda r: r["median_us"])            # noqa: E731
        f, c = best(tf), best(tc)
        flop = 2.0 * n * (H // STRIDE) * (W // STRIDE) * COUT * (9 * CIN + CIN)
        masks = [torch.ones((n, h * h), device=dev) for h in (128, 64, 32)]
        scores = [torch.rand((n, h * h), device=dev) for h in (128, 64, 32)]
        gm = capture_call(lambda: [s.mul_(m) for s, m in zip(scores, masks)])
        rows.append({"agents": n, "fused": f, "composed": c, "fused_runs": tf, "composed_runs": tc,
                     "composed_over_fused": round(c["median_us"] / f["median_us"], 3),
                     "beats_composed_by_more_than_the_spread": bool(c["median_us"] - f["median_us"] > max(f["spread_us"], c["spread_us"])),
                     "gflop": round(flop / 1e9, 3), "fused_share_of_f32_mfma_peak": round(flop / (f["median_us"] * 1e-6) / (F32_MFMA_PEAK_TFLOPS * 1e12), 4),
                     "input_mbytes": round(n * CIN * H * W * 4 / 1e6, 2), "agreement": agree,
                     "mask_multiply_three_levels": windows(gm, args.windows, sync)})
        print(json.dumps({k: rows[-1][k] for k in ("agents", "composed_over_fused", "gflop", "fused_share_of_f32_mfma_peak", "agreement")}), flush=True)
        print("  fused", f["median_us"], "us (spread", f["spread_us"], ") composed", c["median_us"], "us (spread", c["spread_us"], ")", flush=True)
    result = {"tool": "tools/bench_camera_pyramid.py", "git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "shape": {"cin": CIN, "cout": COUT, "h": H, "w": W, "stride": STRIDE, "views": VIEWS, "final_dim": list(FINAL_DIM)}, "rows": rows,
              "reported": "per form the run with the lower median of two alternating runs; each run = median of the windows, spread = max - min window",
              "agent_rows": [] if args.no_agent_row else agent_rows(args.agents, args.windows, dev, sync)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
