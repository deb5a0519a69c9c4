"""The deployed camera encoder (``engine_camera.DeployedCameraEncoder``: stem, layer1, layer2, heads, lift-splat) at the shape of
exemplar.yaml's m4 modality -- ``img_downsample`` 8, ``img_features`` 128 -- on four 384 x 512 cameras, 48 depth bins, the grid
profiles/lift_splat.json uses, for 1 and for 8 agents per call.  One call inside a HIP graph, median of five windows and their spread,
next to a torch transcription of the reference's fake-quant forward written here (``torch_encoder`` below: F.conv2d on dequantized weights,
round / clamp / rescale after every quantized layer, then the reference's outer product and voxel pooling as tools/bench_lift_splat.py
transcribes them) on the same device, state and images, run eagerly.  The parent commit has no camera encoder to compare with.  Weights
and quantizers are the seeded random state of tests/_camera.py with zero point 0 behind every ReLU, as min-max calibration gives.
No figure is required; the file records the times, the work by arithmetic and two rates: the stem's against the f32 vector pipe it runs on
(2 * 147 * 64 * Hc * Wc * V flop) and the heads' against the int8 MFMA peak.  Writes profiles/camera_encoder.json.

    python tools/bench_camera_encoder.py [--out FILE] [--windows 5] [--agents 1 8] [--git-head REV]
    rocprofv3 --kernel-trace -d DIR -o cam -- python tools/bench_camera_encoder.py --kernel-run    (a run of its own: 12 eager calls, 1 agent)
    python tools/bench_camera_encoder.py --kernel-stats DIR [--out FILE]                            (adds the per-stage split to the file)

No GPU: an error, not a fallback."""
import argparse
import csv
import glob
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from bench_lift_splat import FINAL_DIM, GRID, VIEWS, git_head, rig, torch_form, windows  # noqa: E402

FEATURES, DEPTH_BINS, DOWNSAMPLE = 128, 48, 8
F32_VECTOR_PEAK_TFLOPS = 157.3          # packed FMAs (v_pk_fma_f32); the stem issues plain v_fma_f32: half of it
INT8_MFMA_PEAK_TOPS = 5000.0
KERNEL_RUN_CALLS = 12
STAGES = ("stem", "layer1", "layer2", "heads", "splat")
CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "host clock around graph replays (the deployed form) or eager calls (the torch form) that end in torch.cuda.synchronize",
    "graphs warmed up (two eager calls on a side stream before capture, three replays before the first window)",
    "windows of at least 0.25 s of GPU work, five of them; the spread (highest minus lowest window) next to the median",
    "a size a user runs: the m4 camera setting of exemplar.yaml at the OPV2V image size, 1 and 8 agents per call",
    "outputs compared at the timed size: the deployed depth / feature codes against the torch form's, in LSBs",
    "no profiler attached to the timed run; the per-stage split comes from a rocprofv3 run of its own",
]


def state_for_bench():
    from _camera import camera_state
    return camera_state(17, FINAL_DIM, DEPTH_BINS, FEATURES, zero_points=False, grid=GRID, downsample=DOWNSAMPLE)


def torch_encoder(state, imgs):
    """the reference's fake-quant forward of QuantCamEncode_Resnet101 on a state: (depth logits, features), f32 on the device"""
    import torch
    import torch.nn.functional as F
    from quantv2x_amd.camera_encoder import dequant_weight
    dev = imgs.device
    cache = torch_encoder.__dict__.setdefault("cache", {})

    def layer(name, x, stride=1, relu=True):
        if name not in cache:
            w = torch.from_numpy(dequant_weight(state, name)).to(dev)
            cache[name] = (w, torch.from_numpy(state[name + "/bias"]).to(dev), w.shape[-1] // 2)
        w, b, pad = cache[name]
        y = F.conv2d(x, w, b, stride=stride, padding=pad)
        y = F.relu(y) if relu else y
        return y if bool(state[name + "/a_off"]) else fq(y, name)

    def fq(y, name):
        d, z = float(state[name + "/a_delta"]), float(state[name + "/a_zp"])
        return (torch.clamp(torch.round(y / d) + z, 0, 255) - z) * d
    x = F.max_pool2d(layer("conv1", imgs[:, :3], 2), 3, 2, 1)
    for lname, count in (("layer1", 3), ("layer2", 4)):
        for i in range(count):
            b = f"{lname}.{i}"
            stride = 2 if (lname == "layer2" and i == 0) else 1
            res = layer(b + ".downsample", x, stride, relu=False) if (b + ".downsample/w_code") in state else x
            y = layer(b + ".conv3", layer(b + ".conv2", layer(b + ".conv1", x), stride), relu=False)
            x = fq(F.relu(y + res), b)
    return layer("depth_head", x, relu=False), layer("image_head", x, relu=False)


def measure(agents, n_windows, state):
    import numpy as np
    import torch
    from quantv2x_amd import lift_splat as ls
    from quantv2x_amd.engine_camera import DeployedCameraEncoder
    m = rig(agents)
    names = ("rots", "trans", "intrins", "post_rots", "post_trans")
    eng = DeployedCameraEncoder(state, VIEWS, agents, "cuda").plan(*(torch.tensor(m[k]).cuda() for k in names))
    g = torch.Generator(device="cuda").manual_seed(agents)
    imgs = torch.randn((agents * VIEWS, 3, *FINAL_DIM), device="cuda", generator=g)
    sync = torch.cuda.synchronize
    t_all = windows(eng.capture(imgs), n_windows, sync)
    from quantv2x_amd.engine import capture_call
    t_enc = windows(capture_call(lambda: eng.features(imgs)), n_windows, sync)
    depth, feats = (t.clone() for t in eng.features(imgs))
    bev = eng(imgs).clone()
    geom = torch.tensor(ls.geometry_statement(eng.splat.frustum, *(m[k] for k in names))).cuda()
    dx, bx, nx = eng.splat.dx.cuda(), eng.splat.bx.cuda(), eng.splat.nx.cuda()

    def torch_all():
        d, f = torch_encoder(state, imgs)
        return torch_form(geom, d, f, dx, bx, nx)
    with torch.no_grad():
        t_tenc = windows(lambda: torch_encoder(state, imgs), n_windows, sync)
        t_tall = windows(torch_all, n_windows, sync)
        rd, rf = torch_encoder(state, imgs)
        rbev = torch_all()
    lsb_d = ((depth - rd).abs() / float(state["depth_head/a_delta"])).round()
    lsb_f = ((feats - rf).abs() / float(state["image_head/a_delta"])).round()
    inv = eng.work_inventory()
    res = {"agents": agents, "images": agents * VIEWS,
           "deployed": {"images_to_bev": t_all, "images_to_depth_and_features": t_enc},
           "torch_form": {"images_to_bev": t_tall, "images_to_depth_and_features": t_tenc,
                          "what": "eager torch on the same device, state and images: F.conv2d on dequantized weights + round / clamp / rescale per "
                                  "quantized layer, then the outer product and the reference's voxel pooling (tools/bench_lift_splat.py torch_form)"},
           "torch_form_over_deployed_images_to_bev": round(t_tall["median_us"] / t_all["median_us"], 2),
           "torch_form_over_deployed_encoder": round(t_tenc["median_us"] / t_enc["median_us"], 2),
           "outputs": {"depth_share_of_elements_that_differ": float((lsb_d != 0).float().mean()), "depth_largest_difference_lsb": float(lsb_d.max()),
                       "features_share_of_elements_that_differ": float((lsb_f != 0).float().mean()), "features_largest_difference_lsb": float(lsb_f.max()),
                       "note": "end to end, not teacher-forced: one code that the torch form's fp32 convolution rounds the other way is amplified "
                               "by the random-weight stack (tests/test_camera_encoder_cpu.py compares layer by layer)",
                       "bev_largest_abs_difference": float((bev - rbev).abs().max()), "bev_largest_abs_value": float(bev.abs().max())},
           "work_by_arithmetic": inv}
    del eng, geom
    torch.cuda.empty_cache()
    return res


def stage_split(directory, inv):
    """per-stage kernel time of one call, averaged over the traced calls but the first: dispatches in start order, a call = from one
    cam_stem_kernel to the next; inside it 1 stem, then layer1's and layer2's launches by count, cam_heads_kernel, the rest the splat's"""
    rows = []
    for db in glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True):
        con = sqlite3.connect(db)
        tables = [r[0] for r in con.execute("select name from sqlite_master where type='table'")]
        kd = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
        rows += con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id").fetchall()
    if not rows:
        for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: r[1])
    starts = [i for i, r in enumerate(rows) if "cam_stem_kernel" in r[0]]
    if len(starts) < 3:
        raise SystemExit(f"bench_camera_encoder: {len(starts)} stem dispatches under {directory}")
    n1, n2 = inv["layer1"]["launches"], inv["layer2"]["launches"]
    total = {s: 0.0 for s in STAGES}
    gaps, calls = 0.0, 0
    for a, b in zip(starts[1:], starts[2:] + [len(rows)]):
        call = rows[a:b]
        if "cam_heads_kernel" not in call[1 + n1 + n2][0]:
            raise SystemExit(f"bench_camera_encoder: launch {1 + n1 + n2} of a call is {call[1 + n1 + n2][0][:60]}, not the heads")
        parts = {"stem": call[:1], "layer1": call[1:1 + n1], "layer2": call[1 + n1:1 + n1 + n2], "heads": call[1 + n1 + n2:2 + n1 + n2], "splat": call[2 + n1 + n2:]}
        for s, ks_ in parts.items():
            total[s] += sum(e - st for _, st, e in ks_)
        gaps += (call[-1][2] - call[0][1]) - sum(e - st for _, st, e in call)
        calls += 1
    out = {s: {"kernel_us": round(total[s] / calls / 1e3, 2)} for s in STAGES}
    out["sum_of_kernels_us"] = round(sum(total.values()) / calls / 1e3, 2)
    out["gaps_between_kernels_us_eager"] = round(gaps / calls / 1e3, 2)
    out["calls_averaged"], out["launches_per_call"] = calls, len(rows[starts[1]:starts[2]])
    return out


def rates(split, inv):
    stem_flop, heads_ops = 2.0 * inv["stem"]["f32_macs"], 2.0 * inv["heads"]["int8_macs"]
    st, hd = split["stem"]["kernel_us"] * 1e-6, split["heads"]["kernel_us"] * 1e-6
    return {"stem_tflops": round(stem_flop / st / 1e12, 2), "stem_share_of_f32_vector_peak_157.3": round(stem_flop / st / 1e12 / F32_VECTOR_PEAK_TFLOPS, 4),
            "stem_share_of_plain_v_fma_rate_78.65": round(stem_flop / st / 1e12 / (F32_VECTOR_PEAK_TFLOPS / 2), 4),
            "heads_tops": round(heads_ops / hd / 1e12, 2), "heads_share_of_int8_mfma_peak_5000": round(heads_ops / hd / 1e12 / INT8_MFMA_PEAK_TOPS, 5),
            "layer1_tops": round(2.0 * inv["layer1"]["int8_macs"] / (split["layer1"]["kernel_us"] * 1e-6) / 1e12, 2),
            "layer2_tops": round(2.0 * inv["layer2"]["int8_macs"] / (split["layer2"]["kernel_us"] * 1e-6) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_encoder.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--git-head", default=None)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            result = json.load(fh)
        inv = result["runs"][0]["work_by_arithmetic"]
        split = stage_split(args.kernel_stats, inv)
        split["rates"] = rates(split, inv)
        split["source"] = (f"rocprofv3 --kernel-trace over {KERNEL_RUN_CALLS} eager calls at 1 agent (the first left out), a run of its own: "
                           "rocprofv3 --kernel-trace -d DIR -o cam -- python tools/bench_camera_encoder.py --kernel-run, then --kernel-stats DIR")
        result["stages"] = split
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print(json.dumps(split))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_encoder: no GPU -- nothing is measured on the CPU")
    state = state_for_bench()
    if args.kernel_run:
        from quantv2x_amd.engine_camera import DeployedCameraEncoder
        m = rig(1)
        eng = DeployedCameraEncoder(state, VIEWS, 1, "cuda").plan(*(torch.tensor(m[k]).cuda() for k in ("rots", "trans", "intrins", "post_rots", "post_trans")))
        imgs = torch.randn((VIEWS, 3, *FINAL_DIM), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        for _ in range(KERNEL_RUN_CALLS + 1):
            eng(imgs)
            torch.cuda.synchronize()
        return
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "workload": {"cameras_per_agent": VIEWS, "image": list(FINAL_DIM), "downsample": DOWNSAMPLE, "feature_map": [48, 64], "depth_bins": DEPTH_BINS,
                           "features": FEATURES, "grid_conf": GRID, "images": "normal", "state": "tests/_camera.py camera_state(17), zero point 0 behind every ReLU"},
              "method": "deployed form: HIP graph replays, median of the windows' time per replay and the spread (highest minus lowest window); "
                        "torch form: eager calls, the same windows",
              "checklist": CHECKLIST, "runs": [measure(a, args.windows, state) for a in args.agents]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for r in result["runs"]:
        print(json.dumps({"agents": r["agents"], "deployed_us": r["deployed"]["images_to_bev"]["median_us"], "deployed_encoder_us": r["deployed"]["images_to_depth_and_features"]["median_us"],
                          "torch_us": r["torch_form"]["images_to_bev"]["median_us"], "torch_encoder_us": r["torch_form"]["images_to_depth_and_features"]["median_us"],
                          "outputs": {k: v for k, v in r["outputs"].items() if k != "note"}}))


if __name__ == "__main__":
    main()
