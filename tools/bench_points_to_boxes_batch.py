"""Sweeps -> boxes at 8 and 32 frames of the bench's V2X-Real configuration, inside HIP graphs: the per-frame chain exactly as
``bench.points_to_boxes_line`` builds it (``GpuVoxelizer.fixed``: one C call per sweep; the engine; one ``gpu_post_process`` per frame)
against the batched chain (``quantv2x_amd.pipeline.PointsToBoxes``: ``fixed_batch``, the engine, ``gpu_post_process_batch``), and each of
the two stages alone in both forms.  Both arms run in this process, alternating, five windows each; per arm the median window and the
spread (highest minus lowest window).  Writes profiles/points_to_boxes_batch.json.

    python tools/bench_points_to_boxes_batch.py [--out FILE] [--frames 8 32] [--windows 5] [--git-head REV]

No GPU: an error, not a fallback.  The PTQ state comes from tools/cache/v2xreal_state.npz when tools/make_state_cache.py wrote one, else
it is calibrated here (CPU, some tens of seconds)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "host clock around replays that end in torch.cuda.synchronize (a launch returns before its kernels finish)",
    "every graph warmed up (two eager calls on a side stream before capture, three replays before the first window)",
    "windows of at least 0.25 s of GPU work",
    "the two arms alternate in the same process, five windows each; the spread is reported next to the median",
    "sizes a user runs: V2X-Real grid, 60 000-point sweeps, 8 and 32 frames, 1000 boxes",
    "outputs of the two arms compared bit for bit at the timed sizes",
    "no profiler attached",
]


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def windows(arms, n_windows, min_s=0.25):
    """``arms``: {name: replay}.  -> {name: [seconds per replay, one per window]}, the arms alternating window by window"""
    import torch
    reps = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(min_s / max(time.perf_counter() - t0, 1e-6)) + 1)
    out = {name: [] for name in arms}
    for _ in range(n_windows):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / reps[name])
    return out


def verdict(w):
    """median and spread per arm, the ratio, and whether the batched arm wins by more than the larger spread"""
    r = {}
    for name, v in w.items():
        r[name] = {"median_us": round(statistics.median(v) * 1e6, 1), "spread_us": round((max(v) - min(v)) * 1e6, 1),
                   "windows_us": [round(x * 1e6, 1) for x in v]}
    gain = r["per_frame"]["median_us"] - r["batched"]["median_us"]
    r["per_frame_over_batched"] = round(r["per_frame"]["median_us"] / r["batched"]["median_us"], 3)
    r["batched_wins_beyond_spread"] = bool(gain > max(r["per_frame"]["spread_us"], r["batched"]["spread_us"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_to_boxes_batch.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_points_to_boxes_batch: no GPU -- nothing is measured on the CPU")
    import bench
    from quantv2x_amd import synth
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.pipeline import PointsToBoxes
    from quantv2x_amd.plugin.data_utils.post_processor import build_postprocessor
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process, gpu_post_process_batch
    from quantv2x_amd.ptq_state import load_ptq_state
    from quantv2x_amd.voxelizer import GpuVoxelizer
    device = torch.device("cuda", 0)
    cache = os.path.join(ROOT, "tools", "cache", f"{bench.SHAPE}_state.npz")
    state = load_ptq_state(cache) if os.path.exists(cache) else bench.build_engine(16)[0]
    lidar, vox, max_vox, _ = synth.SHAPES[bench.SHAPE]
    gw, gh, _ = synth.grid_size(lidar, vox)
    eng = deploy(state=state)
    cap, max_boxes = 40960, 1000                                  # (bench.points_to_boxes_line's)
    new_vz = lambda: GpuVoxelizer(lidar, vox, 32, max_vox)        # a voxelizer / post-processor per graph: each owns the workspace its graph replays on
    new_pp = lambda: build_postprocessor(synth.mc_postprocess_params(lidar, gw, gh), train=False)
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0), "shape": bench.SHAPE, "points_per_sweep": bench.N_POINTS,
              "pillar_rows_per_sweep": cap, "max_boxes": max_boxes, "windows_per_arm": args.windows,
              "method": "HIP graphs; per arm the median of the windows' time per replay and the spread (highest minus lowest window); the arms alternate",
              "checklist": CHECKLIST, "frames": {}}
    for frames in args.frames:
        sweeps = [torch.from_numpy(synth.make_points(lidar, bench.N_POINTS, 3000 + f)).to(device) for f in range(frames)]
        pairwise = torch.eye(4, dtype=torch.float64).reshape(1, 1, 1, 4, 4).repeat(frames, 5, 5, 1, 1).to(device)
        rl = torch.ones(frames, dtype=torch.int64)
        p2b = PointsToBoxes(eng, new_vz(), new_pp(), cap, max_boxes=max_boxes)
        anchors_dev, per_cell = p2b.anchors_dev, p2b.per_cell
        post_kw = dict(anchors_per_cell=per_cell, num_bins=0, dir_offset=0.0, range_xy_only=True, max_extent=100.0, z_lim=(-100.0, 100.0), max_boxes=max_boxes)

        def post_loop(pp, cls, reg):
            return [gpu_post_process(pp, cls[f:f + 1], reg[f:f + 1], None, anchors_dev, torch.eye(4), num_classes=int(cls.shape[1] // per_cell),
                                     rng=pp.gt_range, sync=False, **post_kw) for f in range(frames)]

        vz_a, pp_a = new_vz(), new_pp()

        def chain_per_frame():                                    # bench.points_to_boxes_line's run()
            inp = vz_a.fixed(sweeps, cap)
            o = eng({"inputs_m1": inp, "agent_modality_list": ["m1"] * frames, "record_len": rl, "pairwise_t_matrix": pairwise})
            return inp, post_loop(pp_a, o["cls_preds"], o["reg_preds"])
        g_a = bench._graph_of(chain_per_frame)
        replay_b = p2b.capture(sweeps)
        entry = {"chain": verdict(windows({"per_frame": g_a, "batched": replay_b}, args.windows))}
        # the two arms computed the same thing
        g_a(); out_b = replay_b(); torch.cuda.synchronize()
        inp_a, res_a = g_a.__self__.keep
        same = torch.equal(inp_a["voxel_counts"], out_b["voxel_counts"])
        for f, (c, s, l, n) in enumerate(res_a):
            k = int(n)
            same = same and int(out_b["counts"][f]) == k and torch.equal(out_b["corners"][f, :k], c[:k]) and torch.equal(out_b["scores"][f, :k], s[:k]) \
                and torch.equal(out_b["labels"][f, :k], l[:k])
        entry["outputs_identical"] = bool(same)
        entry["pillars"] = [int(v) for v in out_b["voxel_counts"].tolist()][:4]
        entry["boxes"] = [int(v) for v in out_b["counts"].tolist()][:4]
        o = eng({"inputs_m1": p2b.voxelizer.fixed_batch(sweeps, cap), "agent_modality_list": ["m1"] * frames, "record_len": rl, "pairwise_t_matrix": pairwise})
        cls, reg = o["cls_preds"].clone(), o["reg_preds"].clone()
        del g_a, replay_b, out_b, inp_a, res_a
        # ---- the stages alone ----
        vz_1, vz_2 = new_vz(), new_vz()
        entry["voxelize"] = verdict(windows({"per_frame": bench._graph_of(lambda: vz_1.fixed(sweeps, cap)),
                                             "batched": bench._graph_of(lambda: vz_2.fixed_batch(sweeps, cap))}, args.windows))
        pp_1, pp_2 = new_pp(), new_pp()
        eye = torch.eye(4, dtype=torch.float32).repeat(frames, 1, 1).to(device).contiguous()
        entry["post_process"] = verdict(windows({
            "per_frame": bench._graph_of(lambda: post_loop(pp_1, cls, reg)),
            "batched": bench._graph_of(lambda: gpu_post_process_batch(pp_2, cls, reg, None, anchors_dev, eye, num_classes=int(cls.shape[1] // per_cell),
                                                                      rng=pp_2.gt_range, **post_kw))}, args.windows))
        for k in ("chain", "voxelize", "post_process"):
            entry[k]["per_frame"]["us_per_frame"] = round(entry[k]["per_frame"]["median_us"] / frames, 1)
            entry[k]["batched"]["us_per_frame"] = round(entry[k]["batched"]["median_us"] / frames, 1)
        entry["chain"]["frames_per_s"] = {a: round(frames * 1e6 / entry["chain"][a]["median_us"], 1) for a in ("per_frame", "batched")}
        result["frames"][str(frames)] = entry
        print(json.dumps({str(frames): entry}), flush=True)
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
