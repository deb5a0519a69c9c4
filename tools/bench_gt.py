"""Ground-truth assembly at a size a user runs: 32 frames x 4 CAVs x 100 objects each (8-float rows, ids shared between the CAVs, a
quarter of the objects out of range).  ``qv2x_gt_boxes_f32`` inside a HIP graph (median of five windows and their spread) against the
plugin's numpy statement (``voxel_postprocessor.gt_boxes_frame``, every frame, the same inputs), outputs compared at the timed size.  The
kernel is small and latency-bound: one workgroup per frame, 32 workgroups on the chip; no ratio is required of it and no roofline fraction
is claimed -- the file records what was measured.  Writes profiles/gt_batch.json.

    python tools/bench_gt.py [--out FILE] [--windows 5] [--git-head REV]

No GPU: an error, not a fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, AGENTS, OBJ_CAP, N_OBJ, GT_CAP = 32, 4, 100, 100, 256
GT_RANGE = [-100.0, -40.0, -15.0, 100.0, 40.0, 15.0]
CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "host clock around graph replays that end in torch.cuda.synchronize",
    "graph warmed up (two eager calls on a side stream before capture, three replays before the first window)",
    "windows of at least 0.25 s of GPU work, five of them; the spread (highest minus lowest window) next to the median",
    "a size a user runs: 32 frames, 4 CAVs, 100 objects per CAV",
    "GPU and numpy outputs compared at the timed size",
    "no profiler attached to the timed run",
]


def workload(seed=9):
    """per frame 160 objects in the ego frame, each seen by 2 or 3 of the 4 CAVs (100 per CAV); a quarter lie outside the range in y"""
    import numpy as np
    g = np.random.default_rng(seed)
    boxes = np.zeros((FRAMES, AGENTS, OBJ_CAP, 8), np.float32)
    ids = np.zeros((FRAMES, AGENTS, OBJ_CAP), np.int32)
    tf = np.zeros((FRAMES, AGENTS, 4, 4), np.float32)
    for f in range(FRAMES):
        n = 160
        x, yaw, lab = g.uniform(-90, 90, n), g.uniform(-np.pi, np.pi, n), g.integers(1, 4, n)
        y = np.where(g.random(n) < 0.25, g.uniform(44, 60, n) * g.choice([-1, 1], n), g.uniform(-34, 34, n))
        seen = [[] for _ in range(AGENTS)]
        for k in g.permutation(n):                                    # fill the CAVs evenly: 400 sightings of 160 objects
            for a in sorted(range(AGENTS), key=lambda a: len(seen[a]))[:(3 if k % 2 else 2)]:
                seen[a].append(k)
        for a in range(AGENTS):
            ang = g.uniform(-np.pi, np.pi) if a else 0.0
            t = np.eye(4)
            t[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
            t[:3, 3] = [g.uniform(-20, 20), g.uniform(-10, 10), g.uniform(-0.3, 0.3)] if a else 0.0
            tf[f, a] = t
            inv = np.linalg.inv(t)
            for s, k in enumerate(seen[a][:N_OBJ]):
                p = inv @ np.array([x[k], y[k], -1.0, 1.0])
                boxes[f, a, s] = [p[0], p[1], p[2], 1.6, 1.9, 4.2, yaw[k] - ang, lab[k]]
                ids[f, a, s] = 10000 * f + k
    mask = (boxes[..., 5] > 0).astype(np.uint8)
    return {"boxes": boxes, "mask": mask, "ids": ids, "transforms": tf, "agent_counts": np.full((FRAMES,), AGENTS, np.int32)}


def cpu_path(w):
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gt_boxes_frame
    return [gt_boxes_frame(w["boxes"][f], w["mask"][f], w["ids"][f], w["transforms"][f], order="hwl", mode=0, gt_range=GT_RANGE, range_xy_only=True)
            for f in range(FRAMES)]


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_batch.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt: no GPU -- nothing is measured on the CPU")
    from quantv2x_amd.engine import capture_call
    from quantv2x_amd.ground_truth import gpu_gt_boxes_batch
    w = workload()
    t = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    out = gpu_gt_boxes_batch(t["boxes"], t["mask"], t["ids"], t["transforms"], t["agent_counts"], order="hwl", mode=0, gt_range=GT_RANGE,
                             range_xy_only=True, gt_cap=GT_CAP)                                  # fixed outputs: the graph writes them in place
    call = lambda: gpu_gt_boxes_batch(t["boxes"], t["mask"], t["ids"], t["transforms"], t["agent_counts"], order="hwl", mode=0,   # noqa: E731
                                      gt_range=GT_RANGE, range_xy_only=True, gt_cap=GT_CAP, out=out)
    replay = capture_call(call)
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    replay()
    torch.cuda.synchronize()
    reps = max(3, int(0.25 / max(time.perf_counter() - t0, 1e-6)) + 1)
    win = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            replay()
        torch.cuda.synchronize()
        win.append((time.perf_counter() - t0) / reps)
    got = {k: v.cpu().numpy() for k, v in replay().items()}
    torch.cuda.synchronize()
    cpu_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = cpu_path(w)
        cpu_s.append(time.perf_counter() - t0)
    same, max_diff = True, 0.0
    for f in range(FRAMES):
        n = len(ref[f]["rows"])
        same &= int(got["counts"][f]) == n == int(got["totals"][f]) and np.array_equal(got["ids"][f, :n], ref[f]["ids"])
        same &= np.array_equal(got["labels"][f, :n], ref[f]["labels"])
        if same and n:
            max_diff = max(max_diff, float(np.abs(got["corners"][f, :n].astype(np.float64) - ref[f]["corners"]).max()))
    same &= max_diff <= 2.0 ** -23 * 256.0                            # one f32 ulp at the workload's magnitude (coordinates below 128 m)
    gpu_us, cpu_us = statistics.median(win) * 1e6, statistics.median(cpu_s) * 1e6
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "workload": {"frames": FRAMES, "cavs_per_frame": AGENTS, "objects_per_cav": N_OBJ, "row_floats": 8, "mode": "de-duplicate by id",
                           "range_xy_only": True, "gt_range": GT_RANGE, "candidates": int(w["mask"].sum()), "gt_boxes": int(got["counts"].sum())},
              "method": "one qv2x_gt_boxes_f32 call (one launch, one workgroup per frame) in a HIP graph; median of the windows' time per replay "
                        "and the spread (highest minus lowest window).  Latency-bound: no roofline fraction is claimed.",
              "checklist": CHECKLIST,
              "gpu": {"median_us": round(gpu_us, 2), "spread_us": round((max(win) - min(win)) * 1e6, 2), "windows_us": [round(x * 1e6, 2) for x in win],
                      "replays_per_window": reps, "us_per_frame": round(gpu_us / FRAMES, 3)},
              "cpu_path": {"what": "plugin voxel_postprocessor.gt_boxes_frame over the 32 frames, numpy, one thread of the host (no upload counted)",
                           "median_us": round(cpu_us, 1), "runs_us": [round(x * 1e6, 1) for x in cpu_s], "us_per_frame": round(cpu_us / FRAMES, 1)},
              "cpu_over_gpu": round(cpu_us / gpu_us, 1), "outputs_identical_decisions": bool(same), "corners_max_abs_diff_m": max_diff}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: result[k] for k in ("gpu", "cpu_path", "cpu_over_gpu", "outputs_identical_decisions", "corners_max_abs_diff_m")}))
    if not same:
        raise SystemExit("bench_gt: GPU and numpy outputs differ")


if __name__ == "__main__":
    main()
