"""The detection evaluator at a size a user runs: 32 frames x 1000 detections x 100 GT, 3 thresholds x 4 ranges, class-agnostic.
``qv2x_eval_tp_fp_f32`` inside a HIP graph (median of five windows and their spread) against the plugin's CPU path
(``plugin/utils/eval_utils.py:tp_fp_frame``, every frame, the same inputs; it is numpy with a vectorized bounding-box test in front of the
clipping -- far quicker than the reference's shapely loop, which cannot run here), outputs compared at the timed size.  Writes
profiles/eval_batch.json.

    python tools/bench_eval.py [--out FILE] [--windows 5] [--git-head REV]
    rocprofv3 --kernel-trace --stats -d DIR -o eval -- python tools/bench_eval.py --kernel-run      (a run of its own: 22 eager calls)
    python tools/bench_eval.py --kernel-stats DIR [--out FILE]                                      (adds the rank / IoU / match split)

No GPU: an error, not a fallback."""
import argparse
import csv
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, DET_CAP, N_DET, GT_CAP, N_GT = 32, 1000, 1000, 100, 100
THRESHOLDS = (0.3, 0.5, 0.7)
RANGES = ((-float("inf"), float("inf")), (0.0, 30.0), (30.0, 50.0), (50.0, 100.0))
KERNELS = {"rank": "ev_rank_kernel", "iou": "ev_iou_kernel", "match": "ev_match_kernel"}
CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "host clock around graph replays that end in torch.cuda.synchronize",
    "graph warmed up (two eager calls on a side stream before capture, three replays before the first window)",
    "windows of at least 0.25 s of GPU work, five of them; the spread (highest minus lowest window) next to the median",
    "a size a user runs: 32 frames, 1000 detections and 100 GT each, the reference's 3 thresholds x 4 ranges",
    "GPU and CPU outputs compared at the timed size",
    "no profiler attached to the timed run; the per-kernel split comes from a rocprofv3 run of its own",
]


def workload(seed=7):
    """jittered copies of the GT (four per GT, competing), the rest clutter; scores distinct and unsorted"""
    import numpy as np
    g = np.random.default_rng(seed)

    def boxes(x, y, l, w, yaw):
        tx, ty = np.array([1, 1, -1, -1]) * 0.5, np.array([-1, 1, 1, -1]) * 0.5
        c, s = np.cos(yaw)[..., None], np.sin(yaw)[..., None]
        px, py = tx * l[..., None], ty * w[..., None]
        out = np.zeros(x.shape + (8, 3), np.float32)
        out[..., :4, 0] = out[..., 4:, 0] = px * c - py * s + x[..., None]
        out[..., :4, 1] = out[..., 4:, 1] = px * s + py * c + y[..., None]
        out[..., :4, 2], out[..., 4:, 2] = -1.0, 0.6
        return out
    r, a = g.uniform(2.0, 108.0, (FRAMES, GT_CAP)), g.uniform(-np.pi, np.pi, (FRAMES, GT_CAP))
    gx, gy, gyaw = r * np.cos(a), r * np.sin(a), g.uniform(-np.pi, np.pi, (FRAMES, GT_CAP))
    gl, gw = 4.2 * g.uniform(0.85, 1.15, (FRAMES, GT_CAP)), 1.9 * g.uniform(0.85, 1.15, (FRAMES, GT_CAP))
    r, a = g.uniform(2.0, 108.0, (FRAMES, DET_CAP)), g.uniform(-np.pi, np.pi, (FRAMES, DET_CAP))
    dx, dy, dyaw = r * np.cos(a), r * np.sin(a), g.uniform(-np.pi, np.pi, (FRAMES, DET_CAP))
    dl, dw = np.full((FRAMES, DET_CAP), 4.2), np.full((FRAMES, DET_CAP), 1.9)
    hit, j = g.random((FRAMES, DET_CAP)) < 0.4, g.integers(0, N_GT, (FRAMES, DET_CAP))
    u = g.uniform(0.0, 1.0, (FRAMES, DET_CAP)) ** 2
    take = lambda v: np.take_along_axis(v, j, axis=1)                 # noqa: E731
    dx, dy = np.where(hit, take(gx) + g.normal(0, 1.2, u.shape) * u, dx), np.where(hit, take(gy) + g.normal(0, 1.2, u.shape) * u, dy)
    dyaw = np.where(hit, take(gyaw) + g.normal(0, 0.5, u.shape) * u, dyaw)
    dl, dw = np.where(hit, take(gl) * (1 + 0.3 * u), dl), np.where(hit, take(gw) * (1 - 0.3 * u), dw)
    scores = np.stack([((g.permutation(DET_CAP) + 1) / (DET_CAP + 1)).astype(np.float32) for _ in range(FRAMES)])
    return {"det_corners": boxes(dx, dy, dl, dw, dyaw), "det_scores": scores, "det_counts": np.full((FRAMES,), N_DET, np.int32),
            "gt_corners": boxes(gx, gy, gl, gw, gyaw), "gt_counts": np.full((FRAMES,), N_GT, np.int32)}


def cpu_path(w):
    from quantv2x_amd.plugin.utils.eval_utils import tp_fp_frame
    return [tp_fp_frame(w["det_corners"][f, :N_DET], w["det_scores"][f, :N_DET], w["gt_corners"][f, :N_GT], THRESHOLDS, RANGES) for f in range(FRAMES)]


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def kernel_stats(directory):
    """{short name: {calls, avg_us, min_us, max_us}} of the three kernels from a rocprofv3 --kernel-trace --stats output directory
    (its rocpd database, or its kernel_stats csv)"""
    rows = []
    for db in glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True):
        con = sqlite3.connect(db)
        tables = [r[0] for r in con.execute("select name from sqlite_master where type='table'")]
        kd = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
        rows += con.execute(f"select s.kernel_name, count(*), avg(d.end - d.start), min(d.end - d.start), max(d.end - d.start) "
                            f"from {kd} d join {ks} s on d.kernel_id = s.id group by s.kernel_name").fetchall()
    if not rows:
        for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])) for r in csv.DictReader(fh)]
    out = {}
    for short, name in KERNELS.items():
        hit = [r for r in rows if name in r[0]]
        if len(hit) != 1:
            raise SystemExit(f"bench_eval: {len(hit)} rows for {name} under {directory}")
        _, calls, avg, mn, mx = hit[0]
        out[short] = {"kernel": name, "calls": int(calls), "avg_us": round(avg / 1e3, 2), "min_us": round(mn / 1e3, 2), "max_us": round(mx / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batch.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--git-head", default=None)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            result = json.load(fh)
        result["kernels"] = kernel_stats(args.kernel_stats)
        result["kernels"]["sum_avg_us"] = round(sum(v["avg_us"] for v in result["kernels"].values()), 2)
        result["kernels"]["source"] = "rocprofv3 --kernel-trace --stats over 22 eager calls, a run of its own"
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print(json.dumps(result["kernels"]))
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: no GPU -- nothing is measured on the CPU")
    from quantv2x_amd.engine import capture_call
    from quantv2x_amd.evaluation import gpu_tp_fp_batch
    w = workload()
    t = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    call = lambda: gpu_tp_fp_batch(t["det_corners"], t["det_scores"], None, t["det_counts"], t["gt_corners"], None, t["gt_counts"],   # noqa: E731
                                   thresholds=THRESHOLDS, ranges=RANGES, num_classes=0)
    if args.kernel_run:
        for _ in range(22):
            call()
        torch.cuda.synchronize()
        return
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
    got = dict(zip(("order", "scores", "flags", "match", "gt"), (o.cpu().numpy() for o in replay())))
    torch.cuda.synchronize()
    cpu_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = cpu_path(w)
        cpu_s.append(time.perf_counter() - t0)
    same = all(np.array_equal(got[k][f], ref[f][k]) for f in range(FRAMES) for k in ("order", "scores", "flags", "match", "gt"))
    gpu_us, cpu_us = statistics.median(win) * 1e6, statistics.median(cpu_s) * 1e6
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "workload": {"frames": FRAMES, "detections_per_frame": N_DET, "gt_per_frame": N_GT, "thresholds": list(THRESHOLDS),
                           "ranges": [[str(a), str(b)] for a, b in RANGES], "num_classes": 0, "problems_per_frame": 12,
                           "true_positives": int((got["flags"] == 2).sum()), "false_positives": int((got["flags"] == 1).sum())},
              "method": "one qv2x_eval_tp_fp_f32 call in a HIP graph; median of the windows' time per replay and the spread (highest minus lowest window)",
              "checklist": CHECKLIST,
              "gpu": {"median_us": round(gpu_us, 1), "spread_us": round((max(win) - min(win)) * 1e6, 1), "windows_us": [round(x * 1e6, 1) for x in win],
                      "replays_per_window": reps, "us_per_frame": round(gpu_us / FRAMES, 2)},
              "cpu_path": {"what": "plugin/utils/eval_utils.py:tp_fp_frame over the 32 frames, numpy, one thread of the host",
                           "median_us": round(cpu_us, 1), "runs_us": [round(x * 1e6, 1) for x in cpu_s], "us_per_frame": round(cpu_us / FRAMES, 1)},
              "cpu_over_gpu": round(cpu_us / gpu_us, 1), "outputs_identical": bool(same), "kernels": None}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: result[k] for k in ("gpu", "cpu_path", "cpu_over_gpu", "outputs_identical")}))
    if not same:
        raise SystemExit("bench_eval: GPU and CPU outputs differ")


if __name__ == "__main__":
    main()
