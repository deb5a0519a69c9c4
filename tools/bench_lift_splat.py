"""Lift-splat BEV pooling at the OPV2V camera shape: 4 cameras, 48 depth bins (LID, 2..50 m), a 48 x 64 feature map (384 x 512 at
downsample 8), 128 features, a 256 x 256 x 1 grid of 0.4 m cells -- for 1 and for 8 agents per call.  ``qv2x_lss_plan_f32`` and
``qv2x_lss_splat_f32`` inside a HIP graph, timed separately and together (median of five windows and their spread), next to a torch
transcription of the reference's ``voxel_pooling`` written here (outer product, truncate, filter, argsort, cumsum differences, scatter:
``torch_form`` below) on the same device and the same inputs, run eagerly as the reference runs it (its boolean filters size tensors from
device data, so it cannot be captured).  Outputs are compared at the timed size.  No ratio is required and no roofline fraction is claimed:
the file records what was measured, the bytes each form has to move by arithmetic, and the fused form's floor bytes over its measured time
as a fraction of the HBM rate.  Writes profiles/lift_splat.json.

    python tools/bench_lift_splat.py [--out FILE] [--windows 5] [--agents 1 8] [--git-head REV]
    rocprofv3 --kernel-trace --stats -d DIR -o lss -- python tools/bench_lift_splat.py --kernel-run   (a run of its own: 22 eager plans and splats, 1 agent)
    python tools/bench_lift_splat.py --kernel-stats DIR [--out FILE]                                  (adds the per-kernel split to the file)

No GPU: an error, not a fallback."""
import argparse
import csv
import glob
import json
import os
import re
import sqlite3
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, FEATURES, FINAL_DIM, DOWNSAMPLE = 4, 128, (384, 512), 8
GRID = {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10, 10, 20], "ddiscr": [2, 50, 48], "mode": "LID"}
HBM_BYTES_PER_S = 8.0e12                                            # the MI355X's stated HBM3E rate
KERNEL_RUN_CALLS = 22
KERNELS = {"plan_clear": "lss_clear_kernel", "plan_views": "lss_views_kernel", "plan_cells": "lss_cells_kernel", "plan_heads": "lss_heads_kernel",
           "splat_softmax": "lss_softmax_kernel", "splat_transpose": "lss_transpose_kernel", "splat": "lss_splat_kernel"}
CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "host clock around graph replays (the fused form) or eager calls (the torch form) that end in torch.cuda.synchronize",
    "graphs warmed up (two eager calls on a side stream before capture, three replays before the first window)",
    "windows of at least 0.25 s of GPU work, five of them; the spread (highest minus lowest window) next to the median",
    "a size a user runs: the OPV2V camera yaml's shape, 1 and 8 agents per call",
    "both forms' outputs compared at the timed size, the fused form's against the float64 statement at 1 agent",
    "no profiler attached to the timed run; the per-kernel split comes from a rocprofv3 run of its own",
]


def rig(samples, seed=11):
    """four cameras per agent, roughly front / left / back / right, 1.5 to 1.9 m up, a few degrees of pitch; f32"""
    import numpy as np
    g = np.random.default_rng(seed)
    h, w = FINAL_DIM
    cam = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    m = {"rots": np.zeros((samples, VIEWS, 3, 3)), "trans": np.zeros((samples, VIEWS, 3)), "intrins": np.zeros((samples, VIEWS, 3, 3)),
         "post_rots": np.tile(np.eye(3), (samples, VIEWS, 1, 1)), "post_trans": np.zeros((samples, VIEWS, 3))}
    for s in range(samples):
        for v in range(VIEWS):
            yaw, pitch = 2 * np.pi * v / VIEWS + g.uniform(-0.2, 0.2), g.uniform(-0.02, 0.06)
            rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
            ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
            m["rots"][s, v] = rz @ ry @ cam
            m["trans"][s, v] = [g.uniform(-1.5, 1.5), g.uniform(-0.8, 0.8), g.uniform(1.5, 1.9)]
            scale = 0.64                                            # 600 x 800 resized to 384 x 512
            m["post_rots"][s, v, :2, :2] *= scale
            m["intrins"][s, v] = [[400.0, 0, 400.0], [0, 400.0, 300.0], [0, 0, 1]]
    return {k: v.astype(np.float32) for k, v in m.items()}


def torch_form(geom, depth_logits, feats, dx, bx, nx):
    """the reference's per-frame work from the geometry on, in its own steps and tensor shapes (lift_splat_shoot.py:125-181 with
    QuickCumsum; the outer product is what CamEncode hands on): f32 on the device"""
    import torch
    b, n, d, h, w, _ = geom.shape
    c = feats.shape[1]
    x = (depth_logits.softmax(dim=1).unsqueeze(1) * feats.unsqueeze(2)).view(b, n, c, d, h, w).permute(0, 1, 3, 4, 5, 2)   # the [B, N, D, fH, fW, C] product
    points = b * n * d * h * w
    x = x.reshape(points, c)
    cell = ((geom - (bx - dx / 2.)) / dx).long().view(points, 3)                                 # truncation toward zero
    sample = torch.arange(points, device=x.device).div(points // b, rounding_mode="floor")
    inside = ((cell >= 0) & (cell < nx)).all(dim=1)                                             # a boolean filter: sizes from device data
    x, cell, sample = x[inside], cell[inside], sample[inside]
    ix, iy, iz = cell.unbind(1)
    ranks = ((ix * nx[1] + iy) * nx[2] + iz) * b + sample                                       # the reference's key: x-major, the sample last
    order = ranks.argsort()
    x, ranks = x[order].cumsum(0), ranks[order]                                                 # a running total over ALL kept points
    ends = torch.cat((ranks[1:] != ranks[:-1], torch.ones(1, device=x.device, dtype=torch.bool)))
    x, at = x[ends], order[ends]
    x = torch.cat((x[:1], x[1:] - x[:-1]))                                                      # differences at the segment ends
    final = torch.zeros((b, c, int(nx[2]), int(nx[1]), int(nx[0])), device=x.device)
    final[sample[at], :, iz[at], iy[at], ix[at]] = x
    return torch.cat(final.unbind(dim=2), 1)


def windows(call, n_windows, sync):
    for _ in range(3):
        call()
    sync()
    t0 = time.perf_counter()
    call()
    sync()
    reps = max(3, int(0.25 / max(time.perf_counter() - t0, 1e-6)) + 1)
    win = []
    for _ in range(n_windows):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        win.append((time.perf_counter() - t0) / reps)
    med = statistics.median(win)
    return {"median_us": round(med * 1e6, 2), "spread_us": round((max(win) - min(win)) * 1e6, 2), "windows_us": [round(v * 1e6, 2) for v in win],
            "calls_per_window": reps}


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def kernel_stats(directory):
    """{short name: {kernel, calls, avg_us, min_us, max_us}} of the stage's seven kernels, and the plan's sort as the sum over hipCUB's own
    kernels per plan, from a rocprofv3 --kernel-trace --stats output directory (its rocpd database, or its kernel_stats csv)"""
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
            raise SystemExit(f"bench_lift_splat: {len(hit)} rows for {name} under {directory}")
        _, calls, avg, mn, mx = hit[0]
        out[short] = {"kernel": name, "calls": int(calls), "avg_us": round(avg / 1e3, 2), "min_us": round(mn / 1e3, 2), "max_us": round(mx / 1e3, 2)}
    sort = [r for r in rows if "rocprim" in r[0] or "hipcub" in r[0]]
    if not sort:
        raise SystemExit(f"bench_lift_splat: no sort kernels under {directory}")
    out["plan_sort"] = {"kernel": "hipcub::DeviceRadixSort::SortPairs (all of its kernels)", "kernels": sorted({(re.search(r"wrapped_(\w+?)_config", r[0]) or re.search(r"(\w+)\s*[<(]", r[0].split("detail::")[-1])
                                           or re.search(r"(.{1,60})", r[0])).group(1) for r in sort}),
                        "launches": int(sum(r[1] for r in sort)), "avg_us": round(sum(r[1] * r[2] for r in sort) / KERNEL_RUN_CALLS / 1e3, 2)}
    return out


def measure(agents, n_windows):
    import numpy as np
    import torch
    from quantv2x_amd import lift_splat as ls
    from quantv2x_amd.engine import capture_call
    m = rig(agents)
    stage = ls.GpuLiftSplat(GRID, FINAL_DIM, DOWNSAMPLE, FEATURES, VIEWS, agents)
    mats = [torch.tensor(m[k]).cuda() for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    g = torch.Generator(device="cuda").manual_seed(agents)
    v = agents * VIEWS
    depth = torch.randn((v, stage.depth_bins, stage.fh, stage.fw), device="cuda", generator=g) * 2
    feats = torch.randn((v, FEATURES, stage.fh, stage.fw), device="cuda", generator=g)
    stage.plan(*mats)
    cells = stage.cells.cpu().numpy()
    kept = int((cells >= 0).sum())
    ncell = int(stage.nx.prod())
    flat = cells.reshape(agents, -1)
    per_cell = np.bincount((flat + np.arange(agents)[:, None] * ncell)[flat >= 0])
    sync = torch.cuda.synchronize
    t_plan = windows(capture_call(lambda: stage.plan(*mats)), n_windows, sync)
    t_splat = windows(capture_call(lambda: stage(depth, feats)), n_windows, sync)
    t_both = windows(capture_call(lambda: stage.plan(*mats)(depth, feats)), n_windows, sync)
    fused = stage(depth, feats).clone()
    # the torch form, on the geometry statement's f32 geometry (the plan's own geometry, to the bit)
    geom = torch.tensor(ls.geometry_statement(stage.frustum, *(m[k] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")))).cuda()
    dx, bx, nx = stage.dx.cuda(), stage.bx.cuda(), stage.nx.cuda()
    t_torch = windows(lambda: torch_form(geom, depth, feats, dx, bx, nx), n_windows, sync)
    ref = torch_form(geom, depth, feats, dx, bx, nx)
    diff_forms = float((fused - ref).abs().max())
    same_cells = bool(torch.equal((fused != 0).any(1), (ref != 0).any(1)))
    points, out_bytes = cells.size, fused.numel() * 4
    in_bytes = depth.numel() * 4 + feats.numel() * 4
    fused_floor = out_bytes + in_bytes
    product = points * FEATURES * 4
    kept_rows = kept * FEATURES * 4
    res = {"agents": agents, "points": points, "kept_points": kept, "occupied_cells": int((per_cell > 0).sum()), "largest_cell_points": int(per_cell.max()),
           "fused": {"plan": t_plan, "splat": t_splat, "plan_and_splat": t_both},
           "torch_form": dict(t_torch, what="eager torch on the same device and inputs, from the f32 geometry on (get_geometry is not in it)"),
           "torch_form_over_fused_splat": round(t_torch["median_us"] / t_splat["median_us"], 2),
           "torch_form_over_fused_plan_and_splat": round(t_torch["median_us"] / t_both["median_us"], 2),
           "outputs": {"largest_abs_difference_between_the_forms": diff_forms, "same_cells_occupied": same_cells,
                       "largest_abs_value": float(fused.abs().max())},
           "bytes_by_arithmetic": {
               "fused_floor": {"output_write": out_bytes, "depth_and_feats_read": in_bytes, "total": fused_floor},
               "fused_also_moves": {"probabilities_write_and_gather": 2 * points * 4, "transposed_feats_write": feats.numel() * 4,
                                    "plan_list_read": kept * 8 + agents * ncell * 8, "feature_rows_gathered_mostly_from_cache": kept_rows},
               "torch_form_at_least": {"product_write": product, "product_read_for_the_filter": product, "kept_rows_write": kept_rows,
                                       "sort_gather_read_and_write": 2 * kept_rows, "cumsum_read_and_write": 2 * kept_rows,
                                       "segment_ends_read": int((per_cell > 0).sum()) * FEATURES * 4 * 2, "output_clear_and_scatter": out_bytes,
                                       "total": 2 * product + 5 * kept_rows + out_bytes}},
           "fused_splat_floor_bytes_over_time_as_fraction_of_hbm_rate": round(fused_floor / (t_splat["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4)}
    if agents == 1:
        want, mag, count = ls.splat_terms_statement(cells, depth.cpu().numpy(), feats.cpu().numpy(), nx=stage.nx)
        bound = ls.splat_bound(count, mag, FEATURES, float(feats.abs().max()))
        d_f, d_t = np.abs(fused.cpu().numpy() - want), np.abs(ref.cpu().numpy() - want)
        res["outputs"].update({"fused_to_float64_statement": float(d_f.max()), "torch_form_to_float64_statement": float(d_t.max()),
                               "fused_largest_ratio_to_the_derived_bound": float((d_f[bound > 0] / bound[bound > 0]).max()),
                               "fused_within_the_derived_bound": bool((d_f <= bound).all())})
    del stage, geom, ref, fused
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_splat.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--git-head", default=None)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            result = json.load(fh)
        k = kernel_stats(args.kernel_stats)
        k["plan_sum_avg_us"] = round(sum(v["avg_us"] for n, v in k.items() if n.startswith("plan_")), 2)
        k["splat_sum_avg_us"] = round(sum(v["avg_us"] for n, v in k.items() if n.startswith("splat")), 2)
        k["source"] = (f"rocprofv3 --kernel-trace --stats over {KERNEL_RUN_CALLS} eager plans and splats at 1 agent, a run of its own: "
                       "rocprofv3 --kernel-trace --stats -d DIR -o lss -- python tools/bench_lift_splat.py --kernel-run, "
                       "then python tools/bench_lift_splat.py --kernel-stats DIR")
        result["kernels"] = k
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print(json.dumps(k))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lift_splat: no GPU -- nothing is measured on the CPU")
    if args.kernel_run:
        from quantv2x_amd import lift_splat as ls
        m = rig(1)
        stage = ls.GpuLiftSplat(GRID, FINAL_DIM, DOWNSAMPLE, FEATURES, VIEWS, 1)
        mats = [torch.tensor(m[k]).cuda() for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
        g = torch.Generator(device="cuda").manual_seed(1)
        depth = torch.randn((VIEWS, stage.depth_bins, stage.fh, stage.fw), device="cuda", generator=g) * 2
        feats = torch.randn((VIEWS, FEATURES, stage.fh, stage.fw), device="cuda", generator=g)
        for _ in range(KERNEL_RUN_CALLS):
            stage.plan(*mats)(depth, feats)
        torch.cuda.synchronize()
        return
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "workload": {"cameras_per_agent": VIEWS, "depth_bins": 48, "feature_map": [48, 64], "features": FEATURES, "grid": [256, 256, 1],
                           "grid_conf": GRID, "logits": "normal, sigma 2", "feats": "normal"},
              "method": "fused form: HIP graph replays, median of the windows' time per replay and the spread (highest minus lowest window); "
                        "torch form: eager calls, the same windows.  hbm fraction = (output + depth + feats bytes) / splat time / 8.0e12 B/s.",
              "checklist": CHECKLIST, "runs": [measure(a, args.windows) for a in args.agents]}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for r in result["runs"]:
        print(json.dumps({"agents": r["agents"], "plan_us": r["fused"]["plan"]["median_us"], "splat_us": r["fused"]["splat"]["median_us"],
                          "both_us": r["fused"]["plan_and_splat"]["median_us"], "torch_us": r["torch_form"]["median_us"], "outputs": r["outputs"],
                          "hbm_fraction": r["fused_splat_floor_bytes_over_time_as_fraction_of_hbm_rate"]}))
    bad = [r["agents"] for r in result["runs"] if not r["outputs"]["same_cells_occupied"] or not r["outputs"].get("fused_within_the_derived_bound", True)]
    if bad:
        raise SystemExit(f"bench_lift_splat: outputs differ at agents {bad}")


if __name__ == "__main__":
    main()
