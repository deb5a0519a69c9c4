"""Rank 0's step of the ``ego_only`` N-GPU line with the post stage unsharded (today's ``ego_only``) and sharded in row bands
(``AgentShardedModel(ego_only=True, shard_post=True)``, both band wires), rehearsed on ONE GPU.
    python tools/bench_band_post.py [--worlds 2,4,8] [--frames 32] [--steps 30] [--repeats 5] [--out profiles/r07_band_post.json]
For every W: the workload ``bench.workload_for(W)`` names, ``--frames`` frames per step, ``emulate_world=W`` -- the own payload (and the own
band slab) copied into every slot where the all-gathers would be, so this times the KERNELS of a rank's step, not the link: the cost of the
second all-gather (the slab bytes are printed beside the times) is NOT measured; no multi-GPU node has been available.
The arms alternate inside one process: ``--repeats`` rounds of (warm-up, ``--steps`` timed steps ending in a device synchronise) per arm,
each window a fraction of a second or more; median, lowest and highest ms per step are kept, the spread is highest - lowest.  Stage times
are HIP events around replays of the captured graphs.  The one-GPU same-scene denominators of the ego-only scaling ratio are measured in the
same process by ``bench.same_scene_one_gpu`` (the function behind ``multi_agent_one_gpu.same_scene_b32`` of a ``bench.py --full`` line).
Prints one JSON record (and writes it to ``--out``)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from quantv2x_amd.dist import AgentShardedModel, band_payload_layout, band_rows
    if not torch.cuda.is_available():
        raise SystemExit("bench_band_post.py measures on the GPU: none found")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B = args.frames
    engines, record = {}, {"metric": "rank 0's step of the ego_only N-GPU line, post stage unsharded vs sharded in row bands (one-GPU rehearsal)",
                           "frames_per_step": B, "steps_per_window": args.steps, "warmup_steps": args.warmup, "repeats": args.repeats,
                           "link": "NOT measured: both all-gathers are device copies of the own payload / slab (one GPU)", "worlds": {}}
    for W in [int(v) for v in args.worlds.split(",")]:
        wl = bench.workload_for(W)
        keep = (bench.SHAPE, bench.N_POINTS)
        bench.SHAPE, bench.N_POINTS = wl["shape"], wl["n_points"]
        try:
            key = (wl["shape"], wl["multiclass"])
            if key not in engines:
                engines[key] = bench.build_engine(max(1, min(32, os.cpu_count() or 8)), multiclass=wl["multiclass"])[1]
            eng = engines[key]
            _, _, mine, poses = bench.frame_batch(W, 0, B, device, layout=wl["layout"], max_cav=wl["max_cav"], own_only=True)
        finally:
            bench.SHAPE, bench.N_POINTS = keep
        pose_t = torch.from_numpy(np.stack(poses)).to(device)
        kw = dict(frames=B, max_cav=wl["max_cav"], emulate_world=W, emulate_poses=pose_t, emulate_rank=0, ego_only=True)
        arms = {"unsharded": AgentShardedModel(eng, **kw)}
        for wire in ("f32", "u8"):
            if eng.head_wire_supported(wire):
                arms["banded_" + wire] = AgentShardedModel(eng, shard_post=True, band_wire=wire, **kw)
        for sh in arms.values():                                        # capture (each arm its own graphs on the one engine)
            sh.forward(mine, pose_t[0])
        torch.cuda.synchronize()
        ms = {name: [] for name in arms}
        for _ in range(args.repeats):                                   # the arms alternate: drift of the box hits them alike
            for name, sh in arms.items():
                for _ in range(args.warmup):
                    sh.forward(mine, pose_t[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    sh.forward(mine, pose_t[0])
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        cout, h, w = eng.band_shape()
        res = {"workload": wl["workload"], "baseline_config_index": wl["index"], "feature_map": [h, w], "head_channels": cout,
               "band_rows_of_rank0": list(band_rows(h, W, 0)), "arms": {}}
        for name, sh in arms.items():
            graphs = sh.stage_graphs()
            stages = dict(zip(("pre_a1_to_a6", "band_a7_to_a11", "assemble") if sh.shard_post else ("pre_a1_to_a6", "post_a7_to_a11"),
                              [round(bench.event_time_us(g.replay, 10), 1) for g in graphs]))
            v = ms[name]
            res["arms"][name] = {"ms_per_step_median": round(statistics.median(v), 4), "ms_per_step_min": round(min(v), 4),
                                 "ms_per_step_max": round(max(v), 4), "spread_ms": round(max(v) - min(v), 4), "ms_per_step_repeats": [round(x, 4) for x in v],
                                 "stage_us": stages, "free_link_frames_per_s": round(B / statistics.median(v) * 1e3, 1)}
            if sh.shard_post:
                res["arms"][name]["slab_bytes_per_rank_per_step"] = band_payload_layout(B, cout, h, w, W, sh.band_wire)[1]
        # both kernel forms of the band at this shape (the selector's rule is the whole-map call's: one launch up to four agents)
        forms = {}
        for label, force in (("one_launch", True), ("fused_rows_then_heads", False)):
            eng.band_one_launch = force
            try:
                sh = AgentShardedModel(eng, shard_post=True, band_wire="f32", **kw)
                sh.forward(mine, pose_t[0])
                forms[label] = round(bench.event_time_us(sh.stage_graphs()[1].replay, 10), 1)
                del sh
            finally:
                eng.band_one_launch = None
        res["band_forms_us_f32"] = forms
        un = res["arms"]["unsharded"]
        for name, a in res["arms"].items():
            if name != "unsharded":
                gain = un["ms_per_step_median"] - a["ms_per_step_median"]
                a["shorter_than_unsharded_ms"] = round(gain, 4)
                a["beyond_spread"] = bool(un["ms_per_step_min"] - a["ms_per_step_max"] > 0)    # every repeat of one arm below every repeat of the other
        del arms
        try:
            scenes = bench.same_scene_scenes(W, B)
            same = bench.same_scene_one_gpu(eng, W, device, scenes)
            res["one_gpu_same_scene"] = same
            for name, a in res["arms"].items():
                a["ego_only_ratio_vs_one_gpu_free_link"] = round(a["free_link_frames_per_s"] / same["fused_frames_per_s"], 3)
        except Exception as e:                                          # (the denominators must not cost the record)
            res["one_gpu_same_scene"] = {"error": repr(e)[:300]}
        record["worlds"][str(W)] = res
        torch.cuda.empty_cache()
    line = json.dumps(record)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
