"""The MSE range search at the sizes a calibration runs: ``qv2x_range_search_f32`` on one per-tensor activation of the V2X-Real shape
([4, 64, 200, 704], post-ReLU and signed) and one per-channel weight ([256, 2304]), 8 bits, the reference's full grid of 100 widths x 256
zero points = 25 600 candidates.  HIP events around whole ``gpu_range_search`` calls (table, kernel, pick), median of five windows and
their spread.  The torch loop (``UniformAffineQuantizer.perform_2D_search``) is timed on the same tensors at ``num = 1`` -- 256 candidates --
ONLY: walking its full grid takes minutes.  Both figures are printed per candidate, with their ratio; nothing is extrapolated to a total.
Also recorded: the kernel's losses against the float64 statement on the five searches of tests/golden/uaq_units.npz (the bound of
tests/test_hip_range_search.py is 4 x this figure), agreement of the two backends at ``num = 1``, and the wall time of a full-grid
calibration of the tiny model.  Writes profiles/range_search.json.

    python tools/bench_range_search.py [--out FILE] [--windows 5] [--git-head REV]

The kernel is bound by VALU issue (per evaluation about 14 plain vector instructions, v_log_f32 and v_exp_f32, one f32->f64 conversion and
one fp64 add; operands come from registers and one LDS broadcast read per four evaluations).  The memory and LDS traffic the shapes imply
is recorded next to the times; no roofline fraction is claimed.  No GPU: an error, not a fallback."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACT_SHAPE, WEIGHT_SHAPE, N_BITS, NUM = (4, 64, 200, 704), (256, 2304), 8, 100
TILE = 256                  # candidates per workgroup (csrc/range_search.hip)
CHECKLIST = [
    "timed on the MI355X only (no GPU: the tool fails)",
    "HIP events around whole gpu_range_search calls (candidate table + two kernels + the pick of lo / hi), event pair closed by a synchronise",
    "every timed shape warmed up by one untimed call (code objects, the cached workspace, torch's allocator)",
    "windows of at least 0.25 s of GPU work, five of them; the spread (highest minus lowest window) next to the median",
    "sizes a user runs: the V2X-Real activation shape and a 256-channel 3x3 weight, 8 bits, the reference's grid of 25 600 candidates",
    "the torch loop timed at num = 1 (256 candidates) only and reported per candidate -- never multiplied up to a total",
    "the kernel's choice compared with the torch loop's at num = 1 on every timed tensor; the losses compared with the float64 statement on the fixture",
    "no profiler attached to the timed run",
]


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def timed_windows(call, windows):
    """median / spread of the time per call over ``windows`` windows of >= 0.25 s, HIP events"""
    import torch
    call()                                                              # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); call(); b.record(); b.synchronize()
    reps = max(1, int(250.0 / max(a.elapsed_time(b), 1e-3)) + 1)
    win = []
    for _ in range(windows):
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        win.append(a.elapsed_time(b) / reps)
    return {"median_ms": round(statistics.median(win), 4), "spread_ms": round(max(win) - min(win), 4), "windows_ms": [round(w, 4) for w in win],
            "calls_per_window": reps}


def agreement_at_num_1(x, channel_wise, q):
    """the timed tensor at num = 1 (256 candidates), judged by the float64 statement: is the kernel's choice the statement's, and how does
    the range the torch loop returns ON THE GPU rate against it.  (On the GPU torch divides by ``num`` and ``2^n - 1`` through a reciprocal:
    the loop there walks floats next to the table's, so its range is usually a neighbour of the kernel's, not the same bits.)"""
    import torch
    from quantv2x_amd.calibration import _qparams, candidate_table, gpu_range_search, range_search_statement
    x2 = (torch.flatten(x, 1) if channel_wise else x.reshape(1, -1)).contiguous()
    _, _, delta, zp = candidate_table(x, N_BITS, channel_wise, "2d", 1)
    want, want_best = range_search_statement(x2, delta, zp, 2 ** N_BITS)
    lo_g, hi_g, _, best = gpu_range_search(x, N_BITS, channel_wise, "2d", 1, return_losses=True)
    lo_t, hi_t = q.perform_2D_search(x)
    d_t, z_t = _qparams(lo_t.reshape(1, -1), hi_t.reshape(1, -1), 2 ** N_BITS)
    loop_loss, _ = range_search_statement(x2, d_t, z_t, 2 ** N_BITS)
    ratio = want.gather(0, best.reshape(1, -1).to(want.device)) / loop_loss
    return {"rows": int(best.numel()), "rows_where_the_kernel_picks_the_statements_candidate": int((best.cpu() == want_best).sum()),
            "rows_where_the_gpu_torch_loop_returns_the_same_bits": int(((lo_t == lo_g) & (hi_t == hi_g)).sum()),
            "statement_loss_of_the_kernels_range_over_the_loops": {"lowest": float(ratio.min()), "highest": float(ratio.max())}}


def search_case(name, x, channel_wise, windows):
    import torch
    from quantv2x_amd.calibration import gpu_range_search
    from quantv2x_amd.plugin.quant import UniformAffineQuantizer
    rows = x.shape[0] if channel_wise else 1
    per_row = x.numel() // rows
    cands = NUM * 2 ** N_BITS
    evals = x.numel() * cands
    gpu = timed_windows(lambda: gpu_range_search(x, N_BITS, channel_wise, "2d", NUM), windows)
    q = UniformAffineQuantizer(n_bits=N_BITS, channel_wise=channel_wise, scale_method="mse")
    q.num = 1
    loop = timed_windows(lambda: q.perform_2D_search(x), windows)
    agreement = agreement_at_num_1(x, channel_wise, q)
    gpu_us_per_cand, loop_us_per_cand = gpu["median_ms"] * 1e3 / cands, loop["median_ms"] * 1e3 / 2 ** N_BITS
    tiles = -(-cands // TILE)
    out = {"shape": list(x.shape), "channel_wise": channel_wise, "rows": rows, "elements_per_row": per_row, "candidates": cands,
           "evaluations": evals,
           "hip": dict(gpu, us_per_candidate=round(gpu_us_per_cand, 4), evaluations_per_s=round(evals / (gpu["median_ms"] * 1e-3), 1)),
           "torch_loop_num_1": dict(loop, candidates=2 ** N_BITS, us_per_candidate=round(loop_us_per_cand, 3),
                                    evaluations_per_s=round(x.numel() * 2 ** N_BITS / (loop["median_ms"] * 1e-3), 1)),
           "torch_over_hip_per_candidate": round(loop_us_per_cand / gpu_us_per_cand, 1),
           "agreement_at_num_1": agreement,
           "traffic_from_shapes": {"what": "every candidate tile of 256 reads its row once from HBM / L2; a wave reads one 16-byte LDS broadcast per four evaluations",
                                   "global_read_bytes": x.numel() * 4 * tiles,
                                   "global_read_GB_per_s": round(x.numel() * 4 * tiles / (gpu["median_ms"] * 1e-3) / 1e9, 2)}}
    print(f"{name}: hip {gpu['median_ms']:.3f} ms for {cands} candidates = {gpu_us_per_cand:.4f} us per candidate "
          f"({out['hip']['evaluations_per_s']:.3e} evaluations/s); torch loop at num = 1: {loop['median_ms']:.3f} ms for 256 candidates = "
          f"{loop_us_per_cand:.3f} us per candidate; ratio per candidate {out['torch_over_hip_per_candidate']}", flush=True)
    return out


def loss_accuracy():
    """largest relative deviation of the kernel's losses from the float64 statement, over every candidate of the five pinned searches"""
    import numpy as np
    import torch
    from quantv2x_amd.calibration import candidate_table, range_search_statement, run_range_search
    g = np.load(os.path.join(ROOT, "tests", "golden", "uaq_units.npz"), allow_pickle=False)
    per, losses = {}, 0
    for tname, (cw, mode) in {"conv": (True, "2d"), "deconv": (True, "2d"), "linear": (True, "2d"), "act_pos": (False, "pos"),
                              "act_signed": (False, "2d")}.items():
        x, n_bits = torch.from_numpy(g["in/" + tname]), int(g[tname + "/mse/n_bits"])
        x2 = (torch.flatten(x, 1) if cw else x.reshape(1, -1)).contiguous()
        _, _, delta, zp = candidate_table(x, n_bits, cw, mode)
        want, want_best = range_search_statement(x2, delta, zp, 2 ** n_bits)
        got, best = run_range_search(x2.cuda(), delta.cuda(), zp.cuda(), 2 ** n_bits)
        per[tname] = {"largest_relative_deviation": float(((got.cpu() - want).abs() / want).max()), "losses": want.numel(),
                      "same_choice_as_statement": bool(torch.equal(best.cpu().long(), want_best))}
        losses += want.numel()
    return {"largest_relative_deviation": max(v["largest_relative_deviation"] for v in per.values()), "losses": losses, "per_search": per,
            "reference": "quantv2x_amd.calibration.range_search_statement (float64) on tests/golden/uaq_units.npz"}


def tiny_model_full_grid():
    """wall time of set_weight_quantize_params + one calibration scene of the tiny model with search_backend='hip' and num = 100"""
    import torch
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.quant import QuantModel, UniformAffineQuantizer, set_weight_quantize_params
    from quantv2x_amd.plugin.tools import train_utils
    from quantv2x_amd.plugin.tools.inference_quant import calibrate_minmax, quant_params
    model = train_utils.create_model(copy.deepcopy(synth.make_hypes("tiny"))).eval()
    synth.load_state_dict_numpy(model, synth.make_state_dict(model.state_dict(), seed=1))
    sc = synth.scene_to_torch(synth.make_scene("tiny", n_agents=2, seed=3, n_points=3000), "cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wq, aq = quant_params(scale_method="mse", search_backend="hip")
    qt = QuantModel(model, wq, aq).eval().cuda()
    set_weight_quantize_params(qt)
    calibrate_minmax(qt, [sc])
    torch.cuda.synchronize()
    return {"what": "QuantModel wrap, set_weight_quantize_params and one calibration scene of two agents on the tiny model, scale_method 'mse', "
                    "search_backend 'hip', num = 100; host clock closed by a synchronise, first call of every shape included",
            "quantizers": sum(isinstance(m, UniformAffineQuantizer) for m in qt.modules()), "wall_s": round(time.perf_counter() - t0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_search.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--git-head", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_range_search: no GPU -- nothing is measured on the CPU")
    g = torch.Generator(device="cuda").manual_seed(11)
    signed = torch.randn(ACT_SHAPE, device="cuda", generator=g) * 0.8 + 0.2
    weight = torch.randn(WEIGHT_SHAPE, device="cuda", generator=g) * (0.02 + 0.08 * torch.rand(WEIGHT_SHAPE[0], 1, device="cuda", generator=g))
    result = {"git_head": args.git_head or git_head(), "device": torch.cuda.get_device_name(0),
              "method": "gpu_range_search (vectorised candidate table + qv2x_range_search_f32 + the pick) under HIP events; median of the windows' "
                        "time per call and the spread (highest minus lowest window).  The torch loop is perform_2D_search at num = 1 on the "
                        "same tensor, per candidate; the ratio is per candidate and is not a measured total.",
              "bound_by": "VALU issue: about 14 plain vector instructions, v_log_f32 + v_exp_f32, one conversion and one fp64 add per evaluation, "
                          "operands in registers; traffic_from_shapes shows how little memory bandwidth the call needs.  No roofline fraction is claimed.",
              "checklist": CHECKLIST,
              "loss_accuracy": loss_accuracy(),
              "searches": {"act_signed": search_case("act_signed", signed, False, args.windows),
                           "act_post_relu": search_case("act_post_relu", torch.relu(signed), False, args.windows),
                           "weight_per_channel": search_case("weight_per_channel", weight, True, args.windows)},
              "tiny_model_full_grid": tiny_model_full_grid()}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"loss_accuracy": result["loss_accuracy"]["largest_relative_deviation"], "tiny_model_full_grid": result["tiny_model_full_grid"],
                      **{k: {"hip_ms": v["hip"]["median_ms"], "ratio_per_candidate": v["torch_over_hip_per_candidate"]} for k, v in result["searches"].items()}}))


if __name__ == "__main__":
    main()
