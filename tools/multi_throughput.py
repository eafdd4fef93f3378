"""What several starts per instance cost and buy on the MI355X (mpcb_solve_multi_device): C2 (kin N=30, one static obstacle) and C3 (kin,
three predicted obstacles), B = 4096 instances each, cold starts.  Variants, alternating inside one run over rounds so that clock and
thermal drift hit all alike:
  cold     the plain mpcb_solve_device without a start vector (the turned cold start and second_start = 3 act), one launch at a time
  multi1   mpcb_solve_multi_device with K = 1, controls (0, 0)
  multi3   K = 3, turn_starts(3)
  multi5   K = 5, turn_starts(5)
Every variant runs on ONE handle with one launch lane: the multi-start call waits for the lanes and runs on the handle's own stream, so
lanes would only help the cold variant.  Timed with a host clock around a final synchronise, after a warm-up; instances/s counts the
caller's instances (B per call), not the K * B candidates.  Per variant: the rate, the share of instances solved (SOLVED or ACCEPTABLE
with a finite objective), the share won by another candidate than 0, the share with two or more distinct solutions among the
candidates, the share whose objective is lower than the cold solve's by more than 1e-6 relative (of the instances both solve), the
instances only this variant / only the cold solve solves, and the mean iterations per candidate and per instance.
The share of the call spent in the two glue kernels comes from ONE separate run under `rocprofv3 --kernel-trace --stats` with nothing
else traced (--profile starts it as a child process).
    python tools/multi_throughput.py [--configs C2,C3] [--batch 4096] [--steps 8] [--warmup 2] [--rounds 5] [--profile] [--out profiles/multi_start.txt]
Every number in the output file is measured by the run that writes it."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_motion_planning_amd import scenes, _abi   # noqa: E402
from mpc_motion_planning_amd.solver import BatchSolver, default_config, turn_starts   # noqa: E402

VARIANTS = (("cold", 0), ("multi1", 1), ("multi3", 3), ("multi5", 5))


def workload(conf, B):
    if conf == "C2":
        return (default_config(model=_abi.MODEL_KIN, N=30, T=0.1, n_obs=1),) + tuple(scenes.sample_c2(B, seed=0)) + (_abi.OBSIN_STATIC,)
    a0, a1, _, a3 = scenes.sample_c3(B, N=30, dt=0.1, seed=100)
    return default_config(model=_abi.MODEL_KIN, N=30, T=0.1, n_obs=3), a0, a1, a3, _abi.OBSIN_PREDICTED


def run_config(conf, args, say):
    B = args.batch
    cfg, x0, xs, obs, kind = workload(conf, B)
    bs = BatchSolver(cfg)
    d = {k: bs.device_array(a.shape).upload(a) for k, a in (("x0", x0), ("xs", xs), ("obs", obs))}
    o = dict(z=bs.device_array((B, bs.nz)), obj=bs.device_array((B,)), st=bs.device_array((B,), np.int32), it=bs.device_array((B,), np.int32),
             which=bs.device_array((B,), np.int32), n_ok=bs.device_array((B,), np.int32), n_basins=bs.device_array((B,), np.int32),
             it_all=bs.device_array((B, 5), np.int32))

    def run(K, n):
        for _ in range(n):
            if K == 0:
                bs.solve_device(B, d["x0"], d["xs"], d["obs"], kind, None, o["z"], d_obj=o["obj"], d_status=o["st"], d_iters=o["it"])
            else:
                bs.solve_multi_device(B, d["x0"], d["xs"], d["obs"], kind, None, o["z"], controls=turn_starts(K), d_obj=o["obj"], d_status=o["st"],
                                      d_iters=o["it"], d_which=o["which"], d_n_ok=o["n_ok"], d_n_basins=o["n_basins"], d_iters_all=o["it_all"])
        bs.sync()

    if args.child:                       # the profiled run: the K = 3 call a few times, nothing else
        run(3, args.warmup + 4)
        return None
    rate = {name: [] for name, _ in VARIANTS}
    res = {}
    for r in range(args.rounds):
        for name, K in VARIANTS:
            run(K, args.warmup)
            t0 = time.perf_counter()
            run(K, args.steps)
            rate[name].append(B * args.steps / (time.perf_counter() - t0))
            say("%s round %d %-6s %10.0f instances/s" % (conf, r, name, rate[name][-1]))
            if r == 0:
                res[name] = dict(obj=o["obj"].download(), st=o["st"].download(), it=o["it"].download(), which=o["which"].download(),
                                 n_basins=o["n_basins"].download(), it_all=o["it_all"].download().ravel()[:B * max(K, 1)].reshape(B, max(K, 1)))      # the call wrote [B, K] into the [B, 5] buffer
    ok = lambda q: ((q["st"] == _abi.ST_SOLVED) | (q["st"] == _abi.ST_ACCEPTABLE)) & np.isfinite(q["obj"])      # noqa: E731
    cold, cold_ok = res["cold"], ok(res["cold"])
    out = dict(config=conf, batch=B, steps=args.steps, rounds=args.rounds, variants={})
    for name, K in VARIANTS:
        q = res[name]; q_ok = ok(q); both = q_ok & cold_ok
        v = dict(K=K, median_instances_per_s=float(np.median(rate[name])), spread_over_rounds=float((max(rate[name]) - min(rate[name])) / np.median(rate[name])),
                 share_solved=float(q_ok.mean()))
        if K:
            v.update(share_which_not_0=float((q["which"][q_ok] != 0).mean()), share_two_or_more_solutions=float((q["n_basins"] >= 2).mean()),
                     share_lower_than_cold_by_1e6=float((q["obj"][both] < cold["obj"][both] - 1e-6 * np.maximum(1.0, np.abs(cold["obj"][both]))).mean()),
                     share_higher_than_cold_by_1e6=float((q["obj"][both] > cold["obj"][both] + 1e-6 * np.maximum(1.0, np.abs(cold["obj"][both]))).mean()),
                     solved_only_here=int((q_ok & ~cold_ok).sum()), solved_only_cold=int((cold_ok & ~q_ok).sum()),
                     mean_iterations_per_candidate=float(q["it_all"].mean()), mean_iterations_per_instance=float(q["it_all"].sum(axis=1).mean()))
            v["rate_over_cold"] = v["median_instances_per_s"] / float(np.median(rate["cold"]))
        else:
            v.update(mean_iterations_per_instance=float(q["it"].mean()))
        out["variants"][name] = v
    bs.close()
    return out


def profile(conf, args):
    """Share of the GPU time of the K = 3 call spent in mpcb_multi_expand and mpcb_multi_select, from one child run under
    rocprofv3 --kernel-trace --stats; or None with the reason."""
    tmp = tempfile.mkdtemp(prefix="mpcb_multi_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--configs", conf, "--child", "--warmup", str(args.warmup), "--batch", str(args.batch)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired) as e:
        return None, "rocprofv3 did not run: %r" % (e,)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not files:
        return None, "rocprofv3 exit %d, no kernel_stats.csv: %s" % (p.returncode, (p.stderr or p.stdout)[-300:])
    total, rows = 0.0, {}
    for r in csv.DictReader(open(files[0])):
        ns = int(r["Calls"]) * float(r["AverageNs"])
        total += ns
        for key in ("mpcb_multi_expand", "mpcb_multi_select"):
            if key in r.get("Name", ""):
                rows[key] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, total_us=ns / 1e3)
    if len(rows) != 2 or total <= 0:
        return None, "rows of the two kernels not found in %s" % files[0]
    return dict(kernels=rows, all_kernels_total_us=total / 1e3, share_of_gpu_time=sum(v["total_us"] for v in rows.values()) / (total / 1e3)), None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="one more run per configuration as a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_start.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not args.child:
        say("# tools/multi_throughput.py on one MI355X: every number below is measured by this run on the GPU (no CPU or oracle figure)")
        say("# batch %d, steps %d, warmup %d, rounds %d, one handle, one launch lane; GPU_MAX_HW_QUEUES = %s" % (
            args.batch, args.steps, args.warmup, args.rounds, os.environ.get("GPU_MAX_HW_QUEUES")))
    for conf in args.configs.split(","):
        out = run_config(conf, args, say)
        if out is None:
            continue
        if args.profile:
            k, why = profile(conf, args)
            out["glue_kernels_K3"] = k if k else "not measured: " + why
        else:
            out["glue_kernels_K3"] = "not measured (run with --profile)"
        say(json.dumps(out))
    if not args.child:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
