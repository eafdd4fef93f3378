"""Cost of certifying every instance of every launch (mpcb_evaluate_device) on the MI355X: C2 (kin N=30, one static obstacle, B = 4096),
C3 (kin, three predicted obstacles, B = 32768) and C4 (dyn N=40, three obstacles, B = 8192), cold starts, ONE handle with sixteen launch
lanes as bench.py runs them.  Per configuration, alternating in rounds so that clock and thermal drift hit both alike:
  (a) solve  mpcb_solve_device alone (with multipliers: the evaluation needs them, and both variants run the same solve)
  (b) pair   the same solve followed by mpcb_evaluate_device with multipliers, g and res, on rotated buffers
Timed with a host clock around a final synchronise, after a warm-up.  The figure is pair / solve (rates) of the same run, beside that
run's own spread of the solve-alone rate.  The evaluation kernel's own time comes from ONE separate run of this script under
`rocprofv3 --kernel-trace --stats` with nothing else traced (--profile starts it as a child process), and is set against the kernel's
compulsory bytes (it reads z, lam_x, lam_g and the scene, writes g and res) over the HBM peak of MI355X_MICROARCH.md (8.0 TB/s spec,
6.29 TB/s measured with a float4 copy).
    python tools/evaluate_throughput.py [--configs C2,C3,C4] [--steps 32] [--warmup 4] [--rounds 5] [--inflight 16] [--profile]
Prints one line per round, configuration and variant, then a JSON summary line per configuration."""
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

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # as bench.py: sixteen lanes want sixteen hardware queues (before the HIP runtime loads); a value the environment sets stands, and the output's first line records it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_motion_planning_amd import scenes, _abi   # noqa: E402
from mpc_motion_planning_amd.solver import BatchSolver, default_config   # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12        # bytes/s: spec peak and the measured float4 copy (MI355X_MICROARCH.md)
BATCH = dict(C2=4096, C3=32768, C4=8192)


def workload(conf, B):
    """(cfg, x0, xs, obs, obs_kind) as bench.py draws the configuration's first batch."""
    if conf == "C2":
        return (default_config(model=_abi.MODEL_KIN, N=30, T=0.1, n_obs=1),) + tuple(scenes.sample_c2(B, seed=0)) + (_abi.OBSIN_STATIC,)
    if conf == "C3":
        a0, a1, _, a3 = scenes.sample_c3(B, N=30, dt=0.1, seed=100)
        return default_config(model=_abi.MODEL_KIN, N=30, T=0.1, n_obs=3), a0, a1, a3, _abi.OBSIN_PREDICTED
    x0, xs, obs = scenes.sample_c4(B, seed=200, n_obs=3)
    return default_config(model=_abi.MODEL_DYN, N=40, T=0.1, n_obs=3), x0, xs, obs, _abi.OBSIN_STATIC


def compulsory_bytes(bs, B, obs):
    """What one evaluation with multipliers, g and res must move: z, lam_x, lam_g, x0, xs, the scene in; g, res, obj out."""
    return 8 * (B * (2 * bs.nz + bs.ng + 2 * bs.nx) + obs.size + B * (bs.ng + _abi.EVAL_COLS + 1))


def run_config(conf, args):
    B, K = args.batch or BATCH[conf], args.inflight
    cfg, x0, xs, obs, kind = workload(conf, B)
    bs = BatchSolver(cfg, inflight=K)
    d = {k: bs.device_array(a.shape).upload(a) for k, a in (("x0", x0), ("xs", xs), ("obs", obs))}
    outs = [dict(z=bs.device_array((B, bs.nz)), st=bs.device_array((B,), np.int32), it=bs.device_array((B,), np.int32),
                 lg=bs.device_array((B, bs.ng)), lx=bs.device_array((B, bs.nz)), obj=bs.device_array((B,)), g=bs.device_array((B, bs.ng)),
                 res=bs.device_array((B, _abi.EVAL_COLS))) for _ in range(K)]

    def run(pair, n):
        for s in range(n):
            o = outs[s % K]
            bs.solve_device(B, d["x0"], d["xs"], d["obs"], kind, None, o["z"], d_status=o["st"], d_iters=o["it"], d_lam_g=o["lg"], d_lam_x=o["lx"])
            if pair:
                bs.evaluate_device(B, d["x0"], d["xs"], d["obs"], kind, o["z"], o["lg"], o["lx"], d_obj=o["obj"], d_g=o["g"], d_res=o["res"])
        bs.sync()

    if args.child:                       # the profiled run: a few pairs, nothing else
        run(True, args.warmup + 4)
        return None
    rate = dict(solve=[], pair=[])
    for r in range(args.rounds):
        for name in ("solve", "pair"):
            run(name == "pair", args.warmup)
            t0 = time.perf_counter()
            run(name == "pair", args.steps)
            rate[name].append(B * args.steps / (time.perf_counter() - t0))
            print("%s round %d %-5s %10.0f instances/s" % (conf, r, name, rate[name][-1]), flush=True)
    st, res = outs[(args.steps - 1) % K]["st"].download(), outs[(args.steps - 1) % K]["res"].download()
    med = {k: float(np.median(v)) for k, v in rate.items()}
    spread = float((max(rate["solve"]) - min(rate["solve"])) / med["solve"])
    by = compulsory_bytes(bs, B, obs)
    out = dict(config=conf, batch=B, inflight=K, steps=args.steps, rounds=args.rounds, median_instances_per_s=med,
               solve_spread_over_rounds=spread, pair_spread_over_rounds=float((max(rate["pair"]) - min(rate["pair"])) / med["pair"]),
               pair_over_solve=med["pair"] / med["solve"], pair_within_solve_spread=bool(1.0 - med["pair"] / med["solve"] <= spread),
               solved=int((st == 0).sum()), solved_and_certified=int(((st == 0) & (res[:, 0] <= 1.01e-8) & (res[:, 5] == 0.0) & (res[:, 3] / res[:, 6] <= 1e-8) & (res[:, 4] <= 1e-4)).sum()),
               eval_compulsory_bytes=int(by), eval_us_at_hbm_spec=by / HBM_SPEC * 1e6, eval_us_at_hbm_copy=by / HBM_COPY * 1e6)
    bs.close()
    return out


def profile(conf, args):
    """The evaluation kernel's average time [us] from one child run under rocprofv3 --kernel-trace --stats, or None with the reason."""
    tmp = tempfile.mkdtemp(prefix="mpcb_eval_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--configs", conf, "--child", "--warmup", str(args.warmup), "--inflight", "1"]          # one launch at a time: a duration that no other launch shares
    cmd += ["--batch", str(args.batch)] if args.batch else []
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired) as e:
        return None, "rocprofv3 did not run: %r" % (e,)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not files:
        return None, "rocprofv3 exit %d, no kernel_stats.csv: %s" % (p.returncode, (p.stderr or p.stdout)[-300:])
    for r in csv.DictReader(open(files[0])):
        if "mpcb_eval" in r.get("Name", ""):
            return dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3), None
    return None, "no mpcb_eval row in %s" % files[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--batch", type=int, default=0, help="0 = the configuration's own batch (C2 4096, C3 32768, C4 8192)")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=16)
    ap.add_argument("--profile", action="store_true", help="one more run per configuration as a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if not args.child:                   # what the HIP runtime of this process was given: sixteen lanes share that many hardware queues
        print("# GPU_MAX_HW_QUEUES = %s in effect (16 is this script's default where the environment sets none), inflight %d, steps %d, rounds %d" % (
            os.environ.get("GPU_MAX_HW_QUEUES"), args.inflight, args.steps, args.rounds), flush=True)
    for conf in args.configs.split(","):
        out = run_config(conf, args)
        if out is None:
            continue
        if args.profile:
            k, why = profile(conf, args)
            if k:
                out["eval_kernel"] = k
                out["eval_kernel_over_hbm_spec_time"] = k["average_us"] / out["eval_us_at_hbm_spec"]
                out["eval_kernel_bytes_per_s"] = out["eval_compulsory_bytes"] / (k["average_us"] * 1e-6)
            else:
                out["eval_kernel"] = "not measured: " + why
        else:
            out["eval_kernel"] = "not measured (run with --profile)"
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
