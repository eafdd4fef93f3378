"""Cost of per-stage reference tracking: C2 (kin N=30, one static obstacle, B = 4096 cold starts) timed through mpcb_solve_device
(the set-point kernels) and through mpcb_solve_device_ref with x_ref rows equal to xs (the mpcb_track_* kernels) on ONE handle with
sixteen launch lanes, as bench.py runs C2.  Rows equal to xs make the two NLPs the same, so the iteration counts are equal and the
difference is the kernels' own.  The two variants alternate in rounds so that clock and thermal drift hit both alike.
    python tools/track_throughput.py [--batch 4096] [--steps 20] [--warmup 4] [--rounds 5] [--inflight 16]
Prints one line per round and variant, then a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_motion_planning_amd import scenes, _abi   # noqa: E402
from mpc_motion_planning_amd.solver import BatchSolver, default_config   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=16)
    args = ap.parse_args(argv)
    B, K = args.batch, args.inflight
    cfg = default_config(N=30, n_obs=1)
    bs = BatchSolver(cfg, inflight=K)
    x0, xs, obs = scenes.sample_c2(B, seed=0)
    xr = np.ascontiguousarray(np.repeat(xs[:, None, :], cfg.N, axis=1))
    d = {k: bs.device_array(a.shape).upload(a) for k, a in (("x0", x0), ("xs", xs), ("obs", obs), ("xr", xr))}
    outs = [dict(z=bs.device_array((B, bs.nz)), st=bs.device_array((B,), np.int32), it=bs.device_array((B,), np.int32)) for _ in range(K)]

    def run(track, n):
        for s in range(n):
            o = outs[s % K]
            bs.solve_device(B, d["x0"], d["xs"], d["obs"], _abi.OBSIN_STATIC, None, o["z"], d_status=o["st"], d_iters=o["it"],
                            d_x_ref=d["xr"] if track else None)
        bs.sync()

    res = {"set_point": [], "tracking": []}
    for r in range(args.rounds):
        for name, track in (("set_point", False), ("tracking", True)):
            run(track, args.warmup)
            bs.timing(reset=True)
            t0 = time.perf_counter()
            run(track, args.steps)
            dt = time.perf_counter() - t0
            tm = bs.timing()
            res[name].append(dict(solves_per_s=B * args.steps / dt, ms_per_solve_launch=tm["total_ms"] / max(1, tm["launches"])))
            print("round %d %-9s %10.0f solves/s  %.3f ms per launch (event pair, lanes overlap)" % (r, name, res[name][-1]["solves_per_s"],
                                                                                               res[name][-1]["ms_per_solve_launch"]))
    # the two variants solve the same NLPs: statuses and iterations must agree
    a = bs.solve_batch(x0, xs, obs); b = bs.solve_batch(x0, xs, obs, x_ref=xr)
    same = bool(np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"]))
    med = {k: float(np.median([v["solves_per_s"] for v in res[k]])) for k in res}
    summary = dict(batch=B, inflight=K, steps=args.steps, rounds=args.rounds, median_solves_per_s=med,
                   tracking_over_set_point=med["tracking"] / med["set_point"], same_status_and_iters=same,
                   mean_iters=float(a["iters"].mean()), solved=int((a["status"] == 0).sum()), bitwise_equal_z=bool(np.array_equal(a["z"], b["z"])))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
