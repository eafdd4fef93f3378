"""Cost of per-instance problem data: C2 (kin N=30, one static obstacle, B = 4096 cold starts) on ONE handle with sixteen launch lanes,
as bench.py runs C2, timed four ways:
  (a) plain        mpcb_solve_device: the mpcb_kernel_* kernels, the handle's config
  (b) uniform      mpcb_solve_device_params with 4096 rows equal to the handle's config: the same NLPs through the mpcb_param_* kernels, so
                   the iteration counts are equal and the difference is the kernels' own
  (c) mixed        mpcb_solve_device_params with the eight-config mix of tests/params_cases.py (row b = config b mod 8)
  (d) the workflow a parameter set replaces: 64 handles of 64 instances each, launched one after another (each on its own stream, one
      synchronisation at the end), against ONE mixed launch of the same 4096 instances under 64 configs
(a), (b), (c) alternate in rounds so that clock and thermal drift hit all alike; the median over the rounds is reported.
    python tools/params_throughput.py [--batch 4096] [--steps 20] [--warmup 4] [--rounds 5] [--inflight 16]
Prints one line per round and variant, then a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # as bench.py: sixteen lanes want sixteen hardware queues (before the HIP runtime loads)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_motion_planning_amd import scenes, _abi   # noqa: E402
from mpc_motion_planning_amd.solver import BatchSolver, default_config, vary   # noqa: E402
from tests import config_cases as cc   # noqa: E402
from tests.params_cases import KIN_MIX   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=16)
    ap.add_argument("--handles", type=int, default=64)
    args = ap.parse_args(argv)
    B, K = args.batch, args.inflight
    cfg = default_config(N=30, n_obs=1)
    bs = BatchSolver(cfg, inflight=K)
    x0, xs, obs = scenes.sample_c2(B, seed=0)
    mix_cfgs = [cc.base(cc.BY_NAME[n], default_config) for n in KIN_MIX]
    sets = dict(plain=None, uniform=bs.params(vary(cfg, B)), mixed=bs.params([mix_cfgs[b % len(mix_cfgs)] for b in range(B)]))
    d = {k: bs.device_array(a.shape).upload(a) for k, a in (("x0", x0), ("xs", xs), ("obs", obs))}
    outs = [dict(z=bs.device_array((B, bs.nz)), st=bs.device_array((B,), np.int32), it=bs.device_array((B,), np.int32)) for _ in range(K)]

    def run(ps, n):
        for s in range(n):
            o = outs[s % K]
            bs.solve_device(B, d["x0"], d["xs"], d["obs"], _abi.OBSIN_STATIC, None, o["z"], d_status=o["st"], d_iters=o["it"], params=ps)
        bs.sync()

    res = {k: [] for k in sets}
    for r in range(args.rounds):
        for name, ps in sets.items():
            run(ps, args.warmup)
            t0 = time.perf_counter()
            run(ps, args.steps)
            dt = time.perf_counter() - t0
            res[name].append(B * args.steps / dt)
            print("round %d %-8s %10.0f solves/s" % (r, name, res[name][-1]))
    a = bs.solve_batch(x0, xs, obs); b = bs.solve_batch(x0, xs, obs, params=sets["uniform"]); c = bs.solve_batch(x0, xs, obs, params=sets["mixed"])
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = float((max(res["plain"]) - min(res["plain"])) / med["plain"])

    # (d) a sweep of `handles` tunings (the Q_y weight swept over a decade), B / handles scenes each
    H = args.handles; n = B // H
    qy = np.geomspace(3e4, 3e5, H)
    sweep = []
    for k in range(H):
        c_k = cfg.copy(); c_k.Q[1] = qy[k]
        sweep.append(c_k)
    hs = [BatchSolver(c_k) for c_k in sweep]
    bufs = []
    for k, h in enumerate(hs):
        sl = slice(k * n, (k + 1) * n)
        bufs.append(dict(x0=h.device_array((n, 4)).upload(x0[sl]), xs=h.device_array((n, 4)).upload(xs[sl]), obs=h.device_array((n, 1, 6)).upload(obs[sl]),
                         z=h.device_array((n, h.nz)), st=h.device_array((n,), np.int32), it=h.device_array((n,), np.int32)))
    one = bs.params([sweep[b // n] for b in range(H * n)])
    dn = {k: bs.device_array(a[:H * n].shape).upload(a[:H * n]) for k, a in (("x0", x0), ("xs", xs), ("obs", obs))}
    on = dict(z=bs.device_array((H * n, bs.nz)), st=bs.device_array((H * n,), np.int32), it=bs.device_array((H * n,), np.int32))

    def many():
        for h, q in zip(hs, bufs):
            h.solve_device(n, q["x0"], q["xs"], q["obs"], _abi.OBSIN_STATIC, None, q["z"], d_status=q["st"], d_iters=q["it"])
        for h in hs:
            h.sync()

    def single():
        bs.solve_device(H * n, dn["x0"], dn["xs"], dn["obs"], _abi.OBSIN_STATIC, None, on["z"], d_status=on["st"], d_iters=on["it"], params=one)
        bs.sync()

    t_many, t_one = [], []
    for r in range(args.rounds):
        for fn, acc in ((many, t_many), (single, t_one)):
            fn()
            t0 = time.perf_counter()
            for _ in range(4):
                fn()
            acc.append((time.perf_counter() - t0) / 4 * 1e3)
        print("round %d  %d handles x %d: %.3f ms   one mixed launch: %.3f ms" % (r, H, n, t_many[-1], t_one[-1]))
    z_many = np.concatenate([q["z"].download() for q in bufs]); z_one = on["z"].download()
    summary = dict(batch=B, inflight=K, steps=args.steps, rounds=args.rounds, median_solves_per_s=med, plain_spread_over_rounds=spread,
                   uniform_over_plain=med["uniform"] / med["plain"], mixed_over_plain=med["mixed"] / med["plain"],
                   uniform_bitwise_equal_plain=bool(np.array_equal(a["z"], b["z"]) and np.array_equal(a["iters"], b["iters"])),
                   mean_iters=dict(plain=float(a["iters"].mean()), mixed=float(c["iters"].mean())),
                   solved=dict(plain=int((a["status"] == 0).sum()), mixed=int((c["status"] == 0).sum())),
                   sweep=dict(handles=H, instances_each=n, ms_many_handles=float(np.median(t_many)), ms_one_mixed_launch=float(np.median(t_one)),
                              speedup=float(np.median(t_many) / np.median(t_one)), bitwise_equal_z=bool(np.array_equal(z_many, z_one))))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
