"""What the stepwise loop costs and what it saves: C5's workload (4096 sample_c3 scenes, 80 receding-horizon steps, predicted obstacles,
hold off) driven six ways on one MI355X:
  (a) closed      mpcb_closed_loop: everything inside one call.  Its round-to-round spread is the yardstick.
  (b) stepwise    one ControlLoop driven by step_device + advance_device (sync = 0): the same device work, two calls per step
  (c4), (c16)     four loops of 1024 scenes on four lanes, sixteen loops of 256 scenes on sixteen lanes, stepped alternately
  (d) host step   ControlLoop.step with the plant and the obstacle advance in numpy: the warm start stays on the device
  (e) today       what a caller does without the loop: solve_batch(z0 = shift(z)) with the shift, the obstacle roll-out and the plant in numpy
(b), (c4), (c16) must reproduce (a) bit for bit (u_hist, status, iters, the final states and obstacles): asserted BEFORE a number is printed.
Timed: from the first call to the synchronisation after the last; for (b), (c) the scenes are resident and the per-step outputs stay on the
device until the clock has stopped ((a) moves its histories inside its call: 4096 x 81 x 4 doubles, noise against 80 solves).
The variants alternate in rounds so that clock and thermal drift hit all alike; medians over the rounds are reported.
    python tools/loop_throughput.py [--batch 4096] [--steps 80] [--rounds 5]
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
from mpc_motion_planning_amd.solver import BatchSolver, default_config   # noqa: E402

N, T, NOBS = 30, 0.1, 3


def kin_step(x, u, wheelbase):
    f = np.stack([x[:, 3] * np.cos(x[:, 2]), x[:, 3] * np.sin(x[:, 2]), x[:, 3] * np.tan(u[:, 0]) / wheelbase, u[:, 1]], axis=1)
    return x + T * f


def move(ob):
    ob = ob.copy()
    ob[..., 0] += ob[..., 3] * np.cos(ob[..., 2]) * T
    ob[..., 1] += ob[..., 3] * np.sin(ob[..., 2]) * T
    return ob


def shift(z):
    B = len(z)
    u = z[:, :2 * N].reshape(B, N, 2); x = z[:, 2 * N:].reshape(B, N + 1, 4)
    return np.concatenate([np.concatenate([u[:, 1:], u[:, -1:]], axis=1).reshape(B, -1), np.concatenate([x[:, 1:], x[:, -1:]], axis=1).reshape(B, -1)], axis=1)


class Stepwise:
    """`parts` loops on one handle with `parts` lanes, each over a contiguous slice of the scenes; the outputs of step t go to row t of
    per-loop device histories, so nothing waits before the end."""

    def __init__(self, cfg, x0, xs, ob0, steps, parts):
        self.bs = BatchSolver(cfg, inflight=parts)
        self.steps, self.cuts = steps, np.array_split(np.arange(len(x0)), parts)
        self.src = (x0, xs, ob0)
        self.runs = []
        for idx in self.cuts:
            n = len(idx)
            self.runs.append(dict(n=n, loop=self.bs.loop(n, predict=True), x0=self.bs.device_array((n, 4)), xs=self.bs.device_array((n, 4)),
                                  ob=self.bs.device_array((n, NOBS, 6)), u=self.bs.device_array((steps, n, 2)),
                                  st=self.bs.device_array((steps, n), np.int32), it=self.bs.device_array((steps, n), np.int32)))

    def load(self):
        for idx, r in zip(self.cuts, self.runs):
            r["x0"].upload(self.src[0][idx]); r["xs"].upload(self.src[1][idx]); r["ob"].upload(self.src[2][idx])
            r["loop"].reset()

    def run(self):
        for t in range(self.steps):
            for r in self.runs:
                n = r["n"]
                u_t = r["u"].ptr.value + t * n * 16
                r["loop"].step_device(r["x0"], r["xs"], u_t, d_obs=r["ob"], d_status=r["st"].ptr.value + t * n * 4, d_iters=r["it"].ptr.value + t * n * 4)
                r["loop"].advance_device(r["x0"], u_t, r["ob"])
        self.bs.sync()

    def result(self):
        cat = lambda k, ax: np.concatenate([r[k].download() for r in self.runs], axis=ax)   # noqa: E731
        return dict(u_hist=cat("u", 1).transpose(1, 0, 2), status=cat("st", 1).T, iters=cat("it", 1).T, x_end=cat("x0", 0), obs_state=cat("ob", 0))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    B, steps = args.batch, args.steps
    cfg = default_config(N=N, T=T, n_obs=NOBS)
    x0, xs, ob0, _ = scenes.sample_c3(B, N=N, dt=T, seed=0, n_obs=NOBS)
    bs = BatchSolver(cfg)
    sw = {"b_stepwise": Stepwise(cfg, x0, xs, ob0, steps, 1), "c4_lanes": Stepwise(cfg, x0, xs, ob0, steps, 4),
          "c16_lanes": Stepwise(cfg, x0, xs, ob0, steps, 16)}
    keep = {}

    def closed():
        keep["a_closed"] = bs.closed_loop(x0, xs, ob0, steps=steps, obs_motion=_abi.OBSMOVE_PREDICTED)

    def host_step():
        x, ob, st = x0.copy(), ob0.copy(), []
        with bs.loop(B, predict=True) as loop:
            for _ in range(steps):
                r = loop.step(x, xs, ob, want_z=False)
                x = kin_step(x, r["u0"], cfg.veh_l); ob = move(ob); st.append(r["status"])
        keep["d_host_step"] = dict(status=np.stack(st, axis=1), x_end=x)

    def today():
        x, ob, z0, st = x0.copy(), ob0.copy(), np.zeros((B, bs.nz)), []
        for _ in range(steps):
            r = bs.solve_batch(x, xs, scenes.predict_obstacles(ob, T, N), z0=z0)
            x = kin_step(x, r["z"][:, :2], cfg.veh_l); ob = move(ob); z0 = shift(r["z"]); st.append(r["status"])
        keep["e_today"] = dict(status=np.stack(st, axis=1), x_end=x)

    variants = [("a_closed", None, closed)] + [(k, v.load, v.run) for k, v in sw.items()] + [("d_host_step", None, host_step), ("e_today", None, today)]
    secs = {k: [] for k, _, _ in variants}
    lines = []
    for r in range(-1, args.rounds):                   # round -1 warms every path up (allocations, LDS attributes) and is not counted
        for name, prepare, fn in variants:
            if prepare:
                prepare()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= 0:
                secs[name].append(dt)
                lines.append("round %d %-12s %8.1f ms  %10.0f solves/s" % (r, name, 1e3 * dt, B * steps / dt))
    a = keep["a_closed"]
    for name, v in sw.items():                          # bit equality first, numbers after
        g = v.result()
        for k, want in (("u_hist", a["u_hist"]), ("status", a["status"]), ("iters", a["iters"]), ("x_end", a["x_hist"][:, -1]), ("obs_state", a["obs_state"])):
            assert np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(want).tobytes(), "%s: %s differs from mpcb_closed_loop" % (name, k)
    print("\n".join(lines))
    med = {k: float(np.median(v)) for k, v in secs.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in secs.items()}
    nz = bs.nz
    pcie = dict(d_host_step=dict(up=8 * (4 + 4 + NOBS * 6), down=8 * 2 + 4 + 4 + 8, down_with_z=8 * 2 + 4 + 4 + 8 + 8 * nz),
                e_today=dict(up=8 * (4 + 4 + NOBS * (N + 1) * 6 + nz), down=8 * nz + 8 + 4 + 4 + 8 * 4))
    b_over_a = med["b_stepwise"] / med["a_closed"]
    summary = dict(batch=B, steps=steps, rounds=args.rounds, median_ms={k: 1e3 * v for k, v in med.items()}, spread_over_rounds=spread,
                   solves_per_s={k: B * steps / v for k, v in med.items()},
                   b_over_a=b_over_a, b_inside_spread_of_a=bool(abs(b_over_a - 1.0) <= spread["a_closed"]),
                   c4_over_b=med["c4_lanes"] / med["b_stepwise"], c16_over_b=med["c16_lanes"] / med["b_stepwise"],
                   d_over_e=med["d_host_step"] / med["e_today"], pcie_bytes_per_instance_and_step=pcie,
                   stepwise_bitwise_equal_closed_loop=True,
                   solved_share=dict(a_closed=float(((a["status"] == 0) | (a["status"] == 8)).mean()),
                                     d_host_step=float(((keep["d_host_step"]["status"] == 0) | (keep["d_host_step"]["status"] == 8)).mean()),
                                     e_today=float(((keep["e_today"]["status"] == 0) | (keep["e_today"]["status"] == 8)).mean())),
                   d_vs_e_final_state_linf=float(np.nanmax(np.abs(keep["d_host_step"]["x_end"] - keep["e_today"]["x_end"]))))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
