"""Launch lanes whose lane 0 is not the handle's stream, and the restoration launch that is not made: kin<1>, N = 30,
the default config, scenes.sample_c2.  The contract of mpcbatch.h must hold as before: (a) work queued on the handle's stream before a
solve call happens before that solve, (b) every entry point other than an asynchronous solve sees all earlier solves finished, (c) calls k
and k + K share a lane and are ordered.  Every comparison is bit for bit: the kernels are the same, only streams and launches differ.
The CPU tier of the skipped pass is tests/test_launch_passes_cpu.py."""
import numpy as np
import pytest

from mpc_motion_planning_amd import scenes, _abi
from mpc_motion_planning_amd.solver import default_config

pytestmark = pytest.mark.gpu
B, NZ = 37, 184
OUT = ("z", "obj", "status", "iters", "kkt")
SWITCHES = ("MPCB_LANE0_OWN_STREAM", "MPCB_SKIP_EMPTY_PASS")
BATCHES = [scenes.sample_c2(B, seed=100 + j) for j in range(33)]          # 2 K + 1 different batches for K up to 16
_REF = {}


def cfg_c2(**kw):
    c = default_config(N=kw.pop("N", 30), n_obs=kw.pop("n_obs", 1))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.fixture
def refs(gpu_solver_factory):
    """refs(j): the synchronous one-lane solve of batch j, computed once per session and never changed"""
    def get(j):
        if j not in _REF:
            if "h" not in _REF:
                _REF["h"] = gpu_solver_factory(cfg_c2())
            _REF[j] = _REF["h"].solve_batch(*BATCHES[j])
            for k in OUT:
                _REF[j][k].setflags(write=False)
        return _REF[j]
    return get


class Set:
    """the device inputs of one batch / one output set"""
    def __init__(self, h, batch=None, b=B, nz=NZ):
        if batch is not None:
            self.x0, self.xs, self.obs = (h.device_array(a.shape).upload(a) for a in batch)
        self.z = h.device_array((b, nz)); self.obj = h.device_array((b,)); self.kkt = h.device_array((b, 4))
        self.st = h.device_array((b,), np.int32); self.it = h.device_array((b,), np.int32)

    def get(self):
        return dict(z=self.z.download(), obj=self.obj.download(), status=self.st.download(), iters=self.it.download(), kkt=self.kkt.download())


def solve(h, inp, out, st=None, it=None, b=B):
    h.solve_device(b, inp.x0, inp.xs, inp.obs, _abi.OBSIN_STATIC, None, out.z, out.obj, st or out.st, it or out.it, out.kkt)


def same(got, ref, what):
    for k in OUT:
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_two_rounds_and_one_of_different_batches(gpu_solver_factory, refs, K):
    """2 K + 1 asynchronous solves of different batches, none waited for.  z, obj and kkt of solve j go to a set of its own, its status
    and iteration columns to set j mod K of a ring, so solves j and j + K write the same columns from the same lane: (c)."""
    h = gpu_solver_factory(cfg_c2(), inflight=K)
    n = 2 * K + 1
    inp = [Set(h, BATCHES[j]) for j in range(n)]
    ring = [(h.device_array((B,), np.int32), h.device_array((B,), np.int32)) for _ in range(K)]
    for j in range(n):
        solve(h, inp[j], inp[j], *ring[j % K])
    h.sync()
    for j in range(n):
        for k in ("z", "obj", "kkt"):
            assert getattr(inp[j], k).download().tobytes() == refs(j)[k].tobytes(), (K, j, k)
    for s in range(K):
        j = max(q for q in range(n) if q % K == s)
        assert ring[s][0].download().tobytes() == refs(j)["status"].tobytes(), (K, s)
        assert ring[s][1].download().tobytes() == refs(j)["iters"].tobytes(), (K, s)


@pytest.mark.parametrize("first_lane", [0, 1])
@pytest.mark.parametrize("K", [3, 16])
def test_an_upload_between_two_solves_of_the_same_arrays(gpu_solver_factory, refs, K, first_lane):
    """(a) and (b): batch A solved asynchronously on lane `first_lane`, batch B uploaded into the same device arrays (the upload must
    see the solve of A finished, lane 0 included), a second solve of those arrays (which must see the upload), then one wait."""
    h = gpu_solver_factory(cfg_c2(), inflight=K)
    A, Bb, C = 0, 1, 2
    inp = Set(h, BATCHES[A]); second = Set(h); other = Set(h, BATCHES[C])
    for _ in range(first_lane):
        solve(h, other, other)                       # takes lane 0, so that the solve of A lands on a lane > 0
    solve(h, inp, inp)
    for d, a in zip((inp.x0, inp.xs, inp.obs), BATCHES[Bb]):
        d.upload(a)
    solve(h, inp, second)
    h.sync()
    same(inp.get(), refs(A), "first solve")
    same(second.get(), refs(Bb), "second solve")
    if first_lane:
        same(other.get(), refs(C), "solve on lane 0")


def test_set_inflight_down_and_up_with_solves_between(gpu_solver_factory, refs):
    """4 -> 1 -> 16 lanes: mpcb_set_inflight waits for what is in flight before it destroys a lane's stream, in both directions."""
    h = gpu_solver_factory(cfg_c2(), inflight=4)
    sets = [Set(h, BATCHES[j]) for j in range(9)]
    for j in range(0, 5):
        solve(h, sets[j], sets[j])
    h.set_inflight(1)                                # five solves outstanding on four lanes
    for j in range(5, 7):
        solve(h, sets[j], sets[j])
    h.set_inflight(16)
    for j in range(7, 9):
        solve(h, sets[j], sets[j])
    same(h.solve_batch(*BATCHES[9]), refs(9), "a host-pointer solve behind the asynchronous ones")
    h.sync()
    for j in range(9):
        same(sets[j].get(), refs(j), "solve %d" % j)


@pytest.fixture
def on_off(gpu_solver_factory, monkeypatch):
    """on_off(cfg, **kw) -> (handle as shipped, handle created with both switches at 0: lane 0 the handle's stream, every pass launched)"""
    def make(cfg, **kw):
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        on = gpu_solver_factory(cfg, **kw)
        for s in SWITCHES:
            monkeypatch.setenv(s, "0")
        off = gpu_solver_factory(cfg, **kw)
        for s in SWITCHES:
            monkeypatch.delenv(s)
        return on, off
    return make


def lanes_and_host(h, batch, b, K, nz=NZ):
    """one host-pointer solve, then K + 1 asynchronous solves of the same batch whose last one is returned too"""
    host = h.solve_batch(*batch)
    inp = Set(h, batch, b, nz); outs = [Set(h, None, b, nz) for _ in range(K + 1)]
    for o in outs:
        solve(h, inp, o, b=b)
    h.sync()
    return host, [o.get() for o in outs]


def test_the_skipped_restoration_launch_changes_no_bit(on_off, gpu_solver_factory):
    """sample_c2(256, seed 0), second_start = 0: the plan is FIRST, RESTO and the RESTO pass is not launched.  The batch exercises the
    restoration phase: with cfg.restoration = 0 some instances end at MPCB_ST_LINESEARCH which the default handle carries further
    (the CPU oracle finds two such instances in this batch)."""
    batch = scenes.sample_c2(256, seed=0)
    on, off = on_off(cfg_c2(second_start=0), inflight=2)
    a, a_async = lanes_and_host(on, batch, 256, 2)
    b, b_async = lanes_and_host(off, batch, 256, 2)
    same(a, b, "switches on against off")
    for x, y in zip(a_async, b_async):
        same(x, a, "asynchronous, on"); same(y, a, "asynchronous, off")
    plain = gpu_solver_factory(cfg_c2(second_start=0, restoration=0)).solve_batch(*batch)
    carried = (plain["status"] == _abi.ST_LINESEARCH) & (a["status"] != _abi.ST_LINESEARCH)
    print("without restoration %s, with %s, carried further: %d" % (np.bincount(plain["status"], minlength=9).tolist(),
                                                                    np.bincount(a["status"], minlength=9).tolist(), carried.sum()))
    assert carried.sum() >= 1
    assert not (a["status"] == 7).any()              # MPCB_ST_NEEDS_RESTO never leaves a solve


@pytest.mark.parametrize("N,n_obs", [(30, 3), (50, 1)])
def test_where_the_rule_says_no_every_pass_is_launched(on_off, N, n_obs):
    """kin<3> restores in a launch of its own, and so does kin<1> at N = 50 (the restoration layout would cost the lean launch a
    workgroup per CU): nothing is skipped, and the lanes' streams change no bit either."""
    b, nz = 64, 2 * N + 4 * (N + 1)
    if n_obs == 3:
        x0, xs, obs = scenes.sample_c3(b, seed=0)[:3]
    else:
        x0, xs, obs = scenes.sample_c2(b, seed=0)
    on, off = on_off(cfg_c2(N=N, n_obs=n_obs, second_start=0), inflight=3)
    a, a_async = lanes_and_host(on, (x0, xs, obs), b, 3, nz)
    c, c_async = lanes_and_host(off, (x0, xs, obs), b, 3, nz)
    same(a, c, "switches on against off")
    for x, y in zip(a_async, c_async):
        same(x, a, "asynchronous, on"); same(y, a, "asynchronous, off")
