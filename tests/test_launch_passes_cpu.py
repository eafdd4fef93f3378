"""Which passes of the plan the library launches (mpcbd::pass_is_empty, mpc_motion_planning_amd/csrc/mpcb_dispatch.h): a small host program
over the dispatch header prints, for every shipped instantiation x N in {30, 50} x (restoration, second_start, start given) x force in
{-1, 0, 1}, the plan, which of its launches restores in place, and the passes that are launched.  The rule is restated here: a pass is
dropped exactly when it is the restoration pass behind a launch that restores its own instances, which only the Euler kin<0|1> kernels
without GEN do, at N = 30 (at N = 50 the restoration layout costs the lean launch a workgroup per CU) or when forced.  No GPU, no solve.
The dispatch header is C++17; the program is built as C++20 because the kernel headers it rests on take std::barrier for the wave's
cross-lane steps when built without HIP (as tests/emu builds them).
The device tier is tests/test_lane_order_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_motion_planning_amd", "csrc")
KIN, DYN = 0, 1
FIRST, SECOND, RESTO = 0, 1, 2            # MPCB_PASS_*

PROGRAM = r"""
#define MPCB_WAVE_EMU 1
#include "mpcb_kernel_dyn.h"
#include "mpcb_dispatch.h"
#include <cstdio>
#include <cstring>
int main() {
  using namespace mpcbd;
  for (int I = 0; I < detail::CANDIDATES; ++I) {
    const Variant v = detail::candidate(I);
    if (!shipped(v)) continue;
    for (int N : {30, 50}) for (int resto = 0; resto < 2; ++resto) for (int ss = 0; ss < 4; ++ss) for (int start = 0; start < 2; ++start)
    for (int force = -1; force < 2; ++force) {
      mpcb_config c; std::memset(&c, 0, sizeof c);
      c.model = v.model; c.N = N; c.restoration = resto; c.second_start = ss; c.init_rollout = 1;
      const Plan p = pass_plan(c, start != 0, fuses(v));
      std::printf("%d %d %d %d %d %d %d %d %d %d %d |", v.model, v.nobs, (int)v.gen, (int)v.rk4, (int)v.track, (int)v.params, N, resto, ss, start, force);
      for (int i = 0; i < p.n; ++i) std::printf(" %d", p.pass[i]);
      std::printf(" |");
      for (int i = 0; i < p.n; ++i) std::printf(" %d", (int)resto_in_launch(v, N, p, i, force));
      std::printf(" |");
      for (int i = 0; i < p.n; ++i) if (!pass_is_empty(v, N, p, i, force)) std::printf(" %d", p.pass[i]);
      std::printf("\n");
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_passes")
    src = d / "passes.cpp"
    src.write_text(PROGRAM)
    exe = d / "passes"
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-pthread", "-o", str(exe), str(src)])
    out = []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        key, plan, here, launched = (tuple(int(x) for x in part.split()) for part in line.split("|"))
        out.append((key, plan, here, launched))
    return out


def restores_in_place(model, nobs, gen, rk4, N, force):
    """the rule of DESIGN.md §5.2, restated: the instantiation has the code, and at N = 30 the restoration layout's LDS leaves it four
    workgroups per CU as its own does (N = 50: three against two)"""
    return model == KIN and nobs <= 1 and not gen and not rk4 and force != 0 and (force == 1 or N == 30)


def test_every_shipped_variant_is_listed(rows):
    variants = {k[:6] for k, _, _, _ in rows}
    assert len(variants) == 31                       # x 2 passes = the 62 solve kernels of the library
    assert len(rows) == 31 * 2 * 2 * 4 * 2 * 3


def test_the_launched_passes_are_the_plan_without_its_empty_restoration_passes(rows):
    dropped_somewhere = 0
    for key, plan, here, launched in rows:
        model, nobs, gen, rk4, track, params, N, resto, ss, start, force = key
        rule = restores_in_place(model, nobs, gen, rk4, N, force)
        want = []
        for i, p in enumerate(plan):
            # a launch restores in place when the rule says so, it is a lean launch and the plan's next pass is the restoration pass
            in_place = rule and p != RESTO and i + 1 < len(plan) and plan[i + 1] == RESTO
            assert here[i] == int(in_place), (key, plan, here)
            if p == RESTO and i > 0 and here[i - 1]:
                continue                             # dropped: a restoration pass behind a launch that restores in place, and nothing else
            want.append(p)
        assert launched == tuple(want), (key, plan, launched)
        it = iter(plan)
        assert all(p in it for p in launched), (key, plan, launched)          # a subsequence of the plan
        assert launched[0] == FIRST
        dropped_somewhere += len(launched) < len(plan)
        if not rule:
            assert launched == plan, (key, plan, launched)
    assert dropped_somewhere > 0


def test_nothing_is_dropped_where_the_rule_says_no(rows):
    for key, plan, here, launched in rows:
        model, nobs, gen, rk4, track, params, N, resto, ss, start, force = key
        if model == DYN or nobs >= 3 or gen or rk4 or force == 0 or (N == 50 and force == -1) or not resto:
            assert launched == plan and not any(here), (key, plan, launched)


def test_the_flagship_and_its_neighbours(rows):
    """C2 as bench.py runs it (kin<1>, N = 30, restoration, second_start = 3, no start vector): planned FIRST, RESTO, launched FIRST.
    With a start vector: FIRST, RESTO, SECOND, RESTO planned, both lean passes launched.  C3 (kin<3>): all three planned passes."""
    table = {k: (p, l) for k, p, _, l in rows}
    assert table[(KIN, 1, 0, 0, 0, 0, 30, 1, 3, 0, -1)] == ((FIRST, RESTO), (FIRST,))
    assert table[(KIN, 1, 0, 0, 0, 0, 30, 1, 3, 1, -1)] == ((FIRST, RESTO, SECOND, RESTO), (FIRST, SECOND))
    assert table[(KIN, 1, 0, 0, 0, 0, 30, 1, 3, 0, 0)] == ((FIRST, RESTO), (FIRST, RESTO))
    assert table[(KIN, 1, 0, 0, 0, 0, 50, 1, 3, 0, -1)] == ((FIRST, RESTO), (FIRST, RESTO))
    assert table[(KIN, 1, 0, 0, 0, 0, 50, 1, 3, 0, 1)] == ((FIRST, RESTO), (FIRST,))
    assert table[(KIN, 3, 0, 0, 0, 0, 30, 1, 3, 0, -1)] == ((FIRST, RESTO), (FIRST, RESTO))
    assert table[(KIN, 5, 0, 0, 0, 0, 30, 1, 3, 0, -1)] == ((FIRST, SECOND, RESTO), (FIRST, SECOND, RESTO))
