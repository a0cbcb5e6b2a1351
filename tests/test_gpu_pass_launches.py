"""GPU: the launches of one evaluation pass, per kernel id, for every way run_evaluate can be configured.

With profiling on, Context.kernel_ms() returns how often each of the 17 kernel ids was launched.  The expected vectors in
tests/golden/pass_launches.json were RECORDED (python tests/test_gpu_pass_launches.py <out.json>, the __main__ block below) from the commit
named inside that file, before run_evaluate was split into per-family steps.  The counts are integers and do not depend on the toolchain;
nothing here is timed or compared in floating point.

What the vectors can and cannot see: kernel_ms() counts PROFILING SCOPES, one per kernel id and step, not launches.  A vector that differs means
a step appeared, vanished or changed its id (fused against per-segment kernels, chain against single-launch reprojection, a fallback list on).
The colour-by-colour launches of DETERMINISTIC sit inside one scope, as do the gyroscope and accelerometer kernels over the IMU list, and a
free time offset selects another template instance under the same id: a wrong instance, stream, PW or list argument does not show here.  Those
are covered by the numeric tests of the suite and were checked for this refactor by bit-identical DETERMINISTIC results (docs/HISTORY.md)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "lvi-exc_amd")]

import lvx
import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_launches.json")
TAU_LOCKS = lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU
SOLVE0_LOCKS = TAU_LOCKS | lvx.LOCK_R3 | lvx.LOCK_ACC_BIAS | lvx.LOCK_GYRO_BIAS   # test_gpu_eval.py::test_so3_only_solve0

# name -> (switches, locks, keyword arguments of Context.evaluate)
CASES = {
    "default": ((), TAU_LOCKS, dict(normal_eq=True)),
    "force_legacy": (("FORCE_LEGACY",), TAU_LOCKS, dict(normal_eq=True)),
    "serial": (("SERIAL",), TAU_LOCKS, dict(normal_eq=True)),
    "deterministic": (("DETERMINISTIC",), TAU_LOCKS, dict(normal_eq=True)),
    "rep_fused": (("REP_FUSED",), TAU_LOCKS, dict(normal_eq=True)),
    "free_time_offsets": ((), 0, dict(normal_eq=True)),
    "lock_r3_solve0": ((), SOLVE0_LOCKS, dict(normal_eq=True)),
    "lock_landmarks": ((), TAU_LOCKS | lvx.LOCK_LANDMARKS, dict(normal_eq=True)),
    "cost_only": ((), TAU_LOCKS, dict(normal_eq=False)),
    "jacobian_blocks": ((), TAU_LOCKS, dict(normal_eq=True, jac_blocks=True)),
    "jacobian_blocks_rep_fused": (("REP_FUSED",), TAU_LOCKS, dict(normal_eq=True, jac_blocks=True)),
    "fallback_lists_on": ((), TAU_LOCKS, dict(normal_eq=True)),
}


@functools.lru_cache(maxsize=None)
def _problem(fallback):
    P = synth.make_problem(seed=4, duration=2.0, n_surfel=700, n_planes=12, n_landmarks=30, n_camsurf=10)
    s = P["state0"].copy()
    if fallback:
        # test_gpu_eval.py::test_merged_hub_segment_corner_takes_the_exact_fallback: t_map 5 us before a knot, a locked lidar offset of 8 us and 40 surfel
        # points in the interval right behind t_map, whose spans merge with the map-time span: those rows go to the surfel fallback list
        P = dict(P)
        P["t_map"] = P["t0"] + 12 * P["dt"] - 5e-6
        assert P["surf_t"].min() > P["t_map"]
        P["surf_t"] = np.sort(np.concatenate([P["t_map"] + np.linspace(2e-3, 0.03, 40), P["surf_t"][40:]]))
        s[7 * P["n_knots"] + 16 + 7] = 8e-6
    s.setflags(write=False)
    return P, s


def launch_vector(name):
    """The launches per kernel id of one pass of case `name` (the SECOND pass, the one with the lists on, for the fallback case)."""
    switches, locks, kw = CASES[name]
    fallback = name == "fallback_lists_on"
    P, s = _problem(fallback)
    g = lvx.Context(0)
    try:
        for sw in switches:
            g.set_switch(sw, 1)
        lvx.load_problem(g, P, locks)
        if fallback:
            g.evaluate(s, **kw)      # discovers the rows, switches the lists on and repeats itself
        g.set_profiling(True); g.kernel_ms()
        g.evaluate(s, **kw)
        _, n = g.kernel_ms()
        g.set_profiling(False)
        lo = g.layout()
        assert lo["exact_fallback"] == 0
        if fallback:
            assert 0 < lo["fallback_rows"] <= 40 and n[lvx.KERNEL_FIXUP] > 0
    finally:
        g.close()
    assert len(n) == len(lvx.KERNEL_NAMES) == 17
    return [int(v) for v in n]


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_covers_the_cases():
    G = _golden()
    assert G["kernel_names"] == lvx.KERNEL_NAMES and sorted(G["vectors"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_pass_launches(name):
    got = launch_vector(name)
    want = _golden()["vectors"][name]
    print(name, dict(zip(lvx.KERNEL_NAMES, got)))
    assert got == want, {k: (a, b) for k, a, b in zip(lvx.KERNEL_NAMES, got, want) if a != b}


if __name__ == "__main__":   # recording mode: python tests/test_gpu_pass_launches.py <out.json> [<commit the library was built from>]
    out = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "problem": "synth.make_problem(seed=4, duration=2.0, n_surfel=700, n_planes=12, n_landmarks=30, n_camsurf=10)",
           "kernel_names": lvx.KERNEL_NAMES, "vectors": {}}
    try:
        for case in CASES:
            out["vectors"][case] = launch_vector(case)
            print(case, out["vectors"][case], flush=True)
    finally:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
