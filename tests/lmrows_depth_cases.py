"""Landmarks by block count, for the load rounds of k_reproj_lmrows (csrc/lvx_eval.hip): a wavefront fetches the indices of up to 64 blocks of its landmark lane-parallel and then
the records and positions of a group of LMR_G = 16 blocks at a time.  Built with the builders of tests/landmark_cases.py (same geometry: dt = 0.02 s, t0 = 99.8 s), about 60 knots.

build(name) -> (P, locks, expect).  expect["counts"]: blocks per landmark; expect["tau"]: the camera time offset set in both states (the stray mechanism of landmark_cases: a view
0.2 ms inside the upper edge of its window leaves the window under tau = 0.5 ms, the chain skips the block — k = -1 — and the exact kernel takes it from the fallback list)."""
import functools

import numpy as np

import landmark_cases as LC

GROUP = 16                                   # LMR_G
COUNTS = (1, 4, 5, 16, 17, 64, 65)           # either side of the old trip of four, of the group, of the 64 lanes of indices
COUNTS_TAU = (1, 4, 5, 15, 16, 17, 2, 64, 65)
NAMES = ["counts", "counts_tau_free", "skipped", "collide"]
DURATION = 0.8


def _track(P, rng, n, k_ref, reach=8.0, with_ref=False):
    """One landmark of n blocks: the reference view evaluated in interval k_ref, the views evaluated within `reach` intervals of it (drawn again until a camera can have them)."""
    def make():
        views = [("at", LC.t_of(P, k_ref, 0.5) + rng.uniform(-reach, reach) * LC.DT) for _ in range(n - (1 if with_ref else 0))]
        return LC.lm_at(P, LC.t_of(P, k_ref, 0.5), ([("ref",)] if with_ref else []) + views, v=rng.uniform(200, 520), u=rng.uniform(400, 880), z=rng.uniform(5.0, 12.0))
    return LC._draw(P, 1, make)[0]


@functools.lru_cache(maxsize=None)
def build(name):
    """(P, locks, expect) of a case; memoised: the arrays are shared between the tests of a session and must not be written to."""
    seed = LC.hash_name("lmrows_depth_" + name)
    rng = np.random.default_rng(seed)
    P = LC._base(301, duration=DURATION)
    locks, expect = LC.TAU, {"tau": 0.0}
    if name in ("counts", "counts_tau_free"):
        cnt = COUNTS if name == "counts" else COUNTS_TAU
        if name == "counts_tau_free":
            locks = LC.FREE_CAM_TAU                                              # the record has 57 entries
        tracks = [_track(P, rng, c, 20 + 3 * l, with_ref=(l % 2 == 1)) for l, c in enumerate(cnt)]
        expect.update(counts=list(cnt))
    elif name == "skipped":
        # tau = 0.5 ms in the state, locked.  Landmark 0: its reference view strays, so ALL its blocks are skipped; landmark 1: 2 of its 6 blocks; landmark 2: 18 blocks, 3 skipped
        # (in its first group of 16 and in its second); landmark 3: none; landmark 4: one block, skipped
        expect["tau"] = 5e-4
        edge = lambda w: P["t0"] + (4 * w + 4) * LC.DT - 2e-4    # noqa: E731
        near = lambda k, n: [("at", LC.t_of(P, k + 0.7 * i, 0.35)) for i in range(n)]   # noqa: E731
        tracks = [LC.lm_at(P, edge(8), near(30, 5), v=300.0),
                  LC.lm_at(P, LC.t_of(P, 33, 0.5), near(36, 2) + [("at", edge(9))] + near(38, 2) + [("at", edge(10))], v=250.0, u=500.0),
                  LC.lm_at(P, LC.t_of(P, 26, 0.5), near(22, 7) + [("at", edge(6))] + near(28, 8) + [("at", edge(7)), ("at", edge(8))], v=420.0, u=800.0, z=9.0),
                  LC.lm_at(P, LC.t_of(P, 40, 0.5), near(41, 3), v=350.0, u=700.0),
                  LC.lm_at(P, LC.t_of(P, 22, 0.5), [("at", edge(5))], v=200.0, u=600.0)]
        expect.update(counts=[5, 6, 18, 3, 1], skipped=[5, 2, 3, 0, 1])
    elif name == "collide":
        # views closer than seven knots to the reference view, and on its very interval: the same variable reaches the row through both poses of a block
        tracks = [LC.lm_at(P, LC.t_of(P, 30, 0.25), [("at", LC.t_of(P, 30, 0.75)), ("at", LC.t_of(P, 31, 0.5)), ("at", LC.t_of(P, 33, 0.5)), ("at", LC.t_of(P, 28, 0.4)), ("ref",)], v=300.0),
                  LC.lm_at(P, LC.t_of(P, 41, 0.6), [("at", LC.t_of(P, 41, 0.1)), ("at", LC.t_of(P, 42, 0.5))], v=420.0, u=500.0, z=5.0)]
        expect.update(counts=[5, 2])
    else:
        raise KeyError(name)
    Q = LC.attach_tracks(P, tracks, seed)
    if expect["tau"] != 0.0:
        for k in ("state0", "state_true"):
            Q[k] = Q[k].copy(); Q[k][LC.tau_cam_slot(Q)] = expect["tau"]
    return Q, locks, expect
