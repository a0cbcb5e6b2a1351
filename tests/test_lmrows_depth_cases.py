"""The premises of tests/lmrows_depth_cases.py on the CPU, from track_regime (the numpy restatement of the host's layout rules) alone: blocks per landmark on either side of the
old trip of four, of the group of 16 and of the 64 lanes of indices; which blocks the chain skips; which blocks reach one variable through both poses."""
import numpy as np
import pytest

import landmark_cases as LC
import lmrows_depth_cases as DC


def _regime(name):
    P, locks, ex = DC.build(name)
    return P, locks, ex, LC.track_regime(P, locks, ex["tau"])


@pytest.mark.parametrize("name", DC.NAMES)
def test_block_counts_and_size(name):
    P, locks, ex, R = _regime(name)
    assert [len(b) for b in R["lm_blocks"]] == ex["counts"]
    assert 55 <= P["n_knots"] <= 66 and len(P["rep_lm"]) <= 200
    assert P["n_landmarks"] % 4 != 0                                      # the last workgroup has idle wavefronts


def test_counts_sit_on_both_sides_of_every_round():
    for cnt in (DC.COUNTS, DC.COUNTS_TAU):
        for edge in (4, DC.GROUP, 64):
            assert edge in cnt and edge + 1 in cnt
    assert 1 in DC.COUNTS and DC.GROUP - 1 in DC.COUNTS_TAU
    assert DC.build("counts_tau_free")[1] == LC.FREE_CAM_TAU and not (LC.FREE_CAM_TAU & LC.lvx.LOCK_CAM_TAU)


def test_skipped_blocks():
    P, locks, ex, R = _regime("skipped")
    got = [int(R["strays"][b].sum()) for b in R["lm_blocks"]]
    assert got == ex["skipped"]
    assert got[0] == ex["counts"][0] and got[4] == ex["counts"][4] == 1    # every block of landmarks 0 and 4
    assert 0 < got[1] < ex["counts"][1] and got[3] == 0
    pos = np.flatnonzero(R["strays"][R["lm_blocks"][2]])                   # landmark 2: a skipped block in its first group of 16 and in its second
    assert ex["counts"][2] > DC.GROUP and (pos < DC.GROUP).any() and (pos >= DC.GROUP).any()
    for name in ("counts", "counts_tau_free", "collide"):
        assert not _regime(name)[3]["strays"].any()


def test_collide_shares_knots_between_the_poses():
    P, locks, ex, R = _regime("collide")
    d = np.abs(R["k0"] - R["k1"])
    assert (d == 0).sum() >= 3 and ((d > 0) & (d < 4)).sum() >= 3         # the same four knots; overlapping knots
    is_ref = np.array([P["rep_t0"][i] == P["lm_t0"][l] and np.array_equal(P["rep_uv"][i], P["lm_uv"][l]) for i, l in enumerate(P["rep_lm"])])
    assert is_ref.sum() == 1
