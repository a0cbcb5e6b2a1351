"""Cases, numpy restatements and float64 reference of lvx_landmark_covariance, shared by tests/test_lmcov_host.py, tests/test_gpu_landmark_cov.py and the generator of
the reference's own accuracy, tests/golden/make_landmark_cov_ref.py.  Not a test module.

Definition (include/lvx.h): with F the free tangent scalars, A_R = s H_FF s + diag(lmd) / R as calib_cov_cases.damped_system builds it, Sigma = s A_R^-1 s; a landmark's
window is (rho_l, the 31 scalars of the LVX_FRAME_CAMERA pose at its reference time), window_cov = Sigma over them, point_cov = J window_cov J^T.  The device does not
invert A_R: it eliminates the landmarks first and reads
    Sigma_ll = w_l + w_l^2 E_l Sigma_xx E_l^T,    Sigma_lx = -w_l E_l Sigma_xx,    w_l = s_l^2 / (s_l^2 H_ll + lmd_l / R)
from the selected inverse of the reduced system (landmark_block below restates that read)."""
import numpy as np

import calib_cov_cases as CC
import lvx
import synth
import trajcov_cases as TC

W = lvx.LM_COV_W   # 32: the inverse depth and the 31 scalars of the reference pose


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the selected inverse with the WIDE band store, and the landmark formula on it
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def up16(x):
    return (x + 15) // 16 * 16


def selinv_wide(Lb, Z, S, nb, bw, nbd, lowest=0):
    """trajcov_cases.selinv_panels with k_band_selinv's second store: sigw [nb, TB + 1], sigw[j, d] = Sigma(j + d, j) for d <= TB = up16(max(bw, 23)); zb [nbd, nb]; cc."""
    TB = up16(max(bw, 23)); R = TB + 16; nbp = up16(nbd); mT = TB + nbp; M = R + nbp
    cc = TC.border_inverse(S)
    D = np.zeros((M, M))
    D[R:R + nbd, R:R + nbd] = cc
    sigw = np.full((max(nb, 1), TB + 1), np.nan)
    zb = np.full((nbd, max(nb, 1)), np.nan)
    j0 = (nb - 1) // 16 * 16 if nb > 0 else -16
    while j0 >= 0 and j0 + 15 >= lowest:
        nk = min(16, nb - j0)
        slot = np.array([(j0 + 16 + k) % R if k < TB else R + k - TB for k in range(mT)])
        sJ = j0 % R
        Gp = np.zeros((16 + mT, 16))
        for c in range(16):
            if c >= nk:
                Gp[c, c] = 1.0
                continue
            j = j0 + c
            for r in range(16 + TB):
                d = j0 + r - j
                if j0 + r < nb and 0 <= d <= bw:
                    Gp[r, c] = Lb[j, d]
            Gp[16 + TB:16 + TB + nbd, c] = Z[:, j]
        GT = Gp[16:]
        Wm = GT.T @ D[np.ix_(slot, slot)]
        Li = np.linalg.inv(Gp[:16])
        X = -(Li.T @ Wm)
        P = Li.T @ (np.eye(16) + Wm @ GT) @ Li
        X[nk:] = 0.0
        P[nk:] = 0.0; P[:, nk:] = 0.0
        D[np.ix_(slot, sJ + np.arange(16))] = X.T
        D[np.ix_(sJ + np.arange(16), slot)] = X
        D[sJ:sJ + 16, sJ:sJ + 16] = P
        for c in range(nk):
            for a in range(c, nk):
                sigw[j0 + c, a - c] = P[a, c]
            for i in range(TB):
                d = 16 + i - c
                if d <= TB and j0 + 16 + i < nb:
                    sigw[j0 + c, d] = X[c, i]
            zb[:, j0 + c] = X[c, TB:TB + nbd]
        j0 -= 16
    return sigw, zb, cc


def sigma_at(pa, pb, sigw, zb, cc):
    """lvx_selinv.h's sigma_at over the wide band store: the scaled inverse between two positions (>= 0 band, < 0 border slot -1 - o)"""
    if pa >= 0 and pb >= 0:
        lo, d = min(pa, pb), abs(pa - pb)
        return sigw[lo, d] if d < sigw.shape[1] else 0.0
    if pa >= 0:
        return zb[-1 - pb, pa]
    if pb >= 0:
        return zb[-1 - pa, pb]
    return cc[max(-1 - pa, -1 - pb), min(-1 - pa, -1 - pb)]


def landmark_block(e_pos, e_val, w, win_pos, scale, nb, sigw, zb, cc):
    """k_landmark_cov's window: e_pos / e_val the non-zeros of the landmark's UNSCALED row (positions as above), w = w_l, win_pos the positions of the other window
    scalars (None: constant), scale over [band | border].  Returns the (1 + len(win_pos))^2 window over (rho, win_pos)."""
    sc = lambda p: scale[p if p >= 0 else nb - 1 - p]
    ev = [v * sc(p) for p, v in zip(e_pos, e_val)]
    q = 0.0
    for a in range(len(ev)):
        for b in range(a, len(ev)):
            t = ev[a] * ev[b] * sigma_at(e_pos[a], e_pos[b], sigw, zb, cc)
            q += t if a == b else 2.0 * t
    n = 1 + len(win_pos)
    Wn = np.zeros((n, n))
    Wn[0, 0] = w + w * w * q
    for m, pm in enumerate(win_pos):
        if pm is None:
            continue
        cm = sum(ev[a] * sigma_at(e_pos[a], pm, sigw, zb, cc) for a in range(len(ev)))
        Wn[0, 1 + m] = Wn[1 + m, 0] = -w * cm * sc(pm)
        for k, pk in enumerate(win_pos):
            if pk is not None:
                Wn[1 + m, 1 + k] = sigma_at(pm, pk, sigw, zb, cc) * (sc(pm) * sc(pk))
    return Wn


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the map point, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def unproject(cam, uv):
    """cam_unproject (lvx_resid.h): the pinhole ray, through eight rounds of the radtan fixed point when the camera is distorted (pinhole_camera.h's test, p1 twice)"""
    mx, my = (uv[0] - cam["cx"]) / cam["fx"], (uv[1] - cam["cy"]) / cam["fy"]
    if not (abs(cam["k1"]) > 1e-5 or abs(cam["k2"]) > 1e-5 or abs(cam["p1"]) > 1e-5):
        return np.array([mx, my, 1.0])

    def dist(x, y):
        r2 = x * x + y * y
        rad = cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
        return (x * rad + 2 * cam["p1"] * x * y + cam["p2"] * (r2 + 2 * x * x), y * rad + 2 * cam["p2"] * x * y + cam["p1"] * (r2 + 2 * y * y))
    x, y = mx, my
    for _ in range(8):
        dx, dy = dist(x, y)
        x, y = mx - dx, my - dy
    return np.array([x, y, 1.0])


def ref_time(P, l):
    """the reference time WITHOUT the camera's time offset (a LVX_FRAME_CAMERA query adds it)"""
    c = P["camera"]
    return P["lm_t0"][l] + P["lm_uv"][l, 1] * (c["readout"] / c["rows"])


def qrot(q, v):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ v


def point_from_pose(P, state, l, q_c, p_c):
    """P_w = R_C (y_h / rho) + p_C from the camera-frame pose (q x, y, z, w; p) at the reference time"""
    rho = state[7 * P["n_knots"] + 32 + l]
    return qrot(q_c, unproject(P["camera"], P["lm_uv"][l]) / rho) + p_c


def window_indices(P, state, l):
    """the 32 tangent indices of landmark l's window (locks not applied)"""
    N = P["n_knots"]
    return [6 * N + 22 + l] + TC.window_indices(dict(P, state0=state), ref_time(P, l), lvx.FRAME_CAMERA)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TRACKS = dict(seed=31, duration=0.6, n_surfel=200, n_planes=10, n_landmarks=70, views_per_lm=3, n_camsurf=0)   # 54 knots, 70 landmarks of 3 views
ND6 = dict(CC.ND, n_landmarks=6)
HUB_LM, NOROWS_LM = 0, 5


def problem(key):
    """small: calib_cov_cases.SMALL.  tracks: 70 short tracks.  hub: SMALL with landmark HUB_LM's reference view moved to t_map, so that its window and its row hold
    hub knots (border slots).  norows: SMALL with every reprojection row of landmark NOROWS_LM removed (H_ll = 0).  nd6: calib_cov_cases.ND with 6 landmarks."""
    if key == "small":
        return synth.make_problem(**CC.SMALL)
    if key == "tracks":
        return synth.make_problem(**TRACKS)
    if key == "nd6":
        return synth.make_problem(**ND6)
    P = synth.make_problem(**CC.SMALL)
    P = dict(P)
    if key == "hub":
        c = P["camera"]
        old = P["lm_t0"][HUB_LM]
        new = P["t_map"] - P["lm_uv"][HUB_LM, 1] * (c["readout"] / c["rows"])
        P["lm_t0"] = P["lm_t0"].copy(); P["rep_t0"] = P["rep_t0"].copy()
        P["lm_t0"][HUB_LM] = new
        P["rep_t0"][(P["rep_lm"] == HUB_LM) & (P["rep_t0"] == old)] = new   # the reference view's own row moves with it
        return P
    if key == "norows":
        keep = P["rep_lm"] != NOROWS_LM
        P["rep_lm"], P["rep_uv"], P["rep_t0"] = P["rep_lm"][keep], P["rep_uv"][keep], P["rep_t0"][keep]
        return P
    raise KeyError(key)


# name -> (problem key, lock mask, radii, scalings)
CASES = {}
for _mask in ("solve2", "solve3"):
    for _r in CC.RADII:
        for _s in (True, False):
            CASES["small_" + CC.case_name(_mask, _r, _s)] = ("small", CC.MASKS[_mask], _r, _s)
for _key, _locks in (("tracks", CC.SOLVE2), ("hub", CC.SOLVE2), ("norows", CC.SOLVE2), ("nd6", CC.ND_LOCKS)):
    for _r in CC.RADII:
        CASES[_key + "_" + CC.case_name("lm", _r, True)] = (_key, _locks, _r, True)


def probe_landmarks(key, P):
    """landmarks whose windows the reference's own error is measured on (tests/golden/make_landmark_cov_ref.py): all of them on the problems of up to 12 landmarks, the
    first two, the middle one and the last of the 70 tracks"""
    L = P["n_landmarks"]
    return list(range(L)) if L <= 12 else [0, 1, L // 2, L - 1]
