"""tests/native/vlp16_demo.cpp: a C++ program that calls the scan-ingestion ABI (lvx_vlp16_unpack, lvx_set_scans_vlp16, lvx_get_scans_raw, a refused call) and builds a
lvx_host::Calibrator from CalibrateInput::vlp16_* — what it prints and writes against the numpy restatement of tests/vlp16_cases.py and the Python binding."""
import os
import subprocess

import numpy as np
import pytest

import lvx
import synth
import vlp16
import vlp16_cases as vc

pytestmark = pytest.mark.gpu


def test_cpp_caller_and_calibrator_from_packets(tmp_path):
    libdir = os.path.join(vc.ROOT, "lvi-exc_amd")
    exe = str(tmp_path / "vlp16_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "host"), os.path.join(vc.ROOT, "tests", "native", "vlp16_demo.cpp"), "-o", exe,
                           "-L" + libdir, "-llvx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    S = synth.make_sequence(seed=50)
    rng = np.random.default_rng(8)
    # 6 scans of 4, 3, 4, 4, 2, 4 packets around the LiDAR: a flat floor 1.2 m below and a wall 4 m ahead (ranges from the elevations; no ray-casting needed here)
    counts = [4, 3, 4, 4, 2, 4]
    el = vlp16.VERT_ANGLE[vlp16.DSR_OF_ROW][:, None]
    packets = b""
    for k in counts:
        r = np.where(el < 0, 1.2 / np.maximum(np.sin(-el), 1e-3), 4.0 / np.cos(el)) + 0.01 * rng.standard_normal((16, 24 * k))
        packets += vlp16.encode_packets(r, rng.integers(0, 256, (16, 24 * k)), 500, 37)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    stamps = S["t_start"] + 0.2 + 0.1 * np.arange(len(counts))
    want, info = vc.restate(offsets, packets, stamps)
    assert info["W"] == 96 and info["n_out_of_range"] == 0
    cam = S["camera"]
    state = np.ascontiguousarray(S["state_true"], np.float64)
    head = [S["t0"], S["dt"], S["n_knots"], S["t_map"]] + [cam[k] for k in ("rows", "cols", "readout", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]
    blob = np.concatenate([head, [len(state)], state, [len(stamps)], stamps, [len(offsets)], offsets.astype(np.float64)]).astype(np.float64)
    fin, fpk, fout = str(tmp_path / "in.bin"), str(tmp_path / "packets.bin"), str(tmp_path / "out.bin")
    blob.tofile(fin)
    open(fpk, "wb").write(packets)
    r = subprocess.run([exe, fin, fpk, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = lvx.Context(0)
    try:
        g.set_spline(S["t0"], S["dt"], S["n_knots"])
        assert g.set_scans_vlp16(packets, offsets, stamps) == info
        npl, npt = lvx.data_association(g, state, S["t_map"])
    finally:
        g.close()
    fields = "%d %d %d %d %d %d" % (info["W"], info["n_packets"], info["n_in_range"], info["n_out_of_range"], info["n_outside_window"], info["n_bad_headers"])
    assert r.stdout.splitlines() == ["unpack 0 " + fields, "set 0 " + fields, "refused %d" % lvx.E_ARG, "after 0",
                                     "calibrator %d 16 %d %d %d" % (len(counts), info["W"], info["n_packets"], info["n_in_range"]), "association %d %d" % (npl, npt)]
    got = np.fromfile(fout, vc.POINT).reshape((4,) + want.shape)
    for k, what in enumerate(("lvx_vlp16_unpack", "lvx_set_scans_vlp16", "after the refused call", "the Calibrator's context")):
        assert vc.same_bytes(got[k], want), what
