"""VLP-16 scan ingestion without a GPU: the per-record function the kernels run (lvi-exc_amd/csrc/lvx_vlp16.h, built here with g++ -O2 -ffp-contract=off:
tests/native/vlp16_host_check.cpp) against the numpy restatement of the reference's unpack_scan (tests/vlp16_cases.py), records compared as bytes (NaN payloads and
signed zeros included), the counts as integers; the tables against this machine's libm; the packet encoder's round trip."""
import numpy as np
import pytest

import vlp16
import vlp16_cases as vc


def test_tables_are_libms():
    """36000 + 36000 + 16 + 16 floats, bit for bit what cosf / sinf of the running machine return for the reference's arguments, and the landmarks of both tables."""
    got, want = vc.host_tables(), vc.tables()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert want[0][0] == 1.0 and want[1][0] == 0.0 and abs(float(want[0][9000])) < 1e-7 and want[1][9000] == 1.0
    assert abs(float(want[2][0]) - np.cos(np.deg2rad(15.0))) < 1e-7 and abs(float(want[3][15]) - np.sin(np.deg2rad(15.0))) < 1e-7


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_case_matches_the_restatement(name):
    c = vc.case(name)
    want, info = vc.restated(name)
    got, ginfo = vc.host_unpack(c["offsets"], c["packets"], c["stamps"], c["W"], **c["options"])
    if c["refused"]:
        assert want is None and got is None and ginfo == (2 if "seventy_seven" in name else 3)
        return
    assert ginfo == info
    assert info["n_in_range"] + info["n_out_of_range"] + info["n_outside_window"] == 384 * info["n_packets"]
    assert vc.same_bytes(got, want)


def test_cases_reach_what_they_are_for():
    """Each edge the cases were built for really occurs in the restatement's own numbers."""
    trace = []
    vc.restated("rounds_to_36000", trace)
    assert 36000 in trace
    trace = []
    vc.restated("raw_rotation_past_36000", trace)
    assert max(trace) > 65535                               # 65535 plus a positive difference
    for name in ("negative_index", "negative_index_wrapped_window"):
        trace = []
        rec, info = vc.restated(name, trace)
        neg = sum(1 for a in trace if a % 36000 != a and a < 0)
        assert 0 < neg <= 32 and info["n_outside_window"] >= neg and (name != "negative_index" or info["n_outside_window"] == neg)
    rec, info = vc.restated("wrap")
    t = rec["timestamp"][0]
    assert (np.diff(t[0]) > 0).all() and rec.shape == (1, 16, 48)
    rec, info = vc.restated("range_and_intensity_edges")
    r = rec[0]
    nan = np.isnan(r["x"])
    assert info["n_out_of_range"] == 384 // 2 and nan.sum() == 192 and (r["timestamp"] != 0).all()           # raw 0 and 299 are out, 300 (0.6 m as a float is above 0.6) and 65535 are in
    assert set(np.unique(r["intensity"][~nan])) == {0.0, 255.0} and not r["intensity"][nan].any()
    assert vc.restated("wrong_headers")[1]["n_bad_headers"] == 2
    for name in ("window_min_below_max", "window_min_above_max"):
        rec, info = vc.restated(name)
        zero = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 32).any(axis=1) == 0
        assert 0 < info["n_outside_window"] < 384 * info["n_packets"] and zero.sum() == info["n_outside_window"]
    rec, info = vc.restated("two_scans_2_and_3")
    assert rec.shape == (2, 16, 72) and np.isnan(rec["x"][0, :, 48:]).all() and not rec["timestamp"][0, :, 48:].any() and rec["timestamp"][1, :, 48:].all()
    assert rec["timestamp"][1, 15, 0] == vc.case("two_scans_2_and_3")["stamps"][1] + 15 * 2.304 * 1e-6     # block_counter restarts; dsr 0 sits in row 15
    rec, info = vc.restated("an_empty_scan_between")
    assert np.isnan(rec["x"][1]).all() and not rec["timestamp"][1].any()


@pytest.mark.parametrize("name", sorted(vc.ORGANISED))
def test_organised_overload(name):
    xyzi, stamps = vc.organised_input(name)
    want = vc.restate_organised(xyzi, stamps)
    assert vc.same_bytes(vc.host_organised(xyzi, stamps), want)
    n, H, W = vc.ORGANISED[name]
    assert want["timestamp"][n - 1, H - 1, W - 1] == stamps[n - 1] + ((H - 1) * 2.304 * 1e-6 + (W - 1) * 55.296 * 1e-6)


def test_encoder_round_trip():
    """encode_packets -> unpack gives back the 2 mm-quantised ranges, at the organised (row, column) they were given for.  Bar: the range comes back as the norm of
    three float products of (raw * 0.002f) with table entries — a handful of float roundings, each 2^-24 relative; 1e-6 relative is four times that sum."""
    rng = np.random.default_rng(3)
    ranges = rng.uniform(0.7, 120.0, (16, 72))
    ranges[3, 5], ranges[9, 70] = np.nan, 0.3            # no return, and one below min_range
    inten = rng.integers(0, 256, (16, 72))
    pk = vlp16.encode_packets(ranges, inten, 35000, 40)
    assert len(pk) == 3 * vlp16.PACKET_BYTES
    rec, info = vc.host_unpack([0, 3], pk, [10.0])
    assert info["n_bad_headers"] == 0 and info["n_out_of_range"] == 2 and info["W"] == 72
    r = rec[0]
    q = vlp16.quantise(ranges).astype(np.float64) * 0.002
    norm = np.sqrt(r["x"].astype(np.float64) ** 2 + r["y"].astype(np.float64) ** 2 + r["z"].astype(np.float64) ** 2)
    ok = ~np.isnan(r["x"])
    assert (~ok).sum() == 2 and not ok[3, 5] and not ok[9, 70]
    assert np.abs(norm[ok] - q[ok]).max() <= 1e-6 * q[ok].max() and np.abs(q[ok] - ranges[ok]).max() <= 0.001 + 1e-12
    assert np.array_equal(r["intensity"][ok], inten[ok].astype(np.float32))
    # the rotation of every block, and the elevation of every row
    pkb = np.frombuffer(pk, np.uint8).reshape(3, vlp16.PACKET_BYTES)[:, :1200].reshape(36, 100)
    assert np.array_equal(pkb[:, 2].astype(int) | (pkb[:, 3].astype(int) << 8), (35000 + 40 * np.arange(36)) % 36000)
    el = np.arcsin(r["z"].astype(np.float64) / norm)
    assert np.nanmax(np.abs(el - vlp16.VERT_ANGLE[vlp16.DSR_OF_ROW][:, None])) < 1e-6
    assert vc.same_bytes(rec, vc.restate([0, 3], pk, [10.0])[0])
