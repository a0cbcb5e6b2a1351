"""VLP-16 scan ingestion on the device (k_vlp16_unpack / k_vlp16_pad / k_vlp16_organised of lvi-exc_amd/csrc/lvx_upstream.hip): every case of tests/vlp16_cases.py
through lvx_vlp16_unpack and through lvx_set_scans_vlp16 + lvx_get_scans_raw, byte for byte the numpy restatement of the reference's unpack_scan, the info record equal
to the restatement's counts; the packet route against lvx_set_scans of host-unpacked records down to one data association; the organised overload; the error codes."""
import numpy as np
import pytest

import lvx
import synth
import vlp16
import vlp16_cases as vc

pytestmark = pytest.mark.gpu
GOOD = [n for n in vc.CASE_NAMES if not vc.case(n)["refused"]]
REFUSED = [n for n in vc.CASE_NAMES if vc.case(n)["refused"]]


@pytest.fixture(scope="module")
def ctx():
    g = lvx.Context(0)
    yield g
    g.close()


def _args(c):
    return (c["packets"], c["offsets"], c["stamps"], c["W"])


@pytest.mark.parametrize("name", GOOD)
def test_case_is_the_restatement_on_both_routes(ctx, name):
    c = vc.case(name)
    want, info = vc.restated(name)
    got, ginfo = lvx.vlp16_unpack(ctx, *_args(c), **c["options"])
    assert ginfo == info
    assert vc.same_bytes(got, want)
    sinfo = ctx.set_scans_vlp16(*_args(c), **c["options"])
    assert sinfo == info
    n = len(c["stamps"])
    assert vc.same_bytes(lvx.get_scans_raw(ctx, 0, n, 16, info["W"]), want)
    assert vc.same_bytes(lvx.get_scans_raw(ctx, n - 1, 1, 16, info["W"]), want[n - 1:])
    again, _ = lvx.vlp16_unpack(ctx, *_args(c), **c["options"])                      # the counters start from zero on every call
    assert vc.same_bytes(again, want)


def test_unpack_leaves_the_context_scans_alone(ctx):
    a, b = vc.case("two_scans_2_and_3"), vc.case("three_packets")
    ctx.set_scans_vlp16(*_args(a))
    lvx.vlp16_unpack(ctx, *_args(b))
    assert vc.same_bytes(lvx.get_scans_raw(ctx, 0, 2, 16, 72), vc.restated("two_scans_2_and_3")[0])


@pytest.mark.parametrize("name", REFUSED)
def test_refused_call_keeps_the_earlier_scans(ctx, name):
    """77 packets in a scan / W too small: LVX_E_ARG from both entry points, and the scans set before still read back unchanged."""
    before = vc.case("two_scans_2_and_3")
    want, info = vc.restated("two_scans_2_and_3")
    ctx.set_scans_vlp16(*_args(before))
    c = vc.case(name)
    for call in (lambda: ctx.set_scans_vlp16(*_args(c)), lambda: lvx.vlp16_unpack(ctx, *_args(c))):
        with pytest.raises(lvx.LvxError) as e:
            call()
        assert e.value.code == lvx.E_ARG
    assert vc.same_bytes(lvx.get_scans_raw(ctx, 0, 2, 16, info["W"]), want)
    assert ctx.set_scans_vlp16(*_args(before)) == info                                # and the context still takes scans


def test_get_scans_raw_needs_scans_and_a_range_inside_them():
    g = lvx.Context(0)
    try:
        with pytest.raises(lvx.LvxError) as e:
            lvx.get_scans_raw(g, 0, 1, 16, 24)
        assert e.value.code == lvx.E_STATE
        g.set_scans_vlp16(*_args(vc.case("one_packet")))
        for first, n in ((0, 2), (1, 1), (-1, 1)):
            with pytest.raises(lvx.LvxError) as e:
                lvx.get_scans_raw(g, first, n, 16, 24)
            assert e.value.code == lvx.E_ARG
        assert lvx.get_scans_raw(g, 1, 0, 16, 24).size == 0
    finally:
        g.close()


@pytest.mark.parametrize("name", sorted(vc.ORGANISED))
def test_organised_overload_is_set_scans_of_the_host_records(ctx, name):
    xyzi, stamps = vc.organised_input(name)
    n, H, W = vc.ORGANISED[name]
    want = vc.restate_organised(xyzi, stamps)
    lvx.set_scans_organised(ctx, xyzi, stamps)
    got = lvx.get_scans_raw(ctx, 0, n, H, W)
    assert vc.same_bytes(got, want)
    lvx.set_scans(ctx, want, H, W)
    assert vc.same_bytes(lvx.get_scans_raw(ctx, 0, n, H, W), got)


def test_organised_overload_refuses_what_the_time_table_does_not_cover(ctx):
    for shape in ((1, 17, 24), (1, 16, 1825)):
        with pytest.raises(lvx.LvxError) as e:
            lvx.set_scans_organised(ctx, np.zeros(shape + (4,), np.float32), [1.0])
        assert e.value.code == lvx.E_ARG


def _room_scans(S, n_scans=8, n_packets=10):
    """The room of synth.make_sequence seen by a VLP-16 on its trajectory: per scan 16 x 240 ranges (synth._raycast_room from the LiDAR pose at each point's own time,
    the 16 laser elevations, 1.5 degrees per column) encoded as packets."""
    N = S["n_knots"]
    u = synth.unpack_state(S["state_true"], N, S["n_landmarks"])
    sp = synth.Spline(S["t0"], S["dt"], u["r3"], u["so3"])
    q_LI, p_LI = u["lidar"][:4], u["lidar"][4:7]
    cols = 24 * n_packets
    step = 36000 // (cols // 2)                                                       # per block
    az = np.deg2rad((1000 + step * (np.arange(cols) // 2) + (step // 2) * (np.arange(cols) % 2)) / 100.0)
    el = vlp16.VERT_ANGLE[vlp16.DSR_OF_ROW]
    E, A = np.meshgrid(el, az, indexing="ij")
    dirs_L = np.stack([np.cos(E) * np.cos(A), -np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)   # the stored point is (y, -x, z)
    row, col = np.meshgrid(np.arange(16), np.arange(cols), indexing="ij")
    stamps = S["t_start"] + 0.1 + 0.1 * np.arange(n_scans)
    packets = b""
    for s in range(n_scans):
        ts = (stamps[s] + row * 2.304e-6 + col * 55.296e-6).ravel()
        ek = sp.eval(ts)
        org = synth.qrot(ek["quat"], np.broadcast_to(p_LI, (len(ts), 3))) + ek["pos"]
        dW = synth.qrot(ek["quat"], synth.qrot(np.broadcast_to(q_LI, (len(ts), 4)), dirs_L))
        packets += vlp16.encode_packets(synth._raycast_room(dW, org).reshape(16, cols), 100, 1000, step)
    return packets, np.arange(n_scans + 1, dtype=np.int32) * n_packets, stamps


def test_packet_route_equals_host_unpacked_route_down_to_the_association():
    """8 scans x 10 packets: lvx_set_scans(host-unpacked records) on one context, lvx_set_scans_vlp16(packets) on another — the same raw scans, and one
    lvx_data_association at the same state gives the same plane count, the same point count and identical SurfelPoint arrays."""
    S = synth.make_sequence(seed=50)
    packets, offsets, stamps = _room_scans(S)
    records, info = vc.restate(offsets, packets, stamps)
    assert info["W"] == 240 and info["n_bad_headers"] == 0 and info["n_in_range"] > 0.95 * 8 * 16 * 240
    state = np.ascontiguousarray(S["state_true"], np.float64)
    a, b = lvx.Context(0), lvx.Context(0)
    try:
        res = []
        for g, route in ((a, "records"), (b, "packets")):
            g.set_spline(S["t0"], S["dt"], S["n_knots"])
            if route == "records":
                lvx.set_scans(g, records, 16, 240)
            else:
                assert g.set_scans_vlp16(packets, offsets, stamps) == info
            raw = lvx.get_scans_raw(g, 0, 8, 16, 240)
            npl, npt = lvx.data_association(g, state, S["t_map"])
            res.append((raw, npl, npt, lvx.get_surfel_points(g, npt)))
        print("planes %d, SurfelPoints %d" % (res[0][1], res[0][2]))
        assert vc.same_bytes(res[0][0], records) and vc.same_bytes(res[1][0], records)
        assert res[0][1] == res[1][1] and res[0][2] == res[1][2] and res[0][1] > 0 and res[0][2] > 0
        for k in ("pt", "pt_map", "t", "plane"):
            assert res[0][3][k].tobytes() == res[1][3][k].tobytes(), k
    finally:
        a.close(); b.close()
