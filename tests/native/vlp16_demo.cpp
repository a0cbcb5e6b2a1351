// A C++ caller of the scan-ingestion ABI (include/lvx.h) and of lvx_host::Calibrator built from CalibrateInput::vlp16_* (lvi-exc_amd/host/lvx_calibrate.hpp).
// Usage: vlp16_demo in.bin packets.bin out.bin
// in.bin (doubles): t0 dt n_knots map_time | camera (12) | state | scan stamps | packet offsets, every array with its length in front; packets.bin: [n][1206] bytes.
// stdout:
//   `unpack <rc> <W> <packets> <in range> <out of range> <outside window> <bad headers>`   lvx_vlp16_unpack with the default options
//   `set <rc> <W> ...` the same fields                                                     lvx_set_scans_vlp16 on the same context
//   `refused <rc>` / `after <rc>`                                                          W = 24 with a longer scan, then lvx_get_scans_raw of the scans set before
//   `calibrator <n_scans> <H> <W> <packets> <in range>`                                    the Calibrator's own context, fed from CalibrateInput::vlp16_*
//   `association <planes> <points>`                                                        one lvx_data_association on that context at the given state
// out.bin: the records of lvx_vlp16_unpack | of lvx_get_scans_raw after lvx_set_scans_vlp16 | of lvx_get_scans_raw after the refused call | of the Calibrator's context.
#include <cstdio>
#include <fstream>

#include "lvx_calibrate.hpp"

static void line(const char* what, int rc, const lvx_vlp16_info& i) {
  std::printf("%s %d %d %lld %lld %lld %lld %lld\n", what, rc, (int)i.W, (long long)i.n_packets, (long long)i.n_in_range, (long long)i.n_out_of_range, (long long)i.n_outside_window,
              (long long)i.n_bad_headers);
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s in.bin packets.bin out.bin\n", argv[0]); return 2; }
  try {
    std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + argv[1]);
    const std::streamsize bytes = f.tellg(); f.seekg(0);
    std::vector<double> d((size_t)bytes / 8);
    f.read(reinterpret_cast<char*>(d.data()), bytes);
    size_t o = 0;
    auto next = [&]() { return d.at(o++); };
    auto vec = [&]() { const size_t n = (size_t)next(); std::vector<double> v(d.begin() + o, d.begin() + o + n); o += n; return v; };
    lvx_host::CalibrateInput in;
    in.t0 = next(); in.dt = next(); in.n_knots = (int)next(); in.map_time = next();
    in.camera.rows = (int)next(); in.camera.cols = (int)next(); in.camera.readout = next(); in.camera.fx = next(); in.camera.fy = next(); in.camera.cx = next(); in.camera.cy = next();
    in.camera.k1 = next(); in.camera.k2 = next(); in.camera.p1 = next(); in.camera.p2 = next(); in.camera.k3 = next();
    const std::vector<double> state = vec();
    in.vlp16_stamps = vec();
    for (double v : vec()) in.vlp16_packet_offsets.push_back((int32_t)v);
    std::ifstream g(argv[2], std::ios::binary | std::ios::ate);
    if (!g) throw std::runtime_error(std::string("cannot open ") + argv[2]);
    in.vlp16_packets.resize((size_t)g.tellg()); g.seekg(0);
    g.read(reinterpret_cast<char*>(in.vlp16_packets.data()), (std::streamsize)in.vlp16_packets.size());
    const int n = (int)in.vlp16_stamps.size();
    int longest = 0;
    for (int s = 0; s < n; ++s) longest = std::max(longest, in.vlp16_packet_offsets[s + 1] - in.vlp16_packet_offsets[s]);
    const size_t per_call = (size_t)n * 16 * 24 * longest;
    std::vector<lvx_point_xyzit> out(4 * per_call);

    // the plain ABI
    lvx_ctx* ctx = nullptr;
    if (lvx_create(&ctx, 0, 0) != LVX_OK) throw std::runtime_error("lvx_create failed");
    lvx_vlp16_options opt; lvx_vlp16_info info{};
    lvx_vlp16_default_options(&opt);
    int rc = lvx_vlp16_unpack(ctx, n, in.vlp16_packet_offsets.data(), in.vlp16_packets.data(), in.vlp16_stamps.data(), 0, &opt, out.data(), &info);
    line("unpack", rc, info);
    if (lvx_get_scans_raw(ctx, 0, n, out.data() + per_call) != LVX_E_STATE) throw std::runtime_error("lvx_vlp16_unpack must not set the context's scans");
    info = lvx_vlp16_info{};
    rc = lvx_set_scans_vlp16(ctx, n, in.vlp16_packet_offsets.data(), in.vlp16_packets.data(), in.vlp16_stamps.data(), 0, nullptr, &info);
    line("set", rc, info);
    if (rc == LVX_OK) rc = lvx_get_scans_raw(ctx, 0, n, out.data() + per_call);
    if (rc != LVX_OK) throw std::runtime_error(std::string("lvx_get_scans_raw: ") + lvx_last_error(ctx));
    std::printf("refused %d\n", lvx_set_scans_vlp16(ctx, n, in.vlp16_packet_offsets.data(), in.vlp16_packets.data(), in.vlp16_stamps.data(), 24, nullptr, nullptr));
    std::printf("after %d\n", lvx_get_scans_raw(ctx, 0, n, out.data() + 2 * per_call));
    lvx_destroy(ctx);

    // the Calibrator takes the packets instead of host-unpacked scans
    lvx_host::CalibrateOptions copt;
    copt.verbose = 0;
    lvx_host::Calibrator cal(0, in, copt);
    std::printf("calibrator %d %d %d %lld %lld\n", (int)cal.n_scans(), cal.scan_height(), cal.scan_width(), (long long)cal.vlp16_info().n_packets, (long long)cal.vlp16_info().n_in_range);
    if ((size_t)cal.n_scans() * cal.scan_height() * cal.scan_width() != per_call) throw std::runtime_error("the Calibrator's scans have another shape");
    if (lvx_get_scans_raw(cal.context(), 0, n, out.data() + 3 * per_call) != LVX_OK) throw std::runtime_error(std::string("lvx_get_scans_raw: ") + lvx_last_error(cal.context()));
    int32_t n_planes = 0, n_points = 0;
    rc = lvx_data_association(cal.context(), state.data(), in.map_time, nullptr, &n_planes, &n_points);
    if (rc != LVX_OK) throw std::runtime_error(std::string("lvx_data_association: ") + lvx_last_error(cal.context()));
    std::printf("association %d %d\n", (int)n_planes, (int)n_points);
    std::ofstream h(argv[3], std::ios::binary);
    h.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(lvx_point_xyzit)));
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
