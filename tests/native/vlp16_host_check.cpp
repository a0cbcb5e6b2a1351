// tests/native/vlp16_host_check.cpp — TEST-ONLY host build of the VLP-16 scan ingestion (lvi-exc_amd/csrc/lvx_vlp16.h), so that the CPU suite (-m "not gpu") can hold the
// per-record function the kernels run against the numpy restatement of tests/vlp16_cases.py without a GPU, byte for byte.  Not a CPU fallback: nothing here is linked
// into liblvx.so.  Built with g++ -O2 -ffp-contract=off, as the device translation unit is.
// With -DVLP16_HOST_CHECK_MAIN it is a program of its own (the build to run under -fsanitize=address,undefined): a few scans with every edge of the packet layout,
// "vlp16_host_check: OK" and exit status 0 on success.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_vlp16.h"

using namespace lvx;

extern "C" void vlp16_tables(float* cos_rot, float* sin_rot, float* cos_vert, float* sin_vert) { vlp16_build_tables(cos_rot, sin_rot, cos_vert, sin_vert); }

// VelodyneCorrection::unpack_scan per scan, in the loop order of the reference.  out: [n_scans][16][W] records, W from vlp16_width (returned; -1, -2, -3 = its
// errors, nothing written).  info5: packets, in range, out of range, outside the window, bad headers.
extern "C" int vlp16_unpack_host(int n_scans, const int32_t* off, const uint8_t* packets, const double* stamp, int W_in, double min_range, double max_range, int min_angle,
                                 int max_angle, int out_capacity, VlpPoint* out, long long* info5) {
  int W = 0;
  const int e = n_scans > 0 ? vlp16_width(n_scans, off, W_in, &W) : 0;
  if (e) return -e;
  if ((long long)n_scans * LVX_VLP16_ROWS * W > out_capacity) return -4;
  std::vector<float> t(2 * LVX_VLP16_ROT + 32);
  vlp16_build_tables(t.data(), t.data() + LVX_VLP16_ROT, t.data() + 2 * LVX_VLP16_ROT, t.data() + 2 * LVX_VLP16_ROT + 16);
  const VlpTables T = {t.data(), t.data() + LVX_VLP16_ROT, t.data() + 2 * LVX_VLP16_ROT, t.data() + 2 * LVX_VLP16_ROT + 16};
  const VlpOptions o = {min_range, max_range, min_angle, max_angle};
  for (int k = 0; k < 5; ++k) info5[k] = 0;
  for (int s = 0; s < n_scans; ++s) {
    VlpPoint* cloud = out + (size_t)s * LVX_VLP16_ROWS * W;
    const int np = off[s + 1] - off[s];
    for (int r = 0; r < LVX_VLP16_ROWS; ++r)
      for (int w = 0; w < W; ++w) cloud[(size_t)r * W + w] = w < LVX_VLP16_COLS * np ? vlp16_zero() : vlp16_padding();
    int block_counter = 0;
    for (int i = 0; i < np; ++i) {
      const uint8_t* packet = packets + (size_t)(off[s] + i) * LVX_VLP16_BYTES;
      ++info5[0];
      for (int block = 0; block < LVX_VLP16_BLOCKS; ++block, ++block_counter) {
        if (vlp16_bad_header(packet, block)) ++info5[4];
        for (int firing = 0; firing < 2; ++firing)
          for (int dsr = 0; dsr < 16; ++dsr) {
            VlpPoint p; int row, col;
            const int cls = vlp16_point(packet, block, firing, dsr, block_counter, stamp[s], T, o, &p, &row, &col);
            ++info5[1 + cls];
            cloud[(size_t)row * W + col] = p;
          }
      }
    }
  }
  return W;
}

extern "C" void vlp16_organised_host(int n_scans, int H, int W, const float* xyzi4, const double* stamp, VlpPoint* out) {
  for (int s = 0; s < n_scans; ++s)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const size_t i = ((size_t)s * H + h) * W + w;
        out[i] = vlp16_organised_point(xyzi4 + 4 * i, h, w, stamp[s]);
      }
}

#ifdef VLP16_HOST_CHECK_MAIN
static void put16(uint8_t* p, unsigned v) { p[0] = (uint8_t)(v & 255); p[1] = (uint8_t)(v >> 8); }
int main() {
  // scans of 1, 0 and 76 packets; rotations that wrap and exceed 36000, distances 0 / 299 / 300 / 65535, one wrong header
  const int32_t off[4] = {0, 1, 1, 77};
  const double stamp[3] = {10.0, 20.0, 30.0};
  std::vector<uint8_t> pk((size_t)77 * LVX_VLP16_BYTES, 0);
  const unsigned dist[4] = {0, 299, 300, 65535};
  for (int p = 0; p < 77; ++p)
    for (int b = 0; b < 12; ++b) {
      uint8_t* blk = pk.data() + (size_t)p * LVX_VLP16_BYTES + 100 * b;
      put16(blk, (p == 3 && b == 5) ? 0xddff : 0xeeff);
      put16(blk + 2, (unsigned)((35000 + 40 * (12 * p + b)) % (p == 7 ? 65536 : 36000)));
      for (int k = 0; k < 32; ++k) { put16(blk + 4 + 3 * k, dist[(p + b + k) & 3]); blk[4 + 3 * k + 2] = (uint8_t)(k * 8); }
    }
  int bad = 0;
  for (int window = 0; window < 3; ++window) {
    const int lo = window == 0 ? 0 : (window == 1 ? 1000 : 30000), hi = window == 0 ? 36000 : (window == 1 ? 20000 : 500);
    std::vector<VlpPoint> out((size_t)3 * 16 * 1824);
    long long info[5];
    const int W = vlp16_unpack_host(3, off, pk.data(), stamp, 0, 0.6, 150.0, lo, hi, (int)out.size(), out.data(), info);
    if (W != 1824 || info[0] != 77 || info[1] + info[2] + info[3] != 77 * 384 || info[4] != 1 || (window == 0 && info[3] != 0) || (window > 0 && info[3] == 0)) ++bad;
    if (out[0].timestamp != (window == 0 ? 10.0 + vlp16_time(0, 0) : out[0].timestamp) || out[(size_t)16 * 1824 + 5].timestamp != 0.0) ++bad;   // scan 1 is all padding
  }
  const int32_t too_long[2] = {0, 77};
  long long info[5]; VlpPoint one;
  if (vlp16_unpack_host(1, too_long, pk.data(), stamp, 0, 0.6, 150.0, 0, 36000, 1, &one, info) != -2) ++bad;
  if (vlp16_unpack_host(3, off, pk.data(), stamp, 24, 0.6, 150.0, 0, 36000, 1, &one, info) != -3) ++bad;
  std::vector<float> cloud((size_t)15 * 24 * 4, 1.5f);
  std::vector<VlpPoint> rec((size_t)15 * 24);
  vlp16_organised_host(1, 15, 24, cloud.data(), stamp, rec.data());
  if (rec[(size_t)14 * 24 + 23].timestamp != 10.0 + vlp16_time(14, 23) || rec[7].x != 1.5f) ++bad;
  std::printf(bad ? "vlp16_host_check: FAILED (%d)\n" : "vlp16_host_check: OK\n", bad);
  return bad ? 1 : 0;
}
#endif
