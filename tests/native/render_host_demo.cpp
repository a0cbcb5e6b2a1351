// The host-side pieces of the coloured map / overlay in lvi-exc_amd/host/lvx_calibrate.hpp that need no device: RenderMap's candidate images, the scan -> image rule of
// ReprojectPointCloudToImage, the ASCII PCD writer.  Prints what tests/test_render_host.py compares.
#include <cstdio>

#include "lvx_calibrate.hpp"

int main(int argc, char** argv) {
  using namespace lvx_host;
  if (argc < 2) return 2;
  for (size_t n : {size_t(5), size_t(50), size_t(55), size_t(200), size_t(1000)}) {
    std::printf("candidates %zu:", n);
    for (int32_t i : RenderCandidates(n)) std::printf(" %d", i);
    std::printf("\n");
  }
  std::printf("match:");
  for (int32_t i : MatchScanImages({1.0, 2.0, 3.0}, {0.99, 1.0, 1.04, 1.049, 2.06, 3.01})) std::printf(" %d", i);
  std::printf("\n");
  std::vector<lvx_point_xyzrgb> cloud(3);
  cloud[1].x = 1.5f; cloud[1].y = -2.25f; cloud[1].z = 0.1f;
  cloud[2].x = 3.f; cloud[2].y = 4.f; cloud[2].z = 5.f; cloud[2].r = cloud[2].g = cloud[2].b = 200; cloud[2].a = 255;
  return WritePcdAscii(argv[1], cloud) ? 0 : 1;
}
