// tests/native/vxradius_host_check.cpp — TEST-ONLY host build of the voxel radius search (lvi-exc_amd/csrc/lvx_vxradius.h), so that the CPU suite (-m "not gpu") can hold
// it against the brute-force numpy restatement of tests/ndt_radius_cases.py without a GPU, and the GPU suite can hold k_vx_radius against the same restatement bit for bit.
// Not a CPU fallback: nothing here is linked into liblvx.so.  Built with g++ -O2 -ffp-contract=off, as the device translation unit is.
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_vxradius.h"

using namespace lvx;

// grid12 = min_b | max_b | div_b | mul of the build; leaf_key[l] = the linear cell index of leaf l (what the dense cell table of the device maps back to l).
// ids27, d2_27: [nq][27]; count: [nq].  Returns the number of cells of the table, -1 if a key lies outside it.
extern "C" long long vr_search(int nq, const float* xyzi4, float leaf, double radius, int min_pts, const int* grid12, int n_leaves, const int* leaf_key, const int* leaf_n,
                               const float* centroid3, int* ids27, float* d2_27, int* count) {
  VxrGrid g;
  for (int a = 0; a < 3; ++a) { g.min_b[a] = grid12[a]; g.max_b[a] = grid12[3 + a]; g.mul[a] = grid12[9 + a]; }
  const long long cells = (long long)grid12[6] * grid12[7] * grid12[8];
  std::vector<int> table((size_t)(cells > 0 ? cells : 1), -1);
  for (int l = 0; l < n_leaves; ++l) {
    if (leaf_key[l] < 0 || leaf_key[l] >= cells) return -1;
    table[(size_t)leaf_key[l]] = l;
  }
  const int none_n = 0; const float none_c[3] = {0.f, 0.f, 0.f};   // a grid without a leaf: slot 0 of the leaf arrays is still read (and never used)
  for (int i = 0; i < nq; ++i)
    count[i] = vxr_search(xyzi4[4 * (size_t)i], xyzi4[4 * (size_t)i + 1], xyzi4[4 * (size_t)i + 2], leaf, radius, min_pts, g, table.data(), n_leaves ? leaf_n : &none_n,
                          n_leaves ? centroid3 : none_c, ids27 + (size_t)i * LVX_VXR_CELLS, d2_27 + (size_t)i * LVX_VXR_CELLS);
  return cells;
}
