// lvx_vxradius.h — radius search over the leaf centroids of the voxel covariance grid, host- and device-callable: VoxelGridCovariance::radiusSearch
// (src/ndt_omp/include/pclomp/voxel_grid_covariance_omp.h:473-502), the neighbour search of pclomp::KDTREE (ndt_omp_impl.hpp:233-236) with radius = resolution.
// The kernels of lvx_upstream.hip (k_vx_radius, k_ndt_derivatives<0, .>, k_ndt_hessian<0>) call these functions one lane per query; tests/native/vxradius_host_check.cpp
// builds them with g++ (-ffp-contract=off, as lvx_upstream.hip is built) and the suites compare ids, order, counts and the bits of the distances.
//
// No tree.  The reference's kd-tree holds ONE point per leaf, the leaf's float centroid, and a centroid lies inside its own voxel; a centroid within r <= leaf size of a
// query therefore sits in one of the 27 cells {-1, 0, 1}^3 around the query's cell.  For one query q = (x, y, z) and one radius:
//   members     every leaf that had at least min_points_per_voxel points when the grid was built: stored nr_points >= min_pts, or nr_points == -1.  The reference pushes
//               the centroid into voxel_centroids_ (voxel_grid_covariance_omp_impl.hpp:301-330) BEFORE the eigenvalue test (:341-345) or the infinity test (:364-368) can
//               reject the leaf: a rejected leaf stays in the tree, and it IS returned here — the cell lookups (getNeighborhoodAtPoint*) never return it.
//   candidates  the member leaves of the 27 cells around (floorf(x / leaf), floorf(y / leaf), floorf(z / leaf)) — the cell as k_ndt_derivatives computes it; a cell
//               outside the grid's box is skipped, never wrapped into the table
//   distance    FLANN's L2_Simple<float>: d = q - c per axis in float (c = the stored float centroid), d2 = (dx dx + dy dy) + dz dz in float
//   hit         d2 < r2, r2 = (float)(radius * radius), the product formed in double.  The strict < is what FLANN's RadiusResultSet is understood to do (neither FLANN nor PCL
//               is available to this project's builds to confirm it); the project's cases keep every centroid at least 4 ulp of r2 away from the edge, so no test
//               depends on the choice
//   order       ascending d2; equal d2 by ascending leaf index (FLANN leaves ties unspecified: this is the project's rule)
//   output      count in 0 .. 27, then count (leaf, d2).  A query with a non-finite coordinate has count 0, the rule of the cell lookups; so has one whose cell index
//               leaves +-2^30 (no grid reaches there: a grid has fewer than 2^31 cells)
// DEVIATION 1 (the 27 cells): the grid build computes a point's cell in float, so a centroid within an ulp of a cell face can be stored one cell away from where the
// division above puts it; at a distance of about r such a leaf can then sit two cells from the query, where the reference's tree finds it and the 27 cells do not.
// DEVIATION 2 (ties): see `order`.
//
// Selection without a dynamically indexed array (which the device would keep in scratch memory): a candidate is ONE 64-bit key, the bits of d2 (a non-negative float:
// its bit pattern orders as the value) above the leaf index; a miss is VXR_NONE.  The k-th result is the smallest key not below (the previous result + 1): 27 compares
// per result over 27 fixed slots.
#pragma once
#include <string.h>

#include "lvx_math.h"

namespace lvx {

#define LVX_VXR_CELLS 27
#define VXR_NONE 0xffffffffffffffffull

struct VxrGrid { int min_b[3], max_b[3], mul[3]; };   // getMinBoxCoordinates, getMaxBoxCoordinates, getDivisionMultiplier of the build

LVX_HD float vxr_r2(double radius) { return (float)(radius * radius); }
LVX_HD bool vxr_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }
LVX_HD bool vxr_member(int nr_points, int min_pts) { return nr_points >= min_pts || nr_points == -1; }
LVX_HD unsigned long long vxr_key(float d2, int leaf) { unsigned u; memcpy(&u, &d2, 4); return ((unsigned long long)u << 32) | (unsigned)leaf; }
LVX_HD int vxr_key_leaf(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }
LVX_HD float vxr_key_d2(unsigned long long key) { const unsigned u = (unsigned)(key >> 32); float f; memcpy(&f, &u, 4); return f; }

// The 27 candidates of one query as keys (VXR_NONE = no hit in that cell).  Three passes, so that the device has the 27 cell probes in flight together, then the 27
// leaf counts, then the centroids (as k_vx_lookup_rel: probe by probe the loads would queue up one behind the other).  cells = the dense cell table (leaf or -1),
// nr_points and centroid3 per leaf.
LVX_HD void vxr_candidates(float x, float y, float z, float leaf, float r2, int min_pts, const VxrGrid& g, const int* cells, const int* nr_points, const float* centroid3,
                           unsigned long long key[LVX_VXR_CELLS]) {
  const float q[3] = {x, y, z};
  const float cf[3] = {floorf(x / leaf), floorf(y / leaf), floorf(z / leaf)};
  bool ok = vxr_finite(x) && vxr_finite(y) && vxr_finite(z);
  for (int a = 0; a < 3; ++a) ok = ok && fabsf(cf[a]) < 1073741824.0f;
  const int ijk[3] = {ok ? (int)cf[0] : 0, ok ? (int)cf[1] : 0, ok ? (int)cf[2] : 0};
  int li[LVX_VXR_CELLS];
#pragma unroll
  for (int s = 0; s < LVX_VXR_CELLS; ++s) {
    const int d[3] = {s % 3 - 1, (s / 3) % 3 - 1, s / 9 - 1};
    bool in = ok;
    int at = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int c = ijk[a] + d[a];   // |ijk| < 2^30: no overflow
      in = in && c >= g.min_b[a] && c <= g.max_b[a];
      at += (c - g.min_b[a]) * g.mul[a];
    }
    const int l0 = cells[in ? at : 0];
    li[s] = in ? l0 : -1;
  }
  bool mem[LVX_VXR_CELLS];
#pragma unroll
  for (int s = 0; s < LVX_VXR_CELLS; ++s) { const int n = nr_points[li[s] >= 0 ? li[s] : 0]; mem[s] = li[s] >= 0 && vxr_member(n, min_pts); }
#pragma unroll
  for (int s = 0; s < LVX_VXR_CELLS; ++s) {
    const float* c = centroid3 + 3 * (size_t)(mem[s] ? li[s] : 0);
    const float dx = q[0] - c[0], dy = q[1] - c[1], dz = q[2] - c[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    key[s] = (mem[s] && d2 < r2) ? vxr_key(d2, li[s]) : VXR_NONE;
  }
}

// the smallest key >= lo, or VXR_NONE.  First result: lo = 0; the one behind a result k: lo = k + 1.
LVX_HD unsigned long long vxr_next(const unsigned long long key[LVX_VXR_CELLS], unsigned long long lo) {
  unsigned long long best = VXR_NONE;
#pragma unroll
  for (int s = 0; s < LVX_VXR_CELLS; ++s) { const unsigned long long k = key[s]; best = (k >= lo && k < best) ? k : best; }
  return best;
}

// radiusSearch of one query: ids27 and d2_27 (either may be NULL) hold the count results in order, then -1 / +infinity; returns the count
LVX_HD int vxr_search(float x, float y, float z, float leaf, double radius, int min_pts, const VxrGrid& g, const int* cells, const int* nr_points, const float* centroid3,
                      int* ids27, float* d2_27) {
  unsigned long long key[LVX_VXR_CELLS];
  vxr_candidates(x, y, z, leaf, vxr_r2(radius), min_pts, g, cells, nr_points, centroid3, key);
  const unsigned inf_bits = 0x7f800000u;
  float inf; memcpy(&inf, &inf_bits, 4);
  int count = 0;
  unsigned long long lo = 0;
  for (int k = 0; k < LVX_VXR_CELLS; ++k) {
    const unsigned long long b = vxr_next(key, lo);
    const bool hit = b != VXR_NONE;
    if (ids27) ids27[k] = hit ? vxr_key_leaf(b) : -1;
    if (d2_27) d2_27[k] = hit ? vxr_key_d2(b) : inf;
    count += hit ? 1 : 0;
    lo = hit ? b + 1 : VXR_NONE;
  }
  return count;
}

}  // namespace lvx
