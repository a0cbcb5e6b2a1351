// g++ build of lvi-exc_amd/csrc/lvx_render.h (the per-point math the rendering kernels run), for tests/test_render_host.py (against a numpy restatement) and
// tests/test_gpu_render.py (the kernels against it, byte for byte).  Built with -ffp-contract=off, as lvx_render.hip is.
#include "../../lvi-exc_amd/csrc/lvx_render.h"

using namespace lvx;

static RenderTable make_table(const double* q_L0, const double* p_L0, int n_images, const double* q_C, const double* p_C, const int32_t* valid) {
  RenderTable t;
  memset(&t, 0, sizeof(t));
  t.map_valid = 1; t.n_images = n_images;
  t.L0 = render_pose(mkq(q_L0[3], q_L0[0], q_L0[1], q_L0[2]), mk(p_L0[0], p_L0[1], p_L0[2]));
  for (int k = 0; k < n_images; ++k) {
    t.valid[k] = valid[k];
    if (valid[k]) t.cam[k] = render_pose(mkq(q_C[4 * k + 3], q_C[4 * k], q_C[4 * k + 1], q_C[4 * k + 2]), mk(p_C[3 * k], p_C[3 * k + 1], p_C[3 * k + 2]));
  }
  return t;
}

extern "C" {

int rh_record_size() { return (int)sizeof(lvx_point_xyzrgb); }

// quaternions x, y, z, w; xyzi4 [n][4] float; images [n_images][rows][pitch]; out [n] records, status [n]; returns the number of coloured points
long long rh_render(int n, const float* xyzi4, const double* q_L0, const double* p_L0, int n_images, const double* q_C, const double* p_C, const int32_t* valid, const lvx_pinhole* cam,
                    const uint8_t* images, int pitch, double z_min, double z_max, lvx_point_xyzrgb* out, int32_t* status) {
  if (n_images < 1 || n_images > LVX_RENDER_MAX_IMAGES) return -1;
  const RenderTable t = make_table(q_L0, p_L0, n_images, q_C, p_C, valid);
  long long colored = 0;
  for (int i = 0; i < n; ++i) {
    status[i] = render_point_images(xyzi4 + 4 * (size_t)i, t, *cam, images, pitch, z_min, z_max, out + i);
    colored += status[i] == RENDER_COLORED;
  }
  return colored;
}
// (depth, u, v) of every point in ONE image, for the tests' margin condition
void rh_render_uv(int n, const float* xyzi4, const double* q_L0, const double* p_L0, const double* q_C, const double* p_C, const lvx_pinhole* cam, double* zuv3) {
  const int32_t one = 1;
  const RenderTable t = make_table(q_L0, p_L0, 1, q_C, p_C, &one);
  for (int i = 0; i < n; ++i) {
    const v3 pc = render_to_camera(xyzi4 + 4 * (size_t)i, t.L0, t.cam[0]);
    double uv[2];
    render_project(*cam, pc, uv);
    zuv3[3 * (size_t)i] = pc.z; zuv3[3 * (size_t)i + 1] = uv[0]; zuv3[3 * (size_t)i + 2] = uv[1];
  }
}
void rh_overlay_chain(const double* q_LtoG, const double* p_LinG, const double* q_CtoG, const double* p_CinG, double* q_LtoC, double* p_LinC) {
  quat q; v3 p;
  overlay_chain(mkq(q_LtoG[3], q_LtoG[0], q_LtoG[1], q_LtoG[2]), mk(p_LinG[0], p_LinG[1], p_LinG[2]), mkq(q_CtoG[3], q_CtoG[0], q_CtoG[1], q_CtoG[2]), mk(p_CinG[0], p_CinG[1], p_CinG[2]), &q, &p);
  q_LtoC[0] = q.x; q_LtoC[1] = q.y; q_LtoC[2] = q.z; q_LtoC[3] = q.w; p_LinC[0] = p.x; p_LinC[1] = p.y; p_LinC[2] = p.z;
}
// pixel index (or -1) of every point; zuv3 (may be null): depth and uv of the point
void rh_overlay(int n, const float* xyzi4, const double* q_LtoC, const double* p_LinC, const lvx_pinhole* cam, int32_t* pixel, double* zuv3) {
  const quat q = mkq(q_LtoC[3], q_LtoC[0], q_LtoC[1], q_LtoC[2]); const v3 p = mk(p_LinC[0], p_LinC[1], p_LinC[2]);
  for (int i = 0; i < n; ++i) {
    const float* x = xyzi4 + 4 * (size_t)i;
    pixel[i] = overlay_point(x, q, p, *cam);
    if (zuv3) {
      const v3 pc = qrot(q, mk((double)x[0], (double)x[1], (double)x[2])) + p;
      double uv[2];
      render_project(*cam, pc, uv);
      zuv3[3 * (size_t)i] = pc.z; zuv3[3 * (size_t)i + 1] = uv[0]; zuv3[3 * (size_t)i + 2] = uv[1];
    }
  }
}

}  // extern "C"
