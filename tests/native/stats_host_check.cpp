// tests/native/stats_host_check.cpp — TEST-ONLY host build of the value-only block evaluation behind the error statistics (lvi-exc_amd/csrc/lvx_stats.h), so that the
// CPU suite (-m "not gpu") can compare it with the oracle without a GPU.  Not a CPU fallback: nothing here is linked into liblvx.so.
// hs_evaluate walks an oracle Problem in the oracle's row order, writes the weighted residual rows and adds every block to its family's record (stat_block) in input
// order: records[LVX_NUM_FAM][ST_W].  Returns -(status bits) of the blocks that could not be evaluated.
#include <cstring>

#include "../../lvi-exc_amd/csrc/lvx_stats.h"
#include "../../oracle/orc_problem.hpp"

using namespace lvx;

extern "C" int hs_record_width() { return ST_W; }

extern "C" int hs_evaluate(const orc_problem* p, const double* state, double* residuals, double* records) {
  const int N = p->n_knots;
  const SplineRef sp{p->t0, p->dt, N, state, state + 3 * N};
  const double* si = state + 7 * N;
  ImuCal imu; imu.roll = si[8]; imu.pitch = si[9]; imu.ba = load_v3(si + 10); imu.bg = load_v3(si + 13); imu.tau = si[7];
  SensorCal lidar, cam;
  lidar.q = load_q(si + 16); lidar.p = load_v3(si + 20); lidar.tau = si[23];
  cam.q = load_q(si + 24); cam.p = load_v3(si + 28); cam.tau = si[31];
  const double* rho = si + 32;
  CamIntr ci; std::memset(&ci, 0, sizeof(ci));
  ci.fx = p->cam.fx; ci.fy = p->cam.fy; ci.cx = p->cam.cx; ci.cy = p->cam.cy; ci.k1 = p->cam.k1; ci.k2 = p->cam.k2; ci.p1 = p->cam.p1; ci.p2 = p->cam.p2; ci.k3 = p->cam.k3;
  ci.readout = p->cam.readout; ci.rows = p->cam.rows; ci.cols = p->cam.cols; ci.do_distortion = p->cam.do_distortion;
  ci.inv_K11 = p->cam.inv_K11; ci.inv_K13 = p->cam.inv_K13; ci.inv_K22 = p->cam.inv_K22; ci.inv_K23 = p->cam.inv_K23;
  const bool tlL = (p->locks & LVXO_LOCK_LIDAR_TAU) != 0, tlC = (p->locks & LVXO_LOCK_CAM_TAU) != 0;
  const double mto = p->sensor_max_time_offset;
  for (int k = 0; k < 6 * ST_W; ++k) records[k] = 0.0;
  int row = 0, err = 0;
  const int nI = static_cast<int>(p->imu_t.size());
  for (int i = 0; i < nI; ++i, row += 3) {
    const int e = stat_gyro(sp, imu, p->imu_t[i], load_v3(&p->imu_gyro[3 * i]), p->w_gyro, residuals + row);
    if (e) { err |= e; continue; }
    stat_block<3>(residuals + row, p->w_gyro, 0.0, records + 0 * ST_W);
  }
  if (!p->so3_only)
    for (int i = 0; i < nI; ++i, row += 3) {
      const int e = stat_accel(sp, imu, p->imu_t[i], load_v3(&p->imu_acc[3 * i]), p->w_acc, residuals + row);
      if (e) { err |= e; continue; }
      stat_block<3>(residuals + row, p->w_acc, 0.0, records + 1 * ST_W);
    }
  if (p->has_prior) {
    const int e = stat_prior(sp, p->prior_t, mkq(p->prior_q[0], p->prior_q[1], p->prior_q[2], p->prior_q[3]), p->prior_w, residuals + row);
    if (e) err |= e; else stat_block<1>(residuals + row, p->prior_w, 0.0, records + 2 * ST_W);
    row += 1;
  }
  StatHub hubL, hubC;
  stat_hub(sp, p->t_map, tlL, mto, lidar.tau, &hubL);
  stat_hub(sp, p->t_map, tlC, mto, cam.tau, &hubC);
  const int nS = static_cast<int>(p->surf_t.size());
  for (int i = 0; i < nS; ++i, row += 1) {
    const int e = stat_surfel(sp, hubL, lidar, tlL, mto, p->t_map, p->surf_t[i], load_v3(&p->surf_pt[3 * i]), load_v3(&p->planes[3 * p->surf_plane[i]]), p->w_surf, residuals + row);
    if (e) { err |= e; continue; }
    stat_block<1>(residuals + row, p->w_surf, p->huber_surf, records + 3 * ST_W);
  }
  const int nR = static_cast<int>(p->rep_lm.size());
  for (int i = 0; i < nR; ++i, row += 2) {
    const int lm = p->rep_lm[i];
    const int e = stat_reproj(sp, ci, cam, tlC, mto, p->lm_uv[2 * lm], p->lm_uv[2 * lm + 1], p->lm_t0[lm], p->rep_uv[2 * i], p->rep_uv[2 * i + 1], p->rep_t0[i], rho[lm], p->w_rep, residuals + row);
    if (e) { err |= e; continue; }
    stat_block<2>(residuals + row, p->w_rep, p->huber_rep, records + 4 * ST_W);
  }
  const int nC = static_cast<int>(p->cs_lm.size());
  for (int i = 0; i < nC; ++i, row += 1) {
    const int lm = p->cs_lm[i];
    const int e = stat_camsurf(sp, hubC, ci, cam, lidar, tlC, mto, p->t_map, p->lm_uv[2 * lm], p->lm_uv[2 * lm + 1], p->lm_t0[lm], rho[lm], load_v3(&p->planes[3 * p->cs_plane[i]]), p->w_cs,
                               residuals + row);
    if (e) { err |= e; continue; }
    stat_block<1>(residuals + row, p->w_cs, p->huber_cs, records + 5 * ST_W);
  }
  return -err;
}
