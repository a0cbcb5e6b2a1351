// lvx_calibration_covariance_shared from C++ with the ranks as threads of ONE process: every rank owns a context with its own sequence, the reduction callback sums
// the ranks' buffers behind a barrier, and every rank's record is printed raw and as lvx_host::FormatJointCalibrationUncertainty prints it.
// Usage: joint_cov_demo in.bin        in.bin (doubles, tests/test_gpu_joint_cov.py::_write_ranks): n_ranks, then per rank
//   t0 dt n_knots locks | camera rows cols readout fx fy cx cy k1 k2 p1 p2 k3 | w_gyro w_acc t_map huber_surf w_surf huber_rep w_rep |
//   counted vectors: state, t_imu, gyro, acc, planes, surf_pt, surf_t, surf_plane, lm_uv, lm_t0, rep_lm, rep_uv, rep_t0
// stdout, per rank:
//   RANK <r> world <w> n_free <k> radius <R> free <c ...>
//   SIGMA <22 values, %.17g>
//   SLOTS <n_shared_free values>
//   EIG <n_shared_free values>
//   VEC <n_shared_free^2 values, row-major>
//   OWN <14 diagonal values of own_info>
//   the formatted lines
//   END
#include <condition_variable>
#include <cstdio>
#include <fstream>
#include <mutex>
#include <thread>

#include "lvx_calibrate.hpp"

struct Exchange {   // in-place sum over the ranks, every rank calls reduce() once per collective
  explicit Exchange(int n) : world(n) {}
  int world, arrived = 0, left = 0; long gen = 0;
  std::vector<double> sum;
  std::mutex m; std::condition_variable cv;
  void reduce(double* buf, int n) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return left == 0; });   // the previous collective has been read by everybody
    if (arrived == 0) sum.assign((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) sum[(size_t)i] += buf[i];
    const long g = gen;
    if (++arrived == world) { ++gen; left = world; cv.notify_all(); }
    else cv.wait(lk, [&] { return gen != g; });
    for (int i = 0; i < n; ++i) buf[i] = sum[(size_t)i];
    if (--left == 0) { arrived = 0; cv.notify_all(); }
  }
};
static int allreduce(void* user, double* buf, int n, int op) {
  if (op != LVX_REDUCE_SUM) return 1;
  static_cast<Exchange*>(user)->reduce(buf, n);
  return 0;
}

struct Rank { lvx_ctx* ctx = nullptr; std::vector<double> state; lvx_joint_calib_cov rec; int rc = 0; std::string err; };

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s ranks.bin\n", argv[0]); return 2; }
  std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const std::streamsize nbytes = f.tellg(); f.seekg(0);
  std::vector<double> d((size_t)nbytes / 8);
  f.read(reinterpret_cast<char*>(d.data()), nbytes);
  size_t o = 0;
  auto next = [&]() { return d.at(o++); };
  auto vec = [&]() { const size_t n = (size_t)next(); if (o + n > d.size()) throw std::runtime_error("truncated file"); std::vector<double> v(d.begin() + o, d.begin() + o + n); o += n; return v; };
  auto ivec = [&]() { const std::vector<double> v = vec(); return std::vector<int32_t>(v.begin(), v.end()); };
  try {
    const int world = (int)next();
    std::vector<Rank> ranks((size_t)world);
    for (Rank& rk : ranks) {
      auto check = [&](int rc) { if (rc != LVX_OK) throw std::runtime_error(std::string(rk.ctx ? lvx_last_error(rk.ctx) : "lvx error") + " (" + std::to_string(rc) + ")"); };
      check(lvx_create(&rk.ctx, 0, 0));
      const double t0 = next(), dt = next(); const int n_knots = (int)next(); const uint32_t locks = (uint32_t)next();
      lvx_pinhole cam;
      cam.rows = (int)next(); cam.cols = (int)next(); cam.readout = next(); cam.fx = next(); cam.fy = next(); cam.cx = next(); cam.cy = next();
      cam.k1 = next(); cam.k2 = next(); cam.p1 = next(); cam.p2 = next(); cam.k3 = next();
      const double w_gyro = next(), w_acc = next(), t_map = next(), huber_surf = next(), w_surf = next(), huber_rep = next(), w_rep = next();
      rk.state = vec();
      const std::vector<double> t_imu = vec(), gyro = vec(), acc = vec(), planes = vec(), surf_pt = vec(), surf_t = vec();
      const std::vector<int32_t> surf_plane = ivec();
      const std::vector<double> lm_uv = vec(), lm_t0 = vec();
      const std::vector<int32_t> rep_lm = ivec();
      const std::vector<double> rep_uv = vec(), rep_t0 = vec();
      check(lvx_set_spline(rk.ctx, t0, dt, n_knots));
      check(lvx_set_camera(rk.ctx, &cam));
      check(lvx_set_imu(rk.ctx, (int)t_imu.size(), t_imu.data(), gyro.data(), acc.data(), w_gyro, w_acc));
      check(lvx_set_planes(rk.ctx, (int)planes.size() / 3, planes.data()));
      check(lvx_set_surfel(rk.ctx, (int)surf_t.size(), surf_pt.data(), surf_t.data(), surf_plane.data(), t_map, huber_surf, w_surf));
      check(lvx_set_landmarks(rk.ctx, (int)lm_t0.size(), lm_uv.data(), lm_t0.data()));
      check(lvx_set_reproj(rk.ctx, (int)rep_lm.size(), rep_lm.data(), rep_uv.data(), rep_t0.data(), huber_rep, w_rep));
      check(lvx_set_locks(rk.ctx, locks));
      if ((int)rk.state.size() != lvx_state_size(rk.ctx)) throw std::runtime_error("state size");
    }
    Exchange ex(world);
    std::vector<std::thread> th;
    for (Rank& rk : ranks) th.emplace_back([&rk, &ex] {
      double cost = 0.0;
      rk.rc = lvx_evaluate(rk.ctx, rk.state.data(), LVX_EVAL_COST | LVX_EVAL_NORMAL_EQ, &cost, nullptr);
      lvx_calib_cov_options co; lvx_calib_cov_default_options(&co);
      // (a rank whose evaluation failed still calls: its missing evaluation is voted and every rank returns)
      const int rc = lvx_calibration_covariance_shared(rk.ctx, &co, allreduce, &ex, &rk.rec);
      if (rk.rc == LVX_OK) rk.rc = rc;
      if (rk.rc != LVX_OK) rk.err = lvx_last_error(rk.ctx);
    });
    for (auto& t : th) t.join();
    int bad = 0;
    for (int r = 0; r < world; ++r) {
      const Rank& rk = ranks[(size_t)r];
      if (rk.rc != LVX_OK) { std::fprintf(stderr, "rank %d: lvx error %d: %s\n", r, rk.rc, rk.err.c_str()); bad = 3; continue; }
      const lvx_joint_calib_cov& c = rk.rec;
      const int ns = c.n_shared_free;
      std::printf("RANK %d world %d n_free %d radius %.17g free", r, (int)c.world, (int)c.n_free, c.radius);
      for (int k = 0; k < c.n_free; ++k) std::printf(" %d", (int)c.free_index[k]);
      std::printf("\nSIGMA");
      for (int k = 0; k < 22; ++k) std::printf(" %.17g", c.sigma[k]);
      std::printf("\nSLOTS");
      for (int k = 0; k < ns; ++k) std::printf(" %d", (int)c.shared_free_slot[k]);
      std::printf("\nEIG");
      for (int k = 0; k < ns; ++k) std::printf(" %.17g", c.info_eig[k]);
      std::printf("\nVEC");
      for (int i = 0; i < ns; ++i) for (int k = 0; k < ns; ++k) std::printf(" %.17g", c.info_vec[i * 14 + k]);
      std::printf("\nOWN");
      for (int k = 0; k < 14; ++k) std::printf(" %.17g", c.own_info[k * 14 + k]);
      std::printf("\n%sEND\n", lvx_host::FormatJointCalibrationUncertainty(c).c_str());
    }
    for (Rank& rk : ranks) lvx_destroy(rk.ctx);
    return bad;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 3; }
}
