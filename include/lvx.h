/* lvx.h — C ABI of the MI355X-native evaluator for LVI-ExC's continuous-time calibration solve.
 *
 * Drop-in boundary.  The reference has no FFI layer; its seam is the Ceres cost-functor surface that every
 * Kontiki measurement builds in AddToEstimator and that ceres::Solve drives per residual block
 * (reference: src/lvi_exc/thirdparty/Kontiki/include/kontiki/trajectory_estimator.h:38-74).  A per-block FFI
 * would serialise the GPU, so this ABI is BATCHED: the host hands over whole measurement arrays once
 * (lvx_set_*: what TrajectoryManagerLVI::add*Measurement loops build, src/lvi_exc/src/core/trajectory_manager_lvi.cpp:464-606)
 * and then asks for one evaluation of all residual blocks + Jacobians + J^T J / J^T r per iterate
 * (lvx_evaluate: what ceres::Problem::Evaluate does through DynamicAutoDiffCostFunction::Evaluate).
 * INTEGRATION.md shows the reference-side binding.
 *
 * Conventions: every pointer is a HOST pointer unless the name ends in _d; the caller owns host buffers,
 * the context owns device buffers; a context is bound to one GPU and is not thread-safe; no exceptions
 * cross the ABI — the reference's std::range_error / std::runtime_error become LVX_E_RANGE / LVX_E_NONUNIT_QUAT.
 * All arithmetic is FP64.  Quaternions are stored (x, y, z, w) like Eigen::Map<Quaternion>
 * (kontiki/trajectories/spline_base.h:118-127, kontiki/sensors/sensors.h:36-43).
 *
 * STATE vector (flat doubles), n = n_knots, L = n_landmarks:
 *   r3_cp[n][3] | so3_cp[n][4] | imu{q4,p3,tau,roll,pitch,b_a3,b_g3} (16) | lidar{q4,p3,tau} (8) | cam{q4,p3,tau} (8) | rho[L]
 * TANGENT vector (what delta / gradient / normal equations are expressed in):
 *   knot k: 6k..6k+2 position, 6k+3..6k+5 rotation (ceres::EigenQuaternionParameterization delta)
 *   | 6n + {0 roll, 1 pitch, 2..4 b_a, 5..7 b_g, 8..10 lidar theta, 11..13 lidar p, 14 lidar tau,
 *           15..17 cam theta, 18..20 cam p, 21 cam tau} | 6n + 22 + l : rho_l
 */
#ifndef LVX_H
#define LVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lvx_ctx lvx_ctx;

/* error codes (0 = success) */
#define LVX_OK 0
#define LVX_E_RANGE (-1)         /* std::range_error: time outside the spline / unordered spans (spline_base.h:207-221, trajectory_estimator.h:102-127) */
#define LVX_E_NONUNIT_QUAT (-2)  /* std::runtime_error in logq (kontiki/math/quaternion_math.h:19-23) */
#define LVX_E_ALLOC (-3)
#define LVX_E_HIP (-4)
#define LVX_E_COMM (-5)          /* the host-supplied all-reduce callback failed (lvx_lm_solve_shared) */
#define LVX_E_RCCL LVX_E_COMM
#define LVX_E_ARG (-6)
#define LVX_E_STATE (-7)         /* call order (e.g. evaluate before set_spline) */
#define LVX_E_NODEVICE (-8)      /* no HIP device: the product path never falls back to the CPU */
#define LVX_E_NOTPD (-9)         /* damped normal equations not positive definite */

/* lock mask: mirrors Lock / IsLocked flags (kontiki/sensors/sensors.h:113-135, kontiki/trajectories/trajectory.h:149-155,
 * kontiki/sensors/constant_bias_imu.h:68-81, kontiki/sfm/landmark.h Lock).  IMU q_rel/p_rel/tau are always constant, as in the reference. */
#define LVX_LOCK_TRAJ (1u << 0)
#define LVX_LOCK_R3 (1u << 1)        /* R3 spline absent: TrajectoryEstimator<UniformSO3SplineTrajectory> of Solve #0 */
#define LVX_LOCK_LIDAR_Q (1u << 2)
#define LVX_LOCK_LIDAR_P (1u << 3)
#define LVX_LOCK_LIDAR_TAU (1u << 4)
#define LVX_LOCK_CAM_Q (1u << 5)
#define LVX_LOCK_CAM_P (1u << 6)
#define LVX_LOCK_CAM_TAU (1u << 7)
#define LVX_LOCK_ACC_BIAS (1u << 8)
#define LVX_LOCK_GYRO_BIAS (1u << 9)
#define LVX_LOCK_LANDMARKS (1u << 10)

/* lvx_evaluate `what` bits */
#define LVX_EVAL_COST (1u << 0)
#define LVX_EVAL_RESIDUALS (1u << 1)
#define LVX_EVAL_NORMAL_EQ (1u << 2)
#define LVX_EVAL_JACOBIAN (1u << 3)   /* debug: per-row (cols, vals) in tangent coordinates, see lvx_get_jacobian */
#define LVX_EVAL_JACOBIAN_BLOCKS (1u << 4)   /* per-block Jacobians in the family's compact record, from the fused kernels: lvx_get_jacobian_blocks */

/* residual families, in the order residual rows are laid out */
#define LVX_FAM_GYRO 0
#define LVX_FAM_ACCEL 1
#define LVX_FAM_PRIOR 2
#define LVX_FAM_SURFEL 3
#define LVX_FAM_REPROJ 4
#define LVX_FAM_CAMSURF 5
#define LVX_NUM_FAM 6
#define LVX_FAM_LIDAR_POS 6   /* LiDAR odometry position blocks (lvx_set_lidar_poses).  NOT counted in LVX_NUM_FAM: the six families of the default schedule keep their arrays */

#define LVX_JAC_WIDTH 64   /* columns per row of the debug Jacobian */

/* PinholeMeta (kontiki/sensors/pinhole_camera.h:20-41) + CameraMeta (kontiki/sensors/camera.h:25-29) */
typedef struct lvx_pinhole {
  int32_t rows, cols;
  double readout;
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
} lvx_pinhole;

/* layout of the structured normal equations kept on the device */
typedef struct lvx_layout {
  int32_t n_knots, n_landmarks, n_tangent;
  int32_t n_band;      /* variables in the banded part (non-hub knots interleaved with landmarks) */
  int32_t bandwidth;   /* scalar half-bandwidth of the banded part */
  int32_t n_border;    /* dense border: hub knots (6 each) then the 22 calibration scalars */
  int32_t border_ld;   /* leading dimension of the border block as exported by lvx_export_border_d (n_border + pseudo-pose rows) */
  int32_t n_hub_knots, hub_knot0;
  int64_t n_blocks;    /* residual blocks per evaluation */
  int64_t n_residuals; /* residual rows per evaluation */
  int32_t exact_fallback; /* 1 once an evaluation needed the per-segment kernels for EVERYTHING (more rows than the fallback lists hold, |tau_imu| >= dt): they are used from then on */
  int32_t solver_fallbacks; /* LM steps so far whose cyclic-reduction factorisation lost positive definiteness and were redone by the sequential band Cholesky */
  int32_t fallback_rows;    /* blocks of the last evaluation whose cost was read that the fused kernels handed, row by row, to the exact per-segment kernel (a control-point
                             * pair beyond 0.8 rad, the merged map-time segment corner): the pass stays on the fused kernels for everything else */
  int32_t solver_separators; /* the last solver plan: separators of the leaves + separators elimination of the band (a band that is narrow except for isolated wide runs:
                              * csrc/lvx_nd.h); 0: the uniform block chain (block cyclic reduction with b = bandwidth) runs */
  int32_t solver_leaves;     /* ... and its leaves (narrow stretches and wide runs) */
  int32_t rep_groups;        /* (reference window, observation window) groups of the reprojection cross-term kernel in the current layout (at most 32 blocks each) */
  int32_t lm_groups;         /* groups of the landmark elimination (at most 32 landmarks whose first band positions lie within 24 scalars) */
  int32_t lm_group_spread;   /* ... the largest distance between the first band positions of two landmarks of one group */
  int32_t lm_row_width;      /* band scalars a landmark row covers (the widest landmark's reach; 1 when no landmark touches the band) */
  int32_t lm_elim_kernel;    /* the landmark elimination of the last lvx_solve_step / LM iteration: 0 none, 1 by groups (k_lm_schur_grp), 2 one workgroup per landmark
                              * (k_lm_schur: the group panel does not fit the LDS, or the test switch TEST_LM_SCHUR_ONE) */
  int32_t rep_colours;       /* DETERMINISTIC only: launches the cross-term groups are spread over so that no two groups of a launch add to the same entry (0 otherwise) */
} lvx_layout;

/* lifetime ------------------------------------------------------------------------------------------------*/
int lvx_create(lvx_ctx** out, int device, uint32_t flags);
void lvx_destroy(lvx_ctx* ctx);
const char* lvx_version(void);
const char* lvx_last_error(const lvx_ctx* ctx);

/* problem description ---------------------------------------------------------------------------------------*/
/* SplineSegmentMeta of both splines (kontiki/trajectories/spline_base.h:31-39; split_trajectory.h:76-82: same dt, t0) */
int lvx_set_spline(lvx_ctx* ctx, double t0, double dt, int n_knots);
int lvx_set_camera(lvx_ctx* ctx, const lvx_pinhole* cam);
/* IO::IMUData stream (src/lvi_exc/include/utils/dataset_reader.h:45-50): one gyro block and one accel block per sample
 * (trajectory_manager_lvi.cpp:464-503); weights = CalibParamManager::global_opt_{gyro,acce}_weight */
int lvx_set_imu(lvx_ctx* ctx, int n, const double* t, const double* gyro3, const double* acc3, double w_gyro, double w_acc);
/* OrientationMeasurement of initialSO3TrajWithGyro (trajectory_manager_lvi.cpp:52-58); q as (w, x, y, z); enable = 0 removes it */
int lvx_set_orientation_prior(lvx_ctx* ctx, int enable, double t, const double* q_wxyz, double weight);
/* closest-point plane parameters Pi[3] of SurfelAssociation::get_surfel_planes() (trajectory_manager_lvi.cpp:567-569) */
int lvx_set_planes(lvx_ctx* ctx, int n_planes, const double* plane_pi3);
/* SurfelPoint list (src/lvi_exc/include/core/surfel_association.h:41-46) -> LiDARSurfelPoint blocks (trajectory_manager_lvi.cpp:571-581) */
int lvx_set_surfel(lvx_ctx* ctx, int n, const double* pt3, const double* t, const int32_t* plane_id, double t_map, double huber, double weight);
/* The same two calls with DEVICE pointers: the context copies what it needs on its stream at the call (the caller may reuse the buffers after lvx_synchronize);
 * argument errors as the host forms (a plane id outside the table: LVX_E_ARG from lvx_set_surfel_d, the family stays as it was); n = 0 clears.  The family's
 * layout (knot interval per row, stable sort, gather, row-ordered plane copy) then runs as kernels; the host reads the row count, the extremes of the plane ids and
 * one count per knot interval, in the one host stop of lvx_set_surfel_d.  A host lvx_set_planes / lvx_set_surfel afterwards replaces the device-origin input. */
int lvx_set_planes_d(lvx_ctx* ctx, int n_planes, const double* plane_pi3_d);
int lvx_set_surfel_d(lvx_ctx* ctx, int n, const double* pt3_d, const double* t_d, const int32_t* plane_id_d, double t_map, double huber, double weight);
/* sfm::Landmark table: reference observation uv and its view's t0 (kontiki/sfm/landmark.h:50-53, observation.h:35-37, view.h:34-35);
 * inverse depths live in the state vector */
int lvx_set_landmarks(lvx_ctx* ctx, int n_landmarks, const double* uv_ref2, const double* t0_ref);
/* StaticRsCameraMeasurement blocks (trajectory_manager_lvi.cpp:505-531): huber = w_cam, weight = 1 reproduces the reference's argument swap */
int lvx_set_reproj(lvx_ctx* ctx, int n, const int32_t* landmark_id, const double* uv_obs2, const double* t0_obs, double huber, double weight);
/* CameraSurfelLandmark blocks (trajectory_manager_lvi.cpp:584-606) */
int lvx_set_camsurf(lvx_ctx* ctx, int n, const int32_t* landmark_id, const int32_t* plane_id, double t_map, double huber, double weight);
/* LiDARPositionMeasurement blocks (kontiki/measurements/lidar_position_measurement.h:23-66, attached by addLidarPoses, trajectory_manager_lvi.cpp:533-559): LiDAR odometry
 * positions p3[i] = p_Lk in L0 at times t[i], L0 the LiDAR frame at t_start; 3 rows per block, r = weight (q_L^* (q0^* (qk p_LI + pk - p0) - p_LI) - p) — the reference's
 * Error = weight * Measure (:73), whose Measure ends in `v_L0Lk_L0 - p_Lk_L0` (:59-65: the measured position is subtracted INSIDE Measure) —, Huber on the
 * block's norm (the reference: weight = global_opt_pos_weight = 1, huber = 5).  n = 0 clears the family.  The odometry's orientation is not used (the reference stores it
 * and never reads it).  Rows are appended AFTER the camera-surfel rows, in input order: lvx_get_lidar_pose_rows; lvx_get_family_rows is unchanged (its last entry is also
 * the first LiDAR-pose row); lvx_layout::n_blocks / n_residuals count them.  State, tangent and lock layouts do not change: the blocks touch the knots, the LiDAR
 * extrinsics and (free) the LiDAR time offset.  lvx_evaluate, lvx_get_jacobian, lvx_get_gradient, lvx_get_normal_eq_dense, lvx_solve_step, lvx_lm_solve and the
 * shared-extrinsics solve include them.  The start time shares the one hub range with t_map: with surfel or camera-surfel blocks set too, t_start must equal their
 * t_map bit for bit (LVX_E_ARG from the next call that lays the problem out).  A pose time outside the spline: LVX_E_RANGE from the evaluation, like any other family.
 * While LiDAR poses are set, LVX_EVAL_JACOBIAN_BLOCKS returns LVX_E_ARG (the family has no per-block record), and so does every evaluation with the
 * DETERMINISTIC switch on (LVX_DETERMINISTIC=1): the family runs on the per-segment kernel only, whose additions are atomic. */
int lvx_set_lidar_poses(lvx_ctx* ctx, int n, const double* t, const double* p3, double t_start, double huber, double weight);
/* first residual row of the LiDAR-pose blocks and the total row count (either pointer may be NULL): block i owns rows row0 + 3 i .. + 2 */
int lvx_get_lidar_pose_rows(lvx_ctx* ctx, int64_t* row0, int64_t* n_rows_total);
int lvx_set_locks(lvx_ctx* ctx, uint32_t lock_mask);
/* experiment / debug switches.  They are read once from the environment (LVX_<NAME>) by lvx_create; this call changes one on a
 * live context (name with or without the LVX_ prefix, e.g. "FORCE_LEGACY", 1).  Unknown name: LVX_E_ARG. */
int lvx_set_switch(lvx_ctx* ctx, const char* name, int value);
/* max |time offset| bounds used to widen spans when a time offset is free (sensors.h:161-162; trajectory_manager_lvi.h:118-119) */
int lvx_set_time_offset_bounds(lvx_ctx* ctx, double imu_max, double sensor_max);

int lvx_state_size(const lvx_ctx* ctx);
int lvx_tangent_size(const lvx_ctx* ctx);
int lvx_get_layout(lvx_ctx* ctx, lvx_layout* out);
/* first residual row of every family (LVX_FAM_* order) and, at [LVX_NUM_FAM], the total: block i of family f owns rows row0[f] + i * rows_per_block */
int lvx_get_family_rows(lvx_ctx* ctx, int64_t row0[LVX_NUM_FAM + 1]);

/* evaluation -------------------------------------------------------------------------------------------------*/
/* One pass over every residual block at `state`: cost = sum 1/2 rho(|r|^2) (HuberLoss where the reference attaches one),
 * raw weighted residuals (family-major, input order inside a family), and — for LVX_EVAL_NORMAL_EQ — the robustified
 * J^T J and J^T r in tangent coordinates, left on the device in the structured layout.  residuals may be NULL. */
int lvx_evaluate(lvx_ctx* ctx, const double* state, uint32_t what, double* cost, double* residuals);
/* same, state already resident on the device; nothing is copied back except *cost (if not NULL) */
int lvx_evaluate_d(lvx_ctx* ctx, const double* state_d, uint32_t what, double* cost);
/* Error statistics: what the reference prints around every optimisation stage (TrajectoryManagerLVI::printErrorStatistics, trajectory_manager_lvi.cpp:621-697) and what
 * decides which surfels / landmarks to drop: per family the block counts, the cost share, the Huber outliers and the sums of the RAW error (the residual row divided by
 * the family weight: unweighted, unrobustified), per surfel plane and per landmark the same over its blocks.  A value-only pass of its own (no Jacobians, no normal
 * equations: it neither reads nor writes anything of lvx_evaluate) reduced on the device in a fixed order — two calls on one state give identical bits.  A block the
 * evaluation cannot take (a time outside the spline, a non-unit quaternion) is not counted in n_evaluated and the call returns LVX_E_RANGE / LVX_E_NONUNIT_QUAT as
 * lvx_evaluate does; `out` then still holds the sums over the blocks that were evaluated. */
typedef struct lvx_family_stats {
  int64_t n_blocks, n_evaluated, n_outliers;      /* outlier: squared norm of the weighted residual > huber^2 (Ceres HuberLoss); 0 for gyro / accel / prior */
  double  cost;                                   /* sum over blocks of 0.5 * rho(||r||^2): the family's share of lvx_evaluate's cost */
  double  sum[3], sum_abs[3], sum_sq[3], max_abs[3];   /* raw error per component; components the family does not have stay 0 */
} lvx_family_stats;
typedef struct lvx_error_stats { lvx_family_stats fam[LVX_NUM_FAM]; double cost; } lvx_error_stats;
int lvx_error_statistics(lvx_ctx* ctx, const double* state, lvx_error_stats* out);
/* state already on the device (NULL: the state of lvx_set_state); one host stop */
int lvx_error_statistics_d(lvx_ctx* ctx, const double* state_d, lvx_error_stats* out);
/* the same record for the LiDAR-pose blocks (what printErrorStatistics(..., show_lidar_pos = true) prints): raw error = row / weight per component, n_outliers by the
 * block's norm; a value-only pass of its own, reduced in a fixed order (identical bits from two calls on one state), one host stop.  lvx_error_stats keeps its six
 * families.  _d: state already on the device (NULL: the state of lvx_set_state).
 * lvx_error_stats::cost stays the sum over its six families: with poses set it is lvx_evaluate's cost MINUS this record's cost. */
int lvx_lidar_pose_statistics(lvx_ctx* ctx, const double* state, lvx_family_stats* out);
int lvx_lidar_pose_statistics_d(lvx_ctx* ctx, const double* state_d, lvx_family_stats* out);
/* of the last statistics call; arrays of n_planes / n_landmarks as set by lvx_set_planes / lvx_set_landmarks; any pointer may be NULL.  A plane / landmark without
 * (evaluated) blocks reports n = 0 and zeros.  LVX_E_STATE: no statistics call yet, or the problem changed since; LVX_E_ARG: another count than the tables'. */
int lvx_get_plane_stats(lvx_ctx* ctx, int n_planes, int64_t* n, double* sum_abs, double* max_abs);        /* surfel family: |point-to-plane distance|, metres */
int lvx_get_landmark_stats(lvx_ctx* ctx, int n_landmarks, int64_t* n, double* sum_sq, double* max_norm);  /* reprojection family: raw pixels, squared norm of the 2-vector */
/* debug / parity: expand the structured normal equations into dense host arrays (n_tangent^2 and n_tangent); small problems only */
int lvx_get_normal_eq_dense(lvx_ctx* ctx, double* H, double* g);
/* g = J^T r and diag(J^T J) (robustified, tangent layout, 0 for constant scalars) of the last LVX_EVAL_NORMAL_EQ evaluation — what
 * ceres::Problem::Evaluate returns as `gradient`; any problem size; either pointer may be NULL */
int lvx_get_gradient(lvx_ctx* ctx, double* g, double* diag);
/* debug / parity: rows of the last LVX_EVAL_JACOBIAN evaluation: cols[n_residuals][LVX_JAC_WIDTH] (-1 = unused), vals likewise (pre-loss) */
int lvx_get_jacobian(lvx_ctx* ctx, int32_t* cols, double* vals);
/* Per-block Jacobians (LVX_EVAL_JACOBIAN_BLOCKS; not together with LVX_EVAL_JACOBIAN: LVX_E_ARG; combines with COST, RESIDUALS, NORMAL_EQ).
 * One record per residual block of a family, in INPUT order (block i = the i-th lvx_set_* entry, as residual rows are):
 *   keys[i][3] = k0, k1, landmark (-1 where a family has none; (-1, -1, -1): the block was not evaluated)
 *   vals[i][rows_per_block][width] = the raw weighted rows (pre-loss) in tangent coordinates, 0.0 at constant columns.
 * Column c of a record is the per-segment kernel's own local column c; its tangent index is lvx_jacobian_block_cols:
 *   family        NR  width (locked / free offset)  k0                         k1                          landmark
 *   gyro           3  15                            interval                   -                           -
 *   accel          3  29                            interval                   -                           -
 *   prior          1  12                            interval                   -                           -
 *   surfel         1  54 / 55 (54: LiDAR offset)    map-time (hub) interval    point-time interval         -
 *   reprojection   2  55 / 56 (55: camera offset)   reference view's interval  observation's interval      landmark (column 54: rho)
 *   camera-surfel  1  60 / 61 (60: camera offset)   map-time interval          landmark's reference pose   -
 *   knot columns: 6 per knot (3 position | 3 rotation) of the 4 knots from k0 (then k1); gyro / prior: the 3 rotation scalars of each knot.
 * When the two poses of a block share knots (merged segments), two columns map to the same tangent index: add them.
 * The arrays are views into context-owned memory (host: pinned) of the last LVX_EVAL_JACOBIAN_BLOCKS evaluation; the call waits for their
 * copies; they stay valid until the next evaluation or lvx_destroy.  No blocks: n_blocks = 0.  Last evaluation without the bit, or failed: LVX_E_STATE. */
typedef struct lvx_jacobian_blocks {
  int64_t n_blocks;
  int32_t rows_per_block;
  int32_t width;
  const int32_t* keys;
  const double* vals;
  const int32_t* keys_d;
  const double* vals_d;
} lvx_jacobian_blocks;
int lvx_get_jacobian_blocks(lvx_ctx* ctx, int family, lvx_jacobian_blocks* out);
/* tangent index of each of the `width` columns of a record with keys key[3] (needs no context and no device); LVX_E_ARG for an unknown family / width */
int lvx_jacobian_block_cols(int family, int n_knots, int width, const int32_t key[3], int32_t* cols);
/* run on a caller-owned HIP stream (e.g. torch's current stream) instead of the context's own; NULL restores the own stream */
int lvx_set_stream(lvx_ctx* ctx, void* hip_stream);
/* multi-GPU (one calibration sequence per GPU): copy the dense border block of the last normal equations —
 * C[border_ld^2] (lower triangle), g_c[border_ld], cost, error word — into a caller-owned DEVICE buffer of border_ld^2 + border_ld + 2 doubles,
 * queued on the context's stream, ready for one RCCL all-reduce.  The last double is the pass's device error word (0 = every residual block
 * was evaluated): after a sum over the ranks a non-zero value tells EVERY rank that some rank's sums are incomplete, with no host
 * synchronisation in between (lvx_synchronize returns the matching error code on the rank that produced it). */
int lvx_export_border_d(lvx_ctx* ctx, double* out_d);
/* debug / repeatability: order-independent 64-bit checksums of the bit patterns of the structured normal equations of the last LVX_EVAL_NORMAL_EQ
 * evaluation — band, band gradient, border rows, dense border block, border gradient, landmark rows.  With LVX_DETERMINISTIC=1 (lvx_set_switch
 * "DETERMINISTIC") every addition of a pass happens in a fixed order — one stream, launches of workgroups with pairwise disjoint knot ranges, one
 * wavefront per workgroup, one replica of the dense accumulators per workgroup — and two evaluations of the same state give identical checksums
 * (fused locked-offset kernels; the per-segment kernels of a free time offset are not covered).  Several times slower than the default. */
int lvx_normal_eq_checksum(lvx_ctx* ctx, uint64_t out[6]);
/* keep `state` resident in the context's device buffer; lvx_evaluate_d(ctx, NULL, ...) then evaluates it without any host traffic */
int lvx_set_state(lvx_ctx* ctx, const double* state);
int lvx_get_state(lvx_ctx* ctx, double* state_out);
/* block until every launch queued on the context's stream has finished; returns the first device-side error of the last evaluation */
int lvx_synchronize(lvx_ctx* ctx);
/* per-kernel timing with HIP events recorded on the context's own stream around every launch (no host sync until read).
 * lvx_get_kernel_ms: sum of durations [ms] and launch counts since the last call, indexed by LVX_FAM_* (+ LVX_KERNEL_* below). */
#define LVX_KERNEL_FOLD 6
#define LVX_KERNEL_SOLVE 7
#define LVX_KERNEL_UPSTREAM 8
#define LVX_KERNEL_CLEAR 9          /* k_clear: structural clear of the accumulators + the state-only prepass */
#define LVX_KERNEL_REP_JAC 10       /* the five kernels of the fused reprojection path (LVX_FAM_REPROJ then times only the per-segment kernel) */
#define LVX_KERNEL_REP_OBS 11
#define LVX_KERNEL_REP_REF 12
#define LVX_KERNEL_REP_CROSS 13
#define LVX_KERNEL_REP_LMROWS 14
#define LVX_KERNEL_REP_FUSED 15     /* round 6: the single-launch reprojection kernel (k_reproj_fused); the five above then stay at zero */
#define LVX_KERNEL_FIXUP 16         /* the exact per-segment kernel over the fused kernels' fallback lists (lvx_layout::fallback_rows), all families */
#define LVX_NUM_KERNELS 17          /* entries lvx_get_kernel_ms writes: unchanged, callers size their arrays by it */
#define LVX_KERNEL_LIDAR_POS 17     /* the per-segment kernel over the LiDAR-pose blocks: beyond LVX_NUM_KERNELS, read with lvx_get_kernel_ms_ext */
#define LVX_KERNEL_POSE_COV 18      /* k_pose_cov of lvx_trajectory_covariance (the selected inverse in front of it is not part of the record) */
#define LVX_KERNEL_POINT_COV 19     /* k_pt_hub + k_point_cov of lvx_map_point_covariance (likewise) */
#define LVX_KERNEL_PROJ_HUB 20      /* k_proj_poses + k_proj_hub of lvx_projection_covariance (likewise) */
#define LVX_KERNEL_PROJ_COV 21      /* k_proj_cov of lvx_projection_covariance */
#define LVX_NUM_KERNELS_EXT 22
/* enable: 0 off | 1 every launch | 2 + k: only the launches of kernel k (e.g. 2 + LVX_FAM_SURFEL: the dominant kernel — two event
 * records per pass instead of ~20, which cost ~5 % of a config-4 pass).  While profiling is on, passes are issued launch by launch (no graph replay). */
int lvx_set_profiling(lvx_ctx* ctx, int enable);
int lvx_get_kernel_ms(lvx_ctx* ctx, double* ms_sum, int64_t* launches);
/* same for the first n_kernels <= LVX_NUM_KERNELS_EXT ids (arrays of n_kernels).  Both calls read and clear ONE list of records: lvx_get_kernel_ms (and any call with
 * n_kernels <= 17) discards the LiDAR-pose kernel's records without reporting them — to time that kernel, read with lvx_get_kernel_ms_ext(ctx, LVX_NUM_KERNELS_EXT, ..) only */
int lvx_get_kernel_ms_ext(lvx_ctx* ctx, int n_kernels, double* ms_sum, int64_t* launches);
/* Levenberg-Marquardt --------------------------------------------------------------------------------------------
 * Replaces ceres::Solve as configured by TrajectoryEstimator::Solve (kontiki/trajectory_estimator.h:38-68: TRUST_REGION,
 * LEVENBERG_MARQUARDT, SPARSE_SCHUR, max_num_iterations per stage; everything else Ceres defaults).  The trust-region loop,
 * LM damping and Jacobi scaling are restated from Ceres' public semantics (out-of-tree, parity unpinned). */
typedef struct lvx_lm_options {
  int32_t max_iterations;          /* options.max_num_iterations (30 / 50 / 80 / 200 per stage: trajectory_manager_lvi.cpp:60,86,125,182,244,340) */
  double initial_radius;           /* 1e4  */
  double max_radius;               /* 1e16 */
  double min_radius;               /* 1e-32 */
  double min_relative_decrease;    /* 1e-3 */
  double min_lm_diagonal;          /* 1e-6 */
  double max_lm_diagonal;          /* 1e32 */
  double function_tolerance;       /* 1e-6 */
  double gradient_tolerance;       /* 1e-10 */
  double parameter_tolerance;      /* 1e-8 */
  int32_t jacobi_scaling;          /* 1 */
  int32_t verbose;
} lvx_lm_options;
#define LVX_LM_NO_CONVERGENCE 0
#define LVX_LM_FUNCTION_TOLERANCE 1
#define LVX_LM_PARAMETER_TOLERANCE 2
#define LVX_LM_GRADIENT_TOLERANCE 3
#define LVX_LM_MAX_ITERATIONS 4
#define LVX_LM_FAILURE 5
#define LVX_LM_MIN_RADIUS 6       /* Ceres: CONVERGENCE, "minimum trust region radius reached" */
typedef struct lvx_lm_summary {
  int32_t iterations, successful_steps, termination;
  double initial_cost, final_cost, final_radius;
} lvx_lm_summary;
int lvx_lm_default_options(lvx_lm_options* opt);
/* minimise from `state` (in/out, host); summary may be NULL */
int lvx_lm_solve(lvx_ctx* ctx, double* state, const lvx_lm_options* opt, lvx_lm_summary* summary);
/* per-iteration trace of the last lvx_lm_solve: cost after the iteration, trust-region radius, accepted (1) / rejected (0) / invalid (-1); returns count */
int lvx_lm_get_history(lvx_ctx* ctx, int max_n, double* cost, double* radius, int32_t* accepted);
/* one damped solve on the normal equations of the last LVX_EVAL_NORMAL_EQ evaluation (if that evaluation was queued without a cost pointer its
 * device error word is read first: the exact kernels re-run a pass that needs them, a range / unit-quaternion error is returned):
 * (S H S + clamp(diag(S H S), 1e-6, 1e32) / radius) y = -S g, delta = S y (S = Jacobi scaling or identity); delta[n_tangent] on the host */
int lvx_solve_step(lvx_ctx* ctx, double radius, int jacobi_scaling, double* delta, double* model_cost_change);

/* Uncertainty of the calibration scalars c = tangent - 6 N (0-1 gravity, 2-4 accelerometer bias, 5-7 gyroscope bias, 8-10 / 11-13 / 14 LiDAR rotation, translation,
 * time offset, 15-17 / 18-20 / 21 the camera's) at the state of the last LVX_EVAL_NORMAL_EQ evaluation, from the factored LM system: landmarks, band and hub knots are
 * eliminated on the device as in lvx_solve_step and the 22 x 22 remainder is decomposed in one workgroup (k_calib_cov).  Same contract as lvx_solve_step: the
 * evaluation's error word is read first, LVX_E_STATE without such an evaluation; the stored normal equations and the LM state are left as they were.  One host stop.
 *   cov = [ s (s H_FF s + diag(clamp(diag(s H_FF s), 1e-6, 1e32)) / radius)^-1 s ]  restricted to the calibration scalars,
 * F = the free tangent scalars, s = the Jacobi scale 1 / (1 + sqrt(diag H)) of THIS evaluation (or 1).  It is the covariance of the DAMPED system at the stated radius:
 * with a free trajectory the scaled H of a short sequence has eigenvalues far below rounding (and four gauge directions that are null), so the LM diagonal acts as a
 * prior the result depends on; where the data decide (trajectory locked) the result is independent of the radius to 1e-5 at 1e8.  info_eig shows which is the case: an
 * eigenvalue at 1e-6 / radius is a direction no residual row touches.
 * A context that takes part in a joint solve (a reduction callback or an RCCL communicator is installed) returns LVX_E_STATE: the covariance of the shared extrinsics
 * over all ranks' sequences is not computed here (lvx_calibration_covariance_shared, below, is the call for it).  LVX_E_NOTPD: a pivot or an eigenvalue was not positive, or max_sweeps Jacobi sweeps did not converge (the
 * off-diagonal measure is in lvx_last_error); `out` is not written then. */
typedef struct lvx_calib_cov_options { double radius; int32_t jacobi_scaling; int32_t max_sweeps; } lvx_calib_cov_options;   /* 1e8, 1, 30 */
typedef struct lvx_calib_cov {
  int32_t n_free; int32_t free_index[22];     /* calibration scalars c that are free under the lock mask, ascending */
  double cov[22 * 22];                        /* row-major over c; rows / columns of constant scalars are 0 */
  double sigma[22];                           /* sqrt(cov[c][c]) in tangent units: a rotation entry is a HALF-angle (EigenQuaternionParameterization), std in rad = 2 sigma */
  double info_eig[22], info_vec[22 * 22];     /* eigenvalues (ascending, first n_free) and unit eigenvectors (row-major, column k over free_index) of the Jacobi-SCALED
                                                 marginal information: dimensionless, in (0, ~1] */
  double scale[22];                           /* the Jacobi scale of each calibration scalar (1 when jacobi_scaling = 0) */
  double radius; int32_t sweeps; int32_t n_hub_eliminated;   /* Jacobi sweeps used; border columns (6 per hub knot) eliminated in front of the 22 */
} lvx_calib_cov;
int lvx_calib_cov_default_options(lvx_calib_cov_options* opt);
int lvx_calibration_covariance(lvx_ctx* ctx, const lvx_calib_cov_options* opt, lvx_calib_cov* out);

/* Uncertainty of trajectory POSES in the same damped system: Sigma = s (s H_FF s + diag(lmd) / radius)^-1 s as above (free landmarks marginalised), restricted to the
 * at most 31 tangent scalars the pose at t[i] in `frame` (LVX_FRAME_TRAJECTORY / _LIDAR / _CAMERA, below) depends on and carried to the pose.  Contract of
 * lvx_calibration_covariance throughout: the normal equations of the last LVX_EVAL_NORMAL_EQ evaluation at the state of that evaluation, its error word read first,
 * LVX_E_STATE without one or on a context of a joint solve, copies only (the stored normal equations and a following lvx_solve_step see nothing), one host stop;
 * LVX_E_NOTPD (a band or border pivot <= 0) writes nothing.  The elimination always takes the sequential band Cholesky, whatever plan the solver would choose: the
 * entries of the inverse on the factor's pattern (band within max(bw, 23), band x border, border x border) come from the Takahashi recurrence over that factor
 * (k_border_inv, k_band_selinv), and the sweep stops at the lowest band position a query needs.
 *   window_idx[i][0..23]: tangent index 6 k .. 6 k + 5 of knots k = i0 .. i0 + 3; [24..30]: the sensor's theta (3), p (3), tau (1), -1 for LVX_FRAME_TRAJECTORY; a
 *     constant (locked) scalar is -1.  window_cov[i] = Sigma over those scalars, zero rows / columns at -1.
 *   cov[i] = J window_cov[i] J^T with J (6 x 31) the derivative of the pose error (dp = p' - p in the world frame; dphi the WORLD-frame rotation vector in radians,
 *     R' = Exp(dphi) R) by the tangent scalars: it carries the half-angle factor of EigenQuaternionParameterization, so sigma is metres and radians.  Sensor frame:
 *     q_S = q(tt) q_rel, p_S = p(tt) + q(tt) p_rel at tt = t + tau, tau column (v + omega x (q p_rel), omega).
 * Validity of a sample as lvx_sample_trajectory (an invalid one: valid = 0, zeros, window_idx -1); a window with a non-unit control quaternion is invalid and the call returns
 * LVX_E_NONUNIT_QUAT with the rest filled.  All sums in a fixed order: two calls return the same bits.  Any output array but `valid` may be NULL.
 * LVX_E_ARG: NULL context / options / t / out / valid, n <= 0, radius <= 0, unknown frame; a border of more than 96 scalars or a half-bandwidth beyond ~380 (the
 * one-workgroup kernels' LDS). */
typedef struct lvx_traj_cov_options { double radius; int32_t jacobi_scaling; int32_t reserved; } lvx_traj_cov_options;   /* 1e8, 1, 0 */
typedef struct lvx_traj_cov {
  double*  cov;        /* [n][36] row-major over (dp_x, dp_y, dp_z, dphi_x, dphi_y, dphi_z); may be NULL */
  double*  sigma;      /* [n][6]: sqrt of the diagonal, metres and RADIANS; may be NULL */
  double*  window_cov; /* [n][31 * 31]; may be NULL */
  int32_t* window_idx; /* [n][31] tangent index of each row of window_cov, -1 = constant or absent; may be NULL */
  uint8_t* valid;      /* [n] */
} lvx_traj_cov;
#define LVX_TRAJ_COV_W 31
int lvx_traj_cov_default_options(lvx_traj_cov_options* opt);
int lvx_trajectory_covariance(lvx_ctx* ctx, const lvx_traj_cov_options* opt, int frame, int n, const double* t, lvx_traj_cov* out);
/* t_d and the arrays of out_d are DEVICE addresses; only enqueues on the context's stream (after the evaluation's error word, which is read as above); a lost pivot
 * (nothing written) or a non-unit quaternion is reported by the next lvx_synchronize, as lvx_sample_trajectory_d's errors are. */
int lvx_trajectory_covariance_d(lvx_ctx* ctx, const lvx_traj_cov_options* opt, int frame, int n, const double* t_d, const lvx_traj_cov* out_d);

/* Uncertainty of LANDMARKS in the same damped system: the variance of the inverse depth rho_l, its covariance with the reference pose, and the covariance of the map
 * point.  The landmarks are eliminated before the band; with E_l the landmark's row of the normal equations over the reduced (band + border) scalars,
 * w_l = s_l^2 / (s_l^2 H_ll + lmd_l / radius) and Sigma_xx the covariance of the reduced system (the selected inverse lvx_trajectory_covariance reads),
 *   Sigma_ll = w_l + w_l^2 E_l Sigma_xx E_l^T,   Sigma_lx = -w_l E_l Sigma_xx.
 * Contract of lvx_trajectory_covariance word for word: the last LVX_EVAL_NORMAL_EQ evaluation at its state, its error word read first, LVX_E_STATE without one or on a
 * context of a joint solve, copies only, one host stop, always the sequential factor, LVX_E_NOTPD writes nothing, all sums in a fixed order (two calls return the same
 * bits), any output array but `valid` may be NULL.  The sweep of the selected inverse stops at the lowest band position a queried landmark needs (the first coupling
 * of its row, its reference window).
 *   The reference pose is the LVX_FRAME_CAMERA pose at t_ref = (t0_ref[l] + tau_C) + v_ref readout / rows, y_h = Unproject(uv_ref) (the radtan iteration when the
 *   camera is distorted): point = R_C(t_ref) (y_h / rho) + p_C(t_ref) in the world frame.
 *   window_idx[i][0] = the landmark's tangent index 6 N + 22 + l; [1..31] the 31 scalars of that pose as lvx_trajectory_covariance orders them, -1 constant.
 *   window_cov[i] = Sigma over those 32 scalars (zero rows / columns at -1); var_rho = window_cov[i][0][0] bit for bit; sigma_rho its square root.
 *   point_cov[i] = J window_cov[i] J^T, J = [ -R_C y_h / rho^2 | (I, -[R_C y_h / rho]_x) J_pose ] (3 x 32).
 * valid = 0 (zeros, window_idx -1) for a landmark that is constant under the lock mask or whose reference pose cannot be evaluated (outside the trajectory; a non-unit
 * control quaternion, and the call returns LVX_E_NONUNIT_QUAT with the rest filled).  A FREE landmark that no row reaches (H_ll = 0) is not special: s_l = 1,
 * var_rho = radius / 1e-6 — the direction is reported, not hidden.  The bound rho >= 0 is ignored; rho = 0 is a point at infinity (point and point_cov not finite).
 * Landmark-landmark covariances are off the factor's pattern and are not available.
 * LVX_E_ARG: NULL context / options / out / valid, n <= 0, n > the number of landmarks, an id outside [0, L), radius <= 0, reserved != 0, and the LDS limits of
 * lvx_trajectory_covariance. */
typedef struct lvx_landmark_cov_options { double radius; int32_t jacobi_scaling; int32_t reserved; } lvx_landmark_cov_options;   /* 1e8, 1, 0 */
#define LVX_LM_COV_W 32
typedef struct lvx_landmark_cov {
  double*  var_rho;     /* [n]; may be NULL */
  double*  sigma_rho;   /* [n]; may be NULL */
  double*  point;       /* [n][3] world frame; may be NULL */
  double*  point_cov;   /* [n][9] row-major; may be NULL */
  double*  window_cov;  /* [n][32 * 32]; may be NULL */
  int32_t* window_idx;  /* [n][32] tangent index, -1 = constant or absent; may be NULL */
  uint8_t* valid;       /* [n] */
} lvx_landmark_cov;
int lvx_landmark_cov_default_options(lvx_landmark_cov_options* opt);
/* landmark_id [n] (NULL: 0 .. n - 1), in any order, repeats allowed */
int lvx_landmark_covariance(lvx_ctx* ctx, const lvx_landmark_cov_options* opt, int n, const int32_t* landmark_id, lvx_landmark_cov* out);
/* landmark_id_d and the arrays of out_d are DEVICE addresses; only enqueues on the context's stream.  An id outside [0, L) is an invalid entry; a lost pivot (nothing
 * written) or a non-unit quaternion is reported by the next lvx_synchronize. */
int lvx_landmark_covariance_d(lvx_ctx* ctx, const lvx_landmark_cov_options* opt, int n, const int32_t* landmark_id_d, const lvx_landmark_cov* out_d);

/* Uncertainty of LiDAR MAP POINTS in the same damped system: how far a scan point moves in the map under the uncertainty of the trajectory and of q_LI, p_LI, tau_L.
 * A point p_L measured at t is placed in the LiDAR frame at t_map as lvx_get_scans_in_map, lvx_undistort_scan and lvx_render_map_d place it,
 *   p_M = T_L(t_map)^-1 T_L(t) p_L,   T_L(t) the LVX_FRAME_LIDAR pose at t + tau_L   (LiDARSurfelPoint::reprojectPoint2map),
 * with t_map the context's, as the surfel / camera-surfel families set it.  With a plane normal as dir3, var_dir is the predicted variance of that surfel row.
 * Contract of lvx_trajectory_covariance word for word: the last LVX_EVAL_NORMAL_EQ evaluation at its state, its error word read first, LVX_E_STATE without one or on a
 * context of a joint solve, copies only, one host stop, always the sequential factor, LVX_E_NOTPD writes nothing, LVX_E_NONUNIT_QUAT with the rest filled, all sums in
 * a fixed order: a point's record is the same bits alone, in any batch and at any position of the input.  Times arrive in any order.
 *   window_idx[i][0..23]: the four knots of the pose at t + tau_L, [24..47]: the four knots of the pose at t_map + tau_L, [48..54]: the LiDAR's theta (3), p (3),
 *     tau (1); -1 constant.  A time inside the window of t_map repeats indices in both knot groups: the window is gathered by index, so that is exact.
 *   window_cov[i] = Sigma over those 55 scalars (zero rows / columns at -1): rows 0..23 + 48..54 are lvx_trajectory_covariance's LVX_FRAME_LIDAR window at t, rows
 *     24..47 + 48..54 the one at t_map, bit for bit.  12 KB per point: for tests and small n.
 *   cov[i] = J window_cov[i] J^T, J (3 x 55) the derivative of p_M (lvi-exc_amd/csrc/lvx_ptcov.h); sigma = sqrt of its diagonal (metres); sigma_max = sqrt of its
 *     largest eigenvalue; var_dir = dir^T cov dir, written only when dir3 is given.  The product is formed from the two poses' 6 x 6 blocks (the one at t_map once per
 *     call), whose terms cancel as t approaches t_map, where the point stops moving: the absolute error of cov is a few eps of the variance the pose at t alone would
 *     give the point (1e-10 m in sigma), and at t = t_map a diagonal entry of -1e-21 can come out; sigma and sigma_max count it as zero.
 * valid = 0 (zeros, window_idx -1) for a point whose time is outside the trajectory or whose coordinates are not finite; the others are unaffected.  A point all of
 * whose scalars are constant under the lock mask is valid with cov exactly zero.
 * LVX_E_STATE also when no surfel / camera-surfel family has set t_map, and when a free knot scalar of the pose at t_map + tau_L is a band position of the factor
 * rather than a border slot (the hub knots are laid out around t_map; a locked tau_L far from zero leaves them): its cross terms are off the factor's pattern, and the
 * call refuses (nothing written) rather than return zeros.  LVX_E_ARG: NULL context / options / points / t / out / valid, n <= 0, radius <= 0, reserved != 0, and the
 * LDS limits of lvx_trajectory_covariance. */
typedef struct lvx_point_cov_options { double radius; int32_t jacobi_scaling; int32_t reserved; } lvx_point_cov_options;   /* 1e8, 1, 0 */
#define LVX_PT_COV_W 55
typedef struct lvx_point_cov {
  double*  point;      /* [n][3] p_M, LiDAR frame at t_map; may be NULL */
  double*  cov;        /* [n][9] row-major; may be NULL */
  double*  sigma;      /* [n][3] metres; may be NULL */
  double*  sigma_max;  /* [n]; may be NULL */
  double*  var_dir;    /* [n]; written only when dir3 is given; may be NULL */
  double*  window_cov; /* [n][55 * 55]; may be NULL */
  int32_t* window_idx; /* [n][55] tangent index, -1 = constant; may be NULL */
  uint8_t* valid;      /* [n] */
} lvx_point_cov;
int lvx_point_cov_default_options(lvx_point_cov_options* opt);
/* pt_lidar3 [n][3], t [n], dir3 [n][3] or NULL (directions in the map frame, e.g. unit plane normals) */
int lvx_map_point_covariance(lvx_ctx* ctx, const lvx_point_cov_options* opt, int n, const double* pt_lidar3, const double* t, const double* dir3, lvx_point_cov* out);
/* DEVICE addresses; only enqueues on the context's stream.  A lost pivot or a t_map window off the border (nothing written) or a non-unit quaternion is reported by the
 * next lvx_synchronize. */
int lvx_map_point_covariance_d(lvx_ctx* ctx, const lvx_point_cov_options* opt, int n, const double* pt3_d, const double* t_d, const double* dir3_d, const lvx_point_cov* out_d);
/* the same for points in the scan buffers' layout: xyzi4_d [n][4] float (x, y, z, intensity), 16-byte aligned; no directions */
int lvx_map_point_covariance_xyzi_d(lvx_ctx* ctx, const lvx_point_cov_options* opt, int n, const float* xyzi4_d, const double* t_d, const lvx_point_cov* out_d);

/* PIXEL uncertainty of LiDAR map points in the images, in the same damped system: how many pixels the uncertainty of the trajectory and of both sensors' extrinsics
 * and time offsets leaves where a map point lands in an image.  A map point x is given in the LiDAR frame at the context's t_map, as lvx_render_map_d takes it; its
 * pixel in the image taken at image_t is RenderMap's chain (LIinitializer::RenderMap, lvi-exc_amd/csrc/lvx_render.h):
 *   pt_G = R_L0 x + p_L0          (R_L0, p_L0): LVX_FRAME_LIDAR pose at t_map (+ tau_L)
 *   pt_C = R_C^T (pt_G - p_C)     (R_C, p_C):   LVX_FRAME_CAMERA pose at image_t (+ tau_C)
 *   uv   = radtan projection of pt_C (k1, k2, k3, p1, p2; no rolling-shutter row time, as RenderMap)
 * The map point is TAKEN AS GIVEN: its own uncertainty (lvx_map_point_covariance) correlates with the image pose off the factor's pattern and is not part of this
 * call.  What is propagated is the joint covariance of the two poses, cross terms included (band window x hub knots x both sensors' scalars: all on the pattern).
 *   window_idx[k][0..23]: the four knots of the camera pose at image_t + tau_C, [24..30]: the camera's theta (3), p (3), tau (1), [31..54]: the four knots of the LiDAR
 *     pose at t_map + tau_L, [55..61]: the LiDAR's theta, p, tau; -1 constant.  An image whose window shares knots with the window of t_map repeats indices: the
 *     window is gathered by index, so that is exact.
 *   window_cov[k] = Sigma over those 62 scalars (zero rows / columns at -1): rows 0..30 are lvx_trajectory_covariance's LVX_FRAME_CAMERA window at image_t, rows 31..61
 *     its LVX_FRAME_LIDAR window at t_map, bit for bit.
 *   pose_cov[k] = J12 window_cov[k] J12^T (12 x 12) over (camera dp, dphi; LiDAR dp, dphi) in lvx_trajectory_covariance's pose-error convention (world frame).
 *   cov[i] = A pose_cov A^T (2 x 2, px^2), A (2 x 12) the derivative of uv by those pose errors for this point (lvi-exc_amd/csrc/lvx_projcov.h); sigma = sqrt of its
 *     diagonal; sigma_max = sqrt of its largest eigenvalue.  For an image near t_map the pose-level terms cancel (the rig's relative pose is what is left).
 * Several images: lvx_render_map_d's rule and its very decisions (the same functions): a point's record refers to the lowest-index image whose pose is valid and in
 * which the point is in depth range [z_min, z_max] and inside the image.  status 0: skipped (a NaN coordinate, out of depth range in every valid image), 1: in depth
 * range somewhere but outside every image, 2: projected; for 0 and 1 the numeric outputs are zero and image = -1.
 * Contract of lvx_map_point_covariance word for word: the last LVX_EVAL_NORMAL_EQ evaluation at its state, its error word read first, copies only, one host stop in the
 * host form, always the sequential factor, all sums in a fixed order (a point's record is the same bits alone, in any batch and at any position), LVX_E_STATE without
 * an evaluation, on a context of a joint solve, without a camera, without t_map, or when a free knot scalar of the t_map window stands in the band; LVX_E_NOTPD writes
 * nothing; LVX_E_NONUNIT_QUAT returns with the rest filled.  LVX_E_ARG: NULL context / options / points (host form) / image_t / img / img->valid / out / out->status,
 * n <= 0, n_images outside 1 .. LVX_RENDER_MAX_IMAGES, radius <= 0, reserved != 0, z_min > z_max, and the LDS limits of lvx_trajectory_covariance. */
#define LVX_PROJ_COV_W 62
typedef struct lvx_proj_cov_options { double radius; int32_t jacobi_scaling; int32_t reserved; double z_min, z_max; } lvx_proj_cov_options; /* 1e8, 1, 0, 0.1, 15 */
typedef struct lvx_proj_cov_images {   /* per image; any array but valid may be NULL */
  double* pose_cov;    /* [n_images][144] */
  double* window_cov;  /* [n_images][62 * 62] */
  int32_t* window_idx; /* [n_images][62] */
  int32_t* valid;      /* [n_images]; 0: image_t outside the spline (not an error), zeros, indices -1 */
} lvx_proj_cov_images;
typedef struct lvx_proj_cov {          /* per point; any array but status may be NULL */
  double* uv;          /* [n][2] */
  double* cov;         /* [n][4] row-major, px^2 */
  double* sigma;       /* [n][2] sqrt of the diagonal (a diagonal entry below zero by rounding counts as zero) */
  double* sigma_max;   /* [n] sqrt of the largest eigenvalue, px */
  int32_t* image;      /* [n] */
  uint8_t* status;     /* [n] */
} lvx_proj_cov;
int lvx_proj_cov_default_options(lvx_proj_cov_options* opt);
/* map_xyzi4 [n][4] float (x, y, z, intensity), image_t [n_images] */
int lvx_projection_covariance(lvx_ctx* ctx, const lvx_proj_cov_options* opt, int n, const float* map_xyzi4, int n_images, const double* image_t, const lvx_proj_cov_images* img,
                              const lvx_proj_cov* out);
/* DEVICE addresses (map_xyzi4_d 16-byte aligned); only enqueues on the context's stream.  A lost pivot or a t_map window off the border (nothing written) or a non-unit
 * quaternion is reported by the next lvx_synchronize.  map_xyzi4_d == NULL: the de-skewed scans of the last data association, as lvx_render_map_d (n is ignored;
 * LVX_E_STATE before any association). */
int lvx_projection_covariance_d(lvx_ctx* ctx, const lvx_proj_cov_options* opt, int n, const float* map_xyzi4_d, int n_images, const double* image_t_d,
                                const lvx_proj_cov_images* img_d, const lvx_proj_cov* out_d);

/* x (+) delta with ceres::EigenQuaternionParameterization::Plus on quaternion blocks */
int lvx_plus(lvx_ctx* ctx, const double* state, const double* delta, double* state_out);

/* upstream point-cloud kernels ---------------------------------------------------------------------------------------*/
/* RsPointXYZIRT as the reference's scanRegistration receives it (src/aloam/src/scanRegistration.cpp:57-66), 32 bytes */
typedef struct lvx_rs_point {
  float x, y, z, pad;
  uint8_t intensity, pad2;
  uint16_t ring;
  uint32_t pad3;
  double timestamp;
} lvx_rs_point;
/* caller-owned host buffers with capacity n_in (scan_start/scan_end: n_rings); any pointer may be NULL.  Mirrors the globals
 * cloudCurvature / cloudSortInd / cloudNeighborPicked / cloudLabel (scanRegistration.cpp:82-85) and the four published clouds
 * as index lists into `cloud` (less_flat BEFORE the 0.2 m VoxelGrid of :440-444, which lvx_scan_less_flat_downsample applies) */
typedef struct lvx_scanreg_out {
  int32_t n;            /* points kept after the range / NaN filter = laserCloud size */
  float* cloud;         /* [n][4] x, y, z, intensity = ring + (t - t_first) */
  float* curvature;     /* [n] */
  int32_t* label;       /* [n] 2 sharp, 1 less sharp, 0 none, -1 flat */
  int32_t* sort_ind;    /* [n] */
  int32_t* picked;      /* [n] */
  int32_t* scan_start;  /* [n_rings] */
  int32_t* scan_end;    /* [n_rings] */
  int32_t* sharp; int32_t* less_sharp; int32_t* flat; int32_t* less_flat;
  int32_t counts[4];
} lvx_scanreg_out;
/* n_rings: 1 .. 1024 (otherwise LVX_E_ARG).  Points whose ring id is >= n_rings are DROPPED like the points the range / NaN filter removes (the reference indexes its
 * per-ring vector with the id unchecked).  A ring is cut into six sectors of at most 2048 points each, i.e. rings of up to 12299 kept points; a longer sector returns
 * LVX_E_ARG "scan sector longer than the LDS sort capacity" and the context stays usable. */
int lvx_scan_register(lvx_ctx* ctx, int n, const lvx_rs_point* pts, int n_rings, float min_range, lvx_scanreg_out* out);
/* The same for n_sweeps sweeps in ONE call (laserCloudHandler is invoked once per sweep, scanRegistration.cpp:134; sweeps are independent): pts holds the sweeps
 * back to back, sweep s = pts[sweep_offsets[s] .. sweep_offsets[s + 1]) (sweep_offsets[0] = 0), outs[s] its caller-owned output buffers (capacity = its input count).
 * One upload, one launch per stage over all sweeps' rings, one download — a single sweep keeps 16 of 256 CUs busy. */
int lvx_scan_register_batch(lvx_ctx* ctx, int n_sweeps, const int32_t* sweep_offsets, const lvx_rs_point* pts, int n_rings, float min_range, lvx_scanreg_out* outs);
/* device-resident variant: the points are already on the device (pts_d, sweeps back to back as above); the results STAY on the device inside the context — only the
 * kept-point count and the four list lengths per sweep come back (n_kept[n_sweeps], counts4[n_sweeps][4]; either may be NULL) — and lvx_scan_register_get downloads
 * one sweep's arrays on demand (the buffers of `out` that are not NULL). */
int lvx_scan_register_batch_d(lvx_ctx* ctx, int n_sweeps, const int32_t* sweep_offsets, const lvx_rs_point* pts_d, int n_rings, float min_range, int32_t* n_kept, int32_t* counts4);
int lvx_scan_register_get(lvx_ctx* ctx, int sweep, lvx_scanreg_out* out);
/* The published less-flat cloud: pcl::VoxelGrid (leaf_size 0.2 m) over every ring's less-flat points, rings concatenated (scanRegistration.cpp:425-447),
 * for the sweep of the last lvx_scan_register of this context.  out_xyzi4 [max_out][4], ring_counts [n_rings] (may be NULL), *n_out = total
 * (also when larger than max_out).  Points of a voxel are averaged in their input order (pcl's std::sort leaves the order of equal keys open). */
int lvx_scan_less_flat_downsample(lvx_ctx* ctx, float leaf_size, int max_out, float* out_xyzi4, int32_t* ring_counts, int32_t* n_out);
/* the same for sweep `sweep` of the context's last lvx_scan_register_batch (sweep 0 = the call above).  A ring is down-sampled in one LDS sort of at most 4096 less-flat
 * points (rings of about 4200 kept points): beyond that the call returns LVX_E_ARG "more less-flat points in one ring than the LDS sort capacity (4096)", writes nothing,
 * and the context and its registration results stay usable. */
int lvx_scan_less_flat_downsample_sweep(lvx_ctx* ctx, int sweep, float leaf_size, int max_out, float* out_xyzi4, int32_t* ring_counts, int32_t* n_out);

/* pclomp::VoxelGridCovariance::applyFilter (src/ndt_omp/include/pclomp/voxel_grid_covariance_omp_impl.hpp:49-374): the grid stays on the
 * device inside the context; leaves are numbered in ascending voxel-key order (std::map iteration order of the reference) */
typedef struct lvx_voxel_info { int32_t n_leaves, n_points; int32_t min_b[3], max_b[3], div_b[3], divb_mul[3]; } lvx_voxel_info;
int lvx_voxel_build(lvx_ctx* ctx, int n, const float* xyzi4, float leaf_size, int min_points_per_voxel, double min_covar_eigvalue_mult, lvx_voxel_info* info);
int lvx_voxel_build_d(lvx_ctx* ctx, int n, const float* xyzi4_d, float leaf_size, int min_points_per_voxel, double min_covar_eigvalue_mult);
/* lvx_voxel_build_d is ASYNCHRONOUS: the whole build is one launch chain on the context's stream without a host hop (extents, cell table, leaf count stay on the
 * device; the cloud must stay alive and unchanged until a consumer has run).  This call waits for it and returns what VoxelGridCovariance's getters report after
 * applyFilter (getMinBoxCoordinates / getMaxBoxCoordinates / getNrDivisions / getDivisionMultiplier, leaves_.size(): pcl/filters/voxel_grid.h, voxel_grid_covariance_omp.h:298-305). */
int lvx_voxel_get_info(lvx_ctx* ctx, lvx_voxel_info* info);
/* Leaf fields (voxel_grid_covariance_omp.h:92-190): nr_points (-1 = rejected), mean_, cov_, icov_, evecs_ (columns), evals_, centroid, pointList_
 * as offsets[n_leaves + 1] into point_ids (input indices, input order inside a leaf); any pointer may be NULL */
int lvx_voxel_get(lvx_ctx* ctx, int32_t* leaf_key, int32_t* leaf_n, double* mean3, double* cov9, double* icov9, double* evecs9, double* evals3, float* centroid3,
                  int32_t* offsets, int32_t* point_ids);
/* getNeighborhoodAtPoint7 (:423-438): leaf index per displacement {0,+x,-x,+y,-y,+z,-z} or -1.
 * A query with a non-finite coordinate (NaN, +-inf) has no neighbour: every id is -1, in lvx_voxel_lookup1 / 7 (_d) and in lvx_voxel_lookup_rel alike (the reference
 * casts floor(NaN) to int, which is undefined).  A leaf that the build rejected (nr_points -1) is never returned. */
int lvx_voxel_lookup7(lvx_ctx* ctx, int nq, const float* xyzi4, int32_t* leaf_ids7);
int lvx_voxel_lookup7_d(lvx_ctx* ctx, int nq, const float* xyzi4_d, int32_t* leaf_ids7_d);
/* getNeighborhoodAtPoint1 (:440-446): the leaf of the query's own cell or -1 */
int lvx_voxel_lookup1(lvx_ctx* ctx, int nq, const float* xyzi4, int32_t* leaf_ids1);
int lvx_voxel_lookup1_d(lvx_ctx* ctx, int nq, const float* xyzi4_d, int32_t* leaf_ids1_d);
/* getNeighborhoodAtPoint(relative_coordinates, reference_point, neighbors) (:378-408), the general form behind the 1- / 7- / 26-cell variants (:411-446):
 * leaf_ids[q][r] = leaf at displacement rel3[r] = (di, dj, dk) from the query's cell, or -1 (outside the grid, empty, fewer than min_points_per_voxel points).
 * The reference returns the hits in this order without the misses.  DIRECT26 = pcl::getAllNeighborCellIndices() as rel3. */
int lvx_voxel_lookup_rel(lvx_ctx* ctx, int nq, const float* xyzi4, int n_rel, const int32_t* rel3, int32_t* leaf_ids);
/* VoxelGridCovariance::radiusSearch(point, radius, k_leaves, k_sqr_distances) (voxel_grid_covariance_omp.h:473-502) against the grid of the last lvx_voxel_build: the
 * leaves whose float centroid lies within `radius` of the query, nearest first.  Per query LVX_VOXEL_RADIUS_MAX slots: count[q] leaf indices in leaf_ids27[q][] and
 * their squared distances in sqr_dist27[q][], then -1 / +infinity.  Defined in lvi-exc_amd/csrc/lvx_vxradius.h: no tree — the 27 cells around the query's cell hold
 * every centroid within a radius <= leaf size; float distance d2 = (dx dx + dy dy) + dz dz to the stored float centroid, a hit is d2 < (float)(radius * radius)
 * (FLANN's L2_Simple and RadiusResultSet); ascending d2, equal d2 by ascending leaf index (FLANN leaves ties unspecified).  Deviation: the build's cell arithmetic is
 * float, so a centroid within an ulp of a cell face and about `radius` away can lie two cells from the query — the reference's tree finds it, the 27 cells do not.
 * MEMBERS are the leaves that had at least min_points_per_voxel points when the grid was built, as in the reference's tree (voxel_grid_covariance_omp_impl.hpp:301-330):
 * a leaf the build rejected afterwards (nr_points -1) IS returned here — and never by lvx_voxel_lookup1 / 7 / _rel.  A non-finite query has count 0.
 * LVX_E_ARG: radius <= 0, not finite or above the grid's leaf size (the 27 cells would no longer cover it), NULL xyzi4.  LVX_E_STATE: no grid.  nq = 0 is fine.
 * Host arrays; any output may be NULL.  The _d form takes device addresses and is ASYNCHRONOUS on the context's stream. */
#define LVX_VOXEL_RADIUS_MAX 27
int lvx_voxel_radius_search(lvx_ctx* ctx, int nq, const float* xyzi4, double radius, int32_t* leaf_ids27, float* sqr_dist27, int32_t* count);
int lvx_voxel_radius_search_d(lvx_ctx* ctx, int nq, const float* xyzi4_d, double radius, int32_t* leaf_ids27_d, float* sqr_dist27_d, int32_t* count_d);
/* SurfelAssociation::getAssociation flag pass (src/lvi_exc/src/core/surfel_association.cpp:111-138): plane_of_point[H*W] = surfel id or -1.
 * Conflicts resolve as the reference's SERIAL plane loop (highest plane id wins); W <= 4096 */
int lvx_surfel_assoc(lvx_ctx* ctx, int H, int W, const float* scan_map_xyzi4, int n_planes, const double* plane_p4, const double* box_min3, const double* box_max3,
                     double radius, int sel_per_ring, int32_t* plane_of_point);
/* device-resident variant: planes10_d = p4[P][4] | box_min[P][3] | box_max[P][3] */
int lvx_surfel_assoc_d(lvx_ctx* ctx, int H, int W, const float* scan_d, int n_planes, const double* planes10_d, double radius, int sel_per_ring, int32_t* plane_of_point_d);

/* n_scans organised scans [n_scans][H][W] against one surfel table in one call (scans are independent: this is also the unit that shards over GPUs) */
int lvx_surfel_assoc_batch_d(lvx_ctx* ctx, int n_scans, int H, int W, const float* scans_d, int n_planes, const double* planes10_d, double radius, int sel_per_ring,
                             int32_t* plane_of_point_d);

/* SurfelAssociation::setSurfelMap happens once per DataAssociation, getAssociation once per scan (lvi_initialize_surfel_orb.cpp:1184-1199): build the association
 * grid of a surfel table once — later lvx_surfel_assoc_batch_d / lvx_surfel_assoc_d calls with THE SAME planes10_d pointer and n_planes reuse it (the caller
 * promises the table's contents are unchanged) until the next prepare or a call with another table. */
int lvx_surfel_map_prepare_d(lvx_ctx* ctx, int n_planes, const double* planes10_d);
/* End of the prepared table's lifetime: call it BEFORE the table's memory is freed, reused or rewritten.  The grid is keyed by (address, n_planes) only — a
 * caching allocator hands the same address to the next table of the same size, and a stale grid would silently miss hits — so a caller that prepares owns
 * the table until it releases (or prepares another one).  Calls without a preceding prepare build the grid per call and are always safe. */
int lvx_surfel_map_release(lvx_ctx* ctx);

/* sequence-per-GPU joint solve (BASELINE config 5) ---------------------------------------------------------*/
/* Every rank owns one calibration sequence (trajectory, gravity, biases, landmarks are private); the rig extrinsics — lidar theta(3) p(3)
 * tau, camera theta(3) p(3) tau = 14 tangent scalars — are shared.  One LM iteration of the JOINT problem: every rank eliminates its private
 * variables on its GPU, ONE all-reduce of the 14 x 14 reduced system (+ rhs + flags, 211 doubles), every rank solves it and back-substitutes;
 * plus tiny reductions of the cost, the model cost change and the step / gradient norms so that all ranks take the same accept / reject and
 * termination decisions.  The library does not link a communication library: the host supplies the reduction over HOST buffers (RCCL via
 * torch.distributed, MPI, ...); messages are <= 278 doubles (the largest: lvx_calibration_covariance_shared) and latency-bound.  All ranks must use the same lock mask and options. */
#define LVX_N_SHARED 14
#define LVX_REDUCE_SUM 0
#define LVX_REDUCE_MAX 1
typedef int (*lvx_allreduce_fn)(void* user, double* buf, int n, int op);   /* in-place over all ranks; returns 0 on success */
/* lvx_solve_step / lvx_lm_solve of the joint problem; fn == NULL degenerates to the single-sequence calls */
int lvx_solve_step_shared(lvx_ctx* ctx, double radius, int jacobi_scaling, lvx_allreduce_fn fn, void* user, double* delta, double* model_cost_change);
int lvx_lm_solve_shared(lvx_ctx* ctx, double* state, const lvx_lm_options* opt, lvx_allreduce_fn fn, void* user, lvx_lm_summary* summary);

/* lvx_calibration_covariance of the JOINT problem: how well all the sequences together determine the shared extrinsics, and how much each one contributed.  Every rank
 * calls it after its own LVX_EVAL_NORMAL_EQ evaluation with the same options and the same locks on the shared scalars; the transport is chosen as in
 * lvx_solve_step_shared (fn: host callback; fn == NULL with an RCCL communicator: the device path; fn == NULL without one: a joint problem of one rank).
 * Definition: H = the joint normal matrix over [every rank's private scalars | the 14 shared scalars once], F its free scalars,
 *   s = 1 / (1 + sqrt(diag H_FF)) (or 1): the shared entries come from the diagonal SUMMED over the ranks,
 *   A_R = s H_FF s + diag(clamp(diag(s H_FF s), 1e-6, 1e32)) / radius,    cov = s A_R^-1 s  restricted to this rank's 8 private calibration scalars and the 14 shared,
 * the system lvx_solve_step_shared factors at that radius (what the radius means: INTEGRATION.md 4d-2).  The spectrum is that of M, the Schur complement of A_R onto the
 * free shared scalars, and own_info is this rank's term of it, T_r = s_sh (C_r - B_r^T A_r^-1 B_r) s_sh with the rank's private damping inside A_r and no shared damping:
 *   sum_r own_info_r + diag(lmd_shared) / radius = M = V diag(info_eig) V^T,   lmd_shared = clamp(diag(s H s), 1e-6, 1e32) at the shared scalars.
 * own_info[k][k] / M[k][k] is the fraction of the joint information about scalar k that this sequence supplied.  The shared part of the record (cov rows / columns
 * 8 .. 21, info_eig, info_vec) is bit-identical on all ranks.  Exactly two collectives: the joint diagonal, and one sum of 278 doubles (T_r, per-slot free
 * indicators, rank count, votes, sweep cap); with RCCL one host stop behind the first.  The stored normal equations and the LM state are left as they were.
 * Errors are voted, every rank returns together and no rank writes `out`: LVX_E_NOTPD (a pivot or an eigenvalue not positive on any rank, or the sweep cap — the
 * SMALLEST max_sweeps over the ranks applies everywhere, values above 64 count as 64); LVX_E_STATE (a rank has no preceding evaluation); LVX_E_ARG (a shared scalar
 * is locked on some ranks and free on others); any other local failure returns its code on the failing rank and LVX_E_COMM on the others.  A pivot lost on the
 * block-reduction route of any rank makes every rank repeat the elimination sequentially, with a third collective. */
typedef struct lvx_joint_calib_cov {
  int32_t n_free; int32_t free_index[22];      /* as lvx_calib_cov, under this rank's lock mask */
  double  cov[22 * 22], sigma[22];             /* c 0..7 (gravity, biases): THIS rank's private scalars; c 8..21: the shared extrinsics; cross terms included */
  int32_t n_shared_free; int32_t shared_free_slot[14];   /* canonical slots 0..13 (c - 8) that are free, ascending */
  double  info_eig[14], info_vec[14 * 14];     /* spectrum of the JOINT Jacobi-scaled marginal information of the free shared scalars (ascending; column k over shared_free_slot) */
  double  own_info[14 * 14];                   /* this rank's own contribution T_r to that matrix: canonical slots, joint scale, WITHOUT the shared damping; 0 in locked rows / columns */
  double  scale[22];                           /* c 0..7 from this rank's diagonal, c 8..21 from the JOINT diagonal */
  double  radius; int32_t sweeps, n_hub_eliminated, world;   /* world = number of ranks that took part (counted in the collective) */
} lvx_joint_calib_cov;
int lvx_calibration_covariance_shared(lvx_ctx* ctx, const lvx_calib_cov_options* opt, lvx_allreduce_fn fn, void* user, lvx_joint_calib_cov* out);

/* RCCL transport: with a communicator installed the reductions of lvx_solve_step_shared / lvx_lm_solve_shared (fn = NULL) run as ncclAllReduce on the
 * context's stream — the per-step [S | rhs | votes] block is packed, reduced and solved on the device with no host round trip.  librccl is loaded with
 * dlopen (no link-time dependency; a process that already loaded RCCL, e.g. through torch, shares it).  Rank 0 creates the 128-byte id, the host
 * distributes it (any side channel), every rank calls lvx_rccl_init; lvx_rccl_finalize (or lvx_destroy) frees the communicator.
 * Collectives: one after the first evaluation, then exactly two per LM iteration — the reduced 14 x 14 system, and the decision block (candidate cost, model terms,
 * norms, the candidate's joint diagonal / gradient); the two cannot merge, the candidate depends on the reduced system's solution.  One more (a vote) when the
 * iteration cap ends the loop right behind a rejected step: the re-evaluation of x that follows a rejection has met no collective yet.
 * A rank that fails locally votes in the next collective and EVERY rank returns there (the failing one with its code, the others LVX_E_COMM). */
int lvx_rccl_unique_id(lvx_ctx* ctx, void* id128);
int lvx_rccl_init(lvx_ctx* ctx, const void* id128, int rank, int world);
int lvx_rccl_finalize(lvx_ctx* ctx);
/* in-place all-reduce (LVX_REDUCE_SUM / LVX_REDUCE_MAX) of a caller's device buffer of n doubles over the installed communicator, queued on the context's stream:
 * the transport of the per-step border-block reduction of a sequence-per-GPU evaluation (lvx_export_border_d -> this) */
int lvx_rccl_allreduce_d(lvx_ctx* ctx, double* buf_d, int n, int op);
/* number of shared scalars the last joint solve of this context kept out of its local elimination (LVX_N_SHARED when a transport was active, 0 for a
 * single-sequence solve): lets a caller / test assert that the joint path was taken */
int lvx_joint_shared_count(lvx_ctx* ctx);
/* reductions issued by this context since the last reset (either transport) */
int64_t lvx_collective_count(lvx_ctx* ctx, int reset);

/* NDT registration derivatives ------------------------------------------------------------------------*/
/* pclomp::NormalDistributionsTransform::computeDerivatives with DIRECT7 search (src/ndt_omp/include/pclomp/ndt_omp_impl.hpp:180-285, 289-430, 484-536)
 * against the voxel grid of the last lvx_voxel_build of this context (resolution = its leaf size): score, 6-gradient and 6 x 6 Hessian (row-major)
 * of the NDT objective at the transform vector p6 = (tx, ty, tz, rx, ry, rz); input = source cloud, trans = the same cloud already transformed by p6
 * (pcl::transformPointCloud, as the caller does before every call).  Per-point arithmetic in float like the reference, accumulation in double.
 * The NDT calls (lvx_ndt_derivatives, lvx_ndt_align, lvx_ndt_fitness) require a finite source cloud: their kernels do not carry the lookups' non-finite guard. */
int lvx_ndt_derivatives(lvx_ctx* ctx, int n, const float* input_xyzi4, const float* trans_xyzi4, const double* p6, double outlier_ratio, int compute_hessian,
                        double* score, double* gradient6, double* hessian36);
/* The same evaluation with the neighbour search of the caller's choice (ndt_omp.h:59-64): search = LVX_NDT_SEARCH_KDTREE (0), 1 (DIRECT1), 7 (DIRECT7: what
 * lvx_ndt_derivatives does) or 26 (DIRECT26).  KDTREE = radiusSearch(x_trans_pt, resolution_, ...) (ndt_omp_impl.hpp:233-236): lvx_voxel_radius_search at the grid's leaf
 * size, neighbours visited nearest first.  A rejected leaf among them is evaluated with what the grid stores for it, as the reference does: a zero inverse covariance
 * (eigenvalue test) adds -gauss_d1 to the score and nothing else; one with infinities is dropped by updateDerivatives' own guard. */
#define LVX_NDT_SEARCH_KDTREE 0
int lvx_ndt_derivatives_search(lvx_ctx* ctx, int n, const float* input_xyzi4, const float* trans_xyzi4, const double* p6, double outlier_ratio, int compute_hessian,
                               int search, double* score, double* gradient6, double* hessian36);

/* NDT registration (the loop around the derivatives) ---------------------------------------------------------------------------*/
/* pcl::Registration::align -> pclomp::NormalDistributionsTransform::computeTransformation (src/ndt_omp/include/pclomp/ndt_omp_impl.hpp:81-171): Newton steps
 * (JacobiSVD solve of the 6 x 6 system :127-129) with the More-Thuente step length (computeStepLengthMT :772-931, updateIntervalMT :648-685, trialValueSelectionMT
 * :689-768), derivatives by computeDerivatives (:180-285) and, after a line search that moved, computeHessian (:540-645), all against the voxel grid of the last
 * lvx_voxel_build of this context (= setInputTarget at that resolution, ndt_omp.h:117-122,275-282).  The Newton / line-search bookkeeping (a handful of scalars per
 * iteration) runs on the host as in the reference; every evaluation over the cloud is one kernel.  Defaults = the reference's constructor (:46-76).
 * search: 0 = KDTREE (LVX_NDT_SEARCH_KDTREE: the radius search over the leaf centroids, see lvx_ndt_derivatives_search), 1 = DIRECT1, 7 = DIRECT7, 26 = DIRECT26
 * (ndt_omp.h:59-64; the calibration uses DIRECT7, lidar_odometry.cpp:32-43). */
typedef struct lvx_ndt_options { double step_size, outlier_ratio, transformation_epsilon; int32_t max_iterations, search; } lvx_ndt_options;
typedef struct lvx_ndt_result {
  float final_transformation[16];   /* row-major 4 x 4: getFinalTransformation() */
  double p6[6];                     /* (tx, ty, tz, rx, ry, rz) the loop ended at */
  double score, trans_probability;  /* the last evaluated score and score / n (getTransformationProbability, :170) */
  int32_t iterations, converged, n_evaluations, reserved;   /* nr_iterations_, converged_, derivative evaluations over the cloud */
} lvx_ndt_result;
int lvx_ndt_default_options(lvx_ndt_options* opt);
/* src = the input cloud (setInputSource); guess16 = row-major initial guess or NULL (identity, as align(output) passes); aligned_xyzi4 (may be NULL) receives the
 * source under the final transformation = the `output` cloud of align(). */
int lvx_ndt_align(lvx_ctx* ctx, int n, const float* src_xyzi4, const float* guess16, const lvx_ndt_options* opt, lvx_ndt_result* result, float* aligned_xyzi4);
/* pcl::Registration::getFitnessScore(max_range) (what src/ndt_omp/apps/align.cpp:30 prints): mean over the source points of the squared distance from the point
 * under `transform16` to its nearest target point (float L2, exact search), counting distances <= max_range; DBL_MAX when nothing is counted. */
int lvx_ndt_fitness(lvx_ctx* ctx, int n_src, const float* src_xyzi4, const float* transform16, int n_tgt, const float* tgt_xyzi4, double max_range, double* fitness);

/* LiDAR odometry: NDT scan-to-map poses without A-LOAM ---------------------------------------------------------------------------------------------*/
/* downsampleCloud (include/utils/pcl_utils.h:46-53) = pcl::VoxelGrid<VPoint> with one leaf size on all axes, all fields averaged, over an UNORGANISED cloud: float
 * min / max of the cloud, min_b = floor(min / leaf), voxel index = sum over axes of int(floor(x * (1 / leaf)) - float(min_b)) * mul, points ordered by index (equal
 * indices in input order), one output point per run in index order = the float sum of x, y, z, intensity in that order divided by the float count.  Points with a
 * non-finite x, y or z are left out (pcl::VoxelGrid on a non-dense cloud).  n = 0: 0 points.  LVX_E_ARG: NULL / negative arguments, leaf <= 0, or a leaf so small that
 * div_x * div_y * div_z exceeds int32 ("Leaf size is too small for the input dataset", as PCL refuses it).  The host form writes at most max_out points and reports
 * the full count in *n_out; the _d form takes device pointers (out_xyzi4_d holds n points) and still returns the count to the host, so it waits for the stream. */
int lvx_voxelgrid_downsample(lvx_ctx* ctx, int n, const float* xyzi4, float leaf_size, int64_t max_out, float* out_xyzi4, int32_t* n_out);
int lvx_voxelgrid_downsample_d(lvx_ctx* ctx, int n, const float* xyzi4_d, float leaf_size, float* out_xyzi4_d, int32_t* n_out);
/* LiDAROdometry::feedScan(t, scan, predict, update_map = true, using_loam = false) (src/core/lidar_odometry.cpp:45-128) over the scans of lvx_set_scans, in order —
 * what CalibrHelperLVI::Initialization runs before EstimateRotation (calib_helper_lvi.cpp:55-60, there with an identity prediction).  Per scan k:
 *   the first scan (empty map, :56-57): pose = identity, no registration (its step record is zero but converged = 1);
 *   otherwise registration() (:76-87): guess = pose[k-1] * predict[k] formed in double and cast to float (predict16 NULL: pose[k-1]); source = the filter above at
 *     downsample_leaf over the scan's x, y, z, intensity; pose = final_transformation of lvx_ndt_align's loop against the current grid, cast to double;
 *   updateKeyScan / checkKeyScan (:89-128, the rule of lvx_data_association_poses): a key scan — all its points, NaN ones included — is moved with its pose
 *     (pcl::transformPointCloud with a Matrix4d: double, summed left to right, rounded to float; non-finite points copied) and appended to the map cloud on the device;
 *     the voxel grid is rebuilt over the WHOLE map at ndt_resolution (setInputTarget(map_cloud_), :98-102).
 * The clouds, the map and the grid stay on the device; the host keeps what the reference keeps in scalars (Newton / More-Thuente bookkeeping, the key decision).
 * After the call the context's voxel grid is that of the final map, as after lvx_voxel_build_d.
 * DEVIATION: a scan whose source is empty (every point non-finite) keeps the guess as its pose, with n_src = 0, converged = 1, n_evaluations = 0 — PCL refuses an
 * empty input cloud.  LVX_E_STATE: before lvx_set_scans, or a map whose grid has no leaf (as lvx_ndt_align).  LVX_E_ARG: NULL pose16 / steps, a non-positive
 * resolution or leaf, an unknown search, or n_key * H * W beyond 2^31 - 1 points. */
typedef struct lvx_odom_options {
  float ndt_resolution, downsample_leaf;        /* 0.5, 0.5 (lidar_odometry.cpp:36,81) */
  double key_dist, key_angle_deg;               /* 0.2 m, 5 deg (:121-122) */
  lvx_ndt_options ndt;                          /* step 0.01, epsilon 1e-3, 50 iterations, DIRECT7 (:36-41); outlier ratio: the constructor's 0.55 */
  int32_t min_points_per_voxel, reserved;       /* 6 (ndt_omp: VoxelGridCovariance default) */
  double min_covar_eigvalue_mult;               /* 0.01 */
} lvx_odom_options;
typedef struct lvx_odom_step {
  int32_t n_src, is_key, iterations, converged, n_evaluations, reserved;   /* filtered source points; 1 = joined the map; then as lvx_ndt_result */
  double score, trans_probability, p6[6];
} lvx_odom_step;
int lvx_odom_default_options(lvx_odom_options* opt);
/* predict16: [n_scans][16] row-major or NULL; pose16: out, [n_scans][16] row-major scan -> map; steps: out, [n_scans]; n_key (may be NULL): out, key scans */
int lvx_lidar_odometry(lvx_ctx* ctx, const lvx_odom_options* opt, const double* predict16, double* pose16, lvx_odom_step* steps, int32_t* n_key);
/* the key-scan map cloud of the last lvx_lidar_odometry (n_key * H * W points, NaN points included): at most max_points are written, *n_points (may be NULL) is the
 * full count.  LVX_E_STATE before any odometry run. */
int lvx_odometry_get_map(lvx_ctx* ctx, int64_t max_points, float* xyzi4, int64_t* n_points);

/* surfel map extraction ------------------------------------------------------------------------------*/
/* SurfelAssociation::setSurfelMap + checkPlaneType (src/lvi_exc/src/core/surfel_association.cpp:50-86, 246-266) over the leaves of the last
 * lvx_voxel_build of this context (the cloud passed to it must still be alive): leaves with >= min_leaf_points points and planarity >= p_lambda,
 * plane fit, Pi = -d n, AABB of the leaf's points; output in voxel-key (std::map) order.  The reference fits with pcl RANSAC (random); this is
 * the deterministic variant documented in DESIGN.md: leaf PCA plane -> inliers strictly within dist_threshold -> PCA refit (three inliers or more) -> reselect;
 * p4 is signed so that d <= 0 (at d == 0: the first non-zero component of the normal positive).
 * *n_planes is the number of planes whatever max_planes is; the first min(*n_planes, max_planes) are written and nothing behind them (max_planes = 0: planes may be NULL).
 * Without a voxel build on this context, and after a build that found no leaf (an empty cloud), the map is empty: *n_planes = 0 and LVX_OK.
 * min_leaf_points below the min_points_per_voxel of the build: a leaf with fewer points than min_points_per_voxel has no eigen data (the reference never gets there,
 * its 10 is hard-coded above ndt_omp's 6); it has no planarity and is never a surfel, whatever p_lambda is.  min_leaf_points <= 0 means 1: a leaf the build rejected
 * (nr_points = -1) is never fitted.  Both hold for lvx_assoc_options::min_leaf_points as well. */
typedef struct lvx_surfel_plane { double p4[4]; double Pi[3]; double box_min[3]; double box_max[3]; int32_t leaf, n_points, n_inliers, plane_type; } lvx_surfel_plane;
int lvx_surfel_extract(lvx_ctx* ctx, double p_lambda, double dist_threshold, int min_leaf_points, int min_inliers, int max_planes, lvx_surfel_plane* planes, int32_t* n_planes);

/* scan de-skew ------------------------------------------------------------------------------------*/
/* licalib PointXYZIT (src/lvi_exc/include/utils/pcl_utils.h:39-44), 32 bytes */
typedef struct lvx_point_xyzit { float x, y, z, pad; float intensity; float pad2; double timestamp; } lvx_point_xyzit;
/* The chronological SurfelPoint emission of getAssociation (src/lvi_exc/src/core/surfel_association.cpp:141-158) for n_scans associated scans (flags from
 * lvx_surfel_assoc_batch_d), all device-resident: per scan column-major (w outer, h inner), points with a flag and a non-zero raw timestamp; scans concatenated.
 * SurfelPoint fields as arrays: raw point (LiDAR frame), point in the map frame, timestamp, plane id.  *n_out = total and per_scan_counts are those of the whole
 * list, also when it is longer than max_out: the entries below max_out are unspecified then (written in part, in full or not at all) and nothing at or beyond
 * max_out is written; size the outputs from *n_out and call again.  max_out = 0 with NULL outputs only counts.  per_scan_counts[n_scans] may be NULL. */
int lvx_surfel_emit_d(lvx_ctx* ctx, int n_scans, int H, int W, const int32_t* flags_d, const float* scans_map_d, const lvx_point_xyzit* scans_raw_d, int max_out,
                      double* pt3_d, double* pt_map3_d, double* t_d, int32_t* plane_d, int32_t* n_out, int32_t* per_scan_counts);
/* getAssociation for n_scans scans with host buffers in and out (what DataAssociation's loop over the scans does, lvi_initialize_surfel_orb.cpp:1192-1199): flags
 * plane_of_point[n_scans * H * W] (may be NULL) and the concatenated SurfelPoint list; *n_out = its length (nothing is written when it exceeds max_out) */
int lvx_surfel_assoc_emit(lvx_ctx* ctx, int n_scans, int H, int W, const float* scans_map_xyzi4, const lvx_point_xyzit* scans_raw, int n_planes, const double* plane_p4,
                          const double* box_min3, const double* box_max3, double radius, int sel_per_ring, int32_t* plane_of_point, int max_out, double* pt3, double* pt_map3, double* t,
                          int32_t* plane, int32_t* n_out);
/* LIinitializer::DataAssociation, refinement branch (src/lvi_exc/test/lvi_initialize_surfel_orb.cpp:1180-1201), device-resident end to end:
 *   ScanUndistortion::undistortScanInMap (every point of every scan de-skewed into the LiDAR frame at the map time; map cloud = the scans concatenated),
 *   LiDAROdometry::ndtInit(resolution) + setInputTarget(map cloud) (voxel covariance grid), SurfelAssociation::setSurfelMap, getAssociation per scan.
 * lvx_set_scans hands over the dataset's organised raw scans once (LioDataset::get_scan_data: [n_scans][H][W], per-point timestamps, NaN x = no return);
 * lvx_data_association runs one association round at `state` and leaves the surfel map and the chronological SurfelPoint list in the context.
 * The FIRST round on a set of scans stops at the host four times (leaf count, plane count, list length of the association grid, SurfelPoint counts); every later round
 * launches the whole chain over capacities learned from the round before — the kernels read the true counts from device memory — and stops ONCE, at the end; a count that
 * outgrew its capacity (or a cell table that was too small) discards that attempt and the round runs the four-stop chain (lvx_data_association_stats counts both).
 * The plane records stay on the device until lvx_get_surfel_map asks for them.
 * averageTimeDownSmaple (every step-th point, surfel_association.cpp:240-244) is the caller's: it picks from the arrays of lvx_get_surfel_points. */
typedef struct lvx_assoc_options {
  float ndt_resolution;              /* lvi.yaml:26, 0.5 */
  int32_t min_points_per_voxel;      /* voxel_grid_covariance_omp.h:207, 6 */
  double min_covar_eigvalue_mult;    /* :208, 0.01 */
  double plane_lambda;               /* 0.7 (lvi_initialize_surfel_orb.cpp:1183) */
  double fit_threshold;              /* RANSAC distance threshold 0.05 (surfel_association.cpp:279) */
  int32_t min_leaf_points, min_inliers;   /* 10 (:61), 20 (:283); min_leaf_points <= 0 means 1, leaves below min_points_per_voxel are never surfels (lvx_surfel_extract) */
  double radius;                     /* associated_radius_ 0.05 */
  int32_t selected_per_ring, reserved;    /* getAssociation(..., 2) */
} lvx_assoc_options;
int lvx_assoc_default_options(lvx_assoc_options* opt);
int lvx_set_scans(lvx_ctx* ctx, int n_scans, int H, int W, const lvx_point_xyzit* raw);
int lvx_data_association(lvx_ctx* ctx, const double* state, double map_time, const lvx_assoc_options* opt, int32_t* n_planes, int32_t* n_points);
/* The FIRST DataAssociation of a calibration — the InitializationDone branch (lvi_initialize_surfel_orb.cpp:1175-1178), where the map comes from per-scan odometry poses
 * (LOAM's, ReadPoseGT :458-516) and only the SO3 spline of Solve #0 exists:
 *   Mapping() (:1262-1300) = ScanUndistortion::undistortScan() (scan_undistortion.h:40-57: rotation-only de-skew of every scan into its own start frame, scans whose stamp
 *     lies outside the spline are dropped) + LiDAROdometry::feedScan(scan_t, scan, pose, update_map = true, using_loam = true) per scan (lidar_odometry.cpp:45-74);
 *     updateKeyScan / checkKeyScan (:89-128): the first scan, or one > key_dist [m] from the last key scan or turned by > key_angle_deg in yaw / pitch / roll, is moved with
 *     its pose and appended to the key-scan map = the NDT target (reference: 0.2 m, 5 deg);
 *   undistortScanInMap(odom_data_map) (scan_undistortion.h:95-116): every de-skewed scan moved with its pose = the scans in the map frame;
 *   setSurfelMap(lidar_odom->getNDTPtr(), map_time) on the voxel grid of the KEY-SCAN map with opt->plane_lambda (the constructor's 0.6, :127,240); getAssociation per scan.
 * scan_t[n_scans]: the scans' header stamps; pose16[n_scans][16]: row-major 4 x 4 scan -> map (LiDAROdometry::OdomData::pose); has_pose (may be NULL = all): 0 = no
 * odometry pose for that stamp (loam_poses_map_.find fails: the scan is skipped).  key_scan (may be NULL): out, 1 where the scan joined the key-scan map.
 * Results as lvx_data_association: lvx_get_surfel_map / lvx_get_surfel_points / lvx_get_scans_in_map (absent scans: NaN). */
int lvx_data_association_poses(lvx_ctx* ctx, const double* state, const double* scan_t, const double* pose16, const int32_t* has_pose, double key_dist, double key_angle_deg,
                               const lvx_assoc_options* opt, int32_t* n_planes, int32_t* n_points, int32_t* key_scan);
int lvx_get_surfel_map(lvx_ctx* ctx, int max_planes, lvx_surfel_plane* planes);
/* rounds that took the one-stop chain since the context was created, and how many of those had to be repeated on the four-stop chain */
int lvx_data_association_stats(lvx_ctx* ctx, int64_t* one_stop_rounds, int64_t* repeated_rounds);
int lvx_get_surfel_points(lvx_ctx* ctx, int max_points, double* pt3, double* pt_map3, double* t, int32_t* plane);
/* The surfel measurements of the evaluator from the last association without the lists leaving the device.  Equivalent to: lvx_get_surfel_map + lvx_set_planes with
 * the records' Pi in order; lvx_get_surfel_points; the points 0, step, 2 step, ... (step <= 0: 1) with t >= t_map, in order; lvx_set_surfel(those, t_map, huber,
 * weight).  n_used (may be NULL): how many were kept (0: the family is cleared).  LVX_E_STATE before any association on this context.  The family owns its copies:
 * a later association or lvx_set_scans does not disturb it.  One host stop. */
int lvx_set_surfel_from_association(lvx_ctx* ctx, int step, double t_map, double huber, double weight, int32_t* n_used);
/* parity / debug: the de-skewed scans of the last lvx_data_association, [n_scans][H][W][4] float */
int lvx_get_scans_in_map(lvx_ctx* ctx, float* xyzi4);

/* scan ingestion: VLP-16 packets to organised raw scans ---------------------------------------------------------------*/
/* licalib::VelodyneCorrection::unpack_scan (src/lvi_exc/include/utils/vlp_common.h:51-149, called per scan from LioDataset::read, dataset_reader.h:152-157) for every
 * scan of a recording, on the device: the context's raw scans come from the 1206-byte packets (12 blocks of {header, rotation, 32 x {distance, intensity}} + 6 trailer
 * bytes) instead of from host-unpacked records — a tenth of the bytes.  Per point, in the reference's arithmetic (csrc/lvx_vlp16.h): azimuth interpolated per firing
 * from the block rotations (block 11 reuses the difference of block 10), rotation-table products with the reference's own float cosf / sinf tables (built on the host,
 * once per context), the stored point (y, -x, z), row scan_mapping_16[dsr], column 2 * block_counter + firing, timestamp scan_stamp + (row * 2.304e-6 + column *
 * 55.296e-6) — indexed with the MAPPED row, as the reference does.  A range outside [min_range, max_range]: x = y = z = NaN, intensity 0, timestamp kept.  A corrected
 * azimuth outside the angle window [min_angle, max_angle] (min > max: the window wraps): the record is 32 zero bytes, as the reference's value-initialised cloud.
 * Block headers are not checked (the reference does not); n_bad_headers counts the blocks that are not 0xEEFF.  pad / pad2 of every record are 0.
 * W = 0: 24 x the longest scan's packet count.  The reference sizes each cloud to its own 24 x packets columns; the context keeps ONE W, so the columns beyond
 * 24 x packets of a shorter scan hold "no return" — x = y = z = NaN, intensity 0, timestamp 0 (the association skips NaN, the emission skips timestamp 0).  That is the
 * one deviation.
 * LVX_E_ARG: a scan of more than 76 packets (the reference's time table ends at column 1824 and it would read past it), W smaller than 24 x the longest scan or above
 * 4096, offsets that decrease, NULL arguments; the context and its previous scans stay as they were. */
#define LVX_VLP16_PACKET_BYTES 1206
typedef struct lvx_vlp16_options { double min_range, max_range; int32_t min_angle, max_angle; } lvx_vlp16_options;   /* 0.6, 150, 0, 36000 (vlp_common.h:186-189) */
typedef struct lvx_vlp16_info { int64_t n_packets, n_in_range, n_out_of_range, n_outside_window, n_bad_headers; int32_t W, reserved; } lvx_vlp16_info;
int lvx_vlp16_default_options(lvx_vlp16_options* opt);
/* scans [s] = packets [packet_offsets[s] .. packet_offsets[s+1]) of `packets` ([n][1206] bytes, host); scan_stamp[s] = the message's header stamp.
 * Result: the context's raw scans exactly as lvx_set_scans(ctx, n_scans, 16, W, ...) would leave them (the association state is reset as there).  opt, info may be NULL. */
int lvx_set_scans_vlp16(lvx_ctx* ctx, int n_scans, const int32_t* packet_offsets, const uint8_t* packets, const double* scan_stamp, int W, const lvx_vlp16_options* opt,
                        lvx_vlp16_info* info);
/* the same into a caller's host buffer [n_scans][16][W], context scans untouched */
int lvx_vlp16_unpack(lvx_ctx* ctx, int n_scans, const int32_t* packet_offsets, const uint8_t* packets, const double* scan_stamp, int W, const lvx_vlp16_options* opt,
                     lvx_point_xyzit* out, lvx_vlp16_info* info);
/* unpack_scan's second overload (vlp_common.h:152-176): organised H x W xyz-intensity clouds ([n_scans][H][W][4] float, host) whose times are
 * scan_stamp[s] + (h * 2.304e-6 + w * 55.296e-6); the context's raw scans as lvx_set_scans(ctx, n_scans, H, W, ...) would leave them.  H <= 16 and W <= 1824 (the
 * reference's time table), otherwise LVX_E_ARG. */
int lvx_set_scans_organised(lvx_ctx* ctx, int n_scans, int H, int W, const float* xyzi4, const double* scan_stamp);
/* parity / hand-over: scans [first, first + n) of the context, however they were set, [n][H][W] records.  LVX_E_STATE: the context has no scans; LVX_E_ARG: a range
 * outside them. */
int lvx_get_scans_raw(lvx_ctx* ctx, int first, int n, lvx_point_xyzit* out);

/* SurfelAssociation::associateVisualPointsWithPlanes (surfel_association.cpp:161-214) over the landmark table of lvx_set_landmarks and the inverse depths in `state`:
 * plane_of_landmark[l] = index of the surfel whose AABB strictly contains the landmark (map frame) within 2 * radius of its plane — the highest such index, as the
 * reference's loop leaves it — or -1 (also for rho < 0.05 and for reference views outside the spline).  q_LtoC (x, y, z, w), t_LinC: LiDAR pose in the camera frame. */
int lvx_landmark_assoc(lvx_ctx* ctx, const double* state, const double* q_LtoC_xyzw, const double* t_LinC3, double map_time, int n_planes, const double* plane_p4,
                       const double* box_min3, const double* box_max3, double radius, int32_t* plane_of_landmark);
/* TrajectoryManagerLVI::evaluateLidarPose for a batch of times (trajectory_manager_lvi.cpp:398-408): q_LtoG (x,y,z,w), p_LinG, valid = 0 outside the spline */
int lvx_evaluate_lidar_pose(lvx_ctx* ctx, const double* state, int n, const double* t, double* q_xyzw4, double* p3, int32_t* valid);
/* ScanUndistortion::undistort (src/lvi_exc/include/core/scan_undistortion.h:132-180): every point is moved with the spline pose at ITS timestamp into the
 * target frame (q_G_to_target, p_target_in_G); out = float xyzi per point */
int lvx_undistort_scan(lvx_ctx* ctx, const double* state, int n, const lvx_point_xyzit* raw, const double* q_G_to_target_xyzw, const double* p_target_in_G3,
                       int correct_position, float* out_xyzi4);

/* coloured map and LiDAR-to-image overlay ---------------------------------------------------------------------------------*/
/* TrajectoryManagerLVI::evaluateCameraPose for a batch of times (trajectory_manager_lvi.cpp:430-440): q_CtoG (x,y,z,w), p_CinG, valid = 0 outside the spline */
int lvx_evaluate_camera_pose(lvx_ctx* ctx, const double* state, int n, const double* t, double* q_xyzw4, double* p3, int32_t* valid);
/* pcl::PointXYZRGB as LIinitializer::RenderMap fills it (src/lvi_exc/test/lvi_initialize_surfel_orb.cpp:759-762, 785-788), 16 bytes.  a = 255 for a coloured point and 0
 * otherwise: "never coloured" and "sampled a black pixel" differ.  A skipped point (NaN coordinate, depth outside [z_min, z_max] in every image) is all zero, as the
 * resize()'d cloud of the reference (:715); a point in depth range but outside the image keeps its xyz with colour 0. */
typedef struct lvx_point_xyzrgb { float x, y, z; uint8_t b, g, r, a; } lvx_point_xyzrgb;
#define LVX_RENDER_MAX_IMAGES 32
typedef struct lvx_render_options { double z_min, z_max; int32_t reserved[2]; } lvx_render_options;   /* 0.1, 15 (:757) */
int lvx_render_default_options(lvx_render_options* opt);
/* LIinitializer::RenderMap (lvi_initialize_surfel_orb.cpp:711-811): every map point (LiDAR frame at map_time, float xyzi) goes through the calibrated chain
 * T_L0inG (evaluateLidarPose(map_time), :720-727) and T_GtoC (evaluateCameraPose(image_t), :738-747, rigid inverse) and the inline radtan projection (:766-779) and takes the
 * grey value of the pixel int(uv) (:781-788).  images: n_images (1 .. LVX_RENDER_MAX_IMAGES) grey images [rows][pitch] back to back, rows / cols from lvx_set_camera,
 * pitch >= cols.  The reference colours from ONE image (the first candidate whose pose evaluates, :738-741,800); with several, a point takes its colour from the
 * LOWEST-index image whose pose is valid and in which it is in depth range and inside the image — with one image that is the reference exactly.
 * image_valid[i] = 0: image_t[i] lies outside the spline (the reference's `continue`, :738-741; not an error).  *n_colored = points with a = 255.
 * LVX_E_RANGE: map_time outside the spline (the early return of :720-723); out is zeroed, image_valid and *n_colored are 0.  LVX_E_STATE: no spline / no camera.
 * LVX_E_ARG: n_images outside 1 .. 32, pitch < cols, a required pointer is NULL.  n = 0: LVX_OK, nothing written.  opt may be NULL (defaults).
 * map_xyzi4 == NULL: the cloud is the de-skewed scans the last lvx_data_association(_poses) of this context left on the device ([n_scans][H][W] points, nothing is
 * uploaded; n is ignored and out holds that many records); LVX_E_STATE before any association. */
int lvx_render_map(lvx_ctx* ctx, const double* state, double map_time, int n, const float* map_xyzi4, int n_images, const uint8_t* images, int pitch, const double* image_t,
                   const lvx_render_options* opt, lvx_point_xyzrgb* out, int32_t* image_valid, int64_t* n_colored);
/* The same with the cloud, the images and the records in device memory (state, image_t, image_valid, n_colored stay host pointers).  map_xyzi4_d == NULL: the cloud is the
 * de-skewed scans of the last lvx_data_association(_poses) of this context ([n_scans][H][W] points; n is ignored, out_d holds that many records); LVX_E_STATE before any
 * association. */
int lvx_render_map_d(lvx_ctx* ctx, const double* state, double map_time, int n, const float* map_xyzi4_d, int n_images, const uint8_t* images_d, int pitch, const double* image_t,
                     const lvx_render_options* opt, lvx_point_xyzrgb* out_d, int32_t* image_valid, int64_t* n_colored);
/* LIinitializer::ReprojectPointCloudToImage (lvi_initialize_surfel_orb.cpp:1307-1363) for n_pairs (scan, image) pairs: scan scan_index[i] of lvx_set_scans (the scans the last
 * data association ran on), rotation-only de-skewed into its own frame at scan_t[i] (ScanUndistortion::undistortScan, scan_undistortion.h:40-57 — the scan_data_ the
 * reference iterates, :1314,1342), is moved with q_LtoC = q_CtoG* (x) q_LtoG, p_LinC = q_CtoG* (p_LinG - p_CinG) (:1333-1336; LiDAR pose at scan_t[i], camera pose at
 * image_t[i]) and projected (:1343-1353: z < 0 skipped, uv < 0 outside, int(uv) > cols - 1 / rows - 1 outside; the projection is RenderMap's radtan formula).
 * mask[i][rows][cols] (host): 1 where a point lands (what the reference paints green), 0 elsewhere.  valid[i] = 0 and an all-zero mask: a pose outside the spline.
 * LVX_E_STATE: no spline / camera / scans; LVX_E_ARG: a scan index outside the scans, a NULL pointer.  n_pairs = 0: LVX_OK. */
int lvx_overlay_scans(lvx_ctx* ctx, const double* state, int n_pairs, const int32_t* scan_index, const double* scan_t, const double* image_t, uint8_t* mask, int32_t* valid);

/* trajectory queries -------------------------------------------------------------------------------------------------------*/
/* TrajectoryView::Evaluate(t, flags) for a batch of times (kontiki/trajectories/uniform_r3_spline_trajectory.h:36-103, uniform_so3_spline_trajectory.h:46-125).
 * A sample at t in frame F is valid iff MinTime <= t + tau_F < MaxTime (MinTime = t0, MaxTime = t0 + (N - 3) dt: the test of evaluateLidarPose,
 * trajectory_manager_lvi.cpp:401-402); the t - 1e-5 retry of SplineView::Evaluate (spline_base.h:196-203) is not part of a query.  NaN and +-inf are invalid.  An invalid
 * sample writes zeros to every requested output and valid = 0.
 *   LVX_FRAME_TRAJECTORY: the spline itself (tau = 0): p, v = p', a = p'', q (x, y, z, w), omega in the WORLD frame (Kontiki's convention: the gyroscope model rotates it
 *     by q*, sensors/imu.h:87-91).
 *   LVX_FRAME_LIDAR / LVX_FRAME_CAMERA: the sensor at t + tau_S with the extrinsics (q_S, p_S) of the state: q = q(tt) (x) q_S, p = q(tt) p_S + p(tt) — the same bits as
 *     lvx_evaluate_lidar_pose / lvx_evaluate_camera_pose —, the velocity of the sensor origin v(tt) + omega(tt) x (q(tt) p_S), omega(tt).  The acceleration of a sensor frame
 *     needs the angular acceleration, which Kontiki does not offer: requesting it is LVX_E_ARG.
 * Any output pointer but valid may be NULL (not computed); arrays are [n][3] / [n][4].
 * A sample inside the range whose four-knot window holds a control quaternion that fails logq's 1e-5 unit check (quaternion_math.h:19-23) gets valid = 0 and zeros; the
 * call returns LVX_E_NONUNIT_QUAT with all other samples filled, as lvx_error_statistics reports.
 * LVX_E_ARG: NULL context, NULL valid / out / t / state, n <= 0, unknown frame, sensor-frame acceleration.  LVX_E_STATE: before lvx_set_spline. */
#define LVX_FRAME_TRAJECTORY 0
#define LVX_FRAME_LIDAR 1
#define LVX_FRAME_CAMERA 2
typedef struct lvx_traj_samples {
  double *position3, *velocity3, *acceleration3, *orientation_xyzw4, *angular_velocity3; int32_t* valid;
} lvx_traj_samples;
int lvx_sample_trajectory(lvx_ctx* ctx, const double* state, int frame, int n, const double* t, const lvx_traj_samples* out);
/* The same on device memory: state_d (NULL: the state of lvx_set_state), t_d and the pointers inside *out_d (a host struct) are device addresses.  Only enqueues on the
 * context's stream; the caller synchronises.  A non-unit quaternion is reported by the next lvx_synchronize, as the errors of a queued evaluation pass are. */
int lvx_sample_trajectory_d(lvx_ctx* ctx, const double* state_d, int frame, int n, const double* t_d, const lvx_traj_samples* out_d);
/* Imu::Gyroscope / Imu::Accelerometer with constant biases (sensors/imu.h:61-101, constant_bias_imu.h:51-61) at tt = t + tau_imu: gyro = q* omega + b_g,
 * acc = q* (p'' + g(roll, pitch)) + b_a with G = -9.79 (imu.h:25) — what the gyroscope / accelerometer residuals subtract from the measurement.  Validity, zeros and error
 * codes as lvx_sample_trajectory; gyro3 or acc3 may be NULL. */
int lvx_predict_imu(lvx_ctx* ctx, const double* state, int n, const double* t, double* gyro3, double* acc3, int32_t* valid);
int lvx_predict_imu_d(lvx_ctx* ctx, const double* state_d, int n, const double* t_d, double* gyro3_d, double* acc3_d, int32_t* valid_d);
/* How far the trajectory is from reference poses (q' (x, y, z, w) — normalised on the way in —, p') at the stamps t, e.g. the LOAM poses the calibration started from:
 * LIinitializer::PublishTrajectory (lvi_initialize_surfel_orb.cpp:834-902) lays the two paths side by side.  Per valid sample (validity as lvx_sample_trajectory, pose in
 * `frame`): translation error |p - p'|, rotation error 2 atan2(|vec(d)|, |d.w|) with d = q* (x) q' (Eigen's angularDistance).
 *   LVX_ALIGN_NONE: compared as given.  LVX_ALIGN_FIRST: with a the lowest valid index and A = T_a o R_a^-1, every reference pose becomes A o R_i (PublishTrajectory's
 *   Twl * Tl, :850-861, for a first pose that need not be the identity).
 * Relative errors: for each valid sample i and the NEXT valid one j, T_i^-1 T_j against R_i^-1 R_j (unaligned reference: they do not depend on align).
 * A summary holds rmse, mean and max of its n terms; argmax is the lowest sample index of the maximum (of i for a relative step).  n_valid = 0: all-zero summaries and
 * LVX_OK.  abs_trans_n / abs_rot_n (NULL or [n]): the per-sample absolute errors, 0 for an invalid sample.  Sums are formed in a fixed order: two calls return the same
 * bits.  Error codes as lvx_sample_trajectory. */
typedef struct lvx_err_summary { double rmse, mean, max; int32_t argmax, n; } lvx_err_summary;
typedef struct lvx_pose_errors { int32_t n, n_valid; lvx_err_summary abs_trans, abs_rot, rel_trans, rel_rot; } lvx_pose_errors;
#define LVX_ALIGN_NONE 0
#define LVX_ALIGN_FIRST 1
int lvx_compare_poses(lvx_ctx* ctx, const double* state, int frame, int n, const double* t, const double* q_xyzw4, const double* p3, int align, lvx_pose_errors* out,
                      double* abs_trans_n, double* abs_rot_n);

/* Sensor-to-IMU rotation from odometry: InertialInitializer::EstimateRotation (src/lvi_exc/src/core/inertial_initializer.cpp:26-81), which CalibrHelperLVI::Initialization
 * (src/lvi_exc/src/core/calib_helper_lvi.cpp:44-96) calls after Solve #0 on the odometry poses so far — from 30 poses on, at every 10th — until one prefix passes.  For
 * consecutive odometry poses (t_i, q'_i), (t_j, q'_j) it pairs the SO3 spline's relative rotation d_i = q(t_i)* (x) q(t_j) with the odometry's d_s = q'_i* (x) q'_j (q'
 * normalised on the way in, d_s with w >= 0), weights the pair by huber = delta > huber_deg ? huber_deg / delta : 1 (delta: difference of the two rotation angles, degrees)
 * and solves q_s (x) x = x (x) q_i over all pairs: x is the right singular vector of the smallest singular value of the stacked huber (L(d_s) - R(d_i)).
 *   x = q_ItoS; the mounting rotation of the state is its conjugate, q_LtoI = conj(q_ItoS) (calib_helper_lvi.cpp:67-68).  Reported with w >= 0.
 *   sigma: the four singular values, descending.  ok = n_pairs >= min_pairs and sigma[2] > min_sigma (the reference's 15 and cov(2) > 0.25); with fewer pairs the record
 *   holds the identity and zero sigmas, as the reference returns before the SVD.
 *   Prefix k uses the poses 0 .. prefix_len[k] - 1.  Its pair list ends at the first j with t_j + tau >= MaxTime (:39-40) or a non-finite stamp.
 * The call is sensor-agnostic: camera odometry quaternions give q_ItoC the same way.  The spline is evaluated in LVX_FRAME_TRAJECTORY: no sensor offset of the state enters.
 * Two deviations from the reference: (1) a pair with an evaluation time outside [MinTime, MaxTime) — t_i + tau < MinTime — is skipped and counted in n_skipped, where the
 * reference's Evaluate would throw std::range_error; (2) the list of shifts tau of the odometry stamps: the same system at t + tau[s] for every s, whose sigma[3] is
 * smallest at the true time offset of the sensor (a coarse offset for lvx_set_time_offset_bounds' small interval); the reference has tau = 0 only.
 * A pair whose spline window holds a control quaternion that fails logq's unit check is skipped (and counted in n_skipped); the call then returns LVX_E_NONUNIT_QUAT with
 * everything else filled, as lvx_sample_trajectory does.  All sums are formed in a fixed order: two calls return the same bits.
 * results: [n_tau][n_prefix]; first_ok: [n_tau], lowest prefix index with ok, or -1.  tau NULL / n_tau 0: one shift of 0.  prefix_len NULL / n_prefix 0: one prefix of n.
 * LVX_E_ARG: NULL context / state / t / q / results / first_ok, n <= 0, a prefix list that is not non-decreasing with every entry in [1, n].  LVX_E_STATE: before
 * lvx_set_spline. */
typedef struct lvx_rotinit_options { double huber_deg; int32_t min_pairs; int32_t reserved; double min_sigma; } lvx_rotinit_options;   /* 1.0, 15, 0.25 */
typedef struct lvx_rotinit_result { double q_ItoS_xyzw[4]; double sigma[4]; int32_t n_poses, n_pairs, n_skipped, ok; } lvx_rotinit_result;
int lvx_rotinit_default_options(lvx_rotinit_options* opt);
int lvx_estimate_rotation(lvx_ctx* ctx, const double* state, int n, const double* t, const double* q_xyzw4, int n_prefix, const int32_t* prefix_len, int n_tau, const double* tau,
                          const lvx_rotinit_options* opt, lvx_rotinit_result* results, int32_t* first_ok);
/* The same on device memory: state_d (NULL: the state of lvx_set_state), t_d, q_xyzw4_d, prefix_len_d, tau_d, results_d and first_ok_d are device addresses (opt is a host
 * struct).  Only enqueues on the context's stream; a non-unit quaternion is reported by the next lvx_synchronize.  The device prefix list is not validated: an entry is
 * read clamped to [1, n]. */
int lvx_estimate_rotation_d(lvx_ctx* ctx, const double* state_d, int n, const double* t_d, const double* q_xyzw4_d, int n_prefix, const int32_t* prefix_len_d, int n_tau,
                            const double* tau_d, const lvx_rotinit_options* opt, lvx_rotinit_result* results_d, int32_t* first_ok_d);

#ifdef __cplusplus
}
#endif
#endif /* LVX_H */
