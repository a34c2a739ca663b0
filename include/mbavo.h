/*
 * mbavo.h -- C ABI of the MI355X-native blur-aware photometric tracking path.
 *
 * Drop-in boundary for the hot path of ethliup/MBA-VO (src/ba_tracker).  Every
 * entry point names the reference interface it replaces (paths relative to the
 * reference's src/).  Plain pointers and sizes only; `d_` = device (HIP) memory,
 * `h_` = host memory.  All functions return 0 on success, a positive hipError_t
 * value on a HIP failure, or a negative MBAVO_E_* code; none of them falls back
 * to a CPU path -- without a usable HIP device the compute entry points fail.
 *
 * The C++ API with the reference's exact signatures (namespace SLAM::VO) is in
 * mba-vo_amd/csrc/ba_tracker.h and is exported by the same shared library.
 */
#ifndef MBAVO_H
#define MBAVO_H

#ifdef __cplusplus
extern "C" {
#endif

#define MBAVO_E_ARG (-1)      /* bad argument (null pointer, unsupported spline degree, ...) */
#define MBAVO_E_RANGE (-2)    /* a blur sample fell outside the spline's knot range (SplineFunctor.h:13-19 has no check) */
/* "Inside the knot range", everywhere in this library, is decided on the double before any conversion to int: with
 * tn = (t - t0) / dt, a time t is inside iff tn > -1.0 && tn < (double)(N - k + 1) (N knots, spline degree k, N >= k).  For every
 * tn that fits an int that is trunc(tn) >= 0 && trunc(tn) + k <= N; a tn in (-1, 0) is inside (segment 0, u < 0: the reference's
 * truncation toward zero).  A NaN or infinite time, start time or spacing, and a time so far off that its segment number does
 * not fit an int (nanosecond stamps on a spline in seconds), fail the comparisons: they are OUTSIDE, and no knot address is ever
 * formed from them -- where a kernel goes on, it does so on a segment index held to [0, N - k]. */
#define MBAVO_E_NODEVICE (-3) /* no HIP device: the product has no CPU fallback */
#define MBAVO_E_TIMEOUT (-4)  /* a bounded device-side wait ran out (a peer rank never arrived; a wedged device) */

typedef struct mbavo_ctx mbavo_ctx;

/* One alignment problem = the argument list of evaluate_cost_hessian_gradient
 * (ba_tracker/spline_update_step.h:70-87) plus the CudaSharedStorages fields it
 * reads (spline_update_step.h:18-58), as POD.  All pointers are DEVICE pointers
 * except h_start_idx.
 * ZERO-INITIALISE the struct (memset / `= {0}`) before filling it in: fields appended by later library versions
 * (grad_fp16, num_residuals -- ABI 2; the scheduling / solver-form tails of the option structs -- ABI 3) select optional
 * behaviour and must read 0 when a caller does not know them.
 * mbavo_abi_version() returns the struct revision the loaded library expects (MBAVO_ABI_VERSION of this header). */
#define MBAVO_ABI_VERSION 3
typedef struct mbavo_problem {
    int S;                                /* n_vir_poses_per_frame */
    int F;                                /* n_frames */
    int K;                                /* num_keypoints */
    int P;                                /* patch_size */
    int N;                                /* num_ctrl_knots */
    int H, W;                             /* im_size_HW; H*W <= 2^29 (32-bit tap offsets), else MBAVO_E_ARG */
    const unsigned char *d_ref_img;       /* cuda_ref_img, H*W u8 */
    const float *d_ref_dIxy;              /* cuda_dIxy_ref, H*W*2 interleaved [dx,dy] */
    const unsigned char *const *d_cur_imgs; /* storages.cuda_cur_images: device array of F device pointers */
    const double *d_kp_xy;                /* keypoint i at d_kp_xy[i*kp_stride + {0,1}] */
    int kp_stride;                        /* 2 = packed xy; 3 = Core::Vector2d array, pointer at .values */
    const double *d_kp_z;                 /* storages.cuda_keypoint_depth_z, K */
    const int *d_pattern;                 /* storages.cuda_local_patch_pattern_xy, P*2 (dx,dy) */
    const unsigned char *d_outlier;       /* storages.cuda_keypoints_outlier_flags, K, or NULL */
    int num_bad;                          /* storages.num_bad_keypoints */
    double intrinsics[4];                 /* fx fy cx cy at this pyramid level */
    const double *d_cap_time;             /* storages.cuda_img_cap_time, F */
    const double *d_exp_time;             /* storages.cuda_img_exp_time, F */
    double t0, dt;                        /* spline_start_time, spline_sample_dt */
    const double *d_knots_t;              /* storages.cuda_spline_ctrl_knots_data_t, 3N */
    const double *d_knots_R;              /* storages.cuda_spline_ctrl_knots_data_R, 4N xyzw */
    const int *h_start_idx;               /* cpu_ctrl_knot_start_indices, F (host; only read by host merges) */
    double huber_a;
    int grad_fp16;                        /* 0: d_ref_dIxy is float [dx,dy] per pixel (reference layout, Gradient.h:16-75);
                                             1: d_ref_dIxy is IEEE half [dx,dy] per pixel (4 B/pixel, BASELINE configs[4]).
                                             Central differences of an 8-bit image are multiples of 0.5 in [-127.5, 127.5],
                                             exactly representable in fp16, so both formats see identical tap values (results agree to rounding).
                                             2: d_ref_dIxy is the packed keyframe of mbavo_pack_keyframe_u8 (4 B/pixel: intensity and both
                                             differences in one word; H/g passes read nothing else of the keyframe, cost-only passes d_ref_img).
                                             All problems of one mbavo_eval_batch call must use the same format. */
    long long num_residuals;              /* 0: the blocks are scaled by 1/((K - num_bad)*F*P) of THIS problem
                                             (inv_num_residuals, spline_update_step.cpp:116-117).  > 0: by 1/num_residuals --
                                             the residual count of the WHOLE problem a keypoint / frame shard belongs to, so
                                             that the shards' packed blocks simply add up to the whole problem's (multi-GPU:
                                             mbavo_shard_keypoints / mbavo_shard_frames fill it in) */
} mbavo_problem;

/* ---- context: owns all device scratch (replaces initialize/free_shared_cuda_storages,
 * ba_tracker/spline_update_step.cpp:9-95, for the fused path) */
int mbavo_create(mbavo_ctx **out, int device_id);
int mbavo_destroy(mbavo_ctx *ctx);
int mbavo_set_stream(mbavo_ctx *ctx, void *hip_stream); /* NULL = default stream */
/* sizeof of the library's own structs, for a foreign-language binding to check its mirror against: 0 mbavo_problem,
 * 1 mbavo_track_opts, 2 mbavo_lm_batch_opts, 3 mbavo_vo_options, 4 mbavo_engine_opts, 5 mbavo_vo_state, 6 mbavo_trace_rec,
 * 7 mbavo_level, 8 mbavo_lm_batch_result, 9 mbavo_vo_info */
int mbavo_sizeof(int which);

/* ---- options instead of environment variables (ABI 3).  The reference configures everything through one plain struct
 * (BlurAwareDirectTrackerOptions, blur_aware_direct_tracker.h:15-67); so does this library: every switch that changes results or
 * scheduling is a field -- here for the evaluation engine (all callers of the context), in the tails of mbavo_track_opts /
 * mbavo_vo_options / mbavo_lm_batch_opts for the LM loops.  A ZEROED struct is the default everywhere: flags are tri-state
 * (0 default, 1 on, -1 off), numbers 0 = default.  The MBAVO_* environment variables of the A/B tools still override an option
 * (one reader: csrc/options.h read_env_overrides); only the diagnostics MBAVO_TIMING / MBAVO_LM_STAMPS / MBAVO_LM_STATS are
 * environment-only. */
typedef struct mbavo_engine_opts {
    int sample_parallel;        /* small lists on the sample-parallel kernel: 0 by size, 1 wherever the list allows, -1 never [MBAVO_SP] */
    int single_launch;          /* small lists in ONE launch (pose prologue + ticket epilogue); default on            [MBAVO_ONE] */
    int fused_pose;             /* pose entries as the fused kernel's prologue; default on                            [MBAVO_FUSED_POSE] */
    int fused_pose_max_samples; /* ... up to this many blur samples; default 8                                        [MBAVO_FUSED_POSE_MAX_S] */
    int persistent;             /* persistent evaluation kernels under the host-driven LM loop; default on            [MBAVO_PERSIST] */
    int prelaunch;              /* next pyramid level's persistent kernel enqueued behind the running one; default on [MBAVO_PRELAUNCH] */
    int tiles_per_cu;           /* default 1                                                                          [MBAVO_TILES_PER_CU] */
    int min_tile_pixels;        /* default 256                                                                        [MBAVO_MIN_TILE_PX] */
    int sp_max_slot_tiles;      /* default 64                                                                         [MBAVO_SP_MAX_SLOT_TILES] */
    int reserved[7];
} mbavo_engine_opts;
int mbavo_set_engine_opts(mbavo_ctx *ctx, const mbavo_engine_opts *opts); /* NULL = all defaults */
int mbavo_get_engine_opts(mbavo_ctx *ctx, mbavo_engine_opts *opts_out);   /* what was set (not the environment's overrides) */
int mbavo_packed_len(int spline_deg_k);                 /* E = (6k+1)(6k+2)/2 */

/* ---- fused evaluation of B independent problems in one pass (poses -> residual /
 * Jacobian -> packed normal-equation blocks).  Replaces steps (1)-(5) of
 * evaluate_cost_hessian_gradient (spline_update_step.cpp:127-227) for every problem.
 * Asynchronous on the context's stream.
 *   d_frame_blocks: sum_b F_b rows of E doubles, problem-major then frame:
 *                   [cost | g_local (6k) | upper(H_local)] == cuda_frame_cost_gradient_hessian_tR
 *   d_patch_cost  : sum_b F_b*K_b doubles (slot 0 of every patch block), or NULL
 *   d_valid       : sum_b F_b doubles, number of in-bounds pixels per frame, or NULL
 * with_hessian = 0 is the reference's cost-only mode (H/g slots left untouched).
 * The sample times are read on the device (d_cap_time, d_exp_time: no host code sees them).  A blur sample outside the knot
 * range -- a NaN or infinite capture or exposure time included -- is evaluated on the nearest segment that exists and raises
 * the context's range status; this call, being asynchronous, still returns 0, and the next call on the context that
 * synchronises (mbavo_eval, mbavo_lm_batch, mbavo_lm_batch_levels) returns MBAVO_E_RANGE once. */
int mbavo_eval_batch(mbavo_ctx *ctx, int B, const mbavo_problem *h_problems, int spline_deg_k,
                     int with_hessian, double *d_frame_blocks, double *d_patch_cost, double *d_valid);

/* The same evaluation ENDING IN THE REFERENCE'S UNIT: evaluate_cost_hessian_gradient with H / g outputs
 * (spline_update_step.cpp:97-241) ends in merge_hessian_gradient_cost (:232-239, merge_hessian_gradient_cost.cpp:39-86),
 * i.e. in [cost | g (6N) | H (6N x 6N, column-major, both triangles)] -- mbavo_eval_batch alone leaves the PACKED per-frame
 * blocks.  d_systems receives mbavo_system_len(N_b) doubles per problem, back to back in problem order (the layout of
 * mbavo_merge_device), d_frame_blocks the packed blocks as before.  Where every problem has one frame and N == k control
 * knots (start index 0: the scatter is a plain unpack) the finalize step stores the system itself -- no merge launch, the
 * evaluation costs what mbavo_eval_batch costs; otherwise mbavo_merge_device's kernel runs behind it (h_start_idx required).
 * Asynchronous on the context's stream. */
int mbavo_eval_batch_merged(mbavo_ctx *ctx, int B, const mbavo_problem *h_problems, int spline_deg_k,
                            double *d_frame_blocks, double *d_systems, double *d_patch_cost, double *d_valid);

/* synchronous single problem, host outputs == evaluate_cost_hessian_gradient
 * (spline_update_step.h:70-87): h_H is the 6N x 6N column-major system, h_g 6N;
 * pass NULL, NULL for cost-only.  d_patch_blocks (F*K*E, may be NULL) receives slot 0
 * of every patch block at stride E like cuda_patch_cost_gradient_hessian_tR.
 * MBAVO_E_RANGE, with the host outputs untouched, if a blur sample lies outside the knot range: a NaN or infinite sample time
 * (from the capture or the exposure time) is outside, as is any time whose segment number does not fit an int. */
int mbavo_eval(mbavo_ctx *ctx, const mbavo_problem *h_problem, int spline_deg_k,
               double *h_total_cost, double *h_H, double *h_g, double *d_patch_blocks);

/* ---- the reference's five launchers, one call each (device buffers caller-owned,
 * synchronous like the reference). */
/* compute_virtual_camera_poses (ba_tracker/compute_virtual_camera_poses.h:18-33) */
int mbavo_compute_virtual_camera_poses(int S, int F, const double *d_cap, const double *d_exp, int spline_deg_k,
                                       double t0, double dt, const double *d_knots_t, const double *d_knots_R,
                                       double *d_poses, double *d_J_t, double *d_J_R);
/* compute_local_patches_xy (ba_tracker/compute_local_patches_xy.h:10-18); xy arrays are Core::Vector2d (24 B) */
int mbavo_compute_local_patches_xy(int S, int F, const double *d_poses, const void *d_keypoints_vec2d,
                                   const double *d_kp_z, int K, const double intrinsics[4], const int HW[2],
                                   void *d_local_patches_vec2d);
/* compute_pixel_jacobian_residual (ba_tracker/compute_hessian_gradients_cost.h:11-29) */
int mbavo_compute_pixel_jacobian_residual(const unsigned char *d_I_ref, const float *d_dIxy_ref,
                                          const unsigned char *const *d_I_cur_imgs, int S, int F,
                                          const double *d_poses, int spline_deg_k, const double *d_J_t,
                                          const double *d_J_R, const void *d_local_patches_vec2d,
                                          const double *d_kp_z, int K, const int *d_pattern, int P,
                                          const double intrinsics[4], const int HW[2],
                                          double *d_pixel_residuals, double *d_pixel_jacobians_or_null);
/* compute_patch_cost_gradient_hessian (compute_hessian_gradients_cost.h:52-60) */
int mbavo_compute_patch_cost_gradient_hessian(int F, int K, int P, int spline_deg_k, const double *d_residuals,
                                              const double *d_jacobians_or_null, double huber_a,
                                              double inv_num_residuals, double *d_patch_blocks);
/* compute_frame_cost_gradient_hessian (compute_hessian_gradients_cost.h:62-68) */
int mbavo_compute_frame_cost_gradient_hessian(int F, int K, int spline_deg_k, const double *d_patch_blocks,
                                              int eval_gradient_hessian, const unsigned char *d_outlier_or_null,
                                              double *d_frame_blocks);
/* merge_hessian_gradient_cost (ba_tracker/merge_hessian_gradient_cost.h:8-15): D2H + scatter */
int mbavo_merge_hessian_gradient_cost(int F, int spline_deg_k, const double *d_frame_blocks, const int *h_start_idx,
                                      int N, double *h_total_cost, double *h_H, double *h_g);
/* the scatter alone, on host blocks (merge_hessian_gradient_cost.cpp:39-86) */
int mbavo_merge_host(int F, int spline_deg_k, const double *h_frame_blocks, const int *h_start_idx, int N,
                     double *h_total_cost, double *h_H, double *h_g);
/* solve_normal_equation (ba_tracker/solve_normal_equation.h:10-35): x = -A^+ b; 0 = Jacobi SVD, 1 = LDLT.
 * Deviation from the reference, on by default: for solver_type 0 a positive definite system whose LDL^T pivot ratio is at
 * most 1e8 is solved by LDL^T instead of the Jacobi SVD (the same x to rounding x cond(A); the batched LM additionally
 * refines in double-double up to a ratio of 1e13).  MBAVO_FAST_SOLVE=0 in the environment (read once per
 * mbavo_solve_normal_equation / mbavo_optimize_trajectory / mbavo_lm_batch call) reproduces solve_normal_equation.h case 0
 * -- JacobiSVD::solve, minimum-norm least squares -- for every system; rank-deficient systems always take it. */
int mbavo_solve_normal_equation(const double *h_A_colmajor, const double *h_b, int n, int solver_type, double *h_x);

/* ---- host control flow that decides how often the path runs */
/* LevenbergMarquardtStrategy (ba_tracker/levenberg_marquardt_strategy.h:8-27) */
typedef struct mbavo_lm mbavo_lm;
mbavo_lm *mbavo_lm_new(void);
void mbavo_lm_delete(mbavo_lm *);
void mbavo_lm_reset(mbavo_lm *);
void mbavo_lm_step_accepted(mbavo_lm *, double step_quality);
void mbavo_lm_step_rejected(mbavo_lm *);
double mbavo_lm_get_radius(mbavo_lm *);
/* TrustRegionStepEvaluator (ba_tracker/trust_region_step_evaluator.h:37-80) */
typedef struct mbavo_tr mbavo_tr;
mbavo_tr *mbavo_tr_new(int max_consecutive_nonmonotonic_steps);
void mbavo_tr_delete(mbavo_tr *);
void mbavo_tr_reset(mbavo_tr *, double initial_cost);
double mbavo_tr_step_quality(mbavo_tr *, double cost, double model_cost_change);
void mbavo_tr_step_accepted(mbavo_tr *, double cost, double model_cost_change);

/* SplineSE3 pieces (core/common/Spline.h:222-330) on flat knot arrays.  mbavo_spline_get_pose: MBAVO_E_RANGE, with the
 * outputs untouched, if t is outside the knot range (a NaN or infinite t included; the reference asserts). */
int mbavo_spline_get_pose(int spline_deg_k, double t0, double dt, const double *h_knots_t, const double *h_knots_R,
                          int N, double t, double h_t_out[3], double h_q_out_xyzw[4],
                          double *h_J_t_or_null /*3x3k*/, double *h_J_R_or_null /*4x3k*/);
int mbavo_spline_plus(const double *h_knots_t, const double *h_knots_R, int N, const double *h_step /*6N*/,
                      double *h_cand_t, double *h_cand_R);
/* SplineFunctor.h:13-19, defined for every double: trunc((t - t0) / dt) held to [INT_MIN, INT_MAX], and INT_MIN if the
 * quotient is NaN, so that a caller's `idx < 0` test fails safe.  (The reference's plain conversion is undefined there.)
 * mbavo_optimize_trajectory's h_start_idx_out holds these values. */
int mbavo_segment_start_index(double t, double t0, double dt);

/* ---- LM loop over the pyramid: BlurAwareDirectTracker::optimizeTrajectory
 * (ba_tracker/blur_aware_direct_tracker.cpp:544-924) on device-resident levels */
typedef struct mbavo_level {
    int H, W, K, P, S;
    const unsigned char *d_ref_img;
    const float *d_ref_dIxy;
    const unsigned char *const *d_cur_imgs; /* device array of F device pointers */
    const double *d_kp_xy;                  /* packed K*2 */
    const double *d_kp_z;
    const int *d_pattern;
} mbavo_level;
typedef struct mbavo_track_opts {
    int num_levels, spline_deg_k, max_num_iterations, max_consecutive_nonmonotonic_steps, solver_type;
    double intrinsics[4]; /* level 0 */
    double huber_k, min_step_quality, min_abs_cost_decrease, max_chi_square_error;
    /* ABI 3 -- zero = default.  Solver form: the pivot ratio up to which LDL^T stands in for solve_normal_equation.h's
     * solvers (0: 1e8; < 0: never -- the Jacobi SVD / pivoted LDL^T for every system; > 1: that ratio)        [MBAVO_FAST_SOLVE] */
    double fast_solve_ratio;
    int speculate;      /* candidates evaluated WITH H / g: 0 on the persistent levels, 1 every level, -1 never [MBAVO_SPECULATE] */
    int persist_levels; /* one persistent kernel for all levels of a call; default on                          [MBAVO_PERSIST_LEVELS] */
    int ride_along;     /* the next pyramid level's first evaluation rides along with this level's candidates (same
                           results, one dependent evaluation less per level); default on; 2 (tests): on, and every
                           ride-along is treated as taken at other knots, i.e. waited out and redone           [MBAVO_RIDE_ALONG] */
    int resum;          /* the H / g evaluation behind an accepted step whose outlier flags changed is the candidate's,
                           summed again on the device under the new flags and scale (bit-identical results, no pixel
                           work); default on                                                                   [MBAVO_RESUM] */
    int reserved[2];
} mbavo_track_opts;
typedef struct mbavo_trace_rec {
    int level, iter, kind; /* 0 initial evaluation, 1 accepted, 2 rejected, 3 invalid step */
    int num_outliers;
    double radius, eval_cost, candidate_cost, model_change, quality;
} mbavo_trace_rec;
/* knots are updated in place; returns the number of trace records (>= 0) or an error (< 0): MBAVO_E_RANGE, before anything
 * is launched and with the knots untouched, if a blur sample of any level lies outside the knot range (NaN and infinite
 * times included) */
int mbavo_optimize_trajectory(mbavo_ctx *ctx, const mbavo_track_opts *opts, const mbavo_level *levels, int F,
                              const double *h_cap, const double *h_exp, double t0, double dt,
                              double *h_knots_t, double *h_knots_R, int N, int *h_start_idx_out,
                              double *h_final_cost, mbavo_trace_rec *trace, int trace_cap);

/* ---- device-side LM over a batch of independent problems (one pyramid level each): optimizePyramidLevel
 * (ba_tracker/blur_aware_direct_tracker.cpp:590-924) for B problems at once with the packed blocks, the 6N x 6N
 * assembly / damping / solve (solve_normal_equation.h:10-35), the radius and step-evaluator state and the outlier
 * statistics all on the device; the host only reads a done-counter: behind an event, one iteration late, while the next
 * iteration is already queued (sync_every <= 0, the default), or after draining the stream every `sync_every` iterations.
 * Each problem's knots (d_knots_t / d_knots_R, device) are updated in place; d_outlier / num_bad of the input are
 * ignored (flags start cleared, as at the start of a level).  Trace records as mbavo_optimize_trajectory writes
 * them (level = 0), `trace_cap` per problem.  At most 16 control knots per problem (the reference's
 * max_num_ctrl_knots: two 6N x 6N work areas in the 160 KB of LDS); more returns MBAVO_E_ARG.  Returns 0 or an error:
 * MBAVO_E_RANGE if a blur sample of any problem lies outside its knot range at any evaluation of the call -- a NaN or infinite
 * capture or exposure time is outside, as is a time whose segment number does not fit an int --, with nothing of the call left in
 * flight and the context as good as new (the results and the knots of such a call are not meaningful). */
typedef struct mbavo_lm_batch_opts {
    int spline_deg_k, max_num_iterations, max_consecutive_nonmonotonic_steps, solver_type, sync_every;
    double min_step_quality, min_abs_cost_decrease, max_chi_square_error;
    /* ABI 3 -- zero = default */
    double fast_solve_ratio; /* as mbavo_track_opts.fast_solve_ratio                                                [MBAVO_FAST_SOLVE] */
    double refined_ratio;    /* pivot ratio up to which the stand-in, refined with double-double residuals, is admitted:
                                0: 1e13; < 0: never (plain stand-in only); > 1: that ratio                          [MBAVO_LM_REFINE] */
    int eig;                 /* the wide workgroup (eigenvalue Jacobi as the fallback) for n <= 48; default on       [MBAVO_LM_EIG] */
    int pose_entries;        /* the solve launch writes the candidate's pose entries; default on                     [MBAVO_LM_POSES] */
    int defer_finalize;      /* the LM kernels sum the tile partials themselves; default on                          [MBAVO_LM_DEFER] */
    int retile;              /* a second, finer tiling for the late slots of big batches; default on                 [MBAVO_LM_RETILE] */
    int groups;              /* independent groups on their own streams: 0 = 2 from 384 problems, else 1; 1 .. 8     [MBAVO_LM_GROUPS] */
    int reserved[5];
} mbavo_lm_batch_opts;
typedef struct mbavo_lm_batch_result {
    int iterations, accepted, rejected, invalid, num_outliers, num_trace;
    double initial_cost, final_cost, radius;
} mbavo_lm_batch_result;
int mbavo_lm_batch(mbavo_ctx *ctx, int B, const mbavo_problem *h_problems, const mbavo_lm_batch_opts *opts,
                   mbavo_lm_batch_result *h_results_or_null /*B*/, mbavo_trace_rec *h_trace_or_null /*B x trace_cap*/,
                   int trace_cap);
/* mbavo_lm_batch for B pairs with L pyramid levels each: optimizeTrajectory (blur_aware_direct_tracker.cpp:544-588) per pair,
 * levels L-1 .. 0 on the device, each a fresh optimizePyramidLevel (outlier flags and count cleared, iteration 0 evaluated, LM
 * radius and step evaluator reset) starting from the knots the coarser level ended at.  A pair goes on to its next level the
 * moment its current one ends: pairs do not wait for each other.
 * h_problems: B x L, pair-major -- entry b*L + l is pair b at pyramid level l (l = 0 finest).  1 <= L <= 8.  Every entry follows
 * the rules of mbavo_lm_batch; within a pair every level has the same F, N, t0, dt, huber_a, d_cap_time, d_exp_time, d_knots_t and
 * d_knots_R (the SAME device pointers: the knots are shared and updated in place) and the same h_start_idx contents; otherwise
 * MBAVO_E_ARG with nothing launched.  The intrinsics are the caller's, per entry: mbavo_optimize_trajectory's results need level
 * 0's divided by 1 << l.
 * Results per pair: iterations, accepted, rejected, invalid and num_trace summed over the levels; initial_cost = iteration 0 of
 * the coarsest level; final_cost, num_outliers and radius as level 0 ends.  Trace records (trace_cap per pair) in the order
 * mbavo_optimize_trajectory writes them for the same pair: level = the pyramid level, iter restarting per level.
 * mbavo_lm_batch_opts as for mbavo_lm_batch (groups split the batch at pair boundaries); `retile` has no effect with L > 1 (the
 * finer second tiling targets the whole list, not a set of active entries that mixes levels).  L = 1 is mbavo_lm_batch. */
int mbavo_lm_batch_levels(mbavo_ctx *ctx, int B, int L, const mbavo_problem *h_problems /* B x L, pair-major */,
                          const mbavo_lm_batch_opts *opts, mbavo_lm_batch_result *h_results_or_null /*B*/,
                          mbavo_trace_rec *h_trace_or_null /*B x trace_cap*/, int trace_cap);

/* ---- keyframe input producers on device (core/measurements/ImagePyramid.h:59-99,
 * core/image_proc/Gradient.h:16-75) */
int mbavo_pyramid_down_u8(const unsigned char *d_src, int H, int W, unsigned char *d_dst, void *hip_stream);
/* levels 1 .. num_levels-1 (level l: (H0 >> l) x (W0 >> l)) below h_level_ptrs[0] on the context's stream, three levels per launch:
 * the same 2 x 2 box with truncation per level (ImagePyramid.h:59-99); h_level_ptrs: host array of device pointers, num_levels <= 8 */
int mbavo_pyramid_levels_u8(mbavo_ctx *ctx, unsigned char *const *h_level_ptrs, int H0, int W0, int num_levels);
int mbavo_image_gradients_u8(const unsigned char *d_src, int H, int W, float *d_dIxy, void *hip_stream);
/* same gradient image stored as IEEE half pairs (fp16 pyramid, mbavo_problem.grad_fp16 = 1) */
int mbavo_image_gradients_u8_half(const unsigned char *d_src, int H, int W, void *d_dIxy_half, void *hip_stream);
/* packed keyframe (mbavo_problem.grad_fp16 = 2): ONE 32-bit word per pixel -- bits 0-7 the intensity, bits 8-16 and 23-31 the
 * doubled central differences 2 dI/dx, 2 dI/dy of Gradient.h:16-75 as 9-bit two's complement (zero on the 1-pixel border).  Holds
 * exactly what the u8 image and its float gradient image hold (4 bytes per pixel instead of 9); d_ref_dIxy then points at it. */
int mbavo_pack_keyframe_u8(const unsigned char *d_src, int H, int W, void *d_packed /* H*W uint32 */, void *hip_stream);

/* gradient magnitude image (Gradient.h:56-71, the detector's score) */
int mbavo_gradient_magnitude_u8(const unsigned char *d_src, int H, int W, float *d_mag, void *hip_stream);
/* semi-dense keypoints of pyramid level `level` with their depths: candidates = magnitude > score_threshold
 * (core/feature_detectors/FeatureDetectorSemiDense.cpp:27-43), one per grid cell (FeatureDetectorBase.cpp:49-91;
 * cell_H/cell_W <= 0: every candidate, row-major), depth at the level-0 position of the H0 x W0 float map
 * d_depth_z, z < 1e-2 dropped (ba_tracker/blur_aware_direct_tracker.cpp:389-415).  Device in, device out (packed
 * K x 2 doubles + K doubles, at most `cap` written); *h_count = number found.  Synchronous on the context's stream. */
int mbavo_detect_semidense(mbavo_ctx *ctx, const unsigned char *d_img, int H, int W, int level, int H0, int W0,
                           int cell_H, int cell_W, float score_threshold, const float *d_depth_z,
                           double *d_kp_xy, double *d_kp_z, int cap, int *h_count);

/* ---- depth maps as the datasets store them.  tmpProcessKeyframe (ba_tracker/blur_aware_direct_tracker.cpp:368-386) has two
 * depth inputs and neither is z-depth; a depth format says what a map holds:
 *   0  float z, as mbavo_detect_semidense and mbavo_vo_* take it
 *   1  float distance along the viewing ray ("unreal": Utils::load_depthMap, utils/InputOutput.cpp:12-37, then
 *      Utils::convert_ray_d_to_z, utils/Geometry.cpp:11-36, for a pinhole camera without distortion, CameraPinhole.cpp:79-95)
 *   2  uint16, z = value / depth_unit ("eth3d": a 16-bit image divided by 5000)
 * The conversions are defined here.  (x0, y0) is the level-0 pixel, intrinsics (fx, fy, cx, cy) are level 0's, all arithmetic
 * is IEEE double without contraction:
 *   format 1   d = map[y0][x0]; if (depth_max > 0 && d > depth_max) d = 0;
 *              xn = ((double)x0 - cx) / fx; yn = ((double)y0 - cy) / fy; n = sqrt(xn*xn + yn*yn + 1.0)  (summed left to right);
 *              z = (float)((double)d * (1.0 / n))
 *   format 2   z = (float)((double)v / (double)depth_unit)
 * followed, where a keypoint's depth is tested, by the test of format 0: !((double)z < 1e-2).  With unit 5000 the value 50 gives
 * float 0.01, whose double lies below 1e-2: no depth.
 * These formulas are the specification.  Two steps of the reference are not pinned by its source -- the order in which Eigen's
 * norm() sums the three squares, and OpenCV's float division `depthf / 5000` -- so the reference may differ from them in the last
 * float bit of z (as with the unpinned JacobiSVD of the solver).
 *
 * mbavo_depth_to_z converts a whole H x W map (device, contiguous; format 2: uint16 elements) to float z in d_z: ONE launch on
 * the context's stream, nothing waited for; format 0 copies.  For callers of mbavo_detect_semidense and mbavo_vo_*, which take
 * float z; mbavo_pairs_* reads the formats directly (mbavo_pairs_opts.depth_format) and converts only the pixels it looks up,
 * with the same device function.  depth_unit is read by format 2 only, depth_max by format 1 only.  MBAVO_E_ARG, nothing
 * launched: a format other than 0, 1, 2; format 2 with depth_unit <= 0; a NULL pointer; H or W < 1 (or H * W >= 2^31). */
int mbavo_depth_to_z(mbavo_ctx *ctx, int depth_format, const void *d_depth, int H, int W, const double intrinsics[4],
                     float depth_unit, float depth_max, float *d_z);

/* ---- images of a camera with lens distortion.  Every entry point of this library takes images of an ideal pinhole camera; the
 * reference models a lens with radial-tangential distortion (core/sensors/DistortionRadTan.cpp:26-36, CameraPinhole.cpp:24-42,
 * 79-95) and removes it before tracking (core/image_proc/Undistort.cpp:17-52: a per-pixel source map, then cv::remap on every
 * image).  mbavo_camera_radtan is the camera the raw images come from; the undistorted `to` camera is a pinhole camera given by
 * its intrinsics (fx, fy, cx, cy) and size.  The map and the remap are defined here.
 * The map (Undistort::computePixelMappings): for output pixel (c, r), all arithmetic IEEE double without contraction, left to
 * right as written:
 *   xn = ((double)c - cx_to) / fx_to;   yn = ((double)r - cy_to) / fy_to;      (unproject at z = 1)
 *   x  = (xn * 1.0) / (1.0 + 1e-8);     y  = (yn * 1.0) / (1.0 + 1e-8);        (project: CameraPinhole.cpp:30-31)
 *   mx2 = x*x; my2 = y*y; mxy = x*y; rho2 = mx2 + my2; rad = k1*rho2 + k2*rho2*rho2;
 *   xd = x + x*rad + 2.0*p1*mxy + p2*(rho2 + 2.0*mx2);
 *   yd = y + y*rad + 2.0*p2*mxy + p1*(rho2 + 2.0*my2);
 *   sx = (float)(fx_from*xd + cx_from);  sy = (float)(fy_from*yd + cy_from);
 * The remap of a u8 image through (sx, sy):
 *   X = (double)sx; Y = (double)sy; x0 = floor(X); y0 = floor(Y); ax = X - x0; ay = Y - y0;
 *   p(y, x) = src[y][x] inside the raw image, 0 outside                         (BORDER_CONSTANT 0)
 *   v = (1.0-ay)*((1.0-ax)*p00 + ax*p01) + ay*((1.0-ax)*p10 + ax*p11);          (p00 = p(y0, x0), p01 = p(y0, x0+1), p10 = p(y0+1, x0))
 *   out = (unsigned char)(int)(v + 0.5)
 * A non-finite sx or sy, or |X| or |Y| >= 2^30, gives 0.
 * These formulas are the specification.  cv::remap's INTER_LINEAR works in fixed point (5 fractional bits of the coordinates,
 * 15-bit weights) and is not pinned by the reference's source, so the reference may differ from them by a grey level (as with
 * `depthf / 5000` above).  Note that the 1 + 1e-8 of `project` moves entries off the pixel grid even for a camera without
 * distortion (every one in double, those near the image origin in float as well); the rounding of the remap returns such an
 * image byte for byte all the same (tests/test_pairs_undistort_api.py, up to 480 x 640).
 *
 * mbavo_undistort_map writes the H x W map of the `to` camera (interleaved [sx, sy], 8 H W bytes); mbavo_undistort_u8 remaps one
 * Hs x Ws image through an H x W map into an H x W image.  ONE launch each on the context's stream, nothing waited for; device
 * pointers, contiguous, of any alignment their element type allows.  For callers of mbavo_vo_* and mbavo_detect_semidense;
 * mbavo_pairs_* remaps where it copies the level-0 images anyway (mbavo_pairs_opts.undistort), with the same device functions.
 * MBAVO_E_ARG, nothing launched: a NULL pointer; a size < 1, or H * W or Hs * Ws > 2^22; fx or fy equal to 0 on either camera. */
typedef struct mbavo_camera_radtan {       /* the camera the raw images come from: CameraPinhole + DistortionRadTan */
    int H, W;                              /* raw image size; H * W <= 2^22 */
    double intrinsics[4];                  /* fx fy cx cy of the raw camera */
    double dist[4];                        /* k1 k2 p1 p2 */
} mbavo_camera_radtan;                     /* 72 bytes, no padding */
int mbavo_camera_radtan_size(void);        /* sizeof(mbavo_camera_radtan) of the loaded library */
int mbavo_undistort_map(mbavo_ctx *ctx, const mbavo_camera_radtan *from, const double to_intrinsics[4], int H, int W,
                        float *d_map_xy /* H*W interleaved [sx, sy] */);
int mbavo_undistort_u8(mbavo_ctx *ctx, const unsigned char *d_src, int Hs, int Ws, const float *d_map_xy, int H, int W,
                       unsigned char *d_dst);
/* mbavo_undistort_u8 over n images in ONE launch on the context's stream (the image index in blockIdx.y), nothing waited for: image
 * i is the Hs x Ws image at d_src + i*Hs*Ws and goes to d_dst + i*H*W, all through the one H x W map.  The same bits as n calls of
 * mbavo_undistort_u8 (the same device function); the images are contiguous, so an image may start off a word boundary (H*W no
 * multiple of 4) and no alignment is assumed.  For callers of mbavo_vo_* and mbavo_detect_semidense with many images at hand.
 * MBAVO_E_ARG, nothing launched: what mbavo_undistort_u8 rejects; n < 1 or n > 65535. */
int mbavo_undistort_u8_batch(mbavo_ctx *ctx, const unsigned char *d_src /* n x Hs x Ws */, int n, int Hs, int Ws,
                             const float *d_map_xy /* H x W */, int H, int W, unsigned char *d_dst /* n x H x W */);

/* ---- the reference's second camera model: the unified / omnidirectional camera (core/sensors/CameraUnified.cpp:23-43) with the
 * mirror parameter xi, optionally followed by the same radial-tangential distortion.  Undistort (core/image_proc/Undistort.cpp:
 * 26-52) takes any camera as `from`; the `to` camera stays a pinhole camera.  The map, for output pixel (c, r), all arithmetic
 * IEEE double without contraction, left to right as written:
 *   xn = ((double)c - cx_to) / fx_to;   yn = ((double)r - cy_to) / fy_to;      (unproject at z = 1)
 *   X = xn * 1.0;  Y = yn * 1.0;                                                (the point; Z = 1.0)
 *   d  = sqrt(X*X + Y*Y + 1.0);                                                 (P3d.norm(); correctly rounded sqrt)
 *   rz = 1.0 / (1.0 + xi * d);                                                  (CameraUnified.cpp:28-29)
 *   x = X * rz;  y = Y * rz;
 *   mx2 .. xd, yd exactly as in the radial-tangential specification above, from (x, y)
 *   sx = (float)(fx_from*xd + cx_from);  sy = (float)(fy_from*yd + cy_from);
 * These formulas are the specification.  The order in which Eigen sums the three squares inside norm() is not pinned by the
 * reference's source (it may vectorise the reduction), so the reference may differ from them in the last bit of d (as with
 * `depthf / 5000` above).  `project` fails only for a point with z < 0, which cannot happen at z = 1: every entry is written.
 * Unlike the pinhole `project` the unified one has no 1 + 1e-8: with xi = 0 and zero coefficients the map is exactly
 * sx = (float)(fx_from*xn + cx_from), the pixel grid of the affine change of camera, whereas mbavo_undistort_map with zero
 * coefficients differs from that grid in the last bits.  All-zero `dist` stands for a camera without a distortion object (the
 * formulas then return x and y unchanged).  Everything downstream of the map (the remap, the pairs batch, the undistort = 2 depth
 * look-up) works from map entries and does not know the camera model.
 * mbavo_undistort_map_unified: as mbavo_undistort_map, ONE launch, nothing waited for.  MBAVO_E_ARG, nothing launched: what
 * mbavo_undistort_map rejects; an xi that is negative or not finite. */
typedef struct mbavo_camera_unified {      /* CameraUnified (+ optional DistortionRadTan) */
    int H, W;                              /* raw image size; H * W <= 2^22 */
    double intrinsics[4];                  /* fx fy cx cy of the raw camera */
    double xi;                             /* mirror parameter; finite and >= 0 */
    double dist[4];                        /* k1 k2 p1 p2; all zero = no distortion object */
} mbavo_camera_unified;                    /* 80 bytes, no padding */
int mbavo_camera_unified_size(void);       /* sizeof(mbavo_camera_unified) of the loaded library */
int mbavo_undistort_map_unified(mbavo_ctx *ctx, const mbavo_camera_unified *from, const double to_intrinsics[4],
                                int H, int W, float *d_map_xy);

/* ---- the input side of a BATCH of keyframe pairs: B pairs (sharp keyframe + its z-depth map, one blurred current frame) to the
 * B x L mbavo_problem array mbavo_lm_batch_levels takes, in a number of launches that does not depend on B.  Per pair and level
 * this is what mbavo_pyramid_levels_u8 (both images), mbavo_image_gradients_u8 / _half / mbavo_pack_keyframe_u8 (keyframe) and
 * mbavo_detect_semidense followed by a border filter give, bit for bit (ImagePyramid.h:59-99, Gradient.h:16-75,
 * FeatureDetectorSemiDense.cpp:27-43, FeatureDetectorBase.cpp:49-91, blur_aware_direct_tracker.cpp:389-415).
 * The object is owned by its context, has fixed shapes and allocates everything at creation.  mbavo_destroy frees the objects
 * that are left: their handles are invalid from then on and must not be passed to mbavo_pairs_destroy or any other call.
 * Keypoints: grid selection (every_candidate = 0: cell_H, cell_W >= 1, one pick per cell) or, with every_candidate = 1, the
 * "every candidate" mode of mbavo_detect_semidense (cell_H = cell_W = 0 there): every pixel above the threshold that has a depth
 * and passes the border test, in row-major order.  That mode's capacity is H_l * W_l keypoints per level, 24 bytes each: 9.8 MB
 * per 640 x 480 x 4 pair, and the byte count of mbavo_pairs_plan is what decides B.
 * Scope: one current frame per pair (F = 1); a level that ends with K = 0 is reported in the counts and stays in the array
 * as it is -- whether the LM accepts it is the LM's contract. */
typedef struct mbavo_pairs mbavo_pairs;
typedef struct mbavo_pairs_opts {          /* zero-initialise */
    int B, L, H, W;                        /* pairs (1 .. 32767), pyramid levels (1 .. 8), level-0 size; (H >> (L-1)) >= 8, same for W;
                                              H * W <= 2^22 (2048 x 2048) */
    int S[8], P[8];                        /* blur samples / patch size per level (>= 1 for every level < L) */
    const int *pattern_xy[8];              /* host (dx,dy) pairs per level, copied at creation */
    int spline_deg_k, N;                   /* 2 or 4; N control knots per pair, spline_deg_k <= N <= 16 */
    double intrinsics[4];                  /* level 0; level l gets them divided by 1 << l */
    double huber_a;
    float score_threshold; int cell_H, cell_W; /* as mbavo_detect_semidense; cell_* >= 1 and still >= 1 after / 1.414^l on every level */
    int border[8];                         /* per level: keypoints with x < m, x >= W_l - m, y < m or y >= H_l - m are dropped; 0 = keep all */
    int keyframe_format;                   /* 0 float gradients, 1 half, 2 packed word: the three values of mbavo_problem.grad_fp16 */
    int every_candidate;                   /* 0: grid selection.  1: no grid, every candidate is a keypoint (cell_H, cell_W are not read
                                              and may be 0).  Anything else: MBAVO_E_ARG */
    int depth_format;                      /* what the depth maps hold (see mbavo_depth_to_z).  0: float z.  1: float distance along the
                                              viewing ray.  2: uint16, z = value / depth_unit.  Anything else: MBAVO_E_ARG */
    float depth_unit;                      /* format 2: units per metre (eth3d: 5000); must be > 0 there (else MBAVO_E_ARG), not read otherwise */
    float depth_max;                       /* format 1: > 0: a distance above it counts as no depth (load_depthMap: 100); 0: no limit */
    int undistort;                         /* 0: the images are those of the pinhole camera `intrinsics`.  1: d_sharp / d_blur of prepare, update
                                              and track_frame are RAW images of the camera given to mbavo_pairs_set_camera (B x Hs x Ws,
                                              contiguous) and are remapped into the object; the depth maps are in the undistorted H x W
                                              geometry.  2: as 1, and the depth maps are raw-geometry Hs x Ws maps in depth_format.
                                              Anything else: MBAVO_E_ARG */
    union {                                /* (anonymous members: C11; in C++ an extension that GCC, Clang and MSVC all have -- a
                                              -pedantic C++ build warns here) */
        int reserved[3];                   /* the name these three words had: code that zeroes them keeps compiling and keeps its meaning */
        struct {
            int num_cameras;               /* 0: one camera for all pairs (`intrinsics`, mbavo_pairs_set_camera*).  G in 1 .. B: a set of G
                                              cameras, every pair assigned to one of them by mbavo_pairs_set_cameras; `intrinsics` is
                                              not read.  Anything else: MBAVO_E_ARG */
            int valid_radius;              /* 0: off, nothing changes.  r in 1 .. 64: the clearance test below with that radius; needs
                                              undistort != 0 or mask = 1.  Anything else, or r > 0 with undistort == 0 and mask == 0:
                                              MBAVO_E_ARG */
            union {
                int reserved2[1];          /* the name this last word had (the seven fields came out of `reserved`: the struct has the size it had) */
                int mask;                  /* 0: off, nothing changes.  1: the object holds caller-supplied masks (mbavo_pairs_set_masks, below)
                                              beside the clearance mask; valid_radius may then be 0 .. 64 under any undistort.  Anything
                                              else: MBAVO_E_ARG */
            };
        };
    };
} mbavo_pairs_opts;
int mbavo_pairs_create(mbavo_ctx *ctx, const mbavo_pairs_opts *opts, mbavo_pairs **out);
int mbavo_pairs_destroy(mbavo_pairs *pairs);
int mbavo_pairs_opts_size(void);           /* sizeof(mbavo_pairs_opts) of the loaded library, for a binding's mirror */
/* Pure host: validates the options exactly as mbavo_pairs_create does (MBAVO_E_ARG; mbavo_detect_semidense's MBAVO_E_RANGE, an
 * image larger than the grid of the H0 x W0 it is given, cannot occur: level l is always (H >> l) x (W >> l)) and reports the device bytes create would allocate and the keypoint capacity (= grid cells; with
 * every_candidate = 1: H_l * W_l, and no pick array is allocated) of every level (0 for levels >= L).  Needs no device. */
int mbavo_pairs_plan(const mbavo_pairs_opts *opts, long long *h_device_bytes, int h_cells_per_level[8]);
/* d_sharp, d_blur: B x H x W u8, d_depth_z: B x H x W float (z < 1e-2 = no depth), all device, contiguous, pair-major; read
 * during the call only.  The depth argument of prepare, update and track_frame keeps its C type for every depth format: with
 * opts.depth_format = 1 the floats are ray distances, with 2 it points at B x H x W (update, track_frame: n_key x H x W) uint16
 * values, passed through a cast.  Only the pixels a keypoint is looked up at are read and converted; launches, synchronisations
 * and D2H bytes are those of format 0.  On the context's stream: two copies of the level-0 images into the object, ceil((L-1)/3) pyramid
 * launches over all 2B images, ONE launch each for the gradient images, the grid selection (with depth and border test) and the
 * ordered compaction of all B x L levels (every_candidate = 1: three launches -- count, scan, write -- in place of those two),
 * one copy of the B x L keypoint counts and ONE stream synchronisation; then K of every problem is filled in.
 * h_counts_or_null: B x L ints, pair-major. */
int mbavo_pairs_prepare(mbavo_pairs *pairs, const unsigned char *d_sharp, const float *d_depth_z, const unsigned char *d_blur,
                        int *h_counts_or_null);
/* opts.undistort != 0: the camera the raw images come from.  ONE launch on the context's stream, nothing waited for: the level-0
 * undistortion map (mbavo_undistort_map with `to` = opts.intrinsics at opts.H x opts.W) into the object's own 8 H W bytes -- one
 * map for all pairs and all frames, counted by mbavo_pairs_plan.  May be called again; the camera applies to later prepares and
 * updates.  From then on ONE remap launch (mbavo_undistort_u8's device function over all images that changed, the image index in
 * blockIdx.y) takes the place of the level-0 copies: a prepare costs ceil((L-1)/3) + 4 launches (every_candidate = 1: + 5), an
 * update with keyframes what it costs with undistort = 0 (the remap in place of the copy kernel), an update with n_key == 0 and a
 * d_blur ceil((L-1)/3) + 1; synchronisations and D2H bytes do not change.  Everything below level 0 is untouched.
 * With opts.undistort = 2 a keypoint's depth is looked up through the map: (sx, sy) is the map entry at the keypoint's level-0
 * pixel (x0, y0), xr = (int)floor((double)sx + 0.5), yr likewise; a non-finite entry (or one of magnitude >= 2^30), or (xr, yr)
 * outside the Hs x Ws map: z = 0, no depth; otherwise the raw element at (xr, yr) goes through the format's formula, format 1 with
 * the ray of (x0, y0) and opts.intrinsics -- the undistorted pixel's ray is the physical ray.
 * MBAVO_E_ARG, nothing launched: opts.undistort == 0, or a camera mbavo_undistort_map rejects.  prepare, update and track_frame
 * called before the first set_camera on an object with opts.undistort != 0 return MBAVO_E_ARG with nothing launched. */
int mbavo_pairs_set_camera(mbavo_pairs *pairs, const mbavo_camera_radtan *from);
/* The same call for a unified raw camera: fills the object's one level-0 map with mbavo_undistort_map_unified, ONE launch, nothing
 * waited for; needs opts.undistort != 0; may be called again and may alternate with mbavo_pairs_set_camera on one object -- the
 * last call decides the map of later prepares and updates.  Nothing else changes: prepare, update, track_frame and the
 * undistort = 2 depth look-up read map entries, and their launches, synchronisations and D2H bytes are those stated above.
 * MBAVO_E_ARG, nothing launched: opts.undistort == 0, or a camera mbavo_undistort_map_unified rejects. */
int mbavo_pairs_set_camera_unified(mbavo_pairs *pairs, const mbavo_camera_unified *from);
/* ---- a SET of cameras in one batch (opts.num_cameras = G in 1 .. B): the cameras of a rig, several sequences or datasets, every
 * pair looking through one of them.  Camera g is a raw camera of either model and the undistorted pinhole camera `to_intrinsics` of
 * its pairs; the object holds G level-0 maps (8 H W G bytes, counted by mbavo_pairs_plan in place of the one map; map g starts at
 * byte 8 H W g, so with an odd H W every other map is 8-byte aligned only and the remap stores those images byte by byte) and a
 * pair -> camera index.  G = B is one camera per pair; pairs that share a camera share its map.  With opts.undistort = 0 no map is
 * held or made: the images are pinhole images of their pairs' `to_intrinsics` (the entries are validated all the same).
 * mbavo_pairs_set_cameras: ONE host-to-device copy of the G cameras and the B indices and, with opts.undistort != 0, ONE launch
 * that fills all G maps (mbavo_undistort_map_batch's kernel) on the context's stream; nothing is waited for (the copy leaves from a
 * pinned mirror; a second call waits, if at all, only until the first call's copy has left that mirror).  `intrinsics` of every
 * entry of mbavo_pairs_problems become the pair's to_intrinsics / (1 << l) at the call.  May be called again; like set_camera the
 * cameras apply to later prepares, updates and track_frames: level-0 images, the format-1 depth conversion, the undistort = 2
 * look-up and the keyframe test (mbavo_pairs_assess, _commit) use the pair's camera.  Launches, synchronisations and D2H bytes of
 * prepare, update, predict, commit and track_frame are those of an object with one camera.
 * Limitation: a pair whose camera changes must be listed with a new keyframe in the next update -- its level-0 keyframe was
 * remapped, and its format-1 depths were converted, with the old camera's map and ray.
 * MBAVO_E_ARG, nothing copied, launched or changed (the cameras before the call stay in force): opts.num_cameras == 0; G !=
 * opts.num_cameras; a NULL pointer; an index outside 0 .. G-1; a model other than 1 or 2; a camera mbavo_undistort_map (model 1) or
 * mbavo_undistort_map_unified (model 2) rejects for this object's H x W; raw sizes that differ between cameras; fx or fy of a
 * to_intrinsics equal to 0.  On an object with opts.num_cameras > 0 mbavo_pairs_set_camera and _set_camera_unified return
 * MBAVO_E_ARG, and prepare, update and track_frame before the first set_cameras return MBAVO_E_ARG with nothing launched (with
 * opts.undistort = 0 as well: the per-pair intrinsics are not there yet). */
typedef struct mbavo_pairs_camera {        /* one camera of a batch; 120 bytes, no padding */
    int model;                             /* 1: CameraPinhole + DistortionRadTan (xi not read)  2: CameraUnified (+ optional DistortionRadTan) */
    int reserved;
    int H, W;                              /* raw image size: the same for every camera of a batch (the raw images are one B x Hs x Ws array) */
    double intrinsics[4], xi, dist[4];     /* as mbavo_camera_radtan / mbavo_camera_unified */
    double to_intrinsics[4];               /* the pinhole camera of this camera's pairs at level 0 */
} mbavo_pairs_camera;
int mbavo_pairs_camera_size(void);         /* sizeof(mbavo_pairs_camera) of the loaded library */
int mbavo_pairs_set_cameras(mbavo_pairs *pairs, int G, const mbavo_pairs_camera *h_cams /* G */, const int *h_camera_of_pair /* B */);
/* The maps of n cameras in ONE launch on the context's stream (the camera index in blockIdx.y; the cameras travel in ONE
 * host-to-device copy into the context's scratch; the copy leaves from pageable memory, so the call returns once it is staged,
 * which the runtime may delay behind work already queued on the stream, and an n larger than any before regrows the scratch, which
 * synchronises the device once), the launch itself is not waited for: map i, at d_maps + 2 H W i floats, is the H x W map of
 * h_cams[i].to_intrinsics into raw camera i and has the bits mbavo_undistort_map (model 1) or mbavo_undistort_map_unified (model 2)
 * writes for that camera -- the same device function per entry.  No alignment beyond the floats' is assumed.
 * MBAVO_E_ARG, nothing launched: a NULL pointer; n < 1 or n > 65535; a model other than 1 or 2; a camera, or an H x W, the single
 * call of its model rejects. */
int mbavo_undistort_map_batch(mbavo_ctx *ctx, int n, const mbavo_pairs_camera *h_cams /* n */, int H, int W,
                              float *d_maps /* n x H x W x 2 */);
/* ---- the CLEARANCE MASK: keypoints off the black margin of undistorted images.  mbavo_undistort_u8 writes 0 wherever a map
 * entry leaves the raw image, so the undistorted image of a wide lens has a black margin with a curved outline -- the strongest
 * edge of the image, which the semi-dense detector selects and which stays where it is whatever the camera does.  border[] cuts a
 * rectangle; the clearance mask is a border of arbitrary shape, derived on the device from the undistortion map(s).  Everything
 * here is integer or comparison logic: every result is exact.
 *   Valid at level 0.  Take the map entry (sx, sy) of output pixel (c, r), X = (double)sx, Y = (double)sy.  Pixel (c, r) is valid
 *     iff 0.0 <= X && X <= (double)(Ws - 1) && 0.0 <= Y && Y <= (double)(Hs - 1).  NaN and +-inf fail the comparisons, -0.0 passes.
 *     That is exactly the set of entries for which no tap of the remap with a non-zero weight lies outside the Hs x Ws raw image.
 *   Valid at level l.  Level l is (H >> l) x (W >> l).  Pixel (x, y) of level l is valid iff all 4^l level-0 pixels
 *     (x 2^l + i, y 2^l + j), 0 <= i, j < 2^l, are valid: the 2 x 2 box pyramid mixes exactly these.  Level-0 rows and columns
 *     beyond (H >> l) << l belong to no box.
 *   Clear at radius r.  Pixel (x, y) of level l is clear iff every (x', y') with |x' - x| <= r and |y' - y| <= r lies inside the
 *     level and is valid.  So "clear" implies a rectangular border of r.  r counts pixels of the level itself, the same at every
 *     level, as a patch pattern does.
 *   Use (opts.valid_radius = r > 0).  A keypoint (x, y) of level l is kept only if it is clear.  The test sits exactly where the
 *     border[] test sits and is combined with it by AND: in grid selection on the cell's pick (a cell whose pick fails gets no
 *     keypoint, as with border[]), with every_candidate = 1 on every candidate.  Order, depths and everything else stay as they are.
 * The object holds one clearance pyramid per map (one with num_cameras = 0, G with a camera set): one byte per pixel of every
 * level, level after level, each level starting on a 256-byte boundary; mbavo_pairs_plan counts these bytes.
 * mbavo_pairs_set_camera, _set_camera_unified and _set_cameras fill the pyramids right behind the map launch, on the same stream,
 * nothing waited for, in 3 launches (L > 4: 4) whatever G, B and r are: the valid bytes of levels 0 .. 3 from the map(s), those of
 * levels 4 .. L-1 from level 3, then the box AND as a row pass and a column pass over all levels of all maps.  A repeated camera
 * call rebuilds them.  (The row pass writes into scratch of the context that the object reserves at creation.)  prepare, update and
 * track_frame apply the test through the pair's camera -- one byte load per pick or per candidate; their launches,
 * synchronisations and D2H bytes are those of valid_radius = 0, and an update still equals a fresh prepare bit for bit.
 * Not covered: warps that land in the CURRENT frame's black margin (the evaluation kernels' validity rule, Huber and the outlier
 * test deal with those).
 *
 * mbavo_undistort_clearance_batch: the same kernels for n maps the caller holds (mbavo_undistort_map*), for callers of
 * mbavo_detect_semidense / mbavo_vo_*: d_clear receives, map after map, the levels 0 .. L-1 one behind the other without padding
 * (mbavo_undistort_clearance_bytes(H, W, L) = sum over l of (H >> l) (W >> l) bytes per map).  radius = 0 is allowed and gives the
 * plain valid pyramid (two launches fewer).  On the context's stream, nothing waited for; with radius > 0 an n * bytes larger than
 * any before regrows the context's scratch, which synchronises the device once.
 * MBAVO_E_ARG, nothing launched: a NULL pointer; n < 1 or n > 65535; L outside 1 .. 8; (H >> (L-1)) < 1, the same for W; H, W, Hs or
 * Ws < 1; H * W or Hs * Ws above 2^22; radius outside 0 .. 64.  mbavo_undistort_clearance_bytes (pure host) returns a negative
 * value for the H, W, L the batch entry rejects. */
int mbavo_undistort_clearance_batch(mbavo_ctx *ctx, int n, const float *d_maps /* n x H x W x 2 */, int H, int W,
                                    int Hs, int Ws, int L, int radius, unsigned char *d_clear /* n x sum_l (H>>l)(W>>l), no padding */);
long long mbavo_undistort_clearance_bytes(int H, int W, int L);   /* per map; pure host */
/* ---- CALLER-SUPPLIED MASKS beside the clearance mask: a vehicle bonnet, a lens hood, a rig strut, a timestamp overlay -- strong
 * edges that never move with the camera, which the semi-dense detector picks and whose residuals say "you are standing still";
 * or, one mask per pair, a segmentation of moving objects per keyframe.  border[] cuts a rectangle, the clearance mask knows the
 * undistortion map only, and a pinhole object (undistort = 0) has no map.  Integer and comparison logic: every byte is exact.
 *   Mask bytes.  A mask is a u8 image; a byte != 0 means "usable", 0 means "masked out".
 *   Warp of a raw-geometry mask.  Take a raw mask R (Hs x Ws) and the map entry (sx, sy) of an output pixel; in double, as the
 *     remap does: X = (double)sx, Y = (double)sy, x0 = (int)floor(X), y0 = (int)floor(Y), ax = X - floor(X), ay = Y - floor(Y).
 *     The warped byte is 1 iff the entry is valid by the level-0 rule above and R is non-zero at every tap that carries weight:
 *     (x0, y0) always; (x0 + 1, y0) iff ax > 0; (x0, y0 + 1) iff ay > 0; (x0 + 1, y0 + 1) iff ax > 0 and ay > 0.  Otherwise 0.
 *     For a valid entry all these taps lie inside the raw image (X <= Ws - 1 with ax > 0 gives x0 + 1 <= Ws - 1); a tap of weight
 *     0 is never read, so an entry on a whole coordinate next to a masked raw pixel stays usable.
 *   Valid at level 0 with a mask.  Pixel (c, r) is valid iff the map term holds -- the rule above where there is a map, true
 *     where there is none (undistort = 0, or a NULL map argument) -- and M[r][c] != 0, M the H x W mask in the undistorted
 *     geometry.  "Valid at level l", "clear at radius r" and the use on keypoints are word for word the ones above; with r = 0,
 *     "clear" is "valid".
 * mbavo_undistort_mask_batch: the warp for n raw masks, mask i through map i, in ONE launch on the context's stream, nothing
 * waited for (the index in blockIdx.y; a lane makes four adjacent bytes from two 16-byte map loads and at most sixteen taps and
 * stores one word where map and destination are aligned, bytes otherwise).  MBAVO_E_ARG, nothing launched: what
 * mbavo_undistort_u8_batch rejects -- a NULL pointer; n < 1 or n > 65535; H, W, Hs or Ws < 1; H * W or Hs * Ws above 2^22.
 * mbavo_mask_clearance_batch: mbavo_undistort_clearance_batch with the level-0 rule "with a mask": the same packed output, the
 * same launches (radius 0: two fewer), the same scratch.  d_masks_or_null == NULL: the bytes of mbavo_undistort_clearance_batch.
 * d_maps_or_null == NULL: the mask alone, Hs and Ws are not read.  Both NULL: MBAVO_E_ARG, as for everything that entry rejects. */
int mbavo_undistort_mask_batch(mbavo_ctx *ctx, int n, const unsigned char *d_raw_masks /* n x Hs x Ws */, int Hs, int Ws,
                               const float *d_maps /* n x H x W x 2 */, int H, int W, unsigned char *d_masks_out /* n x H x W */);
int mbavo_mask_clearance_batch(mbavo_ctx *ctx, int n, const float *d_maps_or_null /* n x H x W x 2 */,
                               const unsigned char *d_masks_or_null /* n x H x W */, int H, int W, int Hs, int Ws, int L, int radius,
                               unsigned char *d_clear /* n x sum_l (H>>l)(W>>l), no padding */);
/* An object with opts.mask = 1 holds, with G' = max(num_cameras, 1), both counted by mbavo_pairs_plan: G' stored level-0 masks in
 * the undistorted geometry (H W bytes each, rounded up to 256), filled with ones at creation, and G' clearance pyramids -- also
 * with valid_radius = 0, where "clear" is "valid".  With undistort = 0 creation builds the pyramids (the rectangular border r
 * until a mask is set); otherwise the camera calls do.
 * mbavo_pairs_set_masks: the G' masks (n must be G'; device memory, read during the call only).  geometry 0: n x H x W in the
 * undistorted geometry, copied into the object.  geometry 1: n x Hs x Ws in the raw geometry, warped into the stored masks
 * through the object's own maps in one launch of mbavo_undistort_mask_batch's kernel; needs undistort != 0 and a camera call
 * before it.  Then the pyramids are rebuilt from map and stored mask by the clearance launches (3, or 4 with L > 4; 1 / 2 with
 * radius 0).  On the context's stream, nothing waited for, nothing allocated; may be repeated.
 * mbavo_pairs_set_camera, _set_camera_unified and _set_cameras on such an object rebuild the pyramids from the new map AND the
 * stored mask, in the launches stated above; the stored mask itself is left alone.  So after a camera change a caller whose masks
 * came in the raw geometry calls mbavo_pairs_set_masks again: the stored masks are still the warp through the old maps.
 * The test sits where keypoints are selected: a changed mask reaches a pair with its next keyframe -- a prepare, or an update that
 * lists it; the keypoints of pairs not listed stay -- the rule a changed camera follows.  Launches, synchronisations and D2H bytes
 * of prepare, update, predict, commit and track_frame are those of the same object with mask = 0 (undistort = 0: with
 * valid_radius = 0).  Out of scope: a mask for mbavo_detect_semidense / mbavo_vo_* (filter with the stand-alone pyramid), a
 * set_masks for a subset of the cameras, masks for the current frame.
 * MBAVO_E_ARG, nothing launched or changed: opts.mask == 0; n != G'; a NULL pointer; a geometry other than 0 or 1; geometry 1 with
 * opts.undistort == 0 or before the first camera call. */
int mbavo_pairs_set_masks(mbavo_pairs *pairs, int geometry, int n, const unsigned char *d_masks);
/* Per pair: capture / exposure time of the blurred frame, spline start time t0 (dt shared), N knots (translations B x 3N, unit
 * quaternions xyzw B x 4N); uploaded in one copy (the B start times in a second one, for mbavo_pairs_assess).  Every pair's start index is that of its capture time
 * (mbavo_segment_start_index).  MBAVO_E_RANGE, with the previous motion left in place, if a blur sample of any level of any pair
 * falls outside its knots. */
int mbavo_pairs_set_motion(mbavo_pairs *pairs, const double *h_cap, const double *h_exp, const double *h_t0, double dt,
                           const double *h_knots_t /*B x 3N*/, const double *h_knots_R /*B x 4N*/);
int mbavo_pairs_get_knots(mbavo_pairs *pairs, double *h_knots_t, double *h_knots_R); /* e.g. after an LM call; synchronises */
/* library-owned B x L array, pair-major, valid until mbavo_pairs_destroy (K: until the next prepare): what mbavo_lm_batch_levels
 * takes as is (or, with L = 1 or one level picked out, mbavo_lm_batch / mbavo_eval_batch).  *h_count = B * L. */
int mbavo_pairs_problems(mbavo_pairs *pairs, const mbavo_problem **h_out, int *h_count);
/* read-only witness, in the spirit of mbavo_last_layout: out[0] kernel launches, out[1] stream synchronisations and out[2]
 * device-to-host bytes of the last prepare (0 before the first), out[3] device bytes the object holds (under
 * mbavo_pairs_set_detector's score = 1: one launch more, the score launch; the other three as they were) */
int mbavo_pairs_last_stats(mbavo_pairs *pairs, long long out[4]);

/* ---- a batch of pairs from frame to frame.  One frame of B trackers (trackFrame, blur_aware_direct_tracker.cpp:88-203) is
 *   mbavo_pairs_update      the B new blurred frames; new keyframes for the pairs whose last verdict was "keyframe"
 *   mbavo_pairs_predict     capture / exposure times, start times; the constant-velocity prediction of every pair's knots, on the device
 *   mbavo_lm_batch_levels   the alignment, on the array of mbavo_pairs_problems
 *   mbavo_pairs_commit      every pair's keyframe verdict, the velocity update, the re-expression of a new keyframe's spline, the
 *                           pose in the world
 * -- or all four in one call, mbavo_pairs_track_frame: a constant number of launches per frame and no pose algebra on the host.
 * The B tracker states (mbavo_vo_state: what mbavo_vo_get_state returns) live on the device from mbavo_pairs_set_states on; the
 * first frame of a tracker is mbavo_pairs_prepare plus the state trackFrame leaves after it (two identity knots at the first
 * capture time, identity poses, zero velocity).  What stays with the caller is the choice of images: the pairs to list in the next
 * update are those whose verdict was 1.  The device LM and the host LM agree on records, not on bits, so a batch follows B
 * mbavo_vo trackers within the LM's tolerances, not bit for bit.
 * The pieces stay available on their own: mbavo_pairs_set_motion uploads knots made on the host, mbavo_pairs_assess runs the
 * keyframe test without touching any state. */
typedef struct mbavo_pairs_assessment {    /* one per pair; 88 bytes, no padding */
    int is_keyframe;                       /* isKeyframe's verdict (blur_aware_direct_tracker.cpp:205-262) under the thresholds given */
    int status;                            /* 0, or MBAVO_E_RANGE: one of the three times lies outside the pair's knots (GetPose
                                              fails: is_keyframe 0 as on the host, NaN in every double below) */
    int num_keypoints0;                    /* level-0 K the sums ran over */
    int num_behind;                        /* projections (keypoint x the three poses) with Pc.z < 0: they stay (0,0) in the sums */
    double avg_flow, avg_kernel;           /* float values, as the host forms them: sqrtf((float)(sum / K)); NaN for K = 0 */
    double T[7];                           /* spline pose at the capture time as GetPose returns it: t[3], q xyzw */
} mbavo_pairs_assessment;
int mbavo_pairs_assessment_size(void);     /* sizeof(mbavo_pairs_assessment) of the loaded library */
/* The keyframe test and the frame pose of all B pairs: ONE launch (a workgroup per pair), one device-to-host copy of
 * B * sizeof(mbavo_pairs_assessment) and one stream synchronisation, whatever B is.  Reads, on the device, the pair's knots as
 * they are now (after an LM call or mbavo_pairs_set_motion), the capture / exposure time, t0 and dt of the last set_motion and
 * the level-0 keypoints and intrinsics of the last prepare / update.  The sums are reduced in a fixed order: the same bits from
 * run to run and for any B.  MBAVO_E_ARG, nothing launched, before the first prepare or the first set_motion. */
int mbavo_pairs_assess(mbavo_pairs *pairs, double flow_mag0, double flow_mag1, double max_blur_kernel_mag,
                       mbavo_pairs_assessment *h_out /* B */);
int mbavo_pairs_assess_stats(mbavo_pairs *pairs, long long out[3]); /* launches, synchronisations, D2H bytes of the last assess */
/* New current frames for all pairs (d_blur: B x H x W, or NULL: they stay) and new keyframes for the n_key pairs listed in
 * h_key_pairs (strictly ascending, 0 <= n_key <= B; d_sharp, d_depth_z: n_key x H x W in the order of the list, NULL iff
 * n_key == 0).  Afterwards every array of the object and every K are, bit for bit, what mbavo_pairs_prepare writes when given
 * every pair's most recent keyframe, depth map and blurred frame; the keyframe side of a pair not listed is not written, knots
 * and motion are untouched.  Launches: one copy kernel for the new keyframes' level 0, ceil((L-1)/3) pyramid launches over the
 * images that changed, one launch each for gradients, grid selection and compaction (every_candidate = 1: count, scan and
 * write) over the listed pairs, one copy of the
 * counts, ONE synchronisation -- whatever B and n_key are (n_key == 0: no keyframe launch and no count copy).
 * h_counts_or_null: B x L, all pairs.  MBAVO_E_ARG, nothing launched: before the first prepare, indices out of range or not
 * ascending, a NULL image with n_key > 0. */
int mbavo_pairs_update(mbavo_pairs *pairs, const unsigned char *d_blur, int n_key, const int *h_key_pairs,
                       const unsigned char *d_sharp, const float *d_depth_z, int *h_counts_or_null);
/* launches, synchronisations, D2H bytes of the last update (under mbavo_pairs_set_detector's score = 1: one launch more where
 * n_key > 0, none more where n_key == 0; synchronisations and bytes as they were) */
int mbavo_pairs_update_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- tracker state of the B pairs on the device (trackFrame's pose bookkeeping, blur_aware_direct_tracker.cpp:119-141, 143-203).
 * Pair b's state is an mbavo_vo_state: a batch is seeded from, and checkpointed to, mbavo_vo trackers.
 * set_states: ONE host-to-device copy (pinned staging) of every pair's knots -- into the buffers the problems' d_knots_t / d_knots_R
 * point at --, t0, T_keyframe, T_prev_b2w, velocity and prev_timestamp; dt becomes the dt of every problem.  MBAVO_E_ARG, nothing
 * changed: N != opts.N, is_first != 0 (the first frame is mbavo_pairs_prepare's job), dt <= 0 or not the same for all pairs.  A
 * pending predict (below) is dropped.
 * get_states: ONE device-to-host copy and one synchronisation; a set followed by a get returns the same bits (knot entries from N
 * on are returned as zero, as mbavo_vo_get_state leaves them). */
struct mbavo_vo_state;                     /* defined with the tracker, below */
int mbavo_pairs_set_states(mbavo_pairs *pairs, const struct mbavo_vo_state *h_states /* B */);
int mbavo_pairs_get_states(mbavo_pairs *pairs, struct mbavo_vo_state *h_states /* B */);
/* trackFrame :119-141 for all pairs.  Host: t0_b = cap_b - 0.5 * exp_b, every pair's start index and the knot-range check of every
 * level's blur samples (MBAVO_E_RANGE, nothing changed), ONE copy of [cap | exp | t0], t0 / dt / h_start_idx of the problems.
 * Device: ONE launch, no synchronisation -- per pair dt_frame = cap - prev_timestamp, dT = exp(velocity * dt_frame), every knot
 * t_i += R_i * dT.t, R_i = R_i * dT.q (a pair's knots on consecutive lanes, dT computed once per pair), and the new times take the
 * place of the last set_motion's.  The stored velocity is not scaled; dt_frame stays on the device for the commit.  MBAVO_E_ARG:
 * before the first prepare, before the first set_states, or while a predict is pending (two predicts without a commit). */
int mbavo_pairs_predict(mbavo_pairs *pairs, const double *h_cap /* B */, const double *h_exp /* B */);
/* ---- THE START OF EVERY PAIR PICKED AMONG M MOTION HYPOTHESES.  mbavo_pairs_predict starts the LM from the constant-velocity
 * extrapolation alone; a camera that stops, reverses or doubles its speed between two frames puts that start outside the coarsest
 * level's basin.  mbavo_pairs_predict_hypotheses takes predict's place in the four- or five-call frame: it forms M candidate
 * starts per pair, evaluates all B * M of them cost-only at one pyramid level and leaves every pair on its cheapest.
 * mbavo_pairs_track_frame and its _points twin stay as they are.
 *   Hypotheses.  All arithmetic is IEEE double without contraction.  With the pair's stored velocity and dt_frame = cap -
 *     prev_timestamp: hypothesis 0 is mbavo_pairs_predict's own, tangent_0[j] = velocity[j] * dt_frame (the very expression of the
 *     predict kernel); hypothesis m >= 1 has tangent_m[j] = (scale[m] * velocity[j]) * dt_frame + twist[m][j] (order (v, w), as
 *     mbavo_se3_exp).  dT_m = exp(tangent_m), the device function predict uses.  Candidate knots of pair b: t_i + R_i * dT_m.t and
 *     R_i * dT_m.q for i < N (SplineSE3::TransformByRight), from the knots as they are before the call.
 *   Evaluation.  ONE mbavo_eval_batch(with_hessian = 0) over B * M entries through the object's own engine: entry (b, m), at b * M + m,
 *     is a copy of pair b's level-`level` entry of mbavo_pairs_problems whose d_knots_t / d_knots_R point at candidate (b, m) in
 *     scratch, with d_outlier = NULL, num_bad = 0 and num_residuals = 0; the times, t0 and start index are those the call publishes.
 *     Of its outputs the frame block's cost slot and d_valid are read.
 *   Score.  K = the pair's keypoint count at `level`, P = opts.P[level] of the object, KP = (double)K * (double)P; score_m =
 *     (cost_m * KP) / valid_m, the mean Huber cost per IN-BOUNDS pixel -- an out-of-bounds pixel contributes residual 0, so a
 *     hypothesis that throws the scene out of the image has cost 0.  Hypothesis m is eligible iff K > 0, valid_m >=
 *     min_valid_frac * KP and score_m is finite.
 *   Winner.  c = the eligible m >= 1 of smallest score, ties to the lowest m.  winner = c iff c exists and (hypothesis 0 is
 *     ineligible or score_c < score_0 * (1.0 - min_gain)); otherwise winner = 0.  No hypothesis eligible: winner = 0 and status =
 *     MBAVO_HYP_NONE_ELIGIBLE.  num_eligible counts the eligible hypotheses, hypothesis 0 included.
 *   State after the call: exactly that of mbavo_pairs_predict(h_cap, h_exp), except that the pair's knots are candidate `winner`'s.
 *     The times, t0, start indices and dt_frame are as predict leaves them, the stored velocity is untouched, a predict is pending
 *     (mbavo_pairs_commit consumes it).  With M = 1 every knot, every state word and every problem time has the bits
 *     mbavo_pairs_predict leaves.
 *   Cost.  One host-to-device copy of the times (as predict), one of the options, ONE launch that writes the B * M candidates and
 *     publishes the times (a workgroup per pair, a lane per (hypothesis, knot)), the evaluation, ONE launch that scores, selects,
 *     copies the winner's knots and writes the records (16 lanes per pair, no atomics: the same bits from run to run).  With
 *     h_out_or_null == NULL nothing is waited for, as in predict; else one copy of B records through a pinned mirror and ONE
 *     synchronisation.  mbavo_pairs_hyp_stats witnesses it: launches (2 + the evaluation's, counted by the rule of
 *     mbavo_pairs_report_stats), synchronisations and D2H bytes of the last call.
 *   Scratch: candidates, blocks, valid counts, records and the options, sized for 16 hypotheses, in one device allocation that the
 *     object makes at its FIRST call (with a pinned mirror of records and options) and keeps; the B * M entry array is host memory
 *     of the object.  mbavo_pairs_plan and mbavo_pairs_last_stats do not count it, as with the report's scratch.
 *   MBAVO_E_ARG, nothing launched or changed: whatever mbavo_pairs_predict rejects; NULL opts; M outside 1 .. 16; level outside
 *     0 .. L-1; min_valid_frac outside [0, 1] or not finite; min_gain outside [0, 1) or not finite; a non-finite scale or twist
 *     entry among 1 .. M-1.  MBAVO_E_RANGE as predict, from the host's check of the times (the same for every hypothesis).  An
 *     error returned by the evaluation itself is passed on and leaves no predict pending: mbavo_pairs_set_states starts over. */
#define MBAVO_PAIRS_MAX_HYP 16
#define MBAVO_HYP_NONE_ELIGIBLE 1
typedef struct mbavo_pairs_hyp_opts {      /* zero-initialise */
    int M;                                 /* 1 .. 16 hypotheses, hypothesis 0 included */
    int level;                             /* pyramid level the costs are taken at, 0 .. L-1 (the caller's choice; L-1 is the usual one) */
    double min_valid_frac;                 /* 0: 0.5; else in (0, 1] */
    double min_gain;                       /* in [0, 1): a challenger must beat hypothesis 0 by this share; 0 = any improvement */
    double scale[16];                      /* s_m for m = 1 .. M-1; entry 0 is not read */
    double twist[16][6];                   /* (v, w) added to the scaled tangent, m = 1 .. M-1; entry 0 is not read */
    int reserved[4];
} mbavo_pairs_hyp_opts;
typedef struct mbavo_pairs_hyp {           /* one per pair; 272 bytes, no padding */
    int winner, status, num_keypoints, num_eligible;
    double score[16], valid[16];           /* entries >= M: 0 */
} mbavo_pairs_hyp;
int mbavo_pairs_hyp_opts_size(void);       /* sizeof(mbavo_pairs_hyp_opts) of the loaded library */
int mbavo_pairs_hyp_size(void);            /* sizeof(mbavo_pairs_hyp) of the loaded library */
int mbavo_pairs_predict_hypotheses(mbavo_pairs *pairs, const double *h_cap /* B */, const double *h_exp /* B */,
                                   const mbavo_pairs_hyp_opts *opts, mbavo_pairs_hyp *h_out_or_null /* B */);
int mbavo_pairs_hyp_stats(mbavo_pairs *pairs, long long out[3]);   /* launches, synchronisations, D2H bytes of the last call */
typedef struct mbavo_pairs_frame {         /* one per pair; 144 bytes, no padding */
    mbavo_pairs_assessment a;              /* exactly what mbavo_pairs_assess returns at that moment */
    double T_world[7];                     /* T_keyframe * pose at the capture time, after the state update: trackFrame's output */
} mbavo_pairs_frame;
int mbavo_pairs_frame_size(void);          /* sizeof(mbavo_pairs_frame) of the loaded library */
/* trackFrame :143-203 after the alignment: ONE launch (a workgroup per pair), one device-to-host copy of
 * B * sizeof(mbavo_pairs_frame) and one synchronisation.  Per pair: the assessment; velocity = log(T_prev^-1 * T) / dt_frame;
 * T_prev = T; if a.is_keyframe: T_keyframe = T_keyframe * T, the knots through TransformTo(cap, identity) in place, T_prev =
 * identity; prev_timestamp = cap; T_world = T_keyframe * GetPose(cap) on the knots as they now are.  A pair with one of its three
 * times outside its knots: a.status = MBAVO_E_RANGE, NaN in every double, its state left as the predict made it, the other pairs
 * commit.  MBAVO_E_ARG unless a predict is pending. */
int mbavo_pairs_commit(mbavo_pairs *pairs, double flow_mag0, double flow_mag1, double max_blur_kernel_mag,
                       mbavo_pairs_frame *h_out /* B */);
/* out[0..2]: launches, synchronisations, D2H bytes of the last predict; out[3..5]: of the last commit (neither detects: the score
 * launch of mbavo_pairs_set_detector inside a track_frame is its update's, in mbavo_pairs_update_stats) */
int mbavo_pairs_track_stats(mbavo_pairs *pairs, long long out[6]);
/* One frame of all B trackers: mbavo_pairs_update(d_blur, n_key, h_key_pairs, d_sharp, d_depth_z, h_counts_or_null), predict(h_cap,
 * h_exp), mbavo_lm_batch_levels on the object's own array (opts, h_results_or_null, h_trace_or_null, trace_cap), commit(the three
 * thresholds, h_out) -- pure host composition.  The first error is returned and nothing later is launched; an error after the
 * predict leaves it pending (mbavo_pairs_set_states starts over).  NULL h_cap, h_exp, opts or h_out: MBAVO_E_ARG, nothing launched. */
int mbavo_pairs_track_frame(mbavo_pairs *pairs, const unsigned char *d_blur, int n_key, const int *h_key_pairs,
                            const unsigned char *d_sharp, const float *d_depth_z, const double *h_cap, const double *h_exp,
                            const mbavo_lm_batch_opts *opts, mbavo_lm_batch_result *h_results_or_null,
                            mbavo_trace_rec *h_trace_or_null, int trace_cap, double flow_mag0, double flow_mag1,
                            double max_blur_kernel_mag, mbavo_pairs_frame *h_out /* B */, int *h_counts_or_null);

/* ---- KEYPOINTS AND DEPTHS FROM THE CALLER, not from a depth map: sparse map points of a back end, LiDAR returns projected into
 * the keyframe, a few hundred stereo depths, pixels a mapper has already chosen.  The reference tracker reads nothing but
 * num_keypoints, tmp_keypoints_xy and tmp_keypoints_z of its options (blur_aware_direct_tracker.h:17-19, .cpp:735-742);
 * tmpProcessKeyframe is one way of filling them, these calls are another.  They work on any pairs object, whatever its options:
 * per pair the caller hands over a list of LEVEL-0 points with depths, and ONE launch, whatever B is, makes every level's keypoint
 * arrays from them.  Pyramids, gradient images, the raw-camera remap, the masks, update, the keyframe test and the tracker state
 * are those of the detector calls; mbavo_pairs_problems, mbavo_lm_batch_levels, assess, predict and commit run unchanged.
 *   Lists.  h_offsets is a HOST array of rows + 1 ints, non-decreasing, h_offsets[0] == 0; row i's points are entries
 *     h_offsets[i] .. h_offsets[i+1] - 1 of d_xy (interleaved [x0, y0] doubles) and d_z (doubles).  A row is a pair in
 *     prepare_points (rows = B) and the i-th listed pair in update_points (rows = n_key).  d_xy and d_z are device memory, 8-byte
 *     aligned, read during the call only.  Coordinates are level-0 pixel coordinates of the object's undistorted H x W geometry
 *     (with opts.undistort != 0 the IMAGES are raw and are remapped exactly as in mbavo_pairs_prepare; the points are raw only
 *     after mbavo_pairs_set_points_geometry(pairs, 1), below); z is the depth along the optical axis.
 *   Level-l position.  For a point (x0, y0, z) and level l: xl = x0 / (double)(1 << l), yl = y0 / (double)(1 << l).  The point is
 *     unusable at that level unless fabs(xl) < 2^30 && fabs(yl) < 2^30 (NaN and +-inf fail).  Its pixel is xi = (int)floor(xl + 0.5),
 *     yi likewise: the inverse of the level-0 position (int)(x * scale + 0.5) at which a detected level-l keypoint's depth is looked up.
 *   Kept at level l iff the point is usable; !(z < 1e-2) in double and z is finite (NaN and +-inf are dropped); xi >= m && xi < W_l - m
 *     && yi >= m && yi < H_l - m with m = border[l] (m = 0: the in-image test); and, where the object has a clearance pyramid
 *     (valid_radius > 0 or mask = 1), pixel (xi, yi) of level l is clear for the pair's camera -- the byte load of a pick, combined by AND.
 *   Stored: the keypoint ((double)xi, (double)yi) with depth z, the caller's double unchanged.  Keypoints are whole pixels of their
 *     level, as the detector's are (the evaluation kernels are held to the oracle at whole-pixel keypoints only).
 *   Order: the kept points of a (pair, level) appear in the order of the caller's list (a stable compaction).  Points that land on
 *     the same pixel of a coarse level are ALL kept: nothing is de-duplicated.
 *   Not read: score_threshold, cell_*, every_candidate and the depth options.  The keypoint capacity of a level is what
 *     mbavo_pairs_plan reports in h_cells_per_level (grid cells, or H_l * W_l with every_candidate = 1); a row longer than the
 *     smallest capacity over levels 0 .. L-1 makes the call return MBAVO_E_RANGE with nothing launched or changed -- a host check on
 *     h_offsets alone.  A caller with long lists creates the object with every_candidate = 1 or with small cells.
 *   Out of scope: sub-pixel keypoints, de-duplication.
 * mbavo_pairs_prepare_points costs what mbavo_pairs_prepare costs up to the gradients -- the two level-0 copies or the one remap
 * launch, ceil((L-1)/3) pyramid launches, ONE gradient launch -- then ONE points launch (a workgroup per (pair, level), no atomics:
 * the same bits from run to run) in place of detect + compact or count + scan + write, one copy of the B x L counts and ONE
 * synchronisation: ceil((L-1)/3) + 2 launches (undistort != 0: + 3), witnessed by mbavo_pairs_last_stats.  The offsets travel in
 * one host-to-device copy into scratch of the context that the object reserves at creation: the byte count of mbavo_pairs_plan
 * does not change and a call allocates nothing.
 * mbavo_pairs_update_points is mbavo_pairs_update with row i's list in place of row i's depth map, one launch fewer for the
 * keypoints (every_candidate = 1: two fewer), witnessed by mbavo_pairs_update_stats.  Afterwards every array and every K are, bit
 * for bit, what prepare_points writes when given every pair's most recent keyframe, list and blurred frame; the keyframe side of a
 * pair not listed is not written.  n_key == 0 is exactly mbavo_pairs_update(d_blur, 0, ..): the point arguments are not read.
 * Keypoints are per-pair storage, so detector and point calls may alternate on one object, pair by pair and frame by frame.
 * mbavo_pairs_track_frame_points is mbavo_pairs_track_frame with update_points as its first call -- pure host composition, the
 * same error rules.
 * MBAVO_E_ARG, nothing launched or changed: a NULL image (update_points: with n_key > 0); NULL h_offsets; NULL d_xy or d_z with a
 * non-zero total; offsets that decrease or do not start at 0; for update_points what mbavo_pairs_update rejects; on an object
 * with a raw camera or a camera set a call before the first camera call. */
int mbavo_pairs_prepare_points(mbavo_pairs *pairs, const unsigned char *d_sharp, const unsigned char *d_blur,
                               const int *h_offsets /* B + 1 */, const double *d_xy /* total x 2 */, const double *d_z /* total */,
                               int *h_counts_or_null /* B x L */);
int mbavo_pairs_update_points(mbavo_pairs *pairs, const unsigned char *d_blur, int n_key, const int *h_key_pairs,
                              const unsigned char *d_sharp, const int *h_offsets /* n_key + 1 */, const double *d_xy,
                              const double *d_z, int *h_counts_or_null /* B x L */);
int mbavo_pairs_track_frame_points(mbavo_pairs *pairs, const unsigned char *d_blur, int n_key, const int *h_key_pairs,
                                   const unsigned char *d_sharp, const int *h_offsets /* n_key + 1 */, const double *d_xy,
                                   const double *d_z, const double *h_cap, const double *h_exp, const mbavo_lm_batch_opts *opts,
                                   mbavo_lm_batch_result *h_results_or_null, mbavo_trace_rec *h_trace_or_null, int trace_cap,
                                   double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out /* B */,
                                   int *h_counts_or_null);

/* ---- THE CALLER'S POINTS IN THE RAW CAMERA'S GEOMETRY.  A caller that brings its own points (map points, LiDAR returns, stereo
 * depths) calibrated the real camera and projects into the RAW image.  On an object with opts.undistort != 0 images, masks
 * (mbavo_pairs_set_masks(geometry = 1)) and depth maps (undistort = 2) are taken raw; these two entries do the same for points.
 *   The inverse camera.  For a raw pixel (u, v) of a camera `cam` (an mbavo_pairs_camera, model 1 or 2), in double, operation by
 *   operation, nothing contracted into a fused multiply-add:
 *     Normalise.  px = (u - cx) / fx, py = (v - cy) / fy.
 *     Inverse distortion, as DistortionRadTan::undistort (DistortionRadTan.cpp:57-80).  Start at q = (px, py) and take at most 5
 *       steps.  A step evaluates the distortion d(q) (the formulas of the map above) and its Jacobian, with mx2 = qx qx, my2 = qy qy,
 *       mxy = qx qy, rho2 = mx2 + my2, rad = k1 rho2 + k2 rho2 rho2:
 *         J00 = 1.0 + rad + 2.0 k1 mx2 + 4.0 k2 mx2 rho2 + 2.0 p1 qy + 6.0 p2 qx
 *         J01 = 2.0 k1 mxy + 4.0 k2 rho2 mxy + 2.0 p1 qx + 2.0 p2 qy,  J10 = J01
 *         J11 = 1.0 + rad + 2.0 k1 my2 + 4.0 k2 my2 rho2 + 2.0 p2 qx + 6.0 p1 qy
 *       (each sum and product from left to right); e = p - d(q); du = (J^T J)^-1 J^T e in closed form: a = J00 J00 + J10 J10,
 *       b = J00 J01 + J10 J11, c = J01 J01 + J11 J11, g0 = J00 ex + J10 ey, g1 = J01 ex + J11 ey, det = a c - b b,
 *       du = ((c g0 - b g1) / det, (a g1 - b g0) / det); q += du; the iteration stops after the update iff ex ex + ey ey < 1e-15.
 *       The reference returns whatever it has after 5 steps; here the point is SOLVED iff the stop test fired and q is finite,
 *       otherwise it has no solution.  With all four coefficients zero the steps still run: d(q) = q, the first step finds e = 0
 *       and stops.
 *     Model 2 only, as CameraUnified::unproject (CameraUnified.cpp:81-99) with its `float` intermediates:
 *         rho2 = (float)(qx qx + qy qy), beta = (float)(1.0 + (1.0 - xi xi) (double)rho2),
 *         lambda = (float)((xi + (double)sqrtf(beta)) / (1.0 + (double)rho2));
 *       no solution if beta < 0 or (double)lambda - xi < 0; x = ((double)lambda qx) / ((double)lambda - xi), y likewise.
 *       Model 1: x = qx, y = qy.
 *     Into the undistorted image.  X = to_fx (x (1.0 + 1e-8)) + to_cx, Y = to_fy (y (1.0 + 1e-8)) + to_cy: the inverse of the map as
 *       mbavo_undistort_map builds it (x = xn / (1 + 1e-8)), not a second projection -- (X, Y) is the position whose map entry is
 *       the raw point.  A result that is not finite (lambda == xi, an overflow) counts as no solution too.
 *     No solution: X = Y = NaN, ok = 0.
 * mbavo_undistort_points_batch is the per-call entry: ONE launch on the context's stream, whatever n_cams is, not waited for (no
 * launch at all where no row has a point).  h_offsets is a HOST array of n_cams + 1 ints, non-decreasing, h_offsets[0] == 0; row
 * i's raw points, entries h_offsets[i] .. h_offsets[i+1] - 1 of d_uv (interleaved [u, v] doubles, device memory, 8-byte aligned),
 * go through camera i; d_xy receives (X, Y) in the same layout and d_ok_or_null, where given, 1 or 0 per point.  The cameras and
 * the offsets travel in ONE host-to-device copy into the context's scratch, as the cameras of mbavo_undistort_map_batch do, with
 * that call's remarks on pageable memory and a scratch that grows.  No H x W of the `to` image is taken: none is needed.
 * MBAVO_E_ARG, nothing launched: NULL ctx, h_cams or h_offsets; NULL d_uv or d_xy with a non-zero total; n_cams < 1 or > 65535;
 * offsets that decrease or do not start at 0; a camera mbavo_undistort_map_batch rejects (that call's checks without the H x W one).
 * mbavo_pairs_set_points_geometry: the geometry of the points of LATER mbavo_pairs_prepare_points, _update_points and
 * _track_frame_points calls, whose signatures do not change.  0, the state at creation: the undistorted geometry, as above.
 * 1: d_xy holds raw level-0 pixel coordinates of the pair's camera -- the object's one camera, or camera h_camera_of_pair[b] of its
 * set; in update_points row i is pair h_key_pairs[i].  A point is first tested against the raw image: 0 <= u && u <= Ws - 1 && 0 <=
 * v && v <= Hs - 1 in double (the rule of "valid at level 0" of the clearance mask; NaN fails): a return that projects outside
 * the raw image has no pixel and is dropped at every level.  Then it goes through the inverse camera, and from there on it is (X, Y, z) of
 * geometry 0, z unchanged -- the optical axis is shared; the NaN of "no solution" fails the "usable" test, so nothing else in the
 * keep rules changes.  The inversion happens inside the one points launch, once per level: launches, synchronisations, D2H bytes
 * (mbavo_pairs_last_stats, _update_stats) and the bytes of mbavo_pairs_plan are those of geometry 0, no scratch is added, and the
 * keypoint arrays and counts are, bit for bit, those of mbavo_undistort_points_batch followed by a geometry-0 call on its output
 * for the points inside the raw image.  A geometry-0 object launches what it launched before this entry existed.
 * MBAVO_E_ARG, nothing changed: a geometry other than 0 or 1; geometry 1 on an object with opts.undistort == 0. */
int mbavo_undistort_points_batch(mbavo_ctx *ctx, int n_cams, const mbavo_pairs_camera *h_cams /* n_cams */,
                                 const int *h_offsets /* n_cams + 1 */, const double *d_uv /* total x 2 */,
                                 double *d_xy /* total x 2 */, unsigned char *d_ok_or_null /* total */);
int mbavo_pairs_set_points_geometry(mbavo_pairs *pairs, int geometry);

/* ---- HOW FAR A POSE CAN BE TRUSTED: a 6 x 6 pose information and covariance and the chi test's keypoint flags per pair, for the
 * pose-graph or map back end that weights the pose, and for the mapper that handed its points to mbavo_pairs_prepare_points and
 * wants to know which of them the alignment rejects.  mbavo_pairs_report reports all B pairs at their knots as they are now: ONE
 * level-0 evaluation (mbavo_eval_batch(with_hessian = 1) on the B level-0 entries of the object's own problem array with
 * d_outlier = NULL, num_bad = 0 and num_residuals = 0 -- no keypoint excluded, whatever flags the last LM call ended with), ONE
 * launch of the report kernel (a workgroup per pair, no atomics), ONE device-to-host copy of B * sizeof(mbavo_pairs_report) and ONE
 * synchronisation, whatever B is.  It reads the knots, writes no state and may be repeated.
 *   The 6 x 6 quantity.  A pair has one frame, degree k and start index s (that of its capture time); its knots s .. s+k-1 are
 *     (t_i, R_i), the block's local parameters [dt_0 .. dt_{k-1} | dw_0 .. dw_{k-1}] with t_i += dt_i, R_i <- R_i Exp(dw_i).  Move
 *     the whole trajectory rigidly in keyframe coordinates by xi = (v, w): t_i <- t_i + v + w x t_i, R_i <- Exp(w) R_i, that is
 *     dt_i = v - [t_i]x w and dw_i = R_i^T w exactly (R_i Exp(R_i^T w) = Exp(w) R_i): stacked, A of 6k x 6, row 3i+r = [e_r |
 *     -[t_i]x row r], row 3k+3i+r = [0 | column r of R_i].  R_i is the rotation matrix of the knot's quaternion divided by its norm.
 *     The shift is exact for the spline -- the translation basis sums to 1, the cumulative rotation spline depends on relative
 *     rotations only -- so every sampled pose moves by the same (v, w).
 *       info_unit = (K P) A^T H_local A      H_local unpacked from the block, which is scaled by 1 / (K P); (K P) as a double product
 *       sigma2    = 2 cost K P / max(num_valid_px - 6, 1)          evaluated as ((2 cost) (K P)) / max(..)
 *       cov       = sigma2 info_unit^-1      by a 6 x 6 Cholesky factorisation in double
 *     H A first, row by row with j ascending, then A^T (H A); the upper triangle is computed and mirrored, info_unit and cov are
 *     symmetric to the bit.  This is the information of the FRAME POSE WITH THE MOTION INSIDE THE EXPOSURE HELD AT ITS ESTIMATE, in
 *     keyframe coordinates, order (v, w); it is not the marginal over all 6k knot parameters (out of scope: one short exposure
 *     leaves about half of H_local's spectrum near zero at k = 4, and a thresholded inverse would make the result jump).
 *     T_world = T_keyframe T: with T_keyframe = (R_k, t_k) and Ad = [R_k, [t_k]x R_k; 0, R_k], the covariance of the same rigid
 *     shift expressed in the world frame is Ad cov Ad^T (and the information Ad^-T info Ad^-1).
 *   Keypoint flags: detectOutliersAndUploadToGpu (blur_aware_direct_tracker.cpp:639-699) on the level-0 patch costs c_i of this
 *     evaluation.  mu and var run over the num_stat patches with c_i >= 1e-8 (var = sum (c_i - mu)^2 / num_stat); bound =
 *     max_chi_square_error * (double)sqrtf((float)var); keypoint i -- any i, also one below 1e-8 -- is flagged iff |c_i - mu| > bound;
 *     num_stat == 0: nothing is flagged.  The sums run in a fixed order (lane i takes keypoints i, i + 256, ..; butterfly within a
 *     wave, the four waves in order): the same bits from run to run and for any B.
 *   d_patch_cost_or_null, d_flags_or_null: device arrays of B x cap0 entries, cap0 = h_cells_per_level[0] of mbavo_pairs_plan; pair
 *     b's K entries start at b * cap0 (the evaluation's patch costs; 1 = flagged), entries from K on are not written.
 *   status: 0 reported.  MBAVO_E_RANGE: the capture time lies outside the pair's knots -- every double is NaN, num_flagged and
 *     num_stat are 0, the pair's patch costs and flags are not written (as mbavo_pairs_assess; the evaluation clamps such a pair's samples
 *     and raises the context's range status like any evaluation off the knots, so the next LM call on the context returns
 *     MBAVO_E_RANGE once -- predict and set_motion keep the times on the knots, only mbavo_pairs_set_states can move them off).  MBAVO_REPORT_SINGULAR: K = 0, or
 *     the factorisation met a pivot that is not finite or <= 0 -- cov is NaN, everything else is reported.  Other pairs are unaffected.
 *   Scratch: B packed blocks, B x cap0 patch costs, B valid counts and the B records, in one device allocation that the object makes
 *     at its FIRST report (with a pinned mirror of the records) and keeps: mbavo_pairs_plan and mbavo_pairs_last_stats do not count
 *     it, an object that never reports never holds it, and the first report pays for the allocation.
 *   mbavo_pairs_report_stats: launches, synchronisations, D2H bytes of the last report.  The evaluation's launches are counted from
 *     the engine's own witnesses, mbavo_last_kernel and mbavo_last_layout: 1 for the single-launch kernel ("k_fused_sp<..,true>"),
 *     else pose kernel (absent when the name ends in ",true>") + fused kernel (absent with out[0] = 0 tiles) + finalize.
 *   MBAVO_E_ARG, nothing launched: before the first prepare; before the first mbavo_pairs_set_motion or mbavo_pairs_predict; NULL
 *     h_out; max_chi_square_error negative or not finite.
 *   The report is meaningful between mbavo_lm_batch_levels and mbavo_pairs_commit: a commit that switches keyframes re-expresses the
 *   knots against a keyframe whose image arrives only with the next update.  mbavo_pairs_track_frame and its _points twin stay as
 *   they are; a frame with a report is the five calls mbavo_pairs_update, mbavo_pairs_predict, mbavo_lm_batch_levels,
 *   mbavo_pairs_report, mbavo_pairs_commit. */
#define MBAVO_REPORT_SINGULAR 1
/* (a struct tag without a typedef: the call carries the same name, and in C a typedef name and a function share one name space;
 * write `struct mbavo_pairs_report`) */
struct mbavo_pairs_report {                /* one per pair; 672 bytes, no padding */
    int status;                            /* 0, MBAVO_E_RANGE or MBAVO_REPORT_SINGULAR */
    int num_keypoints0;                    /* level-0 K */
    int num_flagged;                       /* keypoints the chi test flags at these knots */
    int num_stat;                          /* keypoints that entered mu / var (patch cost >= 1e-8) */
    double num_valid_px;                   /* in-bounds pixels, the evaluation's d_valid */
    double cost;                           /* level-0 cost at these knots, no keypoint excluded */
    double sigma2;                         /* residual variance estimate, grey levels squared */
    double T[7];                           /* pose at the capture time, as mbavo_pairs_assessment.T */
    double info_unit[36];                  /* 6 x 6, row-major, symmetric: pose information for unit residual variance */
    double cov[36];                        /* sigma2 * inverse(info_unit) */
};
int mbavo_pairs_report_size(void);         /* sizeof(mbavo_pairs_report) of the loaded library */
int mbavo_pairs_report(mbavo_pairs *pairs, double max_chi_square_error, struct mbavo_pairs_report *h_out /* B */,
                       double *d_patch_cost_or_null /* B x cap0 */, unsigned char *d_flags_or_null /* B x cap0 */);
int mbavo_pairs_report_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- WHAT THE ALIGNED BLURRED FRAME SAYS ABOUT EVERY KEYPOINT'S DEPTH.  Every other pairs call takes a keypoint's depth as a
 * constant from outside (a depth map, the lists of mbavo_pairs_prepare_points).  mbavo_pairs_refine_depths gives the mapper the
 * other half of a direct method: per keypoint the gradient g and Gauss-Newton curvature h of its blur-aware patch cost with respect
 * to its plane depth D, with the trajectory held at its estimate, and (apply = 1) the damped inverse-depth step written in place
 * into the object's keypoint depths.  It does not touch the evaluation kernels, the LM or any other call.
 *   Arithmetic: IEEE double, operation by operation, nothing contracted into a fused multiply-add, except inside the evaluation's
 *   own device functions, which are the definition of what they return (pose_entries.h, pixel_math.h: the pose entries, unit_ray,
 *   the per-sample warp up to the tap, tap_fetch / tap_blend, huber_weight, patch_rho_sum, patch_centre_rt).
 *   For pair b, level l, keypoint i = (kx, ky, D), the level's camera (fx, fy, cx, cy: the level-0 intrinsics of the pair's camera
 *   each divided by (double)(1 << l)), pattern (P offsets (dx_j, dy_j)) and S blur samples:
 *   1. Pose entries (t_s, R_s) of the S samples from the pair's knots as they are now, at the evaluation's sample times t_cap -
 *      t_exp 0.5 + s t_exp / (S - 1 + 1e-8); the mid-exposure pose is entry S / 2, as in the evaluation.  The patch centre (ox, oy)
 *      is patch_centre_rt at that pose: the reference-order form, so that no truncation below can differ from the evaluation's.
 *   2. Pixel j: px = (int)(ox + dx_j), py = (int)(oy + dy_j); valid iff 0 <= px <= W-1, 0 <= py <= H-1 and all S taps land in the
 *      keyframe (the evaluation's rule).  ray = unit_ray(px, py); iz = reciprocal(D + 1e-8).
 *   3. Sample s: r = R_s ray, C1 = reciprocal_1ulp(r_z), sc = (D - t_z) C1, Px = sc r_x + t_x, Py = sc r_y + t_y; (I_s, gx_s, gy_s) =
 *      the evaluation's tap with gradients of the keyframe at u = (iz fx) Px + cx, v = (iz fy) Py + cy in the object's
 *      keyframe_format; the warp's derivative at the fixed pixel
 *          du_s = fx (((C1 r_x) iz) - ((Px iz) iz)),   dv_s = fy (((C1 r_y) iz) - ((Py iz) iz)).
 *   4. r_j = quotient(sum_s I_s, (double)(float)S) - I_cur(px, py), the sum from s = 0 up, exactly the evaluation's residual: the
 *      synthesised intensity enters with sign sigma = +1.  d_j = inv_S acc_j with inv_S = 1.0 / (double)(float)S and acc_j = the
 *      sum over s ascending, from 0.0, of (gx_s du_s + gy_s dv_s).  The truncated pixel is piecewise constant in D: d_j is the
 *      derivative of the smooth piece.  An invalid pixel has r_j = 0 and d_j = 0.
 *   5. (w_j, rho_j) = huber_weight(r_j, huber_a).
 *   6. valid_i = the number of valid pixels, written for every keypoint; the keypoint is FULL iff valid_i == P.  For a full
 *      keypoint cost_i = patch_rho_sum(rho), g_i = patch_rho_sum(((w_j w_j) r_j) d_j), h_i = patch_rho_sum(((w_j w_j) d_j) d_j) --
 *      the evaluation's summation order for all three; cost_i is the evaluation's patch cost times K P (d_outlier = NULL).  A
 *      keypoint that is not full has g_i = h_i = cost_i = 0.
 *   7. The step, in inverse depth: rho = 1.0 / D, g_rho = -((D D) g_i), h_rho = ((D D) (D D)) h_i.  The keypoint is a candidate
 *      iff it is full and h_rho > min_info and h_rho > 0.  d_rho = -g_rho / h_rho, clamped to [-m, m] with m = max_rel_step rho;
 *      D_new = 1.0 / (rho + d_rho); the keypoint MOVES iff it is a candidate, D_new is finite, D_new >= z_min and (z_max == 0 or
 *      D_new <= z_max).  num_moved counts the moved keypoints and sum_sq_rel sums their (d_rho / rho)^2; only with apply = 1 is
 *      D_new stored (what mbavo_problem.d_kp_z points at; K, the coordinates, every pointer, knots and state never change).  The new
 *      depths hold until the pair's next prepare / update, and the next LM call reads them.
 *   8. A pair one of whose sample times is NaN or lies off its knots: status = MBAVO_E_RANGE in each of its records, the counts
 *      other than num_keypoints 0, the doubles NaN, none of its per-keypoint entries written, no depth moved; other pairs are
 *      unaffected.
 *   9. ONE launch of workgroups of 256 lanes.  The keypoints of a (pair, level) are cut into tiles of T = min(256, 1024 / P)
 *      (integer division) and shared by G = min(64, max(1, ceil(cap / T))) workgroups, cap the level's keypoint CAPACITY
 *      (h_cells_per_level of mbavo_pairs_plan): workgroup w takes tiles w, w + G, w + 2 G, .., and within a tile lane i serves
 *      keypoint tile T + i.  A record sum (cost, sum_sq_rel, num_full, num_moved) is formed as: every lane adds its keypoints'
 *      terms in ascending keypoint order, from 0.0 (a keypoint that is not full / not moved adds nothing); a workgroup's 256 lane
 *      sums are added by a butterfly within each wave (xor 32, 16, 8, 4, 2, 1: v = v + v_partner), then ((w0 + w1) + w2) + w3
 *      over the four waves; with G > 1 the G workgroup sums are added from 0.0 in the order w = 0 .. G-1 by whichever workgroup
 *      finishes last (one integer ticket per (pair, level) finds it; no floating-point atomics).  The same bits from run to run
 *      and for any B.  The grid is G_max x B x (1 or L) whatever the keypoint counts are: nothing is read back to size it.
 *   Arrays.  d_g, d_h, d_cost (doubles) and d_valid (ints) are device arrays, each optional.  level >= 0: B x cap[level] entries,
 *     cap = h_cells_per_level of mbavo_pairs_plan, pair b from b * cap[level]; h_out has B records.  level == -1: every level of
 *     every pair in the same ONE launch, the levels one behind the other per pair (sum_l cap[l] entries per pair, level l from
 *     sum_{m<l} cap[m]); h_out has B x L records, pair-major.  Entries from K on are not written.
 *   Cost: one host-to-device copy of the options, ONE launch whatever B, K and level are; with h_out_or_null == NULL nothing is
 *     waited for, else one copy of the records through a pinned mirror and ONE synchronisation.  mbavo_pairs_refine_stats:
 *     launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   Scratch: B x L records, B x L x 64 x 4 doubles of workgroup sums, B x L tickets and the options on the device, records and
 *     options with a pinned mirror, allocated at the FIRST call and kept; not counted by mbavo_pairs_plan or
 *     mbavo_pairs_last_stats, as the report's and the hypotheses' scratch.
 *   MBAVO_E_ARG, nothing launched or changed: before the first prepare; before the first mbavo_pairs_set_motion / mbavo_pairs_predict;
 *     NULL opts; level outside -1 .. L-1; apply other than 0 or 1; a negative or non-finite min_info, max_rel_step, z_min or z_max;
 *     max_rel_step >= 1; z_max != 0 && z_max < z_min.  Limits of this build, MBAVO_E_ARG as well: a reported level with P > 1024,
 *     or with so many blur samples that its S pose entries (472 bytes each at k = 4) do not fit a workgroup's LDS beside 26 KB.
 *   Like the report, the call is meaningful between mbavo_lm_batch_levels and mbavo_pairs_commit (a commit that switches keyframes
 *   re-expresses the knots against a keyframe whose image and depths arrive only with the next update).  mbavo_pairs_track_frame
 *   and its _points twin stay as they are.  Out of scope: a joint pose-and-depth solve, sub-pixel keypoints, the raw camera's
 *   geometry (depths are those of the undistorted pinhole keypoints).  The evidence of several frames added up per keypoint:
 *   mbavo_pairs_filter_depths, below. */
typedef struct mbavo_pairs_refine_opts {   /* zero-initialise; 56 bytes, no padding */
    int level;                             /* 0 .. L-1, or -1: every level of every pair (still ONE launch) */
    int apply;                             /* 0: report only, nothing of the object changes.  1: write the new depths */
    double min_info;                       /* a keypoint moves only if h_rho > min_info; 0: only h_rho > 0 */
    double max_rel_step;                   /* |d_rho| is clamped to max_rel_step * rho; 0: 0.25; else in (0, 1) */
    double z_min, z_max;                   /* a new depth outside [z_min, z_max] is not written; z_min 0: 1e-2; z_max 0: no limit */
    int reserved[4];
} mbavo_pairs_refine_opts;
/* (a struct tag without a typedef, as mbavo_pairs_report) */
struct mbavo_pairs_refine {                /* one per (pair, level) reported; 32 bytes, no padding */
    int status;                            /* 0, or MBAVO_E_RANGE (a blur sample's time off the knots) */
    int num_keypoints;                     /* K of that level */
    int num_full;                          /* keypoints with all P pixels valid */
    int num_moved;                         /* keypoints whose depth was (apply = 1) or would be (apply = 0) written */
    double cost;                           /* sum over the full keypoints of their unscaled patch cost, fixed order */
    double sum_sq_rel;                     /* sum over moved keypoints of (d_rho / rho)^2, fixed order */
};
int mbavo_pairs_refine_opts_size(void);    /* sizeof(mbavo_pairs_refine_opts) of the loaded library */
int mbavo_pairs_refine_size(void);         /* sizeof(struct mbavo_pairs_refine) of the loaded library */
int mbavo_pairs_refine_depths(mbavo_pairs *pairs, const mbavo_pairs_refine_opts *opts,
                              struct mbavo_pairs_refine *h_out_or_null,
                              double *d_g_or_null, double *d_h_or_null, double *d_cost_or_null, int *d_valid_or_null);
int mbavo_pairs_refine_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- A DEPTH FILTER OVER THE FRAMES OF A KEYFRAME.  One blurred frame constrains a keypoint's depth weakly, along the epipolar
 * direction of a short baseline hardly at all; a keyframe is tracked by many frames, and its keypoints and their order stay put
 * from the prepare / update that made them until the pair's next keyframe.  mbavo_pairs_filter_depths adds the evidence of those
 * frames up per keypoint -- a mean inverse depth and an information, with a prior and an innovation gate -- in state the object
 * keeps on the device, and (apply = 1) writes the fused depth into the object's keypoint depths.  Like the refinement it sits
 * between mbavo_lm_batch_levels and mbavo_pairs_commit; per frame: predict, update, lm_batch_levels, filter_depths, commit.
 *   Arithmetic: as mbavo_pairs_refine_depths -- IEEE double, operation by operation, nothing contracted.
 *   1. Measurement.  For every keypoint of the reported levels: valid_i, cost_i, g_i, h_i and FULL exactly as steps 1 - 6 of
 *      mbavo_pairs_refine_depths (the same device bodies).
 *   2. State, per keypoint slot (pair b, level l, i < cap[l]): mu (double, the mean inverse depth), info (double, the information,
 *      in 1 / (inverse depth)^2), n_obs (int, fused measurements), n_rej (int, gated measurements); four separate arrays, each B x
 *      sum_l cap[l] entries, pair b from b * sum_l cap[l], level l from sum_{m<l} cap[m] within the pair -- the layout of the
 *      refinement's level = -1 arrays, whatever `level` is.  Entries from K on are never written.
 *   3. Seeding.  The object keeps on the host one keypoint serial per pair, bumped whenever a call that returns 0 has rewritten that pair's keypoints:
 *      every pair on mbavo_pairs_prepare / _prepare_points, the pairs of h_key_pairs on mbavo_pairs_update / _update_points /
 *      _track_frame / _track_frame_points (an update with n_key = 0 bumps none).  The filter remembers per (pair, level) the serial
 *      it last seeded it at.  A reported (pair, level) whose serial differs, or every reported one under reset = 1, is SEEDED in
 *      this call before anything else happens to it: for every i < K, with D_i the keypoint's depth as it is,
 *          mu = 1.0 / D_i;  info = (prior_rel_sigma == 0) ? 0.0 : 1.0 / ((prior_rel_sigma mu) (prior_rel_sigma mu));  n_obs = n_rej = 0.
 *      With level >= 0 only that level of a pair is seeded.  Seeding never changes what any other call returns.
 *   4. Fusion of a FULL keypoint, D its depth as it is, s2 = sigma_i sigma_i:
 *          rho_c = 1.0 / D;  DD = D D;  g_rho = -(DD g_i);  h_rho = (DD DD) h_i;  hm = h_rho / s2.
 *      The keypoint is a candidate iff hm > min_info and h_rho > 0.
 *      Gate, only when gate_chi2 > 0 and info > 0:
 *          rho_m = rho_c - g_rho / h_rho;  e = rho_m - mu;  c2 = (e e) ((info hm) / (info + hm)).
 *      c2 > gate_chi2: the candidate is REJECTED -- n_rej + 1, nothing else of it changes, no depth is written.  Otherwise
 *          A = info + hm;  bv = info (mu - rho_c) - g_rho / s2;  d_rho = bv / A clamped to [-m, m], m = max_rel_step rho_c;
 *          rho_n = rho_c + d_rho;  D_new = 1.0 / rho_n.
 *      The candidate FUSES iff D_new is finite, D_new >= z_min and (z_max == 0 or D_new <= z_max): mu = rho_n, info = A, n_obs + 1,
 *      and only with apply = 1 the depth becomes D_new.  A candidate that neither fuses nor is gated changes nothing.  With
 *      prior_rel_sigma = 0, sigma_i = 0 and gate_chi2 = 0 the first call after a seed writes the depths of
 *      mbavo_pairs_refine_depths(apply = 1), bit for bit (info = 0 and mu - rho_c = 0 give A = h_rho and bv = -g_rho).
 *   5. Records: one per (pair, level) reported, ordered as the refinement's.  cost is the refinement's; sum_info sums A and
 *      sum_sq_rel sums (d_rho / rho_c)^2 over the fused keypoints.  Every sum (cost, sum_info, sum_sq_rel, num_full, num_fused,
 *      num_rejected) is formed as step 9 of the refinement forms its sums, on the same grid: the same bits from run to run and for
 *      any B.
 *   6. A pair one of whose sample times is NaN or lies off its knots: status = MBAVO_E_RANGE in each of its records, the counts
 *      other than num_keypoints 0, the doubles NaN, nothing fused, no depth moved; a (pair, level) of it that was to be seeded IS
 *      seeded (the seed needs no pose) and says so in `seeded`.  Other pairs are unaffected.
 *   Cost: one host-to-device copy (the options and one seed word per pair together), ONE launch whatever B, K and level are; with
 *     h_out_or_null == NULL nothing is waited for, else one copy of the records through a pinned mirror and ONE synchronisation.
 *     mbavo_pairs_filter_stats: launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   State and scratch: the four state arrays (24 bytes per keypoint slot), B x L records, B x L x 64 x 6 doubles of workgroup sums,
 *     B x L tickets, the options and seed words on the device, records and options with a pinned mirror, allocated at the FIRST
 *     call and kept; not counted by mbavo_pairs_plan or mbavo_pairs_last_stats.
 *   MBAVO_E_ARG, nothing launched or changed, state and remembered serials included: every case and build limit of
 *     mbavo_pairs_refine_depths; a negative or non-finite sigma_i, prior_rel_sigma or gate_chi2; reset other than 0 or 1.
 *   mbavo_pairs_filter_state hands out the device pointers of the four arrays, the entries per pair and the first entry of every
 *     level within a pair (entries of levels >= L are 0): the counterpart of mbavo_pairs_problems for the keypoints.  The pointers
 *     are writable -- a caller may set info per keypoint, from a sensor model say, after a seeding call -- and hold until
 *     mbavo_pairs_destroy.  MBAVO_E_ARG before the first accepted mbavo_pairs_filter_depths.  There is no other setter.
 *   Out of scope: a prior per keypoint as an argument of mbavo_pairs_prepare_points, the hand-over of a state to the pair's next
 *   keyframe, a joint pose-and-depth solve, sub-pixel keypoints, the raw camera's geometry. */
typedef struct mbavo_pairs_filter_opts {   /* zero-initialise; 96 bytes, no padding */
    int level;                             /* 0 .. L-1, or -1: every level of every pair (still ONE launch) */
    int apply;                             /* 0: the state alone moves.  1: write the fused depths as well */
    double min_info;                       /* a keypoint is a candidate only if hm > min_info; 0: only h_rho > 0 */
    double max_rel_step;                   /* |d_rho| is clamped to max_rel_step * rho_c; 0: 0.25; else in (0, 1) */
    double z_min, z_max;                   /* a new depth outside [z_min, z_max] is not fused; z_min 0: 1e-2; z_max 0: no limit */
    double sigma_i;                        /* intensity noise; 0: 1.0 */
    double prior_rel_sigma;                /* standard deviation of a seeded depth relative to its inverse depth; 0: no prior (info 0) */
    double gate_chi2;                      /* 0: no gate; > 0: a candidate with c2 above it is rejected */
    int reset;                             /* 1: seed every reported (pair, level) in this call; else 0 */
    int reserved[7];
} mbavo_pairs_filter_opts;
struct mbavo_pairs_filter {                /* one per (pair, level) reported; 48 bytes, no padding */
    int status;                            /* 0, or MBAVO_E_RANGE (a blur sample's time off the knots) */
    int num_keypoints;                     /* K of that level */
    int num_full;                          /* keypoints with all P pixels valid */
    int num_fused;                         /* keypoints whose measurement entered their state */
    int num_rejected;                      /* candidates the gate turned away */
    int seeded;                            /* 1: the (pair, level)'s state was seeded in this call */
    double cost;                           /* as mbavo_pairs_refine.cost */
    double sum_info;                       /* sum over fused keypoints of their new information A, fixed order */
    double sum_sq_rel;                     /* sum over fused keypoints of (d_rho / rho_c)^2, fixed order */
};
int mbavo_pairs_filter_opts_size(void);    /* sizeof(mbavo_pairs_filter_opts) of the loaded library */
int mbavo_pairs_filter_size(void);         /* sizeof(struct mbavo_pairs_filter) of the loaded library */
int mbavo_pairs_filter_depths(mbavo_pairs *pairs, const mbavo_pairs_filter_opts *opts, struct mbavo_pairs_filter *h_out_or_null);
int mbavo_pairs_filter_state(mbavo_pairs *pairs, double **d_mu, double **d_info, int **d_n_obs, int **d_n_rej,
                             long long *h_pair_stride, long long h_level_offset[8]);
int mbavo_pairs_filter_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- EVERY KEYPOINT'S DEPTH SEARCHED AMONG ND CANDIDATES.  Refinement and filter are local: their measurement is the derivative
 * of the patch cost at the depth the keypoint already has, and the step is clamped.  mbavo_pairs_search_depths is the global
 * counterpart: the same blur-aware patch cost evaluated at ND inverse-depth candidates per keypoint, the patch centre in the
 * blurred frame moving with the candidate (the epipolar search, done on the blurred image with the estimated in-exposure
 * trajectory), the best candidate kept with a sub-candidate parabola fit, a curvature and a runner-up.  It sits where the
 * refinement sits, between mbavo_lm_batch_levels and mbavo_pairs_commit; per frame: predict, update, lm_batch_levels,
 * [search_depths on a fresh keyframe], filter_depths (reset = 1 after a search), commit.
 *   Arithmetic: as mbavo_pairs_refine_depths -- IEEE double, operation by operation, nothing contracted.
 *   For pair b, level l, keypoint i with depth D_i as it is, ND = num_candidates:
 *   1. Candidates.  relative = 0: lo = rho_lo, hi = rho_hi; relative = 1: lo = rho_lo / D_i, hi = rho_hi / D_i.
 *          step = (hi - lo) / (double)(ND - 1);   rho_d = lo + (double)d * step;   D_d = 1.0 / rho_d,   d = 0 .. ND-1.
 *   2. Cost of candidate d: steps 1 - 6 of mbavo_pairs_refine_depths with D = D_d, the cost alone (the same device bodies without
 *      the gradient taps; the patch centre, hence the P truncated pixels, are those of D_d).  The candidate is FULL iff all P pixels
 *      are valid; c_d = patch_rho_sum(rho).  d_volume gets c_d, or NaN where the candidate is not full; num_full_i counts the full
 *      candidates of the keypoint.
 *   3. Selection, by comparisons only.  best = the full candidate with the lowest cost, the lowest index on a tie; -1 if no
 *      candidate is full.  cost_best = c_best (NaN if best = -1).  cost_second = the lowest cost among the full candidates with
 *      |d - best| > 1; NaN if there is none.
 *   4. Parabola, iff 0 < best < ND-1, candidates best-1 and best+1 are full and den = (c_- - 2.0 c_0) + c_+ > 0 (c_-, c_0, c_+ the
 *      costs at best-1, best, best+1):
 *          delta = 0.5 (c_- - c_+) / den, clamped to [-0.5, 0.5];   rho* = rho_best + delta step;   curv = den / (step step).
 *      Otherwise rho* = rho_best and curv = 0.  d_rho gets rho* (NaN if best = -1), d_curv gets curv.
 *      curv is the second difference of the cost in inverse depth: the units of the filter's `info` at sigma_i = 1, so a caller
 *      may write it through mbavo_pairs_filter_state after the seeding call.
 *   5. Acceptance.  The keypoint is SEARCHED iff best >= 0, and ACCEPTED iff it is searched and
 *          min_ratio == 0, or cost_second >= min_ratio cost_best (a NaN runner-up passes only when min_ratio == 0);
 *          a parabola exists and curv > min_curv, or no parabola exists and min_curv == 0;
 *          D_new = 1.0 / rho* is finite, D_new >= z_min and (z_max == 0 or D_new <= z_max).
 *      Only with apply = 1, and only for accepted keypoints, the depth becomes D_new (what mbavo_problem.d_kp_z points at); K, the
 *      coordinates, every pointer, knots and state never change.
 *   6. What stays untouched: the object's keypoint serial is NOT bumped and the filter's state is not touched, so the filter does
 *      not seed by itself after a search: a caller who searches after a seed passes reset = 1 to the next mbavo_pairs_filter_depths.
 *   7. A pair one of whose sample times is NaN or lies off its knots: as step 8 of mbavo_pairs_refine_depths -- status =
 *      MBAVO_E_RANGE in each of its records, num_searched = num_accepted = 0, the doubles NaN, none of its per-keypoint entries
 *      written, no depth moved; other pairs are unaffected.
 *   8. Records: one per (pair, level) reported, ordered as the refinement's.  cost sums cost_best and sum_ratio sums cost_best /
 *      cost_second (0 where cost_second is NaN or 0) over the accepted keypoints.  Every sum (cost, sum_ratio, num_searched,
 *      num_accepted) is formed as step 9 of the refinement forms its sums, on the same grid and tiles (a lane's keypoints in
 *      ascending order): the same bits from run to run and for any B; no floating-point atomics.
 *   Arrays.  d_rho, d_cost_best, d_cost_second, d_curv (doubles), d_best, d_num_full (ints) are device arrays, each optional, in
 *     the layout of the refinement's per-keypoint arrays for level >= 0 and for level == -1 alike; d_volume (doubles, optional) is
 *     that layout times ND, the candidate index fastest: entry ((pair's and level's offset + i) ND + d).  Entries from K on are not
 *     written.
 *   Cost: one host-to-device copy of the options, ONE launch whatever B, K, level and ND are; with h_out_or_null == NULL nothing
 *     is waited for, else one copy of the records through a pinned mirror and ONE synchronisation.  mbavo_pairs_search_stats:
 *     launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   Scratch: as the refinement's (records, B x L x 64 x 4 doubles of workgroup sums, tickets, options, a pinned mirror), allocated
 *     at the FIRST call and kept; not counted by mbavo_pairs_plan or mbavo_pairs_last_stats.
 *   MBAVO_E_ARG, nothing launched or changed: before the first prepare; before the first mbavo_pairs_set_motion / mbavo_pairs_predict;
 *     NULL opts; level outside -1 .. L-1; apply other than 0 or 1; relative other than 0 or 1; num_candidates outside 2 .. 64;
 *     rho_lo or rho_hi non-finite or not 0 < rho_lo < rho_hi; min_ratio in (0, 1); a negative or non-finite min_ratio, min_curv,
 *     z_min or z_max; z_max != 0 && z_max < z_min; the build limits of mbavo_pairs_refine_depths, with 32 KB of LDS beside the
 *     pose entries.
 *   Out of scope: a joint pose-and-depth solve, sub-pixel keypoints, the raw camera's geometry, a search against more than the one
 *   current frame, the hand-over of a state to the pair's next keyframe. */
typedef struct mbavo_pairs_search_opts {   /* zero-initialise; 80 bytes, no padding */
    int level;                             /* 0 .. L-1, or -1: every level of every pair (still ONE launch) */
    int apply;                             /* 0: report only, nothing of the object changes.  1: write the accepted depths */
    int num_candidates;                    /* ND, 2 .. 64 */
    int relative;                          /* 0: [rho_lo, rho_hi] are inverse depths.  1: they scale the keypoint's own, 1 / D_i */
    double rho_lo, rho_hi;                 /* finite, 0 < rho_lo < rho_hi */
    double min_ratio;                      /* accept only if cost_second >= min_ratio * cost_best; 0: no test; else >= 1 */
    double min_curv;                       /* accept only if curv > min_curv; 0: only curv > 0 where a parabola exists */
    double z_min, z_max;                   /* a new depth outside [z_min, z_max] is not accepted; z_min 0: 1e-2; z_max 0: no limit */
    int reserved[4];
} mbavo_pairs_search_opts;
struct mbavo_pairs_search {                /* one per (pair, level) reported; 32 bytes, no padding */
    int status;                            /* 0, or MBAVO_E_RANGE (a blur sample's time off the knots) */
    int num_keypoints;                     /* K of that level */
    int num_searched;                      /* keypoints with at least one full candidate */
    int num_accepted;                      /* keypoints whose depth was (apply = 1) or would be (apply = 0) written */
    double cost;                           /* sum over accepted keypoints of cost_best, fixed order */
    double sum_ratio;                      /* sum over accepted keypoints of cost_best / cost_second, fixed order */
};
int mbavo_pairs_search_opts_size(void);    /* sizeof(mbavo_pairs_search_opts) of the loaded library */
int mbavo_pairs_search_size(void);         /* sizeof(struct mbavo_pairs_search) of the loaded library */
int mbavo_pairs_search_depths(mbavo_pairs *pairs, const mbavo_pairs_search_opts *opts, struct mbavo_pairs_search *h_out_or_null,
                              double *d_rho_or_null, double *d_cost_best_or_null, double *d_cost_second_or_null,
                              double *d_curv_or_null, int *d_best_or_null, int *d_num_full_or_null, double *d_volume_or_null);
int mbavo_pairs_search_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- KEYPOINT DEPTHS SMOOTHED OVER THEIR IMAGE NEIGHBOURS.  Refinement, filter and search treat a keypoint alone; its neighbours
 * in the image mostly lie on the same surface.  mbavo_pairs_smooth_depths is the regularisation and outlier pass that follows a
 * depth update: every keypoint's inverse depth becomes a weighted mean over itself and those neighbours that agree with it, a
 * keypoint nothing agrees with is filled from all of its neighbours, and what can be done neither for is flagged.  Across a depth
 * step the two sides do not agree, so a surface edge survives.  It stays inside one keyframe and reads no pose; per frame: predict,
 * update, lm_batch_levels, [search_depths], [smooth_depths], filter_depths (reset = 1 after a search), commit.
 *   Arithmetic: IEEE double, operation by operation, nothing contracted, comparisons as written.
 *   For pair b, level l, keypoint i < K: D_i its depth as it is BEFORE the call -- every read of a depth in this call is of that
 *   value (a Jacobi sweep: no result depends on the order in which keypoints are processed); (x_i, y_i) its whole-pixel coordinates
 *   at that level as the object stores them; I_i the byte of the keyframe's level image at that pixel.
 *   1. Validity and weight.  valid_i iff D_i is finite and D_i > 0;  rho_i = 1.0 / D_i.  weights = 0: w_i = 1.0; weights = 1: w_i
 *      = the filter's `info` of that slot; weights = 2: w_i = d_weight[i], a double array in the layout of the refinement's
 *      per-keypoint arrays (for level >= 0 and level == -1 alike).  A weight <= 0 or NaN counts as 0.
 *   2. Neighbours.  N_i = all j != i of the same (pair, level) with |x_j - x_i| <= radius and |y_j - y_i| <= radius (pixels of that
 *      level, bounds inclusive), valid_j, w_j > 0, and max_intensity_diff == 0 or |I_j - I_i| <= max_intensity_diff.  Two keypoints
 *      on one pixel are neighbours.  C_i = the j of N_i with |rho_j - rho_i| <= max_rel_diff rho_i.
 *   3. Sums, always over ascending j, from 0.0, each product rounded, then added left to right:
 *          SW_C = sum_C w_j;  SR_C = sum_C (w_j rho_j);  SW_N, SR_N the same over N_i.
 *   4. A valid keypoint is SUPPORTED iff |C_i| >= min_support: rho' = (w_i rho_i + strength SR_C) / (w_i + strength SW_C).
 *      Otherwise FILLED iff fill == 1 and |N_i| >= min_support: rho' = SR_N / SW_N.  Otherwise OUTLIER: nothing is proposed.
 *   5. A proposal STANDS iff D_new = 1.0 / rho' is finite, D_new >= z_min and (z_max == 0 or D_new <= z_max); otherwise the
 *      keypoint keeps its class, but rho' = rho_i and it is not counted as moved (an outlier: rho' = rho_i).  With apply = 1 every
 *      keypoint whose proposal stands gets D_new as its depth (what mbavo_problem.d_kp_z points at); K, the coordinates, every
 *      pointer, knots, tracker state and the keypoint serial never change.
 *   6. Per-keypoint outputs, each an optional device array in the refinement's layout: d_rho (doubles) rho', NaN for an invalid
 *      keypoint; d_flags (bytes) 0 invalid, 1 supported, 2 filled, 3 outlier; d_support (ints) |C_i| (0 for an invalid keypoint).
 *      Entries from K on are not written.
 *   7. sync_filter = 1 (only with apply = 1 and after the filter's first accepted call): the filter's mu of every MOVED keypoint
 *      -- its proposal stands and rho' != rho_i -- becomes rho'; info, n_obs, n_rej stay.  sync_filter = 0: no filter state is touched.
 *   8. Records: one per (pair, level) reported, ordered as the refinement's.  sum_sq_rel sums ((rho' - rho_i) / rho_i)^2 over the
 *      valid keypoints: a lane's keypoints in ascending order (keypoint i in lane i mod 256 of workgroup (i / 256) mod G, G =
 *      min(64, max(1, ceil(capacity / 256)))), then as step 9 of the refinement forms its sums -- the same bits from run to run and
 *      for any B; no floating-point atomics.
 *   9. No pose is read: the call is valid before mbavo_pairs_set_motion, and there is no MBAVO_E_RANGE case.
 *   The device side: a spatial index per (pair, level) -- bins of edge s, the smallest integer >= radius with ceil(W / s) ceil(H / s)
 *     <= 4096, a bin-start table and the keypoint indices bin after bin, ascending within a bin -- kept by the object and rebuilt
 *     only where the pair's keypoint serial (step 3 of mbavo_pairs_filter_depths) or s differs from what it was built at.
 *   Cost: one host-to-device copy of the options, at most TWO launches (index, gather) whatever B, K and level are; a repeat call
 *     on unchanged keypoints with the same s is ONE.  With h_out_or_null == NULL nothing is waited for, else one copy of the records
 *     through a pinned mirror and ONE synchronisation.  mbavo_pairs_smooth_stats: launches, synchronisations, D2H bytes of the last
 *     call (all 0 after a rejected one).
 *   Scratch: records, B x L x 64 x 7 doubles of workgroup sums, tickets, options, a pinned mirror; the index (4097 ints per (pair,
 *     level), 12 bytes per keypoint slot) and the staging of the new values (16 bytes per slot), allocated at the FIRST call and
 *     kept; not counted by mbavo_pairs_plan or mbavo_pairs_last_stats.
 *   MBAVO_E_ARG, nothing launched or changed: a NULL handle or NULL opts; before the first prepare; level outside -1 .. L-1; apply,
 *     fill or sync_filter other than 0 or 1; weights outside 0 .. 2; weights = 1 or sync_filter = 1 before the filter's first
 *     accepted call; weights = 2 with a NULL d_weight; sync_filter = 1 with apply = 0; radius outside 1 .. 16; min_support < 1;
 *     max_rel_diff or strength not in (0, 1]; max_intensity_diff outside 0 .. 255; z_min or z_max negative or non-finite; z_max != 0
 *     && z_max < z_min.
 *   Out of scope: the hand-over to the next keyframe, a joint pose-and-depth solve, sub-pixel keypoints, an edge-preserving weight
 *   that is continuous in intensity, de-duplication. */
typedef struct mbavo_pairs_smooth_opts {   /* zero-initialise; 80 bytes, no padding */
    int level;                             /* 0 .. L-1, or -1: every level of every pair */
    int apply;                             /* 0: report only, nothing of the object changes.  1: write the depths that stand */
    int fill;                              /* 1: a keypoint without support is filled from all its neighbours; 0: it is an outlier */
    int sync_filter;                       /* 1: the filter's mu follows the moved keypoints (needs apply = 1); else 0 */
    int weights;                           /* 0: 1.0; 1: the filter's info; 2: d_weight */
    int radius;                            /* r, 1 .. 16 pixels of the level */
    int min_support;                       /* >= 1 */
    int max_intensity_diff;                /* 0: no test; else 1 .. 255 */
    double max_rel_diff;                   /* in (0, 1]: j agrees with i iff |rho_j - rho_i| <= max_rel_diff rho_i */
    double strength;                       /* lambda in (0, 1] */
    double z_min, z_max;                   /* a new depth outside [z_min, z_max] does not stand; z_min 0: 1e-2; z_max 0: no limit */
    int reserved[4];
} mbavo_pairs_smooth_opts;
struct mbavo_pairs_smooth {                /* one per (pair, level) reported; 40 bytes, no padding */
    int num_keypoints;                     /* K of that level */
    int num_valid;                         /* keypoints with a finite depth > 0 */
    int num_supported, num_filled, num_outliers; /* the valid keypoints by class */
    int num_moved;                         /* proposals that stand with rho' != rho_i */
    long long sum_support;                 /* sum of |C_i| over the valid keypoints */
    double sum_sq_rel;                     /* sum of ((rho' - rho_i) / rho_i)^2 over the valid keypoints, fixed order */
};
int mbavo_pairs_smooth_opts_size(void);    /* sizeof(mbavo_pairs_smooth_opts) of the loaded library */
int mbavo_pairs_smooth_size(void);         /* sizeof(struct mbavo_pairs_smooth) of the loaded library */
int mbavo_pairs_smooth_depths(mbavo_pairs *pairs, const mbavo_pairs_smooth_opts *opts, struct mbavo_pairs_smooth *h_out_or_null,
                              const double *d_weight_or_null, double *d_rho_or_null, unsigned char *d_flags_or_null,
                              int *d_support_or_null);
int mbavo_pairs_smooth_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- KEYPOINT DEPTHS AND FILTER STATE HANDED TO THE PAIR'S NEXT KEYFRAME.  When mbavo_pairs_commit reports is_keyframe = 1 the
 * next update overwrites the pair's keypoints and the new ones take their depths from the caller again: what the frames of the old
 * keyframe taught about depth is lost.  mbavo_pairs_carry_save warps the old keyframe's keypoints ONCE into the new keyframe's
 * camera and keeps them as a small per-pair set of CARRIED POINTS; after the update, mbavo_pairs_carry_adopt lets every new keypoint
 * gather a depth (and a filter state) from the carried points around it.  No depth map is written or read, nothing is scattered
 * into an image, no atomic touches global memory but the integer ticket the depth kernels share.  Per frame: update, [carry_adopt],
 * predict, lm_batch_levels, [search_depths] [smooth_depths] filter_depths, commit, [carry_save for the pairs whose verdict was 1].
 * mbavo_pairs_track_frame and its _points twin do neither.
 *   Arithmetic: IEEE double, operation by operation, nothing contracted, sums left to right, comparisons as written.
 *
 *   mbavo_pairs_carry_save(pairs, n, h_pairs, h_T, opts, h_out_or_null).  h_pairs: n pair indices, strictly ascending, 0 < n <= B.
 *   h_T: n x 7 doubles (t[3], q xyzw), the pose of the NEW keyframe in the OLD keyframe's frame, X_old = R X_new + t -- what
 *   mbavo_pairs_frame.a.T holds after the commit that gave the verdict; nothing is read from the tracker state.  R is formed from
 *   q on the host, once per listed pair, row-major with (x, y, z, w) = q:
 *       R00 = ww + xx - yy - zz;  R01 = -2 (wz - xy);        R02 = 2 (wy + xz);
 *       R10 = 2 (wz + xy);        R11 = ww - xx + yy - zz;   R12 = -2 (wx - yz);
 *       R20 = -2 (wy - xz);       R21 = 2 (wx + yz);         R22 = ww - xx - yy + zz
 *   (each product rounded, the terms added left to right), and travels with t in the ONE host-to-device copy of the options.
 *   For listed pair b, every level l, every keypoint i < K with (x, y) its coordinates at that level as the object stores them, D its
 *   depth as it is, and (fx, fy, cx, cy) the level-0 intrinsics of the pair's camera divided by 2^l:
 *   1. valid_i iff D is finite and D > 0.  An invalid keypoint is not carried.
 *   2. Warp.  rx = (x - cx) / fx;  ry = (y - cy) / fy;  d = (D rx - t0, D ry - t1, D - t2);
 *          X = (R00 d0 + R10 d1) + R20 d2;   Y = (R01 d0 + R11 d1) + R21 d2;   D' = (R02 d0 + R12 d1) + R22 d2.
 *   3. Projection.  The point is carried only if D' is finite, D' >= z_min and (z_max == 0 or D' <= z_max).
 *          u = fx (X / D') + cx;  v = fy (Y / D') + cy;  xf = floor(u + 0.5);  yf = floor(v + 0.5);
 *      and only if 0 <= xf < W_l and 0 <= yf < H_l (compared as doubles; NaN fails): a point outside is DROPPED, never clamped.
 *      Its pixel is (xi, yi) = ((int)xf, (int)yf).
 *   4. Carried values.  rho' = 1.0 / D';  c = (R02 rx + R12 ry) + R22;  s = (c (D D)) / (D' D')  (that is d rho' / d rho);
 *          w' = (w / (s s)) deflate,  with w = 1.0 (weights = 0) or the filter's `info` of the slot (weights = 1).
 *      A w' that is not > 0 or not finite drops the point.
 *   5. Storage.  Steps 1 - 4 are evaluated once per keypoint and STAGED per source index; the index below is counted and scattered
 *      from the staged values.  The carried points of a (pair, level) are kept with a bin-start table: bins of edge s, the smallest
 *      integer >= radius with ceil(W / s) ceil(H / s) <= 4096 (as mbavo_pairs_smooth_depths chooses it), points bin after bin and
 *      within a bin in ascending source index i -- the counting sort of the smoothing's index, the same device body.
 *   6. Records: one per (listed pair, level), pair after pair in the list's order, levels ascending.  sum_w sums w' over the carried
 *      points: keypoint i in lane i mod 256 of workgroup (i / 256) mod G, G = min(64, max(1, ceil(capacity / 256))), a lane's
 *      keypoints in ascending order, then as step 9 of mbavo_pairs_refine_depths forms its sums -- the same bits from run to run
 *      and for any B and n; no floating-point atomics.
 *   7. State.  The object remembers on the host, per pair, that a carried set is ARMED and with which radius.  A second save on an
 *      armed pair replaces its set.  Keypoints, depths, knots, tracker state, filter state and the keypoint serial never change.
 *   Cost: one host-to-device copy, TWO launches (warp and stage; index) whatever n and K are; with h_out_or_null == NULL nothing
 *     is waited for, else one copy of the records through a pinned mirror and ONE synchronisation.
 *   Scratch, allocated at the first carry call and kept, not counted by mbavo_pairs_plan or mbavo_pairs_last_stats: the carried
 *     sets (4100 ints per (pair, level); 36 bytes per keypoint slot, B x sum_l h_cells_per_level[l] slots), B x L records, B x L x
 *     64 x 4 doubles of workgroup sums, B x L tickets, the options and B list entries with a pinned mirror.
 *
 *   mbavo_pairs_carry_adopt(pairs, n, h_pairs, opts, h_out_or_null, d_rho_or_null, d_info_or_null, d_count_or_null,
 *   d_flags_or_null).  Call it after the update that gave the listed pairs their new keypoints; it reads no pose.  For listed pair
 *   b, every level l, every keypoint i < K at whole pixel (x, y) = ((int)x_i, (int)y_i), D_i its depth as the update left it:
 *   1. Neighbourhood.  N = the carried points j of that (pair, level) with |xj - x| <= radius and |yj - y| <= radius, the radius of
 *      the save that armed the pair.
 *   2. Foreground rule (a z-buffer with tolerance, by comparisons only).  rho_max = the largest rho'_j over N;
 *      C = the j of N with rho'_j >= (1.0 - max_rel_diff) rho_max.
 *   3. Sums over C in ascending source index j (the up-to-nine bins merged as the smoothing merges them), from 0.0, each product
 *      rounded, then added left to right:   SW = sum w'_j;   SR = sum (w'_j rho'_j).
 *   4. Flag.  0: N is empty.  2: |C| < min_support.  Otherwise rho_n = SR / SW, D_n = 1.0 / rho_n, and 1 (ADOPTED) iff D_n is finite,
 *      D_n >= z_min and (z_max == 0 or D_n <= z_max); else 3.
 *   5. apply = 1: an adopted keypoint's depth becomes D_n (what mbavo_problem.d_kp_z points at).  Every read of a carried point is
 *      of the save's buffers, so nothing is staged.  K, the coordinates, the keypoint serial, knots and tracker state never change.
 *   6. seed_filter = 1 (needs apply = 1 and the filter's first accepted call): the filter's state of every i < K of the listed
 *      pairs' levels is written -- adopted: mu = rho_n, info = (max_info == 0 || SW <= max_info) ? SW : max_info; any other keypoint:
 *      step 3 of mbavo_pairs_filter_depths with D_i and this call's prior_rel_sigma; n_obs = n_rej = 0 in both cases -- and the
 *      serial the filter remembers for those (pair, level)s becomes the pair's current one, so the next mbavo_pairs_filter_depths does
 *      not seed over it (it reports seeded = 0).
 *   7. Per-keypoint outputs, each an optional device array in the layout of the refinement's level = -1 arrays (pair b from b x
 *      sum_l cap[l], whether b is listed or not; entries of unlisted pairs and entries from K on are not written): d_rho (doubles)
 *      rho_n, NaN if not adopted; d_info (doubles) SW, 0 if not adopted; d_count (ints) |C|; d_flags (bytes) the flag of step 4.
 *   8. Records: one per (listed pair, level), ordered as the save's.  sum_info sums SW over the adopted keypoints; sum_sq_rel sums
 *      ((rho_n - rho_i) / rho_i)^2, rho_i = 1.0 / D_i, over the adopted keypoints whose D_i is finite and > 0.  Both are formed as the
 *      save's sum_w.
 *   9. Adopt DISARMS the listed pairs' carried sets.
 *   Cost: one host-to-device copy, ONE launch; records and waiting as the save's.
 *
 *   mbavo_pairs_carry_save_stats / _adopt_stats: launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   MBAVO_E_ARG, nothing launched or changed: a NULL handle, options or list (h_T for a save); n outside 1 .. B; indices out of
 *     range or not strictly ascending; before the first prepare; a non-finite h_T or |q|^2 outside 1 +- 1e-9; radius outside 1 ..
 *     16; deflate not in (0, 1]; weights, apply or seed_filter other than 0 or 1; max_rel_diff not in (0, 1]; min_support < 1; z_min,
 *     z_max, prior_rel_sigma or max_info negative or non-finite; z_max != 0 && z_max < z_min; seed_filter = 1 with apply = 0; weights
 *     = 1 or seed_filter = 1 before the filter's first accepted call; an adopt that lists a pair which is not armed.
 *   Out of scope: cross-level gathering, carrying into mbavo_pairs_track_frame, a unified `to` camera, sub-pixel keypoints, any
 *   depth map. */
typedef struct mbavo_pairs_carry_save_opts { /* zero-initialise; 48 bytes, no padding */
    int weights;                           /* 0: w = 1.0; 1: the filter's info */
    int radius;                            /* r of the later adopt, 1 .. 16 pixels of the level */
    double deflate;                        /* in (0, 1]: the carried weight's share that survives the hand-over */
    double z_min, z_max;                   /* a D' outside [z_min, z_max] is not carried; z_min 0: 1e-2; z_max 0: no limit */
    int reserved[4];
} mbavo_pairs_carry_save_opts;
struct mbavo_pairs_carry_save {            /* one per (listed pair, level); 24 bytes, no padding */
    int num_keypoints;                     /* K of that level */
    int num_valid;                         /* keypoints with a finite depth > 0 */
    int num_carried;                       /* points kept for the adopt */
    int reserved;
    double sum_w;                          /* sum of w' over the carried points, fixed order */
};
typedef struct mbavo_pairs_carry_adopt_opts { /* zero-initialise; 72 bytes, no padding */
    int apply;                             /* 0: report only, nothing of the object changes but the disarming.  1: write the adopted depths */
    int seed_filter;                       /* 1: write the filter's state as well (needs apply = 1); else 0 */
    int min_support;                       /* >= 1 */
    int reserved0;
    double max_rel_diff;                   /* in (0, 1]: j is foreground iff rho'_j >= (1 - max_rel_diff) rho_max */
    double z_min, z_max;                   /* a D_n outside [z_min, z_max] is not adopted; z_min 0: 1e-2; z_max 0: no limit */
    double prior_rel_sigma;                /* seed_filter = 1: the prior of a keypoint that is not adopted; 0: no prior (info 0) */
    double max_info;                       /* seed_filter = 1: cap of an adopted keypoint's info; 0: none */
    int reserved[4];
} mbavo_pairs_carry_adopt_opts;
struct mbavo_pairs_carry_adopt {           /* one per (listed pair, level); 32 bytes, no padding */
    int num_keypoints;                     /* K of that level */
    int num_adopted;                       /* flag 1 */
    int num_empty;                         /* flag 0 */
    int reserved;
    double sum_info;                       /* sum of SW over the adopted keypoints, fixed order */
    double sum_sq_rel;                     /* sum of ((rho_n - rho_i) / rho_i)^2 over the adopted keypoints with a valid D_i, fixed order */
};
int mbavo_pairs_carry_save_opts_size(void);  /* sizeof(mbavo_pairs_carry_save_opts) of the loaded library */
int mbavo_pairs_carry_save_size(void);       /* sizeof(struct mbavo_pairs_carry_save) of the loaded library */
int mbavo_pairs_carry_adopt_opts_size(void); /* sizeof(mbavo_pairs_carry_adopt_opts) of the loaded library */
int mbavo_pairs_carry_adopt_size(void);      /* sizeof(struct mbavo_pairs_carry_adopt) of the loaded library */
int mbavo_pairs_carry_save(mbavo_pairs *pairs, int n, const int *h_pairs, const double *h_T, const mbavo_pairs_carry_save_opts *opts,
                           struct mbavo_pairs_carry_save *h_out_or_null);
int mbavo_pairs_carry_adopt(mbavo_pairs *pairs, int n, const int *h_pairs, const mbavo_pairs_carry_adopt_opts *opts,
                            struct mbavo_pairs_carry_adopt *h_out_or_null, double *d_rho_or_null, double *d_info_or_null,
                            int *d_count_or_null, unsigned char *d_flags_or_null);
int mbavo_pairs_carry_save_stats(mbavo_pairs *pairs, long long out[3]);
int mbavo_pairs_carry_adopt_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- FLAGGED KEYPOINTS PRUNED ON THE DEVICE, THEIR STATE MOVED ALONG.  The report's chi-test flags, the smoothing's class bytes,
 * the hand-over's flags, the filter's n_rej / info / n_obs and the depth limits all say which keypoints of a keyframe are bad; the
 * batched LM starts every call with cleared outlier flags, and a keyframe's keypoint arrays otherwise change only in a prepare or
 * an update.  mbavo_pairs_prune_keypoints removes keypoints from the object's OWN arrays, per (pair, level), stable, in place, in
 * one launch: the survivors close ranks in ascending index, their depths and the filter's state move with them, and the device's
 * counts and the host's K (mbavo_pairs_problems) agree again when the call returns.  Nothing is prepared again, no image is read.
 *
 *   mbavo_pairs_prune_keypoints(pairs, n, h_pairs, opts, d_flags_or_null, h_out_or_null, d_keep_or_null).  h_pairs: n pair indices,
 *   strictly ascending, 0 < n <= B (the hand-over's list), or NULL with n = 0: every pair.  Pairs not listed are not touched: a pair
 *   whose keyframe has just changed has n_obs = 0 everywhere and is simply left out.  For listed pair b, every reported level l
 *   (opts->level, -1: every level), every keypoint i < K with D its depth as it is:
 *   1. Verdict, the FIRST criterion that holds, in this order:
 *        flag    d_flags given, f = its byte of the keypoint, f < 32 and bit f of drop_mask set (f >= 32 never drops);
 *        depth   check_depth = 1 and not (D finite, D >= z_min and (z_max == 0 or D <= z_max)): the limits themselves stay;
 *        filter  use_filter = 1 and (min_info > 0 and info < min_info) or (min_obs > 0 and n_obs < min_obs) or (rej_limit > 0 and
 *                n_rej >= rej_limit), on the filter's state of the slot (comparisons as written: a NaN info does not drop).
 *      A keypoint with no verdict is a SURVIVOR; kept = their number.  A zeroed options struct gives no verdict to any keypoint.
 *   2. min_keep.  If kept < K and kept < min_keep the (pair, level) is SKIPPED: nothing of it moves, its record has skipped = 1 and
 *      num_kept = num_before, while by_flag / by_depth / by_filter still count the verdicts of step 1.  Decided on the device, per
 *      (pair, level), after the count and before anything moves.
 *   3. apply = 1, not skipped: survivor i goes to place rank(i), its rank among the survivors in ascending index.  What moves: both
 *      coordinates, the depth and -- once the filter's state exists (its first accepted call), whether use_filter is set or not --
 *      mu, info, n_obs, n_rej of the slot.  Entries at and beyond the new count keep the bits they held; they are never written.
 *      The device's count of the (pair, level) becomes kept.  Images, gradients, picks / segment arrays, the pattern, the motion,
 *      the tracker state, an armed carried set and its radius are not touched; caller-owned per-keypoint arrays are the caller's to
 *      compact (d_keep says how).
 *   4. d_flags_or_null (bytes, read) and d_keep_or_null (bytes, written; not the same memory) are device arrays in the layout of
 *      the refinement's per-keypoint arrays for `level`: B x cap[level], or with level = -1 B x sum_l cap[l], pair b from b times
 *      that, whether b is listed or not.  With level = 0 the d_flags of mbavo_pairs_report can be passed as they are (drop_mask =
 *      1 << 1: the chi flags), with level = -1 those of mbavo_pairs_smooth_depths ((1 << 0) | (1 << 3): invalid and outlier) and of
 *      mbavo_pairs_carry_adopt.  d_keep receives, for every i < K of a served (pair, level), 1 if the keypoint stays and 0 if it
 *      goes (all 1 where the level is skipped), also with apply = 0; entries from K on and of pairs not listed are not written.
 *   5. Records: one per (listed pair, reported level), pair after pair in the list's order, levels ascending.  All sums are
 *      integers: the same bits from run to run and for any B and n.
 *   6. apply = 1: the call ENDS in one device-to-host copy and one synchronisation -- the records and behind them B x L ints, of
 *      which the served (pair, level)s' are their new counts -- and the host's K of those (pair, level)s follows; the next
 *      mbavo_lm_batch_levels, report or depth stage sees the pruned set.  A pair in which any level lost a keypoint gets a new
 *      keypoint serial: the spatial indices of the smoothing and the hand-over's adopt are rebuilt at their next use, and every
 *      level of the pair whose filter state was current stays current -- the next mbavo_pairs_filter_depths carries on from the
 *      moved state and reports seeded = 0; a level that was due for seeding stays due.
 *      apply = 0: a count only, nothing of the object changes; with h_out_or_null == NULL nothing is waited for.
 *   Cost: one host-to-device copy, ONE launch of one workgroup per (listed pair, reported level), which walks its slice twice in
 *     tiles of 256 (the count reads flag, depth and state alone), no atomics, no staging.
 *   Scratch, allocated at the first call and kept, not counted by mbavo_pairs_plan or mbavo_pairs_last_stats: B x L records and
 *     ints, the options and B list entries with a pinned mirror (and the unused sums and tickets of the depth stages' scratch).
 *
 *   mbavo_pairs_prune_stats: launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   MBAVO_E_ARG, nothing launched or changed: a NULL handle or options; before the first prepare; n = 0 with a list or n != 0
 *     without one, n outside 1 .. B, indices out of range or not strictly ascending; level outside -1 .. L - 1; apply, use_filter
 *     or check_depth other than 0 or 1; min_obs, rej_limit or min_keep negative; min_info, z_min or z_max negative or non-finite;
 *     z_max != 0 && z_max < z_min (checked whatever check_depth is); a non-zero reserved word; drop_mask != 0 without d_flags;
 *     use_filter = 1 before the filter's first accepted call.
 *   Out of scope: linking a point's copies across levels (each level is pruned on its own flags), pruning inside an LM call,
 *   moving caller-owned arrays, growing a keypoint set. */
typedef struct mbavo_pairs_prune_opts {    /* zero-initialise; 72 bytes, no padding */
    int level;                             /* -1: every level; else that level */
    int apply;                             /* 0: count only, nothing in the object changes; 1: compact */
    unsigned drop_mask;                    /* with d_flags: a keypoint whose flag byte f < 32 has bit f set here is dropped */
    int use_filter;                        /* 1: the three criteria below are read from the object's filter state */
    double min_info;                       /* > 0: drop if info < min_info */
    int min_obs;                           /* > 0: drop if n_obs < min_obs */
    int rej_limit;                         /* > 0: drop if n_rej >= rej_limit */
    double z_min, z_max;                   /* z_min 0: 1e-2; z_max 0: no limit */
    int check_depth;                       /* 1: drop a depth that is not finite or outside [z_min, z_max] */
    int min_keep;                          /* a (pair, level) that would keep fewer than this is left exactly as it is */
    int reserved[4];                       /* zero */
} mbavo_pairs_prune_opts;
struct mbavo_pairs_prune {                 /* one per (listed pair, reported level); 32 bytes, no padding */
    int status;                            /* 0 (the stage has no per-pair error) */
    int num_before, num_kept;              /* K before the call; the count after it (apply = 0: as it would be) */
    int by_flag, by_depth, by_filter;      /* every verdict counted once, under the FIRST criterion that holds */
    int skipped;                           /* 1: min_keep held it back; num_kept == num_before then */
    int pad;
};
int mbavo_pairs_prune_opts_size(void);     /* sizeof(mbavo_pairs_prune_opts) of the loaded library */
int mbavo_pairs_prune_size(void);          /* sizeof(struct mbavo_pairs_prune) of the loaded library */
int mbavo_pairs_prune_keypoints(mbavo_pairs *pairs, int n, const int *h_pairs, const mbavo_pairs_prune_opts *opts,
                                const unsigned char *d_flags_or_null, struct mbavo_pairs_prune *h_out_or_null,
                                unsigned char *d_keep_or_null);
int mbavo_pairs_prune_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- EACH PAIR'S BRIGHTNESS GAIN AND OFFSET, FITTED AND REMOVED.  The residual of every kernel is the synthesised keyframe
 * intensity against the current frame's grey level, as if both images had the same exposure time and gain.  A camera under
 * auto-exposure gives I_cur = a I_key + b between a keyframe and the frames that track it; the Huber cost then sees that as a
 * residual on every pixel and the pose is biased.  mbavo_pairs_match_brightness fits (a, b) per pair on the aligned patches of
 * one level, by iteratively reweighted least squares under the Huber weight, and (apply = 1) removes it from the pair's
 * current-frame pyramid inside the object, so that every later call (LM, report, refine, filter, search, hypotheses) reads the
 * corrected frame without knowing it.  It does not touch the evaluation kernels, the LM or any other call.
 *   Arithmetic: as mbavo_pairs_refine_depths -- IEEE double, operation by operation, nothing contracted into a fused
 *   multiply-add, except inside the evaluation's own device functions.
 *   For pair b at level l = opts.level, with the knots and depths as they are now, R = rounds:
 *   1. Items: steps 1 - 4 of mbavo_pairs_refine_depths without the gradient taps (the search's item): pose entries, the patch
 *      centre patch_centre_rt at entry S / 2, the truncated pixel, the evaluation's validity rule, the S intensity taps.  A valid
 *      pixel j gives s_j = quotient(sum_s I_s, (double)(float)S) and c_j = (double)I_cur(px, py).  A keypoint is FULL iff all its
 *      P pixels are valid; only full keypoints enter the fit.  num_full counts them, num_pixels = num_full * P.
 *   2. Round r = 0 .. R-1, from (a_0, b_0) = (1.0, 0.0): e_j = c_j - (a_r s_j + b_r) (product, sum, difference as written);
 *      (w_j, rho_j) = huber_weight(e_j, huber); ww_j = w_j w_j.
 *   3. Six sums: n = sum ww, Sx = sum ww s, Sy = sum ww c, Sxx = sum (ww s) s, Sxy = sum (ww s) c, C = sum rho.
 *   4. Their order.  Per full keypoint each of the six is patch_rho_sum over its P terms (the evaluation's order); the keypoint
 *      sums are then added exactly as the record sums of mbavo_pairs_refine_depths (step 9 there: the same tiles of T = min(256,
 *      1024 / P) keypoints and G = min(64, max(1, ceil(cap / T))) workgroups; a lane adds its keypoints ascending from 0.0; the
 *      butterfly within a wave; the four waves in order; the G workgroup sums from 0.0 in the order 0 .. G-1, by the workgroup
 *      that takes the last integer ticket).  No floating-point atomics: the same bits from run to run and for any B.
 *   5. The last workgroup of the (pair, round) solves the weighted normal equations,
 *          det = n Sxx - Sx Sx,   a = (n Sxy - Sx Sy) / det,   b = (Sy - a Sx) / n,
 *      and writes (a_{r+1}, b_{r+1}) = (a, b) to the device for the next round.
 *   6. The pair is DEGENERATE (status = MBAVO_PHOTO_DEGENERATE) iff in any round num_pixels < min_pixels, or !(det > (min_var n)
 *      n) -- the weighted variance of the synthesised intensities is det / (n n) --, or a or b is not finite, or a lies outside
 *      [gain_min, gain_max].  It reports gain 1.0, offset 0.0 and cost_after = cost_before, skips its later rounds and is not
 *      corrected.  (A pair without keypoints is degenerate.)
 *   7. cost_before is C of round 0; cost_after is C formed once more, in a launch of its own, under the final (a_R, b_R); gain
 *      and offset are (a_R, b_R).
 *   8. A pair one of whose sample times is NaN or lies off its knots: status = MBAVO_E_RANGE, the counts other than
 *      num_keypoints 0, the doubles NaN, nothing of it changed; other pairs are unaffected.
 *   Launches: a grid of G x B workgroups of 256 lanes per round and one more for cost_after: R + 1 whatever B and K are.
 *   The correction (apply = 1), for every pair with status 0: every pixel v of the pair's level-0 current frame in the object
 *     becomes (unsigned char)min(255.0, max(0.0, rint(((double)v - b) / a))) -- IEEE division, round half to even -- in ONE launch
 *     over all B frames (a pair that is not corrected keeps its bytes); then levels 1 .. L-1 of the B current frames are rebuilt by
 *     the pyramid launches of prepare and update, ceil((L-1) / 3) of them.  The object then holds exactly what mbavo_pairs_update
 *     with n_key = 0 would have made of the corrected level-0 images.  Nothing else changes: keyframes, gradients, keypoints,
 *     depths, filter state, knots, tracker state.  The correction holds until the pair's next prepare / update / track_frame,
 *     which brings a new frame.  A second call on a corrected frame fits what is left; composing the gains is the caller's
 *     business.  The black margin of an undistorted image is mapped like any other pixel (the clearance mask keeps keypoints off
 *     it).  apply = 0: a report only, nothing of the object changes.
 *   Cost: one host-to-device copy of the options, R + 1 launches, with apply 1 + ceil((L-1) / 3) more; with h_out_or_null == NULL
 *     nothing is waited for, else one copy of the B records through a pinned mirror and ONE synchronisation.
 *     mbavo_pairs_photo_stats: launches, synchronisations, D2H bytes of the last call (all 0 after a rejected one).
 *   Scratch, allocated at the FIRST call and kept, not counted by mbavo_pairs_plan or mbavo_pairs_last_stats: B records, B x 64 x
 *     7 doubles of workgroup sums (the six sums and the count of full keypoints), B tickets, the options and B x 2 doubles of (a,
 *     b) on the device; records and options with a pinned mirror.
 *   MBAVO_E_ARG, nothing launched or changed: a NULL handle or options; before the first prepare; before the first
 *     mbavo_pairs_set_motion / mbavo_pairs_predict; level outside 0 .. L-1; rounds outside 0 .. 8; apply other than 0 or 1;
 *     min_pixels negative; a negative or non-finite huber, min_var, gain_min or gain_max; gain_min > gain_max (after the defaults);
 *     the build limits of mbavo_pairs_refine_depths on that level, with 33 KB of LDS beside the pose entries instead of 26.
 *   Out of scope: a gain and offset inside the LM's state, composing corrections across calls; vignetting and response curves
 *   are the intake's business (mbavo_pairs_set_photometric below).
 *   mbavo_pairs_track_frame and its _points twin stay as they are. */
#define MBAVO_PHOTO_DEGENERATE 1
typedef struct mbavo_pairs_photo_opts {    /* zero-initialise; 64 bytes, no padding */
    int level;                             /* 0 .. L-1: the pyramid level the fit is made on */
    int rounds;                            /* 0: 3; else 1 .. 8 */
    int apply;                             /* 0: report only, nothing of the object changes.  1: correct the pair's current frame */
    int min_pixels;                        /* a pair with fewer fitted pixels is degenerate; 0: 64 */
    double huber;                          /* the fit's Huber threshold; 0: the object's huber_a; else > 0 and finite */
    double min_var;                        /* weighted variance of the s_j below which a pair is degenerate; 0: 4.0 grey levels squared */
    double gain_min, gain_max;             /* 0: 0.25 and 4.0; else 0 < gain_min <= gain_max, finite */
    int reserved[4];
} mbavo_pairs_photo_opts;
/* (a struct tag without a typedef, as mbavo_pairs_report) */
struct mbavo_pairs_photo {                 /* one per pair; 48 bytes, no padding */
    int status;                            /* 0, MBAVO_E_RANGE (a blur sample's time off the knots) or MBAVO_PHOTO_DEGENERATE */
    int num_keypoints;                     /* K of the level */
    int num_full;                          /* keypoints with all P pixels valid */
    int num_pixels;                        /* num_full * P: the pixels of the fit */
    double gain, offset;                   /* I_cur = gain I_key + offset; (1, 0) for a degenerate pair */
    double cost_before, cost_after;        /* sum rho of the fit residuals under (1, 0) and under (gain, offset), fixed order */
};
int mbavo_pairs_photo_opts_size(void);     /* sizeof(mbavo_pairs_photo_opts) of the loaded library */
int mbavo_pairs_photo_size(void);          /* sizeof(struct mbavo_pairs_photo) of the loaded library */
int mbavo_pairs_match_brightness(mbavo_pairs *pairs, const mbavo_pairs_photo_opts *opts, struct mbavo_pairs_photo *h_out_or_null /* B */);
int mbavo_pairs_photo_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- THE SENSOR'S PHOTOMETRIC CALIBRATION AT INTAKE.  Every kernel compares a synthesised keyframe intensity with the current
 * frame's grey level as if both were irradiance.  On an uncalibrated camera that fails twice: the vignette gives a keypoint that
 * moves towards a corner a residual that depends on where it lands, and a non-linear response makes "blur = mean of sharp
 * samples" wrong (averaging commutes with irradiance, not with gamma-encoded bytes).  An affine (a, b) per pair
 * (mbavo_pairs_match_brightness) absorbs neither.  mbavo_pairs_set_photometric gives the object the inverse response curve and the
 * vignette in the form the TUM monoVO / DSO calibration files standardised (pcalib.txt, vignette.png), and every later intake --
 * mbavo_pairs_prepare, _update, _track_frame and their _points twins -- corrects level 0 inside the ONE launch that fills it,
 * before the pyramid, in the geometry the images arrive in, rounding to a byte once.  The reference has no photometric
 * calibration: this comment is the definition.  An object on which the call was never made, or after
 * mbavo_pairs_clear_photometric, does exactly what it did before: the same launches, bytes and stats.
 *   Calibration g holds a table lut_g[256] of float and an inverse vignette inv_g, a float map in the geometry the images arrive
 *   in: Hs x Ws of the raw camera with mbavo_pairs_opts.undistort != 0, H x W otherwise.
 *   Table (mbavo_photometric_table, pure host, no device): lut[i] = (float)(scale * (255.0 * (G[i] - G[0]) / (G[255] - G[0]))),
 *     IEEE double, operation by operation.  G == NULL: the identity G[i] = i (with scale 1: lut[i] == i exactly).  MBAVO_E_ARG, the
 *     output untouched: a NULL output; a non-finite entry; G[255] <= G[0]; a decreasing step G[i+1] < G[i]; scale outside (0, 1]
 *     (NaN included).  `scale` is the headroom against saturation: the object stores bytes and lut / V exceeds 255 wherever V is
 *     small, so the caller chooses it to fit (min V is the safe choice) and expresses huber_a in scaled grey levels.
 *   Inverse vignette, ONE launch for all n maps: inv = (V is finite && V >= v_min) ? 1.0f / V : 0.0f, in float, IEEE division
 *     (v_min = 0: 0.0625f).  A pixel the vignette says nothing about becomes black, like a tap outside the raw image.  V == NULL:
 *     inv = 1.0f everywhere; the object keeps a flag and reads no map.
 *   Tap: t(x, y) = (double)lut[raw(x, y)] * (double)inv(x, y), a product of two floats formed in double: exact.
 *   Pinhole intake (undistort == 0): out = (unsigned char)(int)(fmin(t, 255.0) + 0.5).
 *   Raw intake (undistort != 0): the remap of mbavo_undistort_u8 with every dereferenced tap p_ij replaced by t at that raw pixel;
 *     the usability and outside rules stay, nothing is contracted, and the result is (unsigned char)(int)(fmin(v, 255.0) + 0.5).
 *   With the identity table, scale = 1 and no vignette both give the bytes of the uncalibrated path.
 * mbavo_pairs_set_photometric(pairs, n, h_G, d_vignette, opts): n must equal max(1, opts.num_cameras); calibration g belongs to
 *   camera g, so camera_of_pair selects it, and with one camera it applies to every pair.  h_G: n x 256 doubles or NULL (identity);
 *   d_vignette: n maps of Hr x Wr floats on the device or NULL.  Storage (n tables with a pinned mirror; the n inverse maps at the
 *   first call that brings a vignette) is allocated at the FIRST call and kept, not counted by mbavo_pairs_plan.  Cost: one
 *   host-to-device copy of the tables from the pinned mirror and at most one launch; NOTHING is waited for, not even the copy of
 *   the call before (every reader of the tables is an intake, and every intake ends in a synchronisation: of two calls without an
 *   intake between them the later one holds).  mbavo_pairs_photocal_stats: launches (0 or 1), synchronisations (0), D2H bytes (0)
 *   of the last accepted call.  It may be called again; the calibration applies to later prepares, updates and track_frames.  As
 *   with mbavo_pairs_set_cameras, a pair whose calibration changes needs a new keyframe in the next update.  With undistort != 0
 *   the raw size is the camera's, and once a call has brought a vignette the object holds maps of that size: a later
 *   mbavo_pairs_set_camera / _set_camera_unified / _set_cameras with another raw size returns MBAVO_E_ARG.
 *   MBAVO_E_ARG with nothing copied, launched or changed (the statistics of the call before included): a NULL handle; a wrong n; a
 *   table mbavo_photometric_table rejects (scale = 0 means 1.0); a negative or non-finite v_min; with undistort != 0 or
 *   num_cameras > 0 a call before the camera call.
 * mbavo_pairs_clear_photometric restores the uncalibrated path: launches and stats are again those of an object that never had a
 *   calibration (the storage stays).
 * Launches of an intake under a calibration: with undistort = 0 ONE launch over all n_key + n_cur images that changed, where the
 *   strided copies (no launch) and the scatter of a key list (one launch) were: a prepare and an update without key list count
 *   one launch more in mbavo_pairs_last_stats / _update_stats, an update with a key list the same number.  With undistort != 0
 *   the calibrated remap replaces the plain one: the counts do not change.  Synchronisations and D2H bytes never change.
 * mbavo_photometric_u8_batch is the stand-alone sibling for callers of mbavo_vo_* / mbavo_detect_semidense, as
 *   mbavo_undistort_u8_batch is for the remap: image i of n_img packed H x W images through table h_luts[cal] and the INVERSE
 *   vignette d_inv[cal] (NULL: none), cal = h_cal_of_image[i], or without a list 0 (n_cal == 1) or i (n_cal == n_img); the pinhole
 *   intake's device function, one copy of tables and list, ONE launch, nothing waited for; d_dst == d_src is allowed.  MBAVO_E_ARG:
 *   a NULL context, image or table pointer, n_img outside 1 .. 65535, a size < 1 or above 2^22 pixels, n_cal < 1, an index outside
 *   0 .. n_cal-1, no list with n_cal neither 1 nor n_img.
 * Out of scope: per-frame exposure times (the brightness match fits that gain); float or 16-bit image storage in the object;
 *   putting vignette-dead pixels into the clearance mask (callers can pass mbavo_pairs_set_masks); calibrating inside mbavo_vo_*
 *   (the stand-alone batch call serves those callers); estimating G or V. */
typedef struct mbavo_pairs_photocal_opts { /* zero-initialise; 32 bytes, no padding */
    double scale;                          /* 0: 1.0; else in (0, 1] */
    float v_min;                           /* 0: 0.0625f; else > 0 and finite */
    int reserved[5];
} mbavo_pairs_photocal_opts;
int mbavo_photometric_table(const double h_G_or_null[256], double scale, float h_lut[256]);
int mbavo_pairs_photocal_opts_size(void);  /* sizeof(mbavo_pairs_photocal_opts) of the loaded library */
int mbavo_pairs_set_photometric(mbavo_pairs *pairs, int n, const double *h_G_or_null /* n x 256 */,
                                const float *d_vignette_or_null /* n x Hr x Wr */, const mbavo_pairs_photocal_opts *opts_or_null);
int mbavo_pairs_clear_photometric(mbavo_pairs *pairs);
int mbavo_pairs_photocal_stats(mbavo_pairs *pairs, long long out[3]);
int mbavo_photometric_u8_batch(mbavo_ctx *ctx, int n_img, const unsigned char *d_src /* n_img x H x W */, int H, int W, int n_cal,
                               const float *h_luts /* n_cal x 256 */, const float *d_inv_or_null /* n_cal x H x W */,
                               const int *h_cal_of_image_or_null /* n_img */, unsigned char *d_dst);

/* ---- KEYPOINTS BY CORNER STRENGTH.  A pairs batch finds its keypoints by gradient magnitude, which cannot tell a corner from a
 * straight edge: an edge constrains the motion across it and nothing along it.  The reference's second detector type,
 * ENUM_SPARSE_SHI_TOMASI (FeatureDetectorSparse.cpp), scores with cv::goodFeaturesToTrack on the CPU; here the same response -- the
 * minimum eigenvalue of the windowed structure tensor -- is computed on the device and used under the project's own selection
 * (grid cells, or every candidate).  This comment is the definition of the score.
 *   For a level image I of H x W bytes, a pixel (x, y) and a radius r in {1, 2, 3}:
 *   kx, ky are right - left and bottom - top as integers (the doubled central differences of mbavo_image_gradients_u8), zero on the
 *     1-pixel border.
 *   a = sum kx^2, b = sum kx ky, c = sum ky^2 over the (2r+1) x (2r+1) window centred on the pixel.  Window positions outside the
 *     image contribute 0; n = (2r+1)^2 always, there is no renormalisation at the border; all three sums are exact in int
 *     (|a|, |b|, |c| <= 49 * 255^2).
 *   In double, nothing contracted: tr = (double)(a + c); s = sqrt((double)(a-c) * (double)(a-c) + 4.0 * (double)b * (double)b) (the
 *     argument is an exact integer below 2^53); d = tr - s, and d = 0 where d < 0; score = (float)sqrt(d / (8.0 * n)).
 *   This is the RMS gradient along the weakest direction of the window, in grey levels per pixel: the unit of
 *   mbavo_gradient_magnitude_u8, so a threshold means the same kind of thing under both responses.  Every operation is exact or one
 *   correctly rounded IEEE operation: numpy gives the same bits.  A constant image scores 0; an image with ky = 0 everywhere (a
 *   vertical step edge) scores exactly 0 (s = a exactly), and so does one with kx = ky everywhere (s = 2a exactly).
 *   A pixel is a candidate iff score > threshold, strictly; grid selection keeps the first pixel in row-major order with the
 *   strictly largest score in its cell.  The depth, border, clearance and mask tests and the compaction are what they were: they
 *   see a score where they saw a magnitude.
 * mbavo_corner_score_u8 is the stand-alone sibling of mbavo_gradient_magnitude_u8: one launch on the given stream, nothing waited
 *   for; d_score needs the alignment of a float only.  MBAVO_E_ARG: a NULL pointer, a radius outside 1 .. 3, H or W below 3.
 * mbavo_pairs_set_detector(pairs, opts) applies to every later mbavo_pairs_prepare, _update and _track_frame; the _points calls
 *   have no detector and ignore it.  The call launches nothing, copies nothing and enqueues nothing on the stream; the first
 *   score = 1 call allocates (one device allocation, whatever that costs in the runtime).  opts == NULL means score 0.  The first call
 *   with score = 1 allocates the score slices -- 4 bytes per pixel of every keyframe level, each slice padded as the gradient
 *   slices are: ONE device allocation that the object keeps until it is destroyed; mbavo_pairs_plan and mbavo_pairs_last_stats do
 *   not count it.  Keypoints already in the object stay until the next call that re-detects them.  A return to score 0 restores
 *   the old path exactly: launches, statistics and keypoints (the slices stay).  An object on which the call was never made does
 *   exactly what it did before.
 *   MBAVO_E_ARG with the mode unchanged and nothing allocated: a NULL handle; score outside {0, 1}; with score = 1 a radius outside
 *   1 .. 3 or a threshold that is negative or not finite; a non-zero reserved word.
 * Launches under score = 1: a prepare costs ONE launch more -- the score launch over every level of every keyframe, after the
 *   pyramid and before the selection; an update or track_frame with n_key > 0 one more too (over the listed pairs alone), with
 *   n_key == 0 none.  Synchronisations and D2H bytes do not change (mbavo_pairs_last_stats, _update_stats, _track_stats).
 * mbavo_pairs_detector_stats: out[0] the current score mode, out[1] the radius, out[2] the bytes held (0 for an object that never
 *   asked; still held after a return to score 0).
 * Out of scope: Harris's det - k tr^2; non-maximum suppression beyond one pick per cell; a minimum-distance rule; sub-pixel
 *   refinement; a score for mbavo_detect_semidense or mbavo_vo_* (they keep the reference's detector). */
typedef struct mbavo_pairs_detector_opts { /* zero-initialise; 32 bytes, no padding */
    int score;                             /* 0: gradient magnitude, the object as created.  1: the corner score above.  Else MBAVO_E_ARG */
    int radius;                            /* score 1: 1 .. 3 */
    float score_threshold;                 /* score 1: finite, >= 0; the object's creation threshold is not read in that mode */
    int reserved[5];                       /* must be 0 */
} mbavo_pairs_detector_opts;
int mbavo_corner_score_u8(const unsigned char *d_src, int H, int W, int radius, float *d_score, void *hip_stream);
int mbavo_pairs_detector_opts_size(void);  /* sizeof(mbavo_pairs_detector_opts) of the loaded library */
int mbavo_pairs_set_detector(mbavo_pairs *pairs, const mbavo_pairs_detector_opts *opts_or_null /* NULL = score 0 */);
int mbavo_pairs_detector_stats(mbavo_pairs *pairs, long long out[3]);

/* ---- synthetic blurred frame: synthesize_motion_blurred_img (ba_tracker/generate_synthetic_data.cpp:182-214):
 * mean of `num_samples` warps of the sharp image along the spline over the exposure, on a fronto-parallel plane.
 * Knots are host arrays; d_ref / d_out are device u8 images.  Synchronous. */
int mbavo_synthesize_blur(const unsigned char *d_ref, int H, int W, double plane_depth, const double intrinsics[4],
                          int spline_deg_k, double t0, double dt, const double *h_knots_t, const double *h_knots_R,
                          int N, double cap_time, double exp_time, int num_samples, unsigned char *d_out,
                          void *hip_stream);

/* ---- the caller of the path: BlurAwareDirectTracker (ba_tracker/blur_aware_direct_tracker.{h,cpp}).
 * Poses are 7 doubles: translation, then unit quaternion x,y,z,w (Core::Transformation's layout). */
int mbavo_se3_exp(const double h_tangent[6] /*upsilon, omega*/, double h_pose[7]);   /* Transformation::exp (.cpp:171-177) */
int mbavo_se3_log(const double h_pose[7], double h_tangent[6]);                      /* Transformation::log (.cpp:164-169) */
int mbavo_transform_mul(const double h_A[7], const double h_B[7], double h_out[7]);  /* operator* (.cpp:109-119) */
int mbavo_transform_inverse(const double h_A[7], double h_out[7]);                   /* inverse (.cpp:83-90) */
int mbavo_spline_transform_to(int spline_deg_k, double t0, double dt, double *h_knots_t, double *h_knots_R, int N,
                              double t, const double h_q_xyzw[4], const double h_t[3]); /* Spline.h:183-200 */
/* TransformByRight (Spline.h:212-219) on flat knot arrays: t_i += R_i * h_t, R_i = R_i * h_q; the constant-velocity prediction of
 * trackFrame (.cpp:119-141) */
int mbavo_spline_transform_by_right(double *h_knots_t, double *h_knots_R, int N, const double h_q_xyzw[4], const double h_t[3]);

typedef struct mbavo_vo_options { /* BlurAwareDirectTrackerOptions (blur_aware_direct_tracker.h:15-67) */
    int H, W, num_pyramid_levels;
    double intrinsics[4];
    int num_virtual_poses_per_frame[8], patch_size[8];
    const int *local_patch_pattern_xy[8]; /* host, (dx,dy) pairs; copied at creation */
    double huber_k;
    int max_consecutive_nonmonotonic_steps, max_num_iterations, solver_type, spline_deg_k;
    double min_step_quality, min_abs_cost_decrease;
    double dt_frame, dt_ctrl_knot, max_chi_square_error;
    double keyframe_max_flow_mag0, keyframe_max_flow_mag1, keyframe_max_flow_mag2, keyframe_max_blur_kernel_mag;
    float score_threshold; int grid_selection_cell_H, grid_selection_cell_W; /* reference: 25 / 30 / 30 (.cpp:353-358) */
    /* ABI 3 -- zero = default; the first three as in mbavo_track_opts */
    double fast_solve_ratio;
    int speculate, persist_levels;
    int keyframe_levels_at_once; /* pyramid, gradients and grid selection of ALL levels in three launches; default on [MBAVO_KF_MULTI] */
    int speculate_keyframe;      /* keyframe pre-processing started under the LM loop, on a second stream, when the predicted motion
                                    already passes the keyframe test (identical results); default on              [MBAVO_KF_SPECULATE] */
    int ride_along;              /* as mbavo_track_opts.ride_along */
    int resum;                   /* as mbavo_track_opts.resum */
    int reserved[2];
} mbavo_vo_options;
typedef struct mbavo_vo_info {
    int is_keyframe, num_keypoints0, num_trace, start_idx;
    double avg_flow, avg_kernel, final_cost;
} mbavo_vo_info;
typedef struct mbavo_vo mbavo_vo;
int mbavo_vo_create(mbavo_ctx *ctx, const mbavo_vo_options *opts, mbavo_vo **out);
int mbavo_vo_destroy(mbavo_vo *vo);
/* getSplineTrajectory()->InsertControlKnot(...) before the first frame (the `get_num_knots() == 0` test at .cpp:99) */
int mbavo_vo_set_spline(mbavo_vo *vo, double t0, double dt, int N, const double *h_knots_t, const double *h_knots_R);
int mbavo_vo_get_spline(mbavo_vo *vo, double *h_t0, double *h_dt, int *h_N, double *h_knots_t /*3*16*/, double *h_knots_R /*4*16*/);
/* LM records of the last mbavo_vo_track_frame's optimizeTrajectory (blur_aware_direct_tracker.cpp:590-924 logs them per
 * iteration), as mbavo_optimize_trajectory writes them, at most 512; returns the number copied (>= 0) or an error (< 0) */
int mbavo_vo_last_trace(mbavo_vo *vo, mbavo_trace_rec *trace, int trace_cap);
/* Checkpoint / resume of a tracker (the reference keeps this state in BlurAwareDirectTracker's members,
 * blur_aware_direct_tracker.h:69-125: mSplineTrajectory, mTKeyframe, mTprevB2W, mNeighFrameVelocity, mPrevTimestamp,
 * mIsFirstFrame): everything trackFrame carries from one frame to the next besides the keyframe's own data; the keyframe
 * (pyramid, gradients, keypoints) is re-made from its sharp frame and depth map by mbavo_vo_set_keyframe =
 * tmpProcessKeyframe (blur_aware_direct_tracker.cpp:342-415).  Poses are 7 doubles t[3], q[4] xyzw, restored bit for bit. */
typedef struct mbavo_vo_state {
    double t0, dt; int N, is_first;
    double knots_t[3 * 16], knots_R[4 * 16];
    double T_keyframe[7], T_prev_b2w[7], velocity[6], prev_timestamp;
} mbavo_vo_state;
int mbavo_vo_get_state(mbavo_vo *vo, mbavo_vo_state *h_state);
int mbavo_vo_set_state(mbavo_vo *vo, const mbavo_vo_state *h_state);
int mbavo_vo_set_keyframe(mbavo_vo *vo, const unsigned char *h_sharp, const float *h_depth_z, double sharp_cap_time);
int mbavo_vo_num_keypoints(mbavo_vo *vo, int level);
int mbavo_vo_get_keypoints(mbavo_vo *vo, int level, double *h_xy /*K*2*/, double *h_z /*K*/);
/* trackFrame (.cpp:88-203): images and the z-depth map of the sharp frame are HOST buffers (H x W), as the
 * reference's Core::Frame holds them; everything after the upload stays on the device. */
int mbavo_vo_track_frame(mbavo_vo *vo, const unsigned char *h_sharp, const float *h_depth_z, double sharp_cap_time,
                         const unsigned char *h_blur, double blur_cap_time, double blur_exp_time,
                         double h_T_out[7], mbavo_vo_info *info_or_null);

/* ---- multi-GPU: one process per GPU; the path shards with no exchange except the final sum of the normal equations
 * (the reference's reduction point: merge_hessian_gradient_cost, ba_tracker/merge_hessian_gradient_cost.cpp:39-86, called
 * at spline_update_step.cpp:232-239).  RCCL is resolved at run time (dlopen), so the library loads on hosts without it. */
/* Shards of one problem (host-side pointer arithmetic on the DEVICE pointers of `whole`; nothing is copied): contiguous
 * keypoint range [K*rank/world, K*(rank+1)/world) -- a band of the keyframe, since the detector emits keypoints row-major --
 * or contiguous frame range [F*rank/world, F*(rank+1)/world).  `shard->num_residuals` is set to the whole problem's count,
 * so the packed blocks of all shards ADD UP to the blocks of the whole problem (keypoint shards: every frame block is a
 * partial sum; frame shards: every rank owns its frames' blocks).  A frame shard may come out empty (F == 0 when
 * world > F): the caller skips its evaluation.  *h_first = first keypoint / frame of the shard (may be NULL). */
int mbavo_shard_keypoints(const mbavo_problem *h_whole, int rank, int world, mbavo_problem *h_shard, int *h_first);
int mbavo_shard_frames(const mbavo_problem *h_whole, int rank, int world, mbavo_problem *h_shard, int *h_first);
/* merge_hessian_gradient_cost (merge_hessian_gradient_cost.cpp:39-86) ON THE DEVICE for B problems: the F_b packed frame
 * blocks of problem b (d_frame_blocks, the layout mbavo_eval_batch writes; h_problems[b] supplies F, N, h_start_idx) are
 * scattered into its normal-equation system [cost | g (6N) | H (6N x 6N, column-major, symmetric)] = mbavo_system_len(N)
 * doubles, systems back to back in problem order.  Frames are added in ascending order (bit-reproducible).  For a
 * keypoint / frame shard (mbavo_shard_*) the result is that shard's PARTIAL system; the sum over ranks
 * (mbavo_allreduce_blocks) is the whole problem's system.  Asynchronous on the context's stream. */
int mbavo_system_len(int N); /* 1 + 6N + 36N^2 */
int mbavo_merge_device(mbavo_ctx *ctx, int B, const mbavo_problem *h_problems, int spline_deg_k,
                       const double *d_frame_blocks, double *d_systems);
/* The context's own RCCL communicator: rank 0 calls mbavo_comm_unique_id (ncclGetUniqueId) and hands the bytes to the
 * other ranks through any side channel (bench.py: a torch.distributed broadcast); every rank then calls mbavo_comm_init
 * (ncclCommInitRank on the context's device; collective).  mbavo_comm_ranks = ncclCommCount (0: no communicator). */
#define MBAVO_COMM_ID_BYTES 128
int mbavo_comm_unique_id(unsigned char h_id[MBAVO_COMM_ID_BYTES]);
int mbavo_comm_init(mbavo_ctx *ctx, const unsigned char h_id[MBAVO_COMM_ID_BYTES], int rank, int world);
int mbavo_comm_ranks(mbavo_ctx *ctx);
int mbavo_comm_destroy(mbavo_ctx *ctx);
/* In-place sum over all ranks of `count` doubles (packed blocks or merged systems) with ONE ncclAllReduce on the context's
 * stream, ordered after the kernels that wrote them (RCCL over xGMI).  `rccl_comm` = a caller-owned ncclComm_t, or NULL
 * for the context's own communicator (mbavo_comm_init); with neither: MBAVO_E_ARG. */
int mbavo_allreduce_blocks(mbavo_ctx *ctx, void *rccl_comm, double *d_blocks, long long count);
/* The same sum out of place (d_recv = sum over ranks of d_send).  Independent keyframe pairs sharded pair -> rank
 * (SURVEY.md 8e(1)): every rank evaluates its pairs straight into ITS slice of a send buffer whose other slices stay zero
 * -- nothing else ever writes them -- so the slices are disjoint, the sum is exact (x + 0 + ... + 0) and no buffer has to
 * be cleared between iterations. */
int mbavo_allreduce_blocks_to(mbavo_ctx *ctx, void *rccl_comm, const double *d_send, double *d_recv, long long count);
/* In-place ncclAllGather of equal slices: rank r's `count_per_rank` doubles sit at d_blocks + r * count_per_rank on entry,
 * every rank holds all slices on return (half the all-reduce's traffic for disjoint slices; needs equal slice lengths). */
int mbavo_allgather_blocks(mbavo_ctx *ctx, void *rccl_comm, double *d_blocks, long long count_per_rank);

/* ---- the same two collectives WITHOUT RCCL, sized for this path's messages (19 KB of one joint system ... 1.3 MB of 512 packed
 * blocks: latency-bound, where a ring pays a hop per rank): every rank maps every peer's receive region (hipIpcGetMemHandle /
 * hipIpcOpenMemHandle) and a collective is ONE kernel on the context's stream -- store this rank's slice into every peer's
 * region, raise a per-step flag there, wait for the peers' flags in the own region, then copy the slots out (all-gather) or
 * add them in rank order (all-reduce: every rank gets the same bits).  Replaces the exchange at the reference's reduction
 * point, merge_hessian_gradient_cost.cpp:39-86 / spline_update_step.cpp:232-239, like mbavo_allreduce_blocks above.
 *   mbavo_p2p_create   allocates this rank's region (2 x world slots of max_doubles_per_slot doubles: the largest
 *                      count_per_rank of an all-gather / count of an all-reduce that will be asked for) and returns its
 *                      64-byte IPC handle; the caller hands every rank's handle to every rank (all-gather of 64 bytes, as
 *                      with the RCCL id) and calls
 *   mbavo_p2p_connect  with the world x 64 bytes in rank order.  At most 16 ranks, all on GPUs of one node (ranks may share a GPU).
 *   Every rank must issue the same sequence of p2p collectives.  A peer that does not arrive within 20 s (mbavo_p2p_set_timeout:
 *   any time in (0, 3600] s, for the collectives enqueued after it) ends the kernel: what it would have written -- the peers'
 *   slices of an all-gather, the vector of an all-reduce -- is filled with NaN, so that an unreduced buffer cannot pass for a
 *   result, and mbavo_p2p_status (synchronises the stream) returns MBAVO_E_TIMEOUT from then on (sticky: the ranks' sequence
 *   numbers no longer agree; tear the regions down and create them again).
 *   Tear-down is two-phase, like any shared mapping: every rank finishes its last collective and calls mbavo_p2p_disconnect
 *   (unmaps the PEERS' regions); after a barrier of the caller -- nobody maps anybody any more -- every rank calls
 *   mbavo_p2p_destroy (frees its OWN region; also what mbavo_destroy does).  Freeing a region a peer still maps makes a later
 *   mbavo_p2p_create fail in hipIpcGetMemHandle (seen intermittently with three ranks when tear-down was one call). */
#define MBAVO_P2P_HANDLE_BYTES 64
int mbavo_p2p_create(mbavo_ctx *ctx, int rank, int world, long long max_doubles_per_slot, unsigned char *h_handle_out /*64*/);
int mbavo_p2p_connect(mbavo_ctx *ctx, const unsigned char *h_all_handles /* world x 64, rank order */);
int mbavo_p2p_ranks(mbavo_ctx *ctx); /* world once connected, else 0 */
int mbavo_allgather_blocks_p2p(mbavo_ctx *ctx, double *d_blocks, long long count_per_rank); /* in place, as mbavo_allgather_blocks */
int mbavo_allreduce_blocks_p2p(mbavo_ctx *ctx, double *d_blocks, long long count);          /* in place, as mbavo_allreduce_blocks */
int mbavo_p2p_status(mbavo_ctx *ctx);
int mbavo_p2p_set_timeout(mbavo_ctx *ctx, double seconds);
int mbavo_p2p_disconnect(mbavo_ctx *ctx);
int mbavo_p2p_destroy(mbavo_ctx *ctx);

/* ---- measurement: HIP-event timing of the dominant kernel (the fused residual/Jacobian/JtJ
 * kernel) on the context's stream, attached to the kernel's own dispatch (hipExtLaunchKernelGGL: begin / end
 * timestamps of the kernel).  enable = n > 0 starts a fresh collection that times every n-th launch (a timed
 * launch costs a few us of launch gap, so timing every launch would slow the measured region itself);
 * 0 stops.  read returns the summed duration in ms and the number of timed launches (blocks until the recorded
 * events completed). */
int mbavo_profile(mbavo_ctx *ctx, int enable);
int mbavo_profile_read(mbavo_ctx *ctx, double *h_fused_ms_sum, int *h_launches);
/* name of the dominant kernel the context's last evaluation dispatched, e.g. "k_fused<4,true,false,true>" (labels the timing):
 * k_fused<k, with H / g, gradient format, pose prologue fused> or k_fused_sp<k, with H / g, false, log2 S, single launch> */
const char *mbavo_last_kernel(mbavo_ctx *ctx);
/* read-only: the layout (tiling) the context's last evaluation ran on -- out[0] tiles, out[1] (problem, frame) slots, out[2] most
 * tiles in one slot, out[3] log2 S of the sample-parallel kernel (0: the lane-per-pixel kernel), out[4] 1 = the flat
 * (one-block-per-slot) finalize, out[5] 1 = some slot has no tile, out[6] the device's CU count, out[7] problems in the list.
 * All zero before the first evaluation.  Returns 0 or MBAVO_E_ARG. */
int mbavo_last_layout(mbavo_ctx *ctx, int out[8]);
/* host-side phase timers of the tracking loop (enabled by MBAVO_TIMING=1 in the environment): print the totals since
 * the last report to stderr and reset them.  Development aid; a no-op when the timers are off. */
void mbavo_timing_report(void);
/* The MBAVO_* override variables of the A/B tools (csrc/options.h) are read ONCE per process; a tool that changes one inside a
 * running process calls this afterwards.  Not for concurrent use with running API calls. */
void mbavo_reload_env(void);
/* process-wide counters of the host LM loop's ride-along evaluations (mbavo_track_opts.ride_along) since the last call:
 * out[0] commands that carried one, out[1] pyramid levels that started on theirs, out[2] levels that waited a wasted one
 * out before their first command (it shares the level's ticket counters and partials with that command).  Reset on read. */
void mbavo_ride_along_stats(long long out[3]);

const char *mbavo_version(void);
/* revision of the POD structs above (MBAVO_ABI_VERSION of the header the library was built with): compare before use */
int mbavo_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
