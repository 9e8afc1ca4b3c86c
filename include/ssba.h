/*
 * ssba.h -- C ABI of the MI355X-native stereo bundle-adjustment back end.
 *
 * This is the drop-in boundary for the one hot path of utiasSTARS/ceres-slam:
 * everything that happens inside `ceres::Solve` for the stereo BA problems its
 * drivers build.  The reference has no FFI or plugin table;
 * its "plugin point" is the Ceres C++ API as used by tests/dataset_vo.cpp:22-85 and
 * tests/dataset_ba_phong.cpp:26-255.  Each entry point below names the reference
 * call(s) it replaces (file:line into the reference repo).  A header-only C++ shim
 * with the reference's call shapes on top of this ABI is include/ceres_slam_amd/
 * ceres_shim.hpp; the binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no exceptions cross the ABI; every function returns an ssba_status
 *    (0 = ok, negative = error); ssba_status_string() names it.
 *  - parameter memory stays OWNED BY THE CALLER (the reference hands Ceres raw
 *    pointers into std::vector<SE3>/Point: dataset_vo.cpp:51-53); the library keeps
 *    device mirrors and writes the caller's blocks back in place when a solve ends
 *    with a usable solution -- exactly Ceres's contract.
 *  - a pose block is 12 doubles [t(3) | R row-major(9)] = T_c_g
 *    (include/ceres_slam/geometry/se3group.hpp:425-429); a point block is 3 doubles.
 *  - a handle is single-owner and not thread-safe (like ceres::Problem).
 *  - all arithmetic is IEEE fp64 on the GPU; there is NO CPU fallback: without a
 *    usable HIP device every compute entry point returns SSBA_ERR_NO_DEVICE.
 */
#ifndef SSBA_H_
#define SSBA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libssba.so is built with -fvisibility=hidden and a linker version script: the entry points declared in this header are
 * the ONLY dynamic symbols it defines (tests/test_capi_symbols.py compares `nm -D --defined-only` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#define SSBA_API __attribute__((visibility("default")))
#else
#define SSBA_API
#endif

#define SSBA_VERSION 1
/* longest landmark track (observations of one landmark) of the windowed layout; problems with longer tracks, or
 * with co-observing free poses more than 12 apart, run the general-structure kernels (ssba_stats.general_structure = 1)
 * -- except a loop closure whose far side is at most 5 states and whose landmarks keep <= 12 observations: those
 * states become a border of the block-tridiagonal reduced system and the windowed kernels stay (general_structure = 2;
 * any number of poses).  The border covers Levenberg-Marquardt solves; a DOGLEG solve or ssba_pose_covariance on such a
 * handle runs the symbolic phase again and continues on the general path (general_structure becomes 1);
 * SSBA_NO_CLOSURE_BORDER=1 in the environment of ssba_finalize selects the general path from the start */
#define SSBA_MAX_TRACK 12

typedef struct ssba_problem ssba_problem;

typedef enum {
    SSBA_OK = 0,
    SSBA_ERR_INVALID_ARGUMENT = -1,
    SSBA_ERR_HIP = -2,              /* a HIP runtime call failed (see ssba_last_error) */
    SSBA_ERR_NUMERICAL_FAILURE = -3,
    SSBA_ERR_NOT_FINALIZED = -4,
    SSBA_ERR_NO_DEVICE = -5,        /* no usable gfx950 device: no CPU fallback exists  */
    SSBA_ERR_UNSUPPORTED = -6,      /* structure outside this build's envelope          */
    SSBA_ERR_STATE = -7,            /* call sequence error                              */
    SSBA_ERR_TIMEOUT = -8           /* an RCCL set-up call did not return in time       */
} ssba_status;

/* StereoCamera<double> intrinsics (include/ceres_slam/stereo_camera.hpp:159-163) */
typedef struct { double fu, fv, cu, cv, b; } ssba_camera;

/* The ceres::Solver::Options fields the reference drivers set
 * (tests/dataset_vo.cpp:65-74, tests/dataset_ba_phong.cpp:79-88) plus the Ceres 1.x
 * defaults that shape the trust-region loop.  Unlisted Ceres options keep their
 * defaults.  trust_region_strategy_type: LEVENBERG_MARQUARDT (what dataset_vo.cpp runs)
 * and DOGLEG with dogleg_type TRADITIONAL_DOGLEG / SUBSPACE_DOGLEG (dataset_ba_phong.cpp:85-86,
 * dataset_vo_sun.cpp:142-143), both on an exact Schur-complement solve.  linear_solver_type
 * has no field: every solve is the reduced-camera-system solve Ceres' SPARSE_SCHUR performs. */
typedef struct {
    int32_t max_num_iterations;                 /* 50; drivers: 1000                   */
    int32_t use_nonmonotonic_steps;             /* 0;  drivers: 1                      */
    int32_t max_consecutive_nonmonotonic_steps; /* 5                                   */
    int32_t jacobi_scaling;                     /* 1                                   */
    int32_t max_num_consecutive_invalid_steps;  /* 5                                   */
    int32_t minimizer_progress_to_stdout;       /* 0                                   */
    int32_t num_threads;                        /* accepted, ignored (GPU)             */
    int32_t num_linear_solver_threads;          /* accepted, ignored (GPU)             */
    double initial_trust_region_radius;         /* 1e4                                 */
    double max_trust_region_radius;             /* 1e16                                */
    double min_trust_region_radius;             /* 1e-32                               */
    double min_relative_decrease;               /* 1e-3                                */
    double min_lm_diagonal;                     /* 1e-6                                */
    double max_lm_diagonal;                     /* 1e32                                */
    double function_tolerance;                  /* 1e-6                                */
    double gradient_tolerance;                  /* 1e-10                               */
    double parameter_tolerance;                 /* 1e-8                                */
    int32_t trust_region_strategy_type;         /* 0 = LEVENBERG_MARQUARDT (Ceres default, what
                                                   tests/dataset_vo.cpp runs); 1 = DOGLEG
                                                   (tests/dataset_ba_phong.cpp:85)                */
    int32_t dogleg_type;                        /* 0 = TRADITIONAL_DOGLEG (Ceres default); 1 =
                                                   SUBSPACE_DOGLEG (tests/dataset_ba_phong.cpp:86,
                                                   tests/dataset_vo_sun.cpp:143)                  */
} ssba_options;

/* ceres::TerminationType values the path can produce */
enum { SSBA_CONVERGENCE = 0, SSBA_NO_CONVERGENCE = 1, SSBA_FAILURE = 2 };

/* ceres::Solver::Summary fields the drivers print (summary.BriefReport():
 * tests/dataset_vo.cpp:82) plus per-phase device timings. */
typedef struct {
    int32_t termination_type;
    int32_t num_iterations;          /* recorded iterations incl. iteration 0          */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    double initial_cost;
    double final_cost;
    double total_time_s;             /* wall time of ssba_solve incl. write-back       */
    double device_time_s;            /* GPU time of the iteration loop (HIP events)    */
    /* bounds [Solver::Summary::num_line_search_steps]: evaluations of the projected line search, and how many searches
     * ran entirely on the device / were finished by the host (SSBA_LS_ROUNDS; unset: 2 evaluations enqueued per iteration, up to 4 once a search needed more) */
    int32_t num_line_search_steps;
    int32_t num_line_searches_on_device;
    int32_t num_line_searches_by_host;
    int32_t reserved_;
} ssba_summary;

/* ---- lifetime --------------------------------------------------------------------- */
/* replaces: ceres::Problem problem; + the shared StereoCamera captured by every
 * functor (tests/dataset_vo.cpp:26, stereo_reprojection_error.hpp:73).
 * device < 0 selects the current HIP device. */
SSBA_API int ssba_create(const ssba_camera *camera, int device, ssba_problem **out);
SSBA_API int ssba_destroy(ssba_problem *p);

/* ---- problem building ------------------------------------------------------------- */
/* replaces: the pose blocks passed to AddResidualBlock + SetParameterization(pose,
 * SE3Perturbation) (tests/dataset_vo.cpp:51-58; include/ceres_slam/perturbations.hpp:45-76).
 * `poses` is num*12 doubles, caller-owned, updated in place by a solve. */
SSBA_API int ssba_add_pose_blocks(ssba_problem *p, double *poses, uint32_t num);
/* replaces: the point blocks passed to AddResidualBlock (tests/dataset_vo.cpp:53);
 * `points` is num*3 doubles, caller-owned, updated in place. */
SSBA_API int ssba_add_point_blocks(ssba_problem *p, double *points, uint32_t num);
/* replaces: StereoReprojectionErrorAutomatic::Create(camera, obs, stiffness) +
 * problem.AddResidualBlock(cost, NULL, pose_k, point_j) for every observation
 * (include/ceres_slam/stereo_reprojection_error.hpp:59-69; tests/dataset_vo.cpp:39-56).
 * uvd is num*3 (u_l, v_l, d); stiffness is the shared 3x3 row-major Sigma^{-1/2}
 * (tests/dataset_vo.cpp:29-32).  May be called several times; order is kept. */
SSBA_API int ssba_add_stereo_observations(ssba_problem *p, const uint32_t *pose_index,
                                 const uint32_t *point_index, const double *uvd,
                                 uint64_t num, const double stiffness[9]);
/* replaces: problem.SetParameterBlockConstant / SetParameterBlockVariable(pose)
 * (tests/dataset_vo.cpp:62; tests/dataset_ba_phong.cpp:76,219-243) */
SSBA_API int ssba_set_pose_constant(ssba_problem *p, uint32_t pose, int is_constant);
/* replaces: passing `new ceres::HuberLoss(a)` instead of NULL to AddResidualBlock
 * (call-site shape tests/dataset_vo_sun.cpp:89-95); a <= 0 restores the NULL loss */
SSBA_API int ssba_set_huber_loss(ssba_problem *p, double a);
/* Uploads the problem graph and builds the device-side structure (once per graph). */
SSBA_API int ssba_finalize(ssba_problem *p);

/* ---- solving ---------------------------------------------------------------------- */
/* Ceres 1.x defaults */
SSBA_API void ssba_default_options(ssba_options *o);
/* replaces: ceres::Solve(options, &problem, &summary) (tests/dataset_vo.cpp:81).
 * Blocking.  Re-uploads the caller's current parameter values first. */
SSBA_API int ssba_solve(ssba_problem *p, const ssba_options *o, ssba_summary *s);
/* replaces: summary.BriefReport() (tests/dataset_vo.cpp:82) */
SSBA_API int ssba_brief_report(const ssba_summary *s, char *buf, size_t buf_len);

/* Stepwise form of ssba_solve for the bench harness and for multi-GPU drivers:
 * begin (upload + iteration 0), `step` enqueues n trust-region iterations on the
 * stream without host synchronisation, end synchronises and writes back.
 * With ignore_convergence != 0 the convergence tests are skipped so that exactly n
 * iterations of full work are executed (bench.py's timed region). */
SSBA_API int ssba_solve_begin(ssba_problem *p, const ssba_options *o, int ignore_convergence);
SSBA_API int ssba_solve_step(ssba_problem *p, int n);
SSBA_API int ssba_solve_end(ssba_problem *p, ssba_summary *s);
/* restores the parameter values uploaded by ssba_solve_begin and restarts the
 * trust-region state (device-to-device, asynchronous) */
SSBA_API int ssba_solve_restart(ssba_problem *p);
SSBA_API int ssba_synchronize(ssba_problem *p);

/* Per-iteration log of the last solve (the columns of Ceres's progress table).
 * Arrays of `capacity` entries or NULL; returns the number of recorded iterations. */
SSBA_API int ssba_iteration_log(ssba_problem *p, int32_t capacity, double *cost, double *cost_change,
                       double *gradient_max_norm, double *step_norm, double *relative_decrease,
                       double *trust_region_radius, int32_t *step_is_successful);

/* ---- streams, multi-GPU exchange, instrumentation ---------------------------------- */
/* Run on a caller-provided hipStream_t (e.g. torch's current stream). */
SSBA_API int ssba_set_stream(ssba_problem *p, void *hip_stream);
/* Landmark sharding: every rank adds ALL pose blocks and only ITS landmarks and
 * observations.  The library calls `fn` at the two exchange points of an iteration
 * with a device buffer of `count` doubles that must be reduced in place over all
 * ranks (op 0 = sum, 1 = max) on the stream given to ssba_set_stream -- e.g. a
 * torch.distributed all_reduce over RCCL.  fn == NULL (default) = single GPU. */
typedef int (*ssba_exchange_fn)(void *ctx, void *device_buffer, uint64_t count, int op);
SSBA_API int ssba_set_exchange(ssba_problem *p, ssba_exchange_fn fn, void *ctx);
/* Declares (before ssba_finalize) that the landmarks are sharded over `world_size` ranks:
 * every non-constant pose is then kept in the reduced system even if THIS rank holds no
 * observation of it, so that all ranks agree on the layout of the exchanged system. */
SSBA_API int ssba_set_distributed(ssba_problem *p, int world_size, int rank);
/* Partitioned reduced solve (after ssba_set_distributed, before ssba_finalize).  The free poses are
 * grouped into super-blocks of 12 (free-pose index / 12); separator_superblocks (world_size + 1 ascending
 * entries, first = 0, last = the last super-block) says that rank r's landmarks only observe poses of the
 * super-blocks [sep[r], sep[r+1]] -- i.e. the landmark ranges are cut where the co-visibility band crosses
 * a super-block boundary, so that consecutive ranks share exactly one super-block.  Each rank then
 * eliminates the interior of its own chain of the block-tridiagonal reduced camera system and only the
 * shared chain ends (the separator system: (world_size - 1) blocks of 72 x 72) are summed over the ranks and
 * solved everywhere -- < 1 MB per iteration instead of the whole reduced system, and no redundant solve of
 * the other ranks' chains.  At the end of the solve the poses are gathered (one more exchange), so every
 * rank returns the complete trajectory.  Without this call the ranks sum the whole reduced system and
 * each solves all of it (works for any sharding).  num = 0 clears the partition. */
SSBA_API int ssba_set_partition(ssba_problem *p, const uint32_t *separator_superblocks, uint32_t num);
/* Native exchange: the library itself enqueues ncclAllReduce (RCCL over xGMI) on the solver's stream at the exchange
 * points -- one process per GPU, no host language in the loop (this is what a sharded
 * tests/dataset_vo.cpp:22-85 links against).  Rank 0 calls ssba_rccl_unique_id (128 bytes) and hands the bytes to the
 * other ranks by whatever the application has (MPI, a file, torch.distributed); every rank then calls ssba_set_rccl
 * AFTER ssba_set_distributed(world_size, rank) -- a collective call: it returns once all ranks have joined.  It
 * replaces any callback set with ssba_set_exchange.  librccl.so is loaded on first use. */
#define SSBA_RCCL_UNIQUE_ID_BYTES 128
SSBA_API int ssba_rccl_unique_id(void *out, uint64_t size);
SSBA_API int ssba_set_rccl(ssba_problem *p, const void *unique_id, uint64_t size);
/* Both set-up calls above are time-limited (RCCL's own calls are not): after SSBA_RCCL_TIMEOUT_S seconds (environment,
 * default 180) they return SSBA_ERR_TIMEOUT and ssba_last_error() says which RCCL call did not return, which librccl.so
 * file the process had mapped (PyTorch ships its own copy) and its version, and the IPC / debug environment; the caller
 * can fall back to ssba_set_exchange.  ssba_rccl_describe writes that description of the loaded library at any time;
 * ssba_rccl_ranks returns ncclCommCount of the handle's communicator (0 without one). */
SSBA_API int ssba_rccl_describe(char *buf, uint64_t size);
SSBA_API int ssba_rccl_ranks(ssba_problem *p, int *count);
/* number of doubles in the per-iteration reduced-system exchange */
SSBA_API int ssba_exchange_size(ssba_problem *p, uint64_t *count);

/* Kernel timing with HIP events on the library's stream.  mode 0 = off, 1 = time every
 * kernel class (eager launches).  ssba_kernel_times returns up to `capacity` rows. */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
} ssba_kernel_time;
SSBA_API int ssba_set_kernel_timing(ssba_problem *p, int mode);
SSBA_API int ssba_kernel_times(ssba_problem *p, ssba_kernel_time *rows, int32_t capacity, int32_t *num);

/* Diagnostic builds only (-DSSBA_STAMPS, -DWD_STAMPS: tools/stamps_wide.py, tools/bcr_bench.hip): copies the first n (<= 8192) in-kernel
 * time stamps of the handle's debug buffer; the buffer stays zero in a normal build. */
SSBA_API int ssba_debug_stamps(ssba_problem *p, unsigned long long *out, int n);

/* Problem statistics after ssba_finalize. */
typedef struct {
    uint32_t num_poses, num_free_poses, num_points, num_active_points;
    uint64_t num_observations;
    uint32_t num_windows;          /* landmark groups sharing a <=12-pose window        */
    uint32_t num_superblocks;      /* 72x72 super-blocks of the block-tridiagonal S     */
    uint32_t num_reduced_blocks;   /* non-zero 6x6 blocks of S (upper incl. diagonal)   */
    uint32_t pose_bandwidth;       /* max free-pose index distance of co-observers      */
    uint64_t device_bytes;         /* device memory held by the handle                  */
    uint32_t general_structure;    /* 1: tracks > SSBA_MAX_TRACK or span > 12 poses -> dense reduced system; 2: windowed layout + closure border; 3: pose-only layout (every observed point block constant: one 6x6 system per pose, no Schur or reduction launches) */
    uint32_t pcr_blocks;           /* blocks handed to the parallel cyclic reduction (<= 128), 0 = plain BCR */
    uint32_t pcr_fused;            /* 1: one launch per step of that reduction (no border columns, single GPU; SSBA_NO_PCR_FUSED=1 in the environment of a solve keeps factor + reduce launches) */
    uint32_t wide_superblocks;     /* > 0: general layout whose tracks have 13..24 observations (free poses within a span of 24): the reduced system is block tridiagonal over this many super-blocks of 24 poses (144 rows), solved by parallel cyclic reduction (general_structure stays 1; SSBA_NO_WIDE=1 at ssba_finalize keeps the blocked Cholesky) */
} ssba_stats;
SSBA_API int ssba_get_stats(ssba_problem *p, ssba_stats *st);

/* Destroyed handles leave their device buffers, pinned host buffers and streams in a process-wide cache for the next
 * handle (drivers that solve thousands of small windows are bound by hipMalloc / hipFree otherwise); SSBA_POOL_MB caps
 * the cached device bytes (default 2048, 0 = no caching).  This call frees what is cached now. */
SSBA_API int ssba_release_cached_memory(void);

/* ---- test hooks (parity tests call these through the C ABI) ------------------------ */
/* Normal-equation blocks at the caller's current parameters, in user index order:
 * cost, g_p (P*6), g_l (L*3), H_pp (P*36 row-major), H_ll (L*9).  Blocks of constant
 * poses are zero.  Any output may be NULL. */
SSBA_API int ssba_evaluate(ssba_problem *p, double *cost, double *g_p, double *g_l, double *H_pp,
                  double *H_ll);
/* Dense reduced camera system S (n*n row-major, n = 6*num_free_poses) and rhs (n) for
 * trust-region radius `radius` at the caller's current parameters (S * delta_p = rhs),
 * and the step the device solver computes from it: delta_p (P*6), delta_l (L*3) and the
 * model cost change.  Any output may be NULL. */
SSBA_API int ssba_lm_step(ssba_problem *p, const ssba_options *o, double radius, double *S,
                 double *rhs, double *delta_p, double *delta_l, double *model_cost_change);
/* One DOGLEG step from scratch at the caller's current parameters: the kernels of a solve iteration in its order
 * (linearisation, the reduced system damped at radius 1/mu, its solve with the border of free shared blocks, the dogleg
 * vectors and scalars) with trust-region radius `radius`; o->dogleg_type selects TRADITIONAL (0) or SUBSPACE (1), the
 * strategy field is ignored.  Unscaled coordinates, in user index order:
 *   gn_p, v_p (P*6): Gauss-Newton step and v = s^2 g / D^2 of the poses (constant poses 0);
 *   gn_l, v_l (L*3, or L*6 with lighting observations): the same of the landmarks;
 *   gn_b, v_b (nb, column order of ssba_border_system): the same of the free shared blocks;
 *   scalars (SSBA_DOGLEG_NUM_SCALARS):
 *     [0..5]   |gradient_|^2, |gn|_D^2, gradient_ . gn, |J v|^2, |J gn|^2, Jv . Jgn (the first two squared from the norms
 *              the state keeps)
 *     [6..10]  alpha (Cauchy step), beta, gamma (delta = beta gn + gamma v), |delta|_D, model cost change of delta
 *     [11]     1 when the subspace of (gradient_, gn) is one-dimensional
 *     [12..15] subspace basis u_i = e[i][0] gradient_ + e[i][1] gn: e00, e01, e10, e11
 *     [16..20] subspace model g (2) and B (upper triangle: B00, B01, B11)
 *   (SUBSPACE only for [11..20]; TRADITIONAL leaves them 0).  Any output may be NULL. */
#define SSBA_DOGLEG_NUM_SCALARS 21
SSBA_API int ssba_dogleg_step(ssba_problem *p, const ssba_options *o, double radius, double mu, double *gn_p,
                     double *gn_l, double *gn_b, double *v_p, double *v_l, double *v_b, double *scalars);
/* One evaluation of the line-search function of the projected Armijo search along the step delta the last ssba_lm_step /
 * ssba_dogleg_step left on the device (a handle with lighting observations, bounds or not; SSBA_ERR_STATE otherwise, or once
 * another call has touched the solver state): phi(alpha) = cost(Plus(x, alpha delta)), phi'(alpha) = delta . gradient there.
 * It enqueues what the solver enqueues for one evaluation of a search the host drives, and no other kernel.
 *   ls_out (8): phi, phi', |dx_l|^2 of the landmark blocks, non-finite flag, max |delta|, g(x) . delta (= phi'(0), from the
 *               gradient of the linearisation), step validity, cost at x;
 *   the trial point in user index order: cand_poses (P*12), cand_points (L*3), cand_normals (L*3), cand_light (3),
 *   cand_phong (3M), cand_texture (M).  Any output may be NULL.  May be called again with another alpha. */
SSBA_API int ssba_line_search_probe(ssba_problem *p, double alpha, double *ls_out, double *cand_poses, double *cand_points,
                           double *cand_normals, double *cand_light, double *cand_phong, double *cand_texture);
/* The scalar state machine of the projected line search [Ceres 1.x line_search.cc ArmijoLineSearch::DoSearch, CUBIC
 * interpolation; bounds: tests/dataset_ba_phong.cpp:143-181] replayed on a given sequence of evaluations: phi(0),
 * phi'(0), max |direction|, then values[k] / gradients[k] = phi, phi' at the k-th step it asks for (steps_out[k], capacity
 * n).  on_device = 0 runs it on the host (no GPU needed), 1 in a one-lane kernel on `device` -- the solver uses both (the
 * search rounds enqueued with an iteration, and the searches handed back to the host) and they must agree bit for bit.
 * Returns the number of steps asked for (<= n), a negative status on error; *optimal_step = the accepted step or -1. */
SSBA_API int ssba_armijo_trace(const double *values, const double *gradients, int32_t n, double initial_cost,
                      double initial_gradient, double dir_max_norm, double *steps_out, double *optimal_step,
                      int32_t on_device, int32_t device);

/* ---- config 3: lighting terms on the same graph (tests/dataset_ba_phong.cpp:101-204) ---- */
/* The Phong driver adds, for every stereo observation (pose k, vertex j), an intensity residual
 * block over (pose, position, normal, material Phong parameters, texture, light) (:108-139) and a
 * normal residual block over (pose, normal) (:181-188), with UnitVectorPerturbation on the normal
 * (:191-193) and on a directional light (:201-204).  Landmark blocks become [position | normal]
 * (6-D local step); the shared blocks -- the light, and the Phong parameters [ka, ks, alpha] and the
 * texture kd of each material -- are a dense border of the reduced camera system, solved together
 * with the poses.  The border has nb = 3 + 4M columns with every kind free (M <= SSBA_MAX_MATERIALS:
 * nb <= 63); a border of more than 32 columns is kept as two panels of 32 and solves on one GPU.
 *
 * ssba_add_normal_blocks    : replaces AddParameterBlock / SetParameterization of
 *                             map_vertices[j].normal(); normals (num*3) caller-owned, updated in
 *                             place by ssba_solve like the points; num must equal the point count.
 * ssba_add_material_blocks  : material()->phong_params().data() (M*3) and texture()->data() (M),
 *                             caller-owned and updated in place when free; material_of_point maps
 *                             each point to its material (copied).  M <= SSBA_MAX_MATERIALS, with
 *                             any set of free kinds (landmark sharding: borders of at most 32
 *                             columns, i.e. seven materials with every kind free).
 * ssba_add_light_block      : dataset.light_pos.data() (light_type 0) or light_dir.data() (1),
 *                             caller-owned, updated in place when free.
 * ssba_set_shared_block_constant : SetParameterBlockConstant on ALL blocks of one kind
 *                             (:166-172, :205-206 -- the driver's "DEBUG: hold ... constant" lines and
 *                             its --multistage stages): which = SSBA_BLOCK_LIGHT / _PHONG / _TEXTURE.
 *                             Shared blocks are free by default, as in the driver.
 * ssba_add_lighting_observations : intensity (num) and observed normal (num*3) of the i-th stereo
 *                             observation already added (same order), 1/sqrt(int_var) and the 3x3
 *                             normal stiffness; num must equal the stereo observation count at
 *                             ssba_finalize.
 * ssba_set_shared_block_bounds : SetParameterLowerBound / SetParameterUpperBound on entry `index`
 *                             of ALL Phong-parameter (index 0..2 = ka, ks, alpha) or texture (index
 *                             0 = kd) blocks, as the driver does for every material (:142-180: ka, ks,
 *                             kd in [0,1], alpha >= 1); +-INFINITY = no bound.  With a bound on a free
 *                             block the problem is constrained and the minimiser does what Ceres 1.x
 *                             does: Plus projects onto the box and every trust-region step goes through
 *                             a projected Armijo line search.  The search runs on the device inside the
 *                             iteration's hipGraph: the test of the full step, then up to SSBA_LS_ROUNDS
 *                             (environment; unset: two, and as many as a search took -- at most four -- once
 *                             one has run out of them) further evaluations; a search that needs more parks the
 *                             solver until the host -- inside ssba_solve / ssba_solve_step / ssba_solve_end --
 *                             has run it (same state machine, same bits: csrc/ssba_linesearch.h).
 * With lighting observations present ssba_evaluate / ssba_lm_step return 6-wide landmark blocks:
 * g_l (L*6), H_ll (L*36), delta_l (L*6, local coordinates).  ssba_set_huber_loss keeps its meaning
 * (the loss sits on the stereo residual blocks; lighting blocks take a NULL loss, :113,186).  Lighting
 * terms shard by landmarks like the stereo terms (ssba_set_distributed); with FREE shared blocks the
 * border sums are exchanged in the all-reduce mode only (DOGLEG and bounds included: the projected line
 * search adds its sums over the ranks at every evaluation and is driven by the host in lockstep) -- the
 * partitioned reduced solve with free shared blocks returns SSBA_ERR_UNSUPPORTED, and so does landmark
 * sharding with a border of more than 32 columns. */
#define SSBA_MAX_MATERIALS 15
enum { SSBA_BLOCK_LIGHT = 0, SSBA_BLOCK_PHONG = 1, SSBA_BLOCK_TEXTURE = 2 };
SSBA_API int ssba_add_normal_blocks(ssba_problem *p, double *normals, uint32_t num);
SSBA_API int ssba_add_material_blocks(ssba_problem *p, double *phong, double *texture, uint32_t num_materials,
                             const uint32_t *material_of_point, uint32_t num_points);
SSBA_API int ssba_add_light_block(ssba_problem *p, double *light, int light_type);
SSBA_API int ssba_set_shared_block_constant(ssba_problem *p, int which, int is_constant);
SSBA_API int ssba_set_shared_block_bounds(ssba_problem *p, int which, int index, double lower, double upper);
SSBA_API int ssba_add_lighting_observations(ssba_problem *p, const double *intensity,
                                   double intensity_stiffness, const double *normal_obs,
                                   const double normal_stiffness[9], uint64_t num);
/* test hook: the border of the last ssba_lm_step -- nb = 3 [light] + 3M [Phong] + M [texture] as
 * freed (that column order; nb <= 63, every column whichever panel holds it), S_pb
 * (6*num_free_poses x nb), S_bb (nb x nb, damped), rhs_b (nb) of
 *   [S S_pb; S_pb^T S_bb] [delta_p; delta_b] = [rhs; rhs_b]
 * and the border step delta_b (nb).  Any output may be NULL. */
SSBA_API int ssba_border_system(ssba_problem *p, uint32_t *nb, double *S_pb, double *S_bb, double *rhs_b,
                       double *delta_b);

/* ---- Phong-lighting rows: batch evaluation on the device ------ */
/* replaces, for each of n residual-block instances, the evaluation Ceres performs on
 *   IntensityErrorPointLightAutomatic / IntensityErrorDirectionalLightAutomatic
 *     (include/ceres_slam/intensity_error_point_light.hpp:24-112,
 *      intensity_error_directional_light.hpp:24-113; blocks 12,3,3,3,1,3 -> 1 residual)
 *   NormalErrorAutomatic (include/ceres_slam/normal_error.hpp:22-54; blocks 12,3 -> 3)
 * with SE3Perturbation on the pose and UnitVectorPerturbation on the normal (and on the light
 * direction when light_type = 1) (perturbations.hpp:45-113; tests/dataset_ba_phong.cpp:102-204).
 * Per instance i: pose i (12), point i (3), normal i (3), phong i (ka,ks,alpha), texture i (kd),
 * observed colour i, observed normal i (3); shared: the light (position, light_type 0, or
 * direction, 1), the intensity stiffness 1/sqrt(int_var) and the 3x3 normal stiffness.
 * Outputs: r_int (n), J_int (n x 19 = [pose 6 | point 3 | normal 3 | phong 3 | texture 1 |
 * light 3], local coordinates), r_nrm (n x 3), J_nrm_pose (n x 18), J_nrm_n (n x 9).
 * This is the arithmetic of BASELINE config 3; its solver integration (6-D landmark blocks,
 * shared light/material border, bounds) is the next row. */
SSBA_API int ssba_phong_evaluate(int device, int light_type, uint64_t n, const double *poses,
                        const double *points, const double *normals, const double *phong,
                        const double *texture, const double light[3], const double *colour,
                        double stiffness, const double *normal_obs, const double normal_stiffness[9],
                        double *r_int, double *J_int, double *r_nrm, double *J_nrm_pose,
                        double *J_nrm_n);

/* replaces: problem.SetParameterBlockConstant(map_vertices[j].position().data()) on EVERY position block (stage 2 of
 * --multistage, tests/dataset_ba_phong.cpp:210-228; SetParameterBlockVariable afterwards = 0).  With lighting terms the
 * landmark block is then the normal alone.  On a stereo problem (no lighting terms) it means "every point", as if
 * ssba_set_point_constant had named them all: localisation against a fixed map.  Before ssba_finalize. */
SSBA_API int ssba_set_point_blocks_constant(ssba_problem *p, int is_constant);

/* replaces: problem.SetParameterBlockConstant(point) / SetParameterBlockVariable(point) on the listed position blocks of a
 * stereo problem (anchored or surveyed landmarks, map points of a marginalised window).  As in Ceres a constant point is not
 * part of x: no Jacobian columns, no Jacobi scale, no damping, no share in the step / parameter norms or the gradient max
 * norm; its residual blocks still count in the cost (also those on a constant pose); its coordinates come back bit-unchanged;
 * ssba_lm_step / ssba_dogleg_step report a zero step for it, ssba_evaluate zero H_ll / g_l, ssba_covariance_blocks zeros for
 * every block that touches it (the pose blocks are those of the inverse of the reduced system, to which a constant point adds
 * J_p^T J_p only).  Before ssba_finalize; an index >= the number of points: SSBA_ERR_INVALID_ARGUMENT.
 * Some points constant: windowed layout, one GPU.  ssba_finalize answers SSBA_ERR_UNSUPPORTED (ssba_last_error says which) for
 * a subset of the points with lighting terms, with landmark sharding or ssba_set_partition, on a handle with a closure border,
 * and on the wide (long-track) and blocked-Cholesky layouts.
 * EVERY point that has a residual block constant (one GPU, no lighting terms, no relative-pose block between two free poses):
 * the handle takes the pose-only layout, ssba_stats.general_structure = 3 -- pose-major observation records, one 6x6 system
 * per free pose, four launches per Levenberg-Marquardt iteration; track length, co-visibility span, repeated (pose, point)
 * pairs and per-block stiffness do not matter.  The covariance calls give the inverse of a pose's undamped 6x6 block
 * (SSBA_ERR_NUMERICAL_FAILURE when it is singular) and zeros elsewhere.  A DOGLEG solve and the test hooks (evaluate, LM
 * step, dogleg step) run the symbolic phase again onto the windowed layout before the first solve begins:
 * SSBA_ERR_UNSUPPORTED when the structure does not fit it, SSBA_ERR_STATE once a solve has begun.  SSBA_NO_POSE_ONLY=1 in
 * the environment of ssba_finalize selects the windowed layout from the start. */
SSBA_API int ssba_set_point_constant(ssba_problem *p, const uint32_t *points, uint64_t num, int is_constant);

/* ---- unary pose residual blocks (tests/dataset_vo_sun.cpp:80-124) ------- */
/* ssba_add_pose_prior replaces problem.AddResidualBlock(PoseErrorAutomatic::Create(T_k_0_ref, stiffness), loss,
 *   pose) (include/ceres_slam/pose_error.hpp:22-55; dataset_vo_sun.cpp:116-118): r = stiffness * log(T_ref T^-1) with
 *   the reference's log = [translation ; axis-angle] (se3group.hpp:337-342), 6 residuals; stiffness 6x6 row-major.
 * ssba_add_sun_observation replaces AddResidualBlock(SunSensorErrorAutomatic::Create(observed_dir_c, expected_dir_g,
 *   stiffness, az_err_thresh, zen_err_thresh), loss, pose) (sun_sensor_error.hpp:35-104; dataset_vo_sun.cpp:80-99):
 *   azimuth / zenith of R * expected_dir_g against the observation, wrap-around, outlier thresholds; 2 residuals;
 *   stiffness 2x2 row-major.  huber_a > 0 wraps the block in ceres::HuberLoss(huber_a) (:87-92), 0 = NULL loss.
 * Both before ssba_finalize; not on constant poses; not together with lighting terms or the partitioned reduced solve
 * (ssba_set_partition).  Landmark sharding with the all-reduce of the reduced system takes them: one rank adds them to the sums. */
SSBA_API int ssba_add_pose_prior(ssba_problem *p, uint32_t pose, const double T_ref[12], const double stiffness[36], double huber_a);
/* ssba_add_relative_pose replaces problem.AddResidualBlock(RelativePoseErrorAutomatic::Create(T_2_1_ref, stiffness), loss,
 *   pose1, pose2) (include/ceres_slam/relative_pose_error.hpp:22-57; tests/blowup_test.cpp:70-76):
 *   r = stiffness * log(T_2_1_ref * T_1 * T_2^-1), 6 residuals.  A block with one constant pose is a unary block on the other.
 *   Blocks between two free poses keep the windowed layout (ssba_stats.general_structure = 0) when the problem would be on it
 *   without them (tracks <= SSBA_MAX_TRACK, co-visibility span <= 12, no per-block stereo stiffness, no closure border,
 *   SSBA_FORCE_DENSE unset), has at least one stereo block, no lighting terms, is neither sharded nor partitioned, and every
 *   such block joins poses whose free-pose indices differ by exactly 1 (odometry between consecutive states; a constant pose
 *   between two free ones leaves them consecutive).  Several blocks on one pair are summed in the order they were added.
 *   Any other block (a loop closure, a block over two or more free poses, a pose graph without stereo blocks) sends the
 *   problem to the general-structure kernels (general_structure = 1), single GPU. */
SSBA_API int ssba_add_relative_pose(ssba_problem *p, uint32_t pose1, uint32_t pose2, const double T_2_1_ref[12], const double stiffness[36],
                           double huber_a);
SSBA_API int ssba_add_sun_observation(ssba_problem *p, uint32_t pose, const double observed_dir_c[3],
                             const double expected_dir_g[3], const double stiffness[4], double az_err_thresh,
                             double zen_err_thresh, double huber_a);

/* ssba_pose_covariance replaces ceres::Covariance::Compute + GetCovarianceBlockInTangentSpace for one pose block
 * (tests/dataset_vo_sun.cpp:159-183): cov (6x6 row-major) = that pose's block of (J^T J)^-1 in local (tangent)
 * coordinates at the caller's current parameters, i.e. of the inverse of the undamped reduced camera system.
 * SSBA_ERR_NUMERICAL_FAILURE when the system is rank deficient (Ceres: "Covariance computation failed").
 * Long tracks (a wide handle, ssba_stats.wide_superblocks > 0): once a solve has begun on the handle, the call runs on the
 * handle's own 144-row reduction, between solves or after ssba_solve_end as on a windowed handle; the handle stays on the
 * wide layout and a later ssba_solve runs exactly as if the call had not been made.  BEFORE the handle's first solve the call
 * still finalizes it again onto the general layout (blocked Cholesky), where the solves that follow then run.  A closure-border
 * handle is finalized again the same way, which is only possible before its first solve begins (afterwards SSBA_ERR_STATE; ask
 * before solving, or set SSBA_NO_CLOSURE_BORDER=1).  Landmark-sharded or partitioned handles and lighting terms:
 * SSBA_ERR_UNSUPPORTED. */
SSBA_API int ssba_pose_covariance(ssba_problem *p, uint32_t pose, double cov[36]);

/* ssba_covariance_blocks replaces ceres::Covariance::Compute + GetCovarianceBlock(InTangentSpace) for any list of
 * (pose | point, pose | point) pairs, computed in one call.  out receives the blocks one after another in request order,
 * each row-major and dim(a) x dim(b) with dim(pose) = 6 (tangent space) and dim(point) = 3: the block of (J^T J)^-1 at the
 * caller's current parameters (undamped, Huber-corrected, the system ssba_pose_covariance inverts).
 *   (pose i, pose j): Sigma_ij; (j, i) is its transpose.  (point l, point l): Sigma_ll = V^-1 + V^-1 W^T Sigma_TT W V^-1.
 *   (pose i, point l) / (point l, pose i): -Sigma_iT W V^-1 / its transpose (T: the free poses that observe l).
 *   Blocks touching a constant pose, or a point while points are held constant: zeros (as Ceres).
 *   (point l, point m), l != m: SSBA_ERR_UNSUPPORTED.  Index out of range, unknown kind, a point without residual blocks:
 *   SSBA_ERR_INVALID_ARGUMENT.  Reduced system or a needed landmark block not positive definite: SSBA_ERR_NUMERICAL_FAILURE.
 *   Lighting terms, landmark-sharded or partitioned handles: SSBA_ERR_UNSUPPORTED.
 * Windowed layout: one selected inversion of the block-tridiagonal reduced system (its diagonal and sub-diagonal super-blocks)
 * plus one multi-right-hand-side sweep per 5 poses whose blocks lie outside that band.  General layout: one blocked
 * Cholesky solve per 10 poses the request touches (requested poses and the observing poses of requested points).
 * State rules, closure border and long tracks as ssba_pose_covariance.  A wide (13..24 observation) handle on which a solve
 * has begun serves the request itself: the columns of Sigma for every pose the request touches (the general layout's rule),
 * 8 poses per sweep of its parallel cyclic reduction; it stays on the wide layout.  Before its first solve it is finalized
 * again onto the general layout, as a closure-border handle is -- for the closure border only possible before its first solve
 * begins (afterwards SSBA_ERR_STATE; ask before solving, or set SSBA_NO_CLOSURE_BORDER=1).  A later ssba_solve runs exactly
 * as if the call had not been made. */
#define SSBA_COV_POSE 0
#define SSBA_COV_POINT 1
typedef struct { uint32_t kind_a, index_a, kind_b, index_b; } ssba_cov_block;
SSBA_API int ssba_covariance_blocks(ssba_problem *p, const ssba_cov_block *blocks, uint64_t num, double *out);

/* ---- dense photometric alignment: ImageError blocks (include/ceres_slam/image_error.hpp) ------------------------
 * ssba_add_image_blocks replaces the loop of tests/dense_stereo_test.cpp:101-117: one ImageError residual block
 * (SizedCostFunction<1, 12, 1>) per reference pixel, on ONE pose block T_track_ref (12 doubles, SE3Perturbation) and one
 * disparity block per pixel.  pose, disparity (rows * cols, row-major) are caller-owned and updated in place by a solve; the
 * four images (rows * cols doubles each: reference image, tracked image and the two gradient images the functor samples) are
 * copied to the device at ssba_finalize.  A residual block exists for every pixel whose disparity is finite and > 0 at
 * ssba_finalize (:105); the pose and the disparities are uploaded again when a solve begins.  Pixels without a block and
 * constant disparities come back bit-unchanged.
 *
 * The arithmetic (fp64), for the block at reference pixel (u_r, v_r) with disparity d and pose [t | R]:
 *     p = triangulate(u_r, v_r, d),  q = R p + t,  (u, v) = project(q)[0:2]       (stereo_camera.hpp:77-144)
 *     SSBA_IMAGE_NEAREST   I(u, v) = I[floor(v + 1/2)][floor(u + 1/2)]   (image_error.hpp:156-164 as it stands)
 *     SSBA_IMAGE_BILINEAR  I(u, v) from the four neighbours of (floor u, floor v) (what its comment says it is meant to be)
 *     in bounds: 0 <= u, 0 <= v and u < cols - 1/2, v < rows - 1/2 (NEAREST) or u < cols - 1, v < rows - 1 (BILINEAR)
 *     r = track(u, v) - ref[v_r][u_r],   g = [gradx(u, v), grady(u, v)]
 *     J_pose = g P(q) [I | -q^]   (1 x 6, local coordinates of SE3Perturbation, translation then rotation, as on stereo blocks;
 *                                  P = the first two rows of the projection Jacobian)
 *     J_disp = g P(q) R dp/dd     (dp/dd = the third column of the triangulation Jacobian)
 *     out of bounds: r = 0, J_pose = 0, J_disp = 0 (:102-128).  No stiffness.  NULL loss: cost = 1/2 sum r^2.
 *     ssba_set_huber_loss(p, a) with a > 0 (before or after ssba_finalize; a <= 0 restores the NULL loss) puts ceres::HuberLoss(a)
 *     on every block, applied by Ceres' corrector with rho'' <= 0 exactly as on the stereo blocks:
 *         r^2 > a^2 (strictly):  sc = sqrt(max(DBL_MIN, a / |r|)),  r~ = sc r,  J~_pose = sc J_pose,  J~_disp = sc J_disp,
 *                                the block's cost is 1/2 (2 a |r| - a^2);
 *         otherwise the row is unchanged and the block's cost is 1/2 r^2.  Out-of-bounds rows (r = 0) are never corrected.
 *     Everything the minimiser forms (sums, Jacobi scales, damping, V, delta_d, gradient norm, model cost change) comes from the
 *     corrected row; the cost of a candidate is 1/2 sum rho of its raw residuals.
 * Two deliberate differences from the reference's text.  Its bounds test (u < cols, v < rows, :167-172) lets round() pick column
 * `cols` or row `rows`, one past the end; here a block is in bounds only when every pixel it reads is inside the image, which
 * differs from the reference exactly where the reference reads past the end of a row.  And :97-99 takes
 * tri_jac.block(2, 0, 3, 1), which lies outside the 3 x 3 matrix; the column it means (d p / d disparity) is used.
 * The minimiser is the Levenberg-Marquardt loop of every other layout; free disparities are part of x (norms, step norm,
 * gradient max norm) and are eliminated per block: V = J_d^2 + D_d, S = H_pp + D_p - sum (J_p^T J_d)(J_d J_p) / V,
 * rhs = -(g_p - sum J_p^T J_d J_d r / V), delta_d = -(J_d r + J_d J_p delta_p) / V.
 *
 * An image handle holds nothing else and lives on one GPU (ssba_stats.general_structure = 4; num_active_points and
 * num_observations = the block count).  SSBA_ERR_UNSUPPORTED with a message that names the call: pose, point, stereo,
 * lighting, pose-factor and constant-block calls on it, a second ssba_add_image_blocks, ssba_set_distributed /
 * ssba_set_partition / an exchange, a DOGLEG solve, ssba_evaluate, ssba_lm_step, ssba_dogleg_step, ssba_covariance_blocks.
 * rows or cols = 0, a NULL array, an unknown interpolation: SSBA_ERR_INVALID_ARGUMENT (so is a map without a usable disparity,
 * at ssba_finalize).  ssba_solve, the stepwise calls, ssba_iteration_log, ssba_set_stream, ssba_set_kernel_timing work as on
 * every handle.  ssba_pose_covariance(p, 0, cov) with constant disparities: the inverse of sum J_pose^T J_pose, of the corrected
 * rows J~_pose under a loss (SSBA_ERR_NUMERICAL_FAILURE when singular); with free disparities SSBA_ERR_NUMERICAL_FAILURE (more columns than rows: Ceres
 * reports a failed covariance computation there too). */
#define SSBA_IMAGE_NEAREST 0
#define SSBA_IMAGE_BILINEAR 1
SSBA_API int ssba_add_image_blocks(ssba_problem *p, double *pose, double *disparity, const double *ref_img, const double *track_img,
                          const double *track_gradx, const double *track_grady, uint32_t rows, uint32_t cols, int interpolation);
/* replaces problem.SetParameterBlockConstant / SetParameterBlockVariable on every disparity block (before ssba_finalize) */
SSBA_API int ssba_set_disparity_blocks_constant(ssba_problem *p, int is_constant);
/* test hook: one Levenberg-Marquardt step from the caller's current pose and disparities at the given radius.  cost; residuals
 * (rows * cols), J_pose (rows * cols * 6), J_disp (rows * cols): the rows, zero at pixels without a block; S (36) the damped
 * reduced 6 x 6 system and rhs (6); delta_pose (6), delta_disp (rows * cols, zero when constant); model_cost_change.  Any
 * output may be NULL.  Writes nothing back.  Under a loss (ssba_set_huber_loss) residuals, J_pose and J_disp are the corrected
 * rows r~, J~, cost is 1/2 sum rho(r^2), and S, rhs, delta_pose, delta_disp and model_cost_change are what the solver forms from
 * the corrected rows. */
SSBA_API int ssba_image_step(ssba_problem *p, const ssba_options *o, double radius, double *cost, double *residuals, double *J_pose,
                    double *J_disp, double *S, double *rhs, double *delta_pose, double *delta_disp, double *model_cost_change);

/* ---- dense photometric alignment: many handles in shared launches --------------------------------------------------------
 * A sequence of N stereo frames is N - 1 alignments that do not depend on each other, and one of the driver's size leaves the GPU
 * nearly idle.  ssba_image_solve_batch solves n finalized image handles together: one iteration of the whole batch is five
 * launches whatever n is (k_imb_lin . k_imb_solve . k_imb_eval . k_imb_decide . k_imb_best, the problem in blockIdx.y), members
 * that have terminated ride along as no-ops, and every member's result -- pose, disparity map, summary, iteration log -- is
 * bit-equal to ssba_solve on that handle alone: the batched kernels run the solo kernels' source (shared functions, every sum in
 * the same order, no atomics).  That equality is tested on the device (tests/test_gpu_image_batch.py), not guaranteed by the
 * language: a compiler may contract the same sum of two products differently in two kernels.
 * n = 1 has nothing to share and takes the solo path (ssba_solve, or the stepwise calls with ignore_convergence).
 * The buffers, events and captured graphs of a call stay on handles[0] and serve the next call with the same n and launch shapes;
 * they are released with that handle.
 *
 * The call: ssba_solve_begin on every handle (uploads, options, a reset trust-region state), the rounds, ssba_solve_end on every
 * handle, so pose and disparity of each caller are written back exactly as after ssba_solve.  It returns when every member has
 * terminated, or after max_num_iterations + 3 rounds as ssba_solve does.  ignore_convergence != 0: exactly max_num_iterations
 * rounds, i.e. ssba_solve_begin(.., 1) / ssba_solve_step(max_num_iterations) / ssba_solve_end on every member.
 * Stream: the shared launches run on handles[0]'s stream (ssba_set_stream), ordered behind the begin of every other handle by
 * events (hipStreamWaitEvent); that stream is synchronised before the ends.  The call is synchronous.
 * summaries (n) and statuses (n) may be NULL.  statuses[k] is what ssba_solve would have returned for handle k: SSBA_OK, or
 * SSBA_ERR_NUMERICAL_FAILURE when its minimiser ended without a usable solution (its blocks are then left as they were).  Such a
 * member does not stop the others.  The call returns the first non-zero status in handle order, or SSBA_OK.
 * minimizer_progress_to_stdout is ignored in a batch.
 * Refusals, each with a message (ssba_last_error) that names the call and the index of the offending handle; after a refusal
 * every handle is as it was:
 *   SSBA_ERR_INVALID_ARGUMENT  n = 0, a NULL entry, the same handle twice, handles on different devices,
 *                              n > SSBA_IMAGE_BATCH_MAX (the device array of the handles' states is 3.5 KB per member)
 *   SSBA_ERR_UNSUPPORTED       a handle without image blocks, a DOGLEG solve, a handle with kernel timing switched on
 *   SSBA_ERR_STATE             a handle that is not finalized, a handle inside a stepwise solve
 * Afterwards every handle is an ordinary handle again: ssba_solve, ssba_solve_restart (after a new ssba_solve_begin),
 * ssba_iteration_log and ssba_pose_covariance work on it. */
#define SSBA_IMAGE_BATCH_MAX 4096
SSBA_API int ssba_image_solve_batch(ssba_problem **handles, uint32_t n, const ssba_options *options, int ignore_convergence,
                           ssba_summary *summaries, int *statuses);

/* ---- dense photometric alignment: the driver's pre-processing and a coarse-to-fine solve ------------------------------
 * An image pyramid replaces tests/dense_stereo_test.cpp:52-72 (everything between imread / SGBM and the residual blocks): it is
 * built once from the raw 8-bit pair and one disparity map and holds every level in device memory.  Level 0 is the caller's
 * rows x cols image; level l is floor(rows / 2^l) x floor(cols / 2^l).
 *
 * The arithmetic:
 *     halving     cv::pyrDown(src, dst, Size(cols / 2, rows / 2)) on CV_8U as the driver calls it (:52-59), in integers:
 *                     dst[y][x] = (sum_{i,j=-2..2} w_i w_j src[2y+i][2x+j] + 128) >> 8,   w = [1 4 6 4 1],
 *                 border BORDER_REFLECT_101 (index -1 -> 1, -2 -> 2, n -> n-2, n+1 -> n-3); each level from the rounded 8-bit
 *                 level above it, as the driver's in-place calls do.
 *     conversion  I = (double)u8 * (1.0 / 255.0): one multiplication by that constant (convertTo(CV_64F, 1./255.), :62-64)
 *     gradients   the 3 x 3 Sobel on the converted image, BORDER_REFLECT_101, times gradient_scale, summed as synth.sobel sums:
 *                     gx = scale * (((p[y-1][x+1] - p[y-1][x-1]) + 2 (p[y][x+1] - p[y][x-1])) + (p[y+1][x+1] - p[y+1][x-1]))
 *                     gy = scale * (((p[y+1][x-1] - p[y-1][x-1]) + 2 (p[y+1][x] - p[y-1][x])) + (p[y+1][x+1] - p[y-1][x+1]))
 *                 gradient_scale 1 is cv::Sobel(img, out, -1, 1, 0) (:70-72); 0.125 gives per-pixel slopes.
 *                 SSBA_GRADIENT_OF_REFERENCE differentiates the reference image, which is what :70-72 does as it stands (under
 *                 its TODO); SSBA_GRADIENT_OF_TRACKED the tracked image, which is what the functor samples.
 *     disparity   the caller's map belongs to ONE level, disparity_level, in pixels of that level (the driver runs SGBM after two
 *                 halvings: 2).  Coarser levels: d_{l+1}[y][x] = d_l[2y][2x] / 2; invalid entries (NaN, +-inf, <= 0) stay
 *                 invalid.  Finer levels have no map and cannot be aligned.
 *     camera      of level l from a level-0 camera: fu / 2^l, fv / 2^l, cu / 2^l, cv / 2^l, b (pyrDown samples at even pixels,
 *                 so u_l = u / 2^l exactly).  The reference driver keeps the full-resolution intrinsics at level 2 (:22-27
 *                 against :52-59); a caller who wants that hands its own camera to the handle.  The pyramid forces none.
 *
 * create: the work runs on the pyramid's own stream and is complete on return; device memory comes from the library's pool.
 *   SSBA_ERR_INVALID_ARGUMENT: a NULL array, levels = 0, disparity_level >= levels, an unknown gradient source, a non-finite or
 *   zero gradient_scale, a level with fewer than 8 rows or columns.  SSBA_ERR_NO_DEVICE as for a problem handle.
 * level: downloads whichever outputs are not NULL (rows * cols of that level each); the disparity exists for
 *   level >= disparity_level only (SSBA_ERR_INVALID_ARGUMENT when asked for below it).
 * ssba_add_image_level: ssba_add_image_blocks with the four images of a level.  pose (12) and disparity (rows * cols of the level)
 *   are caller-owned and updated in place, exactly as there; the blocks are the finite positive entries of the CALLER's map at
 *   ssba_finalize.  ssba_finalize copies the images device to device into the handle's own buffers: the pyramid must live until
 *   then and may be destroyed afterwards, and no image crosses the host.  Refusals as ssba_add_image_blocks, plus
 *   SSBA_ERR_INVALID_ARGUMENT when the handle's device differs from the pyramid's or level < disparity_level.
 * align: coarse to fine.  For l = coarsest_level ... disparity_level: a handle with camera0 scaled to l on the level, a
 *   Levenberg-Marquardt solve with `options`, the pose carried to the next level.  Levels above disparity_level hold their derived
 *   disparities constant (free, they absorb the motion and the pose never moves) and leave no trace in the caller's map; the base
 *   level follows disparities_constant and updates `disparity` (the map at disparity_level) in place.  summaries (may be NULL)
 *   has coarsest_level - disparity_level + 1 entries; summaries[coarsest_level - l] is level l's.  A level that ends without a
 *   usable solution stops the loop and returns its status; the pose is then the last usable one.
 * ssba_image_pyramid_set_huber_loss: the width a that align and align_batch give every level's handle (ssba_set_huber_loss on
 *   it); a <= 0, the state after create, is the NULL loss.  One width serves all levels: intensities do not scale with the
 *   level.  The pyramids of one align_batch may differ in it. */
typedef struct ssba_image_pyramid ssba_image_pyramid;
#define SSBA_GRADIENT_OF_REFERENCE 0
#define SSBA_GRADIENT_OF_TRACKED 1
SSBA_API int ssba_image_pyramid_create(const uint8_t *ref_u8, const uint8_t *track_u8, const double *disparity, uint32_t rows, uint32_t cols,
                              uint32_t levels, uint32_t disparity_level, int gradient_source, double gradient_scale, int device,
                              ssba_image_pyramid **out);
SSBA_API int ssba_image_pyramid_destroy(ssba_image_pyramid *pyr);
SSBA_API int ssba_image_pyramid_level(ssba_image_pyramid *pyr, uint32_t level, uint32_t *rows, uint32_t *cols, uint8_t *ref_u8, uint8_t *track_u8,
                             double *ref, double *track, double *gradx, double *grady, double *disparity);
SSBA_API int ssba_add_image_level(ssba_problem *p, ssba_image_pyramid *pyr, uint32_t level, double *pose, double *disparity, int interpolation);
SSBA_API int ssba_image_pyramid_set_huber_loss(ssba_image_pyramid *pyr, double a);
SSBA_API int ssba_image_pyramid_align(ssba_image_pyramid *pyr, const ssba_camera *camera0, double *pose, double *disparity, uint32_t coarsest_level,
                             int interpolation, int disparities_constant, const ssba_options *options, ssba_summary *summaries);
/* align_batch: coarse to fine over n pyramids in lockstep (the pairs of a sequence).  Per level one handle per pyramid, built
 *   exactly as ssba_image_pyramid_align builds it, and ONE ssba_image_solve_batch; every pyramid's pose, map and summaries are
 *   bit-equal to ssba_image_pyramid_align on it alone.  poses: n x 12; disparities: n caller-owned maps at disparity_level, updated
 *   in place as there; summaries (may be NULL): n x (coarsest_level - disparity_level + 1), pyramid-major, each row laid out as the
 *   solo call's, zero where a level was not solved; statuses (may be NULL): n.  Image sizes may differ between the pyramids.
 *   A pyramid whose level ends without a usable solution (or cannot be set up: no usable disparity on a level) keeps its last
 *   usable pose, drops out of the finer levels and gets that status; the others go on.  Returns the first non-zero status in
 *   pyramid order, or SSBA_OK.  SSBA_ERR_INVALID_ARGUMENT (nothing is touched): n = 0 or above SSBA_IMAGE_BATCH_MAX, a NULL entry,
 *   pyramids that differ in device or disparity_level, a pyramid without coarsest_level, coarsest_level < disparity_level, an
 *   unknown interpolation.  SSBA_ERR_UNSUPPORTED: DOGLEG. */
SSBA_API int ssba_image_pyramid_align_batch(ssba_image_pyramid **pyramids, uint32_t n, const ssba_camera *camera0, double *poses, double **disparities,
                                   uint32_t coarsest_level, int interpolation, int disparities_constant, const ssba_options *options,
                                   ssba_summary *summaries, int *statuses);

/* ---- dense photometric alignment: the disparity map from a rectified pair ------------------------------------------------
 * ssba_stereo_sgbm replaces cv::StereoSGBM sgbm(0, 64, 15); sgbm(left0, right0, disp0) (tests/dense_stereo_test.cpp:61-65): a
 * semi-global matcher (Hirschmueller 2008) in the single-pass, five-direction mode that call uses, stated here entirely in
 * integers.  cv::StereoSGBM cannot be compiled or run where this library is built and tested, so bit parity with OpenCV is
 * UNPINNED; the yardstick is the numpy statement tests/sgbm_reference.py, which the device equals to the bit.
 *
 * left, right: rectified 8-bit images, rows x cols, row-major.  D = num_disparities, maxD = min_disparity + D.  The computable
 * columns are x in [maxD, cols), W of them; every other pixel is invalid.  Derived constants:
 *     cap = max(pre_filter_cap, 15) | 1,  P1 = p1 > 0 ? p1 : 2,  P2 = max(p2 > 0 ? p2 : 5, P1 + 1),  r = block_size / 2
 * The arithmetic:
 *     pre-filter  on both images:  g = (I[y-1][x+1] - I[y-1][x-1]) + 2 (I[y][x+1] - I[y][x-1]) + (I[y+1][x+1] - I[y+1][x-1]),
 *                 rows reflected (-1 -> 1, rows -> rows - 2), g = 0 in columns 0 and cols - 1;  P = clamp(g, -cap, cap) + cap
 *     pixel cost  Birchfield-Tomasi of a row signal A (left, at x) against B (right, at x - d):
 *                     a- = (A[x] + A[x-1]) / 2,  a+ = (A[x] + A[x+1]) / 2   (floor division, the neighbour clamped to the row)
 *                     amin / amax = the minimum / maximum of A[x], a-, a+;  B likewise at x - d
 *                     c0 = max(0, a - bmax, bmin - a),  c1 = max(0, b - amax, amin - b),  BT = min(c0, c1)
 *                 c(x, y, d) = BT(P_left, P_right) + (BT(left, right) >> 2)
 *     block cost  C(x, y, d) = sum_{i,j=-r..r} c(x + i, y + j, d), rows clamped to [0, rows), columns to the computable range.
 *                 C <= (2 cap + 63) block_size^2: 93 block_size^2 at the default cap, 20 925 at block size 15.
 *     paths       for the predecessors q = (x-1, y), (x+1, y), (x-1, y-1), (x, y-1), (x+1, y-1) of p:
 *                     L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + P1, L(q, d+1) + P1, m(q) + P2) - m(q),  m(q) = min_k L(q, k)
 *                 d -+ 1 outside [min_disparity, maxD) does not take part; L(p, d) = C(p, d) where q lies outside the computable
 *                 columns or above row 0.  L <= C + P2 fits 16 bits.  S = the sum of the five L (more than 16 bits).
 *     winner      d* = argmin_d S, the smallest d on ties.  Uniqueness: invalid if some d with |d - d*| > 1 has
 *                 S(d) (100 - uniqueness_ratio) < S(d*) 100.  Sub-pixel, where d* is neither the first nor the last disparity:
 *                     den = max(S(d*-1) + S(d*+1) - 2 S(d*), 1)
 *                     disp16 = 16 d* + ((S(d*-1) - S(d*+1)) 16 + den) / (2 den)      (C's truncating division)
 *                 elsewhere disp16 = 16 d*.
 *     left-right  when disp12_max_diff >= 0; a NEGATIVE value switches the check off (this library's own rule).  Per row the
 *                 right view's map: for x from the last computable column down to the first, of the pixels that passed
 *                 uniqueness, x2 = x - d*(x); if S(x, d*) < cost2[x2] strictly, cost2[x2] = S(x, d*) and disp2[x2] = d* (ties
 *                 keep the larger x).  Then for every valid pixel lo = disp16 >> 4, hi = (disp16 + 15) >> 4, a = x - lo,
 *                 b = x - hi; it becomes invalid if BOTH hold: 0 <= a < cols, disp2[a] >= min_disparity and
 *                 |disp2[a] - lo| > disp12_max_diff; the same three conditions for b against hi.
 *     outputs     disp16 (int16, rows * cols): invalid pixels hold (min_disparity - 1) * 16.  disparity (double, rows * cols):
 *                 disp16 / 16.0 where valid, NaN elsewhere.  (The driver's convertTo(CV_64F, 1./16.) gives -1 at an invalid pixel
 *                 for min_disparity 0; its test isfinite(d) && d > 0 drops -1 and NaN alike, and NaN stays dropped for any
 *                 min_disparity.)
 * SSBA_ERR_INVALID_ARGUMENT: a NULL image or parameter block, min_disparity < 0, num_disparities not a multiple of 16 in
 *   16 ... 256, block_size not odd in 1 ... 15, uniqueness_ratio outside 0 ... 100, pre_filter_cap > 127 (P no longer fits
 *   8 bits), full_dp (the eight-direction mode), rows < 2, cols <= maxD (no computable column), maxD > 2047 (disp16 overflows),
 *   (2 cap + 63) block_size^2 + P2 > 65535 (a path cost would not be exact in 16 bits).
 * SSBA_ERR_UNSUPPORTED: nonzero speckle_window_size or speckle_range (no connected-components filter), more than 5461 columns
 *   or 2^31 volume entries rows * W * D.
 * ssba_stereo_sgbm is synchronous: host arrays in and out (either output may be NULL), the work on a pooled stream, the memory
 * (six 16-bit volumes of rows * W * D) from the library's pool.  ssba_sgbm_default_params: the driver's (0, 64, 15), zeros
 * for the rest.
 *
 * ssba_image_pyramid_create_stereo is ssba_image_pyramid_create without a disparity argument: the right image is halved down to
 * disparity_level like the other two, the matcher runs there on the two 8-bit levels (the state in which the driver calls it,
 * :52-64), and its double map is the pyramid's map at disparity_level, from which the coarser levels derive as ever.  No
 * disparity crosses the host.  A handle's blocks are the finite positive entries of the CALLER's map: download it once with
 * ssba_image_pyramid_level and hand it to ssba_add_image_level or ssba_image_pyramid_align.  Refusals: those of
 * ssba_image_pyramid_create and of ssba_stereo_sgbm at the size of disparity_level. */
typedef struct {
    int32_t min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap, uniqueness_ratio;
    int32_t speckle_window_size, speckle_range, full_dp;
} ssba_sgbm_params;
SSBA_API void ssba_sgbm_default_params(ssba_sgbm_params *params);
SSBA_API int ssba_stereo_sgbm(const uint8_t *left, const uint8_t *right, uint32_t rows, uint32_t cols, const ssba_sgbm_params *params, int device,
                     int16_t *disp16_out, double *disparity_out);
SSBA_API int ssba_image_pyramid_create_stereo(const uint8_t *ref_left_u8, const uint8_t *ref_right_u8, const uint8_t *track_u8, uint32_t rows,
                                     uint32_t cols, uint32_t levels, uint32_t disparity_level, const ssba_sgbm_params *params,
                                     int gradient_source, double gradient_scale, int device, ssba_image_pyramid **out);

/* ---- stereo sequences: every frame prepared once, the matcher batched over the pairs ---------- */
/* ssba_stereo_sgbm_batch is ssba_stereo_sgbm over n pairs of one size: left and right hold n images of rows x cols each, one
 * after the other; disp16_out and disparity_out (either may be NULL) receive n maps in the same order.  Member k is bit-equal
 * to the solo call on pair k: the kernels are the solo kernels' bodies with the pair as one more grid dimension, integer
 * throughout.  Both image stacks go up in one copy each and the maps come down in one.
 * workspace_bytes bounds the matcher's volumes, 12 bytes per (row, computable column, disparity) and pair, i.e.
 * 12 * rows * (cols - min_disparity - num_disparities) * num_disparities bytes per pair: the pairs are processed in chunks of
 * as many pairs as fit (at most 65535), five launches per chunk on one stream.  0 stands for the library's default,
 * SSBA_SGBM_DEFAULT_WORKSPACE_BYTES = 1 GiB: a choice, half of what the pool caches by default, so that a long sequence
 * neither holds the device's memory nor loses its buffers between calls.  The per-pixel arrays and the images are not counted.
 * Refusals: every one of ssba_stereo_sgbm with the same status, before a device is looked for; SSBA_ERR_INVALID_ARGUMENT also
 * for n = 0 and for a workspace_bytes below one pair's volumes (the message names the bytes needed).
 *
 * ssba_image_sequence_create prepares F = frames rectified stereo frames of one size for the F - 1 alignments of consecutive
 * left frames: pair k has reference left_k, tracked left_(k+1) and the disparities of (left_k, right_k).  left holds F images,
 * right F - 1 at least (frames 0 ... F - 2; only those are read).  Every image goes up once, in one copy.  Per left frame all
 * levels are built once: the 8-bit image, the double image and both Sobel images (the arithmetic of ssba_image_pyramid_create);
 * per right frame the 8-bit levels down to disparity_level.  The matcher runs over the F - 1 pairs at disparity_level as
 * ssba_stereo_sgbm_batch does under workspace_bytes, its double maps stay on the device, and the coarser maps follow by the
 * rule above.  One level of all frames is one launch of each kind: 2 levels + 4 launches in all while the pairs fit one chunk,
 * whatever F, and one synchronisation.  Refusals: those of ssba_image_pyramid_create_stereo and of ssba_stereo_sgbm_batch at the
 * size of disparity_level, frames < 2, frames > 32768.
 * ssba_image_sequence_pyramid hands out the pyramid of pair k < F - 1, bit-equal in every level and image to
 * ssba_image_pyramid_create_stereo on left_k, right_k, left_(k+1) (gradients of frame k or k + 1 according to gradient_source).
 * It is BORROWED: its levels point into the sequence's buffers and it owns no device memory.  Every pyramid call takes it
 * (level, add_image_level, set_huber_loss, align, align_batch) except ssba_image_pyramid_destroy, which refuses it with
 * SSBA_ERR_INVALID_ARGUMENT and leaves it usable; it ends with the sequence and must not be touched afterwards.  A handle that
 * was finalized from one of its levels holds copies of the images and outlives the sequence.  The same k gives the same pointer.
 * ssba_image_sequence_destroy frees the sequence and its borrowed pyramids. */
#define SSBA_SGBM_DEFAULT_WORKSPACE_BYTES (1ull << 30)
typedef struct ssba_image_sequence ssba_image_sequence;
SSBA_API int ssba_stereo_sgbm_batch(const uint8_t *left, const uint8_t *right, uint32_t n, uint32_t rows, uint32_t cols,
                           const ssba_sgbm_params *params, uint64_t workspace_bytes, int device, int16_t *disp16_out, double *disparity_out);
SSBA_API int ssba_image_sequence_create(const uint8_t *left, const uint8_t *right, uint32_t frames, uint32_t rows, uint32_t cols, uint32_t levels,
                               uint32_t disparity_level, const ssba_sgbm_params *params, uint64_t workspace_bytes, int gradient_source,
                               double gradient_scale, int device, ssba_image_sequence **out);
SSBA_API int ssba_image_sequence_pyramid(ssba_image_sequence *seq, uint32_t k, ssba_image_pyramid **out);
SSBA_API int ssba_image_sequence_destroy(ssba_image_sequence *seq);

/* ---- front end: the VO initial guess --------------------------------- */
/* ssba_frontend_ransac replaces, for `num_pairs` pairs of consecutive states at once,
 *   PointCloudAligner::compute_transformation_and_inliers (src/ceres_slam/point_cloud_aligner.cpp:64-136)
 * as compute_initial_guess calls it (src/ceres_slam/dataset_problem.cpp:246-249: 400 iterations, threshold 4;
 * dataset_problem_phong.cpp:346-348: threshold 9).  Pair p owns the matched points
 * [offset[p], offset[p+1]) of pts0 / pts1 (camera-frame points from StereoCamera::triangulate, 3 doubles each,
 * paired by position as the reference pairs them); samples = num_pairs * num_iters * 3 indices local to the
 * pair; thresh bounds the squared stereo reprojection error (:117-124).  Outputs: T (num_pairs * 12,
 * [t | R row-major] = T_1_0 of the hypothesis with the most inliers, the first one on ties, identity when no
 * hypothesis has an inlier), inlier flags (one byte per matched point; may be NULL), count (num_pairs; may be
 * NULL), device_time_s (kernel time; may be NULL).
 * ssba_ransac_samples (host) restates the reference's draw sequence (:69-91): std::mt19937 re-seeded with 42 in
 * every call and std::uniform_int_distribution<uint>(0, n-1), three distinct indices per iteration.  The
 * distribution is implementation-defined; libstdcxx_variant 1 = libstdc++ >= 11, 0 = libstdc++ <= 10. */
/* ssba_frontend_vo: the WHOLE DatasetProblem::compute_initial_guess(k1, k2) (src/ceres_slam/dataset_problem.cpp:179-270) on the
 * device for `num_states` consecutive states: reciprocal matches of every pair of consecutive states by landmark id
 * (:209-222; both lists in their state's order, paired by position), StereoCamera::triangulate of the matches
 * (:225-230), the num_iters-hypothesis 3-point RANSAC of ALL pairs (one lane per alignment, one workgroup per inlier count;
 * the draws are the reference's: std::mt19937(42) + uniform_int_distribution, libstdcxx_variant as for
 * ssba_ransac_samples), pose chaining poses[k] = T_k_km1 * poses[k-1] (:255) and the map initialisation from the inliers
 * of the first pair that sees a landmark (:259-269).  Observations of state k are the entries
 * [state_start[k], state_start[k+1]) of point_id / uvd (3 per observation).  poses: num_states x 12, poses[0] is the input;
 * map_points (num_points x 3) and initialized (num_points flags) are updated for newly initialised landmarks only.
 * match_count / inlier_count (num_states - 1; may be NULL).  SSBA_ERR_NUMERICAL_FAILURE: a pair has fewer than 3 matches. */
SSBA_API int ssba_frontend_vo(const ssba_camera *camera, int device, uint32_t num_states, const uint32_t *state_start,
                     const uint32_t *point_id, const double *uvd, uint32_t num_points, uint32_t num_iters, double thresh,
                     int libstdcxx_variant, double *poses, double *map_points, uint8_t *initialized, uint32_t *match_count,
                     uint32_t *inlier_count, double *device_time_s);
SSBA_API int ssba_ransac_samples(uint32_t n, uint32_t num_iters, int libstdcxx_variant, uint32_t *idx3);
SSBA_API int ssba_frontend_ransac(const ssba_camera *camera, int device, uint32_t num_pairs, const uint32_t *offset,
                         const double *pts0, const double *pts1, const uint32_t *samples, uint32_t num_iters,
                         double thresh, double *T, uint8_t *inlier, uint32_t *count, double *device_time_s);

SSBA_API const char *ssba_status_string(int status);
SSBA_API const char *ssba_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SSBA_H_ */
