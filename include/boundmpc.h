/*
 * boundmpc.h -- C ABI of libboundmpc_hip.so, the MI355X-native drop-in for the NLP solve of
 * BoundMPC's receding-horizon step.
 *
 * Reference interface replaced (all paths relative to /root/reference):
 *   bound_planner/BoundMPC/BoundMPC.py:594-603    sol = self.solver(x0=w0, lbx=lbx, ubx=ubx,
 *                                                 lbg=self.lbg, ubg=self.ubg, p=params)
 *   bound_planner/BoundMPC/BoundMPC.py:604-617    sol["x"], sol["g"], solver.stats()
 *   bound_planner/BoundMPC/BoundMPC.py:240-246    solver construction (setup_optimization_problem)
 *   bound_planner/RobotModel/RobotModel.py:146-267 fk_pos, fk_pos_col, hom_transform_endeffector,
 *                                                 jacobian_fk (the numeric Pinocchio path)
 * Vector layouts are the reference's own: decision vector w (44N+6, variable-major/time-minor,
 * casadi_ocp_formulation.py:89-101), parameter vector p (875, :383-415), constraint vector g
 * (147(N-1)+21, :106-380).  All host arrays are row-major [instance][index], FP64.
 *
 * Plain C, plain pointers and sizes; no torch/HIP types in the signatures (the `_dev` entry
 * takes a hipStream_t as void*).  A handle is not thread-safe; use one per host thread/stream.
 * Return value: 0 on success, nonzero on API misuse or a HIP error (see bmpc_last_error); 4 = the handle is busy with a
 * solve started from another host thread (nothing was done).
 */
#ifndef BOUNDMPC_H
#define BOUNDMPC_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmpc_handle bmpc_handle;

typedef struct {
    int N;              /* horizon; reference default 15 (utils/util_functions.py:49) */
    int nr_segs;        /* must be 4 (utils/util_functions.py:49) */
    double dt;          /* 0.1 */
    double tol;         /* IPOPT "tol": 10e-6 = 1e-5 (BoundMPC.py:203) */
    int max_iter;       /* IPOPT "max_iter": 100 (BoundMPC.py:204) */
    int device;         /* HIP device ordinal */
    int hess;           /* 0 Gauss-Newton Hessian, 2 hybrid (second-order kinematic terms) */
    double hess_switch; /* hess==2: the exact Lagrangian Hessian (second-order kinematic and sigmoid terms) is tried once the KKT
                           error of the previous iterate is below this (default 1.0) */
    double mu_init, kappa_mu, theta_mu, kappa_eps; /* monotone barrier schedule */
    double mu_floor_k;  /* a barrier decrease stops at (scaled KKT error) / mu_floor_k (default 1e4; 0 = no floor) */
    int inertia;        /* exact Hessian not positive definite on the null space of the dynamics: 0 Gauss-Newton fallback,
                           1 IPOPT's inertia correction (delta_w I added, escalated), 2 (default) Gauss-Newton fallback while
                           the previous KKT error is above inertia_err and the error improved within the last stall_n
                           iterations, inertia correction otherwise */
    double dw0;         /* first delta_w (IPOPT delta_w^0 = 1e-4) */
    double inertia_err; /* 1e-2 */
    int stall_n;        /* 8 */
    int slack_reset;    /* 1 (default): a trial slack is never below the value that closes its row at the trial point,
                           t <- max(t + alpha dt, -h(trial)) (Byrd-Hribar-Nocedal slack reset); 0: off */
    double ls_alpha_mem; /* 0 (default): the filter line search always starts at the fraction-to-boundary length (IPOPT); m > 0: at
                           min(that, m x the step length the previous iteration ended with) -- fewer rejected trials on iterates that
                           crawl, measured neutral on configs[2] and +5 % on configs[4] with m = 4 */
    int gn_backoff;     /* 2: after a Gauss-Newton fallback the exact Hessian is tried again after 1, then 2 iterations
                           (a failed attempt costs a Riccati sweep); 0: every iteration */
    int trial_repeats;  /* 9 (default): a rejected line-search trial is repeated (half the step length) up to this many times by the
                           wavefront that evaluated it (bmpc_k_trial holds all pairs of its instances, so it runs the filter test
                           itself): the whole line search of an iteration in one super-step.  0: one trial per super-step
                           (rounds 1-2).  Scheduling only, results do not depend on it (bitwise) */
    int watchdog_ms;    /* > 0 (default 30000): a wait for the GPU gives up after this long and the call returns 5 with a message
                           (the handle is unusable afterwards: every entry point returns 5, and bmpc_destroy neither waits for the
                           stream nor frees device memory that queued kernels may still write -- it leaks them; end the process
                           with an error and let a fresh one take over); 0: plain hipStreamSynchronize */
    int max_batch;      /* capacity hint for host-pointer calls (device staging buffers) */
    int pool_slots;     /* 0 (default) = every instance of a call has its own workspace slot; > 0 = the workspace
                           holds this many instances and a call with more of them STREAMS them through it: a slot whose
                           instance has finished takes the next one, so a long call keeps the GPU on ~pool_slots instances
                           and pays a single straggler tail.  Results do not depend on it (bitwise). */
} bmpc_opts;

void bmpc_default_opts(bmpc_opts* o, int N);

/* Kinematic table of a 7-joint serial arm in the frame conventions of RobotModel.py:15-54: revolute joints about their
 * local z axes with the URDF <origin xyz rpy> of joint_1..joint_7 (fixed rotation R = Rz(yaw) Ry(pitch) Rx(roll)), the fixed
 * joints to end_effector_link and link4_col_link (child of joint_4's link), URDF limits, BoundMPC.py:171-191 acceleration /
 * jerk limits and the collision-sphere radii col_joint_sizes (RobotModel.py:37-40).  The six collision points are the
 * origins of joint_3..joint_7 and link4_col_link (RobotModel.py:27-35).  Infinite joint limits: +-1e20. */
typedef struct {
    double joint_xyz[7][3], joint_rpy[7][3];
    double ee_xyz[3], ee_rpy[3];
    double link4_col_xyz[3];
    double q_lower[7], q_upper[7], dq_max[7];
    double ddq_max, u_max;
    double col_joint_sizes[7];
} bmpc_robot;
void bmpc_robot_iiwa14(bmpc_robot* r);   /* RobotModel/iiwa.urdf (USE_IIWA = True, the default; RobotModel.py:10) */
void bmpc_robot_gen3(bmpc_robot* r);     /* RobotModel/gen3_arm.urdf (USE_IIWA = False): Kinova Gen3, joints 1/3/5/7 unlimited */

/* replaces setup_optimization_problem(...) + nlpsol construction (BoundMPC.py:240-246) */
int bmpc_create(const bmpc_opts* o, bmpc_handle** h);
void bmpc_destroy(bmpc_handle* h);
const char* bmpc_last_error(const bmpc_handle* h);

/* n_w = 44N+6, n_g = 147(N-1)+21, n_p = 875 */
int bmpc_dims(const bmpc_handle* h, int* n_w, int* n_g, int* n_p);

/* the handle's own HIP stream (a hipStream_t): the one bmpc_solve, bmpc_solve_dev_async and the device loop run on */
void* bmpc_stream(bmpc_handle* h);

/* Robot of the handle (default: iiwa14).  bmpc_set_robot must precede the solves / device loops that are to use it. */
int bmpc_set_robot(bmpc_handle* h, const bmpc_robot* r);
int bmpc_get_robot(const bmpc_handle* h, bmpc_robot* r);

/* the options the handle was created with */
int bmpc_get_opts(const bmpc_handle* h, bmpc_opts* o);

/* constant constraint bounds (self.lbg / self.ubg, casadi_ocp_formulation.py:145-380);
 * infinities are returned as +-1e20 */
int bmpc_gbounds(const bmpc_handle* h, double* lbg, double* ubg);

/* B independent solves = B calls of self.solver(...) (BoundMPC.py:594-603).  Host pointers.
 * x0/lbx/ubx/x: [B][n_w]; p: [B][875]; g: [B][n_g] or NULL; lam_g: [B][n_g] or NULL; lam_x: [B][n_w] or
 * NULL -- sol["lam_g"], sol["lam_x"] (BoundMPC.py:638-645) in CasADi's convention: grad f + J_g^T lam_g + lam_x = 0,
 * positive at an active upper bound, negative at an active lower bound; the entries of the variables that are fixed
 * by lbx == ubx follow from stationarity (IPOPT fixed_variable_treatment=make_parameter).  On a handle created with
 * pool_slots > 0 the multipliers need B <= pool_slots (a streamed call keeps no final iterates): otherwise the call is refused
 * up front with return code 1.
 * f/viol: [B]; iters/status: [B].
 * status: 0 converged, 1 max_iter, 2 stalled, 3 numerical.  viol = sum of constraint
 * violations exactly as BoundMPC.py:613-615, so the caller reproduces
 * `success = stats["success"] or g_viol < 1e-4`.  Infinite bounds may be passed as +-inf or
 * +-1e20. */
int bmpc_solve(bmpc_handle* h, int B, const double* x0, const double* lbx, const double* ubx,
               const double* p, double* x, double* g, double* lam_g, double* lam_x, double* f,
               int* iters, int* status, double* viol);

/* Same with DEVICE pointers; all work is enqueued on `stream` (a hipStream_t).  The call returns
 * when the batch is solved: the interior-point iteration count is data dependent, so the host
 * polls the number of unfinished instances between bursts of launches.  On return `stream`
 * has been synchronised: the outputs are complete and the handle's workspace is free for the next call
 * (on any stream).  A solve started with bmpc_solve_dev_async is waited for first. */
int bmpc_solve_dev(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx,
                   const double* d_ubx, const double* d_p, double* d_x, double* d_g, double* d_f,
                   int* d_iters, int* d_status, double* d_viol, void* stream);

/* Multipliers lam_g [B][n_g], lam_x [B][n_w] (device pointers) of the most recent finished solve on this handle (any
 * entry point): the final iterate stays in the handle's workspace until the next solve.  Enqueued on
 * `stream` and waited for. */
int bmpc_multipliers_dev(bmpc_handle* h, int B, double* d_lam_g, double* d_lam_x, void* stream);

/* Asynchronous form: returns at once, the solve runs on the handle's own stream driven by a worker
 * thread; inputs must already be complete on the device.  One solve in flight per handle;
 * bmpc_wait() blocks until it has finished and returns its status.  Two handles used alternately
 * overlap the straggler tail of one batch with the bulk of the next (bench.py). */
int bmpc_solve_dev_async(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx,
                         const double* d_ubx, const double* d_p, double* d_x, double* d_g, double* d_f,
                         int* d_iters, int* d_status, double* d_viol);
int bmpc_wait(bmpc_handle* h);
/* unfinished instances of the solve in flight on this handle (0 when idle) */
int bmpc_active(bmpc_handle* h);

/* Batched kinematics (RobotModel.py:146-267): ee_pos [B][3], ee_rot [B][9] row-major,
 * col_pts [B][18] (joint_3..joint_7 origins, link4_col_link), jac [B][42] (6x7 geometric,
 * LOCAL_WORLD_ALIGNED), dvdq [B][42] = d(J dq)/dq.  Host pointers; outputs may be NULL. */
int bmpc_fk(bmpc_handle* h, int B, const double* q, const double* dq, double* ee_pos,
            double* ee_rot, double* col_pts, double* jac, double* dvdq);

/* Batched inverse kinematics: the problem of RobotModel.inverse_kinematics (RobotModel.py:79-144),
 *   minimise_q |p_ee(q) - pd|^2 + |R_ee(q) rd^T - I|_F^2   subject to lo <= q <= hi,
 * for B independent targets on the handle's robot (bmpc_set_robot), solved by a projected Levenberg-Marquardt method with n_seeds
 * starts per target (a power of two in [1, 64]): seed 0 is q0, seed s >= 1 is point s of the 7-D Halton sequence (bases 2..17)
 * mapped onto the box (lo + h (hi - lo); q0 + (2h - 1) pi on unlimited joints); the best seed by (status != 0, cost, index) is
 * returned.  Host pointers: pd [B][3], rd [B][9] row-major (the user's matrix as passed), q0 [B][7]; lo / hi [B][7] or NULL = the
 * robot's limits (+-1e20: unlimited).  Outputs q [B][7] (inside [lo, hi] exactly), cost [B], pos_err = |pd - p_ee(q)| [B],
 * rot_err = |rotvec(R_ee(q) rd^T)| [B] (rad), iters [B] (trials, accepted or rejected), status [B] (0 converged: cost <= tol_cost
 * or projected gradient <= tol_grad, 1 max_iter, 2 stalled, 3 numerical: a non-finite input, cost or step, or lo > hi), seed [B]
 * (index of the winning start); any output but q may be NULL.  o == NULL: bmpc_default_ik_opts.  Return value: 0; 1 misuse
 * (n_seeds, a null required pointer, B < 0, lambda0 <= 0; B == 0 does nothing), 4 the handle is busy (an asynchronous solve in
 * flight), 5 the watchdog fired (the wait for the result uses bmpc_opts.watchdog_ms as bmpc_solve does). */
typedef struct {
    double tol_cost;    /* 1e-20 */
    double tol_grad;    /* 1e-10: |P(q - grad J) - q|_inf, P = projection onto [lo, hi] */
    double lambda0;     /* first Levenberg-Marquardt damping, 1e-3 */
    int max_iter;       /* 500 (the reference's IPOPT max_iter) */
} bmpc_ik_opts;
void bmpc_default_ik_opts(bmpc_ik_opts* o);
int bmpc_ik(bmpc_handle* h, int B, int n_seeds, const bmpc_ik_opts* o, const double* pd, const double* rd, const double* q0,
            const double* lo, const double* hi, double* q, double* cost, double* pos_err, double* rot_err, int* iters,
            int* status, int* seed);
/* Same with DEVICE pointers, enqueued on `stream` (a hipStream_t); returns without waiting. */
int bmpc_ik_dev(bmpc_handle* h, int B, int n_seeds, const bmpc_ik_opts* o, const double* d_pd, const double* d_rd,
                const double* d_q0, const double* d_lo, const double* d_hi, double* d_q, double* d_cost, double* d_pos_err,
                double* d_rot_err, int* d_iters, int* d_status, int* d_seed, void* stream);

/* Batched convex free-space sets of the plan phase (boundplanner_amd/convex_set_finder.py, reference ConvexSetFinder.py):
 *   point mode:   the set of find_set_around_point(p0[k], fixed_mid, optimize) -- polyhedron growth around the seed in the metric of
 *                 a maximum-volume inscribed ellipsoid, at most 5 rounds, until the ellipsoid's volume changes by less than 1 %;
 *   segment mode: the set of find_set_collision_avoidance(p0[k], p1[k], compute_ellipsoid=True).
 * One GPU thread per instance; an instance's result does not depend on B or on its position in the batch.
 * Scene (host pointers): n_obs <= 32 obstacle polytopes {x: A x <= b}: obs_A [n_obs][15][3], obs_b [n_obs][15] (rows beyond
 * obs_nrows[o] <= 15 are ignored), their vertices obs_V [n_obs][32][3] (obs_nv[o] in [1, 32] used); the workspace box e_min [3],
 * e_max [3].  Seeds p0 [B][3]; segment mode also p1 [B][3].
 * Outputs: A [B][20][3], b [B][20] (rows 0-5 the workspace box +x, -x, +y, -y, +z, -z, then the separating halfspaces nearest first;
 * rows past nrows are zero), nrows [B], q_ellipse [B][9] (the host's q_ellipse: the inverse of L L^T of the ellipsoid
 * {centre + L u: |u| <= 1}; with optimize = 0 the initial 1e4 I), centre [B][3], rounds [B] (polyhedra grown; 1 in segment mode),
 * newton [B] (Newton steps of the ellipsoid solves), collision [B] (segment mode: the segment touches an obstacle), status [B]:
 *   0 ok;
 *   1 the nearest obstacle is closer than 0.99 in the ellipsoid's metric (the seed lies in or on an obstacle: the host raises
 *     "Ellipse violates constraints");
 *   2 the set would need more than 20 rows (nothing truncated: the instance has no set);
 *   3 no strictly interior point for the ellipsoid (a fixed centre or seed outside the workspace box, or an empty set);
 *   4 numerical: a non-finite seed, or a Newton system that is not positive definite.
 * On status != 0, nrows is 0 and the rows are not meaningful.  rounds, newton and collision may be NULL.  o == NULL:
 * bmpc_default_sets_opts.  Return value: 0; 1 misuse (a null required pointer, B < 0, n_obs, row or vertex counts out of range;
 * B == 0 does nothing), 4 the handle is busy (an asynchronous solve in flight), 5 the watchdog fired (the wait uses
 * bmpc_opts.watchdog_ms as bmpc_solve does). */
typedef struct {
    int segment;        /* 0: point mode (default), 1: segment mode (p1 required) */
    int fixed_mid;      /* point mode: ellipsoids centred at the seed, a free-centre ellipsoid at the end (find_set_around_point) */
    int optimize;       /* point mode: 0 returns the first polyhedron (around the 1e-2 ball), default 1 */
} bmpc_sets_opts;
void bmpc_default_sets_opts(bmpc_sets_opts* o);
int bmpc_convex_sets(bmpc_handle* h, const bmpc_sets_opts* o, int n_obs, const double* obs_A, const double* obs_b, const int* obs_nrows,
                     const double* obs_V, const int* obs_nv, const double* e_min, const double* e_max, int B, const double* p0,
                     const double* p1, double* A, double* b, int* nrows, double* q_ellipse, double* centre, int* rounds, int* newton,
                     int* collision, int* status);
/* Same with DEVICE pointers for the scene, box, seeds and outputs, enqueued on `stream` (a hipStream_t); returns without waiting for
 * the sets (it waits only for the 48-byte copy of e_min / e_max).  The obstacle counts are not checked on the host here: they must
 * be in range. */
int bmpc_convex_sets_dev(bmpc_handle* h, const bmpc_sets_opts* o, int n_obs, const double* d_obs_A, const double* d_obs_b,
                         const int* d_obs_nrows, const double* d_obs_V, const int* d_obs_nv, const double* d_e_min, const double* d_e_max,
                         int B, const double* d_p0, const double* d_p1, double* d_A, double* d_b, int* d_nrows, double* d_q_ellipse,
                         double* d_centre, int* d_rounds, int* d_newton, int* d_collision, int* d_status, void* stream);

/* Duration (ms) of the most recent solve kernel measured with HIP events on its stream
 * (bmpc_solve: events around the launch; bmpc_solve_dev: caller must have synchronised). */
int bmpc_last_kernel_ms(bmpc_handle* h, float* ms);

/* Diagnostic builds (-DBMPC_PROFILE) only: per-phase shader-cycle sums of the last launches. */
int bmpc_debug_phase_cycles(bmpc_handle* h, double* out16);
/* Diagnostic: per-instance solver state of the most recent finished solve (B rows of 12 doubles, host memory): iterations, status,
 * mu, alpha (1e300: no acceptable step), alpha_dual, fraction-to-boundary alpha, delta_w, exact Hessian wanted next, factorisation
 * retries, rejected line-search trials, KKT error of the previous iterate, stall counter.  With max_iter = k: the decisions of
 * iteration k - 1, which the iterate-for-iterate parity test compares with the oracle's.  B <= workspace slots. */
int bmpc_debug_inst_state(bmpc_handle* h, int B, double* out);
/* Test entry: ONE super-step of the product's kernels for B instances at the points x0, from a planted state, stopped where the
 * requested outputs say.  The sequence, every step in brackets only when its arrays are given:
 *   the product's init launch -> [rows and mode overwritten] -> [plant0] -> [ctl_plant] -> the product's evaluation launches
 *     -> (H: the stage matrices out, stop)
 *     -> the product's Riccati launch in the variant B live instances select, k_fwd, k_step -> the Newton step out -> [ctl, first part]
 *     -> (no trial outputs: stop) | [plant1] -> the product's trial launch once, in the variant the number of groups of pairs
 *        selects (bmpc_k_trial_spec / bmpc_k_trial) -> the trial outputs -> [ctl, second part]
 * No list rotation.  H is requested alone; otherwise dzeta, dt, dz, state are required, and the seven trial outputs come all or
 * none.  When the trial runs, the handle's trial_repeats must be the default (>= 9): the whole search ends inside the launch.
 * tol, max_iter, hess_switch, inertia_err, stall_n, gn_backoff, mu_floor_k, dw0 are the handle's options.  Host pointers, per
 * instance [B][...]; B <= workspace slots; the handle must have been created with hess = 2.  rc 1 on misuse, before anything is
 * launched.  A NaN in a planted record leaves the field as the product made it. */
typedef struct bmpc_debug_step {
    const double *x0, *lbx, *ubx, *p;   /* the problems, as for bmpc_solve (required) */
    /* GIVEN row slacks / multipliers t, z [N-1][208] (row slots of csrc/bmpc_device.hpp) and mode: the Hessian of the first
     * factorisation attempt -- 0 Gauss-Newton, 1 exact, 2 exact with the KKT error of the previous iterate set to 0 (a failed attempt is
     * then answered by delta_w, not by the Gauss-Newton fallback).  All three, or all three NULL: the rows stay as the init launch made
     * them (the merit pieces are then those of the init launch) and nothing can be planted.  With H the mode is not used: the
     * matrices are those of the exact Hessian. */
    const double *t, *z;
    const int* mode;
    /* plant0 [22] (or NULL), before the evaluation launches, together with the rows: f0, th0, ls0 (objective, infeasibility and
     *   sum log t of the overwritten rows -- the product takes them from the last accepted trial), the iteration counter, filt_mu,
     *   nfilt, filt_th[8], filt_phi[8].  The line-search start then forms phi0 and applies its own rules to them (theta_max /
     *   theta_min at iteration 0, filter reset when mu != filt_mu).  With the trial outputs only;
     * plant1 [19] (or NULL), after k_step: nfilt, filt_th[8], filt_phi[8], theta_max, theta_min.  With the trial outputs only;
     * ctl_plant [8] (or NULL), the iteration-control state -- what decides whether there is another iteration and with which Hessian,
     *   barrier parameter and delta_w (the KKT test, the barrier update and the factorisation attempts of the Riccati kernels; the
     *   Hessian choice at the end of the line search): mu, err_prev, err_best, stall, dw_last, gn_back, gn_skip, it (planted after
     *   plant0: its iteration counter wins; a NaN leaves what the init launch and `mode` made).  With the trial outputs only. */
    const double *plant0, *plant1, *ctl_plant;
    /* with H only: GIVEN adjoint multipliers of the pi dynamics [N][3] (stage k uses lam_pi[k+1]) */
    const double* lam_pi;
    /* the stage matrices the Riccati sweep factorises (zeta coordinates, [N-1][41][41], row-major): a kernel of the entry's own runs
     * the sweep's load phase per stage and copies the matrix out.  Needs t, z and lam_pi. */
    double* H;
    /* the Newton step: dzeta [N-1][41]; the row steps dt, dz [N-1][208] (NaN in the slots k_step did not write: padding slots are left
     * untouched); state [12] with the fields of bmpc_debug_inst_state, where state[1] is -1 when the instance took a step and its
     * final status (0 converged at entry, 3 every factorisation attempt failed) otherwise, [2] the barrier parameter the forward start
     * used, [4] / [5] the dual / primal fraction-to-boundary lengths, [6] delta_w, [7] the mode the FIRST attempt ran with, [8] the
     * retries.  Taken before the trial launch. */
    double *dzeta, *dt, *dz, *state;
    /* the trial outputs: zeta0 [N-1][41] and t0, z0 [N-1][208], the iterate the search started from; zeta1, t1, z1, the iterate after it
     * (with given rows every slot of the copies the trial writes holds a NaN beforehand: slots the search did not write stay NaN --
     * except that bmpc_k_trial_spec copies whole candidate records over when the accepted trial is not the first, slots no row uses
     * included; with t, z == NULL inactive slots keep t = 1, z = 0; an instance that finished at entry: NaN); ls [36]: ap, ad
     * (fraction-to-boundary lengths), D (merit derivative), phi0, alpha (accepted step length; 1e300: all ten trials rejected, the
     * tenth kept), bt (rejected trials), f0, th0, ls0 of the new iterate, nfilt, filt_th[8], filt_phi[8] (NaN beyond nfilt),
     * theta_max, theta_min, it, flip, hess_mode, state, mu, filt_mu, 0, 0. */
    double *zeta0, *t0, *z0, *zeta1, *t1, *z1, *ls;
    /* ctl [20] (or NULL; with the trial outputs only): after the direction launches state, status (-1: not finished), mu, delta_w,
     * tries, ksel, hess_mode, err_prev, err_best, stall, dw_last, gn_back, gn_skip, it, fk; after the trial launch it, hess_mode,
     * gn_skip, state; 0. */
    double* ctl;
} bmpc_debug_step;
int bmpc_debug_superstep(bmpc_handle* h, int B, const bmpc_debug_step* s);
/* Test entry: ONE part of the set growth of bmpc_convex_sets per item, one GPU thread per item, the same device functions as the
 * product's kernel (tests/test_set_growth_gpu.py compares them with an exact projection and an optimality certificate).
 *   mode 0  one round of the polyhedron growth around p [B][3] in a GIVEN metric E [B][9] (symmetric positive definite; the product's
 *           q_inv = L L^T of the last ellipsoid, 1e-4 I in the first round) in the scene of the obs_ arguments and the workspace box
 *           (as bmpc_convex_sets): A [B][20][3], b [B][20], nrows [B] = the row count, or minus the status (-1 violates, -2 more than
 *           20 rows, -4 numerical) with status [B] set alike; q [B][9] = E^-1 as the lane formed it; rows_A, rows_b, rows_m unused.
 *   mode 1  the inscribed ellipsoid of GIVEN rows rows_A [B][20][3], rows_b [B][20], rows_m [B] in [0, 20] with the centre fixed at
 *           p: q [B][9] = L L^T, c [B][3] = p, newton [B], status [B] (0, 3 no interior point, 4 numerical); A, b, nrows return the rows.
 *   mode 2  the same with a free centre, the interior search started from p; c: the centre.  The scene arguments and E are unused in
 *           modes 1 and 2 (may be NULL / 0).
 * Host pointers.  rc 1 on misuse. */
int bmpc_debug_sets_parts(bmpc_handle* h, int mode, int n_obs, const double* obs_A, const double* obs_b, const int* obs_nrows,
                          const double* obs_V, const int* obs_nv, const double* e_min, const double* e_max, int B, const double* E,
                          const double* p, const double* rows_A, const double* rows_b, const int* rows_m, double* A, double* b,
                          int* nrows, double* q, double* c, int* newton, int* status);
/* Measurement: from the next solve on, HIP events bracket every launch of the Riccati kernel on the handle's stream
 * (bmpc_debug_time_ric(h, 1)); bmpc_debug_ric_stats then returns for the most recent solve {summed launch durations [ms], launches,
 * instance-iterations} of the throughput variant of that kernel in out6[0..2] and of its latency variant (nearly empty super-steps)
 * in out6[3..5].  bench.py derives its roofline line from these. */
int bmpc_debug_time_ric(bmpc_handle* h, int on);
int bmpc_debug_ric_stats(bmpc_handle* h, double* out6);
/* ... and of those launches of the throughput variant whose grid was the whole batch (the first super-steps of a solve, before anybody
 * has finished: the kernel at full occupancy): {summed durations [ms], launches, instance-iterations}. */
int bmpc_debug_ric_stats_full(bmpc_handle* h, double* out3);
/* Diagnostic: keeps the handle's stream busy for `ms` milliseconds (at most 10 s, then the kernel ends by itself), so that the
 * watchdog (bmpc_opts.watchdog_ms) can be exercised without a kernel that really hangs. */
int bmpc_debug_spin(bmpc_handle* h, int ms);

/* ---------------------------------------------------------------------------------------------
 * Device-resident closed loop: R rollouts advanced in lock step, one batched solve per MPC step,
 * per-rollout state in HBM.  Replaces, for every rollout and step, the host code around the solver
 * call: BoundMPC.step before the solve (BoundMPC.py:388-589), the acceptance test and
 * compute_return_data (BoundMPC.py:604-1040), ReferencePath.update (ReferencePath.py:187-207),
 * MPCNode.step's state advance with integrate_joint (MPCNode.py:106-160, util_functions.py:55-65).
 * Plan-time construction (ReferencePath.__init__, BoundMPC.__init__ / update) either stays with the caller, who
 * serialises it into the state vector: bmpc_loop_state_doubles() doubles per rollout, fields located by
 * name with bmpc_loop_field() (names = LP_FIELDS of boundplanner_amd/csrc/bmpc_loop.hpp) -- or runs on the device as well:
 * bmpc_loop_init_rollouts / bmpc_loop_replan below.
 * Per-step collision sets (ConvexSetFinder.find_set_collision_avoidance, ConvexSetFinder.py:309-375) are computed on the
 * device too: boxes around the collision points, plus separating halfspaces of the scene obstacles set with
 * bmpc_loop_set_obstacles (one scene, every rollout uses it) or with bmpc_loop_set_scenes / bmpc_loop_set_rollout_scenes (a table of
 * scenes, every rollout names its own).
 * All pointers below are HOST pointers.  The loop borrows the handle's solver and stream: do not use the handle
 * for other solves while a loop call is running.  The loop keeps the handle alive: a bmpc_destroy(handle)
 * issued while loops exist is deferred until the last bmpc_loop_destroy. */
typedef struct bmpc_loop bmpc_loop;
int bmpc_loop_state_doubles(void);
int bmpc_loop_log_doubles(void);
int bmpc_loop_field(const char* name, int* offset, int* count);
int bmpc_loop_create(bmpc_handle* h, int R, bmpc_loop** out);
void bmpc_loop_destroy(bmpc_loop* l);
const char* bmpc_loop_last_error(const bmpc_loop* l);
/* scene obstacles (BoundMPC.obstacles as polytopes A x <= b with their vertices; ConvexSetFinder.py:309-375):
 * A [n_obs][15][3] and b [n_obs][15] (first nrows[o] rows used), V [n_obs][32][3] (first nv[o] vertices used);
 * n_obs <= 16; n_obs = 0 clears the scene.  One scene that every rollout of the loop uses; for a scene per rollout see
 * bmpc_loop_set_scenes below.  Replaces whatever an earlier bmpc_loop_set_obstacles / bmpc_loop_set_scenes installed. */
int bmpc_loop_set_obstacles(bmpc_loop* l, int n_obs, const double* A, const double* b, const int* nrows, const double* V,
                            const int* nv);
/* One scene per rollout.  bmpc_loop_set_scenes installs a table of n_scenes scenes: scene s has n_obs[s] obstacles
 * (0 <= n_obs[s] <= 16); the obstacles of all scenes are stored back to back in scene order, each in the layout of
 * bmpc_loop_set_obstacles: A [sum n_obs][15][3], b [sum n_obs][15], nrows [sum n_obs], V [sum n_obs][32][3], nv [sum n_obs].
 * It replaces whatever bmpc_loop_set_obstacles / an earlier bmpc_loop_set_scenes installed (the later call wins, in either order), and
 * every rollout is assigned scene -1 (no obstacles) afterwards.  n_scenes = 0 clears the table.
 * bmpc_loop_set_rollout_scenes assigns scene[i] in [-1, n_scenes) to rollouts first .. first+count-1; -1: obstacle-free collision sets.
 * Both synchronise the loop's stream first, so they may be called between two bmpc_loop_run calls (obstacles that move or appear:
 * re-install the table, or re-assign rollouts).  Misuse (null pointers, n_obs[s] / row / vertex counts out of range, a scene index or
 * a rollout range out of range) returns 1 with a message in bmpc_loop_last_error and leaves the loop as it was.
 * The assignment is configuration of the loop, not state of the rollout: it is not part of the state vector, of
 * bmpc_loop_download / bmpc_loop_upload or of the records.  A rollout whose scene needs more than 15 rows in a collision set is
 * frozen (dead = 2) like on the shared scene, one with an obstacle that has no closest pair (empty after the 1 mm shrink) likewise
 * (dead = 3); the others are not affected.
 * Device memory: 3108 bytes per obstacle that exists (A, b, A A^T, V, box), about 50 KB for a scene of 16, plus
 * R * 6 * max n_obs * 64 bytes of closest-pair results. */
int bmpc_loop_set_scenes(bmpc_loop* l, int n_scenes, const int* n_obs, const double* A, const double* b, const int* nrows,
                         const double* V, const int* nv);
int bmpc_loop_set_rollout_scenes(bmpc_loop* l, int first, int count, const int* scene);
/* state: [count][state_doubles]; prev: [count][n_w] previous solutions (warm start) or NULL */
int bmpc_loop_upload(bmpc_loop* l, int first, int count, const double* state, const double* prev);
int bmpc_loop_download(bmpc_loop* l, int first, int count, double* state, double* prev);
/* Reference paths installed on the device, one rollout per thread, with the result the host construction + serialisation gives
 * (boundplanner_amd: ReferencePath.__init__, BoundMPC.update / __init__, device_loop.pack_state) -- no download / upload of states.
 * bmpc_loop_replan: a new via path for each of `count` rollouts (MPCNode.update_reference, MPCNode.py:82-104), tracked from the
 *   rollout's CURRENT device state: q, dq, ddq, jerk, v, p_lie, slacks0, error count, warm start and weights carry over, qf = q, the
 *   path window, split indices and rotation reference start over.  rollouts [count]: indices in any order, each at most once;
 *   n_pts [count]: via points of path i, 2 .. 8; records with the strides of 8 via points, of which the first n_pts (n_pts - 1) are
 *   read: p_via [count][8][3], r_via [count][8][9] (rotation matrices, row-major), bp1 / br1 [count][7][3] (desired basis directions
 *   per segment), e_r_bound [count][7][6] (upper 3, lower 3), a_sets [count][7][15][3], b_sets [count][7][15].
 * bmpc_loop_init_rollouts: rollouts first .. first+count-1 at rest at q0 [count][7] with the MPC weights [11] (Params.weights), on the
 *   trivial start-up path at their own end-effector pose (BoundMPC.__init__ as BatchMPCNode calls it), no warm start.
 * Both enqueue on the loop's stream, after whatever is in flight, and wait.  count = 0 is a no-op.  Misuse (null pointer, rollout index
 * out of range or listed twice, n_pts outside 2 .. 8) returns 1 with a message in bmpc_loop_last_error, checked on the host before
 * anything is enqueued: the device state stays as it was.  2: HIP error.  Neither touches the warm-start rows or a rollout that is
 * not listed.  bmpc_loop_install_ms: HIP-event time of the install kernel of the last successful call of either. */
int bmpc_loop_replan(bmpc_loop* l, int count, const int* rollouts, const int* n_pts, const double* p_via, const double* r_via,
                     const double* bp1, const double* br1, const double* e_r_bound, const double* a_sets, const double* b_sets);
int bmpc_loop_init_rollouts(bmpc_loop* l, int first, int count, const double* q0, const double* weights);
float bmpc_loop_install_ms(const bmpc_loop* l);
/* nsteps MPC steps of all rollouts; log: [nsteps][R][log_doubles] or NULL -- per row: iters, status,
 * viol, error_count, dead, phi, phi_max, split_idx[1], sector, switch, p_lie(6), q(7).
 * ms_total: HIP-event time of the whole run on the loop's stream; ms_solve: host time inside the solves */
int bmpc_loop_run(bmpc_loop* l, int nsteps, double* log, float* ms_total, float* ms_solve);
/* Trace records with the content of the reference's message boundmpcmsg/msg/MPCData.msg:1-64, written by the finish kernel for
 * the rollouts selected with bmpc_loop_set_record (n = 0 switches them off; they cost 16 + 64 N + 600 doubles per rollout and
 * step).  bmpc_loop_records copies the records of the last bmpc_loop_run / bmpc_loop_finish: out [steps][n][record_doubles(N)] with room for
 * max_steps steps (rc 1 when more were recorded; out == NULL returns only *steps, to size the buffer; records of dead rollouts are zero),
 * each: header (iters, status, viol, error_count, valid stages n, sector, phi_max, split_idxs[5], next selector, 0, 0, 0);
 * N stage blocks of 64 (p 6, v 6, q 7, dq 7, ddq 7, dddq 7, phi, dphi, e_p 3, de_p 3, e_r 3, de_r 3, e_r_orth1, e_r_par,
 * e_r_orth2, p_ref 6, segment; zero beyond n); the a_set / b_set / a_set_joints / b_set_joints blocks of the step's parameter
 * vector (600).  boundplanner_amd.mpc_data.from_device_record decodes them.  Lock-step runs only. */
int bmpc_loop_record_doubles(int N);
int bmpc_loop_set_record(bmpc_loop* l, int n, const int* rollouts);
int bmpc_loop_records(bmpc_loop* l, double* out, int max_steps, int* steps);
/* The same nsteps MPC steps of all rollouts WITHOUT lock step: the rollouts are independent, so each one starts its next
 * step as soon as its own solve has retired (its workspace slot is re-admitted with the next problem, prepared on the
 * device) instead of waiting for the slowest solve of the batch at every step.  Same log as bmpc_loop_run (bitwise). */
int bmpc_loop_run_async(bmpc_loop* l, int nsteps, double* log, float* ms_total);
/* the three phases of one step separately, and access to the solver arguments / solution (tests) */
int bmpc_loop_prepare(bmpc_loop* l);
int bmpc_loop_solve(bmpc_loop* l);
int bmpc_loop_finish(bmpc_loop* l, double* log);
int bmpc_loop_problem(bmpc_loop* l, double* x0, double* lbx, double* ubx, double* p);
int bmpc_loop_solution(bmpc_loop* l, double* x, int* iters, int* status, double* viol);
int bmpc_loop_set_solution(bmpc_loop* l, const double* x, const int* iters, const int* status, const double* viol);

#ifdef __cplusplus
}
#endif
#endif
