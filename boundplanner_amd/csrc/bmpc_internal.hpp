// The library's own cross-file interface: every function that one .hip file defines and another calls is declared here and
// nowhere else, and both files include this header.  They are extern "C" symbols, so the linker does not compare signatures: a
// definition that drifts from its prototype is a compile error only because the defining file sees the prototype too.
// Types are forward-declared: a file that only defines launchers does not pull in the other kernels' headers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

struct bmpc_handle;
struct bmpc_debug_step;      // include/boundmpc.h
namespace bmpc {
struct RobotConst;
struct IkOpts;
struct SetScene;
template <int DEV> struct PipeArgsT;
typedef PipeArgsT<0> PipeArgsH;
}  // namespace bmpc

// an integer knob of the environment (A/B runs, tests), `dflt` when it is not set: the one place that reads one.  When a knob is
// read -- once per process, per handle, per call -- is its caller's business.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

extern "C" {
// bmpc_fk.hip
hipError_t bmpc_launch_fk(int B, const bmpc::RobotConst* rc, const double* q, const double* dq, double* ee_pos, double* ee_rot,
                          double* col_pts, double* jac, double* dvdq, hipStream_t st);
hipError_t bmpc_launch_spin(int ms, hipStream_t st);
// bmpc_ik.hip
hipError_t bmpc_launch_ik(int B, int log2s, const bmpc::IkOpts* o, const bmpc::RobotConst* rc, const double* pd, const double* rd,
                          const double* q0, const double* lo, const double* hi, double* q, double* cost, double* pos_err,
                          double* rot_err, int* iters, int* status, int* seed, hipStream_t st);
// bmpc_sets.hip
hipError_t bmpc_launch_sets(int B, int segment, int fixed_mid, int optimize, const bmpc::SetScene* sc, double* AAt_ws,
                            const double* p0, const double* p1, double* A, double* b, int* nrows, double* q, double* c, int* rounds,
                            int* newton, int* collision, int* status, hipStream_t st);
hipError_t bmpc_launch_sets_parts(int B, int mode, const bmpc::SetScene* sc, const double* E, const double* p, const double* A_in,
                                  const double* b_in, const int* m_in, double* A, double* b, int* nrows, double* q, double* c,
                                  int* newton, int* status, hipStream_t st);      // (bmpc_debug_sets_parts)
// bmpc_pipeline.hip
hipError_t bmpc_pipe_launch_init(const bmpc::PipeArgsH* A, int n0, hipStream_t st);
hipError_t bmpc_pipe_launch_retire_out(const bmpc::PipeArgsH* A, int n_max, hipStream_t st);
hipError_t bmpc_pipe_launch_retire_admit(const bmpc::PipeArgsH* A, int n_max, int refill, hipStream_t st);
hipError_t bmpc_pipe_launch_step(bmpc::PipeArgsH* A, int n_act, hipStream_t st, hipEvent_t e0, hipEvent_t e1, int* was_lat);
hipError_t bmpc_pipe_launch_mult(const bmpc::PipeArgsH* A, hipStream_t st);
hipError_t bmpc_pipe_launch_superstep(bmpc::PipeArgsH* A, const bmpc_debug_step* d, hipStream_t st);      // (d: DEVICE pointers)
void bmpc_pipe_ls_sizes(int* plant0, int* plant1, int* out);      // doubles per instance: plant0, plant1, ls of bmpc_debug_step
void bmpc_pipe_ctl_sizes(int* plant, int* out);                   // ... ctl_plant, ctl
long bmpc_pipe_fixed_launches(void);      // launches of this process that went to a fixed-horizon pair kernel (below)
void bmpc_pipe_build_table(int* tbl);
// bmpc_pair_n20.hip, bmpc_pair_n30.hip (bmpc_pair_fixed.hpp): the pair kernels of a super-step compiled for one horizon, slot-major
// layout.  One launch of kernel `kern` (FX_*) over nb workgroups of nt threads for nw groups of pairs.
enum { FX_POINTS, FX_POSE, FX_EVAL_MAIN, FX_EVAL_CHAIN, FX_POINTS_POSE, FX_EVAL_CURV_SPLIT, FX_STEP, FX_TRIAL, FX_TRIAL_SPEC };
typedef void (*bmpc_pair_launcher)(int kern, const bmpc::PipeArgsH* A, int nw, unsigned nb, unsigned nt, size_t lds_bytes, hipStream_t st);
void bmpc_pair_launch_n20(int kern, const bmpc::PipeArgsH* A, int nw, unsigned nb, unsigned nt, size_t lds_bytes, hipStream_t st);
void bmpc_pair_launch_n30(int kern, const bmpc::PipeArgsH* A, int nw, unsigned nb, unsigned nt, size_t lds_bytes, hipStream_t st);
size_t bmpc_pipe_state_bytes(void);

// bmpc_capi.hip, for the device loops of bmpc_loop.hip.  A loop registers with the handle it borrows, so that destroying the
// handle first is safe.
void bmpc_handle_retain(bmpc_handle* h);
void bmpc_handle_release(bmpc_handle* h);
// closed loop: called between the two halves of a retirement with the list of slots whose instances have just retired
// (device pointers: list, its length); enqueues the caller's post-processing / next-problem kernels on the stream
typedef int (*bmpc_retire_hook)(void* ctx, const int* d_done, const int* d_n_done, int n_max, void* stream);
// Closed loop without lock step (bmpc_loop_run_async): B rows, each a rollout whose successive problems are produced in
// place by `hook`; a row is solved again while d_cont[row] != 0.
int bmpc_solve_dev_hooked(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx, const double* d_ubx, const double* d_p,
                          double* d_x, double* d_f, int* d_iters, int* d_status, double* d_viol, void* stream, bmpc_retire_hook hook,
                          void* hook_ctx, const int* d_cont);
}
