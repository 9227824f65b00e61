"""ctypes access to the CPU thread emulation of the batch-synchronous HIP pipeline (tests/emu/emu_pipe.cpp)
-- debugging aid, TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import emu_build
from boundplanner_amd.solver import STOPS, BmpcDebugStep, debug_step      # (ctypes and numpy only: no GPU, no library)

LIB = "libbmpc_emupipe.so"
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def build(force=False, lib=LIB, defs=()):
    return emu_build.build("emu_pipe.cpp", lib, ("-O1", "-g", *defs), force=force)


# build variants of the device source (kept behind build knobs; the product build uses the defaults)
VARIANTS = {"trial4": ("-DEMU_TRIAL_NW=4",)}       # k_trial as a workgroup of four wavefronts, one part of the row walk each


def solve_batch(N, x0, lbx, ubx, p, dt=0.1, tol=1e-5, max_iter=100, hess=2, hess_switch=1.0, mu_init=0.1,
                kappa_mu=0.1, theta_mu=2.0, kappa_eps=1000.0, want_g=False, verbose=0, want_lam=False, slots=0,
                mu_floor_k=1e4, dw0=1e-4, inertia_err=1e-2, inertia=2, stall_n=8, gn_backoff=2, slack_reset=1, ls_alpha_mem=0.0, trial_repeats=9,
                variant=None):
    if variant is None:
        lib = ctypes.CDLL(build())
    else:
        lib = ctypes.CDLL(build(lib=LIB.replace(".so", f"_{variant}.so"), defs=VARIANTS[variant]))
    n_w, n_g = 44 * N + 6, 147 * (N - 1) + 21
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    x0, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (x0, lbx, ubx, p))
    B = x0.shape[0]
    x = np.zeros((B, n_w)); g = np.zeros((B, n_g)) if want_g else None
    f = np.zeros(B); viol = np.zeros(B); it = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    lam_g = np.full((B, n_g), np.nan) if want_lam else None
    lam_x = np.full((B, n_w), np.nan) if want_lam else None
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    D = ctypes.c_double
    steps = lib.emu_pipe_solve(N, D(dt), D(tol), max_iter, hess, D(hess_switch), D(mu_init), D(kappa_mu), D(theta_mu),
                               D(kappa_eps), B, P(x0), P(lbx), P(ubx), P(p), P(x), P(g), P(f),
                               it.ctypes.data_as(_ip), st.ctypes.data_as(_ip), P(viol), verbose, P(lam_g), P(lam_x), slots,
                               D(mu_floor_k), D(dw0), D(inertia_err), inertia, stall_n, gn_backoff, slack_reset, D(ls_alpha_mem), trial_repeats)
    return dict(x=x, g=g, f=f, iters=it, status=st, viol=viol, steps=steps, lam_g=lam_g, lam_x=lam_x)


class EmuStepCfg(ctypes.Structure):
    """emu_step_cfg of tests/emu/emu_pipe.cpp, with bmpc_default_opts' values of the four options."""
    _fields_ = [(k, ctypes.c_int) for k in ("N", "max_iter", "eval_split", "ric_spec", "trial_spec")] + \
               [(k, ctypes.c_double) for k in ("dt", "tol", "mu_floor_k", "dw0")]
    DEFAULTS = dict(max_iter=100, dt=0.1, tol=1e-5, mu_floor_k=1e4, dw0=1e-4)


def superstep(N, want, cfg, **arrays):
    """emu_superstep: the sequence of bmpc_debug_superstep run by the kernel bodies, on the record solver.debug_step makes of the
    named arrays; cfg: fields of EmuStepCfg other than the defaults.  The dict of the outputs `want` names."""
    lib = ctypes.CDLL(build())
    lib.emu_superstep.argtypes = [ctypes.POINTER(EmuStepCfg), ctypes.c_int, ctypes.POINTER(BmpcDebugStep)]
    B, step, out = debug_step(N, want, **arrays)
    rc = lib.emu_superstep(ctypes.byref(EmuStepCfg(N=N, **{**EmuStepCfg.DEFAULTS, **cfg})), B, ctypes.byref(step))
    assert rc == 0, rc
    return out


def stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, dt=0.1, split=0):
    """H [B][N-1][41][41] from the kernel bodies at the points w [B][n_w] with row (t, z) [B][N-1][208] in the kernels' slot
    numbering and lam_pi [B][N][3]; split = 1 runs k_eval as the two-wavefront pair."""
    return superstep(N, STOPS["H"], dict(dt=dt, eval_split=split), x0=w, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=1, lam_pi=lam_pi)["H"]


def newton_step(N, w, lbx, ubx, p, t, z, mode, dt=0.1, variant=0):
    """(dzeta [B][N-1][41], dt [B][N-1][208], dz [B][N-1][208], state [B][12]) of one super-step of the kernel bodies at the points
    w [B][n_w] with row (t, z) [B][N-1][208] and first-attempt Hessian mode [B]; variant = 1 runs the speculative pair of Riccati
    bodies."""
    return tuple(superstep(N, STOPS["newton"], dict(dt=dt, ric_spec=variant), x0=w, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode).values())


def line_search(N, w, lbx, ubx, p, t=None, z=None, mode=None, plant0=None, plant1=None, dt=0.1, variant=1):
    """Newton step and filter line search of one super-step of the kernel bodies (same arguments and the same dict as
    HipBoundMPC.line_search); variant 1: k_trial_spec_body (what the GPU runs for a small batch), 0: k_trial_body."""
    return superstep(N, STOPS["ls"], dict(dt=dt, trial_spec=variant), x0=w, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode, plant0=plant0,
                     plant1=plant1)


def iteration_control(N, w, lbx, ubx, p, t, z, mode, ctl_plant=None, plant0=None, plant1=None, dt=0.1, tol=1e-5, max_iter=100, mu_floor_k=1e4, dw0=1e-4, variant=0):
    """The same with the iteration-control state planted and returned (same arguments and the same dict as
    HipBoundMPC.iteration_control, tol, max_iter, mu_floor_k and dw0 being the handle's there); variant 1 runs the speculative pair
    of Riccati bodies.  The trial body is k_trial_spec_body."""
    cfg = dict(dt=dt, tol=tol, max_iter=int(max_iter), mu_floor_k=mu_floor_k, dw0=dw0, ric_spec=variant, trial_spec=1)
    return superstep(N, STOPS["ctl"], cfg, x0=w, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode, plant0=plant0, plant1=plant1,
                     ctl_plant=ctl_plant)
