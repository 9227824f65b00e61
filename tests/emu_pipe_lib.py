"""ctypes access to the CPU thread emulation of the batch-synchronous HIP pipeline (tests/emu/emu_pipe.cpp)
-- debugging aid, TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import emu_build

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


def stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, dt=0.1, split=0):
    """emu_stage_matrices: H [B][N-1][41][41] from the kernel bodies at the points w [B][n_w] with row (t, z) [B][N-1][208] in the
    kernels' slot numbering and lam_pi [B][N][3]; split = 1 runs k_eval as the two-wavefront pair."""
    lib = ctypes.CDLL(build())
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (w, lbx, ubx, p))
    B = w.shape[0]
    t, z, lam_pi = (np.ascontiguousarray(a, float) for a in (t, z, lam_pi))
    assert t.shape == z.shape == (B, N - 1, 208) and lam_pi.shape == (B, N, 3)
    H = np.zeros((B, N - 1, 41, 41))
    P = lambda a: a.ctypes.data_as(_dp)
    rc = lib.emu_stage_matrices(N, ctypes.c_double(dt), B, P(w), P(lbx), P(ubx), P(p), P(t), P(z), P(lam_pi), split, P(H))
    assert rc == 0, rc
    return H


def newton_step(N, w, lbx, ubx, p, t, z, mode, dt=0.1, variant=0):
    """emu_newton_step: (dzeta [B][N-1][41], dt [B][N-1][208], dz [B][N-1][208], state [B][12]) of one super-step of the kernel
    bodies at the points w [B][n_w] with row (t, z) [B][N-1][208] and first-attempt Hessian mode [B]; variant = 1 runs the
    speculative pair of Riccati bodies."""
    lib = ctypes.CDLL(build())
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (w, lbx, ubx, p))
    B = w.shape[0]
    t, z = (np.ascontiguousarray(a, float) for a in (t, z))
    mode = np.ascontiguousarray(np.broadcast_to(mode, (B,)), np.int32)
    assert t.shape == z.shape == (B, N - 1, 208)
    dzeta, dts, dzs, state = np.zeros((B, N - 1, 41)), np.zeros((B, N - 1, 208)), np.zeros((B, N - 1, 208)), np.zeros((B, 12))
    P = lambda a: a.ctypes.data_as(_dp)
    rc = lib.emu_newton_step(N, ctypes.c_double(dt), B, P(w), P(lbx), P(ubx), P(p), P(t), P(z), mode.ctypes.data_as(_ip), variant,
                             P(dzeta), P(dts), P(dzs), P(state))
    assert rc == 0, rc
    return dzeta, dts, dzs, state


LS_SHAPES = lambda B, N: dict(dzeta=(B, N - 1, 41), dt=(B, N - 1, 208), dz=(B, N - 1, 208), state=(B, 12), zeta0=(B, N - 1, 41),
                              t0=(B, N - 1, 208), z0=(B, N - 1, 208), zeta1=(B, N - 1, 41), t1=(B, N - 1, 208), z1=(B, N - 1, 208), ls=(B, 36))


def line_search(N, w, lbx, ubx, p, t=None, z=None, mode=None, plant0=None, plant1=None, dt=0.1, variant=1):
    """emu_line_search: Newton step and filter line search of one super-step of the kernel bodies (the bodies of
    bmpc_debug_line_search; same arguments and the same dict as HipBoundMPC.line_search); variant 1: k_trial_spec_body (what the
    GPU runs for a small batch), 0: k_trial_body."""
    lib = ctypes.CDLL(build())
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (w, lbx, ubx, p))
    B = w.shape[0]
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    if t is not None:
        t, z = (np.ascontiguousarray(a, float) for a in (t, z))
        mode = np.ascontiguousarray(np.broadcast_to(mode, (B,)), np.int32)
        assert t.shape == z.shape == (B, N - 1, 208)
    if plant0 is not None:
        plant0 = np.ascontiguousarray(plant0, float); assert plant0.shape == (B, 22)
    if plant1 is not None:
        plant1 = np.ascontiguousarray(plant1, float); assert plant1.shape == (B, 19)
    out = {k: np.zeros(v) for k, v in LS_SHAPES(B, N).items()}
    rc = lib.emu_line_search(N, ctypes.c_double(dt), B, P(w), P(lbx), P(ubx), P(p), P(t), P(z),
                             mode.ctypes.data_as(_ip) if mode is not None else None, P(plant0), P(plant1), variant,
                             *(P(out[k]) for k in out))
    assert rc == 0, rc
    return out


def iteration_control(N, w, lbx, ubx, p, t, z, mode, ctl_plant=None, plant0=None, plant1=None, dt=0.1, tol=1e-5, max_iter=100, mu_floor_k=1e4, dw0=1e-4, variant=0):
    """emu_iteration_control: the bodies of bmpc_debug_iteration_control (same arguments and the same dict as
    HipBoundMPC.iteration_control, tol, max_iter, mu_floor_k and dw0 being the handle's there); variant 1 runs the speculative pair of Riccati bodies."""
    lib = ctypes.CDLL(build())
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (w, lbx, ubx, p))
    B = w.shape[0]
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    t, z = (np.ascontiguousarray(a, float) for a in (t, z))
    mode = np.ascontiguousarray(np.broadcast_to(mode, (B,)), np.int32)
    assert t.shape == z.shape == (B, N - 1, 208)
    plant0, plant1, ctl_plant = (None if a is None else np.ascontiguousarray(a, float) for a in (plant0, plant1, ctl_plant))
    assert plant0 is None or plant0.shape == (B, 22)
    assert plant1 is None or plant1.shape == (B, 19)
    assert ctl_plant is None or ctl_plant.shape == (B, 8)
    out = {k: np.zeros(v) for k, v in LS_SHAPES(B, N).items()}
    out["ctl"] = np.zeros((B, 20))
    rc = lib.emu_iteration_control(N, ctypes.c_double(dt), ctypes.c_double(tol), int(max_iter), ctypes.c_double(mu_floor_k), ctypes.c_double(dw0), B, P(w), P(lbx), P(ubx), P(p), P(t), P(z),
                                   mode.ctypes.data_as(_ip), P(plant0), P(plant1), P(ctl_plant), variant, *(P(out[k]) for k in out))
    assert rc == 0, rc
    return out
