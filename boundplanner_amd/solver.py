"""ctypes binding of libboundmpc_hip.so (C ABI: include/boundmpc.h) and the solver object that is
call-compatible with the CasADi function used at BoundMPC.py:594-617.

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible, constructing a
solver raises.
"""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BMPC_LIB") or os.path.join(_HERE, "csrc", "libboundmpc_hip.so")   # BMPC_LIB: experiment builds
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


class BmpcIkOpts(ctypes.Structure):
    _fields_ = [("tol_cost", ctypes.c_double), ("tol_grad", ctypes.c_double), ("lambda0", ctypes.c_double), ("max_iter", ctypes.c_int)]


class BmpcSetsOpts(ctypes.Structure):
    _fields_ = [("segment", ctypes.c_int), ("fixed_mid", ctypes.c_int), ("optimize", ctypes.c_int)]


SETS_ROWS, SETS_MAXOBS, SETS_OROWS, SETS_NV = 20, 32, 15, 32       # include/boundmpc.h bmpc_convex_sets
# Result arrays of the batched kernels, in the order of the C entries' output arguments: name -> (shape after the batch axis, dtype).
# The numpy dicts of ik / convex_sets, the torch dicts of ik_dev / convex_sets_dev and the ctypes arguments all come from these.
_F, _I = np.float64, np.int32
IK_OUT = {"q": ((7,), _F), "cost": ((), _F), "pos_err": ((), _F), "rot_err": ((), _F), "iters": ((), _I), "status": ((), _I), "seed": ((), _I)}
SETS_OUT = {"A": ((SETS_ROWS, 3), _F), "b": ((SETS_ROWS,), _F), "nrows": ((), _I), "q_ellipse": ((3, 3), _F), "centre": ((3,), _F),
            "rounds": ((), _I), "newton": ((), _I), "collision": ((), _I), "status": ((), _I)}


def out_arrays(table, B, alloc=np.empty):
    """The result dict of a table for a batch of B as numpy arrays (alloc: np.empty or np.zeros)."""
    return {k: alloc((B, *shape), dt) for k, (shape, dt) in table.items()}


def out_tensors(table, B, device):
    """The same as uninitialised torch tensors on `device`."""
    import torch
    return {k: torch.empty((B, *shape), dtype=getattr(torch, np.dtype(dt).name), device=device) for k, (shape, dt) in table.items()}


def out_args(table, out):
    """The output arguments of the C entry from a result dict: typed pointers of numpy arrays, device addresses of torch tensors."""
    return [out[k].ctypes.data_as(_ip if dt is _I else _dp) if isinstance(out[k], np.ndarray) else out[k].data_ptr()
            for k, (_, dt) in table.items()]


SETS_STATUS = {1: "Ellipse violates constraints", 2: "the set needs more than 20 rows", 3: "no strictly interior point for the ellipsoid",
               4: "numerical failure"}


def pack_set_scene(obs_sets, obs_points_sets):
    """scenes.pack_scene at the set kernel's limits: the name earlier callers import."""
    from .scenes import pack_scene
    return pack_scene(obs_sets, obs_points_sets, SETS_MAXOBS, min_nv=1, pad_empty=True)


class BmpcOpts(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int), ("nr_segs", ctypes.c_int), ("dt", ctypes.c_double),
                ("tol", ctypes.c_double), ("max_iter", ctypes.c_int), ("device", ctypes.c_int),
                ("hess", ctypes.c_int), ("hess_switch", ctypes.c_double), ("mu_init", ctypes.c_double),
                ("kappa_mu", ctypes.c_double), ("theta_mu", ctypes.c_double), ("kappa_eps", ctypes.c_double),
                ("mu_floor_k", ctypes.c_double), ("inertia", ctypes.c_int), ("dw0", ctypes.c_double),
                ("inertia_err", ctypes.c_double), ("stall_n", ctypes.c_int), ("slack_reset", ctypes.c_int), ("ls_alpha_mem", ctypes.c_double), ("gn_backoff", ctypes.c_int),
                ("trial_repeats", ctypes.c_int), ("watchdog_ms", ctypes.c_int), ("max_batch", ctypes.c_int), ("pool_slots", ctypes.c_int)]


class BmpcDebugStep(ctypes.Structure):
    """bmpc_debug_step of include/boundmpc.h: the arguments of bmpc_debug_superstep."""
    _fields_ = [(k, _ip if k == "mode" else _dp) for k in
                ("x0", "lbx", "ubx", "p", "t", "z", "mode", "plant0", "plant1", "ctl_plant", "lam_pi", "H", "dzeta", "dt", "dz", "state",
                 "zeta0", "t0", "z0", "zeta1", "t1", "z1", "ls", "ctl")]


# The record's arrays for a batch of B at horizon N, name -> shape: the inputs beside mode (int32 [B]), and the outputs.
STEP_IN = lambda B, N: dict(x0=(B, 44 * N + 6), lbx=(B, 44 * N + 6), ubx=(B, 44 * N + 6), p=(B, 875), t=(B, N - 1, 208), z=(B, N - 1, 208),
                            plant0=(B, 22), plant1=(B, 19), ctl_plant=(B, 8), lam_pi=(B, N, 3))
LS_SHAPES = lambda B, N: dict(dzeta=(B, N - 1, 41), dt=(B, N - 1, 208), dz=(B, N - 1, 208), state=(B, 12), zeta0=(B, N - 1, 41),
                              t0=(B, N - 1, 208), z0=(B, N - 1, 208), zeta1=(B, N - 1, 41), t1=(B, N - 1, 208), z1=(B, N - 1, 208),
                              ls=(B, 36), ctl=(B, 20), H=(B, N - 1, 41, 41))
# The outputs to ask for, by where the sequence is to stop (a request bmpc_debug_superstep refuses is any other tuple of names).
_LS = tuple(LS_SHAPES(1, 2))
STOPS = {"H": ("H",), "newton": _LS[:4], "ls": _LS[:11], "ctl": _LS[:12]}


def debug_step(N, want, **arrays):
    """The arguments of bmpc_debug_superstep from named arrays (needs no GPU; tests/emu_pipe_lib.py uses it too): x0, lbx, ubx, p
    and any of t, z, mode, plant0, plant1, ctl_plant, lam_pi (include/boundmpc.h; None = not given); want: the names of the outputs
    to allocate, a tuple of STOPS.  +-inf bounds become +-1e20, mode is broadcast to int32 [B], everything is made contiguous and
    its shape checked.  Returns (B, the filled BmpcDebugStep -- which keeps the arrays alive --, the dict of zeroed outputs)."""
    a = {k: v for k, v in arrays.items() if v is not None}
    a["lbx"] = np.where(np.isinf(a["lbx"]), -1e20, a["lbx"]); a["ubx"] = np.where(np.isinf(a["ubx"]), 1e20, a["ubx"])
    for k in ("x0", "lbx", "ubx", "p"):
        a[k] = np.atleast_2d(a[k])
    B = a["x0"].shape[0]
    shapes = STEP_IN(B, N)
    for k in a:
        if k == "mode":
            a[k] = np.ascontiguousarray(np.broadcast_to(a[k], (B,)), np.int32)
        else:
            a[k] = np.ascontiguousarray(a[k], float)
            assert a[k].shape == shapes[k], (k, a[k].shape, shapes[k])
    shapes = LS_SHAPES(B, N)
    out = {k: np.zeros(shapes[k]) for k in want}
    step = BmpcDebugStep(**{k: v.ctypes.data_as(_ip if k == "mode" else _dp) for k, v in {**a, **out}.items()})
    step.arrays = (a, out)
    return B, step, out


EXPORTS = ["bmpc_default_opts", "bmpc_create", "bmpc_destroy", "bmpc_last_error", "bmpc_dims",
           "bmpc_gbounds", "bmpc_solve", "bmpc_solve_dev", "bmpc_solve_dev_async", "bmpc_multipliers_dev", "bmpc_wait", "bmpc_active", "bmpc_fk",
           "bmpc_last_kernel_ms", "bmpc_get_opts", "bmpc_stream", "bmpc_robot_iiwa14", "bmpc_robot_gen3", "bmpc_set_robot", "bmpc_get_robot",
           "bmpc_debug_phase_cycles", "bmpc_debug_spin", "bmpc_debug_inst_state", "bmpc_debug_superstep", "bmpc_debug_time_ric", "bmpc_debug_ric_stats", "bmpc_debug_ric_stats_full",
           "bmpc_loop_state_doubles", "bmpc_loop_log_doubles", "bmpc_loop_field", "bmpc_loop_create", "bmpc_loop_destroy",
           "bmpc_loop_last_error", "bmpc_loop_record_doubles", "bmpc_loop_set_record", "bmpc_loop_records", "bmpc_loop_set_obstacles", "bmpc_loop_set_scenes", "bmpc_loop_set_rollout_scenes", "bmpc_loop_upload", "bmpc_loop_download", "bmpc_loop_run", "bmpc_loop_run_async", "bmpc_loop_prepare",
           "bmpc_loop_solve", "bmpc_loop_finish", "bmpc_loop_problem", "bmpc_loop_solution", "bmpc_loop_set_solution",
           "bmpc_loop_replan", "bmpc_loop_init_rollouts", "bmpc_loop_install_ms",
           "bmpc_default_ik_opts", "bmpc_ik", "bmpc_ik_dev", "bmpc_default_sets_opts", "bmpc_convex_sets", "bmpc_convex_sets_dev",
           "bmpc_debug_sets_parts"]

_lib = None


def load_library():
    """Load libboundmpc_hip.so (raises if it was not built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        # PyTorch-ROCm wheels bundle their own HIP runtime.  If this library (linked against the system ROCm) is loaded
        # first, a later `import torch` in the same process finds "No HIP GPUs" (measured on ROCm 7.2 + torch 2.10+rocm7.0);
        # the other order works and both then share one runtime.  So when torch is installed it is imported first.
        if "torch" not in sys.modules and not os.environ.get("BMPC_NO_TORCH_PRELOAD"):
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        lib.bmpc_last_error.restype = ctypes.c_char_p
        lib.bmpc_last_error.argtypes = [ctypes.c_void_p]
        lib.bmpc_create.argtypes = [ctypes.POINTER(BmpcOpts), ctypes.POINTER(ctypes.c_void_p)]
        lib.bmpc_destroy.argtypes = [ctypes.c_void_p]
        lib.bmpc_dims.argtypes = [ctypes.c_void_p, _ip, _ip, _ip]
        lib.bmpc_gbounds.argtypes = [ctypes.c_void_p, _dp, _dp]
        lib.bmpc_solve.argtypes = [ctypes.c_void_p, ctypes.c_int] + [_dp] * 4 + [_dp] * 4 + [_dp, _ip, _ip, _dp]
        lib.bmpc_solve_dev.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_void_p]
        lib.bmpc_solve_dev_async.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 10
        lib.bmpc_multipliers_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.bmpc_wait.argtypes = [ctypes.c_void_p]
        lib.bmpc_set_robot.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.bmpc_get_robot.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.bmpc_stream.restype = ctypes.c_void_p
        lib.bmpc_stream.argtypes = [ctypes.c_void_p]
        lib.bmpc_active.argtypes = [ctypes.c_void_p]
        lib.bmpc_fk.argtypes = [ctypes.c_void_p, ctypes.c_int] + [_dp] * 7
        lib.bmpc_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        lib.bmpc_loop_last_error.restype = ctypes.c_char_p
        lib.bmpc_loop_last_error.argtypes = [ctypes.c_void_p]
        lib.bmpc_loop_field.argtypes = [ctypes.c_char_p, _ip, _ip]
        lib.bmpc_loop_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.bmpc_loop_destroy.argtypes = [ctypes.c_void_p]
        lib.bmpc_loop_set_obstacles.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, _dp, _ip, _dp, _ip]
        lib.bmpc_loop_set_scenes.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip, _dp, _dp, _ip, _dp, _ip]
        lib.bmpc_loop_set_rollout_scenes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _ip]
        lib.bmpc_loop_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp, _dp]
        lib.bmpc_loop_download.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp, _dp]
        lib.bmpc_loop_run.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        lib.bmpc_loop_run_async.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_float)]
        lib.bmpc_loop_prepare.argtypes = [ctypes.c_void_p]
        lib.bmpc_loop_solve.argtypes = [ctypes.c_void_p]
        lib.bmpc_loop_finish.argtypes = [ctypes.c_void_p, _dp]
        lib.bmpc_loop_problem.argtypes = [ctypes.c_void_p, _dp, _dp, _dp, _dp]
        lib.bmpc_loop_solution.argtypes = [ctypes.c_void_p, _dp, _ip, _ip, _dp]
        lib.bmpc_loop_set_solution.argtypes = [ctypes.c_void_p, _dp, _ip, _ip, _dp]
        lib.bmpc_debug_spin.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.bmpc_debug_inst_state.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp]
        lib.bmpc_debug_superstep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(BmpcDebugStep)]
        lib.bmpc_debug_time_ric.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.bmpc_debug_ric_stats.argtypes = [ctypes.c_void_p, _dp]
        lib.bmpc_debug_ric_stats_full.argtypes = [ctypes.c_void_p, _dp]
        lib.bmpc_loop_replan.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip, _ip] + [_dp] * 7
        lib.bmpc_loop_init_rollouts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp, _dp]
        lib.bmpc_loop_install_ms.restype = ctypes.c_float
        lib.bmpc_loop_install_ms.argtypes = [ctypes.c_void_p]
        lib.bmpc_loop_set_record.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip]
        lib.bmpc_loop_records.argtypes = [ctypes.c_void_p, _dp, ctypes.c_int, _ip]
        lib.bmpc_loop_record_doubles.argtypes = [ctypes.c_int]
        lib.bmpc_default_ik_opts.argtypes = [ctypes.POINTER(BmpcIkOpts)]
        lib.bmpc_ik.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(BmpcIkOpts)] + [_dp] * 9 + [_ip] * 3
        lib.bmpc_ik_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(BmpcIkOpts)] + [ctypes.c_void_p] * 13
        lib.bmpc_default_sets_opts.argtypes = [ctypes.POINTER(BmpcSetsOpts)]
        lib.bmpc_convex_sets.argtypes = [ctypes.c_void_p, ctypes.POINTER(BmpcSetsOpts), ctypes.c_int, _dp, _dp, _ip, _dp, _ip, _dp, _dp,
                                         ctypes.c_int, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _ip, _ip, _ip]
        lib.bmpc_convex_sets_dev.argtypes = [ctypes.c_void_p, ctypes.POINTER(BmpcSetsOpts), ctypes.c_int] + [ctypes.c_void_p] * 7 + \
            [ctypes.c_int] + [ctypes.c_void_p] * 12
        lib.bmpc_debug_sets_parts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip, _dp, _ip, _dp, _dp, ctypes.c_int,
                                              _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _dp, _dp, _ip, _ip]
        _lib = lib
    return _lib


def _P(a):
    return a.ctypes.data_as(_dp) if a is not None else None


class HipBoundMPC:
    """Owner of one C handle: batched solves + batched kinematics on one MI355X."""

    def __init__(self, N, dt=0.1, tol=1e-5, max_iter=100, device=0, robot=None, **kw):
        """robot: None (iiwa14), "iiwa14", "gen3" or a table of boundplanner_amd.robots"""
        lib = load_library()
        o = BmpcOpts()
        lib.bmpc_default_opts(ctypes.byref(o), N)
        o.dt, o.tol, o.max_iter, o.device = dt, tol, max_iter, device
        for k, v in kw.items():
            setattr(o, k, v)
        self._h = ctypes.c_void_p()
        rc = lib.bmpc_create(ctypes.byref(o), ctypes.byref(self._h))
        if rc != 0:
            msg = lib.bmpc_last_error(self._h).decode() if self._h else "invalid options"
            raise RuntimeError(f"bmpc_create failed ({rc}): {msg} -- the HIP path has no CPU fallback")
        self.lib, self.N, self.opts = lib, N, o
        nw, ng, npar = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.bmpc_dims(self._h, ctypes.byref(nw), ctypes.byref(ng), ctypes.byref(npar))
        self.n_w, self.n_g, self.n_p = nw.value, ng.value, npar.value
        self.lbg, self.ubg = np.zeros(self.n_g), np.zeros(self.n_g)
        lib.bmpc_gbounds(self._h, _P(self.lbg), _P(self.ubg))
        from . import robots
        self.robot = robots.IIWA14
        if robot is not None:
            self.set_robot(robot)

    def set_robot(self, robot):
        """Kinematic table, limits and collision-sphere radii of the handle (bmpc_set_robot)."""
        from . import robots
        table = {"iiwa14": robots.IIWA14, "gen3": robots.GEN3}[robot] if isinstance(robot, str) else robot
        r = robots.to_struct(table)
        self._chk(self.lib.bmpc_set_robot(self._h, ctypes.byref(r)), "bmpc_set_robot")
        self.robot = table

    def close(self):
        if getattr(self, "_h", None):
            self.lib.bmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc == 4:
            raise RuntimeError(f"{what} refused: the handle is in use by another thread (one handle per host thread)")
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.bmpc_last_error(self._h).decode()}")

    def solve_batch(self, x0, lbx, ubx, p, want_g=False, want_lam=False):
        x0, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (x0, lbx, ubx, p))
        B = x0.shape[0]
        assert x0.shape == (B, self.n_w) and lbx.shape == x0.shape and ubx.shape == x0.shape and p.shape == (B, self.n_p)
        x = np.empty((B, self.n_w)); f = np.empty(B); viol = np.empty(B)
        g = np.empty((B, self.n_g)) if want_g else None
        iters = np.empty(B, np.int32); status = np.empty(B, np.int32)
        lam_g = np.empty((B, self.n_g)) if want_lam else None
        lam_x = np.empty((B, self.n_w)) if want_lam else None
        rc = self.lib.bmpc_solve(self._h, B, _P(x0), _P(lbx), _P(ubx), _P(p), _P(x), _P(g), _P(lam_g), _P(lam_x), _P(f),
                                 iters.ctypes.data_as(_ip), status.ctypes.data_as(_ip), _P(viol))
        self._chk(rc, "bmpc_solve")
        return dict(x=x, g=g, f=f, iters=iters, status=status, viol=viol, lam_g=lam_g, lam_x=lam_x)

    def stream(self):
        """The handle's own HIP stream as an integer (hipStream_t): the one bmpc_solve and bmpc_solve_dev_async run on."""
        return int(self.lib.bmpc_stream(self._h) or 0)

    INST_STATE_FIELDS = ("iters", "status", "mu", "alpha", "alpha_dual", "alpha_ftb", "delta_w", "hess_next", "retries", "backtracks",
                         "err_prev", "stall")

    def inst_state(self, B):
        """Diagnostic: [B][12] per-instance solver state of the most recent solve (bmpc_debug_inst_state; INST_STATE_FIELDS)."""
        out = np.zeros((B, 12))
        self._chk(self.lib.bmpc_debug_inst_state(self._h, int(B), _P(out)), "bmpc_debug_inst_state")
        return out

    def _superstep(self, want, **arrays):
        """bmpc_debug_superstep on the named arrays (debug_step): the dict of the outputs `want` names."""
        B, step, out = debug_step(self.N, want, **arrays)
        self._chk(self.lib.bmpc_debug_superstep(self._h, B, ctypes.byref(step)), "bmpc_debug_superstep")
        return out

    def stage_matrices(self, x0, lbx, ubx, p, t, z, lam_pi):
        """Test entry: stage matrices H [B][N-1][41][41] (zeta coordinates) at the points x0 [B][n_w] for given row slacks /
        multipliers t, z [B][N-1][208] and adjoint multipliers lam_pi [B][N][3] (bmpc_debug_superstep stopped after the evaluation)."""
        return self._superstep(STOPS["H"], x0=x0, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=1, lam_pi=lam_pi)["H"]

    def newton_step(self, x0, lbx, ubx, p, t, z, mode):
        """Test entry: the Newton step of one super-step at the points x0 [B][n_w] for given row slacks / multipliers t, z
        [B][N-1][208] and first-attempt Hessian mode [B] (0 Gauss-Newton, 1 exact, 2 exact + inertia correction on failure):
        (dzeta [B][N-1][41], dt [B][N-1][208], dz [B][N-1][208], state [B][12]) (bmpc_debug_superstep stopped after the direction)."""
        return tuple(self._superstep(STOPS["newton"], x0=x0, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode).values())

    LS_FIELDS = ("ap", "ad", "D", "phi0", "alpha", "bt", "f0", "th0", "ls0", "nfilt") + tuple(f"filt_th{j}" for j in range(8)) \
        + tuple(f"filt_phi{j}" for j in range(8)) + ("theta_max", "theta_min", "it", "flip", "hess_mode", "state", "mu", "filt_mu", "armijo", "pad")

    CTL_PLANT_FIELDS = ("mu", "err_prev", "err_best", "stall", "dw_last", "gn_back", "gn_skip", "it")
    CTL_FIELDS = ("state", "status", "mu", "delta_w", "tries", "ksel", "hess_mode", "err_prev", "err_best", "stall", "dw_last", "gn_back",
                  "gn_skip", "it", "fk", "it_after", "hess_mode_after", "gn_skip_after", "state_after", "pad")

    def line_search(self, x0, lbx, ubx, p, t=None, z=None, mode=None, plant0=None, plant1=None):
        """Test entry: Newton step and filter line search of one super-step (bmpc_debug_superstep run through the trial).  t, z
        [B][N-1][208] and mode [B] as for newton_step, or all None (the rows of the init launch; nothing planted); plant0 [B][22],
        plant1 [B][19] or None (include/boundmpc.h; NaN = leave the field).  Returns a dict: dzeta, dt, dz, state (as newton_step),
        zeta0, t0, z0, zeta1, t1, z1, ls [B][36] (LS_FIELDS)."""
        return self._superstep(STOPS["ls"], x0=x0, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode, plant0=plant0, plant1=plant1)

    def iteration_control(self, x0, lbx, ubx, p, t, z, mode, ctl_plant=None, plant0=None, plant1=None):
        """Test entry: the sequence of line_search with the iteration-control state planted (ctl_plant [B][8], CTL_PLANT_FIELDS;
        NaN = leave the field) and returned: the dict of line_search plus ctl [B][20] (CTL_FIELDS)."""
        return self._superstep(STOPS["ctl"], x0=x0, lbx=lbx, ubx=ubx, p=p, t=t, z=z, mode=mode, plant0=plant0, plant1=plant1,
                               ctl_plant=ctl_plant)

    def time_ric(self, on=True):
        """HIP events around every launch of the Riccati kernel, from the next solve on (bmpc_debug_time_ric)."""
        self._chk(self.lib.bmpc_debug_time_ric(self._h, int(bool(on))), "bmpc_debug_time_ric")

    def ric_stats(self):
        """{kernel: (summed launch ms, launches, instance-iterations)} of the most recent solve (bmpc_debug_ric_stats)."""
        out = np.zeros(6)
        self._chk(self.lib.bmpc_debug_ric_stats(self._h, _P(out)), "bmpc_debug_ric_stats")
        full = np.zeros(3)
        self._chk(self.lib.bmpc_debug_ric_stats_full(self._h, _P(full)), "bmpc_debug_ric_stats_full")
        return {"bmpc_k_ric": tuple(out[:3]), "bmpc_k_ric_lat": tuple(out[3:]), "bmpc_k_ric_full_batch": tuple(full)}

    def debug_spin(self, ms):
        """Diagnostic: occupy the handle's stream for `ms` milliseconds (bmpc_debug_spin)."""
        self._chk(self.lib.bmpc_debug_spin(self._h, int(ms)), "bmpc_debug_spin")

    def multipliers_dev(self, B, d_lam_g, d_lam_x, stream=0):
        """lam_g, lam_x (raw device pointers) of the most recent finished solve on this handle."""
        self._chk(self.lib.bmpc_multipliers_dev(self._h, B, d_lam_g, d_lam_x, stream or None), "bmpc_multipliers_dev")

    def solve_dev(self, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_f, d_iters, d_status, d_viol, d_g=0, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`."""
        rc = self.lib.bmpc_solve_dev(self._h, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_g or None, d_f, d_iters, d_status,
                                     d_viol, stream or None)
        self._chk(rc, "bmpc_solve_dev")

    def solve_dev_async(self, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_f, d_iters, d_status, d_viol, d_g=0):
        """Returns at once; the solve runs on the handle's own stream (one in flight per handle)."""
        rc = self.lib.bmpc_solve_dev_async(self._h, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_g or None, d_f, d_iters,
                                           d_status, d_viol)
        self._chk(rc, "bmpc_solve_dev_async")

    def wait(self):
        self._chk(self.lib.bmpc_wait(self._h), "bmpc_wait")

    def active(self):
        """Unfinished instances of the solve in flight (0 when idle)."""
        return self.lib.bmpc_active(self._h)

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self.lib.bmpc_last_kernel_ms(self._h, ctypes.byref(ms))
        return ms.value

    def fk(self, q, dq=None):
        q = np.ascontiguousarray(q, float).reshape(-1, 7)
        B = q.shape[0]
        dq = None if dq is None else np.ascontiguousarray(dq, float).reshape(-1, 7)
        out = dict(ee_pos=np.empty((B, 3)), ee_rot=np.empty((B, 3, 3)), col_pts=np.empty((B, 6, 3)),
                   jac=np.empty((B, 6, 7)), dvdq=np.empty((B, 6, 7)))
        rc = self.lib.bmpc_fk(self._h, B, _P(q), _P(dq), _P(out["ee_pos"]), _P(out["ee_rot"]), _P(out["col_pts"]),
                              _P(out["jac"]), _P(out["dvdq"]))
        self._chk(rc, "bmpc_fk")
        return out

    def _ik_opts(self, opts):
        o = BmpcIkOpts()
        self.lib.bmpc_default_ik_opts(ctypes.byref(o))
        for k, v in opts.items():
            if k not in ("tol_cost", "tol_grad", "lambda0", "max_iter"):
                raise TypeError(f"unknown IK option {k!r}")
            setattr(o, k, v)
        return o

    def ik(self, pd, rd, q0, n_seeds=1, lo=None, hi=None, **opts):
        """Batched inverse kinematics on the handle's robot (bmpc_ik): pd [B,3], rd [B,3,3], q0 [B,7]; lo / hi [B,7] (or [7]) or
        None = the robot's limits; opts: tol_cost, tol_grad, lambda0, max_iter.  Returns q [B,7], cost, pos_err, rot_err, iters,
        status, seed [B] (status 0 converged, 1 max_iter, 2 stalled, 3 numerical)."""
        pd = np.ascontiguousarray(pd, float).reshape(-1, 3)
        B = pd.shape[0]
        rd = np.ascontiguousarray(rd, float).reshape(B, 9)
        q0 = np.ascontiguousarray(q0, float).reshape(B, 7)
        lo = None if lo is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lo, float), (B, 7)))
        hi = None if hi is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hi, float), (B, 7)))
        out = out_arrays(IK_OUT, B)
        o = self._ik_opts(opts)
        rc = self.lib.bmpc_ik(self._h, B, int(n_seeds), ctypes.byref(o), _P(pd), _P(rd), _P(q0), _P(lo), _P(hi), *out_args(IK_OUT, out))
        self._chk(rc, "bmpc_ik")
        return out

    def ik_dev(self, pd, rd, q0, n_seeds=1, lo=None, hi=None, out=None, **opts):
        """bmpc_ik_dev on torch tensors of the GPU (float64, contiguous: pd [B,3], rd [B,3,3], q0 [B,7], lo / hi [B,7] or None),
        enqueued on torch.cuda.current_stream() without waiting.  out: dict of preallocated result tensors (the keys of ik) or None."""
        import torch
        B = pd.shape[0]
        for name, t, shape in (("pd", pd, (B, 3)), ("rd", rd, (B, 3, 3)), ("q0", q0, (B, 7)), ("lo", lo, (B, 7)), ("hi", hi, (B, 7))):
            if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape):
                raise ValueError(f"ik_dev: {name} must be a contiguous float64 GPU tensor of shape {shape}")
        if out is None:
            out = out_tensors(IK_OUT, B, pd.device)
        o = self._ik_opts(opts)
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self.lib.bmpc_ik_dev(self._h, B, int(n_seeds), ctypes.byref(o), ptr(pd), ptr(rd), ptr(q0), ptr(lo), ptr(hi),
                                  *out_args(IK_OUT, out), torch.cuda.current_stream(pd.device).cuda_stream or None)
        self._chk(rc, "bmpc_ik_dev")
        return out


    def _sets_opts(self, segment, fixed_mid, optimize):
        o = BmpcSetsOpts()
        self.lib.bmpc_default_sets_opts(ctypes.byref(o))
        o.segment, o.fixed_mid, o.optimize = int(bool(segment)), int(bool(fixed_mid)), int(bool(optimize))
        return o

    def convex_sets(self, obs_sets, obs_points_sets, e_min, e_max, p0, p1=None, fixed_mid=False, optimize=True):
        """Batched convex free-space sets (bmpc_convex_sets): point mode (p1 None) grows the set of
        ConvexSetFinder.find_set_around_point(p0[k], fixed_mid, optimize) around every row of p0 [B,3]; segment mode (p1 [B,3])
        the set of find_set_collision_avoidance(p0[k], p1[k], compute_ellipsoid=True).  Obstacles as ConvexSetFinder holds them;
        e_min / e_max: the workspace box.  Returns dict(A [B,20,3], b [B,20] (rows past nrows zero), nrows, q_ellipse [B,3,3],
        centre [B,3], rounds, newton, collision, status [B]) -- status 0 ok, else a code of SETS_STATUS."""
        sc = pack_set_scene(obs_sets, obs_points_sets)
        p0 = np.ascontiguousarray(p0, float).reshape(-1, 3)
        B = p0.shape[0]
        p1 = None if p1 is None else np.ascontiguousarray(p1, float).reshape(B, 3)
        e_min, e_max = (np.ascontiguousarray(e, float).reshape(3) for e in (e_min, e_max))
        out = out_arrays(SETS_OUT, B)
        o = self._sets_opts(p1 is not None, fixed_mid, optimize)
        I = lambda a: a.ctypes.data_as(_ip)
        rc = self.lib.bmpc_convex_sets(self._h, ctypes.byref(o), sc["n_obs"], _P(sc["A"]), _P(sc["b"]), I(sc["nrows"]), _P(sc["V"]),
                                       I(sc["nv"]), _P(e_min), _P(e_max), B, _P(p0), _P(p1), *out_args(SETS_OUT, out))
        self._chk(rc, "bmpc_convex_sets")
        return out

    def convex_sets_dev(self, scene, e_min, e_max, p0, p1=None, fixed_mid=False, optimize=True, out=None):
        """bmpc_convex_sets_dev on torch tensors of the GPU, enqueued on torch.cuda.current_stream() without waiting.  scene: dict of
        contiguous GPU tensors in the layout of scenes.pack_scene (A, b float64; nrows, nv int32; V float64) plus the int n_obs;
        e_min / e_max: [3] float64 GPU tensors; p0 / p1: [B,3] float64.  out: dict of preallocated result tensors (the keys of
        convex_sets) or None."""
        import torch
        B = p0.shape[0]
        f64, i32 = torch.float64, torch.int32
        chk = [("p0", p0, (B, 3), f64), ("p1", p1, (B, 3), f64), ("e_min", e_min, (3,), f64), ("e_max", e_max, (3,), f64)]
        for k in ("A", "b", "V"):
            chk.append((k, scene[k], tuple(scene[k].shape), f64))
        for k in ("nrows", "nv"):
            chk.append((k, scene[k], tuple(scene[k].shape), i32))
        for name, t, shape, dt in chk:
            if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape):
                raise ValueError(f"convex_sets_dev: {name} must be a contiguous {dt} GPU tensor of shape {shape}")
        if out is None:
            out = out_tensors(SETS_OUT, B, p0.device)
        o = self._sets_opts(p1 is not None, fixed_mid, optimize)
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self.lib.bmpc_convex_sets_dev(self._h, ctypes.byref(o), int(scene["n_obs"]), ptr(scene["A"]), ptr(scene["b"]),
                                           ptr(scene["nrows"]), ptr(scene["V"]), ptr(scene["nv"]), ptr(e_min), ptr(e_max), B, ptr(p0),
                                           ptr(p1), *out_args(SETS_OUT, out), torch.cuda.current_stream(p0.device).cuda_stream or None)
        self._chk(rc, "bmpc_convex_sets_dev")
        return out

    def sets_parts(self, mode, p, E=None, scene=None, rows=None):
        """Test entry bmpc_debug_sets_parts: one part of the set growth per item.  mode 0: one round of the polyhedron growth around
        p [B,3] in the metric E [B,3,3], scene = (obs_sets, obs_points_sets, e_min, e_max); mode 1 / 2: the inscribed ellipsoid with
        the centre fixed at p / free and started from p, rows = (A [B,20,3], b [B,20], m [B]).  Returns dict(A, b, nrows (mode 0: the
        row count or minus the status), q [B,3,3], c [B,3], newton, status)."""
        p = np.ascontiguousarray(p, float).reshape(-1, 3)
        B = p.shape[0]
        I = lambda a: a.ctypes.data_as(_ip) if a is not None else None
        sc = dict(n_obs=0, A=None, b=None, nrows=None, V=None, nv=None)
        e_min = e_max = rA = rb = rm = None
        if mode == 0:
            sc = pack_set_scene(scene[0], scene[1])
            e_min, e_max = (np.ascontiguousarray(e, float).reshape(3) for e in scene[2:])
            E = np.ascontiguousarray(E, float).reshape(B, 9)
        else:
            rA, rb = np.ascontiguousarray(rows[0], float).reshape(B, SETS_ROWS * 3), np.ascontiguousarray(rows[1], float).reshape(B, SETS_ROWS)
            rm = np.ascontiguousarray(rows[2], np.int32).reshape(B)
        out = dict(A=np.empty((B, SETS_ROWS, 3)), b=np.empty((B, SETS_ROWS)), nrows=np.empty(B, np.int32), q=np.empty((B, 3, 3)),
                   c=np.empty((B, 3)), newton=np.empty(B, np.int32), status=np.empty(B, np.int32))
        rc = self.lib.bmpc_debug_sets_parts(self._h, int(mode), sc["n_obs"], _P(sc["A"]), _P(sc["b"]), I(sc["nrows"]), _P(sc["V"]),
                                            I(sc["nv"]), _P(e_min), _P(e_max), B, _P(E), _P(p), _P(rA), _P(rb), I(rm), _P(out["A"]),
                                            _P(out["b"]), I(out["nrows"]), _P(out["q"]), _P(out["c"]), I(out["newton"]), I(out["status"]))
        self._chk(rc, "bmpc_debug_sets_parts")
        return out


class _DM:
    """Minimal stand-in for casadi.DM results: `.full()` and numpy conversion."""

    def __init__(self, a):
        self._a = np.asarray(a, float)

    def full(self):
        return self._a.reshape(-1, 1) if self._a.ndim == 1 else self._a

    def __array__(self, dtype=None):
        return self._a if dtype is None else self._a.astype(dtype)

    def __float__(self):
        return float(self._a)


class HipNlpSolver:
    """Call-compatible replacement of the CasADi nlpsol function object of BoundMPC.py:240-246:
    sol = solver(x0=, lbx=, ubx=, lbg=, ubg=, p=) -> {"x","g","lam_g","lam_x","f"}; solver.stats()."""

    def __init__(self, N, dt=0.1, backend=None, **kw):
        self.backend = backend or HipBoundMPC(N, dt=dt, **kw)
        self.lbg, self.ubg = self.backend.lbg, self.backend.ubg
        self._stats = {}

    def __call__(self, x0, lbx, ubx, p, lbg=None, ubg=None, **_):
        inf2big = lambda a: np.nan_to_num(np.asarray(a, float), posinf=1e20, neginf=-1e20)
        r = self.backend.solve_batch(np.asarray(x0, float)[None], inf2big(lbx)[None], inf2big(ubx)[None],
                                     np.asarray(p, float)[None], want_g=True, want_lam=True)
        st = int(r["status"][0])
        self._stats = {"iter_count": int(r["iters"][0]), "success": st == 0,
                       "return_status": ["Solve_Succeeded", "Maximum_Iterations_Exceeded",
                                         "Search_Direction_Becomes_Too_Small", "Error_In_Step_Computation"][st],
                       "g_viol": float(r["viol"][0]), "t_kernel_ms": self.backend.last_kernel_ms()}
        n_w, n_g = self.backend.n_w, self.backend.n_g
        return {"x": _DM(r["x"][0]), "g": _DM(r["g"][0]), "f": _DM(r["f"][0]),
                "lam_g": _DM(r["lam_g"][0] if r["lam_g"] is not None else np.zeros(n_g)),
                "lam_x": _DM(r["lam_x"][0] if r["lam_x"] is not None else np.zeros(n_w))}

    def stats(self):
        return dict(self._stats)


def default_ik_fn(robot=None):
    """Batched inverse kinematics backed by the HIP library (used by RobotModel when no ik_fn is given): a function
    (pd [B,3], rd [B,3,3], q0 [B,7], n_seeds=1) -> the dict of HipBoundMPC.ik."""
    be = HipBoundMPC(15, robot=robot)
    return lambda pd, rd, q0, n_seeds=1: be.ik(pd, rd, q0, n_seeds=n_seeds)


def default_sets_fn():
    """Batched convex free-space sets backed by the HIP library (ConvexSetFinder(..., sets_fn=) / BoundPlanner(..., set_backend=)):
    a function (obs_sets, obs_points_sets, e_min, e_max, p0 [B,3], p1=None, fixed_mid=False, optimize=True) -> the dict of
    HipBoundMPC.convex_sets."""
    be = HipBoundMPC(15)
    return be.convex_sets


def default_fk_fn():
    """Batched kinematics backed by the HIP library (used by RobotModel when no backend is given)."""
    be = HipBoundMPC(15)
    return lambda q, dq=None: be.fk(q, dq)
