"""What a solve returns when it stops short of a solution: x, g, f, viol, lam_g, lam_x of k_out / k_fin / k_mult / k_mult_sweep, pinned
to the full-space NLP at the returned point (shared by tests/test_solve_outputs.py, the CPU emulation of the kernel bodies, and
tests/test_solve_outputs_gpu.py, the kernels on the MI355X).  TEST INFRASTRUCTURE ONLY.

Reference: oracle_lib.nlp_eval (f, g, grad f, J_g of the NLP in the reference's layout, itself pinned to the reference's formulation
at 1e-12) and oracle_lib.gbounds; never the kernels' own rows.  viol is restated here from BoundMPC.py:613-615:
    viol = -sum g[g < lbg - 1e-6] + sum g[g > ubg + 1e-6]
and evaluated in long double.  loop_finish accepts a failed solve when viol < 1e-4 (ACCEPT), so viol matters where it is positive,
which it never is at a converged point.

Three families of points off the solution, all through the max_iter option alone:
  natural  cold starts of scenes.make_batch(randomize_sets=True) stopped after k = 1, 2, 5 iterations (status 1, iters k): violated
           inequality rows and, from N = 6 on, defects of the p_rot rows.  Their rs / ps rows stay at rounding: a cold start has
           rs = ps = 0 with zero rates and those rows are linear.
  planted  max_iter = 0: the solve returns the point it was given -- q, dq, ddq, u, dslack as they are, p_pos and v substituted from the
           kinematics.  x0 is integrated in long double from the stage-0 pins with random jerks (the jerk-integrator rows, p_rot, rs,
           ps rows vanish to rounding), with jumps planted into chosen states: plant_rows() x sign x {0.9e-6, 1.1e-6} (one row of g each,
           inside / outside the dead band, on the interior rows, the stage-0 -> 1 transition (the x1fix branch of k_out) and the last
           transition), then instances with several jumps of 1e-3 .. 1e-1 of mixed sign.  The slack variables are set wide (rs = ps =
           dslack = 1), so that no inequality row is violated and viol is the planted rows' alone.
  warm     the oracle's solution perturbed by 1e-3 in every entry, after 0 and 1 iterations: k_init takes p_rot, rs, ps of the stages
           >= 1 from x0, so at k = 0 every equality row group carries a defect, the rs and ps rows among them.

Bounds: g and f 1e-12 max(1, |.|) (the NLP pin's own tolerance); viol 1e-12 max(1, viol); multipliers: the stationarity residual
r = grad f + J_g^T lam_g + lam_x vanishes identically in every column an equality row carries its -1 on (q, dq, ddq, p, v, rs, ps of
the stages >= 1) and in the pinned stage-0 columns, whatever the iterate -- what is left sits on u, drs, dps, dslack.  The bound on
those structural zeros is 32 x ORACLE_WORST, the worst |r| / max(1, |lam_g|, |lam_x|, |grad f|) of the oracle's own
recover_multipliers (dense elimination on the pinned Jacobian) at the same max_iter, measured per family by oracle_worst() below and
rounded up.
"""
import numpy as np

LD = np.longdouble
BAND, ACCEPT, EDGE = 1e-6, 1e-4, 1e-9
TOL = 1e-12
KS = (1, 2, 5)

# (N, B, seed, robot): natural iterates.  CPU: one full and one ragged wavefront at N = 18; GPU: 32 instances per wavefront (N = 3), a
# ragged last wavefront at the N = 20 instantiation, one instance per wavefront (N = 64), the Gen3 (no bound rows on four joints)
CPU_CASES = ((3, 5, 3, None), (6, 6, 77, None), (18, 5, 193, None), (20, 4, 205, None))
GPU_CASES = ((3, 8, 3, None), (6, 32, 60, None), (20, 67, 225, None), (30, 24, 331, None), (64, 3, 644, None), (10, 8, 104, "gen3"))
# what the iterates of a case must show between them (measured with the oracle's iterates when the seeds were chosen): classes of viol --
# "zero": exactly 0 with status 1, "accepted": 0 < viol < 1e-4, a failed solve that loop_finish accepts, "rejected": viol > 1e-4 -- and
# "pi": a p_rot defect row beyond the dead band.  test_solve_outputs.py checks that each half's cases cover all of them.  The seeds
# are the ones of 20 .. 40 tried per case whose rows of g stay furthest from the edges of the dead band (5e-8 .. 9e-9 with the
# oracle's iterates; the check needs 1e-9).
WANTS = {(3, 5, 3, None): {"zero", "accepted", "rejected"}, (6, 6, 77, None): {"zero", "accepted", "rejected", "pi"},
         (18, 5, 193, None): {"rejected", "pi"}, (20, 4, 205, None): {"rejected", "pi"},
         (3, 8, 3, None): {"zero", "accepted", "rejected"}, (6, 32, 60, None): {"zero", "accepted", "rejected", "pi"},
         (20, 67, 225, None): {"rejected", "pi"}, (30, 24, 331, None): {"rejected", "pi"}, (64, 3, 644, None): {"rejected", "pi"},
         (10, 8, 104, "gen3"): {"rejected", "pi"}}
PLANT_N_CPU = (3, 6, 18, 20)
PLANT_N_GPU = (3, 6, 20, 30, 64)
WARM_N_CPU = (6, 18)
WARM_N_GPU = (3, 6, 20, 30)

# worst |r| / scale on the structural columns of the oracle's own multipliers (oracle_worst(), rounded up), per family
# (measured over both halves' cases: natural 4.33e-16 at N = 6, B = 32, k = 5; planted 1.79e-16 at N = 64; warm 8.75e-17 at N = 30, k = 1)
ORACLE_WORST = {"natural": 5e-16, "planted": 2e-16, "warm": 1e-16}
MULT_FACTOR = 32

GROUPS = ("q", "dq", "ddq")


def dims(N):
    return 44 * N + 6, 147 * (N - 1) + 21


def blocks(N):
    """column ranges of x by name"""
    return {"q": (0, 7 * N), "dq": (7 * N, 14 * N), "ddq": (14 * N, 21 * N), "u": (21 * N, 28 * N), "p": (28 * N, 34 * N),
            "v": (34 * N, 40 * N), "dslack": (40 * N, 40 * N + 6), "rs": (40 * N + 6, 41 * N + 6), "drs": (41 * N + 6, 42 * N + 6),
            "ps": (42 * N + 6, 43 * N + 6), "dps": (43 * N + 6, 44 * N + 6)}


def structural_columns(N):
    """columns of x in which r vanishes identically: the variable an equality row carries a -1 on, and the pinned stage 0"""
    n_w, _ = dims(N)
    m = np.zeros(n_w, bool)
    bl = blocks(N)
    for name in ("q", "dq", "ddq", "p", "v", "rs", "ps"):
        m[bl[name][0]:bl[name][1]] = True
    for f in range(28):                     # stage 0 of u (q, dq, ddq are set already)
        m[f * N] = True
    m[bl["drs"][0]] = m[bl["dps"][0]] = True
    return m


def free_columns(N):
    """(u of the stages >= 1, the slack rates drs, dps of the stages >= 1 and dslack): where the dual infeasibility sits"""
    n_w, _ = dims(N)
    bl = blocks(N)
    u = np.zeros(n_w, bool); s = np.zeros(n_w, bool)
    for j in range(7):
        u[bl["u"][0] + j * N + 1:bl["u"][0] + (j + 1) * N] = True
    s[bl["drs"][0] + 1:bl["drs"][1]] = True
    s[bl["dps"][0] + 1:bl["dps"][1]] = True
    s[bl["dslack"][0]:bl["dslack"][1]] = True
    assert not ((u | s) & structural_columns(N)).any() and ((u | s) | structural_columns(N)).all()
    return u, s


def row_masks(N):
    """masks over g: the substituted equality rows (p_pos, v of every block; rs, ps of block 0), the p_rot / rs / ps defect rows, the set rows"""
    _, n_g = dims(N)
    sub = np.zeros(n_g, bool); pi = np.zeros(n_g, bool); rs = np.zeros(n_g, bool); ps = np.zeros(n_g, bool); sets = np.zeros(n_g, bool)
    for k in range(N - 1):
        sub[35 * k + 21:35 * k + 24] = True
        sub[35 * k + 27:35 * k + 33] = True
        pi[35 * k + 24:35 * k + 27] = True
        if k > 0:
            rs[35 * k + 33] = True; ps[35 * k + 34] = True
    sub[33] = sub[34] = True
    for k in range(1, N):
        g0 = 35 * (N - 1) + 112 * (k - 1)
        sets[g0:g0 + 15] = True
        sets[g0 + 21:g0 + 111] = True
        if k == N - 1:
            sets[g0 + 112:g0 + 127] = True
    return dict(sub=sub, pi=pi, rs=rs, ps=ps, sets=sets)


def viol_formula(g, lbg, ubg):
    """BoundMPC.py:613-615 in long double"""
    g = np.asarray(g, LD)
    return -g[g < np.asarray(lbg, LD) - LD(BAND)].sum() + g[g > np.asarray(ubg, LD) + LD(BAND)].sum()


def viol_class(viol):
    return "zero" if viol == 0.0 else ("accepted" if viol < ACCEPT else "rejected")


CLASSES = {"zero", "accepted", "rejected"}


def check_point(N, p, gb, out, i, label):
    """x, g, f, viol of instance i against the NLP at the returned x.  Returns (reference g, dict of the worst figures)."""
    lbg, ubg = gb
    x, g, f, viol = out["x"][i], out["g"][i], float(out["f"][i]), float(out["viol"][i])
    assert np.isfinite(x).all() and np.isfinite(g).all() and np.isfinite(f) and np.isfinite(viol), f"{label}[{i}]: not finite"
    fr, gr, _, _ = NLP.nlp_eval(N, x, p, jac=False)
    fig = {}
    fig["g"] = float(np.abs(g - gr).max()) / max(1.0, float(np.abs(gr).max()))
    fig["f"] = abs(f - fr) / max(1.0, abs(fr))
    # condition on the inputs: no row of the reference g on an edge of the dead band
    edge = float(np.abs(np.abs(gr) - BAND).min())
    assert edge >= EDGE, f"{label}[{i}]: a row of the reference g lies {edge:.1e} from the dead band's edge: take another seed"
    vr = viol_formula(gr, lbg, ubg)
    vg = viol_formula(g, lbg, ubg)
    fig["viol"] = float(abs(LD(viol) - vr)) / max(1.0, float(vr))
    fig["viol_g"] = float(abs(LD(viol) - vg)) / max(1.0, float(vg))
    for k, v in fig.items():
        assert v <= TOL, f"{label}[{i}]: {k} misses the NLP at the returned point: {v:.2e} > {TOL:.0e} (viol {viol!r}, reference {float(vr)!r})"
    if vr == 0:
        assert viol == 0.0, f"{label}[{i}]: viol {viol!r} where every row lies inside the dead band"
    M = row_masks(N)
    assert (g[M["sub"]] == 0.0).all(), f"{label}[{i}]: a substituted equality row of g is not exactly zero"
    return gr, fig


def padding_rows(N, J):
    """set rows of g whose normal is zero (the sets' padding): they hold -b - slack"""
    M = row_masks(N)
    pad = np.zeros(J.shape[0], bool)
    idx = np.flatnonzero(M["sets"])
    pad[idx] = np.abs(J[idx, :40 * N]).sum(axis=1) == 0.0
    return pad


def check_multipliers(N, p, gb, out, i, bound, label):
    """lam_g, lam_x of instance i: structural zeros of r, something left on u and on a slack rate, signs, padding rows, finite; the
    padding rows of g.  Returns (|r| / scale on the structural columns, whether r is beyond rounding on a slack rate -- drs, dps, dslack:
    an instance that has just taken a full step has nothing left there, so that is a condition on the batch, some_slack_rate())."""
    lbg, ubg = gb
    x, lg, lx = out["x"][i], out["lam_g"][i], out["lam_x"][i]
    assert np.isfinite(lg).all() and np.isfinite(lx).all(), f"{label}[{i}]: multipliers not finite"
    upper = (ubg == 0) & (lbg < -1e19)
    lower = (lbg == 0) & (ubg > 1e19)
    assert (upper | lower | ((lbg == 0) & (ubg == 0))).all()
    assert (lg[upper] >= 0).all() and (lg[lower] <= 0).all(), f"{label}[{i}]: sign of an inequality multiplier"
    _, gr, grad, J = NLP.nlp_eval(N, x, p)
    r = grad + J.T @ lg + lx
    scale = max(1.0, float(np.abs(lg).max()), float(np.abs(lx).max()), float(np.abs(grad).max()))
    S = structural_columns(N)
    worst = float(np.abs(r[S]).max()) / scale
    assert worst <= bound, f"{label}[{i}]: stationarity in the structural columns {worst:.2e} > {bound:.2e} (column {int(np.flatnonzero(S)[np.abs(r[S]).argmax()])})"
    u, s = free_columns(N)
    # (elsewhere r is not rounding: the zeros above are the sweep's doing, not a residual that has vanished everywhere)
    floor = 1e3 * bound * scale
    assert np.abs(r[u]).max() > floor, f"{label}[{i}]: no dual infeasibility left on u: the check would pass on zeros"
    slack = bool(np.abs(r[s]).max() > floor)
    pad = padding_rows(N, J)
    assert pad.any() and (lg[pad] == 0.0).all(), f"{label}[{i}]: multiplier on a padding row"
    if out.get("g") is not None:
        assert np.array_equal(out["g"][i][pad], gr[pad]), f"{label}[{i}]: a padding row of g is not -b - slack"
    return worst, slack


def some_slack_rate(flags, label):
    assert any(flags), f"{label}: no instance with dual infeasibility on a slack rate"


def same_outputs(a, b, keys=("x", "f", "viol", "iters", "status"), rows=None):
    """b is bitwise a (or the rows `rows` of a)"""
    diff = [k for k in keys if not np.array_equal(a[k] if rows is None else a[k][rows], b[k])]
    assert not diff, f"outputs differ in {diff}"


# ------------------------------------------------------------------------------------------------------------------------------
# natural iterates
# ------------------------------------------------------------------------------------------------------------------------------
_batches = {}


def natural_batch(case):
    from boundplanner_amd import robots, scenes
    if case not in _batches:
        N, B, seed, robot = case
        table = {"gen3": robots.GEN3}.get(robot)
        b = scenes.make_batch(B, N, seed, NLP.fk_batch, randomize_sets=True, robot=table)
        _batches[case] = tuple(b[k] for k in ("x0", "lbx", "ubx", "p"))
    return _batches[case]


def check_natural(solve, case, label, report=print, pool=None, pool_ks=KS):
    """solve(N, x0, lbx, ubx, p, max_iter=, want_g=, want_lam=) -> the dict of HipBoundMPC.solve_batch.  Every k of the case: each
    instance against the NLP; without g and multipliers bitwise the same; instances alone bitwise themselves.  Over the k: the classes
    of viol and the defect of the p_rot rows that WANTS names for the case.  pool = (solve through a pool of slots, slots): the batch,
    repeated until it has more rows than slots, streams through the pool (k_out on partial done lists) bitwise the same."""
    N, B, seed, robot = case
    a = natural_batch(case)
    gb = NLP.gbounds(N)
    M = row_masks(N)
    pi_seen, classes, outs = False, set(), {}
    for k in (KS if robot is None else (2,)):
        out = solve(N, *a, max_iter=k, want_g=True, want_lam=True)
        assert (out["status"] == 1).all() and (out["iters"] == k).all(), f"{label} k={k}: not every instance stopped at the limit: {out['status']}, {out['iters']}"
        worst = dict(g=0.0, f=0.0, viol=0.0, viol_g=0.0, mult=0.0)
        cl, slack = [], []
        for i in range(B):
            gr, fig = check_point(N, a[3][i], gb, out, i, f"{label} k={k}")
            for key, v in fig.items():
                worst[key] = max(worst[key], v)
            pi_seen = pi_seen or bool((np.abs(gr[M["pi"]]) > BAND).any())
            cl.append(viol_class(float(out["viol"][i])))
            w, sl = check_multipliers(N, a[3][i], gb, out, i, MULT_FACTOR * ORACLE_WORST["natural"], f"{label} k={k}")
            worst["mult"] = max(worst["mult"], w); slack.append(sl)
        classes |= set(cl)
        some_slack_rate(slack, f"{label} k={k}")
        report(f"{label} k={k}: worst g {worst['g']:.1e} f {worst['f']:.1e} viol {worst['viol']:.1e} viol(g) {worst['viol_g']:.1e} (bound {TOL:.0e}); "
               f"structural zeros {worst['mult']:.1e} (bound {MULT_FACTOR * ORACLE_WORST['natural']:.1e}); viol {out['viol'].min():.2e} .. {out['viol'].max():.2e}, "
               f"classes {sorted(set(cl))}")
        # output modes: without g (the device loop's path) and without multipliers, bitwise; an instance alone
        same_outputs(out, solve(N, *a, max_iter=k, want_g=False, want_lam=False))
        ipw = max(1, 64 // (N - 1))
        for j in sorted({0, min(ipw, B - 1), B - 1}) if k == 2 else ():
            alone = solve(N, *(v[j:j + 1] for v in a), max_iter=k, want_g=True, want_lam=True)
            same_outputs(out, alone, keys=("x", "g", "f", "viol", "iters", "status", "lam_g", "lam_x"), rows=slice(j, j + 1))
        if pool is not None and k in pool_ks:
            reps = pool[1] // B + 1
            streamed = pool[0](N, *(np.tile(v, (reps, 1)) for v in a), max_iter=k, want_g=True, want_lam=False)
            for key in ("x", "g", "f", "viol", "iters", "status"):
                assert np.array_equal(streamed[key], np.concatenate([out[key]] * reps)), f"{label} k={k}: {key} differs through a pool of {pool[1]} slots"
        outs[k] = out
    want = WANTS[case]
    missing = (want & CLASSES) - classes
    assert not missing, f"{label}: no instance with viol of the classes {sorted(missing)}"
    assert pi_seen or "pi" not in want, f"{label}: no p_rot row beyond the dead band"
    return outs


# ------------------------------------------------------------------------------------------------------------------------------
# stopped warm starts: the oracle's solution perturbed by 1e-3, after k = 0 and k = 1 iterations
# ------------------------------------------------------------------------------------------------------------------------------
def warm_batch(N, seed=7, B=4):
    from boundplanner_amd import scenes
    key = ("warm", N, seed, B)
    if key not in _batches:
        b = scenes.make_batch(B, N, seed, NLP.fk_batch, randomize_sets=True)
        sol = NLP.solve_batch(N, b["x0"], b["lbx"], b["ubx"], b["p"], nthreads=1)
        assert (sol["status"] == 0).all()
        x0 = sol["x"] + 1e-3 * np.random.default_rng(seed).normal(size=sol["x"].shape)
        x0 = np.where(b["lbx"] == b["ubx"], b["lbx"], x0)
        _batches[key] = (x0, b["lbx"], b["ubx"], b["p"])
    return _batches[key]


def check_warm(solve, N, label, report=print):
    """max_iter = 0: q, dq, ddq, u, dslack come back to 1e-15 (p_pos and v are substituted, rs_0 / ps_0 eliminated); the p_rot, rs and
    ps rows carry the perturbation -- a cold start has rs = ps = 0 with zero rates and the rs / ps rows are linear, so that no
    iterate of a cold start ever leaves them: this family is where they are not zero.  max_iter = 1: the same rows after one step."""
    a = warm_batch(N)
    x0, p = a[0], a[3]
    B = x0.shape[0]
    gb = NLP.gbounds(N)
    M = row_masks(N)
    for k in (0, 1):
        out = solve(N, *a, max_iter=k, want_g=True, want_lam=True)
        assert (out["status"] == 1).all() and (out["iters"] == k).all()
        if k == 0:
            for name in ("q", "dq", "ddq", "u", "dslack"):
                lo, hi = blocks(N)[name]
                d = float(np.abs(out["x"][:, lo:hi] - x0[:, lo:hi]).max())
                assert d <= 1e-15, f"{label}: zero iterations moved {name} by {d:.1e}"
        worst = dict(g=0.0, f=0.0, viol=0.0, viol_g=0.0, mult=0.0)
        seen = {"pi": 0.0, "rs": 0.0, "ps": 0.0}
        slack = []
        for i in range(B):
            gr, fig = check_point(N, p[i], gb, out, i, f"{label} k={k}")
            for key, v in fig.items():
                worst[key] = max(worst[key], v)
            for key in seen:
                seen[key] = max(seen[key], float(np.abs(gr[M[key]]).max()))
            w, sl = check_multipliers(N, p[i], gb, out, i, MULT_FACTOR * ORACLE_WORST["warm"], f"{label} k={k}")
            worst["mult"] = max(worst["mult"], w); slack.append(sl)
        assert min(seen.values()) > BAND or k > 0, f"{label} k={k}: defects of the p_rot / rs / ps rows {seen}"     # (a full step closes the linear rs / ps rows)
        some_slack_rate(slack, f"{label} k={k}")
        assert (out["viol"] > ACCEPT).all()
        report(f"{label} k={k}: worst g {worst['g']:.1e} f {worst['f']:.1e} viol {worst['viol']:.1e} viol(g) {worst['viol_g']:.1e} (bound {TOL:.0e}); "
               f"structural zeros {worst['mult']:.1e} (bound {MULT_FACTOR * ORACLE_WORST['warm']:.1e}); largest p_rot / rs / ps defect "
               f"{seen['pi']:.1e} / {seen['rs']:.1e} / {seen['ps']:.1e}")
        same_outputs(out, solve(N, *a, max_iter=k, want_g=False, want_lam=False))


# ------------------------------------------------------------------------------------------------------------------------------
# planted points
# ------------------------------------------------------------------------------------------------------------------------------
def integrate(N, lbx, u, jumps, dt=0.1):
    """x [n_w]: the jerk integrator (casadi_ocp_formulation.py:145-164: hat-function jerk) from the stage-0 pins lbx[stage 0] with
    the jerks u [7][N] (u[:, 0] is the pin), in long double; jumps: {(group, j, k): d} subtracts d from state `group` of joint j at
    stage k before the integration goes on, so that row (group, j) of block k - 1 becomes d and no other row changes.  p_rot follows
    the trapezoidal rule on the angular velocity, p_pos and v are the kinematics, rs = ps = dslack = 1 with zero rates."""
    n_w, _ = dims(N)
    bl = blocks(N)
    d = LD(dt)
    c3a, c3b, c2a, c2b = d ** 3 / 8, d ** 3 / 24, d ** 2 / 3, d ** 2 / 6
    q, dq, ddq = (np.zeros((7, N), LD) for _ in range(3))
    u = np.asarray(u, LD)
    for blk, arr in enumerate((q, dq, ddq)):
        arr[:, 0] = lbx[blk * 7 * N + np.arange(7) * N]
    assert np.array_equal(np.asarray(u[:, 0], float), lbx[21 * N + np.arange(7) * N])
    for k in range(N - 1):
        q[:, k + 1] = ddq[:, k] * d * d / 2 + dq[:, k] * d + q[:, k] + u[:, k] * c3a + u[:, k + 1] * c3b
        dq[:, k + 1] = ddq[:, k] * d + dq[:, k] + u[:, k] * c2a + u[:, k + 1] * c2b
        ddq[:, k + 1] = ddq[:, k] + u[:, k] * d / 2 + u[:, k + 1] * d / 2
        for (grp, j, kk), dj in jumps.items():
            if kk == k + 1:
                {"q": q, "dq": dq, "ddq": ddq}[grp][j, kk] -= LD(dj)
        # the states the solver sees are doubles: go on from the rounded ones
        q[:, k + 1], dq[:, k + 1], ddq[:, k + 1] = (np.asarray(np.asarray(a[:, k + 1], float), LD) for a in (q, dq, ddq))
    x = np.zeros(n_w)
    for blk, arr in enumerate((q, dq, ddq, u)):
        x[blk * 7 * N:(blk + 1) * 7 * N] = np.asarray(arr, float).reshape(-1)
    fk = NLP.fk_batch(np.asarray(q, float).T, np.asarray(dq, float).T)
    v = np.einsum("kaj,kj->ka", fk["jac"], np.asarray(dq, float).T)          # [N][6]
    v[0] = lbx[34 * N + np.arange(6) * N]
    prot = np.zeros((N, 3), LD)
    prot[0] = lbx[28 * N + (3 + np.arange(3)) * N]
    for k in range(N - 1):
        prot[k + 1] = np.asarray(np.asarray(prot[k] + d / 2 * (np.asarray(v[k, 3:], LD) + np.asarray(v[k + 1, 3:], LD)), float), LD)
    for c in range(3):
        x[28 * N + c * N:28 * N + (c + 1) * N] = fk["ee_pos"][:, c]
        x[28 * N + (3 + c) * N:28 * N + (4 + c) * N] = np.asarray(prot[:, c], float)
    for c in range(6):
        x[34 * N + c * N:34 * N + (c + 1) * N] = v[:, c]
    for c in range(3):
        x[28 * N + c * N] = lbx[28 * N + c * N]
    x[bl["dslack"][0]:bl["dslack"][1]] = 1.0
    x[bl["rs"][0]:bl["rs"][1]] = 1.0
    x[bl["ps"][0]:bl["ps"][1]] = 1.0
    return x


def plant_rows(N):
    """(group, joint, stage whose state jumps): one row each of q, dq, ddq in an interior block, the same in block 0 (stage 0 -> 1: the
    x1fix branch of k_out) and one in the last block"""
    ki = max(2, N // 2) if N > 3 else N - 1          # stage after an interior transition (N = 3 has none: the last one)
    rows = [(g_, j, ki) for g_, j in zip(GROUPS, (1, 4, 6))]
    rows += [(g_, j, 1) for g_, j in zip(GROUPS, (0, 3, 5))]
    rows.append(("dq", 2, N - 1))
    return rows


def row_of(N, grp, j, k):
    """index in g of the defect row of state `grp`, joint j, between the stages k - 1 and k"""
    return 35 * (k - 1) + 7 * GROUPS.index(grp) + j


_plants = {}


def planted_batch(N, seed=None, nbase=4):
    """(x0, lbx, ubx, p, info): info[i] = dict(rows {g index: planted value}, single = (index, value) or None)"""
    from boundplanner_amd import scenes
    seed = 100 + N if seed is None else seed
    if (N, seed) in _plants:
        return _plants[(N, seed)]
    b = scenes.make_batch(nbase, N, seed, NLP.fk_batch, randomize_sets=True)
    rng = np.random.default_rng(seed + 1)
    cases = []
    for row in plant_rows(N):
        for s in (1.0, -1.0):
            for m in (0.9, 1.1):
                cases.append({row: s * BAND * m})
    allrows = [(g_, j, k) for g_ in GROUPS for j in range(7) for k in range(1, N)]
    for c in range(8):
        pick = rng.choice(len(allrows), size=min(len(allrows), 3 + c), replace=False)
        js = {allrows[i]: float(rng.choice((-1.0, 1.0)) * 10 ** rng.uniform(-3, -1)) for i in pick}
        if c % 2 == 0:
            js[("q", int(rng.integers(7)), 1)] = float(rng.choice((-1.0, 1.0)) * 10 ** rng.uniform(-3, -1))      # (the x1fix branch among them)
        cases.append(js)
    B = len(cases)
    n_w, _ = dims(N)
    x0 = np.zeros((B, n_w)); info = []
    sel = np.arange(B) % nbase
    lbx, ubx, p = b["lbx"][sel].copy(), b["ubx"][sel].copy(), b["p"][sel].copy()
    for i, jumps in enumerate(cases):
        ulim = np.minimum(np.abs(lbx[i][21 * N + np.arange(7) * N + 1]), np.abs(ubx[i][21 * N + np.arange(7) * N + 1]))
        ulim = np.where(np.isfinite(ulim) & (ulim < 1e19), ulim, 1.0)
        amp = np.minimum(0.2 * ulim, 0.2 / (N * 0.1) ** 3)          # inside the limits, and the arm stays where the scene's rows hold
        u = rng.uniform(-1, 1, (7, N)) * amp[:, None]
        u[:, 0] = lbx[i][21 * N + np.arange(7) * N]
        x0[i] = integrate(N, lbx[i], u, jumps)
        rows = {row_of(N, *key): val for key, val in jumps.items()}
        info.append(dict(rows=rows, single=next(iter(rows.items())) if len(rows) == 1 else None))
    _plants[(N, seed)] = (x0, lbx, ubx, p, info)
    return _plants[(N, seed)]


def check_planted(solve, N, label, report=print):
    """Returns the classes of viol seen."""
    x0, lbx, ubx, p, info = planted_batch(N)
    B = x0.shape[0]
    gb = NLP.gbounds(N)
    lbg, ubg = gb
    out = solve(N, x0, lbx, ubx, p, max_iter=0, want_g=True, want_lam=True)
    assert (out["status"] == 1).all() and (out["iters"] == 0).all(), f"{label}: {out['status']}, {out['iters']}"
    worst = dict(g=0.0, f=0.0, viol=0.0, viol_g=0.0, mult=0.0, row=0.0)
    classes, slack = [], []
    for name in ("q", "dq", "ddq", "u", "dslack"):
        lo, hi = blocks(N)[name]
        assert np.abs(out["x"][:, lo:hi] - x0[:, lo:hi]).max() <= 1e-15, f"{label}: zero iterations moved {name}"
    for i in range(B):
        gr, fig = check_point(N, p[i], gb, out, i, label)
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        # the construction: the planted rows hold the planted values, every other row lies inside the dead band
        rows = info[i]["rows"]
        idx = np.array(sorted(rows))
        val = np.array([rows[r] for r in idx])
        d = float(np.abs(gr[idx] - val).max())
        worst["row"] = max(worst["row"], d)
        assert d <= 1e-13, f"{label}[{i}]: the planted rows of the reference g miss their values by {d:.1e}"
        rest = np.ones(gr.shape, bool); rest[idx] = False
        clean = viol_formula(np.where(rest, gr, 0.0), lbg, ubg) == 0
        viol = float(out["viol"][i])
        if info[i]["single"] is not None:
            r, t = info[i]["single"]
            assert clean, f"{label}[{i}]: a row that was not planted is violated"
            if abs(t) < BAND:                 # 0.9e-6: inside the dead band, contributes nothing
                assert viol == 0.0, f"{label}[{i}]: a row of {t:.1e} (g index {r}) contributes {viol!r}"
            else:                             # 1.1e-6: its full value, not its excess over the dead band
                assert abs(viol - abs(gr[r])) <= TOL, f"{label}[{i}]: a row of {gr[r]!r} (g index {r}) contributes {viol!r}"
                assert 0 < viol < ACCEPT
        else:
            assert viol > ACCEPT and viol >= float(np.abs(gr[idx]).sum()) * (1 - TOL)
            assert not clean or abs(viol - float(np.abs(gr[idx]).sum())) <= TOL * max(1.0, viol)
        classes.append(viol_class(viol))
        w, sl = check_multipliers(N, p[i], gb, out, i, MULT_FACTOR * ORACLE_WORST["planted"], label)
        worst["mult"] = max(worst["mult"], w); slack.append(sl)
    assert set(classes) == CLASSES, f"{label}: classes of viol {sorted(set(classes))}"
    some_slack_rate(slack, label)
    report(f"{label}: worst g {worst['g']:.1e} f {worst['f']:.1e} viol {worst['viol']:.1e} viol(g) {worst['viol_g']:.1e} (bound {TOL:.0e}); "
           f"planted rows off by {worst['row']:.1e}; structural zeros {worst['mult']:.1e} (bound {MULT_FACTOR * ORACLE_WORST['planted']:.1e})")
    bare = solve(N, x0, lbx, ubx, p, max_iter=0, want_g=False, want_lam=False)
    same_outputs(out, bare)
    for j in (1, B - 1):
        alone = solve(N, x0[j:j + 1], lbx[j:j + 1], ubx[j:j + 1], p[j:j + 1], max_iter=0, want_g=True, want_lam=True)
        same_outputs(out, alone, keys=("x", "g", "f", "viol", "iters", "status", "lam_g", "lam_x"), rows=slice(j, j + 1))
    return out, classes


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle's own multipliers: what ORACLE_WORST is measured with
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_structural_residual(N, x0, lbx, ubx, p, max_iter):
    """worst |r| / max(1, |lam_g|, |lam_x|, |grad f|) on the structural columns of the oracle's recover_multipliers"""
    S = structural_columns(N)
    worst = 0.0
    for i in range(x0.shape[0]):
        o = NLP.solve(N, x0[i], lbx[i], ubx[i], p[i], max_iter=max_iter)
        _, _, grad, J = NLP.nlp_eval(N, o["x"], p[i])
        r = grad + J.T @ o["lam_g"] + o["lam_x"]
        scale = max(1.0, float(np.abs(o["lam_g"]).max()), float(np.abs(o["lam_x"]).max()), float(np.abs(grad).max()))
        worst = max(worst, float(np.abs(r[S]).max()) / scale)
    return worst


def oracle_worst(cases, plant_ns, warm_ns, report=print):
    nat = pl = 0.0
    for case in cases:
        if case[3] is not None:
            from boundplanner_amd import robots
            NLP.set_robot(robots.GEN3)
        try:
            for k in (KS if case[3] is None else (2,)):
                w = oracle_structural_residual(case[0], *natural_batch(case), max_iter=k)
                report(f"natural {case} k={k}: {w:.2e}")
                nat = max(nat, w)
        finally:
            NLP.set_robot(None)
    wm = 0.0
    for N in plant_ns:
        w = oracle_structural_residual(N, *planted_batch(N)[:4], max_iter=0)
        report(f"planted N={N}: {w:.2e}")
        pl = max(pl, w)
    for N in warm_ns:
        for k in (0, 1):
            w = oracle_structural_residual(N, *warm_batch(N), max_iter=k)
            report(f"warm N={N} k={k}: {w:.2e}")
            wm = max(wm, w)
    return {"natural": nat, "planted": pl, "warm": wm}


import oracle_lib as NLP          # noqa: E402  (the pinned NLP, its bounds, the kinematics and the oracle's solves)
