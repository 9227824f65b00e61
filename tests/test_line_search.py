"""The filter line search of one interior-point iteration, pinned to an independent check (CPU half; tests/test_line_search_gpu.py
is the MI355X half).  tests/line_search_lib.py documents the reference, the acceptance rule, the cases, the classes of search and
the bounds.

What runs: emu_line_search (tests/emu/emu_pipe.cpp, the bodies of bmpc_debug_line_search) -- the Newton step's sequence, line-search
state planted before the evaluation bodies and after k_step, then the trial body once: k_trial_spec_body (what the GPU runs for
these batch sizes) and k_trial_body, which must agree bitwise.  Each case runs twice: the first run, with nothing planted, gives
zeta0, dzeta, t, c, from which the reference's ten trials and the planted state of every instance follow; the second is checked.

ORACLE_WORST (the oracle's own trial point, bmpc_oracle_trial_point, against the reference; worst per profile over all cases,
relative to the sum of the absolute terms; t1 / f / theta) as measured:
    (a) 2.4e-14 / 1.8e-15 / 7.1e-17      (b) 6.7e-13 / 3.3e-15 / 2.0e-16      (c) 5.2e-15 / 1.2e-15 / 1.5e-15
(t1 is relative to |t| + alpha |dt|, or to |h| where the slack reset acts: h is a difference of larger terms, hence 1e-14 and not 1e-16).

Reads the oracle library and the scene generator only.
"""
import numpy as np
import pytest

import emu_pipe_lib as E
import line_search_lib as L
import newton_step_lib as NS
import oracle_lib as O

NEWTON = ("dzeta", "dt", "dz", "state", "zeta0", "t0", "z0")


def _run(bt, P0=None, P1=None, variant=1, sub=None, cold=False):
    s = slice(None) if sub is None else sub
    rows = (None, None, None) if cold else (bt["TS"][s], bt["ZS"][s], bt["mode"][s])
    return E.line_search(bt["N"], bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], *rows,
                         plant0=None if P0 is None else P0[s], plant1=None if P1 is None else P1[s], variant=variant)


def same_search(a, b, live):
    """two runs of a search agree bitwise in everything but the slots of t1 that no row uses"""
    diff = [k for k in a if not (np.array_equal(a[k], b[k], equal_nan=True) if k != "t1" else np.array_equal(a["t1"][live], b["t1"][live]))]
    assert not diff, f"two runs of one search differ in {diff}"
    return True


@pytest.mark.parametrize("ci", range(len(L.CASES)))
def test_emulated_line_search_meets_the_reference(ci):
    N, B, profile, seed = L.CASES[ci]
    bt = NS.make_batch(N, B, seed, profile)
    first = _run(bt)
    P0, P1, info = L.plans_for(bt, profile, first, O, ci)
    out = _run(bt, P0, P1)
    for k in NEWTON:          # (state[0] is the planted iteration counter itself)
        a, b = (first[k], out[k]) if k != "state" else (first[k][:, 1:], out[k][:, 1:])
        assert np.array_equal(a, b, equal_nan=True), f"{k} depends on the planted line-search state"
    L.check_case(bt, profile, out, info, True, O, f"emulated k_trial_spec N={N} B={B} ({profile})", L.wanted_classes(ci, B))
    assert same_search(out, _run(bt, P0, P1, variant=0), bt["ZS"] > 0), "k_trial_body and k_trial_spec_body differ"
    if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
        ipw = 64 // (N - 1)
        for j in (0, ipw - 1, ipw, B - 1):
            alone = _run(bt, P0, P1, sub=slice(j, j + 1))
            assert same_search(alone, {k: v[j:j + 1] for k, v in out.items()}, bt["ZS"][j:j + 1] > 0), f"instance {j} alone differs from instance {j} of the batch"


def test_assembly_of_the_full_space_point():
    """w(zeta) once: the substituted equality rows of the pinned g (p = fk(q), v = J dq) vanish to rounding at it, the rows and
    defects of the reference equal bmpc_oracle_newton_system's h, r, r0 at the same point to 1e-13 relative -- a third statement
    of them --, and w(zeta) of a finished solve is the solver's returned x."""
    N, B, profile, seed = 6, 12, "b", 7106
    bt = NS.make_batch(N, B, seed, profile)
    out = _run(bt)
    gb = O.gbounds(N)
    for i in range(3):
        pt = L.Point(bt, i, out["zeta0"][i], O, gb)
        for k in range(N - 1):          # block k: rows 21..23 p_pos, 27..32 v of stage k + 1
            blk = pt.g[35 * k:35 * (k + 1)]
            assert np.abs(blk[21:24]).max() <= 1e-15 and np.abs(blk[27:33]).max() <= 1e-14
        sysd = O.newton_system(N, pt.w, bt["lbx"][i], bt["ubx"][i], bt["p"][i], bt["T"][i], bt["Z"][i], 0, 0.1, step=False)
        live = bt["slot"][i] >= 0
        assert np.array_equal(sysd["nrows"], bt["rows"][i][0])
        sc = lambda a: max(float(np.abs(a).max()), 1.0)
        assert float(np.abs(np.where(live, pt.h - sysd["h"], 0)).max()) <= 1e-13 * sc(sysd["h"])
        assert float(np.abs(pt.r - sysd["r"][:-1]).max()) <= 1e-13 * sc(out["zeta0"][i]) and float(np.abs(pt.r0 - sysd["r0"]).max()) <= 1e-13 * sc(out["zeta0"][i])
    sol = E.solve_batch(N, bt["x0"][:2], bt["lbx"][:2], bt["ubx"][:2], bt["p"][:2])
    for i in range(2):
        assert sol["status"][i] == 0
        x = sol["x"][i]
        T = HP_T(N)
        y = np.zeros((N - 1, 41))
        k = np.arange(1, N)
        for blk, name in enumerate(("q", "dq", "ddq", "u")):
            for j in range(7):
                y[:, L.YI[f"{name}{j}"]] = x[blk * 7 * N + j * N + k]
        fk = O.fk_batch(y[:, :7], y[:, 7:14])
        om = np.einsum("kaj,kj->ka", fk["jac"], y[:, 7:14])[:, 3:]
        for c in range(3):
            y[:, L.YI[f"pi{c}"]] = x[28 * N + (3 + c) * N + k] - 0.05 * om[:, c]
        for m, name in enumerate(("rs", "drs", "ps", "dps")):
            y[:, L.YI[name]] = x[(40 + m) * N + 6 + k]
        for c in range(6):
            y[:, L.YI[f"d{c}"]] = x[40 * N + c]
        zeta = np.linalg.solve(T, y.T).T
        w = L.w_of_zeta(N, zeta, bt["lbx"][i], O)[0]
        assert np.abs(w - x).max() <= 1e-12 * max(1.0, np.abs(x).max())


def HP_T(N, dt=0.1):
    import hessian_pin_lib as HP
    return HP.build_T(L.YN, dt)


def test_cold_start_pins_the_merit_pieces_of_the_init_launch():
    """t, z == NULL: the rows stay as the init launch made them and nothing is planted -- phi0, theta_max / theta_min (iteration 0)
    and the search are those of k_init's own f, theta, sum log t, which the reference recomputes from the returned zeta0, t0"""
    N, B, seed = L.COLD_CASE
    from boundplanner_amd import scenes
    b = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
    x0 = b["x0"] + 1e-2 * np.random.default_rng(seed + 2).normal(size=b["x0"].shape)
    st0 = np.arange(40) * N
    x0[:, st0] = b["lbx"][:, st0]
    bt = dict(N=N, B=B, x0=x0, lbx=b["lbx"], ubx=b["ubx"], p=b["p"])
    out = _run(bt, cold=True)
    L.check_cold(bt, out, O, f"emulated cold start N={N} B={B}")
    other = _run(bt, cold=True, variant=0)
    assert same_search(out, other, out["z0"] > 0)
