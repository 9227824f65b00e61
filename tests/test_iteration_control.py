"""The KKT error and the iteration control of one interior-point iteration, pinned to an independent check (CPU half;
tests/test_iteration_control_gpu.py is the MI355X half).  tests/iteration_control_lib.py documents the reference, the rule, the cases,
the classes and the bounds.

What runs: emu_iteration_control (tests/emu/emu_pipe.cpp, the bodies of bmpc_debug_iteration_control) -- the line-search entry's
sequence with the iteration-control state planted per instance and copied out after k_step and after the trial body -- with both
Riccati variants (k_ric_body; k_ric_att_body + k_ric_body<RESUME>), which must agree bitwise in every returned control field, and the
oracle's own bmpc_oracle_kkt_control, which must decide as the rule does.  Every case runs under each of its settings (the handle's
tol, max_iter, mu_floor_k, dw0) with that setting's planted states.

For the profiles of iteration_control_lib.NO_ATTEMPTS ("x", "d": exact solutions) delta_w, tries, gn_back, gn_skip, dw_last and hess_mode
after the search are not compared (the library's docstring says why); for every other profile they are.

Reads the oracle library and the scene generator only.
"""
import numpy as np
import pytest

import emu_pipe_lib as E
import iteration_control_lib as IC
import oracle_lib as O


def _run(bt, plant, o, variant=0, sub=None):
    s = slice(None) if sub is None else sub
    return E.iteration_control(bt["N"], bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], bt["TS"][s], bt["ZS"][s], bt["mode"][s], plant[s],
                               tol=o["tol"], max_iter=o["max_iter"], mu_floor_k=o["mu_floor_k"], dw0=o["dw0"], variant=variant)


def same(a, b, live):
    """two runs agree bitwise in everything but the slots of t1 that no row uses"""
    return [k for k in a if not (np.array_equal(a[k], b[k], equal_nan=True) if k != "t1" else np.array_equal(a["t1"][live], b["t1"][live]))]


@pytest.mark.parametrize("ci", range(len(IC.ALL_CASES)))
def test_emulated_iteration_control_meets_the_reference(ci):
    N, B, profile, seed = IC.ALL_CASES[ci]
    bt = IC.make_batch(N, B, seed, profile, O)
    reached = set()
    for setting in IC.SETTINGS_OF(N, profile):
        o, plant = IC.opts_of(setting), IC.plant_for(setting, ci, B, bt)
        out = _run(bt, plant, o)
        ms, cls = IC.check_case(bt, profile, out, plant, o, O, f"emulated k_ric N={N} B={B} ({profile}) {setting}")
        reached |= cls
        spec = _run(bt, plant, o, variant=1)
        assert np.array_equal(out["ctl"][:, IC.CONTROL], spec["ctl"][:, IC.CONTROL]), f"{setting}: k_ric_body and the speculative pair differ in the control state"
        assert np.array_equal(out["state"], spec["state"]) and np.array_equal(out["ls"], spec["ls"], equal_nan=True)
        if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
            ipw = 64 // (N - 1)
            for j in (0, ipw - 1, ipw, B - 1):
                alone = _run(bt, plant, o, sub=slice(j, j + 1))
                diff = same(alone, {k: v[j:j + 1] for k, v in out.items()}, bt["ZS"][j:j + 1] > 0)
                assert not diff, f"instance {j} alone differs from instance {j} of the batch in {diff}"
    print(f"case {ci}: classes {sorted(reached)}", flush=True)
    missing = set(IC.CASE_CLASSES[ci]) - reached
    assert IC.CASE_CLASSES[ci] and not missing, f"case {ci} N={N} B={B} ({profile}): classes {sorted(missing)} did not occur: the case tests nothing of its own"


def test_planting_nothing_is_the_line_search_entry():
    """ctl_plant of NaN leaves the state as the init launch and the mode made it: everything the line-search entry returns is bitwise
    what emu_line_search returns on the same inputs (k_ric_body, k_trial_spec_body)"""
    N, B, profile, seed = 4, 5, "b", 7104
    bt = IC.make_batch(N, B, seed, profile, O)
    out = _run(bt, np.full((B, 8), np.nan), IC.OPTS)
    ls = E.line_search(N, bt["x0"], bt["lbx"], bt["ubx"], bt["p"], bt["TS"], bt["ZS"], bt["mode"], variant=1)
    diff = same({k: v for k, v in out.items() if k != "ctl"}, ls, bt["ZS"] > 0)
    assert not diff, diff
    assert np.array_equal(out["ctl"][:, IC.CTL["mu"]], out["state"][:, 2]) and np.array_equal(out["ctl"][:, IC.CTL["delta_w"]], out["state"][:, 6])


@pytest.mark.parametrize("ci", range(len(IC.FD_CASES)))
def test_first_order_pieces_of_the_oracle_meet_differences(ci):
    """gdual and the pi rows of A, B of bmpc_oracle_newton_system -- what dual and lamsum of the reference are formed from -- against
    Richardson-extrapolated central differences of the pinned f, rows and kinematics (iteration_control_lib.first_order_check)"""
    N, B, profile, seed = IC.FD_CASES[ci]
    bt = IC.make_batch(N, B, seed, profile, O)
    out = _run(bt, np.full((B, 8), np.nan), IC.OPTS)
    gb = O.gbounds(N)
    for i in range(B):
        sysd = O.newton_system(N, bt["x0"][i], bt["lbx"][i], bt["ubx"][i], bt["p"][i], bt["T"][i], bt["Z"][i], int(bt["mode"][i] != 0), 0.1, step=False)
        w = IC.first_order_check(bt, i, out["zeta0"][i], sysd, O, gb)
        print(f"N={N} ({profile}) instance {i}: oracle / tolerance gdual {w['gdual']:.2g}, pi rows of A, B {w['AB']:.2g}", flush=True)
        assert w["gdual"] <= 1.0 and w["AB"] <= 1.0, f"N={N} ({profile}) instance {i}: {w}"


def test_every_class_is_reached_somewhere():
    have = set().union(*IC.CASE_CLASSES.values())
    assert set(IC.CLASSES) <= have, sorted(set(IC.CLASSES) - have)
