"""The batched inverse-kinematics kernel's iteration (csrc/bmpc_ik.hpp, CPU build: tests/emu/emu_ik.cpp) against the independent replay
of tests/ik_pin_lib.py: iters, status and seed exactly, q, cost and the two error figures within 32 x the replay's own sensitivity
to rounding, at every cut-off max_iter in {0, 1, 2, 3, 5, 8, 20}, on the iiwa14, the Gen3 and a generic table with no zero in it."""
import numpy as np
import pytest

import emu_ik_lib as E
import ik_pin_lib as P
import oracle_lib as O

TABLES = tuple(P.TABLES)


def run_on(tname):
    return lambda pd, rd, q0, n_seeds, lo, hi, **opts: E.ik(pd, rd, q0, n_seeds=n_seeds, lo=lo, hi=hi, robot=P.TABLES[tname], **opts)


def test_generic_table_has_no_special_entry():
    t = P.GENERIC
    for k in ("joint_xyz", "joint_rpy", "ee_xyz", "ee_rpy", "link4_col_xyz"):
        assert (np.asarray(t[k]) != 0).all(), k
    a = np.asarray(t["joint_rpy"])
    assert a.min() < -2.0 and a.max() > 2.0 and (np.abs(a) < 3.0).all()
    unlimited = np.asarray(t["q_upper"]) >= P.UNLIMITED
    assert unlimited.any() and not unlimited.all()


def test_recorded_gaps_cover_the_cases_and_no_lane_is_undecidable():
    """The double replay against the extended one on the very cases the tests run: same integers in every lane at every depth, every
    difference within the recorded REF_GAP (measured on sixteen times the sample), no comparison of any lane below its margin."""
    P.check_longdouble()
    for tname in TABLES:
        for kind in P.KINDS:
            cases = [c for c in P.truncated_cases(tname) if c["kind"] == kind]
            out, floor, differ = P.measure_gaps(cases)
            assert differ == 0, (tname, kind)
            for f in P.FLOATS:
                for m in P.DEPTHS:
                    assert out[f][m] <= P.REF_GAP[kind][f][m], (tname, kind, f, m, out[f][m])
            for f in P.DECS:
                assert floor[f] <= P.DEC_FLOOR[f], (tname, kind, f, floor[f])
            for c in cases:
                und = [P.undecidable_from(r, d) for r, d in zip(P.replays(c), P.replays(c, np.float64))]
                assert und == [None] * len(und), (c["name"], und)
    w = P.measure_model_gap()
    assert all(w[k] <= P.MODEL_GAP[k] for k in w), w


@pytest.mark.parametrize("tname", TABLES)
def test_model_is_r_jr_explicitly(tname):
    P.check_model(tname, E.model)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("tname", TABLES)
def test_truncated_solves(tname, kind):
    case = [c for c in P.truncated_cases(tname) if c["kind"] == kind][0]
    assert P.check_truncated(case, run_on(tname)) == 0


@pytest.mark.parametrize("tname", TABLES)
def test_every_halton_seed(tname):
    P.check_seeds(tname, run_on(tname))


@pytest.mark.parametrize("tname", TABLES)
def test_winner_order(tname):
    tie = P.seed_run(tname, run_on(tname))["q"][P.TIE_SEED - 1] if tname == "iiwa14" else None
    if tie is not None:                         # the seed point of the box does not depend on q0 when every joint is limited
        assert not (np.asarray(P.TABLES[tname]["q_upper"]) >= P.UNLIMITED).any()
    assert P.check_winner(tname, run_on(tname), tie) == 0


def test_fk_on_the_generic_table():
    """oracle_lib.fk_batch with the generic table against the plain chain: every key, 64 random q, dq, to 1e-12"""
    rng = np.random.default_rng(41)
    q, dq = rng.uniform(-3.0, 3.0, (64, 7)), rng.normal(size=(64, 7))
    O.set_robot(P.GENERIC)
    try:
        got = O.fk_batch(q, dq)
    finally:
        O.set_robot(None)
    P.check_fk(P.GENERIC, got, q, dq)
