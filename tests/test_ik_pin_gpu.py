"""The HIP inverse-kinematics kernel (bmpc_ik through HipBoundMPC.ik) against the independent replay of tests/ik_pin_lib.py: the cases,
bounds and integer equalities of tests/test_ik_pin.py, on handles with robot=None, "gen3" and the generic table.  One case also
through ik_dev, bitwise equal to ik; HipBoundMPC.fk on the generic table against the plain chain."""
import numpy as np
import pytest

import ik_pin_lib as P

pytestmark = pytest.mark.gpu
TABLES = tuple(P.TABLES)
ROBOT = dict(iiwa14=None, gen3="gen3", generic=P.GENERIC)


@pytest.fixture(scope="module")
def handles():
    from boundplanner_amd.solver import HipBoundMPC
    hs = {t: HipBoundMPC(10, robot=ROBOT[t]) for t in TABLES}
    yield hs
    for h in hs.values():
        h.close()


def run_on(h):
    return lambda pd, rd, q0, n_seeds, lo, hi, **opts: h.ik(pd, rd, q0, n_seeds=n_seeds, lo=lo, hi=hi, **opts)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("tname", TABLES)
def test_truncated_solves(handles, tname, kind):
    case = [c for c in P.truncated_cases(tname) if c["kind"] == kind][0]
    assert P.check_truncated(case, run_on(handles[tname])) == 0


@pytest.mark.parametrize("tname", TABLES)
def test_every_halton_seed(handles, tname):
    P.check_seeds(tname, run_on(handles[tname]))


@pytest.mark.parametrize("tname", TABLES)
def test_winner_order(handles, tname):
    run = run_on(handles[tname])
    tie = P.seed_run(tname, run)["q"][P.TIE_SEED - 1] if tname == "iiwa14" else None
    assert P.check_winner(tname, run, tie) == 0


def test_device_entry_is_bitwise_the_host_entry(handles):
    """the box case of the generic table (per-instance lo / hi, B = 29) at depth 8, and the winner instances with 8 seeds"""
    import torch
    h = handles["generic"]
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c = [c for c in P.truncated_cases("generic") if c["kind"] == "box"][0]
    w = P.winner_case("generic")
    for pd, rd, q0, lo, hi, ns, opts in ((c["pd"], c["rd"], c["q0"], c["lo"], c["hi"], 1, dict(c["opts"], max_iter=8)),
                                         (w["pd"], w["rd"], w["q0"], None, None, 8, dict(max_iter=P.WINNER_DEPTH))):
        ref = h.ik(pd, rd, q0, n_seeds=ns, lo=lo, hi=hi, **opts)
        out = h.ik_dev(T(pd), T(rd), T(q0), n_seeds=ns, lo=T(lo), hi=T(hi), **opts)
        torch.cuda.current_stream().synchronize()
        for k in ref:
            assert np.array_equal(out[k].cpu().numpy(), ref[k], equal_nan=True), k


def test_fk_on_the_generic_table(handles):
    rng = np.random.default_rng(41)
    q, dq = rng.uniform(-3.0, 3.0, (64, 7)), rng.normal(size=(64, 7))
    P.check_fk(P.GENERIC, handles["generic"].fk(q, dq), q, dq)
