"""What a solve returns when it stops short of a solution, pinned to the full-space NLP at the returned point (CPU half;
tests/test_solve_outputs_gpu.py is the MI355X half, tests/solve_outputs_lib.py documents the reference, the families of points, the
checks and the bounds).

What runs: emu_pipe_solve (tests/emu/emu_pipe.cpp, the bodies of bmpc_solve: k_out, k_fin, k_mult, k_mult_sweep among them) with
max_iter = 0, 1, 2, 5.  Reads the oracle library and the scene generator only.
"""
import numpy as np
import pytest

import emu_pipe_lib as E
import oracle_lib as O
import solve_outputs_lib as L


def solve(N, x0, lbx, ubx, p, max_iter, want_g, want_lam, slots=0):
    return E.solve_batch(N, x0, lbx, ubx, p, max_iter=max_iter, want_g=want_g, want_lam=want_lam, slots=slots)


def _ids(cases):
    return [f"N{c[0]}-B{c[1]}" + (f"-{c[3]}" if c[3] else "") for c in cases]


@pytest.mark.parametrize("case", L.CPU_CASES, ids=_ids(L.CPU_CASES))
def test_emulated_iterates_return_the_nlp_at_their_point(case):
    N, B = case[:2]
    slots = 5 if B > 5 else 2
    pool = (lambda *a, **kw: solve(*a, slots=slots, **kw), slots)
    L.check_natural(solve, case, f"emulated iterates N={N} B={B}", pool=pool, pool_ks=(2,))


@pytest.mark.parametrize("N", L.PLANT_N_CPU)
def test_emulated_planted_points(N):
    L.check_planted(solve, N, f"emulated planted points N={N}")


@pytest.mark.parametrize("N", L.WARM_N_CPU)
def test_emulated_stopped_warm_starts(N):
    L.check_warm(solve, N, f"emulated stopped warm starts N={N}")


def test_the_cases_cover_every_class():
    """each half's cases name, between them, every class of viol and a p_rot defect (check_natural asserts what a case names)"""
    for cases in (L.CPU_CASES, L.GPU_CASES):
        assert set().union(*(L.WANTS[c] for c in cases)) == L.CLASSES | {"pi"}
    for N in set(L.PLANT_N_CPU) | set(L.PLANT_N_GPU):
        rows = L.plant_rows(N)
        assert {k for _, _, k in rows} >= {1, N - 1} and {g for g, _, k in rows if k == 1} == set(L.GROUPS)


def test_the_restated_formula_on_hand_made_rows():
    """viol_formula itself: rows inside the dead band count nothing, rows outside their full value, by the side their bound is on"""
    lbg = np.array([0, 0, 0, 0, -1e20, -1e20, 0, 0], float)
    ubg = np.array([0, 0, 0, 0, 0, 0, 1e20, 1e20], float)
    g = np.array([0.9e-6, -0.9e-6, 1.1e-6, -1.1e-6, 0.5, -0.5, 0.25, -0.25])
    assert abs(float(L.viol_formula(g, lbg, ubg)) - (2.2e-6 + 0.5 + 0.25)) < 1e-18
    lb, ub = O.gbounds(4)
    assert ((lb == 0) & (ub == 0)).sum() == 35 * 3 and lb.shape == (L.dims(4)[1],)


def test_oracle_worst_is_what_the_oracle_gives():
    """ORACLE_WORST is measured on the oracle's own recover_multipliers, not on the kernels: on this half's cases it stays below the
    recorded figures and reaches a quarter of them"""
    w = L.oracle_worst(L.CPU_CASES, L.PLANT_N_CPU, L.WARM_N_CPU, report=lambda s: None)
    for fam, v in w.items():
        assert v <= L.ORACLE_WORST[fam], (fam, v)
    assert max(w.values()) >= 0.25 * max(L.ORACLE_WORST.values())
