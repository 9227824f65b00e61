"""The pair kernels compiled for one horizon (bmpc_pair_fixed.hpp: N, the SoA stride NP = N - 1 and the slot strides are compile-time
constants, the lane's column of an array is a base pointer with constant offsets) against the generic ones, in the CPU build: the
same source instantiated on the two views of the argument block, on the same inputs, super-step for super-step from the cold start
(tests/emu/emu_fixed_stride.cpp).  Every body bmpc_pipeline.hip dispatches per horizon runs -- k_points, k_pose, k_eval<1>, k_eval<2>,
k_curv beside them, k_step, k_trial or k_trial_spec.  The change is integer address arithmetic only, so the WHOLE workspace (iterates,
rows, steps, partials, stage records, gains) and the instance states must be equal bit for bit.

Cases: N = 20 with B = 4 (three instances per wavefront: 3 + 1, the last wavefront partly filled) and N = 30 with B = 3 (2 + 1);
after one super-step, and after ten, by which some line search of the batch has rejected a trial point -- the `round` loop of
k_trial ran twice for that wavefront (checked: InstState.bt counts the rejected trials of a search)."""
import numpy as np
import pytest

import emu_fixed_stride_lib as F
import oracle_lib as O
from boundplanner_amd import scenes

SEED = 4


def _batch(N, B):
    return scenes.make_batch(B, N, SEED, O.fk_batch, randomize_sets=True)


def _both(N, B, steps, trial_spec):
    b = _batch(N, B)
    return [F.super_steps(N, b["x0"], b["lbx"], b["ubx"], b["p"], fixed, steps, trial_spec) for fixed in (False, True)]


@pytest.mark.parametrize("N,B", [(20, 4), (30, 3)])
def test_one_super_step_with_a_partly_filled_wavefront_is_bitwise_the_generic_one(N, B):
    assert B % (64 // (N - 1)) != 0
    gen, fix = _both(N, B, 1, False)
    assert np.array_equal(gen["work"], fix["work"])
    assert np.array_equal(gen["state"], fix["state"])
    assert np.any(gen["work"] != 0)


@pytest.mark.parametrize("trial_spec", [False, True])
@pytest.mark.parametrize("N,B", [(20, 4), (30, 3)])
def test_super_steps_with_a_backtracking_line_search_are_bitwise_the_generic_ones(N, B, trial_spec):
    gen, fix = _both(N, B, 10, trial_spec)
    assert gen["bt_max"] >= 1 and fix["bt_max"] == gen["bt_max"] and fix["bt_sum"] == gen["bt_sum"]      # it really backtracks
    assert np.array_equal(gen["work"], fix["work"])
    assert np.array_equal(gen["state"], fix["state"])
