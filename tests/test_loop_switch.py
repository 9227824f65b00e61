"""The set-switch state machine at the end of loop_finish (boundplanner_amd/csrc/bmpc_loop.hpp, "split indices: countdown of a
set switch, or detection of a new one") with lp_path_update and lp_set_point, against PLANTED runs of the reference:
tests/golden/switch_cases.npz holds, per script, what the reference's unmodified BoundMPC.step / compute_return_data /
ReferencePath did with a scripted solution in the solver slot (tests/golden/gen/gen_switch_cases.py).  The scripts reach the
branches no closed-loop trace reaches:

  a  i = 1 and i = 2 detect in one step; i = 2 sees the phi_switch that i = 1 has just rewritten (correction >= 0.05)
  b  idx_new[0] == 1: the switch comes in the detecting step          c  idx_new[0] == 0: split -1, clamped to 1
  d  both slots pick the same stage: the clamp lifts split[2]          e  not_at_end false with a full candidate
  f  pairs 1e-6 either side of each gate (path parameter - 0.03, both sets with a non-zero position slack, upper and lower
     rotation bound, next upper bound + 5 degrees and next lower bound - 5 degrees) and a late out-of-set stage that cuts
     the trailing run
  g  failed solves: during a countdown, with a candidate in the solution fallen back on, status != 0 with a small violation
     (a success), the very first solve
  h  eight via points walked to the last sector, every detection at stage 1
  i  a pure-rotation segment walked through                             j  corrections of either sign, phi_max falls below 1

Every segment has its own A (row order), its own b (box) and its own rotation bounds, so reading another segment's shows.  The CPU build of the identical
header (tests/emu/emu_loop.cpp) replays every script: the solver arguments it prepares and ALL state it carries afterwards
(split indices, switch flag, sector, via points, segment lengths, both phi_max, the window, joint state) against the
reference's -- integers and flags exactly, floats to the 1e-9 of tests/test_device_loop.py.  That every case occurred is
asserted on the fixture, not on the code under test.  tests/test_loop_switch_gpu.py runs the same scripts as one batch through
the HIP kernels.

What the scripts catch -- mutations of a scratch copy under test_emulator_replays_the_planted_runs (the scripts that fail @ their
first failing step; step 0 is the warm-up step on the start-up path).  The state is compared with the reference's before the
record is compared with the host mirror's, so a mutant of bmpc_loop.hpp fails on the independent check: the field is `split`
throughout, except where said:
  PHI_M 0.03 -> 0.04                               f_phi_out@1
  IN_SET without + ps                              f_set0_in@1  f_set1_in@1
  trailing-run loop started at 0                   f_run_cut@1
  phi_switch snapshotted before the i loop         a_same_step@1  b_idx1@1
  not_at_end dropped                               all 29 scripts @0 (the start-up path has no next sector; every closed-loop
                                                   trace starts like that as well)
  the final clamp dropped                          b_idx1@1  c_idx0@1  d_same_idx@1
  ROT_M on the wrong pair of bounds                f_rot_out@1  f_rotlo_out@1  f_rotn_in@1  f_rotnup_in@1
  `ers > lower bound` dropped                      f_rotlo_out@1
  `ersn < next upper bound + ROT_M` dropped        f_rotnup_out@1
  `ec == 0` dropped from the detection branch      g_fail_candidate@1
  a0 read from segment i (A of the wrong segment)  22 scripts (every one that detects) @1, g_fail_candidate@3
  a1 read from segment i - 1                       the same 22
  loop_prepare: every a_set block from segment 0   all 29 scripts @1, field `p`
  from_device_record: a_set[0] / a_set[1] for      19 scripts @ the first step with a split index set, field `a_set_next`
    a_set[seg1] / a_set[nxt] (b left right)
The unmutated sources fail none.
"""
import numpy as np
import pytest

import switch_cases_lib as SC
from test_device_loop import replay_trace


@pytest.fixture(scope="module")
def cases(golden_dir):
    return SC.load(golden_dir)


def test_fixture_reaches_every_case(cases):
    """Computed from the reference's record alone: each of a..j occurred, each pair of f split the intended way, every script
    has its own boxes per segment, and no gate quantity of any accepted step is closer than 1e-6 to its threshold."""
    cov = SC.coverage(cases)
    print("coverage:", cov)
    for case in "abcdefghij":
        assert cov[case] is True, (case, cov)
    assert all(cov["f_pairs"].values()) and all(cov["g_parts"].values())
    assert cases["margin"].min() >= 1e-6
    for s, n in enumerate(cases["via_n"]):          # A, b (as a set of faces, whatever the row order) and the rotation bounds
        for key, canon in (("via_a_sets", np.ravel), ("via_b_sets", np.sort), ("via_e_r_bound", np.ravel)):
            assert len({tuple(canon(r)) for r in cases[key][s, :n - 1]}) == n - 1, (s, key)
    assert len(cases["script"]) % 64 != 0 and cases["in_q"].shape[1] <= 17 and int(cases["N"]) == 8


def test_emulator_replays_the_planted_runs(cases):
    """Every script through the CPU build of bmpc_loop.hpp: arguments prepared and state carried equal the reference's, and
    the two decoders of the MPCData record (mpc_data.from_device_record, mpc_data.from_node of the host mirror) agree on
    every field -- the four set fields included, which differ from segment to segment here."""
    worst = {}
    for g in SC.scripts(cases):
        try:
            w = replay_trace(g, set_tol=1e-9, need_sets=True)
        except AssertionError as e:
            raise AssertionError(f"script {g.name}: {e}") from e
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("max deviation from the planted runs:", {k: float(f"{v:.2e}") for k, v in worst.items()})
