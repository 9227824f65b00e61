"""tests/golden/switch_cases.npz (tests/golden/gen/gen_switch_cases.py): planted runs of the reference's set-switch logic --
one script per rollout, all scripts in lock step.  Views of one script with the keys of the closed-loop traces, and what the
fixture itself says about the branches it reaches (TEST INFRASTRUCTURE ONLY)."""
import os

import numpy as np

# event code of a step (bit mask, gen_switch_cases.py)
DET1, DET2, SWITCH, FAIL, CLAMP, SLIDE, CAND_ONLY = 1, 2, 4, 8, 16, 32, 64
WHOLE = ("N", "n_update", "weights", "lbx_const", "ubx_const")


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "switch_cases.npz"))


class Script:
    """One script of the fixture as a closed-loop trace (the keys tests/test_device_loop.py replay_trace reads).  lbx / ubx are
    rebuilt from the constant part and the 40 pins of the step; g is not stored (the replaying solver hands the recorded
    violation on)."""

    def __init__(self, f, s):
        self.f, self.s = f, s
        self.name = str(f["script"][s])
        self.files = [k for k in f.files if k != "pins"] + ["call_lbx", "call_ubx", "call_g"]
        self._cache = {}

    def __getitem__(self, key):
        if key not in self._cache:
            self._cache[key] = self._get(key)
        return self._cache[key]

    def _get(self, key):
        f, s = self.f, self.s
        N = int(f["N"])
        if key in WHOLE:
            return f[key]
        if key in ("call_lbx", "call_ubx"):
            pins = f["pins"][s]
            out = np.tile(f["lbx_const" if key == "call_lbx" else "ubx_const"], (pins.shape[0], 1))
            out[:, :40 * N:N] = pins
            return out
        if key == "call_g":
            return np.zeros((f["pins"].shape[1], 1))
        if key.startswith("via_") and key != "via_n":
            n = int(f["via_n"][s])
            return f[key][s][:n if key in ("via_p_via", "via_r_via") else n - 1]
        return f[key][s]


def scripts(f):
    return [Script(f, s) for s in range(len(f["script"]))]


def coverage(f):
    """Which of the cases a..j the fixture reaches, from the reference's own record: name -> bool."""
    N = int(f["N"])
    name = [str(n) for n in f["script"]]
    ev, split, det, cand = f["event"], f["split_idxs"], f["det"], f["cand"]
    row = lambda nm: name.index(nm)
    has = lambda r, bits: ((ev[r] & bits) == bits).any()
    c = {}
    # a: both slots detect in one step, and the correction of i = 1 (what it took off phi_switch[2]) is at least 0.05 and moves
    # the threshold of i = 2 across the path parameter of the stage i = 2 picked
    r = row("a_same_step")
    k = int(np.where((ev[r] & (DET1 | DET2)) == (DET1 | DET2))[0][0])
    stale, live = f["call_p"][r, k, 65 + 2], f["rp_phi_switch"][r, k, 2]
    phi_pick = f["traj_phi"][r, k, det[r, k, 1] - 1]              # traj_phi starts at stage 1
    c["a"] = bool(stale - live >= 0.05 and live - 0.03 < phi_pick < stale - 0.03 and det[r, k, 0] != det[r, k, 1])
    r = row("b_idx1")
    c["b"] = bool(((det[r, :, 0] == 1) & ((ev[r] & SWITCH) != 0)).any())
    r = row("c_idx0")
    k = int(np.where(det[r, :, 0] == 0)[0][0])
    c["c"] = bool(split[r, k, 1] == 1 and (ev[r, k] & (CLAMP | SWITCH)) == CLAMP and (ev[r, k + 1] & SWITCH))
    r = row("d_same_idx")
    k = int(np.where((ev[r] & DET2) != 0)[0][0])
    c["d"] = bool(det[r, k, 0] == det[r, k, 1] and split[r, k, 2] == split[r, k, 1] + 1 and (ev[r, k] & CLAMP))
    r = row("e_at_end")
    last = f["sector"][r] == f["num_sectors"][r]
    c["e"] = bool(((ev[r] & DET1) != 0)[~last].any() and ((cand[r, :, 0] >= 0) & last & (det[r, :, 0] < 0) & (split[r, :, 1] == N))[1:].any())
    # f: of each pair one member detects and the other does not, and the margin of both is the planted 1.001e-6 (rot / rotlo:
    # upper / lower bound of the current segment, rotnup / rotn: upper + 5 deg / lower - 5 deg of the next)
    pairs = {}
    for q in ("phi", "set0", "set1", "rot", "rotlo", "rotn", "rotnup"):
        i, o = row(f"f_{q}_in"), row(f"f_{q}_out")
        pairs[q] = bool(has(i, DET1) and not (ev[o] & (DET1 | DET2)).any() and abs(f["margin"][i].min() - 1.001e-6) < 1e-11
                        and abs(f["margin"][o].min() - 1.001e-6) < 1e-11 and np.abs(f["call_x"][i] - f["call_x"][o]).max() < 2.5e-6)
    # the position slack of the two set pairs is not zero
    pairs["pslack"] = bool((f["call_x"][row("f_set0_in"), 1, -2 * N:-N] != 0).all() and (f["call_x"][row("f_set1_out"), 1, -2 * N:-N] != 0).all())
    i, o = row("f_run_cut"), row("f_run_whole")
    pairs["run"] = bool(det[i, 1, 0] == 7 and det[o, 1, 0] == 3)
    c["f"] = all(pairs.values())
    c["f_pairs"] = pairs
    g = {}
    r = row("g_fail_countdown")
    fails = (ev[r] & FAIL) != 0
    g["countdown"] = bool((fails[1:] & (split[r, 1:, 1] == split[r, :-1, 1] - 1)).any() and f["error_count"][r].max() == 2
                          and (fails & ((ev[r] & SWITCH) != 0)).any())
    r = row("g_fail_candidate")
    fails = (ev[r] & FAIL) != 0          # the solution the failed step fell back on would have been detected on, had it been accepted
    g["suppressed"] = bool(fails.any() and (f["fallback_cand"][r][fails] >= 0).all() and (det[r][fails] < 0).all())
    r = row("g_status_only")
    g["status_only"] = bool(((f["status"][r] != 0) & (f["viol"][r] < 1e-4) & (f["viol"][r] > 0) & ((ev[r] & DET1) != 0)).any()
                            and not (ev[r] & FAIL).any())
    r = row("g_fail_first")
    g["first"] = bool(f["status"][r, 0] != 0 and f["viol"][r, 0] >= 1e-4 and f["error_count"][r, 0] == 0)
    c["g"], c["g_parts"] = all(g.values()), g
    r = row("h_eight")
    c["h"] = bool(f["via_n"][r] == 8 and f["sector"][r].max() == f["num_sectors"][r, -1] == 6 and (det[r][det[r, :, 0] >= 0, 0] == 1).all()
                  and ((ev[r] & CAND_ONLY) != 0)[7:].any())
    r = row("i_pure_rot")
    n = int(f["via_n"][r])
    seg = np.linalg.norm(np.diff(f["via_p_via"][r, :n], axis=0), axis=1)
    c["i"] = bool((seg < 1e-3).sum() == 1 and f["sector"][r].max() > int(np.argmin(seg)))
    # what a step took off phi_max: the value its prepare was handed (parameter 231, min(phi + 5, phi_max)) less the one it left
    corr = (f["call_p"][:, :, 231] - f["phi_max"][..., 0])[:, 1:]
    r = row("j_phi_max")
    c["j"] = bool((corr > 1e-3).any() and (corr < -1e-3).any() and f["call_p"][r, 1, 231] > 1 > f["phi_max"][r, -1, 0] > 0.001
                  and f["call_p"][r, -1, 220 + 4] != f["weights"][4])
    return c
