"""Generate tests/golden/switch_cases.npz: planted runs of the REFERENCE's set-switch logic.

The reference's unmodified BoundMPC.update / BoundMPC.step / compute_return_data, ReferencePath and integrate_joint run as in
gen_closed_loop.py; the solver slot holds a shim that returns a SCRIPTED solution (the post-solve logic never checks the
dynamics): the joint block rests at the current q, column 0 equals the pins, and the task-space columns (end-effector
positions, integrated omega, position slacks) are planted so that every stage has a chosen path parameter, a chosen distance
to the current and the next set and chosen orientation-error coordinates.  Every script aims at one branch of the split-index
logic at the end of compute_return_data (BoundMPC.py:916-1021); which branch the reference then took is read back from its
state (and from the one line it prints when it adapts a via point) and must equal the script's intention.  Asserted while writing:
  * every gate quantity of every stage of every accepted step is at least 1e-6 from its threshold, a thousand times the 1e-9
    replay tolerance: rounding cannot flip a decision (the pairs around a threshold are planted at +-1.001e-6, so that the
    rounding of the plant, 1e-12, stays inside);
  * the intended event code of every step equals the observed one.
The fixture is data only; no reference source is copied.

    python tests/golden/gen/gen_switch_cases.py
"""
import contextlib
import copy
import io
import os
import re
import sys

import numpy as np
from scipy.spatial.transform import Rotation as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_closed_loop as G  # noqa: E402  (sets up the import paths of the reference and its stubs)
from gen_closed_loop import DM, FakeRobot, make_ref_mpc  # noqa: E402
import bound_planner.BoundMPC.BoundMPC as refmod  # noqa: E402
from bound_planner.utils import get_default_params, integrate_joint  # noqa: E402
from bound_planner.utils.util_functions import Params  # noqa: E402

N = 8
STEPS = 16               # script steps after the warm-up step on the start-up path
MARGIN = 1e-6
PLANT = 1.001e-6          # distance of a tuned quantity from its threshold
DEG = np.pi / 180
IN_SET, PHI_M, ROT_M = 0.005, 0.03, 5 * DEG        # the thresholds under test (BoundMPC.py:917, 926, 963-964)

# event code of a step (bit mask)
DET1, DET2, SWITCH, FAIL, CLAMP, SLIDE, CAND_ONLY = 1, 2, 4, 8, 16, 32, 64
# DET1 / DET2  a new switch was detected at i = 1 / i = 2 (a via point was adapted)
# SWITCH       the switch flag is set after the step
# FAIL         error_count > 0 after the step
# CLAMP        the final monotone fix changed a split index
# SLIDE        the 4-segment window moved at the start of the step
# CAND_ONLY    a free slot had a candidate stage that passed all five gates and no detection followed (not_at_end false)

# the path parameter of every stage as the reference computed it (reference_function is called once per stage)
_PHI = []
_rf = refmod.reference_function


def _recording_reference_function(**kw):
    out = _rf(**kw)
    _PHI.append(float(np.ravel(out["phi"])[0]))
    return out


refmod.reference_function = _recording_reference_function


class PlantSolver:
    """CasADi-function-like shim: returns the solution the current plant scripts."""

    def __init__(self):
        self.calls, self._stats, self.plant = [], {}, None

    def __deepcopy__(self, memo):
        return self

    def __call__(self, x0, lbx, ubx, lbg, ubg, p):
        x0, lbx, ubx, p = (np.asarray(a, float).reshape(-1) for a in (x0, lbx, ubx, p))
        x, status, viol = self.plant(lbx)
        lb, ub = np.asarray(lbg, float), np.asarray(ubg, float)
        g = np.clip(np.zeros(lb.size), lb, ub)
        g[3] = ub[3] + viol                    # one dynamics row off by `viol` (what BoundMPC.py:613-615 sums up)
        self._stats = {"iter_count": 1, "success": status == 0, "return_status": "planted"}
        self.calls.append(dict(x0=x0.copy(), lbx=lbx.copy(), ubx=ubx.copy(), p=p.copy(), x=x.copy(), iters=1, status=status, viol=float(viol)))
        z = np.zeros(1)
        return {"x": DM(x), "g": DM(g), "lam_g": DM(z), "lam_x": DM(z), "f": DM(z)}

    def stats(self):
        return self._stats


def plant_x(pins, pos, iw=None, ps=None, v=None):
    """Solution vector: joints at rest at the pinned q, task-space columns as given ([N][3] each), column 0 = pins."""
    n_w = 44 * N + 6
    x = np.zeros(n_w)
    q, p0 = pins[:7 * N:N], pins[28 * N:34 * N:N]
    x[:7 * N] = np.repeat(q, N)
    P = np.tile(p0[:, None], (1, N))
    P[:3, 1:] = np.asarray(pos, float).T[:, 1:]
    if iw is not None:
        P[3:, 1:] += np.asarray(iw, float).T[:, 1:]
    x[28 * N:34 * N] = P.reshape(-1)
    if v is not None:
        Vv = np.zeros((6, N)); Vv[:3, 1:] = np.asarray(v, float).T[:, 1:]
        x[34 * N:40 * N] = Vv.reshape(-1)
    for blk in (7, 14, 21, 34):      # dq, ddq, jerk, v: column 0 is pinned as well
        w = 7 if blk < 28 else 6
        x[blk * N:(blk + w) * N:N] = pins[blk * N:(blk + w) * N:N]
    if ps is not None:
        x[n_w - 2 * N:n_w - N] = ps
    return x


def gates(m, x, phis):
    """The five gate quantities of the step the reference object `m` has just taken with solution x, per slot i and stage:
    margin > 0 passes.  phi_switch is read after the step: entry 1 is never rewritten inside a step, entry 2 only by the
    detection at i = 1, which precedes the test of i = 2 (the live array of ReferencePath.get_parameters)."""
    rp = m.ref_path
    pos, ps = x[28 * N:31 * N].reshape(3, N), x[44 * N + 6 - 2 * N:44 * N + 6 - N]
    _, a_set, b_set = rp.get_bound_params()
    e_rs = np.array([m.err_data["e_r_orth1"], m.err_data["e_r_par"], m.err_data["e_r_orth2"]], float).reshape(3, N).T
    e_rsn = np.array([m.err_data["e_r_orth1n"], m.err_data["e_r_parn"], m.err_data["e_r_orth2n"]], float).reshape(3, N).T
    lo, up = np.array(m.ref_data["r_bound_lower"], float), np.array(m.ref_data["r_bound_upper"], float)
    lon, upn = np.array(m.ref_data["r_bound_lower_next"], float), np.array(m.ref_data["r_bound_upper_next"], float)
    rot = np.concatenate((up - e_rs, e_rs - lo), axis=1)
    rotn = np.concatenate((upn + ROT_M - e_rsn, e_rsn - (lon - ROT_M)), axis=1)
    out = {}
    for i in (1, 2):
        d0 = np.max(a_set[i - 1] @ pos - b_set[i - 1][:, None], axis=0)
        d1 = np.max(a_set[i] @ pos - b_set[i][:, None], axis=0)
        g = dict(phi=np.asarray(phis) - (rp.phi_switch[i] - PHI_M), set0=IN_SET + ps - d0, set1=IN_SET + ps - d1, rot=rot, rotn=rotn)
        in1 = g["set1"] > 0
        out_idx = np.where(~in1)[0]
        if out_idx.size:
            in1[:out_idx[-1]] = False
        ok = (g["phi"] > 0) & (g["set0"] > 0) & in1 & (rot > 0).all(axis=1) & (rotn > 0).all(axis=1)
        g["cand"] = int(np.where(ok)[0][0]) if ok.any() else -1
        g["worst"] = min(np.abs(g[k]).min() for k in ("phi", "set0", "set1", "rot", "rotn"))
        out[i] = g
    return out


def observe(sb, sa, sw, ec, sector_moved, dets, cand, slots_free, not_at_end):
    """Event code of a step from the reference's state before / after it (split indices sb -> sa, switch flag, error count,
    sector) and the detections it announced ({i: idx_new[0]}); the split indices are re-derived from those and must come out."""
    s, code, flag = list(sb), 0, False
    for i in (1, 2):
        if s[i] < N:
            s[i] -= 1
            if s[i] == 0:
                flag, s[i] = True, N
        elif i in dets:
            s[i] = dets[i] - 1
            code |= DET1 if i == 1 else DET2
            flag = flag or s[i] == 0
    if flag:
        s[1:-1] = s[2:]
        s[-1] = N
    pre = list(s)
    for i in range(1, 4):
        if s[i] <= s[i - 1]:
            s[i] = min(N, s[i - 1] + 1)
    assert s == list(sa) and flag == bool(sw), (sb, sa, sw, dets, s, flag)
    code |= (SWITCH if sw else 0) | (FAIL if ec > 0 else 0) | (CLAMP if pre != s else 0) | (SLIDE if sector_moved else 0)
    if any(cand[i] >= 0 and slots_free[i] and not not_at_end[i] for i in (1, 2)):
        code |= CAND_ONLY
    return code


def box_set(lo, hi, j):
    """The box lo <= x <= hi as 15 halfspace rows (A x <= b, padding rows A = 0, b = 10) with a row order of segment j's own:
    the six faces start at row j, in an order turned by j -- so every segment of a path has its own A as well as its own b."""
    faces = np.roll(np.arange(6), j)
    a6, b6 = np.vstack((np.eye(3), -np.eye(3)))[faces], np.concatenate((np.asarray(hi, float), -np.asarray(lo, float)))[faces]
    a, b = np.zeros((15, 3)), 10.0 * np.ones(15)
    a[j:j + 6], b[j:j + 6] = a6, b6
    return a, b


# ---- paths: via points relative to the start pose, one box per segment, PAIRWISE DIFFERENT (a mix-up of which segment's
# set is read shows), different rotation bounds per segment as well
def path(dp, euler, boxes, erb):
    return dict(dp=np.array(dp, float), euler=np.array(euler, float), boxes=np.array(boxes, float), erb=np.array(erb, float) * DEG)


def bounds(*ups):
    return [[u, u + 2, u + 4, -u - 1, -u - 3, -u - 5] for u in ups]


P5 = path([[0, 0, 0], [.10, 0, .02], [.20, .03, .02], [.30, .03, .06], [.40, 0, .06]],
          [[0, 0, 0], [5, 0, 0], [5, 6, 0], [5, 6, 7], [0, 6, 7]],
          [[-.05, -.10, -.06, .19, .08, .09], [.04, -.12, -.05, .31, .12, .07], [.11, -.06, -.04, .41, .13, .12],
           [.21, -.09, -.03, .52, .11, .14]], bounds(60, 50, 70, 80))
P3 = path(P5["dp"][:3], P5["euler"][:3], P5["boxes"][:2] + np.array([0, 0, -.01, 0, .01, 0]), bounds(65, 55))
# phi_max = 1.03 > 1: a positive correction of 0.05 takes it below 1 (the w_phi rescale of the next prepare goes live, Q10)
PLONG = path([[0, 0, 0], [.10, 0, .02], [1.03, 0, .02]], [[0, 0, 0], [4, 0, 0], [4, 0, 9]],
             [[-.04, -.11, -.07, .20, .09, .08], [.03, -.13, -.04, 1.1, .10, .09]], bounds(62, 52))
# a first segment shorter than the 0.03 margin: stage 0 (the pin) is a candidate
PSHORT = path([[0, 0, 0], [.02, 0, 0], [.12, .02, 0], [.22, .02, .03]], [[0, 0, 0], [3, 0, 0], [3, 4, 0], [3, 4, 5]],
              [[-.06, -.09, -.05, .10, .07, .08], [-.03, -.11, -.04, .20, .09, .06], [.05, -.07, -.03, .30, .12, .10]], bounds(61, 51, 71))
# eight via points (LP_MAXPTS), a zig-zag with 0.1 m steps
P8 = path([[.1 * j, .02 * (j % 2), .01 * (j % 3)] for j in range(8)], [[3 * (j % 3), 2 * j, j] for j in range(8)],
          [[.1 * j - .05 - .002 * j, -.10 - .003 * j, -.06 - .001 * j, .1 * j + .18 + .001 * j, .09 + .002 * j, .08 + .003 * j] for j in range(7)],
          bounds(60, 50, 70, 80, 55, 65, 75))
# segment 1 is a pure rotation (two via points at the same position, 25 degrees apart): its length is |dr| / pi
PROT = path([[0, 0, 0], [.10, 0, .02], [.10, 0, .02], [.20, .03, .02]], [[0, 0, 0], [5, 0, 0], [5, 0, 25], [5, 6, 25]],
            [[-.05, -.10, -.06, .19, .08, .09], [.04, -.12, -.05, .45, .12, .07], [.02, -.06, -.04, .50, .13, .12]], bounds(80, 85, 88))
# rotation-gate paths: tight bounds so that a planted orientation error of a few degrees reaches them
PROT_C = dict(P5, erb=np.array(bounds(12, 40, 70, 80), float) * DEG)      # current bound 12..16 deg, next 40..44 (+5)
PROT_N = dict(P5, erb=np.array(bounds(60, 8, 70, 80), float) * DEG)       # next bound 8..12 deg (+5), current 60..64

PIN = np.zeros(3)
IDLE = dict(pos=[PIN] * N)


def stages(*spec):
    """[(first stage, offset from the start position), ...] -> N stage offsets; stages before the first entry rest at the pin."""
    out, cur = [], PIN
    spec = dict(spec)
    for k in range(N):
        cur = np.asarray(spec.get(k, cur), float)
        out.append(cur)
    return out


X1 = [.16, 0, .02]           # next to via point 1 of P5: inside boxes 0, 1 and 2, beyond phi_switch[1] - 0.03 on segment 0
XF = [.16, -.075, .02]       # the same outside box 2: a candidate of i = 1 alone


def scripts():
    """name -> dict(path, warm (plant of the warm-up step), steps [(plant, intended event code), ...]).  A plant:
    dict(pos=[N offsets from the start position], ps=position slacks, status, viol, tune=(gate quantity of stage 7[, component], signed
    margin to plant))."""
    S = {}
    far = stages((3, XF))
    # a: i = 1 and i = 2 detect in the same step; the correction at i = 1 (0.0565) moves phi_switch[2] from 0.2064 to 0.1499
    # before i = 2 is tested: stages 5.. (phi = 0.161) pass the live threshold 0.120 and not the stale one 0.176
    a_pos = stages((3, [.18, -.07, .02]), (5, X1))
    S["a_same_step"] = dict(path=P5, steps=[(dict(pos=a_pos), DET1 | DET2)] + [(dict(pos=a_pos), 0), (dict(pos=a_pos), SWITCH), (IDLE, SLIDE), (IDLE, SWITCH), (IDLE, SLIDE)])
    # b: idx_new[0] == 1 switches in the detecting step
    S["b_idx1"] = dict(path=P5, steps=[(dict(pos=stages((1, X1))), DET1 | DET2 | SWITCH | CLAMP), (IDLE, SLIDE | SWITCH), (IDLE, SLIDE)])
    # c: idx_new[0] == 0 writes split = -1, the clamp makes it 1, the switch comes one step later
    S["c_idx0"] = dict(path=PSHORT, steps=[(IDLE, DET1 | CLAMP), (IDLE, SWITCH), (IDLE, SLIDE)])
    # d: both slots detect the same stage: the clamp lifts split[2]
    S["d_same_idx"] = dict(path=P5, steps=[(dict(pos=stages((4, [.185, 0, .02]))), DET1 | DET2 | CLAMP)] + [(IDLE, 0)] * 2 + [(IDLE, SWITCH), (IDLE, SLIDE | SWITCH), (IDLE, SLIDE)])
    # e: three via points (one sector to move to); at sector 0 the plant detects at i = 1, and its full candidate of i = 2 is
    # stopped by not_at_end; at the last sector the same kind of plant is a full candidate of i = 1 and does not detect
    e_pos = stages((3, X1), (6, [.21, .03, .02]))
    S["e_at_end"] = dict(path=P3, steps=[(dict(pos=e_pos), DET1 | CAND_ONLY), (dict(pos=e_pos), CAND_ONLY), (dict(pos=e_pos), SWITCH | CAND_ONLY),
                                          (dict(pos=stages((3, [.21, .03, .02]))), SLIDE | CAND_ONLY), (dict(pos=stages((3, [.21, .03, .02]))), CAND_ONLY)])
    # f: gate pairs around the thresholds: stage 7 alone is a candidate, one quantity 1.001e-6 on either side; both sides of both
    # rotation gates (components 0..2 of a rotation gate are the upper bounds, 3..5 the lower ones)
    one = lambda off: stages((7, off))
    # (the set plants start beyond the face they are tuned against -- box 0's upper x, box 1's upper z -- so that this face is the
    # nearest one all the way; the position slack is not zero there)
    for nm, pth, tune, ps, xf in (("f_phi", P5, ("phi",), 0.0, XF), ("f_set0", P5, ("set0",), 0.003, [.21, -.075, .02]),
                                  ("f_set1", P5, ("set1",), 0.003, [.16, -.075, .085]),
                                  ("f_rot", PROT_C, ("rot", 1), 0.0, XF), ("f_rotlo", PROT_C, ("rot", 4), 0.0, XF),
                                  ("f_rotn", PROT_N, ("rotn", 5), 0.0, XF), ("f_rotnup", PROT_N, ("rotn", 1), 0.0, XF)):
        for side, ev in (("in", DET1), ("out", 0)):
            pl = dict(pos=one(xf), ps=np.full(N, ps), tune=tune + ((PLANT if side == "in" else -PLANT),))
            S[f"{nm}_{side}"] = dict(path=pth, steps=[(pl, ev)] + ([(IDLE, 0)] * 5 + [(IDLE, SWITCH), (IDLE, SLIDE)] if ev else []))
    # a late stage outside the next set cuts the trailing run: the candidate is stage 7, not stage 3
    S["f_run_cut"] = dict(path=P5, steps=[(dict(pos=stages((3, XF), (6, [.16, -.075, .085]), (7, XF))), DET1)] + [(IDLE, 0)] * 5 + [(IDLE, SWITCH), (IDLE, SLIDE)])
    S["f_run_whole"] = dict(path=P5, steps=[(dict(pos=far), DET1)] + [(IDLE, 0), (IDLE, SWITCH), (IDLE, SLIDE)])
    # g: failed solves
    bad = dict(IDLE, status=1, viol=1.0)
    S["g_fail_countdown"] = dict(path=P5, steps=[(dict(pos=stages((5, XF))), DET1), (bad, FAIL), (bad, FAIL), (IDLE, 0), (dict(bad, viol=2e-4), FAIL | SWITCH), (IDLE, SLIDE)])
    # the warm start carried over the re-plan holds a full candidate; the first solve on the new path fails and falls back on it
    S["g_fail_candidate"] = dict(path=P5, warm=dict(pos=far), steps=[(bad, FAIL), (IDLE, 0), (dict(pos=far), DET1), (IDLE, 0), (IDLE, SWITCH), (IDLE, SLIDE)])
    S["g_status_only"] = dict(path=P5, steps=[(dict(pos=far, status=1, viol=0.9e-4), DET1), (dict(IDLE, status=2, viol=0.0), 0), (IDLE, SWITCH), (IDLE, SLIDE)])
    S["g_fail_first"] = dict(path=P5, warm=bad, steps=[(dict(pos=far), DET1), (bad, FAIL), (IDLE, SWITCH), (IDLE, SLIDE)])
    # h: eight via points walked to the last sector, every detection at stage 1
    h = []
    for j in range(1, 7):
        v = P8["dp"][j] + np.array([.03, 0, 0])      # outside box j + 1: a candidate of i = 1 alone
        h.append((dict(pos=stages((1, v))), DET1 | SWITCH | (SLIDE if j > 1 else 0)))
    v7 = P8["dp"][7] + np.array([.03, 0, 0])
    S["h_eight"] = dict(path=P8, steps=h + [(dict(pos=stages((1, v7))), SLIDE | CAND_ONLY), (dict(pos=stages((1, v7))), CAND_ONLY)])
    # i: the pure-rotation segment walked through
    S["i_pure_rot"] = dict(path=PROT, steps=[(dict(pos=far), DET1), (dict(pos=far), 0), (dict(pos=far), SWITCH),
                                               (dict(pos=stages((2, [.40, .01, .03]))), SLIDE | DET1 | CAND_ONLY), (IDLE, SWITCH), (IDLE, SLIDE)])
    # j: corrections of either sign; phi_max falls below 1
    S["j_phi_max"] = dict(path=PLONG, steps=[(dict(pos=stages((3, [.152, 0, .02]))), DET1), (IDLE, 0), (IDLE, SWITCH), (IDLE, SLIDE)])
    S["j_negative"] = dict(path=P5, steps=[(dict(pos=stages((3, [.085, 0, .02]))), DET1), (IDLE, 0), (IDLE, SWITCH), (IDLE, SLIDE)])
    return S


def run_script(name, sc, robot, params, q0, p0):
    solver = PlantSolver()
    R0 = R.from_rotvec(p0[3:]).as_matrix()
    mpc = make_ref_mpc([p0[:3]] * 2, [R0] * 2, [np.array([1.0, 0, 0])], [np.array([1.0, 0, 0])], [G.ERB.copy()], [np.zeros((15, 3))],
                       [np.ones(15)], p0, params, solver, robot)
    st = dict(q=q0.copy(), qf=q0.copy(), dq=np.zeros(7), ddq=np.zeros(7), jerk=np.zeros(7), p_lie=p0.copy(), v=np.zeros(6))
    trace = []

    def take(m, state, x, status, viol):
        """One BoundMPC.step of object m with the planted solution; returns what the reference did."""
        solver.plant = lambda lbx: (x, status, viol)
        del _PHI[:]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            traj, ref_data, err_data, _, iters = m.step(state["q"], state["dq"], state["ddq"], state["p_lie"], state["v"], state["jerk"], state["qf"])
        dets = {int(a): int(b) for a, b in re.findall(r"Adapting Path Vias (\d+) (\d+)", buf.getvalue())}
        return traj, ref_data, err_data, dets, list(_PHI)

    def build(plant, pins, m0, state):
        """The plant's solution; a tuned plant moves ONE quantity of stage 7 to its threshold + signed margin, by the affine
        dependence of that quantity on the planted column (probed on copies of the reference object)."""
        pos = [p0[:3] + o for o in plant["pos"]]
        iw = np.zeros((N, 3))
        mk = lambda: plant_x(pins, pos, iw=iw, ps=plant.get("ps"), v=[[0.03, 0.0, 0.01]] * N)
        tune = plant.get("tune")
        if tune is None:
            return mk()

        def quantity():
            m = copy.deepcopy(m0)
            x = mk()
            *_, phis = take(m, state, x, 0, 0.0)
            g = gates(m, x, phis)[1]
            return g[tune[0]][7] if len(tune) == 2 else g[tune[0]][7][tune[1]]
        if tune[0] in ("rot", "rotn"):
            for _ in range(2):
                base = quantity()
                J = np.zeros(3)
                for c in range(3):
                    iw[7, c] += 0.01
                    J[c] = (quantity() - base) / 0.01
                    iw[7, c] -= 0.01
                iw[7] += J * (tune[-1] - base) / (J @ J)
        else:
            # positions: along segment 0's direction for the path parameter, along x / z for the two box faces
            d = {"phi": m0.ref_path.dpd[:3, 0].copy(), "set0": np.array([1.0, 0, 0]), "set1": np.array([0, 0, 1.0])}[tune[0]]
            for _ in range(2):
                base = quantity()
                pos[7] = pos[7] + 0.01 * d
                slope = (quantity() - base) / 0.01
                pos[7] = pos[7] + ((tune[-1] - base) / slope - 0.01) * d
        assert abs(quantity() - tune[-1]) < 1e-12, (name, quantity(), tune)
        return mk()

    def node_step(plant, intended):
        st["p_lie"], _, _ = robot.forward_kinematics(st["q"], st["dq"])
        rec = {"in_" + k: np.copy(v) for k, v in st.items()}
        m0 = copy.deepcopy(mpc)
        state = {k: np.copy(v) for k, v in st.items()}
        pins = np.zeros(44 * N + 6)
        for blk, val in ((0, st["q"]), (7, st["dq"]), (14, st["ddq"]), (21, st["jerk"]), (28, st["p_lie"]), (34, st["v"])):
            pins[blk * N:(blk + len(val)) * N:N] = val
        x = build(plant, pins, m0, state)
        sb, sector_b, phi_max_b = list(mpc.split_idxs), mpc.ref_path.sector, float(mpc.phi_max[0])
        will_slide = bool(mpc.switch) and mpc.ref_path.sector < mpc.ref_path.num_sectors
        traj, ref_data, err_data, dets, phis = take(mpc, st, x, int(plant.get("status", 0)), float(plant.get("viol", 0.0)))
        new = integrate_joint(robot, traj["dddq"], st["q"], st["dq"], st["ddq"], mpc.dt)
        st["q"], st["dq"], st["ddq"], st["p_lie"], st["v"] = new[0], new[1], new[2], new[3], new[4]
        st["qf"] = traj["q"][:, -1]
        st["jerk"] = traj["dddq"][:, 1]
        c = solver.calls[-1]
        assert np.array_equal(c["x"], x)
        # a failed solve falls back on the previous solution: would that solution, accepted as it is, have been detected on?
        fallback = -1
        if mpc.error_count > 0:
            m1 = copy.deepcopy(m0)
            fallback = take(m1, state, np.array(m0.prev_solution, float), 0, 0.0)[3].get(1, -1)
            solver.calls.pop()
        rp = mpc.ref_path
        # ---- what the reference did, against the script's intention and the margins
        cand, worst = {1: -1, 2: -1}, np.inf
        if mpc.error_count == 0:
            gt = gates(mpc, x, phis)
            cand = {i: gt[i]["cand"] for i in (1, 2)}
            worst = min(gt[1]["worst"], gt[2]["worst"])
            assert worst >= MARGIN, (name, len(trace), worst)
        free = {i: sb[i] == N and mpc.error_count == 0 for i in (1, 2)}
        nae = {i: rp.sector + (i - 1) < rp.num_sectors for i in (1, 2)}
        for i in (1, 2):          # the detections the reference announced are the candidates of the gate quantities above
            assert (i in dets) == (free[i] and nae[i] and cand[i] >= 0) and (i not in dets or dets[i] == cand[i]), (name, len(trace), i, dets, cand)
        observed = observe(sb, mpc.split_idxs, mpc.switch, mpc.error_count, rp.sector != sector_b, dets, cand, free, nae)
        assert (rp.sector != sector_b) == will_slide
        assert (float(mpc.phi_max[0]) != phi_max_b) == bool(dets), (name, len(trace))
        if observed != intended and mpc.error_count == 0:
            print({k: np.round(np.min(np.atleast_2d(v.T), axis=0), 4) if isinstance(v, np.ndarray) else v for k, v in gt[1].items()}, rp.phi_switch, rp.sector, file=sys.stderr)
        assert observed == intended, (name, len(trace), "intended", intended, "observed", observed, sb, list(mpc.split_idxs), dets, cand)
        # ---- the record (keys of gen_closed_loop.py; lbx / ubx as the 40 pins, no g)
        assert np.array_equal(c["lbx"][:40 * N:N], c["ubx"][:40 * N:N]) and np.array_equal(c["lbx"][:40 * N:N], pins[:40 * N:N])
        rec.update(call_x0=c["x0"], call_p=c["p"], call_x=c["x"], pins=pins[:40 * N:N].copy(), lbx=c["lbx"], ubx=c["ubx"],
                   iters=c["iters"], status=c["status"], viol=c["viol"], event=intended, cand=np.array([cand[1], cand[2]]),
                   det=np.array([dets.get(1, -1), dets.get(2, -1)]), margin=worst, fallback_cand=fallback)
        pad = lambda a: np.concatenate((np.asarray(a, float), np.full(np.asarray(a).shape[:-1] + (N - np.asarray(a).shape[-1],), np.nan)), axis=-1)
        rec.update({"traj_" + k: pad(traj[k]) for k in ("p", "v", "q", "dq", "ddq", "dddq", "phi", "dphi")})
        rec.update(traj_cols=np.asarray(traj["dddq"]).shape[-1], patched=0,           # (the end effector never turns: no omega re-basing)
                   ref_p1=np.array(ref_data["p"][1]), ref_p0=np.array(ref_data["p"][0]), err_e_p1=np.array(err_data["e_p"][1]),
                   err_e_r1=np.array(err_data["e_r"][1]))
        rec.update(split_idxs=np.array(mpc.split_idxs), switch=int(mpc.switch), pr_ref=np.copy(mpc.pr_ref), iw_ref=np.copy(mpc.iw_ref),
                   phi_current=mpc.phi_current.copy(), dphi_current=mpc.dphi_current.copy(), phi_max=mpc.phi_max.copy(),
                   slacks0=mpc.slacks0.copy(), error_count=mpc.error_count, sector=rp.sector, num_sectors=rp.num_sectors,
                   rp_pd=rp.pd.copy(), rp_phi_switch=rp.phi_switch.copy(), rp_phi_max=float(rp.phi_max),
                   rp_p=np.concatenate((np.array(rp.p, float), np.zeros((11 - len(rp.p), 3)))),
                   rp_phi=np.concatenate((np.array(rp.phi, float), np.zeros(12 - len(rp.phi)))))
        rec.update({"out_" + k: np.copy(v) for k, v in st.items()})
        trace.append(rec)

    node_step(sc.get("warm", IDLE), CAND_ONLY)      # warm-up on the start-up path: everything is a candidate there, and the path has no next sector
    pth = sc["path"]
    p_via = [p0[:3] + d for d in pth["dp"]]
    r_via = [R0 @ R.from_euler("xyz", e, degrees=True).as_matrix() for e in pth["euler"]]
    ns = len(p_via) - 1
    assert ns == len(pth["boxes"]) == len(pth["erb"])
    sets = [box_set(p0[:3] + b[:3], p0[:3] + b[3:], j) for j, b in enumerate(pth["boxes"])]
    for i in range(ns):
        for j in range(i):
            assert not np.array_equal(sets[i][0], sets[j][0]) and not np.array_equal(np.sort(sets[i][1]), np.sort(sets[j][1]))
            assert not np.array_equal(pth["erb"][i], pth["erb"][j])
    via = dict(p_via=np.array(p_via), r_via=np.array(r_via), bp1=np.tile([0.0, 0, 1], (ns, 1)), br1=np.tile([0.0, 0, 1], (ns, 1)),
               e_r_bound=pth["erb"].copy(), a_sets=np.array([s[0] for s in sets]), b_sets=np.array([s[1] for s in sets]))
    with contextlib.redirect_stdout(io.StringIO()):
        mpc.update([p.copy() for p in via["p_via"]], [r.copy() for r in via["r_via"]], [b.copy() for b in via["bp1"]], [b.copy() for b in via["br1"]],
                   [e.copy() for e in via["e_r_bound"]], [a.copy() for a in via["a_sets"]], [b.copy() for b in via["b_sets"]], [], st["v"],
                   p0=np.copy(st["p_lie"]), params=params)
    st["qf"] = st["q"].copy()
    steps = list(sc["steps"])
    assert len(steps) <= STEPS, name
    steps += [(IDLE, 0)] * (STEPS - len(steps))            # idle plants: every script has the same number of steps
    for plant, intended in steps:
        node_step(plant, intended)
    return trace, via


def main():
    base = get_default_params()
    robot = FakeRobot()
    q0 = np.array([0, 0, 0, -np.pi / 2, 0, np.pi / 2, 0.0])
    p0 = robot.fk(q0)
    params = Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)
    S = scripts()
    names = list(S)
    traces, vias = [], []
    for nm in names:
        t, via = run_script(nm, S[nm], robot, params, q0, p0)
        traces.append(t); vias.append(via)
        ev = [int(r["event"]) for r in t]
        print(f"{nm:18s} events {ev[1:]}  splits {[list(r['split_idxs'][1:3]) for r in t[1:8]]}  smallest margin {min(r['margin'] for r in t):.3e}")
    lbx0, ubx0 = traces[0][0]["lbx"].copy(), traces[0][0]["ubx"].copy()
    big = lambda a: np.nan_to_num(a, posinf=1e20, neginf=-1e20)
    free_cols = np.ones(lbx0.size, bool); free_cols[:40 * N:N] = False
    for t in traces:
        for r in t:          # the constant part of the bounds is the same everywhere: stored once
            assert np.array_equal(big(r["lbx"])[free_cols], big(lbx0)[free_cols]) and np.array_equal(big(r["ubx"])[free_cols], big(ubx0)[free_cols])
            del r["lbx"], r["ubx"]
    out = {k: np.array([[r[k] for r in t] for t in traces]) for k in sorted(traces[0][0].keys())}      # [script][step]...
    out.update(script=np.array(names), N=N, n_update=1, weights=params.weights, lbx_const=big(lbx0), ubx_const=big(ubx0))
    npts = np.array([len(v["p_via"]) for v in vias])
    out["via_n"] = npts
    for k in vias[0]:
        shp = (len(vias), 8 if k in ("p_via", "r_via") else 7) + vias[0][k].shape[1:]
        arr = np.zeros(shp)
        for i, v in enumerate(vias):
            arr[i, :len(v[k])] = v[k]
        out["via_" + k] = arr
    fname = os.path.join(G.OUT, "switch_cases.npz")
    np.savez_compressed(fname, **out)
    print("switch_cases.npz written:", len(names), "scripts x", len(traces[0]), "steps,", os.path.getsize(fname), "bytes")
    assert len(names) % 64 != 0 and os.path.getsize(fname) < 1 << 20


if __name__ == "__main__":
    main()
