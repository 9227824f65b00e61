"""The orientation block of the device loop (csrc/bmpc_loop.hpp: lp_rotvec_to_mat, lp_mat_to_rotvec, lp_euler_zyx, lp_jac_inv,
lp_initial_rot_errors, the dual basis v1..v3, lp_integrate_rot_ref) against tests/orientation_lib.py, an extended-precision
reference written from the definitions: the CPU build of the identical source (tests/emu/emu_loop.cpp), helper by helper and through
whole loop_prepare / loop_finish calls, and the host mirror (so3.py on scipy), whose worst deviations are the yardstick
(orientation_lib.HOST_WORST; the device code gets 32 times that).  The families reach what the closed-loop traces never do: error
angles from 0 to a half turn across the series switches, a pitch of the Euler split next to and at +-90 deg (gimbal lock), the
+pi rule of the outer angles, end-effector orientations at a half turn, |omega| on both sides of 1e-4 and a rotation reference
that crosses the half turn."""
import warnings

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import emu_loop_lib as E
import oracle_lib as O
import orientation_lib as L
from boundplanner_amd import so3
from boundplanner_amd.device_loop import state_view
from boundplanner_amd.params import Params, get_default_params
from boundplanner_amd.robot_model import RobotModel

N = 6


def scipy_euler(M):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "Gimbal lock detected": the lock cases are here on purpose
        return R.from_matrix(M).as_euler("zyx")


class Host:
    """The host mirror: so3.py and the scipy calls it is made of."""
    exp = staticmethod(lambda v: R.from_rotvec(v).as_matrix())
    log = staticmethod(lambda M: R.from_matrix(M).as_rotvec())
    jac = staticmethod(lambda v, sign: so3.jac_SO3_inv_right(v) if sign > 0 else so3.jac_SO3_inv_left(v))
    integrate = staticmethod(so3.integrate_rotation_reference)

    @staticmethod
    def euler(M):
        e = scipy_euler(M)
        for i in (0, 2):                          # the +pi rule as so3.compute_initial_rot_errors applies it
            if abs(abs(e[i]) - np.pi) < 1e-12:
                e[i] = np.pi
        return e

    @staticmethod
    def initial_errors(pr, pr_ref, dpn, br1, br2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return so3.compute_initial_rot_errors(pr, pr_ref, dpn, br1, br2)


class Emu:
    """The CPU build of bmpc_loop.hpp."""
    exp = staticmethod(lambda v: E.so3(v, np.eye(3))[0])
    log = staticmethod(lambda M: E.so3(np.zeros(3), M)[1])
    euler = staticmethod(lambda M: E.so3(np.zeros(3), M)[2])
    jac = staticmethod(E.jac_inv)
    initial_errors = staticmethod(E.initial_rot_errors)
    integrate = staticmethod(E.integrate_rot_ref)


def test_reference_library_is_consistent():
    """The definitions against each other: log inverts exp up to the half turn, the Euler split rebuilds its matrix, the adjugate
    inverts, and the reference's Jacobian formula is the derivative it stands for (right for +1, left for -1) up to its 1e-6."""
    rng = np.random.default_rng(1)
    for a in L.ANGLES:
        v = L.ld(L.unit(rng)) * L.LD(a)
        M = L.exp(v)
        assert L.defect(M) < 1e-18 and abs(float(L.angle(M)) - min(a, float(L.PI))) < 1e-17 + 1e-18 / max(float(L.PI) - a, 1e-9)
        if float(L.PI) - a > 1e-8:
            assert np.abs(L.log(M) - v).max() < 1e-18 / np.sin(L.LD(max(a, 1.0)))
        e = L.ld(rng.uniform(-1, 1, size=3) * [3.0, 1.5, 3.0])
        assert np.abs(L.euler_exact(L.euler_build(e)) - e).max() < 1e-17
        assert np.abs(L.inv3(M + 0.1) @ (M + 0.1) - np.eye(3)).max() < 1e-17
        if 0 < a <= 3.0:
            for sign in (+1, -1):
                assert np.abs(L.jac_inv_true(v, sign) - L.jac_inv_formula(v, sign)).max() < L.jac_quirk_bound(v)
    assert len(L.ANGLES) == 14 and len(L.PITCHES) == 10 and all(abs(e0) > 0.1 and abs(e2) > 0.1 for e0, e2 in L.OUTER)


def test_host_mirror_helpers():
    """so3.py through the same reference.  Its worst figures are what HOST_WORST records (rounded up), so this passes at 32 times
    its own error by construction; it is here so that a change of so3.py or of scipy that moves them is seen."""
    W = L.Worst()
    L.check_helpers(Host, W, scipy_euler)
    W.report("host mirror, helpers: worst deviation / bound")
    assert not W.failures(), W.failures()


def test_cpu_build_helpers():
    W = L.Worst()
    L.check_helpers(Emu, W, scipy_euler)
    W.report("CPU build of bmpc_loop.hpp, helpers: worst deviation / bound")
    assert not W.failures(), W.failures()


def _rollouts():
    """The states of all rollout cases before loop_prepare, the oracle's R_ee per case, the layout."""
    from test_device_loop import _rollout_state
    base = get_default_params()
    params = Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)
    lay, robot = E.layout(), RobotModel(O.fk_batch)
    q = np.array(L.Q_ALL)
    Ree = O.fk_batch(q)["ee_rot"]
    bases = [_rollout_state(lay, params, robot, q[i], q[i])[1] for i in range(len(q))]
    cases = L.rollout_cases()
    S = np.array([bases[c["qi"]] for c in cases])
    for r, c in enumerate(cases):
        L.install(state_view(lay, S[r]), c, Ree[c["qi"]])
    assert all(float(L.PI - L.angle(Ree[len(L.Q_GENERIC) + i])) < 1e-6 for i in range(len(L.Q_HALF_TURN)))
    return dict(lay=lay, params=params, cases=cases, S=S, Ree=Ree, robot=robot)


@pytest.fixture(scope="module")
def rollouts():
    return _rollouts()


def test_cpu_build_whole_prepare_and_finish(rollouts):
    lay, cases = rollouts["lay"], rollouts["cases"]
    W, left_out = L.Worst(), {"structured": [0, 0], "random": [0, 0]}
    fams = set()
    for r, c in enumerate(cases):
        S = rollouts["S"][r].copy()
        V0 = {k: v.copy() for k, v in state_view(lay, S).items()}
        prev = np.zeros(44 * N + 6)
        x0, _, _, p = E.prepare(N, S, prev)
        V1 = {k: v.copy() for k, v in state_view(lay, S).items()}
        L.check_prepare_one(W, c, V0, V1, p, rollouts["Ree"][c["qi"]], left_out)
        assert (x0[31 * N:34 * N].reshape(3, N) == V1["p_lie"][3:, None]).all()          # the cold start carries log R_ee
        E.finish(N, rollouts["params"].dt, S, L.plant(N, x0, V1, c), prev, 0, 0.0)
        V2 = state_view(lay, S)
        assert V2["accept"][0] == 1.0 and V2["dead"][0] == 0.0
        L.check_finish_one(W, c, V1, V2)
        fams.update(L.fam_of(t) for t in c["tags"])
    L.check_left_out(left_out)
    assert fams == {"small", "mid", "half", "near", "lock", "pi_outer"} and len(cases) % 64 != 0
    W.report(f"CPU build, loop_prepare + loop_finish over {len(cases)} rollouts (dual basis left out: {left_out}): worst deviation / bound")
    assert not W.failures(), W.failures()


def host_prepare(V0, p_lie):
    """What BoundMPC.prepare computes of the orientation block, in the fields of the device state."""
    S4 = lambda n: np.array(V0[n]).reshape(3, 4)
    br1, br2, dpn = np.array(V0["rp_br1"]).reshape(-1, 3)[:4].T, np.array(V0["rp_br2"]).reshape(-1, 3)[:4].T, S4("rp_dpdn")
    prs = [np.array(V0["pr_ref"])] + [S4("rp_r_taud")[:, i] for i in range(1, 4)]
    out = np.zeros((4, 3, 4))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(4):
            out[:, :, i] = so3.compute_initial_rot_errors(p_lie[3:], prs[i], dpn[:, i], br1[:, i], br2[:, i])
    v1, v2, v3 = np.full((3, 4), np.nan), np.full((3, 4), np.nan), np.full((3, 4), np.nan)
    jr, jl = so3.jac_SO3_inv_right(out[0][:, 0]), so3.jac_SO3_inv_left(out[0][:, 0])
    for i in range(4):       # segment by segment: where [g h k] is singular the host raises (those segments are left out of the check)
        try:
            v1[:, [i]], v2[:, [i]], v3[:, [i]], _, _ = so3.orientation_projection_vectors(
                out[0][:, [0]], out[1][:, [i]], out[2][:, [i]], br1[:, [i]], br2[:, [i]], dpn[:, [i]])
        except np.linalg.LinAlgError:
            pass
    return dict(p_lie=p_lie, dtau=out[0].T.ravel(), dtau_par=out[1].T.ravel(), dtau_o1=out[2].T.ravel(), dtau_o2=out[3].T.ravel(),
                v1=v1.ravel(), v2=v2.ravel(), v3=v3.ravel(), jac_l=jl.ravel(), jac_r=jr.ravel())


def test_host_mirror_whole_prepare_and_finish(rollouts):
    """The host mirror through the checks of the whole calls (see test_host_mirror_helpers for why it is kept)."""
    lay, cases = rollouts["lay"], rollouts["cases"]
    W, left_out = L.Worst(), {"structured": [0, 0], "random": [0, 0]}
    for r, c in enumerate(cases):
        V0 = state_view(lay, rollouts["S"][r])
        V1 = host_prepare(V0, rollouts["robot"].fk(np.array(L.Q_ALL[c["qi"]])))
        L.check_prepare_one(W, c, V0, V1, None, rollouts["Ree"][c["qi"]], left_out)
        _, pr_ref, om, phi0, phi1 = c["fin"]
        phi = (phi1 - phi0) * (c["dp"] @ c["dp"]) + phi0
        V2 = dict(phi_current=np.array([phi]), pr_ref=so3.integrate_rotation_reference(pr_ref, om, phi0, phi),
                  iw_ref=c["pd_r"] + (phi - phi0) * om)
        L.check_finish_one(W, c, V1, V2)
    L.check_left_out(left_out)
    W.report("host mirror, whole calls: worst deviation / bound")
    assert not W.failures(), W.failures()


def measure_host():
    """Prints the table orientation_lib.HOST_WORST is made of: the host mirror's worst deviation over its scale per quantity and
    family, rounded up to two digits."""
    import math
    W = L.Worst(measure=True)
    L.check_helpers(Host, W, scipy_euler)
    ro = _rollouts()
    left_out = {"structured": [0, 0], "random": [0, 0]}
    for r, c in enumerate(ro["cases"]):
        V0 = state_view(ro["lay"], ro["S"][r])
        V1 = host_prepare(V0, ro["robot"].fk(np.array(L.Q_ALL[c["qi"]])))
        L.check_prepare_one(W, c, V0, V1, None, ro["Ree"][c["qi"]], left_out)
        _, pr_ref, om, phi0, phi1 = c["fin"]
        L.check_finish_one(W, c, V1, dict(phi_current=np.array([phi1]), pr_ref=so3.integrate_rotation_reference(pr_ref, om, phi0, phi1),
                                          iw_ref=c["pd_r"] + (phi1 - phi0) * om))
    W.report("host mirror: worst deviation over its scale")
    up = lambda x: 0.0 if x == 0 else math.ceil(x / 10 ** (math.floor(math.log10(x)) - 1)) * 10 ** (math.floor(math.log10(x)) - 1)
    print("HOST_WORST = {")
    for k in sorted(W.ratio):
        print(f'    "{k}": {up(W.ratio[k]):.1e},')
    print("}", left_out)


if __name__ == "__main__":
    measure_host()
