"""k_curv's curvature block evaluated column by column: curvature_emit against the one-nest formulation it replaced (no GPU).

curvature_emit (bmpc_pair_kernels.hpp) evaluates the q x q block of the second-order kinematic terms column by column on copies of
the kinematics, so that nothing stays alive over the whole block; every entry is the same sequence of operations as before.
tests/emu/emu_curv.cpp keeps the earlier formulation as a test-only template and evaluates it in double (what the kernel computed
before) and in long double (the value both are measured against), on the kinematics of the same joint configurations.

Sample: 2000 random configurations with random velocities, forces and rank-2 vectors (forces over four decades), 200 of them again
with dq = 0, and every one of the 27 force components alone (Fp, Fv, Fc; rank-2 term off), each at 8 configurations with a random
dq and at 2 with dq = 0 -- so that each term of the block is exercised without the others.

Conditions: every entry of curvature_emit equals the earlier formulation's bitwise, and its worst error relative to the largest
entry of the block, against the long double values, is at most 4 x the earlier formulation's on the same sample (the bound a
reassociated form would have to meet; the first condition implies it).  Both worst errors are printed.

What this test can and cannot show: in this CPU build the opaque copies are plain copies (BMPC_PIN is empty), so it pins the ORDER
of evaluation -- columns outermost, per entry the same operations on the same values -- against a slip in the rewritten loops.
That the GPU code computes the same block is checked on the GPU: tests/test_curvature_gpu.py against the emulator, and
tests/test_hessian_pin_gpu.py against the oracle and the reference's probes.
"""
import ctypes

import numpy as np
import pytest

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
QLIM = np.array([2.96, 2.09, 2.96, 2.09, 2.96, 2.09, 3.05])      # iiwa14 joint ranges (rad)


def _sample(rng):
    def general(n, zero_dq):
        s = dict(q=rng.uniform(-1, 1, (n, 7)) * QLIM, dq=np.zeros((n, 7)) if zero_dq else rng.normal(size=(n, 7)),
                 Fp=rng.normal(size=(n, 3)) * 10 ** rng.uniform(-2, 2, (n, 1)), Fv=rng.normal(size=(n, 6)) * 10 ** rng.uniform(-2, 2, (n, 1)),
                 Fc=rng.normal(size=(n, 18)) * 10 ** rng.uniform(-2, 2, (n, 1)), sa=rng.normal(size=(n, 7)), sbq=rng.normal(size=(n, 7)),
                 sbdq=rng.normal(size=(n, 7)), sc1=rng.normal(size=n))
        return s

    def single(n, zero_dq):
        """each of the 27 force components alone, n configurations each, no rank-2 term"""
        m = 27 * n
        F = np.zeros((m, 27))
        F[np.arange(m), np.repeat(np.arange(27), n)] = rng.normal(size=m) * 10 ** rng.uniform(-2, 2, m)
        return dict(q=rng.uniform(-1, 1, (m, 7)) * QLIM, dq=np.zeros((m, 7)) if zero_dq else rng.normal(size=(m, 7)),
                    Fp=F[:, :3], Fv=F[:, 3:9], Fc=F[:, 9:], sa=np.zeros((m, 7)), sbq=np.zeros((m, 7)), sbdq=np.zeros((m, 7)), sc1=np.zeros(m))

    parts = [general(2000, False), general(200, True), single(8, False), single(2, True)]
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}


@pytest.fixture(scope="module")
def compared():
    lib = ctypes.CDLL(emu_build.build("emu_curv.cpp", "libbmpc_emucurv.so", ("-O1", "-g")))
    s = _sample(np.random.default_rng(20260))
    n = len(s["q"])
    assert n >= 2000
    out = {k: np.zeros((n, 2)) for k in ("err_new", "err_old", "scale")}
    out["new"], out["old"] = np.zeros((n, 98)), np.zeros((n, 98))
    P = lambda a: a.ctypes.data_as(_dp)
    rc = lib.emu_curv_compare(n, *(P(s[k]) for k in ("q", "dq", "Fp", "Fv", "Fc", "sa", "sbq", "sbdq", "sc1")),
                              *(P(out[k]) for k in ("err_new", "err_old", "scale", "new", "old")))
    assert rc == 0
    return s, out


@pytest.mark.parametrize("blk,name", [(0, "q x q"), (1, "q x dq")])
def test_block_is_bitwise_the_one_nest_formulation(compared, blk, name):
    s, o = compared
    sc = o["scale"][:, blk]
    live = sc > 0
    assert live.sum() >= 2000
    # an exactly vanishing block (no term of it is switched on) vanishes exactly in both
    assert not o["new"][~live, 49 * blk:49 * (blk + 1)].any() and not o["old"][~live, 49 * blk:49 * (blk + 1)].any()
    rel_new, rel_old = o["err_new"][live, blk] / sc[live], o["err_old"][live, blk] / sc[live]
    worst_new, worst_old = rel_new.max(), rel_old.max()
    print(f"{name} block, {live.sum()} samples: worst error / max|block| against long double: column by column {worst_new:.3g}, "
          f"one nest {worst_old:.3g} (ratio {worst_new / worst_old:.2f}); medians {np.median(rel_new):.3g}, {np.median(rel_old):.3g}", flush=True)
    assert np.array_equal(o["new"][:, 49 * blk:49 * (blk + 1)], o["old"][:, 49 * blk:49 * (blk + 1)]), "not the same operations as the one-nest formulation"
    assert worst_old < 1e-13, "the reference evaluation itself is off"
    assert worst_new <= 4 * worst_old


def test_sample_exercises_each_term_alone(compared):
    """the single-force rows: a nonzero q x q block from each force component alone with dq != 0, and from Fp / Fc alone with dq = 0"""
    s, o = compared
    F = np.concatenate([s["Fp"], s["Fv"], s["Fc"]], axis=1)
    alone = ((F != 0).sum(axis=1) == 1) & ~s["sa"].any(axis=1)
    comp = np.argmax(F != 0, axis=1)
    moving = s["dq"].any(axis=1)
    for c in range(27):
        assert (o["scale"][alone & moving & (comp == c), 0] > 0).sum() >= 8
        rest = o["scale"][alone & ~moving & (comp == c), 0]
        assert len(rest) >= 2 and ((rest == 0).all() if 3 <= c < 9 else (rest > 0).all())
