"""Batched inverse kinematics on the MI355X (bmpc_ik / bmpc_ik_dev): the cases of tests/test_ik.py at B = 4096, the GPU against the CPU
build of the same kernel source, batch-position independence, the device path, misuse, NaN inputs and a busy handle."""
import ctypes

import numpy as np
import pytest

import emu_ik_lib as E
import ik_check_lib as C
import oracle_lib as O
from boundplanner_amd import robots

pytestmark = pytest.mark.gpu
LO, HI = C.limits(robots.IIWA14)
B = 4096


@pytest.fixture(scope="module")
def be():
    from boundplanner_amd.solver import HipBoundMPC
    b = HipBoundMPC(10)
    yield b
    b.close()


@pytest.fixture(scope="module")
def reach():
    pd, rd, q0, _ = C.reachable(np.random.default_rng(10), B)
    return pd, rd, q0


def test_reachable(be, reach):
    pd, rd, q0 = reach
    r = be.ik(pd, rd, q0)
    assert C.reached(r).mean() >= 0.99, np.bincount(r["status"])
    assert ((r["q"] >= LO) & (r["q"] <= HI)).all()
    pe, re = C.errors(r["q"], pd, rd)
    assert np.abs(pe - r["pos_err"]).max() <= 1e-9 and np.abs(re - r["rot_err"]).max() <= 1e-9


def test_gpu_against_cpu_build_of_the_same_source(be, reach):
    pd, rd, q0 = reach
    r, e = be.ik(pd, rd, q0), E.ik(pd, rd, q0)
    both = C.reached(r) & C.reached(e)                    # (status 0 can also be a stationary point that misses the target)
    assert both.mean() >= 0.99
    assert (r["cost"][both] <= 1e-15).all() and (e["cost"][both] <= 1e-15).all()
    close = np.abs(r["q"] - e["q"]).max(1) <= 1e-6
    print(f"q within 1e-6 of the CPU build: {close.mean():.4f}")
    assert close.mean() >= 0.99


def test_active_bounds(be):
    pd, rd, q0 = C.beyond_bound(np.random.default_rng(11), 1024)
    r = be.ik(pd, rd, q0)
    assert C.check_active_bounds(r, pd, rd, LO, HI) >= 1


def test_unreachable(be):
    pd, rd, q0 = C.unreachable(np.random.default_rng(12), 256)
    r = be.ik(pd, rd, q0)
    assert (C.cost(r["q"], pd, rd) <= C.cost(q0, pd, rd)).all()
    pg = C.proj_grad(r["q"], C.grad(r["q"], pd, rd), LO, HI)
    claimed = r["status"] != 1
    assert (pg[claimed] <= 1e-6).all() and claimed.mean() >= 0.9


def test_multi_start(be):
    rng = np.random.default_rng(13)
    pd, rd, q0 = C.behind(rng, 1024)
    r1, r16 = be.ik(pd, rd, q0, n_seeds=1), be.ik(pd, rd, q0, n_seeds=16)
    assert (r16["cost"] <= r1["cost"]).all()
    w = r16["seed"] == 0
    for k in r1:
        assert np.array_equal(r16[k][w], r1[k][w]), k
    assert C.reached(r16).sum() > C.reached(r1).sum()
    r64 = be.ik(pd[:64], rd[:64], q0[:64], n_seeds=64)
    assert (r64["cost"] <= r16["cost"][:64]).all()


def test_gen3():
    from boundplanner_amd.solver import HipBoundMPC
    O.set_robot(robots.GEN3)
    try:
        lo, hi = C.limits(robots.GEN3)
        pd, rd, q0, _ = C.reachable(np.random.default_rng(14), B, robots.GEN3)
        g = HipBoundMPC(10, robot="gen3")
        r = g.ik(pd, rd, q0)
        g.close()
        assert C.reached(r).mean() >= 0.99, np.bincount(r["status"])
        assert ((r["q"] >= lo) & (r["q"] <= hi)).all()
    finally:
        O.set_robot(None)


def test_batch_position_independence_bitwise(be, reach):
    pd, rd, q0 = reach
    i = 17
    alone = be.ik(pd[i:i + 1], rd[i:i + 1], q0[i:i + 1], n_seeds=4)
    idx = np.arange(4097) % B
    idx[4000] = i
    big = be.ik(pd[idx], rd[idx], q0[idx], n_seeds=4)
    idx = np.arange(65536) % B
    idx[65535] = i
    huge = be.ik(pd[idx], rd[idx], q0[idx], n_seeds=4)
    for k in alone:
        assert np.array_equal(alone[k][0], big[k][4000]), k
        assert np.array_equal(alone[k][0], huge[k][65535]), k


def test_device_path_bitwise(be, reach):
    import torch
    pd, rd, q0 = reach
    ref = be.ik(pd, rd, q0, n_seeds=2, lo=LO, hi=HI)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lo_t, hi_t = T(np.broadcast_to(LO, (B, 7))), T(np.broadcast_to(HI, (B, 7)))
    out = be.ik_dev(T(pd), T(rd.reshape(B, 3, 3)), T(q0), n_seeds=2, lo=lo_t, hi=hi_t)
    torch.cuda.current_stream().synchronize()
    for k in ref:
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
    out = be.ik_dev(T(pd), T(rd.reshape(B, 3, 3)), T(q0), n_seeds=2)      # the robot's limits
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(out["q"].cpu().numpy(), ref["q"])


def test_misuse_returns_1_and_leaves_the_handle_usable(be, reach):
    pd, rd, q0 = (np.ascontiguousarray(a[:8]) for a in reach)
    P = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    q = np.zeros((8, 7))
    call = lambda Bn, ns, p=P(pd), qq=P(q): be.lib.bmpc_ik(be._h, Bn, ns, None, p, P(rd), P(q0), None, None, qq, None, None, None,
                                                            None, None, None)
    for ns in (0, 3, 6, 128, -1):
        assert call(8, ns) == 1
    assert call(-1, 1) == 1
    assert call(8, 1, p=None) == 1
    assert call(8, 1, qq=None) == 1
    assert call(0, 1) == 0
    o = be._ik_opts(dict(lambda0=0.0))
    assert be.lib.bmpc_ik(be._h, 8, 1, ctypes.byref(o), P(pd), P(rd), P(q0), None, None, P(q), None, None, None, None, None, None) == 1
    assert call(8, 1) == 0
    r = be.ik(pd, rd, q0)
    assert np.array_equal(r["q"], q) and (r["status"] == 0).all()


def test_nan_is_status_3_for_that_instance_only(be, reach):
    pd, rd, q0 = (np.array(a[:64]) for a in reach)
    pd[5, 2] = np.nan
    r = be.ik(pd, rd, q0, n_seeds=8)
    assert r["status"][5] == 3
    assert (np.delete(r["status"], 5) == 0).all()


def test_busy_handle_returns_4(reach):
    import torch
    from boundplanner_amd import scenes
    from boundplanner_amd.solver import HipBoundMPC
    N, Bs = 10, 64
    h = HipBoundMPC(N)
    batch = scenes.make_batch(Bs, N, 1024, h.fk)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x0, lbx, ubx, p = (T(batch[k]) for k in ("x0", "lbx", "ubx", "p"))
    x, f, viol = torch.empty_like(x0), torch.empty(Bs, dtype=torch.float64, device="cuda"), torch.empty(Bs, dtype=torch.float64, device="cuda")
    it, st = (torch.empty(Bs, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    pd, rd, q0 = (np.ascontiguousarray(a[:8]) for a in reach)
    P = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    q = np.zeros((8, 7))
    h.debug_spin(1500)                       # the async solve queues behind this: it is certainly in flight below
    h.solve_dev_async(Bs, x0.data_ptr(), lbx.data_ptr(), ubx.data_ptr(), p.data_ptr(), x.data_ptr(), f.data_ptr(), it.data_ptr(),
                      st.data_ptr(), viol.data_ptr())
    rc = h.lib.bmpc_ik(h._h, 8, 1, None, P(pd), P(rd), P(q0), None, None, P(q), None, None, None, None, None, None)
    d_pd, d_rd, d_q0, d_q = T(pd), T(rd), T(q0), T(q)
    rc_dev = h.lib.bmpc_ik_dev(h._h, 8, 1, None, d_pd.data_ptr(), d_rd.data_ptr(), d_q0.data_ptr(), None, None, d_q.data_ptr(),
                               None, None, None, None, None, None, None)
    h.wait()
    assert rc == 4 and rc_dev == 4
    assert h.ik(pd, rd, q0)["status"].tolist() == [0] * 8
    h.close()
