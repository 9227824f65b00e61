"""Batched convex free-space sets on the GPU (bmpc_convex_sets / HipBoundMPC.convex_sets): agreement with the host finder and
host-independent certificates at B = 4096, results independent of batch size and position (bitwise), a 65 536-seed batch, the
device-pointer entry on torch tensors, and the planner with the HIP backend against tests/golden/plan.npz."""
import os

import numpy as np
import pytest

import sets_check_lib as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(10)


@pytest.fixture(scope="module")
def finder():
    return SC.example_finder()


@pytest.fixture(scope="module")
def seeds(finder):
    return SC.free_seeds(finder, 4096, 11)


def _run(be, f, p0, p1=None, **kw):
    return be.convex_sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, p0, p1, **kw)


@pytest.mark.parametrize("fixed_mid", [True, False])
def test_gpu_sets_match_the_host_finder(be, finder, seeds, fixed_mid):
    r = _run(be, finder, seeds, fixed_mid=fixed_mid)
    assert (r["status"] == 0).all()
    for k in range(len(seeds)):
        SC.certificates(finder, r, k, seed=seeds[k] if fixed_mid else r["centre"][k])
    sub = np.arange(0, len(seeds), 8)          # the host finder takes ~80 ms per set: every 8th seed (512)
    rs = {key: v[sub] for key, v in r.items()}
    bad, msgs = SC.compare_points(finder, rs, seeds[sub], fixed_mid)
    print(f"fixed_mid={fixed_mid}: {bad} of {len(sub)} seeds differ from the host", msgs[:5])
    assert bad <= 0.01 * len(sub)


def test_gpu_segment_sets(be, finder):
    p0, p1 = SC.segments(finder, 256, 7)
    r = _run(be, finder, p0, p1)
    bad, msgs = SC.compare_segments(finder, r, p0, p1)
    assert bad <= 0.01 * len(p0), msgs
    assert r["collision"].sum() > 0


def test_gpu_sets_do_not_depend_on_batch_size_or_position(be, finder, seeds):
    perm = np.random.default_rng(3).permutation(len(seeds))
    rb = _run(be, finder, seeds[perm], fixed_mid=True)
    for k in (0, 1, 777, 4095):
        r1 = _run(be, finder, seeds[k:k + 1], fixed_mid=True)
        j = int(np.nonzero(perm == k)[0][0])
        for key in r1:
            assert np.array_equal(r1[key][0], rb[key][j]), (k, key)


def test_gpu_sets_65536(be, finder):
    p = SC.free_seeds(finder, 65536, 5)
    r = _run(be, finder, p, fixed_mid=True)
    assert (r["status"] == 0).all() and (r["nrows"] >= 6).all()
    print("rounds", np.bincount(r["rounds"]).tolist(), "newton median", int(np.median(r["newton"])))


def test_gpu_convex_sets_dev_equals_convex_sets(be, finder, seeds):
    import torch
    from boundplanner_amd.solver import pack_set_scene
    sc = pack_set_scene(finder.obs_sets, finder.obs_points_sets)
    dev = torch.device("cuda:0")
    sct = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, float)).to(dev)
    p = seeds[:512]
    out = be.convex_sets_dev(sct, t(finder.e_min), t(finder.e_max), t(p), fixed_mid=True)
    torch.cuda.synchronize()
    r = _run(be, finder, p, fixed_mid=True)
    for key in r:
        assert np.array_equal(out[key].cpu().numpy(), r[key]), key
    p0, p1 = SC.segments(finder, 64, 9)
    out = be.convex_sets_dev(sct, t(finder.e_min), t(finder.e_max), t(p0), t(p1))
    torch.cuda.synchronize()
    r = _run(be, finder, p0, p1)
    for key in r:
        assert np.array_equal(out[key].cpu().numpy(), r[key]), key


def test_planner_with_the_hip_backend(golden_dir):
    from test_convex_sets import check_plans
    from boundplanner_amd.solver import default_sets_fn
    check_plans(np.load(os.path.join(golden_dir, "plan.npz")), default_sets_fn())
