"""Throughput of the batched convex-set kernel (bmpc_convex_sets_dev) on one MI355X against the host finder; prints one JSON line.

    timeout -k 10 900 python tools/convex_set_throughput.py [--host-seeds 50] [--max-b 65536]

Example scene (scenes.example_scene(), 12 boxes), free random seeds, point mode with fixed_mid=True (the planner's call) and
fixed_mid=False, for B = 1, 16, 256, 4096, 65536.  Kernel time from HIP events on the current stream (the call's 48-byte copy of the
workspace box included): 3 warm-up calls, then the median of 20.  Distribution of rounds and Newton steps of the largest batch; host
ms/set of ConvexSetFinder.find_set_around_point on the first --host-seeds seeds; plan_convex_set_path from (0.6, 0.1, 0.5) to the
example goal with and without the HIP backend (median of 3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_seeds(f, n, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((0, 3))
    while out.shape[0] < n:
        s = rng.uniform(f.e_min, f.e_max, (4 * n, 3))
        ok = np.ones(len(s), bool)
        for a, b in f.obs_sets:
            ok &= (s @ a.T - b).max(axis=1) > 1e-3
        out = np.vstack((out, s[ok]))
    return out[:n]


def plan_ms(backend, boxes, goal_p, goal_r):
    from boundplanner_amd.bound_planner import BoundPlanner
    ts = []
    for _ in range(3):
        pl = BoundPlanner(obstacles=boxes, e_p_max=0.5, seed=7, set_backend=backend)
        t0 = time.perf_counter()
        pl.plan_convex_set_path(np.array([0.6, 0.1, 0.5]), goal_p, goal_r, goal_r)
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ts)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-seeds", type=int, default=50)
    ap.add_argument("--max-b", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from boundplanner_amd import scenes
    from boundplanner_amd.bound_planner import BoundPlanner
    from boundplanner_amd.scenes import pack_scene
    from boundplanner_amd.solver import SETS_MAXOBS, HipBoundMPC, default_sets_fn
    boxes, _, goal_p, goal_r = scenes.example_scene()
    f = BoundPlanner(obstacles=boxes, e_p_max=0.5, seed=7).set_finder
    be = HipBoundMPC(10)
    sc = pack_scene(f.obs_sets, f.obs_points_sets, SETS_MAXOBS, min_nv=1, pad_empty=True)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sct = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    emin, emax = T(np.asarray(f.e_min, float)), T(np.asarray(f.e_max, float))
    seeds = free_seeds(f, args.max_b, 0)
    res = {"metric": "convex_set_throughput", "unit": "sets/s", "scene": "example (12 boxes)", "runs": []}
    for fixed_mid in (True, False):
        for B in [b for b in (1, 16, 256, 4096, 65536) if b <= args.max_b]:
            p = T(seeds[:B])
            out = be.convex_sets_dev(sct, emin, emax, p, fixed_mid=fixed_mid)
            ms = []
            for k in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                be.convex_sets_dev(sct, emin, emax, p, fixed_mid=fixed_mid, out=out)
                e1.record()
                e1.synchronize()
                if k >= 3:
                    ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            run = dict(fixed_mid=fixed_mid, B=B, kernel_ms=round(med, 4), sets_per_s=round(B / med * 1e3, 1),
                       ok=round(float((out["status"].cpu().numpy() == 0).mean()), 6))
            if B == min(65536, args.max_b):
                rd, nw = out["rounds"].cpu().numpy(), out["newton"].cpu().numpy()
                run.update(rounds_hist=np.bincount(rd, minlength=6).tolist(), newton_p50=float(np.percentile(nw, 50)),
                           newton_p99=float(np.percentile(nw, 99)), newton_max=int(nw.max()))
            res["runs"].append(run)
    for fixed_mid in (True, False):
        t0 = time.perf_counter()
        for s in seeds[:args.host_seeds]:
            f.find_set_around_point(s, fixed_mid=fixed_mid)
        res[f"host_ms_per_set_fixed_mid_{int(fixed_mid)}"] = round(1e3 * (time.perf_counter() - t0) / args.host_seeds, 2)
    res["plan_ms_host"] = plan_ms(None, boxes, goal_p, goal_r)
    res["plan_ms_hip"] = plan_ms(default_sets_fn(), boxes, goal_p, goal_r)
    be.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
