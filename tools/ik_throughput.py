"""Throughput of the batched inverse-kinematics kernel (bmpc_ik_dev) on one MI355X; prints one JSON line.

    timeout -k 10 120 python tools/ik_throughput.py

Reachable iiwa14 targets (FK of q* uniform in the box, seeds q* + N(0, 0.3^2) clipped) for B in {4096, 65536, 262144} x n_seeds in
{1, 8}.  Kernel time from HIP events on the current stream: 3 warm-up calls, then the median of 20.  Iterations and the converged
fraction (status 0) of the last call."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from boundplanner_amd import robots
    from boundplanner_amd.solver import HipBoundMPC
    be = HipBoundMPC(10)
    lo, hi = np.array(robots.IIWA14["q_lower"]), np.array(robots.IIWA14["q_upper"])
    rng = np.random.default_rng(0)
    Bmax = 262144
    qs = rng.uniform(lo + 0.1, hi - 0.1, (Bmax, 7))
    f = be.fk(qs)
    q0 = np.clip(qs + rng.normal(0.0, 0.3, qs.shape), lo, hi)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pd_all, rd_all, q0_all = T(f["ee_pos"]), T(f["ee_rot"]), T(q0)
    res = {"metric": "ik_throughput", "unit": "solves/s", "runs": []}
    for B in (4096, 65536, 262144):
        pd, rd, qq = pd_all[:B].contiguous(), rd_all[:B].contiguous(), q0_all[:B].contiguous()
        for ns in (1, 8):
            out = be.ik_dev(pd, rd, qq, n_seeds=ns)
            ms = []
            for k in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                be.ik_dev(pd, rd, qq, n_seeds=ns, out=out)
                e1.record()
                e1.synchronize()
                if k >= 3:
                    ms.append(e0.elapsed_time(e1))
            it = out["iters"].cpu().numpy()
            st = out["status"].cpu().numpy()
            med = float(np.median(ms))
            res["runs"].append(dict(B=B, n_seeds=ns, kernel_ms=round(med, 4), solves_per_s=round(B / med * 1e3, 1),
                                    iters_p50=float(np.percentile(it, 50)), iters_p99=float(np.percentile(it, 99)), iters_max=int(it.max()),
                                    converged=round(float((st == 0).mean()), 6)))
    be.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
