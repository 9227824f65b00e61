#!/usr/bin/env python3
"""Benchmark of the hot path: batched BoundMPC NLP solves on MI355X.

  python bench.py --gpus N --steps K --warmup W

N = 1: BASELINE.json configs[2] -- 8192 instances, randomized convex-set obstacles, horizon 20, iiwa14 (SURVEY.md
8(d) generator; step 0 is seed 8192, step s > 0 is seed [8192, s]: a fresh batch every step).
N > 1: BASELINE.json configs[3] -- one batch of 8192*N instances (seed 65536; shard r of step s is generated from seed
[65536, s, r]) cut into contiguous shards, one process per GPU, no data-path collective, RCCL all-gather of the solution
blocks.  Started either by the driver (`python -m torch.distributed.run ... bench.py --gpus N ...`) or by this script
itself: without WORLD_SIZE in the environment `--gpus N` launches the N ranks as a child `torch.distributed.run` before
anything touches the GPU, and exits with the child's code.  It refuses (non-zero exit) when fewer than N GPUs are visible.

One "step" = one pass of the hot path over one batch.  Inputs are resident in HBM when the timed region starts
(bmpc_solve_dev_async with device pointers).  Prints ONE JSON line on rank 0.

A plain run measures the headline only (`value`, `ms_per_step`).  `--full` adds everything else in the same line: solver
statistics and the roofline of the step-0 batch solved alone, the shard check of a multi-GPU run, one batch at a time, the
figures with the transfers inside, configs[4] and the CPU baseline.  `--dump-outputs DIR` writes what the last timed step
returned (x, f, viol, iters, status of its batch) as DIR/<name>.npy.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

# Four solver calls in flight need four hardware queues of their own; the HIP runtime's default is 4 per process, one of which
# the null stream holds (a fourth stream would share a queue and serialise).  Set before HIP initialises.
# 12: the four handles' streams + the upload / download streams of the leg with the transfers inside + the three rollout groups of
# the closed-loop leg, all in one process (with 8 the groups shared queues: 29.9 k instead of 48.6 k solves/s; `value` is the same
# with 8, 12 or 16).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HORIZON = 20
BATCH_PER_GPU = 8192
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
FP64_VEC_PEAK_TFLOPS = 78.6    # vector FP64 peak (spec); the binding resource of this kernel
MAX_DISTINCT = 16              # distinct batches resident at once (231 MB each); longer runs (and the warm-up) cycle through them
MAX_DISTINCT_MULTI = 8         # ... per rank of a multi-GPU run: 6 generator processes per rank build 8 batches in < 60 s
RIC_FLOPS_PER_STAGE = 1.13e5   # Riccati share of the SURVEY 8(d) stage model (F_stage = 1.2e5: n_x = 26, n_u = 9), per instance, stage, sweep
DUMP_BUDGET = 64_000_000       # bytes --dump-outputs may write in all


def alg_bytes_per_solve(N):
    # read x0 + write x + read p + read state0
    return 8 * (2 * (44 * N + 6) + 875 + 40)


def alg_flops_per_solve(N, iters):
    # iters * N * F_stage, F_stage = 1.2e5 (condensed stage n_x=26, n_u=9)
    return iters * N * 1.2e5


def kernel_src_sha():
    """Hash of the device sources the library was built from: profiles/pmc_traffic.json is stamped with it when the PMC passes are
    taken (tools/summarize_pmc.py), so that a traffic figure measured on an older build is flagged (the GPU box has no .git)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "boundplanner_amd", "csrc", "*.h*"))):
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def batch_seed(world, rank, step):
    """Seed of the batch rank `rank` solves in step `step` (see the module docstring)."""
    if world == 1:
        return 8192 if step == 0 else [8192, step]
    return [65536, step, rank]


def block_diffs(N, xa, xb):
    """max |xa - xb| per block of the decision vector (casadi_ocp_formulation.py:89-101), over the rows given."""
    blocks = {"q": (0, 7 * N), "dq": (7 * N, 14 * N), "ddq": (14 * N, 21 * N), "u": (21 * N, 28 * N),
              "p": (28 * N, 34 * N), "v": (34 * N, 40 * N), "slacks": (40 * N, 44 * N + 6)}
    d = np.abs(xa - xb)
    return {k: float(d[:, a:b].max()) if d.size else None for k, (a, b) in blocks.items()}


def usable_cpus():
    """CPUs this process may run on: the affinity mask, cut down by a cgroup CPU quota (a container can see every core of the
    host while its quota allows a few)."""
    n = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


# ---- problem instances ----
# scenes.make_batch draws everything for a batch from one random stream, in instance order, in the calling process, and maps
# the per-instance construction over its pool.  Those draws take ~2.5 s per batch: with many batches they, not the
# construction, set the generation time.  generate() therefore runs the draws of each batch in a worker too: the main process
# only computes the kinematics the draws need (on the GPU, recorded), the worker replays them into make_batch and hands back
# the per-instance jobs, which the pool builds.  The result is bitwise what make_batch returns for the same seed.

_FK_KEYS = ("ee_pos", "ee_rot", "col_pts")      # the kinematics outputs make_batch reads


def _fk_recorder(fk):
    """fk wrapper that keeps the input and the outputs make_batch reads of every call, in call order."""
    calls = []

    def rec(q, dq=None):
        r = fk(q, dq)
        calls.append((np.array(q, dtype=float), {k: r[k] for k in _FK_KEYS}))
        return r
    return rec, calls


def _fk_replayer(calls):
    """fk stand-in that returns the recorded outputs, and fails unless it is asked for exactly the recorded inputs."""
    it = iter(calls)

    def replay(q, dq=None):
        q0, r = next(it)
        if not np.array_equal(np.asarray(q, dtype=float), q0):
            raise RuntimeError("bench.py: the generator asked for other kinematics than were recorded")
        return r
    return replay


class _JobCapture:
    """Stands in for make_batch's pool: keeps the per-instance jobs instead of building them."""
    jobs = None

    def imap(self, fn, jobs, chunksize=1):
        self.jobs = jobs
        return iter([(0.0, 0.0, 0.0, 0.0, None)] * len(jobs))


def _draw_jobs(B, N, seed, fk_calls):
    """(worker) the random draws of make_batch for one batch -> its per-instance jobs."""
    from boundplanner_amd import scenes
    cap = _JobCapture()
    scenes.make_batch(B, N, seed, _fk_replayer(fk_calls), randomize_sets=True, pool=cap)
    return cap.jobs


def _build_chunk(jobs):
    """(worker) make_batch's per-instance construction over consecutive jobs -> x0, lbx, ubx, p stacked (one row per job)."""
    from boundplanner_amd import scenes
    res = [scenes._build_instance(j) for j in jobs]
    return tuple(np.array([r[i] for r in res], dtype=float) for i in range(4))


def generate(seeds, B, N, fk, pool=None):
    """Yields, seed by seed, the arrays x0, lbx, ubx, p of scenes.make_batch(B, N, seed, fk, randomize_sets=True).  `pool`: a
    fork pool of processes that never touch the GPU (None: everything in this process)."""
    from boundplanner_amd import scenes
    if pool is None:
        for seed in seeds:
            batch = scenes.make_batch(B, N, seed, fk, randomize_sets=True)
            yield {k: batch[k] for k in ("x0", "lbx", "ubx", "p")}
        return
    drawn = []
    for seed in seeds:
        rec, calls = _fk_recorder(fk)
        q_start, q_goal = scenes.sample_start_goal(np.random.default_rng(seed), rec, B)      # make_batch's kinematics calls, in order
        rec(q_start); rec(q_goal)
        drawn.append(pool.apply_async(_draw_jobs, (B, N, seed, calls)))
    chunk = 64
    built = []
    for d in drawn:
        jobs = d.get()
        built.append(pool.imap(_build_chunk, [jobs[i:i + chunk] for i in range(0, B, chunk)]))
    for res in built:
        out = {}
        for i, arrays in enumerate(res):
            for k, a in zip(("x0", "lbx", "ubx", "p"), arrays):
                if k not in out:
                    out[k] = np.empty((B, a.shape[1]))
                out[k][i * chunk:i * chunk + len(a)] = a
        yield out


def write_outputs(dirname, groups, budget=DUMP_BUDGET):
    """--dump-outputs: `groups` = [(prefix, {name: array with one row per instance})]; every array goes to
    dirname/<prefix><name>.npy as float64.  Each group may use an equal share of `budget`; a group larger than that is cut to a
    fixed, seeded sample of its rows (the same rows for all its arrays), whose indices go to <prefix>rows.npy."""
    os.makedirs(dirname, exist_ok=True)
    share = budget // max(1, len(groups))
    for prefix, arrays in groups:
        arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
        n = len(next(iter(arrays.values())))
        row_bytes = sum(a[0].nbytes for a in arrays.values())
        if n * row_bytes > share:
            k = share // (row_bytes + 8)
            rows = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
            arrays = {name: a[rows] for name, a in arrays.items()}
            arrays["rows"] = rows.astype(np.float64)
        for name, a in arrays.items():
            np.save(os.path.join(dirname, f"{prefix}{name}.npy"), a)


def visible_gpus():
    """GPUs this process would see, WITHOUT touching the HIP runtime (the launcher must not initialise the GPU before it starts
    its ranks): the KFD topology nodes that have SIMDs and whose render node this process may open (a container can list every GPU
    of the host in sysfs while only some /dev/dri/renderD* are passed in), cut down by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES."""
    n = 0
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        nodes = os.listdir(base)
    except OSError:
        nodes = []
    for node in nodes:
        try:
            with open(os.path.join(base, node, "properties")) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) > 0:
            minor = props.get("drm_render_minor")
            if minor is not None and int(minor) > 0 and not os.access(f"/dev/dri/renderD{int(minor)}", os.R_OK | os.W_OK):
                continue                      # listed, but not ours to open
            n += 1
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def launch_ranks(args):
    """`--gpus N` without a launcher: start N ranks as a child torch.distributed.run (a child process, before this
    process has touched the GPU -- never a re-exec) and return its exit code."""
    have = visible_gpus()
    if have < args.gpus and not args.rehearse_one_gpu:
        print(f"bench.py: --gpus {args.gpus} but only {have} GPU(s) visible; refusing to print a line for fewer ranks",
              file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32, help="timed batches (default 32: four streaming calls of eight batches; the steps cycle through 16 distinct batches)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=BATCH_PER_GPU, help="instances per GPU")
    ap.add_argument("--horizon", type=int, default=HORIZON)
    ap.add_argument("--hess", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="solver calls in flight (the straggler tail of one overlaps the bulk of "
                    "the next); 1: one at a time.  Default 4 (with GPU_MAX_HW_QUEUES=12, set above)")
    ap.add_argument("--merge", type=int, default=2, help="--pool 0 only: batches handed to the solver per call (they are "
                    "independent: a larger launch amortises the straggler tail over more bulk work)")
    ap.add_argument("--gate", type=float, default=1.0, help="start the next solver call when the others have < gate * their instances "
                    "active (1.0: at once)")
    ap.add_argument("--pool", type=int, default=16384, help="bmpc_opts.pool_slots: workspace slots of a solver handle.  > 0 (default): "
                    "the timed batches are handed over in `depth` solver calls, each streaming its instances through the pool "
                    "(a slot whose instance has finished takes the next one: one straggler tail per call, hidden behind the "
                    "other call).  0: every call holds all its instances (`merge` batches), `depth` calls in flight")
    ap.add_argument("--opt", action="append", default=[], help="solver option key=value (bmpc_opts field), A/B runs")
    ap.add_argument("--same-batch", action="store_true", help="every step solves the seed-8192 batch (profiling passes)")
    ap.add_argument("--gen-workers", type=int, default=None, help="processes building problem instances (0: in this process)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: solver statistics and roofline of "
                    "the step-0 batch solved alone, the shard check (--gpus N), one batch at a time, the transfers inside, configs[4], the "
                    "CPU baseline (the --no-* options below switch legs off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write x, f, viol, iters, status of the last timed step's batch "
                    "to DIR/<name>.npy (float64; a larger output than 64 MB in all is cut to a fixed, seeded sample of rows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the single-batch, PCIe-inclusive and closed-loop measurements")
    ap.add_argument("--no-closed-loop", action="store_true", help="skip the configs[4] leg")
    ap.add_argument("--rehearse-one-gpu", action="store_true", help="--gpus N on a box with ONE GPU: every rank uses device 0 and the all-gather "
                    "runs over gloo (RCCL refuses two ranks on one device).  Rehearses the launch, sharding, gather and timing path of "
                    "the N-rank run; the line it prints is marked and is NOT a scaling measurement")
    ap.add_argument("--closed-loop-steps", type=int, default=200, help="MPC steps of the configs[4] leg (4096 rollouts, N=30; the config has 200)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)

    from boundplanner_amd import scenes
    N, B = args.horizon, args.batch
    depth = max(1, min(args.depth if args.depth is not None else 4, 4))
    M = max(1, min(args.merge, 4))
    if args.pool > 0:
        M = max(1, min((args.steps + depth - 1) // depth, MAX_DISTINCT))      # the timed batches in `depth` streaming calls
    n_distinct = 1 if args.same_batch else min(max(args.steps, M), MAX_DISTINCT if world == 1 else MAX_DISTINCT_MULTI)
    n_distinct = M * ((n_distinct + M - 1) // M)
    # instance-building workers: forked BEFORE this process initialises the GPU; they never touch it
    pool = None
    n_workers = args.gen_workers if args.gen_workers is not None else max(0, min(32, usable_cpus() // max(1, world) - 1))
    if n_workers > 0 and n_distinct > 1:
        import multiprocessing as mp
        pool = mp.get_context("fork").Pool(n_workers)

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        if args.rehearse_one_gpu:
            local_rank = 0
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py: RCCL sees {dist.get_world_size()} ranks, --gpus {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    from boundplanner_amd.batch_stream import BatchStream, HipHandle
    from boundplanner_amd.solver import HipBoundMPC

    kw = {} if args.hess is None else {"hess": args.hess}
    for kv in args.opt:
        k_, v_ = kv.split("=")
        kw[k_] = float(v_) if ("." in v_ or "e" in v_) else int(v_)
    if args.pool > 0:
        kw["pool_slots"] = args.pool
    bes = [HipBoundMPC(N, device=local_rank, max_batch=min(M * B, args.pool) if args.pool > 0 else M * B, **kw) for _ in range(depth)]
    be = bes[0]
    n_w = be.n_w
    big = lambda a: np.nan_to_num(a, posinf=1e20, neginf=-1e20)

    # ---- problem instances: n_distinct fresh batches (steps cycle through them), resident in HBM ----
    t0 = time.time()
    host0 = None
    d = {k: torch.empty((n_distinct * B, be.n_p if k == "p" else n_w), dtype=torch.float64, device=dev) for k in ("x0", "lbx", "ubx", "p")}
    # fresh batches: at most MAX_DISTINCT(_MULTI) -- the ring of whole solver calls can round n_distinct up to twice that, and
    # generation is CPU-bound (~1 s per batch on 16 cores): slots past the fresh ones repeat them
    n_gen = 1 if args.same_batch else min(n_distinct, MAX_DISTINCT if world == 1 else MAX_DISTINCT_MULTI)
    for s, batch in enumerate(generate([batch_seed(world, rank, s) for s in range(n_gen)], B, N, be.fk, pool)):
        hb = {k: big(batch[k]) for k in ("x0", "lbx", "ubx", "p")}
        if s == 0:
            host0 = hb
        for k in d:
            d[k][s * B:(s + 1) * B] = torch.from_numpy(hb[k]).to(dev)
    for s in range(n_gen, n_distinct):      # slot s holds fresh batch s mod n_gen (--same-batch: the step-0 batch everywhere)
        r = s % n_gen
        for k in d:
            d[k][s * B:(s + 1) * B] = d[k][r * B:(r + 1) * B]
    if pool is not None:
        pool.close(); pool.join()
    t_gen = time.time() - t0

    def make_outs(n):
        return dict(x=torch.empty((n, n_w), dtype=torch.float64, device=dev), f=torch.empty(n, dtype=torch.float64, device=dev),
                    viol=torch.empty(n, dtype=torch.float64, device=dev), iters=torch.empty(n, dtype=torch.int32, device=dev),
                    status=torch.empty(n, dtype=torch.int32, device=dev))
    outs = [make_outs(M * B) for _ in range(depth)]      # one set of output buffers per handle in flight
    gathered = torch.empty((world * M * B, n_w), dtype=torch.float64, device=dev) if world > 1 else None
    torch.cuda.synchronize(dev)      # inputs complete before any handle's own stream reads them
    # the gather runs on torch's current stream; the next solve on the handle overwrites its x: wait for the read
    stream = BatchStream([HipHandle(b_) for b_ in bes], outs, d, B, merge=M, gate=args.gate, dist=dist, gathered=gathered,
                         sync_gather=lambda: torch.cuda.current_stream(dev).synchronize())

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    profiling_pass = args.full and world == 1 and depth == 1 and M == 1 and n_distinct == 1      # (the timed batch IS the lone batch below)
    if rank == 0 and profiling_pass:
        be.time_ric(True)
    stream.run(args.warmup)
    barrier()
    stream.kernel_ms.clear()
    t0 = time.perf_counter()
    stream.run(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    if args.dump_outputs and rank == 0:
        # the last timed step = the last batch of the last solver call (rows (m_last - 1) * B ... of its handle's outputs)
        m_last = args.steps - M * ((args.steps - 1) // M)
        o = outs[(stream.calls - 1) % depth]
        last = slice((m_last - 1) * B, m_last * B)
        groups = [("", {k: o[k][last].cpu().numpy() for k in ("x", "f", "viol", "iters", "status")})]
        if world > 1:           # the same step's x of every rank, as the all-gather of that call delivered it
            n = m_last * B
            groups.append(("gathered_", {"x": torch.cat([gathered[r * n + (m_last - 1) * B:(r + 1) * n] for r in range(world)]).cpu().numpy()}))
        write_outputs(args.dump_outputs, groups)

    total_solves = world * B * args.steps
    value = total_solves / elapsed
    gather_name = "gloo all-gather (one-GPU rehearsal)" if args.rehearse_one_gpu else "RCCL all-gather"
    out = {
        "metric": "MPC solves/sec (whole node), iiwa14 7-DOF, N=20",
        "value": value, "unit": "solves/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": (f"BASELINE configs[2]: {B}-batch, randomized convex-set obstacles, N={N}, cold start, tol 1e-5, "
                                "max_iter 100; a fresh batch every step" if world == 1 else
                                f"BASELINE configs[3]: one {world * B}-batch (seed 65536) cut into {world} contiguous shards of {B}, "
                                f"randomized convex-set obstacles, N={N}, cold start, {gather_name} of x"),
                   "value_is": "inputs resident in HBM when the timed region starts, pipelined solver calls (solver_handles_in_flight / "
                               "batches_per_solver_call): `value` EXCLUDES host<->device transfers.  The SURVEY 8(d) figure with the transfers "
                               "inside the same schedule is value_pcie_inclusive_pipelined; value_single_batch / value_pcie_inclusive are one batch at a time",
                   "batch_per_gpu": B, "horizon": N, "distinct_batches": n_distinct, "fresh_batches": n_gen,
                   "sharding": f"contiguous shards, no data-path collective, {gather_name} of x" if world > 1 else "single GPU",
                   "hess": int(be.opts.hess), "solver_handles_in_flight": depth,
                   "batches_per_solver_call": M, "batches_in_flight": depth * M, "pool_slots": args.pool},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return

    event_ms = float(np.mean(stream.kernel_ms)) if stream.kernel_ms else None

    # ---- untimed: the seed-of-step-0 batch alone on one handle -> solver statistics, parity sample, shard check ----
    one = BatchStream([HipHandle(be)], [outs[0]], {k: v[:B] for k, v in d.items()}, B, merge=1, dist=dist,
                      gathered=gathered, sync_gather=lambda: torch.cuda.current_stream(dev).synchronize())
    if not profiling_pass:
        if rank == 0:
            be.time_ric(True)       # HIP events around every launch of the Riccati kernel on the handle's stream: the roofline leg
        one.run(1)
    torch.cuda.synchronize(dev)
    ric = be.ric_stats() if rank == 0 else None
    if rank == 0:
        be.time_ric(False)
    x = outs[0]["x"][:B]
    it_np, st_np, viol_np = (outs[0][k][:B].cpu().numpy() for k in ("iters", "status", "viol"))
    ok = (st_np == 0) | (viol_np < 1e-4)            # the reference's acceptance test (BoundMPC.py:617)
    shard_check = None
    if world > 1:
        # batch independence across the sharding: rank 0 solves the first 512 instances of two different shards
        # alone and compares them bitwise with the rows the all-gather delivered
        ns = min(512, B)
        xg = gathered[:world * B].clone()
        heads = {k: torch.empty((world * ns, v.shape[1]), dtype=torch.float64, device=dev) for k, v in d.items()}
        for k, v in d.items():
            dist.all_gather_into_tensor(heads[k], v[:ns].contiguous())
        torch.cuda.synchronize(dev)
        if rank == 0:
            shard_check = {}
            for r in sorted({0, world - 1}):
                o = make_outs(ns)
                torch.cuda.synchronize(dev)
                HipHandle(be).solve_async(ns, {k: v[r * ns:(r + 1) * ns] for k, v in heads.items()}, o)
                be.wait()
                torch.cuda.synchronize(dev)
                same = bool(torch.equal(o["x"], xg[r * B:r * B + ns]))
                shard_check[f"shard{r}_first{ns}_bitwise_equal"] = same
                if not same:
                    raise SystemExit(f"bench.py: shard {r}: gathered solutions differ from a stand-alone solve")

    # GPU time per batch: with several calls in flight they overlap, so the per-batch share of the timed region is the
    # honest denominator (event_ms_per_batch = HIP events around one call on its own stream / its batches)
    k_ms = event_ms if depth == 1 else 1e3 * elapsed / args.steps
    ach_gbs = alg_bytes_per_solve(N) * B / (k_ms * 1e-3) / 1e9
    mean_it = float(it_np.mean())
    ach_tf = alg_flops_per_solve(N, mean_it) * B / (k_ms * 1e-3) / 1e12

    # HBM bytes of one batch from the PMC passes of tools/gpu_quick.sh / profile_round.sh (separate rocprofv3 --pmc runs of one
    # synchronous batch of this same workload), FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950; stamped with the
    # hash of the device sources it was taken on -- a figure from another build is reported as stale
    traffic, traffic_note, fetch_raw, write_raw, traffic_stale = None, None, None, None, None
    tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(tj) and (B, N) == (BATCH_PER_GPU, HORIZON):
        t = json.load(open(tj))
        fetch_raw, write_raw = t["fetch_bytes_raw"], t["write_bytes"]
        traffic = 2.0 * fetch_raw + write_raw
        traffic_stale = t.get("kernel_src_sha16") != kernel_src_sha()
        traffic_note = (f"profiles/pmc_traffic.json (device sources {t.get('kernel_src_sha16', 'unstamped')}): 2 x FETCH_SIZE {t['fetch_bytes_raw'] / 1e9:.1f} GB (gfx950 "
                        f"correction, MI355X_MICROARCH.md HBM section) + WRITE_SIZE {t['write_bytes'] / 1e9:.1f} GB per batch, all kernels")

    # roofline of the DOMINANT KERNEL, bmpc_k_ric (the backward Riccati sweep: ~40 % of a batch's kernel time): algorithmic flops of
    # its launches over their summed duration, measured live with HIP events around every launch on the handle's stream while the
    # step-0 batch is solved alone (no other call in flight: a launch's duration is its own).  An instance-iteration is one
    # backward sweep over the N-1 stages (retry sweeps -- Gauss-Newton fallback, delta_w escalation -- run in the same launch
    # and are not counted as work).  The tail regime (fewer than 512 live instances: bmpc_k_ric_att / _att_thr + bmpc_k_ric_sel, the
    # attempts of an iteration side by side; bmpc_k_ric_lat with BMPC_RIC_SPEC_BELOW=0) is reported beside it.
    roof = {"bound": "valu_fp64", "kernel": "bmpc_k_ric", "achieved": None, "peak": FP64_VEC_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": None}
    if ric is not None:
        ms_b, n_b, sw_b = ric["bmpc_k_ric"]
        ms_l, n_l, sw_l = ric["bmpc_k_ric_lat"]
        fl = RIC_FLOPS_PER_STAGE * (N - 1)
        if ms_b > 0:
            roof["achieved"] = sw_b * fl / (ms_b * 1e-3) / 1e12
            roof["frac"] = roof["achieved"] / FP64_VEC_PEAK_TFLOPS
        roof.update({"launches": int(n_b), "launch_ms_avg": ms_b / n_b if n_b else None, "launch_ms_sum": ms_b, "instance_iterations": int(sw_b),
                     "alg_flops_per_instance_iteration": fl,
                     "measured": "HIP events around every launch on the solver handle's stream (bmpc_debug_time_ric), the step-0 batch alone",
                     "latency_variant": {"kernel": "bmpc_k_ric_att(_thr) + bmpc_k_ric_sel (tail regime, < 512 live instances; bmpc_k_ric_lat when speculation is off)", "launches": int(n_l), "launch_ms_avg": ms_l / n_l if n_l else None,
                                         "launch_ms_sum": ms_l, "instance_iterations": int(sw_l)}})
        # the same kernel at full occupancy: its launches over the whole batch (the first super-steps of the solve, before anybody
        # has finished) -- what the per-kernel tables of DESIGN.md section 3 and the round-3 verdict's 0.13 refer to; `frac` above
        # averages over every bulk launch of the batch, down to 512 live instances
        ms_f, n_f, sw_f = ric.get("bmpc_k_ric_full_batch", (0.0, 0.0, 0.0))
        if ms_f > 0:
            roof["full_batch_launches"] = {"launches": int(n_f), "launch_ms_avg": ms_f / n_f, "instance_iterations": int(sw_f),
                                           "achieved": sw_f * fl / (ms_f * 1e-3) / 1e12, "frac": sw_f * fl / (ms_f * 1e-3) / 1e12 / FP64_VEC_PEAK_TFLOPS}
    roof.update({"traffic": traffic, "traffic_stale": traffic_stale, "traffic_note": traffic_note,
                 # measured HBM bytes of a batch (all kernels) over the per-batch time of THIS run: what the memory system sustains
                 "traffic_gbs": (traffic / (k_ms * 1e-3) / 1e9) if traffic else None,
                 "traffic_frac_of_peak": (traffic / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                 "fetch_size_raw_bytes": fetch_raw, "write_size_bytes": write_raw,
                 # SURVEY 8(d)'s HBM figure: compulsory bytes of a solve (x0, p, state in; x out) over the per-batch time
                 "hbm_alg_gbs": ach_gbs, "hbm_alg_frac": ach_gbs / HBM_PEAK_GBS, "alg_bytes_per_solve": alg_bytes_per_solve(N),
                 "per_batch_ms": k_ms, "event_ms_per_batch": event_ms})

    out.update({
        "solver": {"iters_mean": mean_it, "iters_p50": float(np.median(it_np)), "iters_p99": float(np.percentile(it_np, 99)),
                   "iters_max": int(it_np.max()), "converged_frac": float((st_np == 0).mean()),
                   "accepted_frac": float(ok.mean()), "gen_s": t_gen, "stats_of": "the step-0 batch solved alone"},
        "roofline": roof,
        # the whole path against the same peak: SURVEY 8(d)'s flop model of a solve over the per-batch time of the timed region
        "valu_fp64": {"achieved": ach_tf, "peak": FP64_VEC_PEAK_TFLOPS, "unit": "TFLOP/s",
                      "frac": ach_tf / FP64_VEC_PEAK_TFLOPS, "alg_flops_per_solve": alg_flops_per_solve(N, mean_it)},
    })
    if shard_check is not None:
        out["shard_check"] = shard_check
    if args.rehearse_one_gpu:
        out["rehearsal"] = f"{world} ranks sharing ONE GPU, all-gather over gloo: exercises the N-rank code path, not a scaling measurement"

    if rank == 0 and not args.no_extra:
        # SURVEY 8(d) as written: ONE batch at a time (depth 1, merge 1) ...
        solo = BatchStream([HipHandle(be)], [outs[0]], {k: v[:B] for k, v in d.items()}, B, merge=1)     # no gather: rank 0 only
        t1 = time.perf_counter()
        solo.run(2)
        torch.cuda.synchronize(dev)
        out["value_single_batch"] = 2 * B / (time.perf_counter() - t1)
        # ... and through the host-pointer entry: H2D of x0, lbx, ubx, p and D2H of x, f, iters, status, viol inside the time
        be.solve_batch(host0["x0"][:64], host0["lbx"][:64], host0["ubx"][:64], host0["p"][:64])     # staging buffers
        t1 = time.perf_counter()
        rh = be.solve_batch(host0["x0"], host0["lbx"], host0["ubx"], host0["p"])
        out["value_pcie_inclusive"] = B / (time.perf_counter() - t1)
        out["pcie_note"] = "bmpc_solve with pageable host arrays: 3 x 58 MB + 57 MB H2D, 58 MB D2H per batch inside the timed call"
        assert np.array_equal(rh["x"], x.cpu().numpy()), "host-pointer and device-pointer entries disagree"

    if rank == 0 and not args.no_extra and args.pool > 0:
        # ... and the same pipelined schedule as `value` WITH its transfers: inputs from pinned host memory by asynchronous copies
        # on the handles' streams, outputs back to pinned host memory; 231 MB in, 58 MB out per batch
        from boundplanner_amd.batch_stream import HostBatchStream
        nd_h = min(n_distinct, depth * M)
        pinned = {k: torch.empty((nd_h * B, v.shape[1]), dtype=torch.float64, pin_memory=True) for k, v in d.items()}
        for k, v in d.items():
            pinned[k].copy_(v[:nd_h * B])
        torch.cuda.synchronize(dev)
        hs = HostBatchStream(bes, pinned, B, M, dev)
        hs.run(depth * M)                                    # warm-up: staging buffers touched, pools allocated
        t1 = time.perf_counter()
        hs.run(args.steps)
        torch.cuda.synchronize(dev)
        out["value_pcie_inclusive_pipelined"] = args.steps * B / (time.perf_counter() - t1)
        out["pcie_pipelined_note"] = (f"{depth} solver calls in flight, each: hipMemcpyAsync of x0, lbx, ubx, p for {M} batches from pinned host memory (upload "
                                      "stream; a handle's next call is fetched while its current one is solved) -> streaming solve -> x, f, iters, status, viol "
                                      "back to pinned host memory (download stream); the timed region starts with nothing uploaded")
        same = all(bool(torch.equal(hs.h_out[0][k][:B], outs[0][k][:B].cpu())) for k in ("x", "iters", "status")) if nd_h >= 1 and args.steps % (depth * M) == 0 else None
        out["pcie_pipelined_first_batch_equals_device_resident"] = same
        del hs, pinned

    if rank == 0 and world == 1 and not args.no_extra and not args.no_closed_loop:
        # BASELINE configs[4] (tools/closed_loop_device.py; --closed-loop-steps MPC steps, 200 = the config): 4096 rollouts,
        # N=30, fixed sets, the reference's warm start, device-resident loop, three rollout groups in flight
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import closed_loop_device as CL
            cl = CL.run(CL.parser().parse_args(["--steps", str(args.closed_loop_steps), "--chunk", str(max(1, args.closed_loop_steps // 2))]), progress=False)
            out["closed_loop_configs4"] = {k: cl[k] for k in ("config", "groups", "solves", "wall_s", "solves_per_s", "ms_per_step", "iters_mean", "iters_p99",
                                                              "fail_frac", "dead_frac", "reached_end_frac")}
        except Exception as e:           # (reported, not fatal: the headline above is measured)
            out["closed_loop_configs4"] = {"error": repr(e)}

    if rank == 0 and not args.no_cpu_baseline:
        import oracle_lib as O               # cpu_baseline leg only
        cores = len(os.sched_getaffinity(0))
        nthr = min(cores, 64)
        ns = min(B, 128 * nthr)         # ~12 s of host work at ~670 solves/s on 64 threads
        hess = int(be.opts.hess)
        t0 = time.perf_counter()
        ro = O.solve_batch(N, host0["x0"][:ns], host0["lbx"][:ns], host0["ubx"][:ns], host0["p"][:ns], nthreads=nthr, hess=hess)
        tc = time.perf_counter() - t0
        x_gpu = x[:ns].cpu().numpy()
        both = (ro["status"] == 0) & (st_np[:ns] == 0)
        same_it = both & (ro["iters"] == it_np[:ns])
        # a genuine CasADi + IPOPT timing if the box happens to have the wheel -- probed, not assumed
        try:
            import casadi  # noqa: F401
            ipopt_on_box = True
        except Exception:
            ipopt_on_box = False
        out["cpu_baseline"] = {
            "value": ns / tc, "unit": "solves/s", "cores": nthr, "kind": "port", "ipopt_on_box": ipopt_on_box,
            "sample": f"first {ns} instances of the step-0 batch, oracle/bmpc_solve.c (same algorithm, FP64, -O3 -march=x86-64-v3, "
                      f"OpenMP over instances) on {nthr} host threads in {tc:.1f} s, threads not pinned, the box is shared: +-25 % between runs; "
                      + ("casadi imports on this box but the IPOPT leg is not wired up: parity with IPOPT stays unpinned" if ipopt_on_box else
                         "`import casadi` fails on this box, so the reference's CasADi+IPOPT cannot be timed: IPOPT parity unpinned"),
            "iters_mean": float(ro["iters"].mean()),
            "status_equal_frac": float((ro["status"] == st_np[:ns]).mean()),
            "iters_equal_frac_of_both_converged": float(same_it.sum() / max(1, both.sum())),
            "max_abs_dx_vs_gpu_by_block": block_diffs(N, ro["x"][both], x_gpu[both]),
            "max_abs_dx_vs_gpu_by_block_same_iters": block_diffs(N, ro["x"][same_it], x_gpu[same_it]),
            # the maxima above are heavy-tailed (single exact-Hessian iterations amplify rounding noise by up to 1e5, DESIGN.md
            # section 5): per-instance max |dq| over the joint block, quantiles over the instances with equal iteration counts
            "dq_vs_gpu_same_iters_median_p90_p99": [float(v) for v in np.quantile(np.abs(ro["x"][same_it][:, :7 * N] - x_gpu[same_it][:, :7 * N]).max(axis=1), [0.5, 0.9, 0.99])] if same_it.any() else None,
        }
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
