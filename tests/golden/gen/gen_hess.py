"""Second-order fixtures tests/golden/hess_N*.npz: bilinear probes of the Hessian of the SUBSTITUTED stage Lagrangian, from the
REFERENCE's own formulation.  Build container only (needs the reference tree):

    python tests/golden/gen/gen_hess.py [6] [10] [20] [30] [--procs P] [--out DIR]

What is pinned.  With the natural stage coordinates y_k = (q, dq, ddq, u, pi, rs, drs, ps, dps, d) (names stored in the file as
`y_names`; d = the six global dslacks, part of every stage's y_k) and w(y) filling in p_pos = fk(q), v = J(q) dq,
p_rot = pi + dt/2 J_ang(q) dq from the reference's kinematic tapes (ca_tape.py),

    L~(y) = f(w(y)) + lam_g^T g(w(y))      (lam_g = 0 on the substituted rows p_new - p[:3], v_new - v)

where f and g are the reference's setup_optimization_problem run numerically at complex arguments (ref_eval.py).  Per stage k and
probe pair (s, r) of directions in y_k:  b = D^2 L~ [s, r]  =  central difference along s (real steps H1, H1/2, Richardson
extrapolated) of the complex-step derivative along r (1e-30).  `pr_err` = |Richardson value - value at the smaller step|.
Probes: random pairs over all of y_k ("all": s on the stage's own 35 variables, r on own + d, so that only stage k is involved;
"own": both without d), and pairs confined to q x q, q x dq, q x pi, dq x dq,
q x slacks, pi x pi, so that a failure names a block; "dd_*": pairs on d alone = the sum of all stages' d x d blocks.
Beside every probe the first-order data of the barrier term: `pr_as`, `pr_ar` = J_g Dw[s], J_g Dw[r] on the stage's 112 inequality
rows (+ the 21 terminal rows at the last stage), one complex step each; z, t per finite side of every inequality row
(`z_up, t_up, z_lo, t_lo`; lam_g = z_up - z_lo on those rows), random multipliers on the dynamics rows.

Points.  "split<i>": gen_golden.random_point with each of the five split patterns.  "cold", "iter8", "conv": inputs produced by
THIS project (boundplanner_amd.scenes.make_batch; the start vector, the iterate after 8 iterations and the final iterate of the
project's CPU oracle) -- the VALUES stored for them are the reference's, like everywhere else in the file.

Self-checks (the generator fails otherwise): substituted equality rows vanish along w(y) (<= 1e-13); a pair and its transpose
agree within the two error estimates + 1e-9 x scale + the rounding of the two difference quotients (64 eps |grad L~ . r| / h);
adding components of another stage to r does not change the value (same bound); every
error estimate is <= 1e-7 x the probe's scale (|s| |r| x the largest |b| / (|s| |r|) of that stage).  No probe is dropped.

Only arrays and name lists are written.  Time here: see TIMES below (8 processes).
"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.abspath(os.path.join(HERE, ".."))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, HERE)

# wall time of `python gen_hess.py <N>` with 8 processes in the build container, seconds
TIMES = {6: 74, 10: 99, 20: 98, 30: 111}

H1 = 5e-5          # larger real step; the smaller one is H1 / 2
HC = 1e-30
NY = 41
Y_NAMES = ([f"q{i}" for i in range(7)] + [f"dq{i}" for i in range(7)] + [f"ddq{i}" for i in range(7)] + [f"u{i}" for i in range(7)]
           + ["pi0", "pi1", "pi2", "rs", "drs", "ps", "dps"] + [f"d{i}" for i in range(6)])
IQ, IDQ, IPI, ISL, ID = slice(0, 7), slice(7, 14), slice(28, 31), slice(31, 35), slice(35, 41)
BLOCKS = ["all", "own", "qxq", "qxdq", "qxpi", "dqxdq", "qxslacks", "pixpi"]
# per horizon: (random-point variants, solver points (kind, seed, instance), probes per stage and block round, d x d pairs)
PLAN = {6: dict(splits=5, solver=True, per_stage=8, dd=3, seed=606),
        10: dict(splits=5, solver=True, per_stage=4, dd=2, seed=610),
        20: dict(splits=2, solver=True, per_stage=2, dd=1, seed=620),
        30: dict(splits=1, solver=True, per_stage=2, dd=1, seed=630)}
SOLVER_KINDS = {6: ("cold", "iter8", "conv"), 10: ("cold", "iter8", "conv"), 20: ("iter8", "conv"), 30: ("iter8",)}

_RE = _TAPES = None


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: a second run reproduces the file bit for bit"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(zi, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def _init():
    global _RE, _TAPES
    if _RE is None:
        import ref_eval as RE           # changes the working directory
        from ca_tape import load_all
        _RE, _TAPES = RE, load_all()
    return _RE, _TAPES


def w_to_y(N, w, dt):
    """natural coordinates [N][41] of a full-space point (stage 0 included; its row is never perturbed)"""
    _, T = _init()
    w = np.asarray(w)
    Y = np.zeros((N, NY), dtype=w.dtype)
    g = lambda blk, n: w[blk * N * 7:blk * N * 7 + n * N].reshape(n, N).T
    Y[:, 0:7], Y[:, 7:14], Y[:, 14:21], Y[:, 21:28] = g(0, 7), g(1, 7), g(2, 7), g(3, 7)
    prot = w[28 * N + 3 * N:28 * N + 6 * N].reshape(3, N).T
    for k in range(N):
        om = (T["jacobian"](Y[k, 0:7]) @ Y[k, 7:14])[3:]
        Y[k, 28:31] = prot[k] - dt / 2 * om
    o = 40 * N + 6
    for m in range(4):
        Y[:, 31 + m] = w[o + m * N:o + (m + 1) * N]
    Y[:, 35:41] = w[40 * N:40 * N + 6]
    return Y


def y_to_w(N, Y, w0, dt):
    """w(y): stage 0 from w0, stages >= 1 from Y with p_pos, v, p_rot through the reference's tapes; d from Y[1]"""
    _, T = _init()
    w = np.array(w0, dtype=Y.dtype)
    for k in range(1, N):
        q, dq = Y[k, 0:7], Y[k, 7:14]
        v = T["jacobian"](q) @ dq
        pos = T["fk_pos"](q).ravel()
        for j in range(7):
            for blk in range(4):
                w[blk * 7 * N + j * N + k] = Y[k, blk * 7 + j]
        for c in range(3):
            w[28 * N + c * N + k] = pos[c]
            w[28 * N + (3 + c) * N + k] = Y[k, 28 + c] + dt / 2 * v[3 + c]
        for c in range(6):
            w[34 * N + c * N + k] = v[c]
        o = 40 * N + 6
        for m in range(4):
            w[o + m * N + k] = Y[k, 31 + m]
    w[40 * N:40 * N + 6] = Y[1, 35:41]
    return w


def sub_rows(N):
    """indices of the substituted equality rows of g (p_new[:3] - p[:3], v_new - v) in every dynamics block"""
    return np.array([35 * k + o for k in range(N - 1) for o in (21, 22, 23, 27, 28, 29, 30, 31, 32)])


def spread(N, k, d41):
    """direction [N][41] with d41 on stage k; its d part on every stage (d is global)"""
    D = np.zeros((N, NY))
    D[k, :35] = d41[:35]
    D[:, 35:] = d41[35:]
    return D


def lag_im(N, w0, p, dt, lam, Y0, S, hs, R):
    """Im L~(Y0 + hs S + i HC R) / HC and Im g / HC"""
    RE, _ = _init()
    Y = Y0.astype(complex) + hs * S + 1j * HC * R
    f, g, _, _ = RE.eval_fg(N, y_to_w(N, Y, np.asarray(w0, dtype=complex), dt), p, dt)
    return (f.imag + lam @ g.imag) / HC, g.imag / HC


def job(a):
    """one task of the pool"""
    kind, N, w0, p, dt, lam, Y0, S, R = a
    if kind == "b":                         # probe value: (b at H1, b at H1/2)
        out = []
        for h in (H1, H1 / 2):
            lp, _ = lag_im(N, w0, p, dt, lam, Y0, S, h, R)
            lm, _ = lag_im(N, w0, p, dt, lam, Y0, S, -h, R)
            out.append(((lp - lm) / (2 * h), max(abs(lp), abs(lm))))
        return out
    if kind == "a":                         # J_g Dw[R] on all rows
        return lag_im(N, w0, p, dt, lam, Y0, 0 * R, 0.0, R)[1]
    raise ValueError(kind)


def draw_pair(rng, blk):
    s, r = np.zeros(NY), np.zeros(NY)
    n = lambda m: rng.normal(size=m)
    if blk == "all":                        # s on the stage's own variables, r on own + d: involves stage k only
        s[:35], r[:] = n(35), n(NY)
    elif blk == "own":
        s[:35], r[:35] = n(35), n(35)
    elif blk == "qxq":
        s[IQ], r[IQ] = n(7), n(7)
    elif blk == "qxdq":
        s[IQ], r[IDQ] = n(7), n(7)
    elif blk == "qxpi":
        s[IQ], r[IPI] = n(7), n(3)
    elif blk == "dqxdq":
        s[IDQ], r[IDQ] = n(7), n(7)
    elif blk == "qxslacks":
        s[IQ] = n(7); r[ISL] = n(4); r[ID] = n(6)
    elif blk == "pixpi":
        s[IPI], r[IPI] = n(3), n(3)
    return s, r


def solver_points(N, kinds, seed):
    """inputs of this project: cold start / iterate 8 / final iterate of the CPU oracle on scenes.make_batch"""
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    from boundplanner_amd import scenes
    b = scenes.make_batch(2, N, seed, O.fk_batch, randomize_sets=True)
    a = lambda i: (b["x0"][i], b["lbx"][i], b["ubx"][i], b["p"][i])
    out = []
    for kind in kinds:
        i = 0 if kind != "iter8" else 1
        if kind == "cold":
            x = b["x0"][i].copy()
            x[np.arange(40) * N] = b["lbx"][i][np.arange(40) * N]           # the pinned stage 0
        else:
            x = O.solve(N, *a(i), max_iter=8 if kind == "iter8" else 100)["x"]
        out.append((kind, x, b["p"][i].copy()))
    return out


def gen(N, procs, out_dir=OUT):
    t0 = time.time()
    plan = PLAN[N]
    dt = 0.1
    pts = solver_points(N, SOLVER_KINDS[N], plan["seed"]) if plan["solver"] else []
    RE, _ = _init()
    import gen_golden as GG
    rng = np.random.default_rng(plan["seed"])
    for i in range(plan["splits"]):
        w, p = GG.random_point(N, rng, i)
        pts.append((f"split{i}", w, p))
    n_g, n_dyn = RE.n_g(N), 35 * (N - 1)
    sub = sub_rows(N)
    P = dict(kind=[], w=[], p=[], lam=[], zu=[], tu=[], zl=[], tl=[], Y=[])
    tasks, meta = [], []                        # meta: what each task is
    probes = []                                 # dict per probe
    dds = []
    for ip, (kind, w_in, p) in enumerate(pts):
        Y0 = w_to_y(N, np.asarray(w_in, float), dt)
        Y0[:, 35:] = Y0[0, 35:]
        w = y_to_w(N, Y0, np.asarray(w_in, float), dt)
        f, g, lbg, ubg = RE.eval_fg(N, w, p, dt)
        worst = np.abs(g[sub]).max()
        assert worst <= 1e-13, ("substituted rows do not vanish", kind, worst)
        assert np.all(lbg[:n_dyn] == 0) and np.all(ubg[:n_dyn] == 0)
        up, lo = np.isfinite(ubg[n_dyn:]) & (ubg[n_dyn:] < 1e19), np.isfinite(lbg[n_dyn:]) & (lbg[n_dyn:] > -1e19)
        m = n_g - n_dyn
        zu, tu = np.where(up, 0.5 * np.exp(rng.normal(size=m)), 0.0), np.where(up, 0.3 * np.exp(rng.normal(size=m)), 1.0)
        zl, tl = np.where(lo, 0.5 * np.exp(rng.normal(size=m)), 0.0), np.where(lo, 0.3 * np.exp(rng.normal(size=m)), 1.0)
        lam = np.zeros(n_g)
        lam[:n_dyn] = rng.normal(size=n_dyn)
        lam[sub] = 0.0
        lam[n_dyn:] = zu - zl
        for key, val in zip(("kind", "w", "p", "lam", "zu", "tu", "zl", "tl", "Y"), (kind, w, p, lam, zu, tu, zl, tl, Y0)):
            P[key].append(val)
        base = (N, w, p, dt, lam, Y0)
        for rnd in range(plan["per_stage"]):
            S_all, R_all = np.zeros((N, NY)), np.zeros((N, NY))
            for k in range(1, N):
                # every block on every stage when per_stage >= 8; otherwise the confined blocks rotate over stages and points
                # (the first probe of every stage is an "all" pair: it sets the stage's scale)
                ps = plan["per_stage"]
                blk = BLOCKS[rnd % len(BLOCKS)] if ps >= 8 or rnd == 0 else BLOCKS[1 + (rnd - 1 + (ps - 1) * (k + ip)) % (len(BLOCKS) - 1)]
                s, r = draw_pair(rng, blk)
                pr = dict(point=ip, stage=k, block=BLOCKS.index(blk), s=s, r=r, rnd=rnd)
                probes.append(pr)
                # D^2 L~ is symmetric: the complex step goes along the direction WITHOUT d components.  Along d the directional
                # derivative collects the gradients of every stage (its rounding error, divided by the real step, grew with N and
                # reached the test's tolerance at N = 20 and 30); along a stage's own variables it sees that stage alone.
                sw = bool(r[35:].any()) and not s[35:].any()
                S_, R_ = (spread(N, k, r), spread(N, k, s)) if sw else (spread(N, k, s), spread(N, k, r))
                tasks.append(("b",) + base + (S_, R_)); meta.append(("b", pr))
                chk = rng.random()
                if chk < 0.12:                  # transpose (the other assignment of the two steps)
                    tasks.append(("b",) + base + (R_, S_)); meta.append(("bt", pr))
                elif chk < 0.24 and not r[35:].any():   # block structure: components of another stage added to r
                    k2 = 1 + (k % (N - 1))
                    R2 = spread(N, k, r)
                    if k2 != k:
                        R2[k2, :35] = rng.normal(size=35)
                        tasks.append(("b",) + base + (spread(N, k, s), R2)); meta.append(("bx", pr))
                # first-order rows: own components of all stages in one evaluation, the d components in another
                S_all[k, :35], R_all[k, :35] = s[:35], r[:35]
                for nm, vec in (("as_d", s), ("ar_d", r)):
                    if vec[35:].any():
                        D = np.zeros((N, NY)); D[:, 35:] = vec[35:]
                        tasks.append(("a",) + base + (None, D)); meta.append((nm, pr))
            tasks.append(("a",) + base + (None, S_all)); meta.append(("as_all", (ip, rnd)))
            tasks.append(("a",) + base + (None, R_all)); meta.append(("ar_all", (ip, rnd)))
        for _ in range(plan["dd"]):
            s, r = np.zeros(NY), np.zeros(NY)
            s[ID], r[ID] = rng.normal(size=6), rng.normal(size=6)
            dd = dict(point=ip, s=s[ID].copy(), r=r[ID].copy())
            dds.append(dd)
            S, R = np.zeros((N, NY)), np.zeros((N, NY))
            S[:, 35:], R[:, 35:] = s[ID], r[ID]
            tasks.append(("b",) + base + (S, R)); meta.append(("ddb", dd))
            tasks.append(("a",) + base + (None, S)); meta.append(("dds", dd))
            tasks.append(("a",) + base + (None, R)); meta.append(("ddr", dd))
    print(f"N={N}: {len(pts)} points, {len(probes)} probes, {len(dds)} d x d pairs, {len(tasks)} tasks", flush=True)
    with Pool(procs) as pool:
        res = pool.map(job, tasks, chunksize=1)
    # (Richardson value, |Richardson value - value at H1/2|, rounding allowance of the difference quotient at H1/2: both terms
    #  of the difference are directional derivatives g = grad L~ . r with a relative rounding error of some 64 eps after the
    #  reference's long expressions; used by the self-checks only)
    rich = lambda v: ((4 * v[1][0] - v[0][0]) / 3, abs((4 * v[1][0] - v[0][0]) / 3 - v[1][0]), 64 * 2.2e-16 * v[1][1] / (H1 / 2))
    rows_all = {}
    n_in = n_g - n_dyn

    def stage_rows(k, gi):          # 112 rows of stage k (+ 21 terminal rows at the last stage), padded to 133
        out = np.zeros(133)
        out[:112] = gi[n_dyn + 112 * (k - 1):n_dyn + 112 * k]
        if k == N - 1:
            out[112:] = gi[n_g - 21:]
        return out

    for (what, ref), val in zip(meta, res):
        if what == "b":
            ref["b"], ref["err"], ref["rnd_noise"] = rich(val)
        elif what in ("bt", "bx"):
            ref[what] = rich(val)
        elif what in ("as_all", "ar_all"):
            rows_all[(what,) + ref] = val
        elif what in ("as_d", "ar_d"):
            ref[what] = val
        elif what == "ddb":
            ref["b"], ref["err"], ref["rnd_noise"] = rich(val)
        elif what in ("dds", "ddr"):
            ref[what] = val[n_dyn:]
    for pr in probes:
        k = pr["stage"]
        for nm in ("as", "ar"):
            a = stage_rows(k, rows_all[(nm + "_all", pr["point"], pr["rnd"])])
            if nm + "_d" in pr:
                a = a + stage_rows(k, pr[nm + "_d"])
            pr[nm] = a
    # scales and self-checks
    nrm = lambda pr: np.linalg.norm(pr["s"]) * np.linalg.norm(pr["r"])
    for ip in range(len(pts)):
        for k in range(1, N):
            mine = [pr for pr in probes if pr["point"] == ip and pr["stage"] == k]
            top = max(abs(pr["b"]) / nrm(pr) for pr in mine)
            for pr in mine:
                pr["scale"] = nrm(pr) * top
        for dd in [d for d in dds if d["point"] == ip]:
            dd["scale"] = max(abs(dd["b"]), np.linalg.norm(dd["s"]) * np.linalg.norm(dd["r"]) * max(pr["scale"] / nrm(pr) for pr in probes if pr["point"] == ip))
    worst = dict(err=0.0, bt=0.0, bx=0.0)
    for pr in probes + dds:
        worst["err"] = max(worst["err"], pr["err"] / pr["scale"])
        assert pr["err"] <= 1e-7 * pr["scale"], ("error estimate too large", pts[pr["point"]][0], pr.get("stage"), pr["err"], pr["scale"])
        for nm in ("bt", "bx"):
            if nm in pr:
                v, e, noise = pr[nm]
                d = abs(v - pr["b"])
                worst[nm] = max(worst[nm], d / pr["scale"])
                assert d <= pr["err"] + e + pr["rnd_noise"] + noise + 1e-9 * pr["scale"], (nm, pts[pr["point"]][0], pr["stage"], BLOCKS[pr["block"]], v, pr["b"], pr["err"], e)
    nt, nx = sum("bt" in pr for pr in probes), sum("bx" in pr for pr in probes)
    print(f"N={N}: worst err/scale {worst['err']:.2e}; {nt} transposes, worst {worst['bt']:.2e} x scale; {nx} block-structure checks, worst {worst['bx']:.2e} x scale")
    A = lambda key, src=probes: np.array([pr[key] for pr in src])
    path = os.path.join(out_dir, f"hess_N{N}.npz")
    save_npz(
        path, N=N, dt=dt, y_names=np.array(Y_NAMES), block_names=np.array(BLOCKS), point_kind=np.array(P["kind"]),
        w=np.array(P["w"]), p=np.array(P["p"]), y=np.array(P["Y"]), lam_g=np.array(P["lam"]),
        z_up=np.array(P["zu"]), t_up=np.array(P["tu"]), z_lo=np.array(P["zl"]), t_lo=np.array(P["tl"]),
        pr_point=A("point"), pr_stage=A("stage"), pr_block=A("block"), pr_s=A("s"), pr_r=A("r"), pr_b=A("b"), pr_err=A("err"),
        pr_scale=A("scale"), pr_as=A("as"), pr_ar=A("ar"),
        dd_point=A("point", dds), dd_s=A("s", dds), dd_r=A("r", dds), dd_b=A("b", dds), dd_err=A("err", dds), dd_scale=A("scale", dds),
        dd_as=A("dds", dds), dd_ar=A("ddr", dds))
    print(f"hess_N{N}.npz written: {os.path.getsize(path)} bytes, {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    procs = 8
    if "--procs" in args:
        i = args.index("--procs")
        procs = int(args[i + 1])
        del args[i:i + 2]
    out_dir = OUT
    if "--out" in args:
        i = args.index("--out")
        out_dir = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    for N in [int(a) for a in args] or [6, 10, 20, 30]:
        gen(N, procs, out_dir)
