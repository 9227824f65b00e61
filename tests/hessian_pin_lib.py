"""Second-order pin: stage matrices against the reference-derived probes of tests/golden/hess_N*.npz -- TEST INFRASTRUCTURE.

A fixture (tests/golden/gen/gen_hess.py) holds, per point, stage k and probe pair (s, r) of directions in the natural stage
coordinates y_k, the number b = D^2 L~ [s, r] of the SUBSTITUTED stage Lagrangian computed from the reference's own formulation,
an error estimate, and J_g Dw[s], J_g Dw[r] on the stage's inequality rows.  A stage matrix H (zeta coordinates, 41 x 41: the
oracle's s->H, the kernels' R_W) must satisfy

    (T^-1 s)^T H (T^-1 r)  =  b  +  sum_i (z_i / t_i) (a_i^T s) (a_i^T r)            for every probe,

the sum running over the inequality rows of g (from the fixture's first-order data) and over the bound rows of x (unit rows,
added here).  T is built here from dt alone (y = T zeta), independently of build_T in oracle/bmpc_solve.c and of the column
pass of ric_phase_load_impl.  Tolerance per probe: 10 x its stored error estimate + 1e-9 x its scale.
"""
import os

import numpy as np

NZ = 41
MAXROWS = 216
HORIZONS = (6, 10, 20, 30)
# zeta = (q~, dq~, ddq~, pi, rs~, ps~, d | u, drs, dps)
ZETA_NAMES = ([f"q{i}" for i in range(7)] + [f"dq{i}" for i in range(7)] + [f"ddq{i}" for i in range(7)] + ["pi0", "pi1", "pi2", "rs", "ps"]
              + [f"d{i}" for i in range(6)] + [f"u{i}" for i in range(7)] + ["drs", "dps"])


# the oracle's own order of the natural coordinates (oracle/bmpc_solve.c Y_*): names of the indices bmpc_oracle_stage_rows returns
ORACLE_Y_NAMES = ([f"q{i}" for i in range(7)] + [f"dq{i}" for i in range(7)] + [f"ddq{i}" for i in range(7)] + [f"u{i}" for i in range(7)]
                  + ["pi0", "pi1", "pi2", "rs", "drs", "ps", "dps"] + [f"d{i}" for i in range(6)])


def build_T(y_names, dt):
    """y = T zeta by name: q = q~ + dt^3/24 u, dq = dq~ + dt^2/6 u, ddq = ddq~ + dt/2 u, rs = rs~ + dt/2 drs, ps = ps~ + dt/2 dps,
    everything else unchanged (the hat-function jerk: x_k = x~_k + B1 u_k)."""
    y_names = [str(n) for n in y_names]
    T = np.zeros((NZ, NZ))
    zi = {n: i for i, n in enumerate(ZETA_NAMES)}
    for i, n in enumerate(y_names):
        T[i, zi[n]] = 1.0
        for pre, c in (("q", dt ** 3 / 24), ("dq", dt ** 2 / 6), ("ddq", dt / 2)):
            if n[:len(pre)] == pre and n[len(pre):].isdigit():
                T[i, zi["u" + n[len(pre):]]] = c
        if n in ("rs", "ps"):
            T[i, zi["d" + n]] = dt / 2
    assert sorted(y_names) == sorted(ZETA_NAMES) and np.linalg.matrix_rank(T) == NZ
    return T


def load(golden_dir, N):
    return dict(np.load(os.path.join(str(golden_dir), f"hess_N{N}.npz")))


def point_inputs(fx, ip, O, seed=0):
    """(w, lbx, ubx, p, t, z, lam_pi, rows) for point ip of a fixture: stage 0 pinned at w, finite boxes around every q, dq, ddq, u of
    the later stages (so that every bound row exists), the fixture's (t, z) on the rows of g, seeded random (t, z) on the bound
    rows, lam_pi from the fixture's multipliers of the p_rot dynamics rows (row 24..26 of block k is pi_k + dt w_k - pi_{k+1})."""
    N = int(fx["N"])
    w, p = fx["w"][ip], fx["p"][ip]
    rng = np.random.default_rng(1000 * N + 10 * ip + seed)
    lbx, ubx = np.full(w.size, -np.inf), np.full(w.size, np.inf)
    box = np.zeros(w.size, bool)
    box[:28 * N] = True
    lbx[box], ubx[box] = w[box] - rng.uniform(0.05, 1.0, box.sum()), w[box] + rng.uniform(0.05, 1.0, box.sum())
    st0 = np.arange(40) * N
    lbx[st0] = ubx[st0] = w[st0]
    nrows, meta, coef = O.stage_rows(N, w, lbx, ubx, p, float(fx["dt"]))
    t, z = np.ones((N - 1, MAXROWS)), np.zeros((N - 1, MAXROWS))
    for k in range(1, N):
        for i in range(nrows[k - 1]):
            gidx, gsign = meta[k - 1, i, 0], meta[k - 1, i, 1]
            if gidx >= 0:
                g = 112 * (k - 1) + gidx
                t[k - 1, i], z[k - 1, i] = (fx["t_up"][ip][g], fx["z_up"][ip][g]) if gsign > 0 else (fx["t_lo"][ip][g], fx["z_lo"][ip][g])
                assert z[k - 1, i] > 0 and t[k - 1, i] > 0, "a row of the oracle on a side the reference leaves open"
            else:
                t[k - 1, i], z[k - 1, i] = 0.3 * np.exp(rng.normal()), 0.5 * np.exp(rng.normal())
    lam_pi = np.zeros((N, 3))
    for j in range(1, N):
        lam_pi[j] = fx["lam_g"][ip][35 * (j - 1) + 24:35 * (j - 1) + 27]
    return w, lbx, ubx, p, t, z, lam_pi, (nrows, meta, coef)


def _bound_term(rows, t, z, k, s, r):
    """sum over the rows of stage k that are not rows of g (bounds of x; unit rows in y): (z / t) (a.s) (a.r)"""
    nrows, meta, coef = rows
    acc = 0.0
    for i in range(nrows[k - 1]):
        gidx, kind, i0, i1 = meta[k - 1, i, 0], meta[k - 1, i, 3], meta[k - 1, i, 4], meta[k - 1, i, 5]
        if gidx >= 0:
            continue
        assert kind == 2
        c0, c1 = coef[k - 1, i]
        a_s = c0 * s[i0] + (c1 * s[i1] if i1 >= 0 else 0.0)
        a_r = c0 * r[i0] + (c1 * r[i1] if i1 >= 0 else 0.0)
        acc += z[k - 1, i] / t[k - 1, i] * a_s * a_r
    return acc


def probe_ratios(fx, ip, H, t, z, rows):
    """|H-side value - expected| / tolerance for every probe of point ip: list of (block name, stage, ratio, got, expected).
    The d x d pairs come last, as block "dxd" with stage 0 (compared with the sum of all stages' d x d blocks)."""
    N = int(fx["N"])
    Ti = np.linalg.inv(build_T(fx["y_names"], float(fx["dt"])))
    sig = fx["z_up"][ip] / fx["t_up"][ip] + fx["z_lo"][ip] / fx["t_lo"][ip]
    # Rows of g that the project leaves out (all-zero padding rows of a set, `0 . p - b - slack <= 0` with b > 0 and slack >= 0:
    # never active) carry no (t, z) here.  They are linear in y: whatever direction in q a probe has, their Jacobian is zero.
    nrows, meta, _ = rows
    has = np.zeros(sig.size, bool)
    for k in range(1, N):
        gi = meta[k - 1, :nrows[k - 1], 0]
        has[112 * (k - 1) + gi[gi >= 0]] = True
    for m in np.nonzero(fx["pr_point"] == ip)[0]:
        if str(fx["block_names"][fx["pr_block"][m]]) == "qxq":
            k = int(fx["pr_stage"][m])
            gone = ~has[112 * (k - 1):112 * k]
            assert not fx["pr_as"][m][:112][gone].any() and not fx["pr_ar"][m][:112][gone].any(), "a row that depends on q was left out"
    sig = np.where(has, sig, 0.0)
    out = []
    for m in np.nonzero(fx["pr_point"] == ip)[0]:
        k = int(fx["pr_stage"][m])
        s, r = fx["pr_s"][m], fx["pr_r"][m]
        sg = np.zeros(133)
        sg[:112] = sig[112 * (k - 1):112 * k]
        if k == N - 1:
            sg[112:] = sig[112 * (N - 1):]
        want = fx["pr_b"][m] + np.sum(sg * fx["pr_as"][m] * fx["pr_ar"][m]) + _bound_term(rows, t, z, k, s, r)
        got = (Ti @ s) @ H[k - 1] @ (Ti @ r)
        tol = 10 * fx["pr_err"][m] + 1e-9 * fx["pr_scale"][m]
        out.append((str(fx["block_names"][fx["pr_block"][m]]), k, abs(got - want) / tol, got, want))
    for m in np.nonzero(fx["dd_point"] == ip)[0]:
        s, r = np.zeros(NZ), np.zeros(NZ)
        s[35:], r[35:] = fx["dd_s"][m], fx["dd_r"][m]
        want = fx["dd_b"][m] + np.sum(sig * fx["dd_as"][m] * fx["dd_ar"][m]) + sum(_bound_term(rows, t, z, k, s, r) for k in range(1, N))
        got = sum((Ti @ s) @ H[k - 1] @ (Ti @ r) for k in range(1, N))
        tol = 10 * fx["dd_err"][m] + 1e-9 * fx["dd_scale"][m]
        out.append(("dxd", 0, abs(got - want) / tol, got, want))
    return out


def worst_by_block(ratios):
    w = {}
    for blk, k, ratio, got, want in ratios:
        if ratio > w.get(blk, (-1.0,))[0]:
            w[blk] = (ratio, k, got, want)
    return w


# row slots of the kernels (boundplanner_amd/csrc/bmpc_device.hpp S_*), stated here by what the rows ARE
NSLOT = 208
S_NONNEG, S_RS1, S_D1, S_EE, S_ROTU, S_ROTL, S_COL, S_PHI, S_TSET, S_TROTU, S_TROTL = 56, 60, 62, 68, 83, 86, 89, 179, 180, 195, 198


def slot_of_row(N, k, m, y_names):
    """kernel slot of an oracle row with meta m = (gidx, gsign, xidx, kind, i0, i1)"""
    gidx, gsign, xidx, kind, i0, i1 = (int(v) for v in m)
    if gidx >= 0:
        for lo, hi, s0 in ((0, 15, S_EE), (15, 18, S_ROTU), (18, 21, S_ROTL), (21, 111, S_COL), (111, 112, S_PHI), (112, 127, S_TSET),
                           (127, 130, S_TROTU), (130, 133, S_TROTL)):
            if lo <= gidx < hi:
                return s0 + gidx - lo
    if 0 <= xidx < 28 * N:                   # box of q, dq, ddq, u: upper bound on the even slot, lower on the odd one
        blk, jj = xidx // (7 * N), (xidx % (7 * N)) // N
        assert xidx % N == k
        return 2 * (blk * 7 + jj)
    if 40 * N <= xidx < 40 * N + 6:
        return S_D1 + xidx - 40 * N
    if xidx >= 40 * N + 6:
        return S_NONNEG + (xidx - 40 * N - 6) // N
    name = str(y_names[i0])                  # stage 1: rs~_1, ps~_1 >= 0
    assert k == 1 and i1 >= 0 and name in ("rs", "ps")
    return S_RS1 + (name == "ps")


def slot_arrays(N, rows, t, z, y_names):
    """(t, z) [N-1][216] in the oracle's row order -> [N-1][208] in the kernels' slot numbering (unused slots: t = 1, z = 0)"""
    nrows, meta, coef = rows
    ts, zs = np.ones((N - 1, NSLOT)), np.zeros((N - 1, NSLOT))
    for k in range(1, N):
        seen = set()
        for i in range(nrows[k - 1]):
            s = slot_of_row(N, k, meta[k - 1, i], y_names)
            if 0 <= meta[k - 1, i, 2] < 28 * N and coef[k - 1, i, 0] < 0:
                s += 1
            assert s not in seen
            seen.add(s)
            ts[k - 1, s], zs[k - 1, s] = t[k - 1, i], z[k - 1, i]
    return ts, zs
