"""The backtracking line search of the SQP mode restated in plain NumPy from its contract (include/ihm2mpc.h: ihm2mpc_set_sqp_options,
ihm2mpc_set_path_constraints, ihm2mpc_set_soft; the header comment of csrc/kernels_sqp.hip) -- the reference of tests/test_oracle_merit.py
and tests/test_gpu_merit.py.  One instance at a time, long-double sums, its own loops; the only thing taken from elsewhere is the
state-only integrator Phi, a callable the caller supplies (the oracle's, pinned against SciPy Radau by tests of its own).

    m(alpha) = cost + sum w_pi |x0 - x_0| + sum w_pi |Phi(x_k, u_k) - x_{k+1}| + sum w_lam max(0, violation - slack)
    cost     = sum_k cs/2 e_k' W_k e_k + 1/2 e_N' W_e e_N + sum_{soft sides} z s + 1/2 Z s^2,   e_k = Vx x_k + Vu u_k - yref_k
at the point p + alpha (f - p) between the iterate p the QP was built at and the QP's full step f, the weights following the QP
multipliers (|mult|, later max(|mult|, (w + |mult|) / 2); entry 0 of w_pi: the multiplier of x_0 = x0, from the stage-0 stationarity row).

Every value comes with a rounding band  gamma S + R:  S the same sum with every product replaced by its absolute value, gamma = 2 n 2^-53
with n the number of addends (the bound between two float64 summations of different order), R = sum w tol_roll (1 + |Phi|) over the
dynamics defects -- tol_roll: what two implementations of Phi may differ by.  A comparison of two merit values adds their bands."""
import numpy as np

LD = np.longdouble
NX, NU, NY, NC = 8, 2, 12, 14
DROPS = ("slack_in_D", "slack_cost", "slack_in_violation", "x0_term", "pi0", "carry", "track_rows", "stages_ge_64")
U53 = 2.0 ** -53


class MeritProblem:
    """The data of one instance.  lb, ub (N+1,14): the bound of every row [x(8) u(2) g(2) h(2)] at every stage, -+inf = absent;
    soft_z, soft_Z (N+1,28) or None: lower sides then upper sides, Z < 0 = hard; track: None or (w_R, w_L, car_L, car_W);
    phi(x, u) -> Phi(x, u) over one shooting interval."""

    def __init__(self, W, W_e, Vx, Vu, cost_scale_stage, lb, ub, soft_z, soft_Z, C, D, track, phi):
        self.N = N = W.shape[0]
        self.W, self.W_e, self.cs = np.asarray(W, dtype=LD), np.asarray(W_e, dtype=LD), LD(cost_scale_stage)
        self.V = np.concatenate([np.asarray(Vx), np.asarray(Vu)], axis=1).astype(LD)          # (12,10)
        self.lb, self.ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        assert self.lb.shape == (N + 1, NC) and self.ub.shape == (N + 1, NC) and self.W.shape == (N, NY, NY)
        self.z = np.zeros((N + 1, 2 * NC)) if soft_Z is None else np.asarray(soft_z, dtype=np.float64)
        self.Z = np.full((N + 1, 2 * NC), -1.0) if soft_Z is None else np.asarray(soft_Z, dtype=np.float64)
        self.CD = np.concatenate([np.asarray(C), np.asarray(D)], axis=2).astype(LD)           # (N,2,10)
        self.track, self.phi = track, phi


def ladder(alpha_min, alpha_reduction):
    """The trial step lengths 1, rho, rho^2, ... >= alpha_min, by repeated float64 multiplication."""
    out, al = [], 1.0
    while True:
        out.append(al)
        al *= alpha_reduction
        if al < alpha_min:
            return out


class _Sum:
    """A long-double sum, the sum of the absolute values of its products, and the number of addends."""

    def __init__(self):
        self.v, self.s, self.n = [], [], 0

    def add(self, val, mag, n=1):
        self.v.append(LD(val)); self.s.append(LD(mag)); self.n += int(n)

    def extend(self, other):
        self.v += other.v; self.s += other.s; self.n += other.n

    def total(self):
        return (float(np.sum(np.array(self.v, dtype=LD))) if self.v else 0.0, float(np.sum(np.array(self.s, dtype=LD))) if self.s else 0.0, self.n)


class LineSearchRef:
    def __init__(self, prob, x0, yref, yref_e, xp, up, slp, xf, uf, pif, lamf, slf, A0, w_prev=None, alpha_min=0.05, alpha_reduction=0.7,
                 eps=1e-4, use_sufficient_descent=False, tol_roll=0.0):
        self.p, self.N = prob, prob.N
        f8 = lambda a, sh: np.asarray(a, dtype=np.float64).reshape(sh)
        N = self.N
        self.x0, self.yref, self.yref_e = f8(x0, (NX,)), f8(yref, (N, NY)), f8(yref_e, (NX,))
        self.xp, self.up, self.slp = f8(xp, (N + 1, NX)), f8(up, (N, NU)), f8(slp, (N + 1, 2 * NC))
        self.xf, self.uf, self.slf = f8(xf, (N + 1, NX)), f8(uf, (N, NU)), f8(slf, (N + 1, 2 * NC))
        self.pif, self.lamf, self.A0 = f8(pif, (N + 1, NX)), f8(lamf, (N + 1, 2 * NC)), f8(A0, (NX, NX))
        self.w_prev = w_prev
        self.alpha_min, self.rho, self.eps, self.suff, self.tol_roll = float(alpha_min), float(alpha_reduction), float(eps), bool(use_sufficient_descent), float(tol_roll)
        self.rungs = ladder(self.alpha_min, self.rho)
        self._pieces = {}

    # ---- merit weights ----
    def stage0_multiplier(self):
        """pi_0 from the stage-0 stationarity row of the QP:  H_0 dz_0 + g_0 + A_0' pi_1 - pi_0 - C_0' (lam_l - lam_u) = 0  (state rows; H_0 the
        Gauss-Newton Hessian cs V' W V, g_0 = cs V' W e_0; of the rows of stage 0 only the general rows touch the state)."""
        p = self.p
        z0 = np.concatenate([self.xp[0], self.up[0]]).astype(LD)
        dz0 = np.concatenate([self.xf[0] - self.xp[0], self.uf[0] - self.up[0]]).astype(LD)
        e0 = p.V @ z0 - self.yref[0].astype(LD)
        G = p.cs * (p.V.T @ p.W[0])                   # (10,12)
        pi0 = (G @ e0)[:NX] + ((G @ p.V) @ dz0)[:NX] + self.A0.astype(LD).T @ self.pif[1].astype(LD)
        dl = (self.lamf[0, 10:12] - self.lamf[0, NC + 10:NC + 12]).astype(LD)
        return np.asarray(pi0 - p.CD[0, :, :NX].T @ dl, dtype=np.float64)

    def weights(self, drop=None):
        assert drop is None or drop in DROPS, drop
        m_pi = np.abs(self.pif)
        if drop != "pi0":
            m_pi[0] = np.abs(self.stage0_multiplier())
        m_lam = np.abs(self.lamf)
        if self.w_prev is None or drop == "carry":
            return m_pi, m_lam
        return np.maximum(m_pi, 0.5 * (self.w_prev[0] + m_pi)), np.maximum(m_lam, 0.5 * (self.w_prev[1] + m_lam))

    # ---- everything of a trial point that does not depend on the weights ----
    def pieces(self, alpha):
        if alpha in self._pieces:
            return self._pieces[alpha]
        p, N = self.p, self.N
        x = self.xp + alpha * (self.xf - self.xp)         # float64, as every implementation forms the trial point
        u = self.up + alpha * (self.uf - self.up)
        sl = self.slp + alpha * (self.slf - self.slp)
        xl, ul = x.astype(LD), u.astype(LD)
        cost = [(_Sum()) for _ in range(N + 1)]
        for k in range(N):
            e = p.V @ np.concatenate([xl[k], ul[k]]) - self.yref[k].astype(LD)
            cost[k].add(0.5 * p.cs * (e @ p.W[k] @ e), 0.5 * p.cs * (np.abs(e) @ np.abs(p.W[k]) @ np.abs(e)), NY * NY)
        e = xl[N] - self.yref_e.astype(LD)
        cost[N].add(0.5 * (e @ p.W_e @ e), 0.5 * (np.abs(e) @ np.abs(p.W_e) @ np.abs(e)), NX * NX)
        phi = np.array([p.phi(x[k], u[k]) for k in range(N)])
        # constraint values and the magnitudes of what they are summed from
        cv, cm = np.zeros((N + 1, NC), dtype=LD), np.zeros((N + 1, NC), dtype=LD)
        cv[:, :NX] = xl; cm[:, :NX] = np.abs(xl)
        cv[:N, 8:10] = ul; cm[:N, 8:10] = np.abs(ul)
        for k in range(N):
            zk = np.concatenate([xl[k], ul[k]])
            cv[k, 10:12] = p.CD[k] @ zk; cm[k, 10:12] = np.abs(p.CD[k]) @ np.abs(zk)
        if p.track is not None:
            w_R, w_L, L, Wc = (LD(v) for v in p.track)
            for k in range(1, N + 1):
                n, psi = xl[k, 1], xl[k, 2]
                foot, lat = 0.5 * L * np.sin(np.abs(psi)), 0.5 * Wc * np.cos(psi)
                cv[k, 12] = n - foot + lat - w_R; cv[k, 13] = -n + foot + lat - w_L
                cm[k, 12] = np.abs(n) + np.abs(foot) + np.abs(lat) + np.abs(w_R); cm[k, 13] = np.abs(n) + np.abs(foot) + np.abs(lat) + np.abs(w_L)
        out = dict(x=x, u=u, sl=sl, cost=cost, phi=phi, cv=cv, cm=cm)
        self._pieces[alpha] = out
        return out

    def merit(self, alpha, drop=None):
        """m(alpha) = (value, band), and its infeasibility part (value, band)."""
        p, N = self.p, self.N
        q = self.pieces(alpha)
        wpi, wlam = self.weights(drop)
        kmax = 64 if drop == "stages_ge_64" else N + 1          # stages >= kmax are left out
        cost, inf, R = _Sum(), _Sum(), LD(0)
        x, sl = q["x"].astype(LD), q["sl"].astype(LD)
        if drop != "x0_term":
            for i in range(NX):
                inf.add(wpi[0, i] * np.abs(LD(self.x0[i]) - x[0, i]), wpi[0, i] * (abs(self.x0[i]) + np.abs(x[0, i])))
        for k in range(min(N + 1, kmax)):
            cost.extend(q["cost"][k])
            if k < N:
                for i in range(NX):
                    ph = LD(q["phi"][k, i])
                    inf.add(wpi[k + 1, i] * np.abs(ph - x[k + 1, i]), wpi[k + 1, i] * (np.abs(ph) + np.abs(x[k + 1, i])))
                    R += LD(wpi[k + 1, i]) * self.tol_roll * (1 + np.abs(ph))
            for c in range(NC):
                if drop == "track_rows" and c >= 12:
                    continue
                for up_side in (0, 1):
                    bound = (p.ub if up_side else p.lb)[k, c]
                    if not np.isfinite(bound):
                        continue
                    e1 = up_side * NC + c
                    viol = (q["cv"][k, c] - LD(bound)) if up_side else (LD(bound) - q["cv"][k, c])
                    mag = np.abs(LD(bound)) + q["cm"][k, c]
                    if p.Z[k, e1] >= 0.0:
                        s = sl[k, e1]
                        if drop != "slack_cost":
                            cost.add(LD(p.z[k, e1]) * s, np.abs(LD(p.z[k, e1]) * s))
                            cost.add(0.5 * LD(p.Z[k, e1]) * s * s, 0.5 * LD(p.Z[k, e1]) * s * s)
                        if drop != "slack_in_violation":
                            viol = viol - s; mag = mag + np.abs(s)
                    inf.add(LD(wlam[k, e1]) * max(LD(0), viol), LD(wlam[k, e1]) * mag)
        cv, cs_, cn = cost.total()
        iv, is_, in_ = inf.total()
        R = float(R)
        n = cn + in_
        return (cv + iv, 2 * n * U53 * (cs_ + is_) + R), (iv, 2 * in_ * U53 * is_ + R)

    def slope(self, drop=None):
        """D = min(0, grad cost . (f - p) - infeasibility part of m(0)): (value, band); (0, 0) on plain decrease."""
        if not self.suff:
            return 0.0, 0.0
        p, N = self.p, self.N
        kmax = 64 if drop == "stages_ge_64" else N + 1
        acc = _Sum()
        for k in range(min(N + 1, kmax)):
            if k < N:
                zk = np.concatenate([self.xp[k], self.up[k]]).astype(LD)
                d = np.concatenate([self.xf[k] - self.xp[k], self.uf[k] - self.up[k]]).astype(LD)
                e = p.V @ zk - self.yref[k].astype(LD)
                g = p.cs * (p.V.T @ (p.W[k] @ e))
                ga = p.cs * (np.abs(p.V).T @ (np.abs(p.W[k]) @ np.abs(e)))
                acc.add(g @ d, ga @ np.abs(d), NY * NY + NY * 10 + 10)
            else:
                d = (self.xf[N] - self.xp[N]).astype(LD)
                e = self.xp[N].astype(LD) - self.yref_e.astype(LD)
                acc.add((p.W_e @ e) @ d, (np.abs(p.W_e) @ np.abs(e)) @ np.abs(d), NX * NX + NX)
            if drop != "slack_in_D":
                for e1 in range(2 * NC):
                    bound = (p.ub if e1 >= NC else p.lb)[k, e1 % NC]
                    if p.Z[k, e1] >= 0.0 and np.isfinite(bound):
                        sp, ds = LD(self.slp[k, e1]), LD(self.slf[k, e1]) - LD(self.slp[k, e1])
                        acc.add((LD(p.z[k, e1]) + LD(p.Z[k, e1]) * sp) * ds, (np.abs(LD(p.z[k, e1])) + np.abs(LD(p.Z[k, e1]) * sp)) * np.abs(ds), 2)
        gv, gs, gn = acc.total()
        (_, _), (i0, i0_band) = self.merit(0.0, drop)
        D = gv - i0
        return min(D, 0.0), 2 * gn * U53 * gs + i0_band

    def walk(self, drop=None):
        """The ladder: the set of admissible step lengths (more than one member: a tie inside the rounding band), with the merit values
        (value, band) at 0 and at every rung tried.  `last[alpha]` = the rung whose merit an implementation that ends at alpha reports."""
        m0, inf0 = self.merit(0.0, drop)
        D = self.slope(drop)
        adm, tried, last = [], {}, {}
        floor = True
        for al in self.rungs:
            m1, _ = self.merit(al, drop)
            tried[al] = m1
            gap = m0[0] - m1[0] + (self.eps * al * D[0] if self.suff else 0.0)        # > 0: accepted
            band = m0[1] + m1[1] + (self.eps * al * D[1] if self.suff else 0.0)
            if gap > band:
                adm.append(al); last[al] = al; floor = False
                break
            if gap >= -band:
                adm.append(al); last[al] = al
        if floor:
            if self.alpha_min not in last:
                adm.append(self.alpha_min)
                last[self.alpha_min] = self.rungs[-1]
        return dict(admissible=adm, tied=len(adm) > 1, m0=m0, inf0=inf0, D=D, m=tried, last=last, weights=self.weights(drop))


def interpolation_bound(alpha, p, f, result):
    """|result - (p + alpha (f - p))| may be 2^-52 (|alpha (f - p)| + |result|): one fused against one unfused rounding."""
    return 2.0 ** -52 * (np.abs(alpha * (f - p)) + np.abs(result))
