"""Independent KKT certificate for the reference's NLP.  TEST INFRASTRUCTURE ONLY (numpy).

The NLP is written here a second time, straight from the reference's text and in its flat ordering
(z = [vec(U); vec(X)], g rows in the order they are appended), with NO hand-written derivative: gradients and the
constraint Jacobian come from complex-step differentiation of these functions.  A solver result (z, lam_g, lam_x)
is then judged by the first-order optimality conditions in IPOPT's sign convention
    grad f(z) + J_g(z)^T lam_g + lam_x = 0,   lbg <= g(z) <= ubg,   lbx <= z <= ubx,
    lam > 0 only at an upper bound, lam < 0 only at a lower bound.
This depends on neither the oracle's nor the kernel's algebra, so it certifies both.

References (CMOM = CasaDi_MPC_Optimize_Multishoot/):
  model           CMOM/MPC_CBF_optimize_kin.py:153-156
  objective       CMOM/MPC_CBF_optimize_kin.py:168-205
  rows            CMOM/MPC_CBF_optimize_kin.py:190-191,207-216,236-248 ; _kin_pre.py:236-253
  bounds          CMOM/MPC_CBF_optimize_kin.py:84-134
"""
import numpy as np

# values of the enums of include/mpcbatch.h that from_config() reads off a config, restated (this module parses no header and
# imports neither the oracle nor the package)
_MODEL_DYN, _OBS_DCBF, _INT_RK4 = 1, 1, 1


def _bounds(N, nx, n_obs, u_lo, u_hi, x_lo, x_hi, rate_lo, rate_hi, interleaved, obs_nodes, obs_lb):
    """lbx/ubx/lbg/ubg in the flat ordering: z = [vec(U); vec(X)]; g = [X_0 - x0; dynamics and rate rows; obstacle rows].  Rate rows
    (one per entry of rate_lo/rate_hi and stage 1..N-1, stage-major) form one block after all dynamics rows (kin.py:211-216) or follow
    the dynamics rows of their stage (interleaved, dyn.py:226-231)."""
    lbx = np.concatenate([np.tile(np.asarray(u_lo, float), N), np.tile(np.asarray(x_lo, float), N + 1)])
    ubx = np.concatenate([np.tile(np.asarray(u_hi, float), N), np.tile(np.asarray(x_hi, float), N + 1)])
    rate_lo, rate_hi = list(rate_lo), list(rate_hi)
    lbg, ubg = [0.0] * nx, [0.0] * nx
    if interleaved:
        for i in range(N):
            lbg += [0.0] * nx; ubg += [0.0] * nx
            if i > 0:
                lbg += rate_lo; ubg += rate_hi
    else:
        lbg += [0.0] * (nx * N); ubg += [0.0] * (nx * N)
        lbg += rate_lo * (N - 1); ubg += rate_hi * (N - 1)
    lbg += [obs_lb] * (obs_nodes * n_obs); ubg += [np.inf] * (obs_nodes * n_obs)
    return lbx, ubx, np.array(lbg, float), np.array(ubg, float)


def _semi_axes(cfg, obs):
    """Semi-axes of the keep-out ellipse per obstacle and node: fixed (dyn.py:240-241) or ego half-size + obstacle half-size + safety
    distance (kin.py:242-243)."""
    if cfg.obs_sx_fixed > 0:
        sx = np.full(obs.shape[:2], float(cfg.obs_sx_fixed))
    else:
        sx = cfg.ego_hl + obs[:, :, 4] / 2 + cfg.safe_disl
    if cfg.obs_sy_fixed > 0:
        sy = np.full(obs.shape[:2], float(cfg.obs_sy_fixed))
    else:
        sy = cfg.ego_hw + obs[:, :, 5] / 2 + cfg.safe_disw
    return sx, sy


def _obs_array(obs, N, n_obs):
    """obs as (n_obs, N+1, 6): static rows repeated over the nodes, missing columns (the dyn reference passes x, y only) zero."""
    if n_obs == 0 or obs is None or np.size(obs) == 0:
        return np.zeros((0, N + 1, 6))
    obs = np.asarray(obs, float)
    if obs.ndim == 1:
        obs = obs[None]
    if obs.ndim == 2:
        obs = np.repeat(obs[:, None, :], N + 1, axis=1)
    assert obs.shape[:2] == (n_obs, N + 1), "obs must be (n_obs, cols) or (n_obs, N+1, cols), got %s" % (obs.shape,)
    out = np.zeros((n_obs, N + 1, 6))
    out[:, :, :obs.shape[2]] = obs
    return out


def _shooting_and_rate_rows(rows, defect, U, rate_cols, interleaved):
    """Appends the dynamics rows X_{i+1} - F(X_i, U_i) (defect [N, nx]) and the rate rows U[c,i] - U[c,i-1], i = 1..N-1, of the controls
    in rate_cols, in the order _bounds() lays out."""
    N = len(defect)
    rate = [np.stack([U[i, c] - U[i - 1, c] for c in rate_cols]) for i in range(1, N)] if rate_cols else []
    if interleaved:
        for i in range(N):
            rows.append(defect[i])
            if i > 0 and rate_cols:
                rows.append(rate[i - 1])
    else:
        rows.append(defect.reshape(-1))
        rows.extend(rate)


class KinNlp:
    """The kinematic NLP for one instance.  obs: (n_obs,6) static or (n_obs,N+1,6) predicted; rows [x,y,th,v,l,w]."""

    def __init__(self, N, T, x0, xs, obs=None, Q=(1e1, 1e5, 3e5, 1e4), R=(1e4, 1e4), DR=(1e5, 1e2), veh_l=2.6,
                 veh_L=4.8, veh_W=1.8, safe_disl=1.0, safe_disw=0.5, df_lim=35 * np.pi / 180, a_lim=3.0, y_lim=(-1.0, 5.0),
                 v_lim=(0.0, 40.0), ddf_lim=5 * np.pi / 180, obs_mode="keepout", gamma=1.0, u_last=(0.0, 0.0), integrator="euler"):
        self.N, self.T = N, T
        self.integrator = integrator          # "euler": X+ = X + T f (kin.py:207); "rk4": classical Runge-Kutta step, control held (MPCB_INT_RK4)
        self.x0 = np.asarray(x0, float).reshape(4); self.xs = np.asarray(xs, float).reshape(4)
        self.Q, self.R, self.DR = np.asarray(Q, float), np.asarray(R, float), np.asarray(DR, float)
        self.veh_l = veh_l
        self.u_last = np.asarray(u_last, float)
        self.obs_mode, self.gamma = obs_mode, gamma
        if obs is None or np.size(obs) == 0:
            self.obs = np.zeros((0, N + 1, 6))
        else:
            obs = np.asarray(obs, float)
            if obs.ndim == 2:
                obs = np.repeat(obs[:, None, :], N + 1, axis=1)
            self.obs = obs
        self.n_obs = self.obs.shape[0]
        self.sx = veh_L / 2 + self.obs[:, :, 4] / 2 + safe_disl      # kin.py:242
        self.sy = veh_W / 2 + self.obs[:, :, 5] / 2 + safe_disw      # kin.py:243
        self.nz = 2 * N + 4 * (N + 1)
        # rows: the steering-rate block (kin.py:211-216), obstacle rows at nodes 0..N-1 (kin.py:236), the stage-0 rate cost (kin.py:203-204)
        self.rate_cols, self.rate_interleaved, self.obs_nodes, self.du0_cost = [0], False, N, True
        # bounds (kin.py:84-134)
        self.lbx, self.ubx, self.lbg, self.ubg = _bounds(N, 4, self.n_obs, [-df_lim, -a_lim], [df_lim, a_lim], [-np.inf, y_lim[0], -np.inf, v_lim[0]],
                                                         [np.inf, y_lim[1], np.inf, v_lim[1]], [-ddf_lim * T], [ddf_lim * T], False, N, 0.0)
        self.ng = len(self.lbg)

    @classmethod
    def from_config(cls, cfg, x0, xs, obs, x_ref=None):
        """The kinematic NLP that a config (struct mpcb_config) describes, from the config alone: N, T, weights, u_last and du0_cost,
        the boxes as they are (asymmetric, or absent where non-finite), a rate row per control whose du bound is finite, in block or
        interleaved order, semi-axes from ego_* + safe_* + the obstacle's l, w or from obs_s*_fixed, obs_hmin, obs_terminal, obs_mode,
        gamma, the integrator and the wheelbase.  x_ref (N, 4): per-stage references of the tracking cost, in place of xs."""
        assert cfg.model != _MODEL_DYN, "DynNlp.from_config states the dynamic model"
        self = cls.__new__(cls)
        N = self.N = int(cfg.N); self.T = float(cfg.T)
        self.integrator = "rk4" if cfg.integrator == _INT_RK4 else "euler"
        self.x0 = np.asarray(x0, float).reshape(4)
        self.xs = np.asarray(xs, float).reshape(4) if x_ref is None else np.asarray(x_ref, float).reshape(N, 4)
        self.Q, self.R, self.DR = np.array(cfg.Q[:4], float), np.array(cfg.R[:2], float), np.array(cfg.DR[:2], float)
        self.veh_l = float(cfg.veh_l)
        self.u_last = np.array(cfg.u_last[:2], float)
        self.du0_cost = bool(cfg.du0_cost)
        self.obs_mode, self.gamma = ("dcbf" if cfg.obs_mode == _OBS_DCBF else "keepout"), float(cfg.gamma)
        self.obs = _obs_array(obs, N, int(cfg.n_obs))
        self.n_obs = self.obs.shape[0]
        self.sx, self.sy = _semi_axes(cfg, self.obs)
        assert not (cfg.obs_terminal and self.obs_mode == "dcbf"), "a CBF row at node N would need X_{N+1}"
        self.obs_nodes = N + 1 if cfg.obs_terminal else N
        self.rate_cols = [c for c in range(2) if np.isfinite(cfg.du_lo[c]) or np.isfinite(cfg.du_hi[c])]
        self.rate_interleaved = bool(cfg.rate_interleaved)
        self.nz = 2 * N + 4 * (N + 1)
        obs_lb = float(cfg.obs_hmin) * (self.gamma if self.obs_mode == "dcbf" else 1.0)       # gamma (h_i - hmin) + (h_next - h_i) >= 0
        self.lbx, self.ubx, self.lbg, self.ubg = _bounds(N, 4, self.n_obs, cfg.u_lo[:2], cfg.u_hi[:2], cfg.x_lo[:4], cfg.x_hi[:4],
                                                         [cfg.du_lo[c] for c in self.rate_cols], [cfg.du_hi[c] for c in self.rate_cols],
                                                         self.rate_interleaved, self.obs_nodes, obs_lb)
        self.ng = len(self.lbg)
        return self

    def split(self, z):
        N = self.N
        U = z[:2 * N].reshape(N, 2)          # U[i] = [df_i, ax_i]
        X = z[2 * N:].reshape(N + 1, 4)      # X[k] = [x, y, phi, vx]
        return U, X

    def rhs(self, X, U):
        return np.stack([X[:, 3] * np.cos(X[:, 2]), X[:, 3] * np.sin(X[:, 2]), X[:, 3] * np.tan(U[:, 0]) / self.veh_l, U[:, 1]], axis=1)

    def step(self, X, U):
        """One shooting step for every stage at once: X [N,4], U [N,2] -> X+ [N,4]."""
        T = self.T
        if self.integrator == "euler":
            return X + T * self.rhs(X, U)
        k1 = self.rhs(X, U); k2 = self.rhs(X + 0.5 * T * k1, U); k3 = self.rhs(X + 0.5 * T * k2, U); k4 = self.rhs(X + T * k3, U)
        return X + (T / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)

    def f(self, z):
        U, X = self.split(z)
        e = X[:-1] - self.xs
        Up = np.vstack([self.u_last.astype(z.dtype)[None, :], U[:-1]])
        dU = U - Up if self.du0_cost else (U - Up)[1:]                  # kin.py:203-204 has the stage-0 term, dyn.py:223-224 has none
        return (e * e * self.Q).sum() + (U * U * self.R).sum() + (dU ** 2 * self.DR).sum()

    def h(self, X, k, step):
        o = self.obs[:, step, :]
        return (X[k, 0] - o[:, 0]) ** 2 / self.sx[:, step] ** 2 + (X[k, 1] - o[:, 1]) ** 2 / self.sy[:, step] ** 2 - 1.0

    def g(self, z):
        U, X = self.split(z)
        N = self.N
        rows = [X[0] - self.x0]
        _shooting_and_rate_rows(rows, X[1:] - self.step(X[:-1], U), U, self.rate_cols, self.rate_interleaved)
        for i in range(self.obs_nodes):
            if self.n_obs == 0:
                break
            hi = self.h(X, i, i)
            if self.obs_mode == "keepout":
                rows.append(hi)                                           # kin.py:247
            else:
                rows.append(self.gamma * hi + (self.h(X, i + 1, i) - hi))   # kin.py:245-248
        return np.concatenate([np.asarray(r).reshape(-1) for r in rows])

    # complex-step derivatives ------------------------------------------------------------------------------------
    def grad_f(self, z, h=1e-30):
        g = np.empty(self.nz)
        zc = z.astype(complex)
        for i in range(self.nz):
            zc[i] += 1j * h
            g[i] = self.f(zc).imag / h
            zc[i] = z[i]
        return g

    def jac_g_dense(self, z, h=1e-30):
        """One complex step per variable: the plain definition (nz evaluations of g)."""
        J = np.empty((self.ng, self.nz))
        zc = z.astype(complex)
        for i in range(self.nz):
            zc[i] += 1j * h
            J[:, i] = self.g(zc).imag / h
            zc[i] = z[i]
        return J

    _patterns = {}

    def _pattern_key(self):
        return (type(self).__name__, self.N, self.n_obs, getattr(self, "obs_mode", ""), getattr(self, "integrator", "euler"),
                self.nz, self.ng, tuple(self.rate_cols), self.rate_interleaved, self.obs_nodes)

    def jac_g(self, z, h=1e-30):
        """The same Jacobian from a handful of evaluations: columns that share no row (variables three or more stages apart) are
        perturbed together (Curtis-Powell-Reid colouring of the structural pattern, which is found once per NLP structure from two
        dense Jacobians at random points and cached).  tests/test_config_cpu.py checks it against jac_g_dense."""
        key = self._pattern_key()
        if key not in KinNlp._patterns:
            rng = np.random.default_rng(0)
            P = np.zeros((self.ng, self.nz), bool)
            for _ in range(2):
                zr = z + rng.uniform(0.05, 0.5, self.nz) * rng.choice([-1.0, 1.0], self.nz)
                P |= self.jac_g_dense(zr) != 0.0
            groups = []                                  # greedy: a column joins the first group none of whose rows it touches
            rows_of = []
            for j in range(self.nz):
                rj = P[:, j]
                for gi, used in enumerate(rows_of):
                    if not (used & rj).any():
                        groups[gi].append(j); used |= rj
                        break
                else:
                    groups.append([j]); rows_of.append(rj.copy())
            KinNlp._patterns[key] = (P, [np.array(g_) for g_ in groups])
        P, groups = KinNlp._patterns[key]
        J = np.zeros((self.ng, self.nz))
        zc = z.astype(complex)
        for cols in groups:
            zc[cols] += 1j * h
            d = self.g(zc).imag / h
            zc[cols] = z[cols]
            for j in cols:
                r = P[:, j]
                J[r, j] = d[r]
        return J


def certificate(nlp, z, lam_g, lam_x, act_tol=1e-6):
    """Returns dict of unscaled KKT residuals."""
    z = np.asarray(z, float); lam_g = np.asarray(lam_g, float); lam_x = np.asarray(lam_x, float)
    gv = nlp.g(z)
    stat = nlp.grad_f(z) + nlp.jac_g(z).T @ lam_g + lam_x
    viol_g = np.maximum(0, np.maximum(nlp.lbg - gv, gv - nlp.ubg)).max()
    viol_x = np.maximum(0, np.maximum(nlp.lbx - z, z - nlp.ubx)).max()

    def compl(lam, v, lo, hi):
        eq = lo == hi
        dist_hi = np.where(np.isfinite(hi), hi - v, np.inf)
        dist_lo = np.where(np.isfinite(lo), v - lo, np.inf)
        with np.errstate(invalid="ignore"):
            c = np.where(lam > 0, lam * np.maximum(dist_hi, 0), -lam * np.maximum(dist_lo, 0))
        c = np.where(eq, 0.0, c)
        wrong_sign = np.where(~eq & (lam > 0) & ~np.isfinite(hi), lam, 0.0) + np.where(~eq & (lam < 0) & ~np.isfinite(lo), -lam, 0.0)
        return np.nan_to_num(c, posinf=0.0).max(), wrong_sign.max()

    cg, sg = compl(lam_g, gv, nlp.lbg, nlp.ubg)
    cx, sx = compl(lam_x, z, nlp.lbx, nlp.ubx)
    return dict(stationarity=np.abs(stat).max(), feas_g=viol_g, feas_x=viol_x, compl=max(cg, cx), sign=max(sg, sx),
                f=float(nlp.f(z)), lam_scale=max(1.0, np.abs(lam_g).max(), np.abs(lam_x).max()))


class DynNlp:
    """The dynamic-bicycle NLP (CMOM/MPC_CBF_optimize_dyn.py) for one instance, g rows and bounds ALIGNED (the
    reference's own lbg/ubg are interleaved one stage off its g).  obs: (n_obs, >=2) static centres.
    The obstacle row is kept in the reference's form sqrt(h) >= 1 so that this certificate also shows that the
    solver's h >= 1 formulation reaches a KKT point of the reference's row (multipliers scale by 2 sqrt(h))."""

    def __init__(self, N, T, x0, xs, obs, Q=(10, 1e5, 1e3, 1e3, 1, 1), R=(1e3, 1e3), DR=(5e3, 5e2), m=1575.0, lf=1.2, lr=1.6, Iz=2875.0,
                 aopt_f=0.3490658503988659, aopt_r=0.19198621771937624, Cf0=-50000.0, Cr0=-50000.0, sx=4.0, sy=1.0):
        self.N, self.T = N, T
        self.x0 = np.asarray(x0, float).reshape(6); self.xs = np.asarray(xs, float).reshape(6)
        self.Q, self.R, self.DR = np.asarray(Q, float), np.asarray(R, float), np.asarray(DR, float)
        self.m, self.lf, self.lr, self.Iz, self.af, self.ar = m, lf, lr, Iz, aopt_f, aopt_r
        self.Fyf, self.Fyr = Cf0 * aopt_f / 2, Cr0 * aopt_r / 2                       # dyn.py:55-56
        ob = np.asarray(obs, float).reshape(-1, np.shape(obs)[-1])[:, :2]
        self.obs = _obs_array(ob, N, len(ob))                                          # (n_obs, N+1, 6), x and y filled
        self.n_obs = len(ob)
        self.sx, self.sy = np.full((self.n_obs, N + 1), float(sx)), np.full((self.n_obs, N + 1), float(sy))
        self.nz = 2 * N + 6 * (N + 1)
        # rows: rate rows of both controls after each stage's dynamics rows (dyn.py:226-231), sqrt(h) >= 1 at nodes 0..N (dyn.py:242-243),
        # no stage-0 rate cost (dyn.py:223-224)
        self.rate_cols, self.rate_interleaved, self.obs_nodes, self.du0_cost = [0, 1], True, N + 1, False
        self.u_last = np.zeros(2)
        self.obs_mode, self.gamma, self.integrator = "keepout", 1.0, "euler"
        deg = np.pi / 180
        self.lbx, self.ubx, self.lbg, self.ubg = _bounds(N, 6, self.n_obs, [-35 * deg, -3.0], [35 * deg, 3.0], [-np.inf, -1.0, -np.inf, 0.0, -5.0, -np.inf],
                                                         [np.inf, 5.0, np.inf, 40.0, 5.0, np.inf], [-5 * deg * T, -3.0 * T], [5 * deg * T, 1.5 * T], True, N + 1, 1.0)
        self.ng = len(self.lbg)

    @classmethod
    def from_config(cls, cfg, x0, xs, obs):
        """The dynamic-bicycle NLP that a config (struct mpcb_config) describes, from the config alone (see KinNlp.from_config), with the
        vehicle and tyre parameters.  Keep-out rows stay in the reference's form sqrt(h) >= sqrt(obs_hmin); CBF rows (gamma = 1 on this
        model) are gamma h_i(X_i) + h_i(X_{i+1}) - h_i(X_i) >= gamma obs_hmin as the kinematic reference writes them."""
        assert cfg.model == _MODEL_DYN and cfg.integrator != _INT_RK4
        self = cls.__new__(cls)
        N = self.N = int(cfg.N); self.T = float(cfg.T)
        self.x0 = np.asarray(x0, float).reshape(6); self.xs = np.asarray(xs, float).reshape(6)
        self.Q, self.R, self.DR = np.array(cfg.Q[:6], float), np.array(cfg.R[:2], float), np.array(cfg.DR[:2], float)
        self.m, self.lf, self.lr, self.Iz = float(cfg.veh_m), float(cfg.veh_lf), float(cfg.veh_lr), float(cfg.veh_Iz)
        self.af, self.ar, self.Fyf, self.Fyr = float(cfg.aopt_f), float(cfg.aopt_r), float(cfg.Fymax_f), float(cfg.Fymax_r)
        self.u_last = np.array(cfg.u_last[:2], float)
        self.du0_cost = bool(cfg.du0_cost)
        self.obs_mode, self.gamma, self.integrator = ("dcbf" if cfg.obs_mode == _OBS_DCBF else "keepout"), float(cfg.gamma), "euler"
        self.obs = _obs_array(obs, N, int(cfg.n_obs))
        self.n_obs = self.obs.shape[0]
        self.sx, self.sy = _semi_axes(cfg, self.obs)
        assert not (cfg.obs_terminal and self.obs_mode == "dcbf"), "a CBF row at node N would need X_{N+1}"
        self.obs_nodes = N + 1 if cfg.obs_terminal else N
        self.rate_cols = [c for c in range(2) if np.isfinite(cfg.du_lo[c]) or np.isfinite(cfg.du_hi[c])]
        self.rate_interleaved = bool(cfg.rate_interleaved)
        self.nz = 2 * N + 6 * (N + 1)
        obs_lb = float(cfg.obs_hmin) * self.gamma if self.obs_mode == "dcbf" else float(np.sqrt(cfg.obs_hmin))
        self.lbx, self.ubx, self.lbg, self.ubg = _bounds(N, 6, self.n_obs, cfg.u_lo[:2], cfg.u_hi[:2], cfg.x_lo[:6], cfg.x_hi[:6],
                                                         [cfg.du_lo[c] for c in self.rate_cols], [cfg.du_hi[c] for c in self.rate_cols],
                                                         self.rate_interleaved, self.obs_nodes, obs_lb)
        self.ng = len(self.lbg)
        return self

    def split(self, z):
        N = self.N
        return z[:2 * N].reshape(N, 2), z[2 * N:].reshape(N + 1, 6)

    def rhs(self, X, U):                                                               # dyn.py:156-170
        phi, vx, vy, r, df, ax = X[:, 2], X[:, 3], X[:, 4], X[:, 5], U[:, 0], U[:, 1]
        alf = df - (vy + self.lf * r) / vx
        alr = -(vy - self.lr * r) / vx
        Cf = self.Fyf * 2 * self.af / (self.af ** 2 + alf ** 2)
        Cr = self.Fyr * 2 * self.ar / (self.ar ** 2 + alr ** 2)
        Fcf, Fcr = -Cf * alf, -Cr * alr
        return np.stack([vx * np.cos(phi) - vy * np.sin(phi), vx * np.sin(phi) + vy * np.cos(phi), r, ax + r * vy,
                         -r * vx + 2 / self.m * (Fcf * np.cos(df) + Fcr), 2 / self.Iz * (self.lf * Fcf - self.lr * Fcr)], axis=1)

    def f(self, z):                                                                    # dyn.py:212-225
        U, X = self.split(z)
        e = X[:-1] - self.xs
        Up = np.vstack([self.u_last.astype(z.dtype)[None, :], U[:-1]])
        dU = U - Up if self.du0_cost else (U - Up)[1:]
        return (e * e * self.Q).sum() + (U * U * self.R).sum() + (dU * dU * self.DR).sum()

    def h(self, X, k, step):
        o = self.obs[:, step, :]
        return (X[k, 0] - o[:, 0]) ** 2 / self.sx[:, step] ** 2 + (X[k, 1] - o[:, 1]) ** 2 / self.sy[:, step] ** 2 - 1

    def g(self, z):                                                                    # dyn.py:215-243
        U, X = self.split(z)
        rows = [X[0] - self.x0]
        nxt = X[:-1] + self.T * self.rhs(X[:-1], U)
        _shooting_and_rate_rows(rows, X[1:] - nxt, U, self.rate_cols, self.rate_interleaved)
        for k in range(self.obs_nodes):
            if self.n_obs == 0:
                break
            hk = self.h(X, k, k)
            rows.append(np.sqrt(hk) if self.obs_mode == "keepout" else self.gamma * hk + (self.h(X, k + 1, k) - hk))
        return np.concatenate([np.asarray(r).reshape(-1) for r in rows])

    grad_f = KinNlp.grad_f
    jac_g_dense = KinNlp.jac_g_dense
    _pattern_key = KinNlp._pattern_key
    jac_g = KinNlp.jac_g

    def convert_obstacle_multipliers(self, z, lam_g):
        """The solver's row is h >= 1 with multiplier lam_h; the reference's is sqrt(h) >= 1: lam_sqrt = 2 sqrt(h) lam_h."""
        out = np.array(lam_g, float)
        if self.obs_mode != "keepout":                                                 # CBF rows are stated in h itself
            return out
        gv = self.g(np.asarray(z, float))
        n0 = self.ng - self.obs_nodes * self.n_obs
        out[n0:] = out[n0:] * 2 * gv[n0:]
        return out
