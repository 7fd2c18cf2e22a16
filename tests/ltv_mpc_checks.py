"""Test infrastructure of the LTV-MPC tracker (tests/test_ltv_mpc.py, tests/test_ltv_mpc_host.py): a literal numpy restatement of ONE QP
iteration of the reference (DGSQP/solvers/CA_LTV_MPC.py) in its UNCONDENSED form -- H, h, A_eq, b_eq, variable bounds, A_in as :459-537
and :740-748 lay them out -- with fd and [fAd fBd] from the CPU oracle, evaluated at (q_k, u_{k-1}).  The equalities are eliminated in numpy
and the condensed QP is solved with ``oracle.qp``; the answer is checked against the uncondensed QP's KKT conditions and for strict
complementarity BEFORE any device value is looked at.  The product never imports this."""
import numpy as np

NU = 2
RATE, SLACK, INPUT, STATE, SOFT, OBS = range(6)
STRICT = 1e-6          # strict complementarity: active multipliers and inactive slacks above this, relative


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max())


def record_dict(rec, n_q):
    """The fields of a dgsqp_mpc_t as plain numpy."""
    ns = int(rec.n_soft)
    return dict(N=int(rec.N), n_q=n_q, w_q=np.array(rec.w_q[:n_q]), c_N=np.array(rec.c_N[:n_q]), w_u=np.array(rec.w_u[:]), w_du=np.array(rec.w_du[:]),
                q_ub=np.array(rec.q_ub[:n_q]), q_lb=np.array(rec.q_lb[:n_q]), u_ub=np.array(rec.u_ub[:]), u_lb=np.array(rec.u_lb[:]),
                du_ub=np.array(rec.du_ub[:]), du_lb=np.array(rec.du_lb[:]), soft_idx=[int(i) for i in rec.soft_idx[:ns]],
                soft_quad=np.array(rec.soft_quad[:ns]), soft_lin=np.array(rec.soft_lin[:ns]), obs_r=float(rec.obs_r))


def oracle_dyn(oracle, P, agent):
    def dyn(q, u):
        _, qn, Jac, _ = oracle.dynamics(P, agent, q, u)
        return qn, Jac
    return dyn


def numpy_dyn(fd, h=1e-3):
    """(fd, [fAd fBd]) from a numpy fd by fourth-order central differences (five-point stencil) with step h max(1, |z_i|): truncation
    ~h^4 times the fifth derivative / 30 and rounding ~eps / h, both about 1e-13 relative on these models (a second-order stencil stops at
    1e-10, above the 1e-11 bar of the equality residuals).  The points stay inside one track segment.  For the point mass, which the
    oracle lacks."""
    def dyn(q, u):
        q, u = np.asarray(q, float), np.asarray(u, float)
        z, nq = np.concatenate((q, u)), len(q)
        f = lambda v: np.asarray(fd(v[:nq], v[nq:]), float)
        J = np.zeros((nq, len(z)))
        for i in range(len(z)):
            e = np.zeros(len(z)); e[i] = h * max(1.0, abs(z[i]))
            d = ((z + e)[i] - (z - e)[i]) / 2
            J[:, i] = (8 * (f(z + e) - f(z - e)) - (f(z + 2 * e) - f(z - 2 * e))) / (12 * d)
        return f(z), J
    return dyn


def rollout(dyn, q0, U):
    Q = [np.asarray(q0, float)]
    for u in U:
        Q.append(dyn(Q[-1], u)[0])
    return np.array(Q)


def uncondensed_qp(R, dt, dyn, D, q0, u_prev, q_ref, p_obs, scale_q=None, scale_u=None):
    """H, h, A_eq, b_eq, lb, ub, A_in, lb_in, ub_in of CA_LTV_MPC._build_solver / _solve_casadi at D (len (N+1) n_z + N n_u + 2 n_soft),
    in the reference's scaled variables when scale_q / scale_u (its q_scaling = 1 / state_scaling) are given."""
    N, nq = R['N'], R['n_q']
    nz, ns = nq + NU, len(R['soft_idx'])
    nD = (N + 1) * nz + N * NU + 2 * ns
    Tq = np.ones(nq) if scale_q is None else np.asarray(scale_q, float)
    Tu = np.ones(NU) if scale_u is None else np.asarray(scale_u, float)
    Tqu = np.concatenate((Tq, Tu))
    H, h = np.zeros((nD, nD)), np.zeros(nD)
    A_eq, b_eq = np.zeros(((N + 1) * nz, nD)), np.zeros((N + 1) * nz)
    A_eq[:nz, :nz] = np.eye(nz)
    b_eq[:nz] = Tqu * np.concatenate((q0, u_prev))
    obs_rows, obs_ub = [], []
    for k in range(N + 1):
        q, u = D[k * nz:k * nz + nq], D[k * nz + nq:(k + 1) * nz]
        Mq, mq = np.diag(R['w_q']), R['w_q'] * (q - q_ref[k]) + (R['c_N'] if k == N else 0.0)
        Mu, mu = np.diag(R['w_u']), R['w_u'] * u
        Qk, qk = np.zeros((nz, nz)), np.zeros(nz)
        Qk[:nq, :nq] = Mq / np.outer(Tq, Tq)
        qk[:nq] = (mq - Mq @ q) / Tq
        Qk[nq:, nq:] = Mu / np.outer(Tu, Tu)
        qk[nq:] = (mu - Mu @ u) / Tu
        H[k * nz:(k + 1) * nz, k * nz:(k + 1) * nz] = (Qk + Qk.T) / 2 + 1e-10 * np.eye(nz)
        h[k * nz:(k + 1) * nz] = qk
        if k >= 1 and R['obs_r'] > 0:
            d = q[:2] - p_obs[k - 1]
            C = (2 * R['obs_r']) ** 2 - d @ d
            row = np.zeros(nD)
            row[k * nz:k * nz + 2] = -2 * d / Tq[:2]
            obs_rows.append(row)
            obs_ub.append(-C + (-2 * d) @ q[:2])
        if k < N:
            fd, Jac = dyn(q, u)
            Ad, Bd = Jac[:, :nq], Jac[:, nq:]
            A = np.zeros((nz, nz))
            A[:nq, :nq] = Tq[:, None] * Ad / Tq[None, :]
            A[:nq, nq:] = Tq[:, None] * Bd / Tu[None, :]
            A[nq:, nq:] = np.eye(NU)
            Bm = np.zeros((nz, NU))
            Bm[:nq] = dt * Tq[:, None] * Bd / Tu[None, :]
            Bm[nq:] = dt * np.eye(NU)
            g = np.zeros(nz)
            g[:nq] = Tq * (fd - Ad @ q - Bd @ u)
            A_eq[(k + 1) * nz:(k + 2) * nz, k * nz:(k + 1) * nz] = -A
            A_eq[(k + 1) * nz:(k + 2) * nz, (k + 1) * nz:(k + 2) * nz] = np.eye(nz)
            s, e = (N + 1) * nz + k * NU, (N + 1) * nz + (k + 1) * NU
            A_eq[(k + 1) * nz:(k + 2) * nz, s:e] = -Bm
            b_eq[(k + 1) * nz:(k + 2) * nz] = g
            H[s:e, s:e] = np.diag(R['w_du'])
    cs = (N + 1) * nz + N * NU
    if ns:
        H[cs:, cs:] = 2 * np.diag(np.concatenate((R['soft_quad'], R['soft_quad'])))
        h[cs:] = np.concatenate((R['soft_lin'], R['soft_lin']))
    # variable bounds (:740-748)
    sub, slb = R['q_ub'].copy(), R['q_lb'].copy()
    for j in R['soft_idx']:
        sub[j], slb[j] = np.inf, -np.inf
    qu_ub, qu_lb = np.concatenate((sub, R['u_ub'])), np.concatenate((slb, R['u_lb']))
    lb = np.concatenate((-np.inf * np.ones(nq), R['u_lb'], np.tile(qu_lb, N), np.tile(R['du_lb'], N), np.zeros(2 * ns)))
    ub = np.concatenate((np.inf * np.ones(nq), R['u_ub'], np.tile(qu_ub, N), np.tile(R['du_ub'], N), np.inf * np.ones(2 * ns)))
    scal = np.concatenate((np.tile(Tqu, N + 1), np.ones(N * NU + 2 * ns)))
    lb, ub = scal * lb, scal * ub
    # A_in: the state_input rows stage by stage, then the soft rows (:519-533)
    rows, lbi, ubi = list(obs_rows), [-1e10] * len(obs_rows), list(obs_ub)
    for i, j in enumerate(R['soft_idx']):
        for k in range(N):
            r1 = np.zeros(nD); r1[(k + 1) * nz + j] = 1 / Tq[j]; r1[cs + i] = -1
            r2 = np.zeros(nD); r2[(k + 1) * nz + j] = 1 / Tq[j]; r2[cs + ns + i] = 1
            rows += [r1, r2]; lbi += [-1e10, R['q_lb'][j]]; ubi += [R['q_ub'][j], 1e10]
    A_in = np.array(rows).reshape(-1, nD)
    return dict(H=H, h=h, A_eq=A_eq, b_eq=b_eq, lb=lb, ub=ub, A_in=A_in, lb_in=np.array(lbi), ub_in=np.array(ubi), nD=nD, nz=nz, ns=ns, cs=cs, scal=scal)


def eliminate(qp, N):
    """D = T x + d0 with x = (du, slacks): the equalities solved stage by stage."""
    nD, nz, ns = qp['nD'], qp['nz'], qp['ns']
    nx = N * NU + 2 * ns
    T, d0 = np.zeros((nD, nx)), np.zeros(nD)
    T[(N + 1) * nz:, :] = np.eye(nx)
    d0[:nz] = qp['b_eq'][:nz]
    for k in range(N):
        r = slice((k + 1) * nz, (k + 2) * nz)
        A = -qp['A_eq'][r, k * nz:(k + 1) * nz]
        Bm = -qp['A_eq'][r, (N + 1) * nz + k * NU:(N + 1) * nz + (k + 1) * NU]
        T[r] = A @ T[k * nz:(k + 1) * nz]
        T[r, k * NU:(k + 1) * NU] += Bm
        d0[r] = A @ d0[k * nz:(k + 1) * nz] + qp['b_eq'][r]
    return T, d0


def row_vectors(qp, R, rows):
    """Each condensed row of the device's table as (a over D, bound in `sign a.D <= sign bound`): read off the uncondensed bounds / A_in."""
    N, nq, nz, ns, cs, nD = R['N'], R['n_q'], qp['nz'], qp['ns'], qp['cs'], qp['nD']
    n_obs = N if R['obs_r'] > 0 else 0
    out = []
    for kind, stage, index, sign in rows:
        a = np.zeros(nD)
        if kind in (RATE, SLACK, INPUT, STATE):
            i = {RATE: (N + 1) * nz + stage * NU + index, SLACK: cs + index, INPUT: stage * nz + nq + index, STATE: stage * nz + index}[kind]
            a[i] = 1.0
            bound = qp['ub'][i] if sign > 0 else qp['lb'][i]
        elif kind == SOFT:
            r = n_obs + 2 * N * index + 2 * (stage - 1) + (0 if sign > 0 else 1)
            a = qp['A_in'][r].copy()
            bound = qp['ub_in'][r] if sign > 0 else qp['lb_in'][r]
        else:
            a = qp['A_in'][stage - 1].copy()
            bound = qp['ub_in'][stage - 1]
        assert np.isfinite(bound) and abs(bound) < 1e9, (kind, stage, index, sign, bound)
        out.append((sign * a, sign * bound))
    # the table holds every finite bound of the uncondensed QP past block 0, and every A_in row
    n_fin = int((np.abs(qp['lb'][nz:]) < 1e9).sum() + (np.abs(qp['ub'][nz:]) < 1e9).sum())
    n_ain = int((np.abs(qp['lb_in']) < 1e9).sum() + (np.abs(qp['ub_in']) < 1e9).sum())
    assert len(rows) == n_fin + n_ain, (len(rows), n_fin, n_ain)
    return out


UTOL = 1e-12          # DG_MPC_UTOL (csrc/dgsqp_mpc.h)


def clamp_u_prev(R, u_prev):
    """The product's stated rule for the fixed and bounded u_{-1}: within UTOL max(1, |bound|) beyond an input bound it is moved onto the
    bound (a saturated input the tracker returned comes back a row tolerance or an ulp outside); farther out it stays, and the QP is
    infeasible as in the reference."""
    u = np.array(u_prev, float)
    for j in range(NU):
        ub, lb = R['u_ub'][j], R['u_lb'][j]
        if abs(ub) < 1e9 and ub < u[j] <= ub + UTOL * max(1.0, abs(ub)):
            u[j] = ub
        if abs(lb) < 1e9 and lb - UTOL * max(1.0, abs(lb)) <= u[j] < lb:
            u[j] = lb
    return u


def solve_iteration(oracle, R, dt, dyn, rows, D, q0, u_prev, q_ref, p_obs):
    """One QP of the reference at D.  Returns the helper's own, checked answer (D_bar, lam per row, active set, scales) or flag != 0."""
    N = R['N']
    u_prev = clamp_u_prev(R, u_prev)
    qp = uncondensed_qp(R, dt, dyn, D, q0, u_prev, q_ref, p_obs)
    T, d0 = eliminate(qp, N)
    Hc = T.T @ qp['H'] @ T
    Hc = (Hc + Hc.T) / 2
    gc = T.T @ (qp['H'] @ d0 + qp['h'])
    rv = row_vectors(qp, R, rows)
    Ad = np.array([a for a, _ in rv]).reshape(-1, qp['nD'])
    bd = np.array([b for _, b in rv])
    G, g = Ad @ T, Ad @ d0 - bd
    out = dict(qp=qp, T=T, d0=d0, Hc=Hc, gc=gc, G=G, g=g, Ad=Ad, bd=bd)
    # block 0's bound on u_{-1} is a constant: violated means infeasible
    nz, nq = qp['nz'], R['n_q']
    if np.any(d0[nq:nz] > qp['ub'][nq:nz]) or np.any(d0[nq:nz] < qp['lb'][nq:nz]):
        out['flag'] = 1
        return out
    x, lam, flag = oracle.qp(Hc, gc, G, g)
    out['flag'] = flag
    if flag != 0:
        return out
    Dbar = T @ x + d0
    scale = max(1.0, np.abs(gc).max())
    # KKT of the UNCONDENSED QP: stationarity with the equality multipliers by least squares, feasibility, complementarity
    rhs = -(qp['H'] @ Dbar + qp['h'] + Ad.T @ lam)
    nu = np.linalg.lstsq(qp['A_eq'].T, rhs, rcond=None)[0]
    stat = np.abs(qp['A_eq'].T @ nu - rhs).max()
    assert stat < 1e-7 * max(1.0, np.abs(qp['h']).max()), stat
    assert np.abs(qp['A_eq'] @ Dbar - qp['b_eq']).max() < 1e-11 * max(1.0, np.abs(Dbar).max())
    slack = -(Ad @ Dbar - bd)
    assert slack.min() > -1e-9 and lam.min() >= 0 and np.abs(lam * slack).max() < 1e-8 * scale
    act = lam > 0
    lam_scale, slack_scale = max(1.0, lam.max() if len(lam) else 0.0), max(1.0, np.abs(bd).max() if len(bd) else 0.0)
    out.update(x=x, lam=lam, D_bar=Dbar, active=act, scale=scale,
               strict=bool((lam[act] > STRICT * lam_scale).all() and (slack[~act] > STRICT * slack_scale).all()),
               cond_scale=1.0)      # (test_qp_parity_and_kkt: raw over projected Hessian; nothing is projected here)
    return out


def replay_update(D, D_bar, damping, lenD_state_du, N, nz, zero_du):
    """numpy replay of the damped update and the zeroing (CA_LTV_MPC.py:185-186, :255-257), bit for bit what the device does."""
    new = damping * D + (1.0 - damping) * D_bar
    new[lenD_state_du:] = 0.0
    if zero_du:
        new[(N + 1) * nz:] = 0.0
    return new
