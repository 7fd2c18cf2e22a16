"""Known-answer vectors for the MULTI-STAGE stage quantities x, g, G, q, Q of ``_evaluate`` (DGSQP.py:509-533) from plain functions
in 60-digit arithmetic and central differences.  Writes tests/golden/multistage_<case>.npz.

DGSQP.py:937-941 states what Q is: row block a of  d2/du2 [J^a(u) + l . C(u)],  J^a and C functions of the input sequence u through
the rollout.  This tool writes the rollout, the costs and the rows as plain mpmath functions of u and differences them:

    G[:, i]  = (C(u + h e_i) - C(u - h e_i)) / 2h                   q[i] = the same of J^a(i)
    Q[i, j]  = (L^a(i)(+i +j) - L^a(i)(+i -j) - L^a(i)(-i +j) + L^a(i)(-i -j)) / 4h^2,      L^a = J^a + l . C
    (G v)    = (C(u + h v) - C(u - h v)) / 2h                       (Q v)[i] = the mixed difference along e_i and v

with 60 digits and h = 1e-20 (first derivatives good to ~1e-40, second to ~1e-20).  No dynamic programming, no Taylor arithmetic, no
adjoints, no A/B/E/F/G tensors: nothing is shared with oracle/ or dgsqp_amd/csrc except the reference's text --

    continuous dynamics   dynamics_models.py:331-339 (unicycle), :536-541 (Frenet point mass), :1046-1070 (kinematic bicycle), :2013-2062 (dynamic bicycle; Pacejka
                          and linear tyres, simple slip angle, rear-wheel drive), ca_abs :228-234, ca_sign :236-238
    discretisation        :88-99 euler, :188-219 rk4 / rk3 / rk2 with M substeps of h = dt / M
    track                 radius_arclength_track.py:361-408 (key points), :199-225 (curvature pw_const, tangent pw_lin) as a true
                          piecewise function of s
    racing costs          DGSQP_ALGAMES_monte_carlo_chicane.py:47, :223-277; comparison_study_barc/exact_dynamic_game_dynamic.py:140-168
    merge costs / lanes   DGSQP_merge_monte_carlo.py:66-74, :253-261, :316-342
    rows, their order     DGSQP.py:730-821 (shared rows first, then per agent: function rows, input ub, input lb, state ub, state lb;
                          state boxes from k = 1); u_{-1} = 0, or the scenario's u_prev in the *_uprev cases (the `up` that
                          DGSQP.py:509-533, :656-670 carry through every stage function)

The numbers the reference computes in double precision before it builds its expressions (track tables, h = dt / M, dt * rate) are
computed in double precision here too and enter the 60-digit arithmetic exactly.  Vehicle parameters are the defaults of the
reference's own config classes (DGSQP/dynamics/model_types.py, imported live from the tree given with --reference) plus the literals
of the scripts; every parameter is stored in the file and tests/multistage_kat.py asserts that the game the tests build has them.
The package is used for ONE thing: ``sample_scenarios`` draws the input points (x0, warm start) -- any point is a valid input, the
answers never see the package.

Every answer is computed twice (60 digits / h = 1e-20 -- 70 digits for the merge game, see DIGITS -- and 90 digits / h = 1e-30; the largest relative disagreement is stored as
``acc_<key>`` and a file is refused above 1e-18) and carries its SENSITIVITY ``sens_<key>``: the largest relative change of the
quantity over 8 evaluations with x0 and u perturbed by 2^-53 relative -- the floor any fp64 evaluation of the same inputs can be held
to, from the reference side alone.  Every evaluated state, at every integrator stage, is asserted to stay 1e-3 away from the
breakpoints of the piecewise definitions (segment boundaries, v = 0, the hinge of the obstacle cost, the lane normals' brk).

    usage: python tools/make_multistage_kats.py [--reference DIR] [--jobs J] [case ...]
"""
import argparse
import os
import pathlib
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLD = ROOT / 'tests' / 'golden'
MARGIN = 1e-3
INF = float('inf')


# ---------------------------------------------------------------------------------------------
# numbers the reference prepares in double precision
# ---------------------------------------------------------------------------------------------
def arc_track_tables(cl_segs):
    """get_track_key_pts (radius_arclength_track.py:361-408: cumulative length, segment length, curvature 1 / r) and abs_angs of
    get_tangent_angle_casadi_fn (:207-217).  cl_segs rows are (length, radius), radius 0 = straight."""
    cl = np.asarray(cl_segs, float)
    n = len(cl)
    cum, seg_len, curv = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
    for i in range(1, n + 1):
        l, r = cl[i - 1]
        cum[i], seg_len[i], curv[i] = cum[i - 1] + l, l, (0.0 if r == 0 else 1 / r)
    ang = np.zeros(n + 2)
    for i in range(n + 1):
        ang[i + 1] = ang[i] if curv[i] == 0 else ang[i] + seg_len[i] * curv[i]
    return dict(L=float(cum[-1]), seg_s=cum, seg_curv=curv[1:].copy(), seg_ang=ang[1:].copy())


def curve_track(theta_deg=45):          # DGSQP_ALGAMES_monte_carlo_curve.py:140-146, track_lib.py:27-52
    th = theta_deg * np.pi / 180
    return arc_track_tables([[1, 0], [8, 8 / th], [5, 0]])


def chicane_track(theta_deg=45):        # DGSQP_ALGAMES_monte_carlo_chicane.py:140-149, track_lib.py:54-87 (mirror=False: s1, s2 = -1, 1)
    th = theta_deg * np.pi / 180
    return arc_track_tables([[1, 0], [4, -1 * 4 / th], [1, 0], [4, 1 * 4 / th], [5, 0]])


# ---------------------------------------------------------------------------------------------
# the game as plain functions (mpmath)
# ---------------------------------------------------------------------------------------------
class Margin:
    """Smallest distance of any evaluated state to a breakpoint of a piecewise definition."""
    def __init__(self):
        self.m, self.what = INF, ''

    def see(self, d, what):
        d = abs(float(d))
        if d < self.m:
            self.m, self.what = d, what


def F(x):
    return mp.mpf(float(x))             # a double, exactly


def ca_abs(x, mg):                      # dynamics_models.py:228-234: if_else(x > 0, x, -x)
    mg.see(x, 'v = 0')
    return x if x > 0 else -x


def ca_sign(x):                         # :236-238, eps = 1e-3
    return x / mp.sqrt(x ** 2 + F(1e-3) ** 2)


def track_fn(tr, s, mg):
    """curvature pw_const(sbar, key_pts[1:-1, 3], key_pts[1:, 5]), tangent pw_lin(sbar, key_pts[:, 3], abs_angs) with
    sbar = fmod(fmod(s, L) + L, L) (radius_arclength_track.py:199-225); pw_lin's slopes are doubles (numeric DM arithmetic)."""
    L = F(tr['L'])
    sbar = s - L * mp.floor(s / L)
    seg_s = tr['seg_s']
    n = len(tr['seg_curv'])
    for b in seg_s:
        mg.see(sbar - F(b), f'segment boundary s = {b:g}')
    i = 0
    while i + 1 < n and sbar >= F(seg_s[i + 1]):
        i += 1
    slope = (tr['seg_ang'][i + 1] - tr['seg_ang'][i]) / (seg_s[i + 1] - seg_s[i])
    return F(tr['seg_curv'][i]), F(tr['seg_ang'][i]) + F(slope) * (sbar - F(seg_s[i]))


def fc_uni(p, tr, q, u, mg):            # dynamics_models.py:331-339
    x, y, v, psi = q
    return [v * mp.cos(psi), v * mp.sin(psi), u[0] / F(p['mass']), u[1]]


def fc_pm(p, tr, q, u, mg):             # dynamics_models.py:536-541 (mass and damping_coefficient: all the class reads there)
    x, y, v, epsi, s, xtran = q
    Fx, wz = u
    c, psi_t = track_fn(tr, s, mg)
    dx = v * mp.cos(psi_t + epsi)
    dy = v * mp.sin(psi_t + epsi)
    dv = (Fx - F(p['damping_coefficient']) * v) / F(p['mass'])
    depsi = wz - c * (v * mp.cos(epsi)) / (1 - xtran * c)
    ds = v * mp.cos(epsi) / (1 - xtran * c)
    dxtran = v * mp.sin(epsi)
    return [dx, dy, dv, depsi, ds, dxtran]


def fc_kin(p, tr, q, u, mg):            # dynamics_models.py:1046-1070
    x, y, v, epsi, s, xtran = q
    a, gamma = u
    L_f, L_r, m = F(p['wheel_dist_front']), F(p['wheel_dist_rear']), F(p['mass'])
    beta = mp.atan2(mp.tan(gamma) * L_r, L_f + L_r)
    psidot = v / L_r * mp.sin(beta)
    F_ext = - F(p['damping_coefficient']) * v - F(p['drag_coefficient']) * v * ca_abs(v, mg) - F(p['slip_coefficient']) * psidot ** 2
    if p['rolling_resistance'] != 0:
        F_ext -= F(p['rolling_resistance']) * ca_abs(v, mg) ** F(p['rolling_resistance_exponent']) * ca_sign(v)
    c, psi_t = track_fn(tr, s, mg)
    den = 1 - xtran * c
    return [v * mp.cos(beta + psi_t + epsi), v * mp.sin(beta + psi_t + epsi), a + F_ext / m,
            psidot - c * v * mp.cos(beta + epsi) / den, v * mp.cos(beta + epsi) / den, v * mp.sin(beta + epsi)]


def fc_dyn(p, tr, q, u, mg):            # dynamics_models.py:2013-2062
    x, y, vx, vy, psidot, epsi, s, xtran = q
    a, gamma = u
    L_f, L_r, m, I_z, g = (F(p[k]) for k in ('wheel_dist_front', 'wheel_dist_rear', 'mass', 'yaw_inertia', 'gravity'))
    c, psi_t = track_fn(tr, s, mg)
    if p['simple_slip']:
        alpha_f = -mp.atan2(vy + L_f * psidot, vx) + gamma
    else:
        alpha_f = -mp.atan2((vy + L_f * psidot) * mp.cos(gamma) - vx * mp.sin(gamma), vx * mp.cos(gamma) + (vy + L_f * psidot) * mp.sin(gamma))
    alpha_r = -mp.atan2(vy - L_r * psidot, vx)
    if p['tire_model'] == 'pacejka':
        fyf = F(p['pacejka_d_front']) * mp.sin(F(p['pacejka_c_front']) * mp.atan(F(p['pacejka_b_front']) * alpha_f))
        fyr = F(p['pacejka_d_rear']) * mp.sin(F(p['pacejka_c_rear']) * mp.atan(F(p['pacejka_b_rear']) * alpha_r))
    else:
        assert p['tire_model'] == 'linear'
        fyf = F(p['linear_bf']) * m * g * L_r / (L_f + L_r) * alpha_f
        fyr = F(p['linear_br']) * m * g * L_f / (L_f + L_r) * alpha_r
    F_ext = - F(p['damping_coefficient']) * vx - F(p['drag_coefficient']) * vx * ca_abs(vx, mg)
    if p['rolling_resistance'] != 0:
        F_ext -= F(p['rolling_resistance']) * ca_abs(vx, mg) ** F(p['rolling_resistance_exponent']) * ca_sign(vx)
    mg.see(vx, 'v = 0')                                                      # (atan2(., vx): the slip angles' own breakpoint)
    if p['drive_wheels'] == 'all':
        ar, af = a / 2, a / 2
    else:
        assert p['drive_wheels'] == 'rear'
        ar, af = a, mp.mpf(0)
    ax = ar + af * mp.cos(gamma) + (F_ext - fyf * mp.sin(gamma)) / m
    ay = af * mp.sin(gamma) + (fyf * mp.cos(gamma) + fyr) / m
    alphaz = (L_f * fyf * mp.cos(gamma) - L_r * fyr) / I_z
    vlon = vx * mp.cos(epsi) - vy * mp.sin(epsi)
    den = 1 - xtran * c
    return [vx * mp.cos(epsi + psi_t) - vy * mp.sin(epsi + psi_t), vy * mp.cos(epsi + psi_t) + vx * mp.sin(epsi + psi_t),
            ax + psidot * vy, ay - psidot * vx, alphaz, psidot - c * vlon / den, vlon / den, vx * mp.sin(epsi) + vy * mp.cos(epsi)]


FC = {'uni': fc_uni, 'kin': fc_kin, 'dyn': fc_dyn, 'pm': fc_pm}
NQ = {'uni': 4, 'kin': 6, 'dyn': 8, 'pm': 6}
S_IDX = {'kin': 4, 'dyn': 6, 'pm': 4}   # s; e_y (x_tran) is the state after it
VEHICLE_KEYS = {
    'uni': ['mass'],
    'pm': ['mass', 'damping_coefficient'],
    'kin': ['wheel_dist_front', 'wheel_dist_rear', 'mass', 'drag_coefficient', 'damping_coefficient', 'slip_coefficient', 'rolling_resistance',
            'rolling_resistance_exponent'],
    'dyn': ['wheel_dist_front', 'wheel_dist_rear', 'mass', 'yaw_inertia', 'gravity', 'drag_coefficient', 'damping_coefficient', 'rolling_resistance',
            'rolling_resistance_exponent', 'simple_slip', 'tire_model', 'drive_wheels', 'pacejka_b_front', 'pacejka_c_front', 'pacejka_d_front',
            'pacejka_b_rear', 'pacejka_c_rear', 'pacejka_d_rear', 'linear_bf', 'linear_br'],
}


def fd(spec, ag, q, u, mg):
    """dynamics_models.py:88-99, :188-219."""
    f = lambda x: FC[ag['model']](ag['vehicle'], spec['track'], x, u, mg)
    axpy = lambda x, c, a: [xi + c * ai for xi, ai in zip(x, a)]
    meth = spec['method']
    if meth == 'euler':
        return axpy(q, F(spec['dt']), f(q))
    h = F(spec['dt'] / spec['substeps'])
    x = list(q)
    for _ in range(spec['substeps']):
        if meth == 'rk4':
            a1 = f(x); a2 = f(axpy(x, h / 2, a1)); a3 = f(axpy(x, h / 2, a2)); a4 = f(axpy(x, h, a3))
            x = [xi + h * (b1 + 2 * b2 + 2 * b3 + b4) / 6 for xi, b1, b2, b3, b4 in zip(x, a1, a2, a3, a4)]
        elif meth == 'rk3':
            a1 = [h * v for v in f(x)]
            a2 = [h * v for v in f(axpy(x, mp.mpf(1) / 2, a1))]
            a3 = [h * v for v in f([xi - b1 + 2 * b2 for xi, b1, b2 in zip(x, a1, a2)])]
            x = [xi + (b1 + 4 * b2 + b3) / 6 for xi, b1, b2, b3 in zip(x, a1, a2, a3)]
        else:
            assert meth == 'rk2'
            a1 = f(x); a2 = f(axpy(x, h, a1))
            x = [xi + h * (b1 + b2) / 2 for xi, b1, b2 in zip(x, a1, a2)]
    return x


def stage_state_cost(spec, a, xs, mg):
    """The state part of agent a's stage AND terminal cost: blocking + soft obstacle (chicane.py:227-228, 234-242; over all opponents,
    DGSQP_monte_carlo_agents.py) / goal tracking (merge.py:253-261, without the terminal multiplier)."""
    c = spec['agents'][a]['cost']
    J = mp.mpf(0)
    if c['kind'] == 'goal':
        for i, (w, gl) in enumerate(zip(c['state_weight'], c['goal'])):
            J += F(w) * (xs[a][i] - F(gl)) ** 2 / 2
        return J
    for b in range(spec['M']):
        if b == a:
            continue
        if c['blocking_weight'] != 0:
            ey = lambda i: xs[i][S_IDX[spec['agents'][i]['model']] + 1]
            J += F(c['blocking_weight']) * (ey(a) - ey(b)) ** 2 / 2
        if c['obs_weight'] != 0:
            d = F(c['obs_r'] + spec['agents'][b]['cost']['obs_r']) - mp.sqrt((xs[a][0] - xs[b][0]) ** 2 + (xs[a][1] - xs[b][1]) ** 2)
            mg.see(d, 'hinge of the obstacle cost')
            J += F(c['obs_weight']) * (d if d > 0 else mp.mpf(0)) ** 2 / 2        # saturation_cost = fmax(0, .) (chicane.py:47)
    return J


def zero_up(M):
    return [[mp.mpf(0), mp.mpf(0)] for _ in range(M)]


def costs(spec, traj, ua, mg, up=None):
    """J^a = sum_k stage(x_k, u_k, u_{k-1}) + terminal(x_N), u_{-1} = up[a] (None: 0) (DGSQP.py:656-670).  traj[a][k] the states, ua[a][k]
    the inputs."""
    up = zero_up(spec['M']) if up is None else up
    N, M = spec['N'], spec['M']
    out = []
    for a in range(M):
        c = spec['agents'][a]['cost']
        J = mp.mpf(0)
        for k in range(N):
            um = ua[a][k - 1] if k > 0 else up[a]
            for j in range(2):
                J += F(c['input_weight'][j]) * ua[a][k][j] ** 2 / 2 + F(c['input_rate_weight'][j]) * (ua[a][k][j] - um[j]) ** 2 / 2
            J += stage_state_cost(spec, a, [traj[b][k] for b in range(M)], mg)
        xN = [traj[b][N] for b in range(M)]
        if c['kind'] == 'goal':
            J += F(c['terminal_multiplier']) * stage_state_cost(spec, a, xN, mg)
        else:
            s = lambda i: xN[i][S_IDX[spec['agents'][i]['model']]]
            J += -F(c['comp_weights'][0]) * s(a) + stage_state_cost(spec, a, xN, mg)
            for b in range(M):
                if b != a:
                    d = s(b) - s(a)
                    J += F(c['comp_weights'][1]) * (mp.atan(d) if c['comp_type'] == 'atan' else d)
        out.append(J)
    return out


def rows(spec, traj, ua, mg, up=None):
    """C(u), DGSQP.py:730-821; the rate rows of stage 0 are measured against up[a] (None: 0)."""
    up = zero_up(spec['M']) if up is None else up
    N, M = spec['N'], spec['M']
    dt = spec['dt']
    C = []
    for k in range(N + 1):
        if spec['obstacle_rows'] and k >= 1:                     # shared rows: None at k = 0 (chicane.py:324-330); pairs i < j (merge.py:344-349)
            for i in range(M):
                for j in range(i + 1, M):
                    r = F(spec['agents'][i]['radius'] + spec['agents'][j]['radius'])
                    C.append(r ** 2 - ((traj[i][k][0] - traj[j][k][0]) ** 2 + (traj[i][k][1] - traj[j][k][1]) ** 2))
        for a in range(M):
            ag = spec['agents'][a]
            if k < N and ag['rate'] is not None:                  # chicane.py:282-285
                um = ua[a][k - 1] if k > 0 else up[a]
                for j in range(2):
                    C.append((ua[a][k][j] - um[j]) - F(dt * ag['rate'][0][j]))
                    C.append(F(dt * ag['rate'][1][j]) - (ua[a][k][j] - um[j]))
            for ln in ag['lanes']:                                # merge.py:66-74: n(p_x)^T (p - (anchor - r n(p_x))), at every stage
                px, py = traj[a][k][0], traj[a][k][1]
                if ln['brk'] < INF:
                    mg.see(px - F(ln['brk']), 'brk of a lane normal')
                n = ln['n_lo'] if px < F(ln['brk']) else ln['n_hi']
                C.append(F(n[0]) * (px - (F(ln['anchor'][0]) - F(ln['r']) * F(n[0]))) + F(n[1]) * (py - (F(ln['anchor'][1]) - F(ln['r']) * F(n[1]))))
            if k < N:
                C += [ua[a][k][j] - F(ag['in_ub'][j]) for j in range(2) if ag['in_ub'][j] < INF]
                C += [F(ag['in_lb'][j]) - ua[a][k][j] for j in range(2) if ag['in_lb'][j] > -INF]
            if k > 0:
                C += [traj[a][k][i] - F(ag['st_ub'][i]) for i in range(NQ[ag['model']]) if ag['st_ub'][i] < INF]
                C += [F(ag['st_lb'][i]) - traj[a][k][i] for i in range(NQ[ag['model']]) if ag['st_lb'][i] > -INF]
    return C


class GameMP:
    """J^a and C at u + h (sum_i c_i e_i + c_v v), the agents' rollouts cached by the part of the perturbation that reaches them
    (the dynamics are decoupled: dynamics_models.py:2521-2528)."""
    def __init__(self, spec, x0, u, l, h, v=None, up=None):
        self.spec, self.h = spec, h
        M, N = spec['M'], spec['N']
        self.up = zero_up(M) if up is None else [[mp.mpf(e) for e in up[2 * a:2 * a + 2]] for a in range(M)]      # joint order: agent a's inputs at 2 a
        self.n = 2 * M * N
        self.u = [mp.mpf(e) for e in u]
        self.v = None if v is None else [F(e) for e in v]
        self.l = [F(e) for e in l]
        off = np.cumsum([0] + [NQ[ag['model']] for ag in spec['agents']])
        self.x0 = [[mp.mpf(e) for e in x0[off[a]:off[a + 1]]] for a in range(M)]
        self.mg = Margin()
        self.cache, self.points = {}, {}

    def agent(self, a, pert, cv):
        N = self.spec['N']
        lo, hi = 2 * N * a, 2 * N * (a + 1)
        sub = tuple((i, c) for i, c in pert if lo <= i < hi)
        key = (a, sub, cv)
        if key not in self.cache:
            ua = self.u[lo:hi]
            for i, c in sub:
                ua[i - lo] = ua[i - lo] + c * self.h
            if cv:
                ua = [e + cv * self.h * w for e, w in zip(ua, self.v[lo:hi])]
            ua = [ua[2 * k:2 * k + 2] for k in range(N)]
            xs = [self.x0[a]]
            for k in range(N):
                xs.append(fd(self.spec, self.spec['agents'][a], xs[-1], ua[k], self.mg))
            self.cache[key] = (xs, ua)
        return self.cache[key]

    def at(self, pert=(), cv=0):
        """(J [M], C [n_c], L [M]) at the perturbed point; ``pert`` a sorted tuple of (index, integer multiple of h)."""
        key = (pert, cv)
        if key not in self.points:
            both = [self.agent(a, pert, cv) for a in range(self.spec['M'])]
            traj, ua = [b[0] for b in both], [b[1] for b in both]
            J, C = costs(self.spec, traj, ua, self.mg, self.up), rows(self.spec, traj, ua, self.mg, self.up)
            lC = mp.fsum(li * ci for li, ci in zip(self.l, C) if li != 0)
            self.points[key] = (J, C, [j + lC for j in J])
        return self.points[key]


def split(nested):
    """Nested lists of mpf -> (hi, lo) float64 arrays with hi + lo the value to ~32 digits: the answers go to the file as ``hi``, the
    accuracy record and the sensitivity are taken from hi + lo (differences of rounded float64 values would only show whole ulps)."""
    a = np.array(nested, dtype=object)
    hi = np.array([float(e) for e in a.ravel()]).reshape(a.shape)
    lo = np.array([float(e - mp.mpf(h)) for e, h in zip(a.ravel(), hi.ravel())]).reshape(a.shape)
    return hi, lo


def answers(spec, x0, u, l, dps, h_exp, vs=(), full=True, up=None):
    """x, g, J, q and G, Q (``full``) and/or G v, Q v for the directions ``vs``, each as (float64 array, float64 array of what the
    rounding to float64 left over); plus the breakpoint margin.  ``up`` [n_u]: the joint input before stage 0 (None: zeros)."""
    mp.mp.dps = dps
    h = mp.mpf(10) ** (-h_exp)
    M, N = spec['M'], spec['N']
    n = 2 * M * N
    own = lambda i: i // (2 * N)
    gm = GameMP(spec, x0, u, l, h, up=up)
    J0, C0, L0 = gm.at()
    nc = len(C0)
    assert nc == len(l), (nc, len(l))
    out = {}
    traj = [gm.agent(a, (), 0)[0] for a in range(M)]
    out['x'] = [[e for a in range(M) for e in traj[a][k]] for k in range(N + 1)]
    out['g'] = list(C0)
    out['J'] = list(J0)
    q = [None] * n
    G = [[None] * n for _ in range(nc)]
    for i in range(n):
        (Jp, Cp, _), (Jm, Cm, _) = gm.at(((i, 1),)), gm.at(((i, -1),))
        q[i] = (Jp[own(i)] - Jm[own(i)]) / (2 * h)
        if full:
            for r, (cp, cm) in enumerate(zip(Cp, Cm)):
                G[r][i] = (cp - cm) / (2 * h)
    out['q'] = q
    if full:
        Q = [[None] * n for _ in range(n)]
        for i in range(n):
            Q[i][i] = (gm.at(((i, 1),))[2][own(i)] - 2 * L0[own(i)] + gm.at(((i, -1),))[2][own(i)]) / h ** 2
            for j in range(i + 1, n):
                Ls = [gm.at(((i, si), (j, sj)))[2] for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
                for r, c in ((i, j), (j, i)):
                    Q[r][c] = (Ls[0][own(r)] - Ls[1][own(r)] - Ls[2][own(r)] + Ls[3][own(r)]) / (4 * h ** 2)
        out['G'], out['Q'] = G, Q
    margin = (gm.mg.m, gm.mg.what)
    Gv, Qv = [], []
    for v in vs:
        gv = GameMP(spec, x0, u, l, h, v=v, up=up)
        gv.cache.update({k: val for k, val in gm.cache.items()})          # (rollouts without a v part are the same)
        Cp, Cm = gv.at((), 1)[1], gv.at((), -1)[1]
        Gv.append([(cp - cm) / (2 * h) for cp, cm in zip(Cp, Cm)])
        row = []
        for i in range(n):
            Ls = [gv.at(((i, si),), sv)[2][own(i)] for si, sv in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
            row.append((Ls[0] - Ls[1] - Ls[2] + Ls[3]) / (4 * h ** 2))
            for si in (1, -1):                                            # (bounded memory on the n = 150 cases)
                for sv in (1, -1):
                    gv.points.pop((((i, si),), sv), None)
        Qv.append(row)
        margin = min(margin, (gv.mg.m, gv.mg.what))
    if vs:
        out['Gv'], out['Qv'] = Gv, Qv
    return {k: split(v) for k, v in out.items()}, margin


def relerr(a, b):
    return float(np.abs((a[0] - b[0]) + (a[1] - b[1])).max() / max(1e-300, np.abs(b[0]).max()))


def _run(job):
    spec, x0, u, l, dps, h_exp, vs, full, up = job
    return answers(spec, x0, u, l, dps, h_exp, vs, full, up)


KEYS = ('x', 'g', 'q', 'G', 'Q', 'Gv', 'Qv')


def solve_case(spec, x0, u, l, vs=(), full=True, pool=None, n_sens=8, seed=0, dps=60, up=None):
    """All scenarios of a case: the answers at ``dps`` digits, their accuracy record against 90 digits, their sensitivity.  ``up`` [B, n_u]:
    u_prev per scenario (None: zeros); it is perturbed with x0 and u for the sensitivity (after them: a case without one draws what it drew)."""
    rng = np.random.default_rng(seed)
    mp.mp.dps = 60
    jobs, tags = [], []
    for b in range(len(x0)):
        upb = None if up is None else up[b]
        jobs += [(spec, x0[b], u[b], l[b], dps, 20, vs, full, upb), (spec, x0[b], u[b], l[b], 90, 30, vs, full, upb)]
        tags += [(b, 'ans'), (b, 'chk')]
        for _ in range(n_sens):
            # 2^-53 relative, as exact 60-digit numbers (a double times 1 + 2^-53 is no double)
            px = [mp.mpf(float(e)) * (1 + mp.mpf(2) ** -53 * int(s)) for e, s in zip(x0[b], rng.choice((-1, 1), len(x0[b])))]
            pu = [mp.mpf(float(e)) * (1 + mp.mpf(2) ** -53 * int(s)) for e, s in zip(u[b], rng.choice((-1, 1), len(u[b])))]
            pp = None if upb is None else [mp.mpf(float(e)) * (1 + mp.mpf(2) ** -53 * int(s)) for e, s in zip(upb, rng.choice((-1, 1), len(upb)))]
            jobs.append((spec, px, pu, l[b], dps, 20, vs, full, pp))
            tags.append((b, 'sens'))
    res = list(pool.map(_run, jobs)) if pool is not None else [_run(j) for j in jobs]
    out = {}
    acc, sens = {}, {}
    margin = (INF, '')
    per = [dict() for _ in x0]
    for (b, tag), (ans, mgn) in zip(tags, res):
        if tag != 'sens':
            margin = min(margin, mgn)
        per[b].setdefault(tag, []).append(ans)
    for k in KEYS + ('J',):
        if k not in per[0]['ans'][0]:
            continue
        out[k] = np.array([p['ans'][0][k][0] for p in per])
        if k == 'J':
            continue
        acc[k] = max(relerr(p['ans'][0][k], p['chk'][0][k]) for p in per)
        sens[k] = max(relerr(s[k], p['ans'][0][k]) for p in per for s in p['sens'])
    return out, acc, sens, margin


# ---------------------------------------------------------------------------------------------
# parameters <-> file
# ---------------------------------------------------------------------------------------------
def flatten_spec(spec):
    """Every parameter of the game as plain arrays / strings under ``p_*`` (data only)."""
    out = {'p_M': spec['M'], 'p_N': spec['N'], 'p_dt': spec['dt'], 'p_method': spec['method'], 'p_substeps': spec['substeps'],
           'p_obstacle_rows': int(spec['obstacle_rows']), 'p_has_track': int(spec['track'] is not None)}
    if spec['track'] is not None:
        for k, v in spec['track'].items():
            out['p_track_' + k] = np.asarray(v, float)
    for a, ag in enumerate(spec['agents']):
        pre = f'p_a{a}_'
        out[pre + 'model'] = ag['model']
        for k, v in ag['vehicle'].items():
            out[pre + 'vehicle_' + k] = v
        for k, v in ag['cost'].items():
            out[pre + 'cost_' + k] = v if isinstance(v, str) else np.asarray(v, float)
        out[pre + 'has_rate'] = int(ag['rate'] is not None)
        if ag['rate'] is not None:
            out[pre + 'rate'] = np.asarray(ag['rate'], float)
        out[pre + 'n_lane'] = len(ag['lanes'])
        for j, ln in enumerate(ag['lanes']):
            out[pre + f'lane{j}'] = np.array([ln['brk'], ln['r'], *ln['n_lo'], *ln['n_hi'], *ln['anchor']], float)
        for k in ('in_ub', 'in_lb', 'st_ub', 'st_lb'):
            out[pre + k] = np.asarray(ag[k], float)
        out[pre + 'radius'] = float(ag['radius'])
    return out


def unflatten_spec(kat):
    """The inverse of ``flatten_spec``: the game of a fixture from its ``p_*`` entries alone (what a test needs to run this generator on a
    committed case without the reference tree)."""
    item = lambda k: kat[k].item() if kat[k].ndim == 0 else kat[k]
    track = None
    if int(item('p_has_track')):
        track = {k[len('p_track_'):]: (float(kat[k]) if kat[k].ndim == 0 else [float(e) for e in kat[k]]) for k in kat.files if k.startswith('p_track_')}
    agents = []
    for a in range(int(item('p_M'))):
        pre = f'p_a{a}_'
        take = lambda group: {k[len(pre + group):]: item(k) for k in kat.files if k.startswith(pre + group)}
        cost = {k: (v if isinstance(v, str) else (float(v) if np.ndim(v) == 0 else tuple(float(e) for e in v))) for k, v in take('cost_').items()}
        lanes = []
        for j in range(int(item(pre + 'n_lane'))):
            ln = [float(e) for e in kat[pre + f'lane{j}']]
            lanes.append(dict(brk=ln[0], r=ln[1], n_lo=tuple(ln[2:4]), n_hi=tuple(ln[4:6]), anchor=tuple(ln[6:8])))
        rate = tuple(tuple(float(e) for e in r) for r in kat[pre + 'rate']) if int(item(pre + 'has_rate')) else None
        agents.append(dict(model=str(item(pre + 'model')), vehicle=take('vehicle_'), cost=cost, rate=rate, lanes=lanes,
                           **{k: [float(e) for e in kat[pre + k]] for k in ('in_ub', 'in_lb', 'st_ub', 'st_lb')}, radius=float(item(pre + 'radius'))))
    return dict(M=int(item('p_M')), N=int(item('p_N')), dt=float(item('p_dt')), method=str(item('p_method')), substeps=int(item('p_substeps')),
                track=track, obstacle_rows=bool(item('p_obstacle_rows')), agents=agents)


# ---------------------------------------------------------------------------------------------
# games: the reference's config defaults + the literals of its scripts
# ---------------------------------------------------------------------------------------------
def reference_defaults(ref_dir):
    """Defaults of the reference's own config classes (model_types.py needs no casadi)."""
    os.environ.setdefault('MPLBACKEND', 'Agg')
    mine = [m for m in sys.modules if m == 'DGSQP' or m.startswith('DGSQP.')]
    saved = {m: sys.modules.pop(m) for m in mine}
    sys.path.insert(0, str(ref_dir))
    try:
        from DGSQP.dynamics.model_types import DynamicBicycleConfig, KinematicBicycleConfig, UnicycleConfig
        assert pathlib.Path(sys.modules['DGSQP.dynamics.model_types'].__file__).resolve().is_relative_to(pathlib.Path(ref_dir).resolve())
        cfgs = {'kin': KinematicBicycleConfig, 'dyn': DynamicBicycleConfig, 'uni': UnicycleConfig, 'pm': UnicycleConfig}
        return {kind: (lambda cls, keys: (lambda **over: {k: getattr(cls(**over), k) for k in keys}))(cfgs[kind], VEHICLE_KEYS[kind]) for kind in cfgs}
    finally:
        sys.path.remove(str(ref_dir))
        for m in [m for m in sys.modules if m == 'DGSQP' or m.startswith('DGSQP.')]:
            sys.modules.pop(m)
        sys.modules.update(saved)


def racing_cost(comp_weights=(10.0, 5.0), comp_type='atan', blocking_weight=0.0, obs_weight=0.0, obs_r=0.3):   # chicane.py:111-122
    return dict(kind='racing', input_weight=(1.0, 1.0), input_rate_weight=(1.0, 1.0), comp_weights=tuple(comp_weights), comp_type=comp_type,
                blocking_weight=blocking_weight, obs_weight=obs_weight, obs_r=obs_r)


def bicycle_agent(model, vehicle, cost, rate, radius, half_width=1.0):
    """Boxes of chicane.py:80-95 / exact_dynamic_game_dynamic.py:68-95: |u_a| <= 2.1, |u_steer| <= 0.436, |e_y| <= half width."""
    nq = NQ[model]
    st_ub, st_lb = [INF] * nq, [-INF] * nq
    st_ub[nq - 1], st_lb[nq - 1] = half_width, -half_width
    return dict(model=model, vehicle=vehicle, cost=cost, rate=rate, lanes=[], in_ub=(2.1, 0.436), in_lb=(-2.1, -0.436), st_ub=st_ub, st_lb=st_lb,
                radius=radius)


def kinematic_game(defaults, track, N, M=2, method='euler', substeps=1, steer_rate=4.5, radius=0.2, cost=racing_cost):
    """chicane.py / curve.py: vehicle :52-75, rate limits :92-93 (pi on the chicane, 4.5 on the curve track), radii :126-127."""
    veh = lambda: defaults['kin'](wheel_dist_front=0.13, wheel_dist_rear=0.13, drag_coefficient=0.1, slip_coefficient=0.1)
    rate = ((10.0, steer_rate), (-10.0, -steer_rate))
    return dict(M=M, N=N, dt=0.1, method=method, substeps=substeps, track=track, obstacle_rows=True,
                agents=[bicycle_agent('kin', veh(), cost(), rate, radius) for _ in range(M)])


def dynamic_game(defaults, N, method='rk4', substeps=10, **over):
    """comparison_study_barc/exact_dynamic_game_dynamic.py, cost_setting 0: vehicle :26-66, weights :100-105, linear competition term
    :146-147, no agent function rows :197-201, radii 0.23 (globals.py:12-13), on the curve track."""
    veh = lambda: defaults['dyn'](**{**dict(simple_slip=False, tire_model='pacejka', mass=2.2187, yaw_inertia=0.02723, wheel_friction=0.9,
                                            pacejka_b_front=5.0, pacejka_b_rear=5.0, pacejka_c_front=2.28, pacejka_c_rear=2.28), **over})
    return dict(M=2, N=N, dt=0.1, method=method, substeps=substeps, track=curve_track(), obstacle_rows=True,
                agents=[bicycle_agent('dyn', veh(), racing_cost((1.0, 5.0), 'linear'), None, 0.23) for _ in range(2)])


def point_mass_agent(vehicle, cost, rate, radius=0.21, half_width=1.0):
    """game_setup_unicycle.py:66-94: |Fx| <= 2, |wz| <= 2, |x_tran| <= half width - 0.1, no other state bound; radii :106-107."""
    st_ub, st_lb = [INF] * 6, [-INF] * 6
    st_ub[5], st_lb[5] = half_width - 0.1, -(half_width - 0.1)
    return dict(model='pm', vehicle=vehicle, cost=cost, rate=rate, lanes=[], in_ub=(2.0, 2.0), in_lb=(-2.0, -2.0), st_ub=st_ub, st_lb=st_lb,
                radius=radius)


def point_mass_cost(**over):            # game_setup_unicycle.py:99-104, :154-166: 1/2 0.1 |u|^2 per stage (no rate term), -1 s + 5 atan(ds) at the end
    return {**dict(kind='racing', input_weight=(0.1, 0.1), input_rate_weight=(0.0, 0.0), comp_weights=(1.0, 5.0), comp_type='atan',
                   blocking_weight=0.0, obs_weight=0.0, obs_r=0.3), **over}


def point_mass_game(defaults, track, N, M=2, method='euler', substeps=1, cost=point_mass_cost, rate=None, **vehicle):
    """game_setup_unicycle.py: vehicle :35-55 (drag, damping, rolling resistance 0), euler with dt 0.1 :21, :34, collision rows at stages
    1..N :246-252, no rate rows :213, :229 -- on a Monte-Carlo track of half width 1."""
    veh = lambda: defaults['pm'](**{**dict(damping_coefficient=0), **vehicle})
    return dict(M=M, N=N, dt=0.1, method=method, substeps=substeps, track=track, obstacle_rows=True,
                agents=[point_mass_agent(veh(), cost(), rate) for _ in range(M)])


def merge_game_spec(defaults, N, M=3):
    """DGSQP_merge_monte_carlo.py: lanes :40-74, goals :85-87, rk3 with one substep :90-123, boxes :126-159, radii 0.1 :162-164,
    costs :253-303."""
    lw, mw, mpos, th, r = 0.3, 0.3, 1.5, np.pi / 12, 0.1
    ns, nm = (0.0, 1.0), (-np.sin(th), np.cos(th))
    x1, x3 = (0.0, lw), (0.0, 0.0)
    x6 = (mpos + lw / np.tan(th), lw)
    x7 = (mpos + mw / np.sin(th), 0.0)
    neg = lambda v: (-v[0], -v[1])
    lane = lambda n_lo, anchor, n_hi=None, brk=INF: dict(brk=brk, r=r, n_lo=n_lo, n_hi=n_lo if n_hi is None else n_hi, anchor=anchor)
    straight = lambda: [lane(ns, x1), lane(neg(ns), x3)]           # -ns^T (p - (x3 + r ns)) = n^T (p - (x3 - r n)), n = -ns
    ramp = lambda: [lane(nm, x6, ns, x6[0]), lane(neg(nm), x7, neg(ns), x7[0])]
    goal_x = (4.0, 4.5, 4.25)
    agents = []
    for i in range(M):
        cost = dict(kind='goal', input_weight=(0.1, 0.1), input_rate_weight=(0.0, 0.0), state_weight=(1.0, 10.0, 1.0, 1.0),
                    goal=(goal_x[i], 0.15, 0.3, 0.0), terminal_multiplier=10.0)
        agents.append(dict(model='uni', vehicle=defaults['uni'](), cost=cost, rate=None, lanes=ramp() if i == 2 else straight(),
                           in_ub=(2.0, 4.5), in_lb=(-2.0, -4.5), st_ub=[INF, INF, 2.0, INF], st_lb=[-INF, -INF, -2.0, -INF], radius=0.1))
    return dict(M=M, N=N, dt=0.1, method='rk3', substeps=1, track=None, obstacle_rows=True, agents=agents)


def one_stage_spec(kind, method, substeps, vehicle):
    """The N = 1 two-car race of tests/conftest.py::sympy_one_stage_game: the vehicle of tests/golden/sympy_fd_<kind>.npz on the
    curve track, the racing cost of chicane.py:223-277, rate rows, the obstacle row with radii 0.2."""
    rate = ((10.0, 4.5), (-10.0, -4.5))
    return dict(M=2, N=1, dt=0.1, method=method, substeps=substeps, track=curve_track(), obstacle_rows=True,
                agents=[bicycle_agent(kind, dict(vehicle), racing_cost(), rate, 0.2) for _ in range(2)])


def one_stage_answers(kind, method, kat, k1, k2, l_obs=0.7):
    """x_1 and Q of the one-stage game at points k1, k2 of the sympy file: the tie of this generator to the symbolic pin."""
    vehicle = {k: kat['param_' + k].item() for k in VEHICLE_KEYS[kind] if 'param_' + k in kat.files}
    if kind == 'dyn':
        vehicle.setdefault('linear_bf', 1.0); vehicle.setdefault('linear_br', 1.0)
    spec = one_stage_spec(kind, method, int(kat[f'{method}_M']), vehicle)
    nqa = NQ[kind]
    pts = kat['points']
    x0 = np.concatenate([pts[k1][:nqa], pts[k2][:nqa]])
    u = np.concatenate([pts[k1][nqa:], pts[k2][nqa:]])
    l = np.zeros(8 + 8 + 1 + 4)                   # k = 0: 2 x (4 rate + 4 input box); k = 1: the obstacle row, 2 x 2 state box
    l[16] = l_obs
    out, margin = answers(spec, x0, u, l, 60, 20)
    assert margin[0] > MARGIN, margin
    return {k: v[0] for k, v in out.items()}


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def agent_major(u_tm, M):
    B = u_tm.shape[0]
    return np.concatenate([u_tm[:, :, 2 * a:2 * a + 2].reshape(B, -1) for a in range(M)], axis=1)


def draw(case, game, B, seed, n_c):
    """x0 and the warm start from the package's sampler, u = warm start + 0.05 N(0, 1), l = max(0, N(0, 1)) on ALL rows."""
    from dgsqp_amd.montecarlo import sample_scenarios
    x0, u_tm = sample_scenarios(game, B, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    u = agent_major(u_tm, game.joint_model.n_a) + 0.05 * rng.standard_normal((B, u_tm.shape[1] * u_tm.shape[2]))
    l = np.maximum(0, rng.standard_normal((B, n_c)))
    return x0.copy(), u, l


def n_rows(spec):
    z = [[[mp.mpf(0)] * NQ[ag['model']] for _ in range(spec['N'] + 1)] for ag in spec['agents']]
    return len(rows(spec, z, [[[mp.mpf(0)] * 2] * spec['N']] * spec['M'], Margin()))


def slow_branch_points(x0, seg1, before=0.04):
    """tests/test_split_rollout.py::_slow_branch_points 0-2 (q = [x, y, vx, vy, w, e_psi, s, e_y] per car): a car sliding sideways, a
    car across the track, a car ``before`` the first segment boundary (not the 5 cm of that test: at 1.5 m/s a substep of dt / 3 covers 5 cm and
    would put an integrator stage ON the boundary; chosen per integrator to fall between its stages)."""
    x0[0, 2:5] = (1.5, 0.8, 0.0)
    x0[1, 8 + 5] = 0.9
    x0[2, 2], x0[2, 6] = 1.5, seg1 - before
    return x0


def case_inputs(case, defaults, shift=0):
    """(spec, x0, u, l, directions, checks, u_prev [B, n_u] or None) of a case; ``checks(x)`` asserts what the points are there for, on the generator's own
    trajectory x [B, N + 1, n_q].  ``shift`` is added to the sampler's seed (main takes the first that keeps the margin)."""
    sys.path.insert(0, str(ROOT / 'tests'))
    sys.path.insert(0, str(ROOT))
    import multistage_kat as mk
    import point_mass_kat as pk
    if case.endswith(UPREV):
        # the parent's game and scenarios, and a u_prev per scenario drawn inside the input box (its inner 90 %)
        spec, x0, u, l, vs, checks, _ = case_inputs(case[:-len(UPREV)], defaults, shift)
        rng = np.random.default_rng(4242 + sum(map(ord, case)))
        lb, ub = (np.concatenate([np.asarray(ag[k], float) for ag in spec['agents']]) for k in ('in_lb', 'in_ub'))
        assert np.isfinite(lb).all() and np.isfinite(ub).all(), 'a *_uprev case needs a finite input box'
        mid, half = 0.5 * (lb + ub), 0.45 * (ub - lb)
        return spec, x0, u, l, vs, checks, mid + half * rng.uniform(-1.0, 1.0, (len(x0), len(lb)))
    game = (pk if case in pk.CASES else mk).build_game(case)
    vs, checks = (), (lambda x: None)
    if case == 'kin2_euler_N3':
        spec = kinematic_game(defaults, curve_track(), 3)
        x0, u, l = draw(case, game, 3, 11 + 100 * shift, n_rows(spec))
        x0[0, 4] = 0.9                                        # car 1 crosses the segment boundary s = 1 between stages 0 and 1

        def checks(x):
            assert x[0, 0, 4] < 1.0 < x[0, 1, 4], x[0, :2, 4]
    elif case == 'kin2_rk4_N4':
        cost = lambda: racing_cost((10.0, 5.0), 'linear', blocking_weight=0.7, obs_weight=3.0, obs_r=0.9)
        spec = kinematic_game(defaults, chicane_track(), 4, method='rk4', substeps=2, steer_rate=np.pi, radius=0.4, cost=cost)
        x0, u, l = draw(case, game, 3, 12 + 100 * shift, n_rows(spec))
        x0[1, 4] += 4.6; x0[1, 6 + 4] += 4.6                  # scenario 1: out of curve 1 (c < 0) over the mid straight ...
        x0[2, 4] += 5.4; x0[2, 6 + 4] += 5.4                  # scenario 2: ... into curve 2 (c > 0)

        def checks(x):
            tr = spec['track']
            curv = lambda s: tr['seg_curv'][np.searchsorted(tr['seg_s'], s, side='right') - 1]
            cs = curv(x[:, :, [4, 10]])
            assert (cs < 0).any() and (cs > 0).any() and (cs == 0).any(), cs
            d = np.linalg.norm(x[:, :, 0:2] - x[:, :, 6:8], axis=2)
            assert (d < 1.8 - MARGIN).all(), d               # the hinge of the soft-obstacle cost is active
    elif case == 'kin3_euler_N3':
        spec = kinematic_game(defaults, curve_track(), 3, M=3)
        x0, u, l = draw(case, game, 2, 13 + 100 * shift, n_rows(spec))
    elif case in ('dyn2_rk4m3_N3', 'dyn2_rk4m10_N2', 'dyn2_rk3_N3', 'dyn2_rk2_lin_N3'):
        N = 2 if case == 'dyn2_rk4m10_N2' else 3
        if case == 'dyn2_rk3_N3':
            spec = dynamic_game(defaults, N, 'rk3', 4)       # (4 substeps as tests/test_split_rollout.py: with 2 the Pacejka model's rk3 step amplifies a 2^-53 perturbation to 3e-14)
        elif case == 'dyn2_rk2_lin_N3':
            spec = dynamic_game(defaults, N, 'rk2', 2, tire_model='linear', simple_slip=True, drive_wheels='rear')
        else:
            spec = dynamic_game(defaults, N, 'rk4', 10 if case == 'dyn2_rk4m10_N2' else 3)
        x0, u, l = draw(case, game, 3, 14 + 100 * shift, n_rows(spec))
        x0 = slow_branch_points(x0, spec['track']['seg_s'][1], {'dyn2_rk4m3_N3': 0.04, 'dyn2_rk4m10_N2': 0.034}.get(case, 0.055))

        def checks(x):
            L_r = spec['agents'][0]['vehicle']['wheel_dist_rear']
            slip = np.abs(np.arctan2(x[0, :, 3] - x[0, :, 4] * L_r, x[0, :, 2])).max()
            assert slip > np.arctan(7.0 / 16.0), slip
            assert np.abs(x[1, :, 8 + 5]).max() > 0.78
            assert x[2, 0, 6] < spec['track']['seg_s'][1] < x[2, 1, 6], x[2, :2, 6]
    elif case == 'uni3_merge_N3':
        spec = merge_game_spec(defaults, 3)
        x0, u, l = draw(case, game, 3, 15 + 100 * shift, n_rows(spec))
        brk = [ln['brk'] for ln in spec['agents'][2]['lanes']]
        x0[1, 8], x0[1, 11] = 0.5 * (brk[0] + brk[1]), np.pi / 2     # the ramp car between the two lane normals' breakpoints (4 cm apart: heading
        x0[2, 8] = brk[1] + 0.2                                      # along y, so that it stays there) and past both (scenario 0: before both)

        def checks(x):
            px = x[:, :, 8]
            assert (px[0] < brk[0]).all() and ((px[1] > brk[0]) & (px[1] < brk[1])).all() and (px[2] > brk[1]).all(), px
    elif case in ('kin3_N20_dir', 'kin3_N25_dir'):
        N = {'kin3_N20_dir': 20, 'kin3_N25_dir': 25}[case]
        spec = kinematic_game(defaults, curve_track(), N, M=3)
        x0, u, l = draw(case, game, 2, 16 + 100 * shift, n_rows(spec))
        vs = tuple(np.random.default_rng(99).standard_normal((2, 2 * 3 * N)))
    elif case == 'pm2_euler_N3':
        spec = point_mass_game(defaults, curve_track(), 3)
        x0, u, l = draw(case, game, 3, 21 + 100 * shift, n_rows(spec))
        x0[0, 4] = 0.9                                        # car 1 crosses the segment boundary s = 1 between stages 0 and 1

        def checks(x):
            assert x[0, 0, 4] < 1.0 < x[0, 1, 4], x[0, :2, 4]
    elif case == 'pm2_rk4_N4':
        cost = lambda: point_mass_cost(input_rate_weight=(0.3, 0.2), comp_type='linear', blocking_weight=0.7, obs_weight=3.0, obs_r=0.9)
        spec = point_mass_game(defaults, chicane_track(), 4, method='rk4', substeps=2, cost=cost, rate=((10.0, 4.5), (-10.0, -4.5)),
                               damping_coefficient=0.3, mass=1.9)
        x0, u, l = draw(case, game, 3, 22 + 100 * shift, n_rows(spec))
        x0[1, 4] += 4.6; x0[1, 6 + 4] += 4.6                  # scenario 1: out of curve 1 (c < 0) over the mid straight ...
        x0[2, 4] += 5.4; x0[2, 6 + 4] += 5.4                  # scenario 2: ... into curve 2 (c > 0)

        def checks(x):
            tr = spec['track']
            curv = lambda s: tr['seg_curv'][np.searchsorted(tr['seg_s'], s, side='right') - 1]
            cs = curv(x[:, :, [4, 10]])
            assert (cs < 0).any() and (cs > 0).any() and (cs == 0).any(), cs
            d = np.linalg.norm(x[:, :, 0:2] - x[:, :, 6:8], axis=2)
            assert (d < 1.8 - MARGIN).all(), d               # the hinge of the soft-obstacle cost is active
    elif case == 'mix3_rk4m3_N3':
        # agents (kinematic bicycle, point mass, dynamic bicycle), each with its own game's vehicle, boxes and cost, radii 0.2, on the curve track
        kin = kinematic_game(defaults, curve_track(), 3, M=1)['agents'][0]
        pm = point_mass_agent(defaults['pm'](damping_coefficient=0.2), point_mass_cost(), None, radius=0.2)
        dyn = dynamic_game(defaults, 3)['agents'][0]
        dyn['radius'] = 0.2
        spec = dict(M=3, N=3, dt=0.1, method='rk4', substeps=3, track=curve_track(), obstacle_rows=True, agents=[kin, pm, dyn])
        x0, u, l = draw(case, game, 2, 23 + 100 * shift, n_rows(spec))
    elif case in ('pm3_N20_dir', 'pm3_N25_dir'):
        N = {'pm3_N20_dir': 20, 'pm3_N25_dir': 25}[case]
        spec = point_mass_game(defaults, curve_track(), N, M=3)
        x0, u, l = draw(case, game, 2, 24 + 100 * shift, n_rows(spec))
        vs = tuple(np.random.default_rng(98).standard_normal((2, 2 * 3 * N)))
    else:
        raise ValueError(case)
    return spec, x0, u, l, vs, checks, None


# digits of the first pass where 60 are too few: the merge game's L^a is ~1e3 x the largest entry of its Q (goal costs of ~100 against
# input weights of 0.1), and 1e-60 |L| / 4 h^2 leaves Q at 2e-18 of its largest entry -- above the 1e-18 this tool accepts
DIGITS = {'uni3_merge_N3': 70}
UPREV = '_uprev'      # <parent>_uprev: the parent's scenarios with a non-zero input before stage 0, stored as ``u_prev``
CASES = ('kin2_euler_N3', 'kin2_rk4_N4', 'kin3_euler_N3', 'dyn2_rk4m3_N3', 'dyn2_rk4m10_N2', 'dyn2_rk3_N3', 'dyn2_rk2_lin_N3', 'uni3_merge_N3',
         'kin3_N20_dir', 'kin3_N25_dir', 'kin2_rk4_N4' + UPREV, 'dyn2_rk4m3_N3' + UPREV,
         'pm2_euler_N3', 'pm2_rk4_N4', 'mix3_rk4m3_N3', 'pm3_N20_dir', 'pm3_N25_dir')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference', help='the reference tree (for the defaults of DGSQP/dynamics/model_types.py)')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('cases', nargs='*', default=list(CASES))
    args = ap.parse_args()
    defaults = reference_defaults(args.reference)
    with ProcessPoolExecutor(args.jobs) as pool:
        for case in args.cases:
            t = time.time()
            for shift in range(50):                            # the first seed whose points keep the margin (nominal rollout, 30 digits)
                spec, x0, u, l, vs, checks, up = case_inputs(case, defaults, shift)
                mp.mp.dps = 30
                gms = [GameMP(spec, x0[b], u[b], l[b], mp.mpf(0), up=None if up is None else up[b]) for b in range(len(x0))]
                if all(gm.at() and gm.mg.m > 1.1 * MARGIN for gm in gms):
                    break
                print(f'{case}: seed shift {shift} comes within {min(gm.mg.m for gm in gms):.2e} of a breakpoint, next', flush=True)
            else:
                raise SystemExit(f'{case}: no seed keeps the margin')
            full = not vs
            out, acc, sens, margin = solve_case(spec, x0, u, l, vs, full, pool, dps=DIGITS.get(case, 60), up=up)
            assert margin[0] > MARGIN, f'{case}: a state comes within {margin[0]:.2e} of a breakpoint ({margin[1]})'
            checks(out['x'].reshape(len(x0), spec['N'] + 1, -1))
            worst = max(acc.values())
            print(f'{case}: B {len(x0)}, n {u.shape[1]}, rows {l.shape[1]}, {time.time() - t:.1f} s, breakpoint margin {margin[0]:.3g} ({margin[1]}), '
                  f'accuracy record {worst:.1e}; sensitivity ' + ', '.join(f'{k} {v:.1e}' for k, v in sens.items())
                  + (f'; max |Q - Q^T| {np.abs(out["Q"] - out["Q"].transpose(0, 2, 1)).max():.2e}' if full else ''), flush=True)
            if worst > 1e-18:
                raise SystemExit(f'{case}: the 60- and the 90-digit answers disagree by {worst:.1e} > 1e-18, not written')
            data = dict(flatten_spec(spec), x0=x0, u=u, l=l, margin=margin[0], **out)
            if vs:
                data['v'] = np.array(vs)
            if up is not None:
                data['u_prev'] = up
            data.update({'acc_' + k: v for k, v in acc.items()})
            data.update({'sens_' + k: v for k, v in sens.items()})
            np.savez_compressed(GOLD / f'multistage_{case}.npz', **data)


if __name__ == '__main__':
    main()
