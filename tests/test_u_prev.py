"""The input before stage 0 on the device: solve_batch / evaluate_batch / qp_batch / solve_batches (..., u_prev=...), dgsqp_set_u_prev, and
the carry of closed-loop launches, step_batch(..., u_prev=...) / dgsqp_set_closed_loop_u_prev / dgsqp_fetch_u_prev.

No oracle: the oracle has no u_prev.  What stands in for it:

* OFF IS OFF: zeros and none give the same bits.
* THE DELTAS: with p = u_prev, ``evaluate_batch(u_prev=p)`` against ``evaluate_batch()`` on the same device -- x, G, Q and everything of g and q
  outside stage 0's rate terms bit for bit; the k = 0 rate rows by -/+ p_j to 1e-14 max(1, |u|_inf, |p|_inf) (four roundings of O(1)
  quantities); the stage-0 columns of q by -w_rate[j] p_j to 1e-12 max(1, |q|_inf); the cost by 1/2 w_rate ((u_0 - p)^2 - u_0^2) to
  1e-12 max(1, |J|).  The cost is read from a solver whose tolerances are 1e30: its solve ends at its first convergence test with
  u = u_ws and reports f_J there.  And the two exact fixtures tests/golden/multistage_*_uprev.npz at the device bar already in force.
* TEACHER FORCING with the recorded u_prev[t]: every step of every chain is bit for bit the solve_batch from (q[t], u_ws[t], u_prev[t]),
  and u_prev[t + 1] is bit for bit ``closed_loop.next_u_prev`` of the recorded u_applied[t] / u_cmd[t]."""
import ctypes

import numpy as np
import pytest

import multistage_kat as mk
from closed_loop_checks import (CHAIN, COUNTS, DELAYS, DOUBLES, check_chain, check_feedback, same, scenarios,
                                 solver_of)      # noqa: F401  (solver_of is a fixture)

pytestmark = pytest.mark.gpu

KEYS = DOUBLES + COUNTS


def xl_game():
    from dgsqp_amd import montecarlo as mc
    return mc.kinematic_racing_game('curve', N=25, M=3)          # kb_curve3_N25: n = 150, the XL layout


@pytest.fixture(scope='module')
def three(games, solver_of):
    """name -> (game, solver, layout) of the games of items 1 and 2: the kinematic chicane with rate rows (n = 60) and configs[1]'s game
    (n = 100, rate cost only), both LDS-resident; kb_curve3_N25 on the XL layout; and, for the big layout, the three-car N = 20 game of
    tests/multistage_kat.py (n = 120)."""
    from dgsqp_amd.solver import DGSQP
    gx, gb = xl_game(), mk.build_game('kin3_N20_dir')
    out = {'kb_chicane_N15': (games['kb_chicane_N15'][0], solver_of('kb_chicane_N15'), 0),
           'dyn_curve_N25': (games['dyn_curve_N25'][0], solver_of('dyn_curve_N25'), 0),
           'kb_curve3_N20': (gb, DGSQP(*gb.solver_args(), print_method=None), 1),
           'kb_curve3_N25': (gx, DGSQP(*gx.solver_args(), print_method=None), 2)}
    for name, (g, s, layout) in out.items():
        assert s.dims.layout == layout, (name, s.dims.layout)
    assert out['kb_chicane_N15'][1].n == 60
    yield out
    out.clear()


def box(s):
    P = s._problem
    lb = np.array([P.agents[a].in_lb[j] for a in range(s.M) for j in range(2)])
    ub = np.array([P.agents[a].in_ub[j] for a in range(s.M) for j in range(2)])
    return lb, ub


def draw_u_prev(s, B, seed):
    """[B, n_u] inside the inner 90 % of the input box."""
    lb, ub = box(s)
    return 0.5 * (lb + ub) + 0.45 * (ub - lb) * np.random.default_rng(seed).uniform(-1.0, 1.0, (B, s.n_u))


def stage0_layout(s):
    """(columns [M, 2] of stage 0, w_rate [M, 2], rate rows [M, 2, 2] (ub, lb; -1: the agent has none)) of the solver's game: row order
    DGSQP.py:730-821 -- at k = 0 no shared rows; per agent the rate rows (ub, lb per channel), the lane rows, input ub, input lb."""
    P = s._problem
    cols = np.array([[2 * s.N * a + j for j in range(2)] for a in range(s.M)])
    w = np.array([[P.agents[a].w_rate[j] for j in range(2)] for a in range(s.M)])
    rate = -np.ones((s.M, 2, 2), int)
    r = 0
    for a in range(s.M):
        A = P.agents[a]
        if A.has_rate:
            for j in range(2):
                rate[a, j] = (r, r + 1)
                r += 2
        r += A.n_lane + sum(A.in_ub[j] < np.inf for j in range(2)) + sum(A.in_lb[j] > -np.inf for j in range(2))
    return cols, w, rate


def check_deltas(s, x0, u_am, l, p, tag):
    """Item 2's delta check of evaluate_batch(u_prev=p) against evaluate_batch() on solver ``s``; returns the two evaluations."""
    ev0, evp = s.evaluate_batch(x0, u_am, l), s.evaluate_batch(x0, u_am, l, u_prev=p)
    cols, w, rate = stage0_layout(s)
    for k in ('x', 'G', 'Q'):
        assert same(ev0[k], evp[k]), (tag, k)
    tg, tq = np.zeros(s.n_c_total, bool), np.zeros(s.n, bool)
    tg[rate[rate >= 0]] = True
    tq[cols.ravel()] = True
    assert same(ev0['g'][:, ~tg], evp['g'][:, ~tg]) and same(ev0['q'][:, ~tq], evp['q'][:, ~tq]), tag
    worst_g = worst_q = 0.0
    for b in range(len(x0)):
        pb = p[b].reshape(s.M, 2)
        bar_g = 1e-14 * max(1.0, np.abs(u_am[b]).max(), np.abs(p[b]).max())
        bar_q = 1e-12 * max(1.0, np.abs(ev0['q'][b]).max())
        for a in range(s.M):
            for j in range(2):
                dq = (evp['q'][b, cols[a, j]] - ev0['q'][b, cols[a, j]]) - (-w[a, j] * pb[a, j])
                worst_q = max(worst_q, abs(dq) / bar_q)
                if rate[a, j, 0] >= 0:
                    d_ub = (evp['g'][b, rate[a, j, 0]] - ev0['g'][b, rate[a, j, 0]]) + pb[a, j]
                    d_lb = (evp['g'][b, rate[a, j, 1]] - ev0['g'][b, rate[a, j, 1]]) - pb[a, j]
                    worst_g = max(worst_g, abs(d_ub) / bar_g, abs(d_lb) / bar_g)
    print(f'{tag}: k = 0 rate rows off -/+ p by {worst_g:.2e} x their bar (1e-14 max(1, |u|, |p|)), stage-0 q columns off -w_rate p by {worst_q:.2e} x '
          f'theirs (1e-12 max(1, |q|))')
    assert worst_g <= 1.0 and worst_q <= 1.0, (tag, worst_g, worst_q)
    return ev0, evp


def loose(g, **kw):
    """A solver of game ``g`` whose solve ends at its first convergence test: u = u_ws, cost = f_J(u_ws) (tolerances 1e30)."""
    import copy
    from dgsqp_amd.solver import DGSQP
    g2 = copy.copy(g)
    g2.params = copy.copy(g.params)
    g2.params.p_tol = g2.params.d_tol = 1e30
    return DGSQP(*g2.solver_args(), print_method=None, **kw)


def check_cost_delta(s_loose, x0, u_tm, p, tag):
    s = s_loose
    a0, ap = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm, u_prev=p)
    u_am = s._to_agent_major(np.asarray(u_tm, float))
    assert same(a0['u'], u_am) and same(ap['u'], u_am) and (a0['num_iters'] == 0).all(), tag     # nothing moved: the cost is f_J(u_ws)
    P = s._problem
    worst = 0.0
    for b in range(len(x0)):
        for a in range(s.M):
            u0 = u_am[b, 2 * s.N * a:2 * s.N * a + 2]
            want = sum(0.5 * P.agents[a].w_rate[j] * ((u0[j] - p[b, 2 * a + j]) ** 2 - u0[j] ** 2) for j in range(2))
            worst = max(worst, abs((ap['cost'][b, a] - a0['cost'][b, a]) - want) / (1e-12 * max(1.0, abs(a0['cost'][b, a]))))
    print(f'{tag}: cost off 1/2 w_rate ((u_0 - p)^2 - u_0^2) by {worst:.2e} x its bar (1e-12 max(1, |J|))')
    assert worst <= 1.0, (tag, worst)
    assert not same(ap['cost'], a0['cost'])


# ---- 1. off is off ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,qp_method', [('kb_chicane_N15', None), ('kb_chicane_N15', 'osqp'), ('dyn_curve_N25', None), ('kb_curve3_N20', None), ('kb_curve3_N25', None)])
def test_zero_u_prev_is_no_u_prev(three, solver_of, name, qp_method):
    g, s, _ = three[name]
    if qp_method:
        s = solver_of(name, qp_method=qp_method)
    B = 4 if name == 'kb_chicane_N15' else 2
    x0, u_tm = scenarios(g, B, 3)
    a = s.solve_batch(x0, u_tm)
    z = np.zeros((B, s.n_u))
    b = s.solve_batch(x0, u_tm, u_prev=z)
    c = s.solve_batch(x0, u_tm)                                  # ... and the setting is gone afterwards
    for key in KEYS:
        assert same(a[key], b[key]) and same(a[key], c[key]), (name, qp_method, key)
    assert (a['num_iters'] > 0).all()


def test_step_batch_without_u_prev_is_the_launch_it_was(games, solver_of):
    from dgsqp_amd import _ffi
    g, s = games['kb_chicane_N15'][0], solver_of('kb_chicane_N15')
    x0, u_tm = scenarios(g, 4, 7)
    plain = s.step_batch(x0, u_tm, 3, keep_predictions=True)
    assert 'u_prev' not in plain
    # the raw setting: mode 0 with an all-zero u_prev0 is off
    z = np.zeros((4, s.n_u))
    assert s._lib.dgsqp_set_closed_loop_u_prev(s._h, 0, 4, _ffi.dptr(z)) == 0
    off = s.step_batch(x0, u_tm, 3, keep_predictions=True)
    # one step with carry from zeros: there is nothing to carry yet
    one = s.step_batch(x0, u_tm, 1, keep_predictions=True, u_prev=z)
    for key in CHAIN:
        if key in plain:
            assert same(plain[key], off[key]), key
    for key in KEYS:
        assert same(one[key][:, 0], plain[key][:, 0]), key
    assert same(one['u_prev'], np.zeros((4, 1, s.n_u)))


# ---- 2. stage quantities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parent', ['kin2_rk4_N4', 'dyn2_rk4m3_N3'])
def test_evaluate_with_u_prev_against_the_exact_fixtures(parent):
    from dgsqp_amd.solver import DGSQP, build_problem
    kat = np.load(mk.GOLD / f'multistage_{parent}_uprev.npz')
    g = mk.build_game(parent)
    mk.assert_same_parameters(kat, build_problem(*g.solver_args()))
    for k in kat.files:
        if k.startswith('acc_'):
            assert kat[k] <= 1e-18, (k, float(kat[k]))
    assert kat['margin'] > 1e-3
    s = DGSQP(*g.solver_args(), print_method=None)
    assert (s.n, s.n_c_total) == (kat['u'].shape[1], kat['l'].shape[1]) and kat['u_prev'].shape == (len(kat['x0']), s.n_u)
    ev = s.evaluate_batch(kat['x0'], kat['u'], kat['l'], u_prev=kat['u_prev'])
    for b in range(len(kat['x0'])):
        mk.compare(kat, b, {key: ev[key][b] for key in ('x', 'g', 'q', 'G', 'Q')}, mk.DEVICE_BAR, f'{parent}_uprev device')
    ev0 = s.evaluate_batch(kat['x0'], kat['u'], kat['l'])
    assert not same(ev0['q'], ev['q'])                           # (the fixture is not met without its u_prev)
    par = np.load(mk.GOLD / f'multistage_{parent}.npz')
    for b in range(len(kat['x0'])):
        mk.compare(par, b, {key: ev0[key][b] for key in ('x', 'g', 'q', 'G', 'Q')}, mk.DEVICE_BAR, f'{parent} device, after a call with u_prev')


@pytest.mark.parametrize('name', ['kb_chicane_N15', 'dyn_curve_N25', 'kb_curve3_N20', 'kb_curve3_N25'])
def test_u_prev_changes_the_stage_0_rate_terms_and_nothing_else(three, name):
    g, s, _ = three[name]
    B = 3
    x0, u_tm = scenarios(g, B, 5)
    rng = np.random.default_rng(17)
    u_am = s._to_agent_major(np.asarray(u_tm, float)) + 0.05 * rng.standard_normal((B, s.n))
    l = np.maximum(0.0, rng.standard_normal((B, s.n_c_total)))
    p = draw_u_prev(s, B, 19)
    check_deltas(s, x0, u_am, l, p, name)
    check_cost_delta(loose(g), x0, s._to_time_major(u_am), p, name)


# ---- 3. the limit binds -------------------------------------------------------------------------------------------------------------------
def test_the_rate_limit_against_u_prev_binds(games, solver_of):
    g, s = games['kb_chicane_N15'][0], solver_of('kb_chicane_N15')
    P, par = s._problem, s._cparams
    x0, u_tm = scenarios(g, 8, 3)
    base = s.solve_batch(x0, u_tm)
    lb, ub = box(s)
    lim = P.dt * P.agents[0].rate_ub[0]                          # channel 0 (acceleration) of agent 0: 1.0 per step, box +-2.1
    u0 = base['u'][:, 0]
    ok = base['converged'] & (u0 - 3 * lim > lb[0] + 1e-3) & (u0 < lim - 0.01)      # p inside the box; the limit not active against 0
    assert ok.any(), (base['status'], u0)
    b = int(np.nonzero(ok)[0][0])
    p = np.zeros((1, s.n_u))
    p[0, 0] = u0[b] - 3 * lim
    res = s.solve_batch(x0[b:b + 1], u_tm[b:b + 1], u_prev=p)
    ev0 = s.evaluate_batch(x0[b:b + 1], res['u'], res['l'])
    ev = s.evaluate_batch(x0[b:b + 1], res['u'], res['l'], u_prev=p)
    row = int(np.nonzero(ev['g'][0] - ev0['g'][0] > 0.5 * abs(p[0, 0]))[0][0])        # the ub row: g = u_0 - p - dt rate, and p < 0
    step = res['u'][0, 0] - p[0, 0]
    print(f'scenario {b}: u_0* = {u0[b]:.4f} against 0, p = {p[0, 0]:.4f}; with p: status {res["msg"][0]}, {res["num_iters"][0]} iterations, u_0 = {res["u"][0, 0]:.4f}, '
          f'u_0 - p = {step:.6f} (limit {lim}), multiplier {res["l"][0, row]:.4f}, cond {res["cond"][0]}')
    assert res['converged'][0], res['msg']
    assert step <= lim + par.p_tol and res['l'][0, row] > 0.0
    assert abs(ev['g'][0, row] - (step - lim)) < 1e-14 * max(1.0, abs(p[0, 0]))
    assert abs(res['u'][0, 0] - u0[b]) > 1.0                     # ... which the answer against 0 (3 limits away) does not meet
    d = ev['q'][0] + ev['G'][0].T @ res['l'][0]
    cond = np.array([max(0.0, ev['g'][0].max()), np.abs(ev['g'][0] * res['l'][0]).max(), np.abs(d).max()])
    print(f'cond from evaluate_batch(u*, l*, u_prev=p): {cond}, returned {res["cond"][0]}')
    assert cond[0] < par.p_tol and cond[1] < par.d_tol and cond[2] < par.d_tol
    assert np.abs(cond - res['cond'][0]).max() < 1e-9            # the same three maxima, summed in another order


# ---- 4. helpers, deferral, groups, v2, f32, the 256-thread build --------------------------------------------------------------------------
def test_cooperative_helpers_see_the_scenarios_u_prev(games):
    from dgsqp_amd.solver import DGSQP
    g = games['dyn_curve_N25'][0]
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = scenarios(g, 8, 5)
    p = draw_u_prev(s, 8, 23)
    s.set_cooperative(0)
    ref = s.solve_batch(x0, u_tm, u_prev=p)
    s.set_cooperative(2)
    res = s.solve_batch(x0, u_tm, u_prev=p)
    st = s.coop_stats()
    print('cooperative launch of 8 scenarios with u_prev:', st, 'iterations', ref['num_iters'])
    for key in KEYS:
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    assert st['finished'] == 8 and st['helper_registrations'] > 0


def test_deferred_scenarios_resume_with_their_u_prev(games):
    """B = 600 of the n = 60 game, deferral on against off.  Measured: at that size nothing is set aside -- two workgroups of this game fit a
    CU, the grid is 512, and the 88 tickets behind it are gone before any scenario has run long (0 deferred at both settings) --, so one
    more pair of solves runs at B = 1,536, the size test_deferral_of_long_scenarios_is_bit_identical uses for this game family, where
    scenarios are set aside and resumed (385 of them; 0.17 s a solve): without it nothing here would pass through dev_park_load."""
    from dgsqp_amd.solver import DGSQP
    g = games['kb_chicane_N15'][0]
    s = DGSQP(*g.solver_args(), print_method=None)
    deferred = 0
    for B in (600, 1536):
        x0, u_tm = scenarios(g, B, 11)
        p = draw_u_prev(s, B, 29)
        s.set_cooperative(0)
        ref = s.solve_batch(x0, u_tm, u_prev=p)
        s.set_cooperative(1)
        for min_it, factor in ((4, 0.5), (1, 0.25)) if B == 600 else ((4, 0.5),):
            s.set_deferral(min_it, factor)
            res = s.solve_batch(x0, u_tm, u_prev=p)
            st = s.deferral_stats()
            print(f'deferral {(min_it, factor)} with u_prev, B = {B}:', st, 'kernel ms', ref['kernel_ms'], res['kernel_ms'], 'iterations mean / max', ref['num_iters'].mean(), ref['num_iters'].max())
            for key in KEYS:
                assert np.array_equal(res[key], ref[key], equal_nan=True), (B, min_it, factor, key)
            assert st['deferred'] == st['resumed']
            deferred += st['deferred']
        s.set_deferral(8, 2.0)
        zero = s.solve_batch(x0[:8], u_tm[:8])
        assert not same(zero['u'], ref['u'][:8])
    assert deferred > 0


def test_grouped_batches_keep_their_own_u_prev(games):
    from dgsqp_amd.solver import DGSQP, solve_batches
    g = games['kb_chicane_N15'][0]
    solvers = [DGSQP(*g.solver_args(), print_method=None) for _ in range(2)]
    batches = [scenarios(g, 6, 31 + i) for i in range(2)]
    ps = [draw_u_prev(solvers[0], 6, 37 + i) for i in range(2)]
    ref = [s.solve_batch(x0, u, u_prev=p) for s, (x0, u), p in zip(solvers, batches, ps)]
    res = solve_batches(solvers, [(x0, u, p) for (x0, u), p in zip(batches, ps)])
    mixed = solve_batches(solvers, [(batches[0][0], batches[0][1], ps[0]), batches[1]])      # a triple next to a pair
    plain = solvers[1].solve_batch(*batches[1])
    for key in KEYS:
        for i in range(2):
            assert np.array_equal(res[i][key], ref[i][key], equal_nan=True), (i, key)
        assert np.array_equal(mixed[0][key], ref[0][key], equal_nan=True) and np.array_equal(mixed[1][key], plain[key], equal_nan=True), key
    assert not same(plain['u'], ref[1]['u'])


def test_v2_reads_u_prev():
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver_types import DGSQPV2Params
    from dgsqp_amd.solver_v2 import DGSQP as DGSQPV2
    worst = {}
    for merit in ('stat_l1', 'sum_obj_l1'):
        g = mc.kinematic_racing_game('curve', N=12)
        g.params = DGSQPV2Params(dt=0.1, N=12, merit_function=merit, sqp_iters=8)
        g.params.time_limit = None
        s = DGSQPV2(*g.solver_args(), print_method=None)
        assert s._cparams.variant == 1
        x0, u_tm = scenarios(g, 2, 2)
        rng = np.random.default_rng(3)
        u_am = s._to_agent_major(np.asarray(u_tm, float)) + 0.05 * rng.standard_normal((2, s.n))
        p = draw_u_prev(s, 2, 41)
        check_deltas(s, x0, u_am, np.maximum(0.0, rng.standard_normal((2, s.n_c_total))), p, f'v2 {merit}')
        a, b = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm, u_prev=p)
        c = s.solve_batch(x0, u_tm, u_prev=np.zeros_like(p))
        assert not same(a['u'], b['u']) and all(same(a[k], c[k]) for k in KEYS), merit
        worst[merit] = (a['num_iters'].tolist(), b['num_iters'].tolist())
    print('v2 iterations without / with u_prev:', worst)


def test_f32_boundary_returns_the_rounded_fp64_results(games, solver_of):
    g, s = games['kb_chicane_N15'][0], solver_of('kb_chicane_N15')
    x0, u_tm = scenarios(g, 4, 13)
    p = draw_u_prev(s, 4, 43)
    x32, u32 = x0.astype(np.float32), np.asarray(u_tm).astype(np.float32)
    r64 = s.solve_batch(x32.astype(np.float64), u32.astype(np.float64), u_prev=p)
    r32 = s.solve_batch(x32, u32, dtype=np.float32, u_prev=p)
    z32 = s.solve_batch(x32, u32, dtype=np.float32)
    for key in DOUBLES:
        assert r32[key].dtype == np.float32 and np.array_equal(r32[key], r64[key].astype(np.float32), equal_nan=True), key
    for key in COUNTS:
        assert np.array_equal(r32[key], r64[key]), key
    assert not np.array_equal(z32['u'], r32['u'])


def test_half_arena_build_reads_u_prev(games, solver_of):
    """workgroups_per_cu=2 against the product build, to the bar of test_workgroups_per_cu_option_in_one_process (250 of 256 scenarios with
    identical (status, iterations, QPs): here every one of 8; their converged iterates within 1e-5), and that build's own deltas."""
    g = games['kb_chicane_N15'][0]
    s1, s2 = solver_of('kb_chicane_N15'), solver_of('kb_chicane_N15', workgroups_per_cu=2)
    assert s1._lib is not s2._lib
    x0, u_tm = scenarios(g, 8, 11)
    p = draw_u_prev(s1, 8, 47)
    r1, r2 = s1.solve_batch(x0, u_tm, u_prev=p), s2.solve_batch(x0, u_tm, u_prev=p)
    ident = (r1['status'] == r2['status']) & (r1['num_iters'] == r2['num_iters']) & (r1['qp_solves'] == r2['qp_solves'])
    conv = ident & (r1['status'] <= 1)
    rel = lambda a, b: float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
    print(f'256-thread build with u_prev: identical control flow on {int(ident.sum())}/8, converged iterates within '
          f'{max([rel(r2["u"][b], r1["u"][b]) for b in np.nonzero(conv)[0]], default=0.0):.1e}')
    assert ident.sum() >= 8 * 250 / 256 and all(rel(r2['u'][b], r1['u'][b]) < 1e-5 for b in np.nonzero(conv)[0])
    rng = np.random.default_rng(5)
    check_deltas(s2, x0[:3], s2._to_agent_major(np.asarray(u_tm[:3], float)), np.maximum(0.0, rng.standard_normal((3, s2.n_c_total))), p[:3], '256-thread build')


# ---- 5. chains ----------------------------------------------------------------------------------------------------------------------------
def teacher_force_u_prev(s, res):
    """closed_loop_checks.teacher_force with the recorded u_prev[t]: one solve_batch over every step that ran."""
    bb, tt = np.nonzero(np.arange(res['status'].shape[1])[None, :] < res['steps_done'][:, None])
    start = res['q_est'] if 'q_est' in res else res['q']
    assert np.isfinite(res['u_prev'][bb, tt]).all()
    ref = s.solve_batch(start[bb, tt], res['u_ws'][bb, tt], u_prev=res['u_prev'][bb, tt])
    for key in KEYS:
        got = res[key][bb, tt]
        bad = [(int(bb[i]), int(tt[i])) for i in range(len(bb)) if not same(got[i], ref[key][i])]
        assert not bad, f'{key}: closed-loop steps (scenario, step) {bad[:8]} differ from solve_batch on the same (q, u_ws, u_prev)'
    assert [res['msg'][b][t] for b, t in zip(bb, tt)] == ref['msg']
    return len(bb)


def check_carry(s, res, u_prev0=None):
    """u_prev[0] is u_prev0 (or zeros); u_prev[t + 1] is next_u_prev of step t's records where the chain went on to step t + 1, NaN where
    it did not."""
    from dgsqp_amd.closed_loop import next_u_prev
    B, T = res['status'].shape
    assert res['u_prev'].shape == (B, T, s.n_u)
    assert same(res['u_prev'][:, 0], np.zeros((B, s.n_u)) if u_prev0 is None else np.ascontiguousarray(u_prev0, dtype=np.float64))
    for t in range(T - 1):
        on = res['steps_done'] > t + 1
        want = next_u_prev(res['u_applied'][:, t], res['u_cmd'][:, t] if 'u_cmd' in res else None)
        assert same(res['u_prev'][on, t + 1], want[on]), t
        assert np.isnan(res['u_prev'][~on, t + 1]).all(), t


def test_chain_without_a_plant_carries_stage_0(games, solver_of):
    g, s = games['kb_chicane_N15'][0], solver_of('kb_chicane_N15')
    P, par = s._problem, s._cparams
    x0, u_tm = scenarios(g, 6, 41)
    u_am = s._to_agent_major(np.asarray(u_tm, float))
    plain = s.step_batch(x0, u_tm, 4, keep_predictions=True)
    res = s.step_batch(x0, u_tm, 4, keep_predictions=True, u_prev=True)
    check_feedback(s, res, x0, u_am)
    check_carry(s, res)
    assert teacher_force_u_prev(s, res) == int(res['steps_done'].sum())
    for key in KEYS:
        assert same(res[key][:, 0], plain[key][:, 0]), key          # step 0 runs against zeros either way
    assert not same(res['u'][:, 1], plain['u'][:, 1])               # ... step 1 does not
    # a given u_prev0
    p0 = draw_u_prev(s, 6, 53)
    given = s.step_batch(x0, u_tm, 2, keep_predictions=True, u_prev=p0)
    check_carry(s, given, p0)
    teacher_force_u_prev(s, given)
    assert not same(given['u'][:, 0], plain['u'][:, 0])
    # the limit holds ACROSS steps on converged steps, which it does not without the carry
    lim = P.dt * np.array([P.agents[a].rate_ub[j] for a in range(s.M) for j in range(2)])
    assert all(P.agents[a].rate_lb[j] == -P.agents[a].rate_ub[j] for a in range(s.M) for j in range(2))

    def worst_jump(r):
        prev = np.concatenate([np.zeros((len(x0), 1, s.n_u)), r['u_applied'][:, :-1]], axis=1)
        jump = np.abs(r['u_applied'] - prev) / lim
        return jump[r['converged']], jump
    with_carry, _ = worst_jump(res)
    without, _ = worst_jump(plain)
    print(f'largest |u_applied[t] - u_applied[t-1]| / (dt rate_ub) over converged steps: {with_carry.max():.4f} with carry, {without.max():.4f} without '
          f'({int((without.max(axis=-1) > 1.0 + 1e-3).sum())} of {len(without)} steps over the limit)')
    assert (with_carry * lim <= lim + par.p_tol).all()


def test_chain_with_delay_lines_carries_the_appended_command(games, solver_of):
    from dgsqp_amd.closed_loop import PlantModel
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    plant = PlantModel(method='rk4', M=3, sim_steps=2, delay_steps=DELAYS)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, u_prev=True)
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)))
    check_carry(s, res)
    teacher_force_u_prev(s, res)
    assert (res['steps_done'] == 3).all()
    delayed = res['u_plant'][:, :2, -1]                          # what the plant integrated under in its last simulation step
    assert not same(res['u_prev'][:, 1:], delayed)               # ... is not what was carried


def test_chain_with_a_pid_opponent_carries_u_cmd(games, solver_of):
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(du_max=(0.5, 0.05)))
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel(), drivers=drivers, u_prev=True)
    check_carry(s, res)
    teacher_force_u_prev(s, res)
    on = res['steps_done'] > 1
    assert on.any() and same(res['u_prev'][on, 1], res['u_cmd'][on, 0])
    assert not same(res['u_cmd'][on, 0, 2:], res['u_applied'][on, 0, 2:])      # the opponent's command is not the game's
    assert same(res['u_cmd'][on, 0, :2], res['u_applied'][on, 0, :2])


def test_600_identical_chains_on_a_smaller_grid(games, solver_of):
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    x1, u1 = scenarios(g, 1, 47)
    B = 600
    x0, u_tm = np.repeat(x1, B, axis=0), np.repeat(np.asarray(u1), B, axis=0)
    p0 = np.repeat(draw_u_prev(s, 1, 59), B, axis=0)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, u_prev=p0)
    for key in KEYS + ('q', 'u_ws', 'u_prev', 'steps_done'):
        assert same(res[key], np.repeat(res[key][:1], B, axis=0)), key       # nothing survives from a workgroup's previous chain
    first = {k: (v[:2] if isinstance(v, np.ndarray) else v[:2]) for k, v in res.items() if isinstance(v, (np.ndarray, list))}
    check_carry(s, first, p0[:2])
    teacher_force_u_prev(s, first)


def test_chain_that_ends_early_and_chain_after_a_failed_qp(games):
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    xa, ua = scenarios(g, 1, 31)
    xb, ub = scenarios(g, 2, 37)
    x0, u_tm = np.stack([xb[0], xa[0], xb[1]]), np.stack([ub[0], ua[0], ub[1]])
    x0[1, 11] = g.half_width + 1.0                               # car 2 of chain 1 starts outside the track: its step 0 is 'qp_fail'
    w = np.zeros((3, 4, s.n_q))
    w[2, 1, :] = np.nan                                          # chain 2 ends after two steps
    res = s.step_batch(x0, u_tm, 4, disturbance=w, keep_predictions=True, u_prev=True)
    check_feedback(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), w)
    check_carry(s, res)
    teacher_force_u_prev(s, res)
    assert res['steps_done'].tolist() == [4, 4, 2] and np.isnan(res['u_prev'][2, 2:]).all() and np.isfinite(res['u_prev'][2, :2]).all()
    assert res['msg'][1][0] == 'qp_fail' and same(res['u_ws'][1, 1], res['u_ws'][1, 0])
    assert same(res['u_prev'][1, 1], res['u_applied'][1, 0]) and np.isfinite(res['u_prev'][1, 1]).all()      # still the applied stage 0


# ---- 6. refusals through the raw ABI, coexistence -----------------------------------------------------------------------------------------
def test_refusals_and_coexistence(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None)
    lib, h = s._lib, s._h
    msg = lambda: lib.dgsqp_last_error(h).decode()
    B, T = 4, 3
    x0, u_tm = scenarios(g, B, 61)
    u_am = s._to_agent_major(np.asarray(u_tm, float))
    p = draw_u_prev(s, B, 67)
    buf = np.empty((T, B, s.n_u))
    # nothing recorded yet
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size) == -1 and 'no closed-loop launch' in msg()
    assert lib.dgsqp_set_u_prev(None, 0, None) == -1 and lib.dgsqp_set_closed_loop_u_prev(None, 0, 0, None) == -1 and lib.dgsqp_fetch_u_prev(None, None, 0) == -1
    before_solve = s.solve_batch(x0, u_tm)
    before_chain = s.step_batch(x0, u_tm, T, keep_predictions=True)
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size) == -1                 # a plain launch records none
    # NaN, in both setters; a bad mode; B < 0; an array without a size
    for v in (np.nan, np.inf):
        bad = p.copy()
        bad[2, 1] = v
        assert lib.dgsqp_set_u_prev(h, B, _ffi.dptr(bad)) == -1 and msg().startswith('u_prev: ') and '[2][1]' in msg()
        assert lib.dgsqp_set_closed_loop_u_prev(h, 1, B, _ffi.dptr(bad)) == -1 and msg().startswith('closed-loop u_prev: ') and '[2][1]' in msg()
    assert lib.dgsqp_set_closed_loop_u_prev(h, 2, B, None) == -1 and 'mode' in msg()
    assert lib.dgsqp_set_closed_loop_u_prev(h, 1, -1, None) == -1 and 'negative' in msg()
    assert lib.dgsqp_set_u_prev(h, 0, _ffi.dptr(p)) == -1 and lib.dgsqp_set_u_prev(h, B, None) == -1 and lib.dgsqp_set_u_prev(h, -1, _ffi.dptr(p)) == -1
    # (none of the refused calls left a setting behind)
    again = s.solve_batch(x0, u_tm)
    assert all(same(again[k], before_solve[k]) for k in KEYS)
    # wrong B: every entry point the setting applies to
    assert lib.dgsqp_set_u_prev(h, B, _ffi.dptr(p)) == 0
    x3, u3, l3 = np.ascontiguousarray(x0[:3]), np.ascontiguousarray(u_am[:3]), np.zeros((3, s.n_c_total))
    out = np.empty((3, s.n))
    tm = _ffi.TimingT()
    calls = {'solve_batch': lambda: lib.dgsqp_solve_batch(h, 3, _ffi.dptr(x3), _ffi.dptr(u3), _ffi.dptr(out), *([None] * 7), ctypes.byref(tm)),
             'stage_inputs': lambda: lib.dgsqp_stage_inputs(h, 3, _ffi.dptr(x3), _ffi.dptr(u3)),
             'solve_batch_f32': lambda: lib.dgsqp_solve_batch_f32(h, 3, x3.astype(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                                  u3.astype(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)), *([None] * 8), ctypes.byref(tm)),
             'evaluate_batch': lambda: lib.dgsqp_evaluate_batch(h, 3, _ffi.dptr(x3), _ffi.dptr(u3), None, _ffi.dptr(out), *([None] * 5)),
             'qp_batch': lambda: lib.dgsqp_qp_batch(h, 3, _ffi.dptr(x3), _ffi.dptr(u3), _ffi.dptr(l3), _ffi.dptr(out), None, None, None)}
    for name, call in calls.items():
        assert call() == -1 and msg().startswith('u_prev: ') and 'B = 4' in msg() and 'B = 3' in msg(), (name, msg())
    with_p = s.solve_batch(x0, u_tm)                             # sticky: the Python call passes none, the raw setting is still there
    assert not same(with_p['u'], before_solve['u'])
    sticky = s.step_batch(x0, u_tm, T, keep_predictions=True)    # a closed-loop launch ignores it
    assert all(same(sticky[k], before_chain[k]) for k in KEYS)
    assert lib.dgsqp_set_u_prev(h, 0, None) == 0
    for name, call in calls.items():
        if name != 'qp_batch':                                   # (l = 0 is no linearisation point the QP has to accept)
            assert call() == 0, (name, msg())
    # a carry launch; its record; capacities; a launch of another B than u_prev0's
    carry = s.step_batch(x0, u_tm, T, keep_predictions=True, u_prev=p)
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size - 1) == -1 and 'too small' in msg() and str(buf.size) in msg()
    assert lib.dgsqp_fetch_u_prev(h, None, buf.size) == -1
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size) == 0 and same(np.swapaxes(buf, 0, 1), carry['u_prev'])
    assert lib.dgsqp_set_closed_loop_u_prev(h, 1, B, _ffi.dptr(p)) == 0
    with pytest.raises(RuntimeError, match='closed-loop u_prev: '):
        s.step_batch(x0[:3], u_tm[:3], T)
    assert lib.dgsqp_set_closed_loop_u_prev(h, 1, 0, None) == 0
    raw_carry = s.step_batch(x0, u_tm, T, keep_predictions=True)                  # the raw setting is on: this launch carries, from zeros
    mid_solve = s.solve_batch(x0, u_tm)                          # ... and a solve_batch ignores the closed-loop setting
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size) == 0 and same(buf[0], np.zeros((B, s.n_u))) and not same(raw_carry['u'], before_chain['u'])
    assert lib.dgsqp_set_closed_loop_u_prev(h, 0, 0, None) == 0
    # coexistence: after all that, the plain launch and the plain solve give what they gave before
    after_chain, after_solve = s.step_batch(x0, u_tm, T, keep_predictions=True), s.solve_batch(x0, u_tm)
    for key in KEYS:
        assert same(after_solve[key], before_solve[key]) and same(mid_solve[key], before_solve[key]), key
    for key in CHAIN:
        if key in before_chain:
            assert same(after_chain[key], before_chain[key]), key
    assert 'u_prev' not in after_chain and not same(carry['u'], before_chain['u'])
    assert lib.dgsqp_fetch_u_prev(h, _ffi.dptr(buf), buf.size) == -1 and 'no closed-loop launch' in msg()      # the last launch carried nothing
    with pytest.raises(ValueError, match='u_prev must be'):
        s.solve_batch(x0, u_tm, u_prev=p[:3])
    with pytest.raises(ValueError, match='not finite'):
        s.step_batch(x0, u_tm, T, u_prev=np.full((B, s.n_u), np.nan))


def test_single_scenario_surface_carries_on_request(games):
    """DGSQP(..., carry_u_prev=True): solve() runs against self.u_prev, which step() sets to u_pred[0]; the default resets it."""
    from dgsqp_amd.solver import DGSQP
    g = games['kb_chicane_N15'][0]
    x0, u_tm = scenarios(g, 1, 3)
    from dgsqp_amd.types import VehicleState
    batch = DGSQP(*g.solver_args(), print_method=None)
    states = [VehicleState(t=0.0), VehicleState(t=0.0)]
    g.joint_model.qu2state(states, x0[0], None)
    for carry in (False, True):
        s = DGSQP(*g.solver_args(), print_method=None, carry_u_prev=carry)
        s.set_warm_start(np.asarray(u_tm[0], float))
        s.u_prev = np.array([-1.2, 0.1, 0.4, -0.2])
        s.solve(states)
        want = batch.solve_batch(x0, u_tm, u_prev=s.u_prev[None, :] if carry else None)
        assert same(s._last_u_agent_major, want['u'][0]), carry
        assert carry or not s.u_prev.any()
