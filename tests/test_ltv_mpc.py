"""LTV-MPC reference tracker on the MI355X (dgsqp_amd/ltv_mpc.py, csrc/dgsqp_mpc.h), teacher-forced per iteration: for every logged
iteration the helper (tests/ltv_mpc_checks.py) rebuilds the reference's QP from the DEVICE's own logged D and the device's D_bar and
multipliers are held to the bars of test_qp_parity_and_kkt (primal 1e-8, multipliers 1e-6 relative, identical active sets, stationarity
1e-7 scale, feasibility 1e-12, complementarity 1e-10 scale), the equality residuals of D_bar to 1e-11 relative, the damped update, zeroing,
unpacking and fallback bit for bit to a numpy replay, and q_ws to the oracle's rollout at rtol 1e-13."""
import numpy as np
import pytest

import ltv_mpc_checks as chk

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def vs(q=None, u=(0.0, 0.0), ey=0.0, v=0.0, s=0.0, epsi=0.0):
    from dgsqp_amd.types import VehicleState, ParametricPose, BodyLinearVelocity, VehicleActuation
    return VehicleState(p=ParametricPose(s=s, x_tran=ey, e_psi=epsi), v=BodyLinearVelocity(v_long=v), u=VehicleActuation(u_a=u[0], u_steer=u[1]))


def box(mdl, q_ub, q_lb, u_ub, u_lb, du_ub, du_lb):
    """The reference's bounds dict from plain vectors (through the model's own q2state)."""
    from dgsqp_amd.types import VehicleState
    out = {}
    for key, q, u in (('qu_ub', q_ub, u_ub), ('qu_lb', q_lb, u_lb), ('du_ub', np.zeros(mdl.n_q), du_ub), ('du_lb', np.zeros(mdl.n_q), du_lb)):
        st = VehicleState()
        mdl.qu2state(st, np.asarray(q, float), np.asarray(u, float))
        out[key] = st
    return out


INF = 1e10


def scenario(kind, B, N, seed, spread=1.0):
    """q0, u_ws, du_ws, q_ref of B scenarios on the curve track: a car near the centre line at ~1.5 m/s, a reference that runs ahead at
    1.8 m/s, a small random warm start."""
    rng = np.random.default_rng(seed)
    nq = 8 if kind == 'dyn' else 6
    q0 = np.zeros((B, nq))
    s0 = 0.3 + 0.5 * rng.random(B)
    if kind == 'dyn':
        q0[:, 2], q0[:, 3], q0[:, 4], q0[:, 5], q0[:, 6], q0[:, 7] = 1.5 + 0.2 * rng.random(B), 0.02 * rng.standard_normal(B), 0.05 * rng.standard_normal(B), 0.05 * rng.standard_normal(B), s0, 0.2 * spread * rng.standard_normal(B)
        V, S, EY = 2, 6, 7
    else:
        q0[:, 2], q0[:, 3], q0[:, 4], q0[:, 5] = 1.5 + 0.2 * rng.random(B), 0.05 * rng.standard_normal(B), s0, 0.2 * spread * rng.standard_normal(B)
        V, S, EY = 2, 4, 5
    q0[:, 0], q0[:, 1] = s0, q0[:, EY]
    u_ws = np.concatenate((0.3 * rng.standard_normal((B, N + 1, 1)), 0.05 * rng.standard_normal((B, N + 1, 1))), axis=2)
    du_ws = 0.1 * rng.standard_normal((B, N, 2))
    q_ref = np.zeros((B, N + 1, nq))
    q_ref[:, :, V] = 1.8
    q_ref[:, :, S] = s0[:, None] + 0.18 * np.arange(N + 1)[None, :]
    q_ref[:, :, 0] = q_ref[:, :, S]
    return q0, u_ws, du_ws, q_ref, (V, S, EY)


def weights(kind, idx, terminal=False):
    from dgsqp_amd.ltv_mpc import TrackingCost
    V, S, EY = idx
    nq = 8 if kind == 'dyn' else 6
    w = np.zeros(nq)
    w[V], w[S], w[EY], w[EY - 2 if kind == 'dyn' else 3] = 1.0, 2.0, 5.0, 0.5
    cN = None
    if terminal:
        cN = np.zeros(nq); cN[S] = -1.0
    return TrackingCost(state_weight=w, input_weight=(1e-2, 1e-2), rate_weight=(0.01, 1.0), terminal_linear=cN)


@pytest.fixture(scope='module')
def handles(games):
    from dgsqp_amd.solver import DGSQP
    out = {}
    for kind, name in (('kin', 'kb_curve_N10'), ('dyn', 'dyn_curve_N15')):
        g, P, par = games[name]
        out[kind] = (DGSQP(*g.solver_args(), print_method=None), g, P)
    return out


def wide_bounds(mdl, idx, v_lb=-INF, ey=INF, u=(2.1, 0.436), du=(10.0, 4.5), v_ub=INF):
    V, S, EY = idx
    q_ub, q_lb = INF * np.ones(mdl.n_q), -INF * np.ones(mdl.n_q)
    q_ub[EY], q_lb[EY], q_lb[V], q_ub[V] = ey, -ey, v_lb, v_ub
    return box(mdl, q_ub, q_lb, u, (-u[0], -u[1]), du, (-du[0], -du[1]))


def teacher_forced(oracle, solver, P, agent, out, rec_kw, q0, u_ws, q_ref, p_obs, expect=(), dyn=None):
    """Every logged iteration of every scenario against the helper's QP at the device's own D.  Returns the kinds of rows seen active."""
    from dgsqp_amd import ltv_mpc
    d = out['dims']
    mdl = solver.joint_dynamics.dynamics_models[agent]
    rec = rec_kw
    R = chk.record_dict(rec, mdl.n_q)
    N, nz = R['N'], mdl.n_q + 2
    dyn = chk.oracle_dyn(oracle, P, agent) if dyn is None else dyn
    dt = float(P.dt)
    rows = [tuple(int(v) for v in r) for r in d['rows']]
    seen = set()
    worst = dict(primal=0.0, lam=0.0, stat=0.0, feas=-np.inf, comp=0.0, eq=0.0)
    want_status = [0] * q0.shape[0]
    for b in range(q0.shape[0]):
        # q_ws: iteration 0's D against the oracle rollout
        D0 = out['log_D'][b, 0]
        q_ws = D0[:(N + 1) * nz].reshape(N + 1, nz)[:, :mdl.n_q]
        np.testing.assert_allclose(q_ws, chk.rollout(dyn, q0[b], u_ws[b, 1:]), rtol=1e-13, atol=1e-13)
        for it in range(int(rec.qp_iters)):
            D = out['log_D'][b, it]
            if np.isnan(D).any():
                continue
            h = chk.solve_iteration(oracle, R, dt, dyn, rows, D, q0[b], u_ws[b, 0], q_ref[b], None if p_obs is None else p_obs[b])
            Db, lam = out['log_D_bar'][b, it], out['log_lam'][b, it]
            if h['flag'] != 0:
                assert np.isnan(Db).all() and out['status'][b] == 4, (b, it)
                want_status[b] = 4
                continue
            assert h['strict'], ('the case is not strictly complementary: advance its seed', b, it)
            cs = h['cond_scale']
            x_dev = Db[(N + 1) * nz:]
            worst['primal'] = max(worst['primal'], chk.rel(x_dev, h['x'])); worst['lam'] = max(worst['lam'], chk.rel(lam, h['lam']))
            print(f'b={b} it={it} primal {chk.rel(x_dev, h["x"]):.2e} lam {chk.rel(lam, h["lam"]):.2e} active {int(h["active"].sum())}')
            assert chk.rel(x_dev, h['x']) < 1e-8 * cs and chk.rel(lam, h['lam']) < 1e-6 * cs, (b, it)
            assert np.array_equal(lam > 0, h['active']), (b, it)
            stat = np.abs(h['Hc'] @ x_dev + h['gc'] + h['G'].T @ lam).max()
            feas = (h['G'] @ x_dev + h['g']).max() if len(rows) else -np.inf
            comp = np.abs(lam * (h['G'] @ x_dev + h['g'])).max() if len(rows) else 0.0
            eq = np.abs(h['qp']['A_eq'] @ Db - h['qp']['b_eq']).max() / max(1.0, np.abs(Db).max())
            print(f'      stat {stat:.2e} feas {feas:.2e} comp {comp:.2e} eq {eq:.2e} (scale {h["scale"]:.2e})')
            for k, v in (('stat', stat), ('feas', feas), ('comp', comp), ('eq', eq)):
                worst[k] = max(worst[k], v)
            assert stat < 1e-7 * h['scale'] and feas < 1e-12 and lam.min() >= 0 and comp < 1e-10 * h['scale'], (b, it, stat, feas, comp)
            assert eq < 1e-11, (b, it, eq)
            seen |= {(rows[i][0], rows[i][2], rows[i][3]) for i in np.nonzero(h['active'])[0]}
            # the update, bit for bit
            new = chk.replay_update(D, Db, float(rec.damping), (N + 1) * nz + N * 2, N, nz, bool(rec.zero_du))
            if it + 1 < int(rec.qp_iters):
                assert np.array_equal(bits(out['log_D'][b, it + 1]), bits(new)), (b, it)
            else:
                assert np.array_equal(bits(out['q_pred'][b]), bits(new[:(N + 1) * nz].reshape(N + 1, nz)[:, :mdl.n_q]))
                assert np.array_equal(bits(out['u_pred'][b]), bits(new[:(N + 1) * nz].reshape(N + 1, nz)[1:, mdl.n_q:]))
                assert np.array_equal(bits(out['du_pred'][b]), bits(new[(N + 1) * nz:(N + 1) * nz + 2 * N].reshape(N, 2)))
    print('worst', worst)
    assert out['status'].tolist() == want_status, (out['status'].tolist(), want_status)
    return seen


def run(solver, agent, cost, bounds, q0, u_ws, du_ws, q_ref, p_obs=None, **kw):
    from dgsqp_amd import ltv_mpc
    mdl = solver.joint_dynamics.dynamics_models[agent]
    q_ub, u_ub = mdl.state2qu(bounds['qu_ub']); q_lb, u_lb = mdl.state2qu(bounds['qu_lb'])
    _, du_ub = mdl.state2qu(bounds['du_ub']); _, du_lb = mdl.state2qu(bounds['du_lb'])
    rec = ltv_mpc.lower(agent, mdl.n_q, cost, kw.get('soft'), kw.get('obstacle'), q_ub, q_lb, u_ub, u_lb, du_ub, du_lb, kw['N'], kw.get('qp_iters', 2),
                        kw.get('damping', 0.75), kw.get('zero_du', False))
    return rec, solver.mpc_batch(agent, cost, bounds, q0, u_ws, du_ws, q_ref, p_obs, log=True, **kw)


@pytest.mark.parametrize('kind,N', [('kin', 3), ('dyn', 4)])
def test_basic_models_teacher_forced(oracle, handles, kind, N):
    solver, g, P = handles[kind]
    q0, u_ws, du_ws, q_ref, idx = scenario(kind, 4, N, seed=5)
    mdl = solver.joint_dynamics.dynamics_models[0]
    rec, out = run(solver, 0, weights(kind, idx), wide_bounds(mdl, idx), q0, u_ws, du_ws, q_ref, N=N)
    assert (out['status'] == 0).all()
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)


def test_spline_track(oracle):
    """Kinematic bicycle, N = 3, on the F1 cubic-spline track (the SPL instantiations of the rollout and of the linearisation)."""
    from dgsqp_amd.montecarlo import f1_racing_game
    from dgsqp_amd.solver import DGSQP, build_problem
    g = f1_racing_game(N=6)
    solver, P = DGSQP(*g.solver_args(), print_method=None), build_problem(*g.solver_args())
    assert int(P.track_kind) == 1
    N = 3
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=23)
    q0[:, idx[1]] += np.array([0.0, 7.3, 21.9])            # three places on the circuit, curvature of both signs
    q_ref[:, :, idx[1]] += np.array([0.0, 7.3, 21.9])[:, None]
    mdl = solver.joint_dynamics.dynamics_models[0]
    rec, out = run(solver, 0, weights('kin', idx), wide_bounds(mdl, idx, u=(0.6, 0.2), du=(3.0, 1.0)), q0, u_ws, du_ws, q_ref, N=N)
    assert (out['status'] == 0).all()
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)


def test_point_mass(oracle):
    """The track-frame point mass, N = 3.  The oracle has no point mass: fd is the package's numpy model (closed_loop.track_reference with
    the game's integrator) and [fAd fBd] its fourth-order central differences (ltv_mpc_checks.numpy_dyn: accurate to ~1e-13, below every bar used here)."""
    from dgsqp_amd.closed_loop import track_reference
    from dgsqp_amd.montecarlo import point_mass_racing_game
    from dgsqp_amd.solver import DGSQP, build_problem
    g = point_mass_racing_game(N=5)
    solver, P = DGSQP(*g.solver_args(), print_method=None), build_problem(*g.solver_args())
    cfg = g.joint_model.model_config
    mdl = solver.joint_dynamics.dynamics_models[0]
    dyn = chk.numpy_dyn(lambda q, u: track_reference(mdl, q, u, cfg.discretization_method, cfg.dt, cfg.M))
    N = 3
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=29)
    rec, out = run(solver, 0, weights('kin', idx), wide_bounds(mdl, idx, u=(0.6, 0.2), du=(3.0, 1.0)), q0, u_ws, du_ws, q_ref, N=N)
    assert (out['status'] == 0).all()
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None, dyn=dyn)


def test_active_sets_teacher_forced(oracle, handles):
    """Input box, rate box, hard state boxes (e_y and the v_long lower bound), a soft bound with positive slack, an obstacle row and the
    terminal linear term, each active in at least one scenario of the batch (asserted from the helper's own answer)."""
    from dgsqp_amd.ltv_mpc import ObstacleAvoidance, SoftStateBounds
    solver, g, P = handles['kin']
    N = 5
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 6, N, seed=11, spread=2.0)
    V, S, EY = idx
    # hard boxes: the reference asks for 1 m/s and e_y = 1 m; the car (1.6 .. 1.7 m/s, e_y = 0.15) brakes into the acceleration box and its
    # rate box, down to the v_long lower bound, and steers out to the e_y bound
    qa, qr = q0.copy(), q_ref.copy()
    qa[:, V], qa[:, EY], qa[:, 3] = 1.6 + 0.1 * np.random.default_rng(2).random(6), 0.15, 0.0
    qr[:, :, V], qr[:, :, EY] = 1.0, 1.0
    b1 = wide_bounds(mdl, idx, v_lb=1.55, ey=0.25, u=(0.5, 0.436), du=(1.5, 4.5))
    rec, out = run(solver, 0, weights('kin', idx, terminal=True), b1, qa, u_ws, du_ws, qr, N=N, qp_iters=2)
    seen = teacher_forced(oracle, solver, P, 0, out, rec, qa, u_ws, qr, None)
    assert out['status'].tolist() == [4, 0, 0, 0, 0, 0]          # (scenario 0: u_prev = -0.58 lies outside the acceleration box)
    # a soft e_y bound (starts lie outside it: positive slack), an acceleration box the 1.8 m/s reference runs into, and an obstacle beside
    # the path that comes within 2 r of the car at the last stages only
    p_obs = np.stack([q_ref[:, 1:, 0], q0[:, None, 1] + (0.55 - 0.03 * np.arange(1, N + 1))[None, :]], axis=2)
    b2 = wide_bounds(mdl, idx, ey=0.1, u=(0.2, 0.436), du=(10.0, 4.5))
    # (scenario 0 keeps a u_prev outside the acceleration box: u_{-1} is fixed AND bounded, CA_LTV_MPC.py:742-743, so its QP is infeasible)
    u2 = u_ws.copy()
    u2[1:, 0, 0] = np.clip(u2[1:, 0, 0], -0.2, 0.2)
    assert abs(u2[0, 0, 0]) > 0.2
    rec2, out2 = run(solver, 0, weights('kin', idx, terminal=True), b2, q0, u2, du_ws, q_ref, p_obs, N=N, qp_iters=2,
                     soft=SoftStateBounds([EY], [5.0], [25.0]), obstacle=ObstacleAvoidance(0.21))
    seen2 = teacher_forced(oracle, solver, P, 0, out2, rec2, q0, u2, q_ref, p_obs)
    assert out2['status'].tolist() == [4, 0, 0, 0, 0, 0]
    print('active kinds', seen, seen2)
    kinds, kinds2 = {k for k, _, _ in seen}, {k for k, _, _ in seen2}
    assert chk.RATE in kinds and chk.INPUT in kinds | kinds2 and (chk.STATE, EY, 1) in seen and (chk.STATE, V, -1) in seen, seen
    assert {chk.SOFT, chk.OBS} <= kinds2, seen2
    assert rec.c_N[S] == -1.0
    assert np.nanmax(out2['log_D_bar'][:, :, -2:]) > 1e-3          # a positive slack


def test_warm_start_variant_and_iteration_counts(oracle, handles):
    solver, g, P = handles['kin']
    N = 4
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=7)
    b = wide_bounds(mdl, idx, u=(1.0, 0.2), du=(3.0, 1.0))
    for kw in (dict(qp_iters=2, damping=0.5, zero_du=True), dict(qp_iters=2, damping=0.75), dict(qp_iters=5, damping=0.75)):
        rec, out = run(solver, 0, weights('kin', idx), b, q0, u_ws, du_ws, q_ref, N=N, **kw)
        assert (out['status'] == 0).all()
        teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)
        if kw.get('zero_du'):
            assert not out['du_pred'].any() and not out['log_D'][:, 1, (N + 1) * (mdl.n_q + 2):].any()


def test_infeasible_qp_falls_back_and_leaves_the_others(oracle, handles):
    """v_long upper bound below what the rate box can reach at stage 1 (scenario 1 only starts that fast)."""
    solver, g, P = handles['kin']
    N = 4
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=9)
    V = idx[0]
    q0[1, V] = 3.0
    u_ws[:, 0, 0] = 0.0
    b = wide_bounds(mdl, idx, v_ub=2.0, du=(1.0, 4.5))
    rec, out = run(solver, 0, weights('kin', idx), b, q0, u_ws, du_ws, q_ref, N=N)
    assert out['status'].tolist() == [0, 4, 0]
    dyn = chk.oracle_dyn(oracle, P, 0)
    assert np.array_equal(bits(out['u_pred'][1]), bits(u_ws[1, 1:])) and np.array_equal(bits(out['du_pred'][1]), bits(du_ws[1]))
    assert np.array_equal(bits(out['q_pred'][1]), bits(out['log_D'][1, 0][:(N + 1) * 8].reshape(N + 1, 8)[:, :6]))
    np.testing.assert_allclose(out['q_pred'][1], chk.rollout(dyn, q0[1], u_ws[1, 1:]), rtol=1e-13, atol=1e-13)
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)
    keep = [0, 2]
    rec2, alone = run(solver, 0, weights('kin', idx), b, q0[keep], u_ws[keep], du_ws[keep], q_ref[keep], N=N)
    for k in ('q_pred', 'u_pred', 'du_pred'):
        assert np.array_equal(bits(out[k][keep]), bits(alone[k]))


@pytest.mark.parametrize('N', [40, 64])
def test_large_n(oracle, handles, N):
    from dgsqp_amd.ltv_mpc import mpc_dims
    solver, g, P = handles['kin']
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 2, N, seed=3)
    u_ws *= 0.2
    b = wide_bounds(mdl, idx, ey=0.6, u=(1.0, 0.2), du=(3.0, 1.0))
    rec, out = run(solver, 0, weights('kin', idx), b, q0, u_ws, du_ws, q_ref, N=N, qp_iters=1)
    assert out['dims']['n'] == 2 * N and (out['status'] == 0).all()
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)


def test_refusals_through_the_raw_abi(handles):
    import ctypes as C
    from dgsqp_amd import _ffi, ltv_mpc
    solver, g, P = handles['kin']
    lib, h = solver._lib, solver._h
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 1, 3, seed=1)
    cost = weights('kin', idx)

    def rec(N=3, agent=0, **kw):
        q_ub, q_lb = INF * np.ones(6), -INF * np.ones(6)
        r = ltv_mpc.lower(agent, 6, cost, None, kw.pop('obstacle', None), q_ub, q_lb, (1, 1), (-1, -1), (1, 1), (-1, -1), N, 2, 0.75)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def refused(r, code, word):
        assert lib.dgsqp_set_mpc(h, C.byref(r)) == code
        assert word in lib.dgsqp_last_error(h).decode(), lib.dgsqp_last_error(h)

    refused(rec(N=65), _ffi.E_TOO_LARGE, '130 condensed variables')
    assert lib.dgsqp_set_mpc(h, C.byref(rec(N=64))) == 0
    refused(rec(agent=2), _ffi.E_ARG, 'agent 2')
    refused(rec(agent=-1), _ffi.E_ARG, 'agent -1')
    r = rec(); r.w_du[1] = 0.0
    refused(r, _ffi.E_ARG, 'w_du must be positive')
    refused(rec(qp_iters=0), _ffi.E_ARG, 'qp_iters')
    refused(rec(damping=1.5), _ffi.E_ARG, 'damping')
    refused(rec(n_soft=2), _ffi.E_ARG, 'n_soft')
    # a missing p_obs with obs_r > 0, no tracker set, a short log capacity
    assert lib.dgsqp_set_mpc(h, C.byref(rec(obstacle=ltv_mpc.ObstacleAvoidance(0.2)))) == 0
    args = [_ffi.dptr(np.ascontiguousarray(a)) for a in (q0, u_ws, du_ws, q_ref)]
    assert lib.dgsqp_mpc_batch(h, 1, *args, None, None, None, None, None, None, None) == _ffi.E_ARG and b'p_obs' in lib.dgsqp_last_error(h)
    assert lib.dgsqp_set_mpc(h, None) == 0
    assert lib.dgsqp_mpc_batch(h, 1, *args, None, None, None, None, None, None, None) == _ffi.E_ARG and b'no tracker set' in lib.dgsqp_last_error(h)
    assert lib.dgsqp_set_mpc(h, C.byref(rec())) == 0 and lib.dgsqp_set_mpc_log(h, 1) == 0
    assert lib.dgsqp_mpc_batch(h, 1, *args, None, None, None, None, None, None, None) == 0
    buf = np.zeros(10000)
    assert lib.dgsqp_fetch_mpc_log(h, _ffi.dptr(buf), None, None, 0) == _ffi.E_ARG and b'too small' in lib.dgsqp_last_error(h)
    d = _ffi.MpcDimsT()
    assert lib.dgsqp_mpc_dims(h, C.byref(d), (_ffi.MpcRowT * 1)(), 1) == _ffi.E_ARG and b'row table too small' in lib.dgsqp_last_error(h)
    assert lib.dgsqp_set_mpc_log(h, 0) == 0


def test_batch_larger_than_the_grid_and_reproducible(handles):
    """600 identical scenarios on a grid of at most one workgroup per CU: bitwise equal results (nothing survives a workgroup's previous
    scenario), and a second run of a mixed batch repeats the first bit for bit."""
    solver, g, P = handles['kin']
    N = 4
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 2, N, seed=13)
    b = wide_bounds(mdl, idx, ey=0.3, u=(0.6, 0.15), du=(2.0, 0.8))
    B = 600
    # scenario 1 first on every workgroup's second visit: interleave two different scenarios, then compare each with its twins
    sel = np.arange(B) % 2
    rec, out = run(solver, 0, weights('kin', idx), b, q0[sel], u_ws[sel], du_ws[sel], q_ref[sel], N=N)
    assert out['timing']['grid'] < B
    for k in ('q_pred', 'u_pred', 'du_pred', 'status', 'qp_steps', 'log_D', 'log_D_bar', 'log_lam'):
        for s_ in (0, 1):
            a = out[k][sel == s_]
            assert (a.view(np.uint64 if a.dtype == np.float64 else a.dtype) == a[:1].view(np.uint64 if a.dtype == np.float64 else a.dtype)).all(), k
    rec, again = run(solver, 0, weights('kin', idx), b, q0[sel], u_ws[sel], du_ws[sel], q_ref[sel], N=N)
    for k in ('q_pred', 'u_pred', 'du_pred', 'log_D_bar', 'log_lam'):
        assert np.array_equal(bits(out[k]), bits(again[k])), k


def test_agent_one_between_solves_on_one_handle(oracle, games, handles):
    """Agent 1 of the two-agent game's handle, with a solve_batch before and after on that handle whose results equal a fresh handle's."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP
    solver, g, P = handles['kin']
    x0, u0 = sample_scenarios(g, 4, seed=3)
    fresh = DGSQP(*g.solver_args(), print_method=None).solve_batch(x0, u0)
    before = solver.solve_batch(x0, u0)
    N = 4
    mdl = solver.joint_dynamics.dynamics_models[1]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=21)
    rec, out = run(solver, 1, weights('kin', idx), wide_bounds(mdl, idx, u=(0.8, 0.2)), q0, u_ws, du_ws, q_ref, N=N)
    teacher_forced(oracle, solver, P, 1, out, rec, q0, u_ws, q_ref, None)
    after = solver.solve_batch(x0, u0)
    for k in ('u', 'l', 'status', 'num_iters'):
        assert np.array_equal(np.asarray(fresh[k]), np.asarray(before[k])) and np.array_equal(np.asarray(fresh[k]), np.asarray(after[k])), k


def test_256_thread_build(oracle, games):
    """The N = 4 case on libdgsqp_hip_b256.so, and its refusal where the half arena does not hold the tracker."""
    import ctypes as C
    from dgsqp_amd import _ffi, ltv_mpc
    from dgsqp_amd.solver import DGSQP
    g, P, par = games['kb_curve_N10']
    solver = DGSQP(*g.solver_args(), print_method=None, workgroups_per_cu=2)
    N = 4
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=7)
    b = wide_bounds(mdl, idx, u=(1.0, 0.2), du=(3.0, 1.0))
    rec, out = run(solver, 0, weights('kin', idx), b, q0, u_ws, du_ws, q_ref, N=N)
    assert out['timing']['block'] == 256 and (out['status'] == 0).all()
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)
    q_ub, q_lb = INF * np.ones(6), -INF * np.ones(6)
    big = ltv_mpc.lower(0, 6, weights('kin', idx), None, None, q_ub, q_lb, (1, 1), (-1, -1), (1, 1), (-1, -1), 64, 2, 0.75)
    assert solver._lib.dgsqp_set_mpc(solver._h, C.byref(big)) == _ffi.E_TOO_LARGE
    assert b'LDS' in solver._lib.dgsqp_last_error(solver._h)


def test_class_surface_equals_the_batched_entry(handles):
    """solve() / step() bit for bit the batched entry with B = 1, set_warm_start(state=...) the 2-iteration / 0.5 / zeroed-du variant."""
    from dgsqp_amd.ltv_mpc import CA_LTV_MPC, shift_warm_start
    from dgsqp_amd.solver_types import CALTVMPCParams
    solver, g, P = handles['kin']
    mdl = solver.joint_dynamics.dynamics_models[0]
    N = 4
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 1, N, seed=17)
    b = wide_bounds(mdl, idx, u=(1.0, 0.2), du=(3.0, 1.0))
    cost = weights('kin', idx)
    mpc = CA_LTV_MPC(mdl, cost, None, b, CALTVMPCParams(N=N, dt=0.1), print_method=None)
    from dgsqp_amd.types import VehicleState
    st = VehicleState()
    mdl.qu2state(st, q0[0], u_ws[0, 0])
    q0r = mdl.state2qu(st)[0][None]
    mpc.set_warm_start(u_ws[0], du_ws[0])
    assert mpc.solve(st, q_ref[0].ravel())
    rec, ref = run(solver, 0, cost, b, q0r, u_ws, du_ws, q_ref, N=N)
    for k in ('q_pred', 'u_pred', 'du_pred'):
        assert np.array_equal(bits(getattr(mpc, k)), bits(ref[k][0])), k
    mpc.step(st, q_ref[0].ravel())
    uw, dw = shift_warm_start(ref['u_pred'][0], ref['du_pred'][0])
    assert np.array_equal(bits(mpc.u_ws), bits(uw)) and np.array_equal(bits(mpc.du_ws), bits(dw)) and st.u.u_a == ref['u_pred'][0][0, 0]
    mpc.set_warm_start(u_ws[0], du_ws[0], state=st, parameters=q_ref[0].ravel())
    rec, ws = run(solver, 0, cost, b, q0r, u_ws, du_ws, q_ref, N=N, qp_iters=2, damping=0.5, zero_du=True)
    assert np.array_equal(bits(mpc.q_pred), bits(ws['q_pred'][0])) and np.array_equal(bits(mpc.u_ws[1:]), bits(ws['u_pred'][0])) and not mpc.du_ws.any()
    assert mpc.get_prediction().s is not None


def test_saturated_input_survives_its_own_feedback(oracle, handles):
    """step() feeds u_pred[0] back as u_prev.  With the acceleration box active at stage 0 that value is the bound give or take a row
    tolerance and an ulp of the damped update; u_{-1} is fixed AND bounded, so a strict test would call every QP of the next step
    infeasible.  Eight steps at full throttle stay at status 0; through the batched entry a u_prev 5e-13 beyond the bound is solved on the
    bound (teacher forced, the helper restates the rule), 1e-9 beyond it is infeasible."""
    from dgsqp_amd.ltv_mpc import CA_LTV_MPC
    from dgsqp_amd.solver_types import CALTVMPCParams
    from dgsqp_amd.types import VehicleState
    solver, g, P = handles['kin']
    mdl = solver.joint_dynamics.dynamics_models[0]
    N = 4
    q0, u_ws, du_ws, q_ref, idx = scenario('kin', 3, N, seed=31)
    V, S, EY = idx
    b = wide_bounds(mdl, idx, u=(0.5, 0.3), du=(10.0, 4.5))
    cost = weights('kin', idx)
    mpc = CA_LTV_MPC(mdl, cost, None, b, CALTVMPCParams(N=N, dt=0.1), print_method=None)
    st = VehicleState()
    mdl.qu2state(st, q0[0], np.array([0.5, 0.0]))
    mpc.set_warm_start(np.tile([0.5, 0.0], (N + 1, 1)), np.zeros((N, 2)))
    dyn = chk.oracle_dyn(oracle, P, 0)
    beyond = 0
    for step in range(8):
        q = mdl.state2qu(st)[0]
        ref = np.zeros((N + 1, 6))
        ref[:, V], ref[:, S] = 4.0, q[S] + 0.4 * np.arange(N + 1)            # far faster than the car: full throttle
        assert mpc.solve(st, ref.ravel()), step
        u0 = mpc.u_pred[0].copy()
        assert abs(u0[0] - 0.5) < 1e-9, (step, u0)                            # the acceleration box is active at stage 0
        beyond += u0[0] > 0.5
        mpc.step(st, ref.ravel())
        mdl.qu2state(st, dyn(q, mpc.u_ws[0])[0], mpc.u_ws[0])
    print('steps whose applied input lay beyond the bound:', beyond)
    u2 = u_ws.copy()
    u2[:, 0, 0] = [0.5 + 5e-13, 0.5 + 1e-9, -0.5 - 5e-13]
    rec, out = run(solver, 0, cost, b, q0, u2, du_ws, q_ref, N=N)
    assert out['status'].tolist() == [0, 4, 0]
    teacher_forced(oracle, solver, P, 0, out, rec, q0, u2, q_ref, None)
