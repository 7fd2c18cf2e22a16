"""The Frenet point mass (``CasadiKinematicUnicycleCombined``, DGSQP_MODEL_UNICYCLE_COMBINED = 3) on the device.

No oracle anywhere in this file: oracle/ has no model 3 and would run the kinematic bicycle in its place.  What stands in for it:

* the five exact fixtures tests/golden/multistage_{pm2_euler_N3, pm2_rk4_N4, mix3_rk4m3_N3, pm3_N20_dir, pm3_N25_dir}.npz (mpmath, 60
  digits, tools/make_multistage_kats.py) at the device bar in force: 1e-11 relative to the largest entry of each array, or 64 x the
  fixture's sensitivity where that is larger; x elementwise at rtol 1e-13;
* the numpy mirror ``CasadiKinematicUnicycleCombined.fd``, which tests/test_point_mass_host.py ties to the same fixtures, for the
  closed-loop plant: q[t+1] from the device's own q[t] and u_plant[t], 1e-12 relative to max(1, |q|_inf) (row (f3)'s bar);
* teacher forcing and the bit-for-bit rules of tests/closed_loop_checks.py for everything that is data movement or a repeated solve.

Sizes: N <= 10, B <= 8, T <= 4 except where a fixture says otherwise."""
import copy
import ctypes
import dataclasses

import numpy as np
import pytest

import point_mass_kat as pk
from closed_loop_checks import BAR, COUNTS, DELAYS, DOUBLES, check_chain, check_monitor, same, scenarios, teacher_force
from closed_loop_hold_checks import check_plan_chain, teacher_force_solved

pytestmark = pytest.mark.gpu

KEYS = DOUBLES + COUNTS
KNOWN = {0, 1, 2, 3, 4, 5}
MEASURED = {}


def pm_game(kind='curve', **kw):
    from dgsqp_amd.montecarlo import point_mass_racing_game
    return point_mass_racing_game(kind, **kw)


@pytest.fixture(scope='module')
def race():
    """(game, solver) of the race game on the curve track at N = 10, one per module."""
    from dgsqp_amd.solver import DGSQP
    g = pm_game('curve', N=10)
    s = DGSQP(*g.solver_args(), print_method=None)
    yield g, s


# ---- 1. fixtures --------------------------------------------------------------------------------------------------------------------------
def _against_fixture(case, reg=None, **kw):
    from dgsqp_amd.solver import DGSQP
    kat, g, P = pk.load(case)
    if reg is not None:                                   # a solver parameter: no stage quantity reads it, no fixture stores it
        g = dataclasses.replace(g, params=copy.copy(g.params))
        g.params.reg = reg
    s = DGSQP(*g.solver_args(), print_method=None, **kw)
    if case in pk.DIRECTIONAL_CASES:
        assert s.dims.layout == pk.DIRECTIONAL_CASES[case]
    assert (s.n, s.n_c_total) == (kat['u'].shape[1], kat['l'].shape[1])
    ev = s.evaluate_batch(kat['x0'], kat['u'], kat['l'])
    worst = {}
    for b in range(len(kat['x0'])):
        errs = pk.compare(kat, b, {key: ev[key][b] for key in ('x', 'g', 'q', 'G', 'Q')}, pk.DEVICE_BAR, f'{case} device {kw or ""}')
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    MEASURED[(case, tuple(kw))] = worst
    print(f'{case} {kw or ""}: device against the exact answers, maxima over the scenarios: ' + ', '.join(f'{k} {e:.2e}' for k, e in worst.items()))


@pytest.mark.parametrize('case', pk.CASES)
def test_evaluate_against_the_exact_fixtures(case):
    _against_fixture(case)


def test_the_literal_game_on_the_256_thread_library():
    """The race game's own reg = 0 selects the classical QP kernels, which the 256-thread build does not hold (it refuses the game as too
    large: asserted); the stage quantities do not depend on reg, so the fixture is evaluated on a handle with reg = 1e-3."""
    with pytest.raises(RuntimeError, match='DG_BLOCK = 256'):
        _against_fixture('pm2_euler_N3', workgroups_per_cu=2, qp_method='active_set')
    _against_fixture('pm2_euler_N3', reg=1e-3, workgroups_per_cu=2, qp_method='active_set')


# ---- 2. solves ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('qp_method', ['active_set', 'osqp'])
def test_solves_of_the_race_game(qp_method):
    from dgsqp_amd.solver import DGSQP
    g = pm_game('curve', N=10)
    s = DGSQP(*g.solver_args(), print_method=None, qp_method=qp_method)
    par = s._cparams
    assert par.variant == 0
    x0, u_tm = scenarios(g, 8, 3)
    res = s.solve_batch(x0, u_tm)
    for key in DOUBLES:
        assert np.isfinite(res[key]).all(), key
    assert set(np.unique(res['status'])) <= KNOWN and (res['num_iters'] >= 0).all() and (res['num_iters'] <= par.sqp_iters).all()
    ev = s.evaluate_batch(x0, res['u'], res['l'])
    np.testing.assert_allclose(ev['x'], res['x'], rtol=pk.X_RTOL, atol=pk.X_ATOL)
    conv = np.nonzero(res['status'] <= 1)[0]
    print(f'point-mass race game, curve track, N = 10, {qp_method}: {len(conv)} of 8 scenarios converged; status {res["status"].tolist()}, '
          f'iterations {res["num_iters"].tolist()}')
    MEASURED[('converged', qp_method)] = len(conv)
    for b in conv:
        d = ev['q'][b] + ev['G'][b].T @ res['l'][b]
        cond = np.array([max(0.0, ev['g'][b].max()), np.abs(ev['g'][b] * res['l'][b]).max(), np.abs(d).max()])
        assert (res['l'][b] >= 0).all()
        if res['status'][b] == 0:
            assert cond[0] < par.p_tol and cond[1] < par.d_tol and cond[2] < par.d_tol, (b, cond)
        assert np.abs(cond - res['cond'][b]).max() < 1e-9, (b, cond, res['cond'][b])      # the same three maxima, summed in another order
    assert len(conv) >= 1


# ---- 3. step() ----------------------------------------------------------------------------------------------------------------------------
def test_three_receding_horizon_steps_are_three_batch_solves(race):
    from dgsqp_amd.solver import DGSQP
    from dgsqp_amd.types import VehicleState
    g, batch = race
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = scenarios(g, 1, 7)
    states = [VehicleState(t=0.0), VehicleState(t=0.0)]
    g.joint_model.qu2state(states, x0[0], None)
    s.set_warm_start(np.asarray(u_tm[0], float))
    x, ws = x0[0].copy(), np.asarray(u_tm[0], float)
    for k in range(3):
        assert np.array_equal(g.joint_model.state2q(states), x)
        info = s.step(states)
        ref = batch.solve_batch(x[None], ws[None])
        assert same(s._last_u_agent_major, ref['u'][0]) and same(s.q_pred, ref['x'][0].reshape(s.N + 1, s.n_q)) and same(s.l_pred, ref['l'][0]), k
        assert (info['msg'], info['num_iters']) == (ref['msg'][0], int(ref['num_iters'][0]))
        preds = s.get_prediction()
        for a, pr in enumerate(preds):
            q, u = s.q_pred[:, 6 * a:6 * a + 6], s.u_pred[:, 2 * a:2 * a + 2]
            for fld, col in (('x', 0), ('y', 1), ('v_long', 2), ('e_psi', 3), ('s', 4), ('x_tran', 5)):
                assert np.array_equal(np.array(getattr(pr, fld)), q[:, col]), (k, a, fld)
            assert np.array_equal(np.array(pr.u_a), u[:, 0]) and np.array_equal(np.array(pr.u_steer), u[:, 1])
            assert (states[a].u.u_a, states[a].u.u_steer) == (s.u_pred[0, 2 * a], s.u_pred[0, 2 * a + 1])
        if info['msg'] not in ('diverged', 'qp_fail'):
            ws = np.vstack((s.u_pred[1:], s.u_pred[-1]))
        x = s.q_pred[1].copy()                            # the model's own next state is the next start
        g.joint_model.qu2state(states, x, None)


# ---- 4. device PID warm start and sampler -------------------------------------------------------------------------------------------------
def test_pid_kernel_against_its_host_mirror(race):
    """The bar of test_pid_kernel_against_vectors_of_the_reference_controller: 1e-10 absolute on inputs and states."""
    from dgsqp_amd.montecarlo import pid_warm_start
    g, s = race
    x0, _ = scenarios(g, 8, 11)
    x0[:, 3] = np.linspace(-0.1, 0.1, 8)                  # e_psi of car 1 off zero: the law reads state 3
    x0[:, 6 + 5] += 0.05
    dev = s.pid_warm_start_batch(x0, du_max=(10.0, 4.5), want_trajectories=True)
    q_ws, u_ws = zip(*[pid_warm_start(m, x0[:, 6 * a:6 * a + 6], s.N, 0.1, du=(10.0, 4.5)) for a, m in enumerate(g.joint_model.dynamics_models)])
    u_ref, q_ref = np.concatenate(u_ws, axis=2), np.concatenate(q_ws, axis=2)
    eu, eq = np.abs(dev['u_ws'] - u_ref).max(), np.abs(dev['q_ws'].reshape(q_ref.shape) - q_ref).max()
    print(f'device PID warm start against the numpy mirror: inputs {eu:.2e}, states {eq:.2e} (bar 1e-10)')
    assert eu < 1e-10 and eq < 1e-10
    assert np.abs(u_ref[:, 0, 1]).max() > 0.05            # it steered on e_psi


def test_device_sampler_matches_its_host_mirror(race):
    """The bars of tests/test_gpu.py::test_device_sampler_matches_its_host_mirror: same candidates, x0 to 1e-12, warm starts to 1e-9."""
    from dgsqp_amd import sampler as smp
    g, s = race
    dev = s.sample_batch(g, 8, seed=11)
    x0, u_ws, used = smp.sample_scenarios_counter(g, 8, seed=11, chunk=64)
    assert dev['candidates'] == used, (dev['candidates'], used)
    assert np.abs(dev['x0'] - x0).max() < 1e-12 and np.abs(dev['u_ws'] - u_ws).max() < 1e-9
    assert (dev['x0'][:, [3, 9]] == 0).all() and (np.abs(dev['x0'][:, [5, 11]]) <= g.half_width).all()


# ---- 5. closed loop -----------------------------------------------------------------------------------------------------------------------
def check_plant_host(g, s, res, plant, entered, tag):
    """q[t+1] against the numpy ``fd`` of the chain's plant, one simulation step at a time from the device's own q[t] and u_plant[t];
    u_plant bit for bit against the delay lines of ``closed_loop.plant_feedback`` fed with ``entered`` (the command that entered the
    plant).  Returns Z [B, T, S, n_q], the mirror's state after every simulation step, for ``check_monitor``."""
    from dgsqp_amd import closed_loop
    P = s._problem
    pt = plant.lower(P)
    B, T = res['status'].shape
    S, M = pt.sim_steps, s.M
    jc = g.joint_model.model_config
    method = plant.method or jc.discretization_method
    sub = pt.substeps if method != 'euler' else 1
    cfgs = plant.dynamics_configs or [m.model_config for m in g.joint_model.dynamics_models]
    plants = [type(m)(0, dataclasses.replace(c, dt=jc.dt / S, discretization_method=method, M=sub), track=g.track)
              for m, c in zip(g.joint_model.dynamics_models, cfgs)]
    assert res['u_plant'].shape == (B, T, S, s.n_u)
    delay = [[pt.delay[a][j] for j in range(2)] for a in range(M)]
    Z = np.full((B, T, S, s.n_q), np.nan)
    worst = 0.0
    for b in range(B):
        lines = closed_loop.new_lines(delay)
        for t in range(int(res['steps_done'][b])):
            _, used, _ = closed_loop.plant_feedback(lambda q, u: q, res['q'][b, t], entered[b, t], lines, sim_steps=S)
            assert same(res['u_plant'][b, t], used), f'{tag}: u_plant of chain {b}, step {t} is not what its delay lines deliver'
            q = res['q'][b, t].copy()
            for j in range(S):
                for a, m in enumerate(plants):
                    q[6 * a:6 * a + 6] = m.fd(q[6 * a:6 * a + 6], res['u_plant'][b, t, j, 2 * a:2 * a + 2])
                Z[b, t, j] = q
            assert np.isfinite(q).all()
            worst = max(worst, float(np.abs(res['q'][b, t + 1] - q).max() / max(1.0, np.abs(q).max())))
    MEASURED[('plant', tag)] = worst
    print(f'{tag}: max |q[t+1] - host fd| / max(1, |q|_inf) = {worst:.3e} over {int(res["steps_done"].sum())} control steps (bar {BAR:g})')
    assert worst < BAR, (tag, worst)
    return Z


def test_closed_loop_identity_plant(race):
    from dgsqp_amd.closed_loop import PlantModel
    g, s = race
    x0, u_tm = scenarios(g, 6, 43)
    plain = s.step_batch(x0, u_tm, 3, keep_predictions=True)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel())
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)))
    assert teacher_force(s, res) == int(res['steps_done'].sum())
    check_plant_host(g, s, res, PlantModel(), res['u_applied'], 'point mass, identity plant')
    for key in KEYS + ('q',):
        assert same(res[key][:, 0], plain[key][:, 0]), key          # step 0 does not know about the plant
    assert (res['steps_done'] == 3).all()


def test_closed_loop_mismatched_plant(race):
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.dynamics import UnicycleConfig
    g, s = race
    x0, u_tm = scenarios(g, 6, 47)
    cfgs = [UnicycleConfig(dt=0.1, mass=2.366 * 1.2, damping_coefficient=0.15), UnicycleConfig(dt=0.1, mass=2.366 * 0.9, damping_coefficient=0.05)]
    plant = PlantModel(dynamics_configs=cfgs, method='rk4', M=2, sim_steps=2, delay_steps=[[0, 0], [0, 3]])
    res = s.step_batch(x0, u_tm, 4, keep_predictions=True, plant=plant)
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)))
    teacher_force(s, res)
    check_plant_host(g, s, res, plant, res['u_applied'], 'point mass, mismatched plant')
    ident = s.step_batch(x0, u_tm, 4, keep_predictions=True, plant=PlantModel())
    assert not same(ident['q'][:, 1], res['q'][:, 1])
    assert (res['u_plant'][:, 0, :, 3] == 0).all()        # the delayed channel delivers its empty line first


def test_closed_loop_pid_driver_with_the_monitor(race):
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g, s = race
    x0, u_tm = scenarios(g, 6, 53)
    plant = PlantModel(sim_steps=2)
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(ki_s=0.05, du_max=(10.0, 0.05)))
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, drivers=drivers, monitor=True)
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)))
    teacher_force(s, res)
    Z = check_plant_host(g, s, res, plant, res['u_cmd'], 'point mass, PID driver on car 2')
    check_monitor(s, res, Z, 'point mass, PID driver on car 2')
    assert same(res['u_cmd'][:, :, :2], res['u_applied'][:, :, :2]) and not same(res['u_cmd'][:, :, 2:], res['u_applied'][:, :, 2:])
    # the first command of the lane follower by hand: references from x0, so e = e_psi (state 3 of car 2) = 0 and v = v_ref
    assert (res['u_cmd'][:, 0, 2:] == 0).all()
    # ... and its second one from the plant's state: speed P on v - v0, steering PI on 5 (x_tran - x_tran0) + e_psi, rate 0.05
    q1, q0 = res['q'][:, 1, 6:], x0[:, 6:]
    e = 5.0 * (q1[:, 5] - q0[:, 5]) + q1[:, 3]
    want = np.stack([np.clip(-(q1[:, 2] - q0[:, 2]), -2.1, 2.1), np.clip(-(e + 0.05 * np.clip(e * 0.1, -100, 100)), -0.05, 0.05)], axis=1)
    np.testing.assert_allclose(res['u_cmd'][:, 1, 2:], want, rtol=0, atol=1e-12)


def test_closed_loop_held_plan_with_u_prev(race):
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    g, s = race
    x0, u_tm = scenarios(g, 6, 59)
    plant, hold = PlantModel(), PlanHold(replan_every=2)
    res = s.step_batch(x0, u_tm, 4, keep_predictions=True, plant=plant, hold=hold, u_prev=True)
    n_solved, n_held = check_plan_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), hold)
    assert teacher_force_solved(s, res) == n_solved
    check_plant_host(g, s, res, plant, res['u_game'], 'point mass, plan held for two steps, u_prev carried')
    assert n_held > 0 and n_solved > 0 and 'u_prev' in res
    print(f'{n_solved} solved and {n_held} held steps')


# ---- 6. coexistence -----------------------------------------------------------------------------------------------------------------------
def test_a_bicycle_handle_and_a_point_mass_handle_in_one_process(race):
    """The game lives in one __constant__ block: two handles of games that differ in nothing the state count shows, used alternately,
    must each give what a fresh handle of their own gives."""
    from dgsqp_amd.montecarlo import kinematic_racing_game
    from dgsqp_amd.solver import DGSQP
    gp, _ = race
    gk = kinematic_racing_game('curve', N=10)
    fresh = {}
    batches = {'kin': scenarios(gk, 4, 61), 'pm': scenarios(gp, 4, 61)}
    for name, g in (('kin', gk), ('pm', gp)):
        s = DGSQP(*g.solver_args(), print_method=None)
        fresh[name] = (s.solve_batch(*batches[name]), s.step_batch(*batches[name], 2, keep_predictions=True))
        del s
    sk, sp = DGSQP(*gk.solver_args(), print_method=None), DGSQP(*gp.solver_args(), print_method=None)
    for _ in range(2):
        for name, s in (('kin', sk), ('pm', sp)):
            got = s.solve_batch(*batches[name])
            for key in KEYS:
                assert same(got[key], fresh[name][0][key]), (name, key)
        for name, s in (('pm', sp), ('kin', sk)):
            got = s.step_batch(*batches[name], 2, keep_predictions=True)
            for key in KEYS + ('q', 'u_ws'):
                assert same(got[key], fresh[name][1][key]), (name, key)
    assert not same(fresh['kin'][0]['x'], fresh['pm'][0]['x'])


# ---- 7. refusals through the raw ABI ------------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi(race):
    from dgsqp_amd import _ffi
    from dgsqp_amd.dynamics import CasadiDecoupledMultiAgentDynamicsModel
    from dgsqp_amd.solver import build_params, build_problem
    from dgsqp_amd.tracks import get_track
    g, s = race
    lib, h = s._lib, s._h
    msg = lambda: lib.dgsqp_last_error(h).decode()
    par = build_params(g.params)

    def create(P):
        out = ctypes.c_void_p()
        rc = lib.dgsqp_create(ctypes.byref(P), ctypes.byref(par), 0, ctypes.byref(out))
        text = lib.dgsqp_last_error(out).decode() if out else ''
        if out:
            lib.dgsqp_destroy(out)
        return rc, text

    def planned(P):
        d, buf = _ffi.DimsT(), ctypes.create_string_buffer(256)
        return lib.dgsqp_plan(ctypes.byref(P), ctypes.byref(par), ctypes.byref(d), buf, 256), buf.value.decode()
    # a spline track: dgsqp_plan and dgsqp_create agree
    f1 = get_track('f1_austin_tenth_scale')
    models = [type(m)(0, m.model_config, track=f1) for m in g.joint_model.dynamics_models]
    gs = dataclasses.replace(g, joint_model=CasadiDecoupledMultiAgentDynamicsModel(0, models, g.joint_model.model_config), track=f1)
    Ps = build_problem(*gs.solver_args())
    rc_p, text_p = planned(Ps)
    rc_c, _ = create(Ps)
    assert rc_p == rc_c == _ffi_E_ARG and 'arc tracks only' in text_p
    P4 = build_problem(*g.solver_args())
    P4.agents[0].model = 4
    assert planned(P4)[0] == create(P4)[0] == _ffi_E_ARG and 'unsupported vehicle model' in planned(P4)[1]
    # allowed: the racing costs, and the game itself
    P = build_problem(*g.solver_args())
    P.agents[1].w_block = 0.3
    assert planned(P)[0] == 0 and create(P)[0] == 0
    # a plant of another class than the game's agent: the kinematic bicycle has the same six states
    pt = _ffi.PlantT()
    pt.sim_steps, pt.integrator, pt.substeps, pt.use_game_agents = 1, 0, 1, 0
    for a in range(2):
        ctypes.memmove(ctypes.byref(pt.agents[a]), ctypes.byref(s._problem.agents[a]), ctypes.sizeof(_ffi.VehicleT))
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0
    for other in (0, 1, 2):
        pt.agents[1].model = other
        assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == -1 and f'model class {other}' in msg() and "the game's is 3" in msg(), msg()
    assert lib.dgsqp_set_plant(h, None) == 0
    # ... and the same for a per-chain vehicle
    pt.agents[1].model = 3
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0
    vehicles = (_ffi.VehicleT * 4)()
    for i in range(4):
        ctypes.memmove(ctypes.byref(vehicles[i]), ctypes.byref(s._problem.agents[i % 2]), ctypes.sizeof(_ffi.VehicleT))
    assert lib.dgsqp_set_plant_ensemble(h, 2, vehicles, None) == 0
    vehicles[3].model = 0
    assert lib.dgsqp_set_plant_ensemble(h, 2, vehicles, None) == -1 and msg().startswith('plant ensemble: ') and 'model class 0' in msg(), msg()
    assert lib.dgsqp_set_plant_ensemble(h, 0, None, None) == 0 and lib.dgsqp_set_plant(h, None) == 0
    # the handle still solves what it solved
    x0, u_tm = scenarios(g, 2, 3)
    a, b = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm)
    assert all(same(a[k], b[k]) for k in KEYS)


_ffi_E_ARG = -1
