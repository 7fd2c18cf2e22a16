"""A plant of its own in closed-loop batches on the device: DGSQP.step_batch(..., plant=PlantModel(...)) / dgsqp_set_plant
(dev_plant_feedback, csrc/dgsqp_closed_loop.h).

Every case first repeats the two checks of tests/test_closed_loop.py (the helpers are those of tests/closed_loop_checks.py) -- TEACHER
FORCING (every step that ran is, bit for bit, the ``solve_batch`` solve from the recorded (q[t], u_ws[t]): a plant only changes which state is fed back) and the warm-start chain with the
records of steps that never ran.  Then the plant itself:

* ``q[t+1]`` against the CPU oracle's next state (``oracle.dynamics`` on a copy of the game's POD with dt / S, the plant's integrator,
  sub-steps and vehicle fields), applied one control step at a time from the device's own ``q[t]`` and ``u_plant[t]`` so that errors do
  not compound along a chain: 1e-12 relative to max(1, |q|_inf), the device-against-oracle bar for x;
* ``u_plant`` against the delay lines of the host mirror ``closed_loop.plant_feedback``: bit for bit, it is data movement."""
import numpy as np
import pytest

from closed_loop_checks import (BAR, COUNTS, DELAYS, DOUBLES, check_chain, check_plant, configs_of, same, scenarios, solver_of,
                                 teacher_force)      # noqa: F401  (solver_of is a fixture)
from conftest import agent_major

pytestmark = pytest.mark.gpu


def run_and_check(oracle, s, x0, u_tm, T, plant, w=None, tag=''):
    res = s.step_batch(x0, u_tm, T, disturbance=w, keep_predictions=True, plant=plant)
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)))
    teacher_force(s, res)
    check_plant(oracle, s, res, plant, w, tag)
    return res


def test_identity_plant(oracle, games, solver_of):
    """Case 1: the game's own parameters, integrator and sub-steps, S = 1, no delay: the plant IS stage 1 of the prediction."""
    from dgsqp_amd.closed_loop import PlantModel
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 6, 41)
    w = 1e-3 * np.random.default_rng(5).standard_normal((6, 4, s.n_q))
    res = run_and_check(oracle, s, x0, u_tm, 4, PlantModel(), w, 'identity kb_curve_N10')
    assert (res['steps_done'] == 4).all()
    want = res['x'][:, :, 1] + w
    assert np.abs(res['q'][:, 1:] - want).max() / max(1.0, np.abs(want).max()) < BAR
    assert same(res['u_plant'][:, :, 0], res['u_applied'])
    # without keep_predictions: the same chain
    lean = s.step_batch(x0, u_tm, 4, disturbance=w, plant=PlantModel())
    assert 'x' not in lean and 'l' not in lean
    for key in ('q', 'u_ws', 'u', 'cond', 'cost', 'u_applied', 'u_plant') + COUNTS + ('steps_done',):
        assert same(lean[key], res[key]), key


def test_mismatch_and_finer_integration(oracle, games, solver_of):
    """Case 2: mass x 1.2, drag x 1.5, rk4 with 3 sub-steps, 2 simulation steps per control step (the game integrates with euler)."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2, drag_coefficient=1.5), method='rk4', M=3, sim_steps=2)
    res = run_and_check(oracle, s, x0, u_tm, 3, plant, tag='mismatch kb_curve_N10')
    assert (res['steps_done'] == 3).all()
    gap = np.abs(res['q'][:, 1:] - res['x'][:, :, 1]).max(axis=(1, 2))
    assert (gap > 1e-6).all(), gap                                     # the mismatch really entered, on every chain
    for integ in ('rk2', 'rk3', 'euler'):                               # the other integrators, one control step each
        run_and_check(oracle, s, x0[:2], u_tm[:2], 1, PlantModel(dynamics_configs=plant.dynamics_configs, method=integ, M=2, sim_steps=3),
                      tag=f'mismatch kb_curve_N10 {integ}')


def test_input_delay(oracle, games, solver_of):
    """Case 3: S = 2, delays [[2, 1], [0, 3]] simulation steps, T = 4."""
    from dgsqp_amd.closed_loop import PlantModel
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 4, 47)
    plant = PlantModel(sim_steps=2, delay_steps=DELAYS)
    res = run_and_check(oracle, s, x0, u_tm, 4, plant, tag='delay kb_curve_N10')
    assert (res['steps_done'] == 4).all()
    up, ua = res['u_plant'], res['u_applied']
    # the first control step integrates under zeros where the line says so ...
    assert not up[:, 0, :, 0].any() and not up[:, 0, :, 3].any() and not up[:, 0, 0, 1].any()
    assert same(up[:, 0, 1, 1], ua[:, 0, 1]) and same(up[:, 0, :, 2], np.repeat(ua[:, 0, None, 2], 2, axis=1))
    # ... and the lines carry over between control steps: simulation step 2 t + j sees the input appended d simulation steps earlier
    for ch, d in enumerate(np.reshape(DELAYS, -1)):
        flat = up[:, :, :, ch].reshape(4, 8)
        want = np.concatenate((np.zeros((4, d)), np.repeat(ua[:, :, ch], 2, axis=1)), axis=1)[:, :8]
        assert same(flat, want), ch
    assert ua[:, 0].all() and ua[:, 1].all()                           # (none of those inputs is a zero of its own)


def test_delay_lines_are_reset_for_every_chain(oracle, games, solver_of):
    """Case 3, B = 600 > the grid: a workgroup starts a second chain after finishing a first one; a line carried over from the first
    chain would show in u_plant of the second (non-zero where its line must still deliver zeros) and in everything after it.  The last
    chains of the batch, run again as a batch of four, must give bit-identical results."""
    from dgsqp_amd.closed_loop import PlantModel
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 600, 47)
    plant = PlantModel(sim_steps=2, delay_steps=DELAYS)
    res = s.step_batch(x0, u_tm, 2, keep_predictions=True, plant=plant)
    check_chain(s, res, x0, agent_major(u_tm))
    assert teacher_force(s, res) == 1200
    assert not res['u_plant'][:, 0, :, 0].any() and not res['u_plant'][:, 0, :, 3].any() and not res['u_plant'][:, 0, 0, 1].any()
    few = s.step_batch(x0[-4:], u_tm[-4:], 2, keep_predictions=True, plant=plant)
    check_plant(oracle, s, few, plant, tag='delay kb_curve_N10, last 4 of 600')
    for key in DOUBLES + COUNTS + ('q', 'u_ws', 'u_applied', 'u_plant', 'steps_done'):
        assert same(res[key][-4:], few[key]), key


def test_dynamic_bicycle(oracle, games, solver_of):
    """Case 4: dyn_curve_N15; Pacejka D x 0.8 on car 2, linear tyres on car 1, S = 2, 5 sub-steps."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['dyn_curve_N15'][0]
    s = solver_of('dyn_curve_N15')
    cfgs = configs_of(g, pacejka_d_front={1: 0.8}, pacejka_d_rear={1: 0.8})
    cfgs[0].tire_model = 'linear'
    plant = PlantModel(dynamics_configs=cfgs, M=5, sim_steps=2)
    pt = plant.lower(s._problem)
    assert (pt.agents[0].tire_model, pt.agents[1].tire_model, pt.integrator) == (1, 0, 1)
    x0, u_tm = scenarios(g, 4, 53)
    res = run_and_check(oracle, s, x0, u_tm, 3, plant, tag='dyn_curve_N15')
    assert (np.abs(res['q'][:, 1] - res['x'][:, 0, 1]).max(axis=1) > 1e-6).all()


def test_unicycle(oracle, games, solver_of):
    """Case 5: merge_N8, three cars, mass x 1.3, euler plant (the game integrates with rk3)."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['merge_N8'][0]
    s = solver_of('merge_N8')
    assert s.M == 3
    x0, u_tm = scenarios(g, 4, 53)
    run_and_check(oracle, s, x0, u_tm, 3, PlantModel(dynamics_configs=configs_of(g, mass=1.3), method='euler'), tag='merge_N8')


def test_spline_track(oracle):
    """Case 6: the F1 game at N = 12 (test_f1_spline_track_game's), rk4 with 2 sub-steps."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=12, model='kinematic', rk4_substeps=3)
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    assert s._problem.track_kind == 1
    x0, u_tm = mc.sample_scenarios(g, 3, seed=0)
    run_and_check(oracle, s, x0, u_tm, 2, PlantModel(method='rk4', M=2, delay_steps=[[1, 0], [0, 0]]), tag='f1 N12')


def test_xl_layout(oracle):
    """Case 7a: kin3_N25_dir (n = 150, XL layout), a plant with delay: it must not disturb the solve's scratch; teacher forcing proves it."""
    import multistage_kat as mk
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.solver import DGSQP
    g = mk.build_game('kin3_N25_dir')
    s = DGSQP(*g.solver_args(), print_method=None)
    assert s.dims.layout == 2 and s.n == 150
    x0, u_tm = scenarios(g, 2, 59)
    run_and_check(oracle, s, x0, u_tm, 2, PlantModel(method='rk4', M=2, sim_steps=2, delay_steps=[[1, 2], [0, 1], [3, 0]]), tag='kin3_N25_dir')


def test_half_arena_build(oracle, games, solver_of):
    """Case 7b: libdgsqp_hip_b256.so (256-thread workgroups, two per CU)."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_chicane_N15'][0]
    s = solver_of('kb_chicane_N15', workgroups_per_cu=2)
    x0, u_tm = scenarios(g, 4, 61)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    run_and_check(oracle, s, x0, u_tm, 3, plant, tag='kb_chicane_N15 b256')


def test_v2(oracle):
    """Case 7c: DG-SQP v2 through DGSQPV2."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.solver_types import DGSQPV2Params
    from dgsqp_amd.solver_v2 import DGSQP as DGSQPV2
    g = mc.kinematic_racing_game('curve', N=12)
    g.params = DGSQPV2Params(dt=0.1, N=12)
    g.params.time_limit = None
    s = DGSQPV2(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    assert s._cparams.variant == 1
    x0, u_tm = scenarios(g, 3, 2)
    run_and_check(oracle, s, x0, u_tm, 2, PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk2', M=2, delay_steps=1), tag='v2 kb_curve_N12')


def test_chain_end_on_a_non_finite_plant_state(oracle, games, solver_of):
    """Case 8: disturbance[1, 1, :] = nan ends chain 1 after two steps, as without a plant; the others are bit-identical to a clean run."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 3, 43)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    w = np.zeros((3, 4, s.n_q))
    clean = run_and_check(oracle, s, x0, u_tm, 4, plant, w, 'chain end, clean')
    w[1, 1, :] = np.nan
    res = run_and_check(oracle, s, x0, u_tm, 4, plant, w, 'chain end')
    assert res['steps_done'].tolist() == [4, 2, 4] and clean['steps_done'].tolist() == [4, 4, 4]
    assert res['msg'][1][2:] == ['not_run', 'not_run'] and (res['status'][1, 2:] == -1).all()
    assert np.isnan(res['q'][1, 2:]).all() and np.isnan(res['u_ws'][1, 2:]).all() and np.isnan(res['u_plant'][1, 2:]).all()
    for key in DOUBLES + COUNTS + ('q', 'u_ws', 'u_applied', 'u_plant'):
        assert same(res[key][[0, 2]], clean[key][[0, 2]]), key
        assert same(res[key][1, :2], clean[key][1, :2]), key          # ... and chain 1 itself up to its end
    assert same(res['q'][1, 1], clean['q'][1, 1]) and np.isnan(res['q'][1, 2]).all()


def test_coexistence(oracle, games, solver_of):
    """Case 9: step_batch without a plant, with one, without again: the first and the third are bit-identical, the second differs, and
    solve_batch in between is unchanged.  A plant lasts for the call it was given to."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 67)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    sol_a = s.solve_batch(x0, u_tm)
    first = s.step_batch(x0, u_tm, 3, keep_predictions=True)
    sol_b = s.solve_batch(x0, u_tm)
    second = run_and_check(oracle, s, x0, u_tm, 3, plant, tag='coexistence')
    sol_c = s.solve_batch(x0, u_tm)
    third = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=None)
    assert 'u_plant' not in first and 'u_plant' not in third and 'u_plant' in second
    for key in DOUBLES + COUNTS + ('q', 'u_ws', 'u_applied', 'steps_done'):
        assert same(first[key], third[key]), key
    assert same(first['q'][:, 1], first['x'][:, 0, 1]) and not same(second['q'][:, 1], second['x'][:, 0, 1])
    for key in DOUBLES + COUNTS:
        assert same(sol_a[key], sol_b[key]) and same(sol_a[key], sol_c[key]), key
        assert same(second[key][:, 0], sol_a[key]), key               # step 0 is that very solve, plant or not


def test_argument_errors_through_the_c_abi(games, solver_of):
    """Case 10: DGSQP_E_ARG and a message for every invalid field of dgsqp_plant_t; nothing of it reaches the next launch."""
    import ctypes
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    lib, h = s._lib, s._h
    x0, u_tm = scenarios(g, 2, 73)
    good = lambda: PlantModel(dynamics_configs=configs_of(g), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS).lower(s._problem)

    def refused(change, word):
        pt = good()
        change(pt)
        assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == -1
        msg = lib.dgsqp_last_error(h).decode()
        assert msg.startswith('plant: ') and word in msg, msg

    refused(lambda pt: setattr(pt, 'integrator', 7), 'integrator')
    refused(lambda pt: setattr(pt, 'integrator', -1), 'integrator')
    refused(lambda pt: setattr(pt, 'substeps', 0), 'substeps')
    refused(lambda pt: setattr(pt, 'sim_steps', 0), 'sim_steps')
    refused(lambda pt: pt.delay[1].__setitem__(0, _ffi.MAX_DELAY + 1), 'delay')
    refused(lambda pt: pt.delay[0].__setitem__(1, -1), 'delay')
    refused(lambda pt: setattr(pt.agents[1], 'model', 1), 'model class')
    # a refused plant leaves the handle as it was: no plant
    base = s.step_batch(x0, u_tm, 2)
    assert 'u_plant' not in base
    # entries beyond the game's agents are not read; with use_game_agents neither is agents[]
    pt = good()
    pt.delay[5][0] = 99
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0 and lib.dgsqp_set_plant(h, None) == 0
    pt = PlantModel().lower(s._problem)
    pt.agents[0].model = 1
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0 and lib.dgsqp_set_plant(h, None) == 0
    assert lib.dgsqp_set_plant(None, None) == -1
    # the fetch: a buffer that is too small, a NULL buffer
    res = s.step_batch(x0, u_tm, 2, plant=PlantModel(sim_steps=2))
    buf = np.empty(res['u_plant'].size)
    assert lib.dgsqp_fetch_u_plant(h, _ffi.dptr(buf), buf.size - 1) == -1 and 'too small' in lib.dgsqp_last_error(h).decode()
    assert lib.dgsqp_fetch_u_plant(h, None, buf.size) == -1
    assert lib.dgsqp_fetch_u_plant(h, _ffi.dptr(buf), buf.size) == 0
    assert same(buf.reshape(2, 2, 2, s.n_u).swapaxes(0, 1), res['u_plant'])
    # PlantModel refuses the same things before the library sees them, and step_batch leaves no plant behind when it raises
    with pytest.raises(ValueError):
        s.step_batch(x0, u_tm, 2, plant=PlantModel(sim_steps=0))
    again = s.step_batch(x0, u_tm, 2)
    for key in ('q', 'u', 'u_ws') + COUNTS:
        assert same(again[key], base[key]), key
