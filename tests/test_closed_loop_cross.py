"""A plant of another model class than the game's on the device: DGSQP.step_batch(..., plant=PlantModel(..., own_class=True), z0=...) /
dgsqp_set_cross_plant, dgsqp_fetch_plant_state, dgsqp_fetch_track_ref and DGSQP_DRIVER_TRACK (the DgCrossPack instantiation of
dg_closed_loop_kernel, csrc/dgsqp_closed_loop.h).  The plant keeps a state z of its own, the game sees q = p(z); a 'track' driver follows
the game's plan with the lane follower.  The checks common to every case are those of tests/closed_loop_cross_checks.py."""
import ctypes

import numpy as np
import pytest

from closed_loop_checks import CHAIN, COUNTS, DELAYS, DOUBLES, check_monitor, configs_of, same, scenarios, solver_of      # noqa: F401  (solver_of is a fixture)
from closed_loop_cross_checks import check_cross, plant_bases

pytestmark = pytest.mark.gpu

PLANT_KW = dict(method='rk4', M=3, sim_steps=2, delay_steps=DELAYS)
VY, W = 3, 4                    # of an 8-state block


@pytest.fixture(scope='module')
def bases():
    return plant_bases()


@pytest.fixture(scope='module')
def pm(games):
    """The point-mass race game on the curve track and its solver, built once."""
    from dgsqp_amd.montecarlo import point_mass_racing_game
    from dgsqp_amd.solver import DGSQP
    g = point_mass_racing_game('curve', N=10)
    return g, DGSQP(*g.solver_args(), print_method=None)


def dyn_configs(M=2):
    """The Pacejka vehicle of the comparison studies (montecarlo.dynamic_racing_game)."""
    from dgsqp_amd.dynamics import DynamicBicycleConfig
    return [DynamicBicycleConfig(dt=0.1, model_name='dynamic_bicycle', noise=False, discretization_method='rk4', simple_slip=False,
                                 tire_model='pacejka', mass=2.2187, yaw_inertia=0.02723, wheel_friction=0.9, pacejka_b_front=5.0,
                                 pacejka_b_rear=5.0, pacejka_c_front=2.28, pacejka_c_rear=2.28, M=4) for _ in range(M)]


def kin_configs(M=2):
    from dgsqp_amd.dynamics import KinematicBicycleConfig
    return [KinematicBicycleConfig(dt=0.1, model_name='kinematic_bicycle', noise=False, discretization_method='rk4', code_gen=False) for _ in range(M)]


@pytest.mark.parametrize('which', ['kb_curve_N10', 'point mass'])
def test_identity_cross_plant_is_the_plant_of_the_games_class(oracle, games, solver_of, pm, bases, which):
    """Case 1: own_class=True with the game's classes: every shared record equals the plain plant's bit for bit, and z == q."""
    from dgsqp_amd.closed_loop import PlantModel
    g, s = (games[which][0], solver_of(which)) if which != 'point mass' else pm
    x0, u_tm = scenarios(g, 4, 41)
    plain = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel(**PLANT_KW))
    plant = PlantModel(own_class=True, **PLANT_KW)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant)
    for key in CHAIN + ('u_pred', 'converged'):
        assert same(res[key], plain[key]), key
    assert res['msg'] == plain['msg'] and same(res['z'], res['q']) and 'track_ref' not in res and 'z' not in plain
    assert same(res['u_cmd'], res['u_applied']) and (res['plan_stage'] == 0).all()
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, tag=f'identity cross plant, {which}')
    # with the game's own configs named the plant is the same one
    named = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel(dynamics_configs=configs_of(g), own_class=True, **PLANT_KW))
    for key in CHAIN + ('z',):
        assert same(named[key], res[key]), key


def test_kinematic_game_on_dynamic_plants(oracle, games, solver_of, bases):
    """Case 2: the kinematic game's solution applied to Pacejka bicycles, no drivers argument (all GAME)."""
    from dgsqp_amd.closed_loop import PlantModel
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    B, T = 5, 4
    x0, u_tm = scenarios(g, B, 43)
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, **PLANT_KW)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, tag='kinematic game on dynamic plants')
    assert res['z'].shape == (B, T + 1, 16) and (res['steps_done'] == T).all()
    vyw = res['z'][:, 1:][..., [VY, W, 8 + VY, 8 + W]]
    assert (vyw != 0).any() and np.isfinite(vyw).all()                      # the plant really has a state of its own
    assert same(res['u_cmd'], res['u_game'])


@pytest.mark.parametrize('cls', ['kinematic', 'dynamic'])
def test_point_mass_game_tracked_on_bicycles(oracle, pm, bases, cls):
    """Case 3: the race demo's planning game, both cars following their plan with the TRACK driver on bicycles; without drivers the launch
    is refused, since a point mass's (Fx, wz) cannot command a bicycle."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    g, s = pm
    B, T = 4, 4
    x0, u_tm = scenarios(g, B, 47)
    plant = PlantModel(dynamics_configs=kin_configs() if cls == 'kinematic' else dyn_configs(), own_class=True, method='rk4', M=2, sim_steps=2)
    drivers = Drivers(kinds=['track', 'track'])
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=drivers)
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, drivers=drivers, tag=f'point-mass game tracked on {cls} plants')
    assert (res['steps_done'] == T).all() and np.isfinite(res['track_ref']).all() and res['track_ref'].shape == (B, T, 2, 3)
    assert not same(res['u_cmd'], res['u_game'])
    with pytest.raises(ValueError, match='agent 0'):                        # (the host layer's own refusal)
        s.step_batch(x0, u_tm, T, plant=plant)
    pt = plant.lower(s._problem)
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import lift_state
    z0 = lift_state([3, 3], plant.plant_classes(s._problem), x0)
    assert s._lib.dgsqp_set_cross_plant(s._h, ctypes.byref(pt), B, _ffi.dptr(z0)) == 0
    try:
        rc, _ = raw_launch(s, x0, s._to_agent_major(u_tm), T)
        msg = s._lib.dgsqp_last_error(s._h).decode()
        assert rc == -1 and msg.startswith('drivers: ') and 'agent 0' in msg, msg
    finally:
        assert s._lib.dgsqp_set_cross_plant(s._h, None, 0, None) == 0


def raw_launch(s, x0, u_am, T, w=None):
    from dgsqp_amd import _ffi
    from dgsqp_amd.solver import _record_ptrs
    B = len(x0)
    sm = dict(q=np.empty((T + 1, B, s.n_q)), u_ws=np.empty((T + 1, B, s.n)), **s._records((T, B), predictions=False))
    done = np.empty(B, np.int32)
    rc = s._lib.dgsqp_closed_loop_batch(s._h, B, T, _ffi.dptr(x0), _ffi.dptr(u_am), _ffi.dptr(w), _ffi.dptr(sm['q']), _ffi.dptr(sm['u_ws']),
                                        *_record_ptrs(sm), _ffi.iptr(done), None)
    return rc, dict(sm, steps_done=done)


def test_mixed_with_the_other_settings_at_once(oracle, games, solver_of, bases):
    """Case 4: car 1 TRACK on a dynamic plant, car 2 PID on its kinematic one; a vehicle and delays per chain, the monitor, estimate noise,
    a plan every second step and the carried u_prev (the kinematic game has rate rows)."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlanHold, PlantModel, perturbed_configs
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    B, T = 4, 4
    x0, u_tm = scenarios(g, B, 61)
    cfgs = [dyn_configs(1)[0], configs_of(g)[1]]
    delays = np.array([[[2, 1], [0, 3]], [[0, 0], [1, 1]], [[1, 2], [2, 0]], [[3, 0], [0, 1]]])
    plant = PlantModel(dynamics_configs=cfgs, per_chain_configs=perturbed_configs(cfgs, dict(mass=0.1), B, seed=1), per_chain_delay_steps=delays,
                       method='rk4', M=2, sim_steps=2, own_class=True)
    drivers = Drivers(kinds=['track', 'pid'], pid=PidGains(ki_s=0.05, du_max=(10.0, 0.05)))
    hold = PlanHold(replan_every=2)
    v = 1e-3 * np.random.default_rng(5).standard_normal((B, T, s.n_q))
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=drivers, hold=hold, monitor=True, estimate_noise=v, u_prev=True)
    assert {'z', 'track_ref', 'u_game', 'plan_stage', 'u_cmd', 'u_plant', 'u_prev', 'q_est', 'clearance', 'box_excess', 'hit_step'} <= set(res)
    m = check_cross(oracle, s, res, g, x0, u_tm, plant, bases, drivers=drivers, hold=hold, tag='mixed: track + pid, vehicles, delays, monitor, noise, hold, u_prev')
    check_monitor(s, res, m['Z'], 'mixed, monitor on projected states')
    assert m['held'] >= B and (res['steps_done'] == T).all() and res['z'].shape[-1] == 14
    solved = res['status'] >= 0
    assert same(res['q_est'][solved], (res['q'][:, :T] + v)[solved]) and np.isnan(res['q_est'][~solved]).all()
    # the carry: the TRACK agent's u_prev is the GAME's command, the PID agent's its own
    assert same(res['u_prev'][:, 0], np.zeros((B, s.n_u)))
    assert same(res['u_prev'][:, 1:, :2], res['u_game'][:, :T - 1, :2]) and same(res['u_prev'][:, 1:, 2:], res['u_cmd'][:, :T - 1, 2:])
    assert not same(res['u_cmd'][:, :, :2], res['u_game'][:, :, :2])
    assert np.isfinite(res['track_ref'][:, :, 0]).all() and np.isnan(res['track_ref'][:, :, 1]).all()


def test_no_state_survives_beyond_the_grid(oracle, games, solver_of, bases):
    """Case 5: 600 identical chains on a grid smaller than B (a workgroup starts further chains after its first): every chain equals the
    first record for record, so no delay line, PID state or (age, due) survives a workgroup's previous chain."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlanHold, PlantModel
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    x1, u1 = scenarios(g, 1, 41)
    x0, u_tm = np.tile(x1, (600, 1)), np.tile(u1, (600, 1, 1))
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    drivers, hold = Drivers(kinds=['track', 'pid'], pid=PidGains(ki_s=0.05)), PlanHold(replan_every=2)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, drivers=drivers, hold=hold)
    keys = CHAIN + DOUBLES + COUNTS + ('u_game', 'plan_stage', 'u_pred', 'msg', 'converged', 'z', 'u_cmd', 'track_ref')
    few = {k: v[:2] for k, v in res.items() if k in keys}
    m = check_cross(oracle, s, few, g, x0[:2], u_tm[:2], plant, bases, drivers=drivers, hold=hold, tag='beyond the grid, first 2 of 600')
    assert m['held'] == 2 and (res['steps_done'] == 3).all()
    for key in CHAIN + ('u_game', 'plan_stage', 'z', 'u_cmd', 'track_ref'):
        assert same(res[key], np.tile(res[key][:1], (600,) + (1,) * (res[key].ndim - 1))), key


def test_a_non_finite_plant_state_ends_its_chain(oracle, games, solver_of, bases):
    """Case 6: vy of chain 1 is NaN in z0.  The projection drops it, so solve 0 runs from a finite state; the plant's next state is not
    finite and the chain ends with steps_done = 1.  The other chains do not notice.  A NaN replay entry ends one chain in the same way."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel, lift_state
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10')
    B, T = 3, 3
    x0, u_tm = scenarios(g, B, 67)
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, method='rk4', M=2, sim_steps=2)
    clean = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    z0 = lift_state([0, 0], [1, 1], x0)
    z0[1, VY] = np.nan
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, z0=z0)
    assert res['steps_done'].tolist() == [T, 1, T] and not np.isfinite(res['z'][1, 1]).all() and np.isnan(res['z'][1, 2:]).all()
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, z0=z0, tag='NaN vy in z0 of chain 1')
    for key in CHAIN + ('z', 'u_cmd', 'u_game'):
        assert same(res[key][[0, 2]], clean[key][[0, 2]]), key
    rep = np.zeros((B, T, s.n_u))
    rep[2, 1, 3] = np.nan
    drivers = Drivers(kinds=['game', 'replay'], u_replay=rep)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=drivers)
    assert res['steps_done'].tolist() == [T, T, 2] and not np.isfinite(res['z'][2, 2]).all() and np.isnan(res['z'][2, 3]).all()
    assert np.isnan(res['u_cmd'][2, 1, 3]) and np.isnan(res['u_plant'][2, 1, :, 3]).all()
    rep[2, 1, 3] = 0.0
    fine = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=Drivers(kinds=['game', 'replay'], u_replay=rep))
    check_cross(oracle, s, fine, g, x0, u_tm, plant, bases, drivers=Drivers(kinds=['game', 'replay'], u_replay=rep), tag='replay on car 2')
    for key in [k for k in CHAIN if k != 'steps_done'] + ['z', 'u_cmd', 'u_game']:      # (the solve of step 1 ran before the NaN entered the plant)
        assert same(res[key][:2], fine[key][:2]) and same(res[key][2, :1], fine[key][2, :1]), key
    assert same(res['z'][2, :2], fine['z'][2, :2]) and same(res['u'][2, :2], fine['u'][2, :2])


def test_the_256_thread_build(oracle, games, solver_of, bases):
    """Case 7a: two workgroups per CU."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    g, s = games['kb_curve_N10'][0], solver_of('kb_curve_N10', workgroups_per_cu=2)
    x0, u_tm = scenarios(g, 3, 71)
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, **PLANT_KW)
    drivers = Drivers(kinds=['game', 'track'])
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, drivers=drivers)
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, drivers=drivers, tag='256-thread build')
    assert (res['steps_done'] == 3).all()


def test_the_spline_track(oracle):
    """Case 7b: the kinematic game on the F1 spline track, dynamic plants."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    from dgsqp_amd.montecarlo import f1_racing_game
    from dgsqp_amd.solver import DGSQP
    g = f1_racing_game(N=10)
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = scenarios(g, 3, 73)
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, method='rk4', M=2, sim_steps=2)
    drivers = Drivers(kinds=['game', 'track'])
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, drivers=drivers)
    check_cross(oracle, s, res, g, x0, u_tm, plant, plant_bases('f1'), drivers=drivers, tag='spline track')
    assert (res['steps_done'] >= 1).all()


def test_dgsqp_v2(oracle, bases):
    """Case 7c: a DG-SQP v2 kinematic game."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.solver_types import DGSQPV2Params
    from dgsqp_amd.solver_v2 import DGSQP as DGSQPV2
    g = mc.kinematic_racing_game('curve', N=12)
    g.params = DGSQPV2Params(dt=0.1, N=12)
    g.params.time_limit = None
    s = DGSQPV2(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    assert s._cparams.variant == 1
    x0, u_tm = scenarios(g, 2, 2)
    plant = PlantModel(dynamics_configs=dyn_configs(), own_class=True, method='rk4', M=2, sim_steps=2)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant)
    check_cross(oracle, s, res, g, x0, u_tm, plant, bases, tag='DG-SQP v2')
    assert (res['steps_done'] >= 1).all()


def test_coexistence_and_every_refusal_through_the_c_abi(games):
    """Case 8: a cross launch, then a set_plant launch, a plant-less launch and a solve_batch on the same handle, each bit-identical to a
    fresh handle's; then every refusal and fetcher error of the raw ABI."""
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel, lift_state
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s, fresh = DGSQP(*g.solver_args(), print_method=None), DGSQP(*g.solver_args(), print_method=None)
    lib, h = s._lib, s._h
    B, T = 3, 3
    x0, u_tm = scenarios(g, B, 73)
    u_am = s._to_agent_major(u_tm)
    msg = lambda: lib.dgsqp_last_error(h).decode()
    cross, plain = PlantModel(dynamics_configs=dyn_configs(), own_class=True, sim_steps=2), PlantModel(sim_steps=2)
    first = s.step_batch(x0, u_tm, T, plant=cross)
    for kw in (dict(plant=plain), dict(), None):
        a, b = (s.step_batch(x0, u_tm, T, **kw), fresh.step_batch(x0, u_tm, T, **kw)) if kw is not None else (s.solve_batch(x0, u_tm), fresh.solve_batch(x0, u_tm))
        for key in DOUBLES[:1] + COUNTS + (('q', 'u_ws', 'steps_done') if kw is not None else ()):
            assert same(a[key], b[key]), (kw, key)
    again = s.step_batch(x0, u_tm, T, plant=cross)
    for key in ('q', 'z', 'u', 'status', 'u_ws', 'u_plant'):
        assert same(first[key], again[key]), key
    # ---- the raw ABI ----
    h2 = fresh._h
    zbuf, tr = np.empty((T + 1, B, 16)), np.empty((T, B, 2, 3))
    assert lib.dgsqp_fetch_plant_state(h2, _ffi.dptr(zbuf), zbuf.size) == -1 and 'no closed-loop launch with a cross plant' in lib.dgsqp_last_error(h2).decode()
    assert lib.dgsqp_fetch_track_ref(h2, _ffi.dptr(tr), tr.size) == -1
    assert lib.dgsqp_set_cross_plant(None, None, 0, None) == -1 and lib.dgsqp_set_cross_plant(h, None, 0, None) == 0
    pt = cross.lower(s._problem)
    z0 = lift_state([0, 0], [1, 1], x0)

    def refused(p, word, Bz=B, z=z0):
        assert lib.dgsqp_set_cross_plant(h, ctypes.byref(p), Bz, _ffi.dptr(z)) == -1
        assert msg().startswith('cross plant: ') and word in msg(), msg()

    def changed(**kw):
        p = _ffi.PlantT.from_buffer_copy(pt)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    refused(changed(integrator=9), 'integrator')
    refused(changed(substeps=0), 'substeps')
    refused(changed(sim_steps=0), 'sim_steps')
    refused(pt, 'z0', Bz=0)
    refused(pt, 'z0', z=None)
    p = changed()
    p.delay[1][0] = 17
    refused(p, 'delay')
    p = changed()
    p.agents[0].model = 2                                                     # a unicycle under a kinematic bicycle's game
    refused(p, 'not a supported pair')
    p.agents[0].model = 3                                                     # 0 -> 3 is not in the table either
    refused(p, 'not a supported pair')
    dt = _ffi.DriversT()
    dt.kind[0] = _ffi.DRIVER_TRACK
    assert lib.dgsqp_set_drivers(h, ctypes.byref(dt), T, B, None, None, None) == -1 and msg().startswith('drivers: ') and 'no plant' in msg()
    ppt = plain.lower(s._problem)
    assert lib.dgsqp_set_plant(h, ctypes.byref(ppt)) == 0
    assert lib.dgsqp_set_drivers(h, ctypes.byref(dt), T, B, None, None, None) == -1 and msg().startswith('drivers: ') and 'cross plant' in msg()
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == -1 and msg().startswith('plant: ')      # dgsqp_set_plant keeps its refusal
    assert lib.dgsqp_set_cross_plant(h, ctypes.byref(pt), B, _ffi.dptr(z0)) == 0
    assert lib.dgsqp_set_drivers(h, ctypes.byref(dt), T, B, None, None, None) == 0
    # the launch: a disturbance, another B, an x0 that is not p(z0)
    rc, _ = raw_launch(s, x0, u_am, T, w=np.zeros((T, B, s.n_q)))
    assert rc == -1 and msg().startswith('cross plant: ') and 'disturbance' in msg()
    rc, _ = raw_launch(s, x0[:2], u_am[:2], T)
    assert rc == -1 and (msg().startswith('cross plant: ') or msg().startswith('drivers: ')) and 'B = 2' in msg()
    assert lib.dgsqp_set_drivers(h, None, 0, 0, None, None, None) == 0
    rc, _ = raw_launch(s, x0[:2], u_am[:2], T)
    assert rc == -1 and msg().startswith('cross plant: ') and 'B = 2' in msg()
    bad = x0.copy()
    bad[1, 7] = np.nextafter(bad[1, 7], np.inf)
    rc, _ = raw_launch(s, bad, u_am, T)
    assert rc == -1 and msg().startswith('cross plant: ') and 'chain 1, agent 1, entry 1' in msg()
    # the ensemble compares with the PLANT's class
    veh = (_ffi.VehicleT * (B * 2))()
    for i in range(B * 2):
        veh[i] = _ffi.VehicleT.from_buffer_copy(bytes(s._problem.agents[i % 2])[:ctypes.sizeof(_ffi.VehicleT)])      # the game's class 0
    assert lib.dgsqp_set_plant_ensemble(h, B, veh, None) == -1 and msg().startswith('plant ensemble: ') and "cross plant's agent is of class 1" in msg()
    rc, out = raw_launch(s, x0, u_am, T)
    assert rc == 0 and (out['steps_done'] == T).all()
    assert lib.dgsqp_fetch_plant_state(h, _ffi.dptr(zbuf), zbuf.size - 1) == -1 and 'too small' in msg()
    assert lib.dgsqp_fetch_plant_state(h, None, zbuf.size) == -1
    assert lib.dgsqp_fetch_plant_state(h, _ffi.dptr(zbuf), zbuf.size) == 0 and lib.dgsqp_fetch_track_ref(h, _ffi.dptr(tr), tr.size) == 0
    assert same(zbuf[0], z0) and same(np.swapaxes(zbuf, 0, 1), first['z']) and np.isnan(tr).all()
    # dgsqp_set_plant clears the cross plant; a TRACK driver that outlives it is refused by the launch
    assert lib.dgsqp_set_drivers(h, ctypes.byref(dt), T, B, None, None, None) == 0
    assert lib.dgsqp_set_plant(h, ctypes.byref(ppt)) == 0
    rc, _ = raw_launch(s, x0, u_am, T)
    assert rc == -1 and msg().startswith('drivers: ') and 'TRACK' in msg()
    assert lib.dgsqp_set_drivers(h, None, 0, 0, None, None, None) == 0 and lib.dgsqp_set_plant(h, None) == 0
    rc, out = raw_launch(s, x0, u_am, T)
    ref = fresh.step_batch(x0, u_tm, T)
    assert rc == 0 and same(np.swapaxes(out['q'], 0, 1), ref['q'])
