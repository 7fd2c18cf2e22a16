"""Held plans of closed-loop batches on the device: DGSQP.step_batch(..., hold=PlanHold(...)) / dgsqp_set_plan_hold, dgsqp_fetch_plan_hold (the
held plan's fields of DgPlantPack, dev_hold_due and dev_hold_next, csrc/dgsqp_closed_loop.h): a chain solves only when a plan is due -- every R-th
step after an accepted solve -- and otherwise feeds the plant the next stage of the warm start it holds; after a failed solve it does so
too when on_fail = 'hold'.

The checks common to every case are those of tests/closed_loop_hold_checks.py: teacher forcing of every step that solved, the chain
(u_game, u_ws[t+1], plan_stage, status == held) bit for bit against ``closed_loop.hold_step`` replaying the recorded statuses, u_plant bit for
bit against the delay-line mirror fed with the command that entered the plant, q[t+1] against the CPU oracle at 1e-12 relative to
max(1, |q|_inf), and the fill values of held and never-run steps."""
import ctypes

import numpy as np
import pytest

from closed_loop_checks import BAR, CHAIN, COUNTS, DELAYS, DOUBLES, configs_of, same, scenarios, solver_of      # noqa: F401  (solver_of is a fixture)
from closed_loop_hold_checks import HELD, check_all

pytestmark = pytest.mark.gpu

PLANT_KW = dict(method='rk4', M=3, sim_steps=2, delay_steps=DELAYS)
H = HELD


def stage0(s, u_am):
    return s._to_time_major(np.asarray(u_am))[..., 0, :]


def failed_qp_chains(games):
    """The three chains of test_chain_goes_on_after_a_failed_qp: car 2 of chain 1 starts one metre outside the track."""
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    xa, ua = scenarios(g, 1, 31)
    xb, ub = scenarios(g, 2, 37)
    x0, u_tm = np.stack([xb[0], xa[0], xb[1]]), np.stack([ub[0], ua[0], ub[1]])
    x0[1, 11] = g.half_width + 1.0
    return s, x0, u_tm


@pytest.mark.parametrize('which', ['six chains', 'failed qp'])
def test_default_hold_is_the_launch_without_it(oracle, games, solver_of, which):
    """Case 1: R = 1 / 'reference' / the default mask: every shared record is bit-identical to the same launch without ``hold`` and
    plan_stage is 0 -- also where every solve of a chain is 'qp_fail' (the reference row of the table)."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    if which == 'six chains':
        s, T = solver_of('kb_curve_N10'), 4
        x0, u_tm = scenarios(games['kb_curve_N10'][0], 6, 41)
    else:
        (s, x0, u_tm), T = failed_qp_chains(games), 3
    plant = PlantModel(**PLANT_KW)
    plain = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, hold=PlanHold())
    m = check_all(oracle, s, res, x0, u_tm, PlanHold(), plant, f'default hold, {which}')
    for key in CHAIN + ('u_pred', 'converged'):
        assert same(res[key], plain[key]), key
    assert res['msg'] == plain['msg'] and 'u_game' not in plain and 'plan_stage' not in plain
    assert same(res['u_game'], plain['u_applied']) and (res['plan_stage'] == 0).all() and m['held'] == 0
    assert (res['steps_done'] == T).all()
    if which == 'failed qp':
        assert (res['status'][1] == 4).all() and (res['status'][[0, 2]] != 4).all()
        assert all(same(res['u_ws'][1, t], res['u_ws'][1, 0]) for t in range(T + 1))
    # without a plant argument the identity plant is used
    ident = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=PlantModel())
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, hold=PlanHold())
    for key in CHAIN:
        assert same(res[key], ident[key]), key


@pytest.mark.parametrize('R', [2, 3])
def test_replan_rate(oracle, games, solver_of, R):
    """Case 2: a plan every R-th control step.  By the CPU oracle (game model as plant) all six chains solve [0, held, 0, held, 0, held] at
    R = 2 and [0, held, held, 0, held, held] at R = 3."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 6, 41)
    plant, hold = PlantModel(), PlanHold(replan_every=R)
    res = s.step_batch(x0, u_tm, 6, keep_predictions=True, plant=plant, hold=hold)
    print(f'R = {R}: statuses {res["status"].tolist()}')
    accepted = ~np.isin(res['status'][:, 0], (3, 4)) & (res['status'][:, 0] >= 0)
    assert accepted.all(), res['status'][:, 0]
    assert ((res['status'] == H).sum(axis=1) >= 1).all() and ((res['status'] >= 0).sum(axis=1) >= 2).all(), res['status']
    check_all(oracle, s, res, x0, u_tm, hold, plant, f'replan every {R}')
    assert (res['steps_done'] == 6).all()


def noisy_estimates(s, g, B, T):
    v = np.zeros((B, T, s.n_q))
    v[1, 2, 11] = 2.0 * g.half_width + 1.0                        # car 2's estimated e_y is off the track at step 2 of chain 1 only
    return v


@pytest.mark.parametrize('R,on_fail,want', [(1, 'reference', [0, 0, 4, 0, 0, 0]), (1, 'hold', [0, 0, 4, 0, 0, 0]),
                                            (2, 'reference', [0, H, 4, 0, H, 0]), (2, 'hold', [0, H, 4, 0, H, 0])])
def test_transient_failure_and_recovery(oracle, games, solver_of, R, on_fail, want):
    """Case 3: the estimate of step 2 puts car 2 off the track: that solve is 'qp_fail', falls on a due step, and is retried and accepted at
    step 3 (the patterns are the CPU oracle's).  Under 'hold' the chain applies the next stage of the plan it holds, under 'reference' stage 0
    of the failed iterate with the warm start kept."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel, shift_warm_start
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 3, 6
    x0, u_tm = scenarios(g, B, 41)
    plant, hold = PlantModel(), PlanHold(replan_every=R, on_fail=on_fail)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, hold=hold, estimate_noise=noisy_estimates(s, g, B, T))
    print(f'R = {R}, {on_fail}: statuses {res["status"].tolist()}')
    assert res['status'][1].tolist() == want, res['status'][1]
    check_all(oracle, s, res, x0, u_tm, hold, plant, f'transient failure, R = {R}, {on_fail}')
    assert (res['steps_done'] == T).all() and np.isfinite(res['q']).all()
    if on_fail == 'hold':
        assert same(res['u_game'][1, 2], stage0(s, res['u_ws'][1, 2]))
        assert same(res['u_ws'][1, 3], shift_warm_start(res['u_ws'][1, 2], s.N, s.num_ua_d))
        assert res['plan_stage'][1, 2] == (1 if R == 1 else 2)
    else:
        assert same(res['u_game'][1, 2], stage0(s, res['u'][1, 2]))
        assert same(res['u_ws'][1, 3], res['u_ws'][1, 2]) and res['plan_stage'][1, 2] == 0


def test_noise_on_a_held_step_is_never_read(oracle, games, solver_of):
    """Case 3, R = 3: step 2 is held, its noise is not read: chain 1 equals the noise-free run bit for bit, q_est is NaN on held steps."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 3, 6
    x0, u_tm = scenarios(g, B, 41)
    plant, hold = PlantModel(), PlanHold(replan_every=3, on_fail='hold')
    v = noisy_estimates(s, g, B, T)
    v[1, 1, :] = np.nan                                           # ... nor does a non-finite entry there end the chain
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, hold=hold, estimate_noise=v)
    clean = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, hold=hold, estimate_noise=np.zeros_like(v))
    assert res['status'][1].tolist() == [0, H, H, 0, H, H], res['status'][1]
    check_all(oracle, s, res, x0, u_tm, hold, plant, 'noise on a held step')
    assert (res['steps_done'] == T).all() and np.isfinite(res['q']).all()
    held = res['status'] == H
    assert np.isnan(res['q_est'][held]).all() and same(res['q_est'][~held], res['q'][:, :T][~held] + 0.0)
    for key in CHAIN + ('u_game', 'plan_stage', 'q_est'):
        assert same(res[key], clean[key]), key


def test_fail_mask_that_accepts_nothing(oracle, games, solver_of):
    """Case 4: every status fails and on_fail = 'hold': the initial warm start is consumed row by row while every step still solves."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    s = solver_of('kb_curve_N10')
    B, T = 3, 4
    x0, u_tm = scenarios(games['kb_curve_N10'][0], B, 41)
    plant, hold = PlantModel(), PlanHold(on_fail='hold', accept=0b111111)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, hold=hold)
    m = check_all(oracle, s, res, x0, u_tm, hold, plant, 'nothing accepted')
    assert m['solved'] == B * T and m['held'] == 0 and (res['status'] >= 0).all()
    for t in range(T):
        assert same(res['u_game'][:, t], np.ascontiguousarray(np.asarray(u_tm, float)[:, t])), t
        assert (res['plan_stage'][:, t] == t).all(), t


def test_no_plan_state_survives_beyond_the_grid(oracle, games, solver_of):
    """Case 5: two scenarios tiled to 600 chains on the launch's ordinary grid (smaller than B: a workgroup starts a second chain after its
    first), R = 2: every chain equals its twin bit for bit."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    s = solver_of('kb_curve_N10')
    x2, u2 = scenarios(games['kb_curve_N10'][0], 2, 41)
    x0, u_tm = np.tile(x2, (300, 1)), np.tile(u2, (300, 1, 1))
    plant, hold = PlantModel(method='rk4', M=2, sim_steps=2, delay_steps=DELAYS), PlanHold(replan_every=2)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, hold=hold)
    few = {k: v[:4] for k, v in res.items() if k in CHAIN + DOUBLES + COUNTS + ('u_game', 'plan_stage', 'u_pred', 'msg', 'converged')}
    m = check_all(oracle, s, few, x0[:4], u_tm[:4], hold, plant, 'beyond the grid, first 4 of 600')
    assert m['held'] == 4 and m['solved'] == 8 and (res['steps_done'] == 3).all()
    for key in CHAIN + ('u_game', 'plan_stage'):
        twin = np.tile(res[key][:2], (300,) + (1,) * (res[key].ndim - 1))
        assert same(res[key], twin), key


def test_with_the_other_settings_at_once(oracle, games, solver_of):
    """Case 6: car 2 on the PID driver, a vehicle and delays per chain, the monitor, the carried u_prev, R = 2."""
    from test_closed_loop_drivers import check_commands
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlanHold, PlantModel, perturbed_configs
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 4, 5
    x0, u_tm = scenarios(g, B, 61)
    delays = np.array([[[2, 1], [0, 3]], [[0, 0], [1, 1]], [[1, 2], [2, 0]], [[3, 0], [0, 1]]])
    plant = PlantModel(per_chain_configs=perturbed_configs(configs_of(g), dict(mass=0.1), B, seed=1), per_chain_delay_steps=delays, method='rk4', M=2,
                       sim_steps=2)
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(ki_s=0.05, du_max=(10.0, 0.05)))
    hold = PlanHold(replan_every=2)
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=drivers, hold=hold, monitor=True, u_prev=True)
    assert {'u_game', 'plan_stage', 'u_cmd', 'u_plant', 'u_prev', 'clearance', 'box_excess', 'hit_step'} <= set(res)
    m = check_all(oracle, s, res, x0, u_tm, hold, plant, 'hold with drivers, vehicles, delays, monitor, u_prev')
    assert m['held'] >= B and (res['steps_done'] == T).all()
    check_commands(s, res, drivers, 'hold with drivers')                 # a GAME agent receives u_game (u_applied), the PID agent follows its mirror
    assert same(res['u_cmd'][:, :, :2], res['u_game'][:, :, :2]) and not same(res['u_cmd'][:, :, 2:], res['u_game'][:, :, 2:])
    assert same(res['u_prev'][:, 0], np.zeros((B, s.n_u))) and same(res['u_prev'][:, 1:], res['u_cmd'][:, :T - 1])


def other_kernel(name, games, solver_of):
    import multistage_kat as mk
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    if name in ('dyn_curve_N15', 'merge_N8'):
        return solver_of(name), scenarios(games[name][0], 2, 53)
    if name == 'kb_chicane_N15 b256':
        return solver_of('kb_chicane_N15', workgroups_per_cu=2), scenarios(games['kb_chicane_N15'][0], 2, 61)
    if name == 'v2':
        from dgsqp_amd.solver_types import DGSQPV2Params
        from dgsqp_amd.solver_v2 import DGSQP as DGSQPV2
        g = mc.kinematic_racing_game('curve', N=12)
        g.params = DGSQPV2Params(dt=0.1, N=12)
        g.params.time_limit = None
        s = DGSQPV2(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
        assert s._cparams.variant == 1
        return s, scenarios(g, 2, 2)
    g = mk.build_game(name)
    s = DGSQP(*g.solver_args(), print_method=None)
    assert s.dims.layout == {'kin3_N20_dir': 1, 'kin3_N25_dir': 2}[name]
    return s, scenarios(g, 2, 59)


@pytest.mark.parametrize('name', ['dyn_curve_N15', 'merge_N8', 'v2', 'kb_chicane_N15 b256', 'kin3_N20_dir', 'kin3_N25_dir'])
def test_other_kernels_of_the_family(oracle, games, solver_of, name):
    """Case 7: the dynamic bicycle, the unicycle, DG-SQP v2, the 256-thread build, a big-layout and an XL-layout game: R = 2, common checks."""
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    s, (x0, u_tm) = other_kernel(name, games, solver_of)
    plant, hold = PlantModel(), PlanHold(replan_every=2)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant, hold=hold)
    print(f'{name}: statuses {res["status"].tolist()}')
    m = check_all(oracle, s, res, x0, u_tm, hold, plant, f'hold, {name}')
    assert m['solved'] >= 2 and (res['steps_done'] >= 1).all()


def test_argument_errors_and_coexistence_through_the_c_abi(games, solver_of):
    """Case 8: every refusal is DGSQP_E_ARG with its message; a plain-plant launch and a solve_batch give what they gave before a hold
    launch on the same handle."""
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlanHold, PlantModel
    from dgsqp_amd.solver import DGSQP, _record_ptrs
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None)                  # a handle of its own: nothing has run on it
    lib, h = s._lib, s._h
    B, T = 3, 4
    x0, u_tm = scenarios(g, B, 73)
    u_am = s._to_agent_major(u_tm)
    msg = lambda: lib.dgsqp_last_error(h).decode()
    ug, ps = np.empty((T, B, s.n_u)), np.empty((T, B), np.int32)
    fetch = lambda cap=ug.size, a=ug, b=ps: lib.dgsqp_fetch_plan_hold(h, _ffi.dptr(a), _ffi.iptr(b), cap)

    def hold_t(R=2, on_fail=0, mask=0b011000):
        ht = _ffi.HoldT()
        ht.replan_every, ht.on_fail, ht.fail_mask = R, on_fail, mask
        return ht

    def refused(ht, word):
        assert lib.dgsqp_set_plan_hold(h, ctypes.byref(ht)) == -1
        assert msg().startswith('plan hold: ') and word in msg(), msg()

    def launch():
        sm = dict(q=np.empty((T + 1, B, s.n_q)), u_ws=np.empty((T + 1, B, s.n)), **s._records((T, B), predictions=False))
        done = np.empty(B, np.int32)
        rc = lib.dgsqp_closed_loop_batch(h, B, T, _ffi.dptr(x0), _ffi.dptr(u_am), None, _ffi.dptr(sm['q']), _ffi.dptr(sm['u_ws']),
                                         *_record_ptrs(sm), _ffi.iptr(done), None)
        return rc, dict(sm, steps_done=done)

    assert fetch() == -1 and 'no closed-loop launch' in msg()                      # fetch before a launch
    refused(hold_t(), 'no plant')                                                   # no plant set: switching on is refused, switching off is fine
    assert lib.dgsqp_set_plan_hold(h, None) == 0 and lib.dgsqp_set_plan_hold(None, None) == -1
    pt = PlantModel(sim_steps=2).lower(s._problem)
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0
    sol_a = s.solve_batch(x0, u_tm)
    rc, plain_a = launch()
    assert rc == 0
    refused(hold_t(R=0), 'replan_every')
    refused(hold_t(R=s.N + 1), f'1 .. N = {s.N}')
    refused(hold_t(on_fail=2), 'on_fail')
    refused(hold_t(on_fail=-1), 'on_fail')
    refused(hold_t(mask=1 << 6), 'bit above 5')
    rc, again = launch()                                                             # the refusals left nothing behind
    assert rc == 0 and all(same(again[k], plain_a[k]) for k in plain_a if plain_a[k] is not None)
    assert fetch() == -1 and 'no closed-loop launch' in msg()
    assert lib.dgsqp_set_plan_hold(h, ctypes.byref(hold_t(R=s.N))) == 0              # R = N is allowed
    assert lib.dgsqp_set_plan_hold(h, ctypes.byref(hold_t(R=2, on_fail=1))) == 0
    rc, held = launch()
    assert rc == 0
    assert fetch(ug.size - 1) == -1 and 'too small' in msg()
    assert lib.dgsqp_fetch_plan_hold(h, None, _ffi.iptr(ps), ug.size) == -1 and lib.dgsqp_fetch_plan_hold(h, _ffi.dptr(ug), None, ug.size) == -1
    assert fetch() == 0
    assert (held['status'][0] >= 0).all() and (held['status'][1] == HELD).all()      # (step-major: every chain solves at step 0 and holds at step 1) and (ps[1] == 1).all() and (ps[0] == 0).all() and np.isfinite(ug).all()
    assert same(ug[0], stage0(s, held['u'][0])) and same(ug[1], stage0(s, held['u_ws'][1]))
    # a hold that outlives its plant is refused by the launch
    assert lib.dgsqp_set_plant(h, None) == 0
    rc, _ = launch()
    assert rc == -1 and msg().startswith('plan hold: ') and 'no plant' in msg()
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0
    assert lib.dgsqp_set_plan_hold(h, None) == 0
    rc, plain_b = launch()
    sol_b = s.solve_batch(x0, u_tm)
    assert rc == 0
    for key in plain_a:
        assert plain_a[key] is None or same(plain_a[key], plain_b[key]), key
    for key in DOUBLES + COUNTS:
        assert same(sol_a[key], sol_b[key]), key
    assert not same(held['q'], plain_a['q'])
    assert fetch() == 0                                                              # the records of the last hold launch are still there
    assert lib.dgsqp_set_plant(h, None) == 0
