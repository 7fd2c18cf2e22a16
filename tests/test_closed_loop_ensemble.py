"""Per-chain plants, state estimates and the safety monitor of closed-loop batches on the device: DGSQP.step_batch(..., plant=PlantModel(
per_chain_configs=...), estimate_noise=..., monitor=...) / dgsqp_set_plant_ensemble, dgsqp_set_estimate_noise, dgsqp_set_monitor
(their fields of DgPlantPack, the pack of every launch with a plant: csrc/dgsqp_closed_loop.h).

The idiom is that of tests/test_closed_loop_plant.py, with the helpers of tests/closed_loop_checks.py: TEACHER FORCING (every step that ran
is, bit for bit, the ``solve_batch`` solve from the recorded (state the solve started from, u_ws[t]) -- the state is q_est[t] with
estimates), the warm-start chain with the records of steps that never ran, and the plant against the CPU oracle one control step at a time from the device's own
q[t] and u_plant[t], with CHAIN b's vehicle record and delays: 1e-12 relative to max(1, |q|_inf), the project's bar for x.

The monitor is checked against ``closed_loop.monitor`` fed with the oracle's z_j.  With eps = 1e-12 max(1, |z|_inf) each position coordinate
is within eps and a pair distance is 1-Lipschitz in each of its four coordinates, so clearance is held to 4 eps; a box excess is one
difference of a state entry and a constant and is held to 2 eps.  A case is only valid when every monitored pairwise clearance is at least
1e-6 in magnitude by the oracle (else a hit could be decided by rounding): the test asserts that."""
import numpy as np
import pytest

from closed_loop_checks import (CHAIN, COUNTS, DELAYS, DOUBLES, check_chain, check_monitor, check_plant, configs_of, game_bounds, same, scenarios,
                                 solver_of, teacher_force)      # noqa: F401  (solver_of is a fixture)

pytestmark = pytest.mark.gpu


def run_and_check(oracle, s, x0, u_tm, T, plant, w=None, tag='', chains=None, **kw):
    res = s.step_batch(x0, u_tm, T, disturbance=w, keep_predictions=True, plant=plant, **kw)
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), min_done=0 if 'estimate_noise' in kw else 1)
    teacher_force(s, res)
    Z = check_plant(oracle, s, res, plant, w, tag, chains)
    if 'clearance' in res:
        check_monitor(s, res, Z, tag)
    return res


def test_uniform_ensemble_is_the_plain_plant(oracle, games, solver_of):
    """Case 1: every chain gets the configs of the plain plant (and its delays): every output is bit-identical to the plain-plant launch."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    kw = dict(method='rk4', M=3, sim_steps=2, delay_steps=DELAYS)
    plain = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel(dynamics_configs=configs_of(g, mass=1.2), **kw))
    cfgs = [configs_of(g, mass=1.2) for _ in range(5)]
    for tag, plant in (('configs', PlantModel(per_chain_configs=cfgs, **kw)),
                       ('configs and delays', PlantModel(per_chain_configs=cfgs, per_chain_delay_steps=[DELAYS] * 5, method='rk4', M=3, sim_steps=2)),
                       ('delays alone', PlantModel(dynamics_configs=configs_of(g, mass=1.2), per_chain_delay_steps=[DELAYS] * 5, method='rk4', M=3, sim_steps=2))):
        res = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant)
        for key in CHAIN:
            assert same(res[key], plain[key]), (tag, key)
    assert (plain['steps_done'] == 3).all() and plain['u_plant'][:, 1:].any()


def chain_delays(B, M, seed):
    return np.random.default_rng(seed).integers(0, 4, size=(B, M, 2))


@pytest.mark.parametrize('name,B,T,spread,kw', [
    ('kb_curve_N10', 5, 3, dict(mass=0.2, drag_coefficient=0.2), dict(method='rk4', M=3, sim_steps=2)),
    ('dyn_curve_N15', 3, 2, dict(pacejka_d_front=0.2, pacejka_d_rear=0.2), dict(M=5, sim_steps=2)),
    ('merge_N8', 3, 2, dict(mass=0.2), dict(method='euler')),
])
def test_distinct_vehicles_and_delays_per_chain(oracle, games, solver_of, name, B, T, spread, kw):
    """Case 2: vehicles from perturbed_configs and a delay of its own for every chain, agent and channel."""
    from dgsqp_amd.closed_loop import PlantModel, perturbed_configs
    g = games[name][0]
    s = solver_of(name)
    x0, u_tm = scenarios(g, B, 43)
    x0[1:], u_tm[1:] = x0[0], u_tm[0]                                  # one scenario B times: only the plants tell the chains apart
    delays = chain_delays(B, s.M, 7)
    plant = PlantModel(per_chain_configs=perturbed_configs(configs_of(g), spread, B, seed=3), per_chain_delay_steps=delays, **kw)
    res = run_and_check(oracle, s, x0, u_tm, T, plant, tag=f'ensemble {name}')
    assert (res['steps_done'] == T).all()
    for b in range(B):
        for c in range(b + 1, B):
            assert np.abs(res['q'][b, 1:] - res['q'][c, 1:]).max() > 1e-6, (b, c)
    if name == 'merge_N8':
        assert s.M == 3


def test_records_are_indexed_by_chain_beyond_the_grid(oracle, games, solver_of):
    """Case 3: B = 600 > the grid, distinct vehicles and delays: a workgroup starts a second chain after its first.  The last four chains,
    run again as a batch of four with their own records, must be bit-identical: indexing by workgroup, or a copy left over from the
    workgroup's previous chain, would show."""
    from dgsqp_amd.closed_loop import PlantModel, perturbed_configs
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 600, 47)
    ens = perturbed_configs(configs_of(g), dict(mass=0.2, drag_coefficient=0.2), 600, seed=5)
    delays = chain_delays(600, 2, 9)
    kw = dict(method='rk4', M=2, sim_steps=2)
    res = s.step_batch(x0, u_tm, 2, keep_predictions=True, plant=PlantModel(per_chain_configs=ens, per_chain_delay_steps=delays, **kw))
    check_chain(s, res, x0, s._to_agent_major(u_tm))
    assert teacher_force(s, res) == 1200
    few_plant = PlantModel(per_chain_configs=ens[-4:], per_chain_delay_steps=delays[-4:], **kw)
    few = s.step_batch(x0[-4:], u_tm[-4:], 2, keep_predictions=True, plant=few_plant)
    check_plant(oracle, s, few, few_plant, tag='ensemble kb_curve_N10, last 4 of 600')
    for key in CHAIN:
        assert same(res[key][-4:], few[key]), key


def test_estimates(oracle, games, solver_of):
    """Case 4: the solves start from q_est = q + v, the plant advances the true q."""
    from dgsqp_amd.closed_loop import PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 4, 4
    x0, u_tm = scenarios(g, B, 43)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    v = 1e-2 * np.random.default_rng(3).standard_normal((B, T, s.n_q))
    base = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    res = run_and_check(oracle, s, x0, u_tm, T, plant, tag='estimates', estimate_noise=v)
    assert (res['steps_done'] == T).all() and res['q_est'].shape == (B, T, s.n_q)
    assert same(res['q_est'], res['q'][:, :T] + v)
    assert same(res['u'][:, 0], s.solve_batch(x0 + v[:, 0], u_tm)['u'])              # step 0 starts from the estimate of x0
    assert not same(res['u'], base['u']) and not same(res['q'][:, 1], base['q'][:, 1])
    # v = 0: the launch without estimates, bit for bit
    zero = run_and_check(oracle, s, x0, u_tm, T, plant, tag='estimates, v = 0', estimate_noise=np.zeros_like(v))
    for key in CHAIN:
        assert same(zero[key], base[key]), key
    assert same(zero['q_est'], zero['q'][:, :T]) and 'q_est' not in base
    # a non-finite estimate ends the chain BEFORE that solve
    v2 = v.copy()
    v2[1, 2] = np.nan
    res2 = run_and_check(oracle, s, x0, u_tm, T, plant, tag='estimates, chain end', estimate_noise=v2)
    assert res2['steps_done'].tolist() == [4, 2, 4, 4]
    assert np.isnan(res2['q_est'][1, 2]).all() and np.isnan(res2['q_est'][1, 3]).all() and same(res2['q_est'][1, :2], res['q_est'][1, :2])
    assert same(res2['q'][1, :3], res['q'][1, :3]) and np.isnan(res2['q'][1, 3:]).all()      # the true state the chain reached is kept
    assert (res2['status'][1, 2:] == -1).all() and res2['msg'][1][2:] == ['not_run', 'not_run']
    for key in CHAIN + ('q_est',):
        assert same(res2[key][[0, 2, 3]], res[key][[0, 2, 3]]), key
        if key != 'steps_done':
            assert same(res2[key][1, :2], res[key][1, :2]), key
    v2[:] = v
    v2[3, 0, 1] = np.inf
    res3 = run_and_check(oracle, s, x0, u_tm, T, plant, tag='estimates, chain end at step 0', estimate_noise=v2)
    assert res3['steps_done'].tolist() == [4, 4, 4, 0] and np.isinf(res3['q_est'][3, 0, 1]) and np.isnan(res3['q'][3, 1:]).all()


def hit_disturbance(s, clean, b, t):
    """w [B, T, n_q], zero but for (b, t): it moves car 1's position in q[t+1] onto the point 0.5 (r_0 + r_1) to the right of car 0's."""
    radii, _, _, qoff = game_bounds(s)
    w = np.zeros(clean['q'][:, 1:].shape)
    q = clean['q'][b, t + 1]
    target = q[qoff[0]:qoff[0] + 2] + np.array([0.5 * (radii[0] + radii[1]), 0.0])
    w[b, t, qoff[1]:qoff[1] + 2] = target - q[qoff[1]:qoff[1] + 2]
    return w


@pytest.mark.parametrize('name,wg', [('kb_curve_N10', 1), ('kb_chicane_N15', 2)])
def test_monitor(oracle, games, solver_of, name, wg):
    """Case 5: clearance, box_excess and hit_step over all simulation steps, and a provoked hit; kb_chicane_N15 on the build with
    256-thread workgroups, two per CU."""
    from dgsqp_amd.closed_loop import PlantModel, perturbed_configs
    g = games[name][0]
    s = solver_of(name, **(dict(workgroups_per_cu=2) if wg == 2 else {}))
    B, T, S = 4, 3, 2
    x0, u_tm = scenarios(g, B, 61)
    plant = PlantModel(per_chain_configs=perturbed_configs(configs_of(g), dict(mass=0.1), B, seed=1), method='rk4', M=2, sim_steps=S, delay_steps=DELAYS)
    w0 = np.zeros((B, T, s.n_q))
    clean = run_and_check(oracle, s, x0, u_tm, T, plant, w0, f'monitor {name}, clean', monitor=True)
    assert (clean['steps_done'] == T).all() and (clean['hit_step'] == -1).all() and (clean['clearance'] > 0).all()
    assert np.isfinite(clean['box_excess']).all()                       # (the game bounds some state)
    plain = s.step_batch(x0, u_tm, T, disturbance=w0, keep_predictions=True, plant=plant)
    for key in CHAIN:
        assert same(clean[key], plain[key]), key                        # recording changes nothing
    b, t = 2, 1
    w = hit_disturbance(s, clean, b, t)
    hit = run_and_check(oracle, s, x0, u_tm, T, plant, w, f'monitor {name}, hit', monitor=True)
    want = np.full(B, -1)
    want[b] = t * S + S - 1
    assert hit['hit_step'].tolist() == want.tolist() and hit['clearance'][b, t] < 0 and (np.delete(hit['steps_done'], b) == T).all()
    for key in DOUBLES + COUNTS + ('u_plant',):                         # the chain is reproducible up to the step of the hit
        assert same(hit[key][b, :t + 1], clean[key][b, :t + 1]), key
    assert same(hit['clearance'][b, :t], clean['clearance'][b, :t]) and same(hit['box_excess'][b, :t], clean['box_excess'][b, :t])
    # 'stop': the chain ends after the control step of its first hit, the others do not notice
    stop = s.step_batch(x0, u_tm, T, disturbance=w, keep_predictions=True, plant=plant, monitor='stop')
    stopped = np.full(B, -1)
    stopped[b] = t
    check_chain(s, stop, x0, s._to_agent_major(u_tm), stopped=stopped)
    teacher_force(s, stop)
    check_monitor(s, stop, check_plant(oracle, s, stop, plant, w, f'monitor {name}, stop'), f'monitor {name}, stop')
    assert stop['steps_done'].tolist() == [T if c != b else t + 1 for c in range(B)]
    assert np.isnan(stop['u_ws'][b, t + 1]).all() and same(stop['q'][b, :t + 2], hit['q'][b, :t + 2]) and np.isfinite(stop['q'][b, t + 1]).all()
    assert np.isnan(stop['clearance'][b, t + 1:]).all() and same(stop['clearance'][b, :t + 1], hit['clearance'][b, :t + 1])
    others = [c for c in range(B) if c != b]
    for key in CHAIN + ('clearance', 'box_excess', 'hit_step'):
        assert same(stop[key][others], hit[key][others]), key


def test_coexistence(oracle, games, solver_of):
    """Case 6a: after a launch with all three settings on, a plain-plant launch, a plant-less launch and solve_batch give what they gave."""
    from dgsqp_amd.closed_loop import PlantModel, perturbed_configs
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 5, 3
    x0, u_tm = scenarios(g, B, 67)
    kw = dict(method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), **kw)
    sol_a = s.solve_batch(x0, u_tm)
    less_a = s.step_batch(x0, u_tm, T, keep_predictions=True)
    plain_a = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    v = 1e-2 * np.random.default_rng(1).standard_normal((B, T, s.n_q))
    full_plant = PlantModel(per_chain_configs=perturbed_configs(configs_of(g), dict(mass=0.2), B, seed=2), **kw)
    full = run_and_check(oracle, s, x0, u_tm, T, full_plant, tag='coexistence, all three', estimate_noise=v, monitor=True)
    assert {'q_est', 'clearance', 'box_excess', 'hit_step', 'u_plant'} <= set(full)
    plain_b = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    less_b = s.step_batch(x0, u_tm, T, keep_predictions=True)
    sol_b = s.solve_batch(x0, u_tm)
    for key in CHAIN:
        assert same(plain_a[key], plain_b[key]), key
        if key != 'u_plant':
            assert same(less_a[key], less_b[key]), key
    for key in DOUBLES + COUNTS:
        assert same(sol_a[key], sol_b[key]), key
    for res in (plain_b, less_b):
        assert not {'q_est', 'clearance', 'box_excess', 'hit_step'} & set(res)
    assert not same(full['q'], plain_a['q'])
    # none of it without a plant
    for kw2 in (dict(estimate_noise=v), dict(monitor=True), dict(monitor='stop')):
        with pytest.raises(ValueError, match='plant'):
            s.step_batch(x0, u_tm, T, **kw2)
    with pytest.raises(ValueError, match='estimate_noise'):
        s.step_batch(x0, u_tm, T, plant=plant, estimate_noise=v[:, :2])
    with pytest.raises(ValueError, match='monitor'):
        s.step_batch(x0, u_tm, T, plant=plant, monitor='halt')
    with pytest.raises(ValueError, match=r'\[B\]\[M\]'):
        s.step_batch(x0[:3], u_tm[:3], T, plant=full_plant)
    again = s.step_batch(x0, u_tm, T, keep_predictions=True)
    for key in ('q', 'u', 'u_ws') + COUNTS:
        assert same(again[key], less_a[key]), key


def test_argument_errors_through_the_c_abi(games, solver_of):
    """Case 6b: every refusal is DGSQP_E_ARG with a message and leaves the next launch clean; the fetchers refuse a buffer that is too
    small or NULL, and a fetch before any such launch."""
    import ctypes
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None)                      # a handle of its own: nothing has run on it
    lib, h = s._lib, s._h
    B, T = 2, 2
    x0, u_tm = scenarios(g, B, 73)
    msg = lambda: lib.dgsqp_last_error(h).decode()
    good = PlantModel(per_chain_configs=[configs_of(g) for _ in range(B)], per_chain_delay_steps=[DELAYS] * B, sim_steps=2)
    veh, delay = good.lower_ensemble(s._problem, B)
    v = np.zeros((T, B, s.n_q))
    buf, ibuf = np.empty(T * B * s.n_q), np.empty(B, np.int32)
    # nothing has run: the fetchers say so
    assert lib.dgsqp_fetch_q_est(h, _ffi.dptr(buf), buf.size) == -1 and 'no closed-loop launch' in msg()
    assert lib.dgsqp_fetch_monitor(h, _ffi.dptr(buf), _ffi.dptr(buf), _ffi.iptr(ibuf)) == -1 and 'no closed-loop launch' in msg()
    # no plant set: every switch-on is refused, every switch-off is fine
    assert lib.dgsqp_set_plant_ensemble(h, B, veh, _ffi.iptr(delay)) == -1 and msg().startswith('plant ensemble: ') and 'no plant' in msg()
    assert lib.dgsqp_set_estimate_noise(h, T, B, _ffi.dptr(v)) == -1 and 'no plant' in msg()
    assert lib.dgsqp_set_monitor(h, 1) == -1 and 'no plant' in msg()
    assert lib.dgsqp_set_plant_ensemble(h, 0, None, None) == 0 and lib.dgsqp_set_estimate_noise(h, 0, 0, None) == 0 and lib.dgsqp_set_monitor(h, 0) == 0
    assert lib.dgsqp_set_plant_ensemble(None, 0, None, None) == -1 and lib.dgsqp_set_monitor(None, 0) == -1
    base = s.step_batch(x0, u_tm, T)
    pt = PlantModel(sim_steps=2).lower(s._problem)
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0

    def launch():
        sm = dict(q=np.empty((T + 1, B, s.n_q)), u_ws=np.empty((T + 1, B, s.n)), **s._records((T, B), predictions=False))
        done = np.empty(B, np.int32)
        from dgsqp_amd.solver import _record_ptrs
        rc = lib.dgsqp_closed_loop_batch(h, B, T, _ffi.dptr(x0), _ffi.dptr(s._to_agent_major(u_tm)), None, _ffi.dptr(sm['q']), _ffi.dptr(sm['u_ws']),
                                         *_record_ptrs(sm), _ffi.iptr(done), None)
        return rc, sm

    rc, plain = launch()
    assert rc == 0

    def refused(call, start, word):
        assert call() == -1
        assert msg().startswith(start) and word in msg(), msg()
        rc, sm = launch()                                               # the refusal left nothing behind
        assert rc == 0 and all(same(sm[k], plain[k]) for k in ('q', 'u', 'u_ws', 'status'))

    def with_vehicle(change):
        veh2, _ = good.lower_ensemble(s._problem, B)
        change(veh2)
        return lambda: lib.dgsqp_set_plant_ensemble(h, B, veh2, _ffi.iptr(delay))

    def with_delay(value):
        d2 = delay.copy()
        d2[1, 0, 1] = value
        return lambda: lib.dgsqp_set_plant_ensemble(h, B, veh, _ffi.iptr(d2))

    refused(with_vehicle(lambda vv: setattr(vv[3], 'model', 1)), 'plant ensemble: ', 'model class')
    refused(with_delay(_ffi.MAX_DELAY + 1), 'plant ensemble: ', 'delay')
    refused(with_delay(-1), 'plant ensemble: ', 'delay')
    refused(lambda: lib.dgsqp_set_plant_ensemble(h, -1, veh, None), 'plant ensemble: ', 'negative')
    refused(lambda: lib.dgsqp_set_monitor(h, 3), 'monitor: ', 'mode')
    refused(lambda: lib.dgsqp_set_monitor(h, -1), 'monitor: ', 'mode')
    # a launch whose shape differs from what the settings were made for
    veh3, delay3 = PlantModel(per_chain_configs=[configs_of(g) for _ in range(3)], sim_steps=2).lower_ensemble(s._problem, 3)
    assert lib.dgsqp_set_plant_ensemble(h, 3, veh3, None) == 0
    rc, _ = launch()
    assert rc == -1 and msg().startswith('plant ensemble: ') and 'B = 2' in msg()
    assert lib.dgsqp_set_plant_ensemble(h, 0, None, None) == 0
    for shape in ((T + 1, B), (T, B + 1)):
        assert lib.dgsqp_set_estimate_noise(h, shape[0], shape[1], _ffi.dptr(np.zeros(shape + (s.n_q,)))) == 0
        rc, _ = launch()
        assert rc == -1 and msg().startswith('estimate noise: '), msg()
    assert lib.dgsqp_set_estimate_noise(h, 0, 0, None) == 0
    rc, sm = launch()
    assert rc == 0 and all(same(sm[k], plain[k]) for k in ('q', 'u', 'u_ws', 'status'))
    # settings that outlive their plant are refused by the launch
    assert lib.dgsqp_set_monitor(h, 1) == 0 and lib.dgsqp_set_plant(h, None) == 0
    rc, _ = launch()
    assert rc == -1 and msg().startswith('monitor: ') and 'no plant' in msg()
    assert lib.dgsqp_set_monitor(h, 0) == 0
    # the fetchers after a launch with everything on
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0 and lib.dgsqp_set_plant_ensemble(h, B, veh, _ffi.iptr(delay)) == 0
    assert lib.dgsqp_set_estimate_noise(h, T, B, _ffi.dptr(v)) == 0 and lib.dgsqp_set_monitor(h, 1) == 0
    rc, sm = launch()
    assert rc == 0
    assert lib.dgsqp_fetch_q_est(h, _ffi.dptr(buf), buf.size - 1) == -1 and 'too small' in msg()
    assert lib.dgsqp_fetch_q_est(h, None, buf.size) == -1
    assert lib.dgsqp_fetch_q_est(h, _ffi.dptr(buf), buf.size) == 0 and same(buf.reshape(T, B, s.n_q), sm['q'][:T])
    cl, bx = np.empty(T * B), np.empty(T * B)
    assert lib.dgsqp_fetch_monitor(h, None, _ffi.dptr(bx), _ffi.iptr(ibuf)) == -1 and 'null' in msg()
    assert lib.dgsqp_fetch_monitor(h, _ffi.dptr(cl), _ffi.dptr(bx), None) == -1
    assert lib.dgsqp_fetch_monitor(h, _ffi.dptr(cl), _ffi.dptr(bx), _ffi.iptr(ibuf)) == 0
    assert np.isfinite(cl).all() and np.isfinite(bx).all() and (ibuf == -1).all()
    for off in (lambda: lib.dgsqp_set_monitor(h, 0), lambda: lib.dgsqp_set_estimate_noise(h, 0, 0, None), lambda: lib.dgsqp_set_plant_ensemble(h, 0, None, None),
                lambda: lib.dgsqp_set_plant(h, None)):
        assert off() == 0
    again = s.step_batch(x0, u_tm, T)
    for key in ('q', 'u', 'u_ws') + COUNTS:
        assert same(again[key], base[key]), key
