"""Drivers of closed-loop batches on the device: DGSQP.step_batch(..., drivers=Drivers(...)) / dgsqp_set_drivers, dgsqp_fetch_u_cmd (the
drivers' fields of DgPlantPack and step 2 of dev_plant_feedback, csrc/dgsqp_closed_loop.h): per agent and per chain the command that enters the plant
is stage 0 of the game's solution, the PID lane follower run closed-loop on the true state, or a replayed sequence.

The idiom is that of tests/test_closed_loop_ensemble.py, with the helpers of tests/closed_loop_checks.py: TEACHER FORCING, the warm-start
chain, u_plant bit for bit against the delay-line mirror -- now fed with u_cmd, the commands the plants received -- and q[t+1] against the CPU oracle at
1e-12 relative to max(1, |q|_inf).  On top of that ``check_commands``: u_cmd of a game agent is bit for bit stage 0 of u, of a replay agent
bit for bit u_replay, of a PID agent within 1e-12 max(1, |q[t]|_inf) of ``closed_loop.pid_driver_step`` stepped from the device's own
q[t].  That bar: the law is under twenty roundings of 2^-53 per step, the device may contract multiply-add pairs (so it is not bit for
bit), each rounding is amplified by at most kp_s ey_gain <= 10 and carried through at most three steps by the 1-Lipschitz clamps: about
2e-13."""
import ctypes

import numpy as np
import pytest

from closed_loop_checks import (BAR, CHAIN, COUNTS, DELAYS, DOUBLES, check_chain, check_monitor, check_plant, configs_of, same, scenarios,
                                 solver_of, teacher_force)      # noqa: F401  (solver_of is a fixture)

pytestmark = pytest.mark.gpu

PLANT_KW = dict(method='rk4', M=3, sim_steps=2, delay_steps=DELAYS)


def qoff_of(s):
    return np.concatenate(([0], np.cumsum(s.num_qa_d)))


def chain_kinds(drivers, B, M):
    from dgsqp_amd.closed_loop import _kind_id
    if drivers.per_chain_kinds is not None:
        return [[_kind_id(k) for k in row] for row in drivers.per_chain_kinds]
    return [[_kind_id(k) for k in (drivers.kinds if drivers.kinds is not None else [0] * M)]] * B


def check_commands(s, res, drivers, tag=''):
    """u_cmd against closed_loop.drive stepped from the device's own TRUE q[t] and its stage 0.  Returns dict(worst, rate, free, state0):
    the largest PID deviation relative to max(1, |q[t]|_inf), how many steering commands of PID agents the mirror found rate-saturated and
    how many neither rate- nor magnitude-saturated, and the mirror's PID states after step 0 [B, M, 3]."""
    from dgsqp_amd import closed_loop
    B, T = res['status'].shape
    M, qoff, dt = s.M, qoff_of(s), float(s._problem.dt)
    gains = drivers.gains(M)
    kinds = chain_kinds(drivers, B, M)
    assert res['u_cmd'].shape == (B, T, s.n_u)
    rep = None if drivers.u_replay is None else np.asarray(drivers.u_replay, float)
    out = dict(worst=0.0, rate=0, free=0, state0=np.zeros((B, M, 3)))
    for b in range(B):
        x0 = res['q'][b, 0]
        refs = np.array([[x0[qoff[a] + 2], x0[qoff[a + 1] - 1]] for a in range(M)]) if drivers.refs is None else np.asarray(drivers.refs, float)[b]
        states = closed_loop.new_pid_state((M,))
        done = int(res['steps_done'][b])
        assert np.isnan(res['u_cmd'][b, done:]).all(), (tag, b)
        for t in range(done):
            prev = states
            want, states = closed_loop.drive(kinds[b], res['u_applied'][b, t], res['q'][b, t], gains, refs, states, dt, qoff,
                                             u_replay=None if rep is None else rep[b, t])
            if t == 0:
                out['state0'][b] = states
            got = res['u_cmd'][b, t]
            for a in range(M):
                sl = slice(2 * a, 2 * a + 2)
                if kinds[b][a] != 1:
                    assert same(got[sl], want[sl]), (tag, 'game / replay command', b, t, a)
                    continue
                err = float(np.abs(got[sl] - want[sl]).max() / max(1.0, np.abs(res['q'][b, t]).max()))
                out['worst'] = max(out['worst'], err)
                step = abs(want[2 * a + 1] - prev[a, 2])
                out['rate'] += int(step >= gains[a].du_max[1] * (1 - 1e-12))
                out['free'] += int(step < gains[a].du_max[1] * (1 - 1e-9) and abs(want[2 * a + 1]) < gains[a].u_max[1])
    print(f'{tag}: max |u_cmd - pid_driver_step| / max(1, |q[t]|_inf) = {out["worst"]:.3e} (bar {BAR:g}); steering commands of the PID agents: '
          f'{out["rate"]} rate-saturated, {out["free"]} unsaturated')
    assert out['worst'] < BAR, (tag, out['worst'])
    return out


def run_and_check(oracle, s, x0, u_tm, T, plant, drivers, tag='', min_done=1, **kw):
    """The four checks of every case (teacher forcing, the warm-start chain, u_plant against the delay lines fed with u_cmd, q[t+1] against the
    oracle) and the commands; with monitor='stop' a chain that was hit ends after that control step."""
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=drivers, **kw)
    stopped = None
    if kw.get('monitor') == 'stop':
        stopped = np.where(res['hit_step'] >= 0, res['hit_step'] // plant.sim_steps, -1)
        assert np.array_equal(res['steps_done'][stopped >= 0], stopped[stopped >= 0] + 1), tag
    check_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), min_done=min_done, stopped=stopped)
    teacher_force(s, res)
    Z = check_plant(oracle, s, dict(res, u_applied=res['u_cmd']), plant, kw.get('disturbance'), tag)
    if 'clearance' in res:
        check_monitor(s, res, Z, tag)
    return res, check_commands(s, res, drivers, tag)


def refs_around_x0(s, x0, offsets):
    """[B, M, 2]: v_ref = v of x0, lat_ref = e_y of x0 + offsets[b] (so the first steering command of chain b is -ey_gain * -offsets[b])."""
    qoff = qoff_of(s)
    return np.array([[[x0[b, qoff[a] + 2], x0[b, qoff[a + 1] - 1] + offsets[b]] for a in range(s.M)] for b in range(len(x0))])


def test_all_game_drivers_are_the_plain_plant(oracle, games, solver_of):
    """Case 1: every agent on GAME: every output is bit-identical to the same launch without drivers, and u_cmd is u_applied."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    plant = PlantModel(**PLANT_KW)
    plain = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant)
    for tag, drivers in (('default', Drivers()), ('kinds', Drivers(kinds=['game', 'game'])), ('per chain', Drivers(per_chain_kinds=[[0, 0]] * 5))):
        res, _ = run_and_check(oracle, s, x0, u_tm, 3, plant, drivers, f'all game ({tag})')
        for key in CHAIN:
            assert same(res[key], plain[key]), (tag, key)
        assert same(res['u_cmd'], res['u_applied']) and 'u_cmd' not in plain
    assert (plain['steps_done'] == 3).all()
    # without a plant argument the identity plant is used
    ident = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=PlantModel())
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True, drivers=Drivers())
    for key in CHAIN:
        assert same(res[key], ident[key]), key


def test_replay_of_the_games_own_commands(oracle, games, solver_of):
    """Case 2: agent 1 replays what the game applied for it in a plain-plant run: every output is bit-identical to that run."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 5, 43)
    plant = PlantModel(**PLANT_KW)
    A = s.step_batch(x0, u_tm, 3, keep_predictions=True, plant=plant)
    rep = np.full_like(A['u_applied'], 123.0)                     # agent 0's entries are not read
    rep[:, :, 2:4] = A['u_applied'][:, :, 2:4]
    Bres, _ = run_and_check(oracle, s, x0, u_tm, 3, plant, Drivers(kinds=['game', 'replay'], u_replay=rep), 'replay of the game')
    for key in CHAIN:
        assert same(Bres[key], A[key]), key
    assert same(Bres['u_cmd'], A['u_applied'])


@pytest.mark.parametrize('name,B,T,kw,wg', [
    ('kb_curve_N10', 5, 3, PLANT_KW, 1),
    ('dyn_curve_N15', 3, 2, dict(M=5, sim_steps=2), 1),
    ('kb_curve_N10', 5, 3, PLANT_KW, 2),                           # case 7: the build with 256-thread workgroups
])
def test_pid_opponent(oracle, games, solver_of, name, B, T, kw, wg):
    """Cases 3 and 7: agent 0 plays the game, agent 1 is the lane follower (kp_s ey_gain = 5).  Chain 0's lateral reference is 0.2 beside
    its e_y, so its first steering command (-1.0 before the clamps) is rate-saturated at du_max = 0.05; chain 1's is 0.002 beside it
    (-0.01: unsaturated); the others take x0's."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g = games[name][0]
    s = solver_of(name, **(dict(workgroups_per_cu=2) if wg == 2 else {}))
    x0, u_tm = scenarios(g, B, 43)
    plant = PlantModel(**kw)
    A = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    refs = refs_around_x0(s, x0, [0.2, 0.002] + [0.0] * (B - 2))
    refs[:, :, 0] += 0.3                                          # a speed reference 0.3 above x0's: the first u_a is 0.3 in every chain
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(ki_s=0.05, du_max=(10.0, 0.05)), refs=refs)
    res, m = run_and_check(oracle, s, x0, u_tm, T, plant, drivers, f'PID opponent {name}, {wg} workgroup(s) per CU')
    assert same(res['u_cmd'][:, :, :2], res['u_applied'][:, :, :2])             # the game agent's command IS stage 0 of u
    assert m['rate'] >= 1 and m['free'] >= 1, m
    assert (res['steps_done'] == T).all() and (A['steps_done'] == T).all()
    for b in range(B):
        assert np.abs(res['q'][b, 1:] - A['q'][b, 1:]).max() > 1e-6, b          # the opponent really deviated


def test_kinds_per_chain(oracle, games, solver_of):
    """Case 4: a row of kinds and a pair of references per chain."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 6, 3
    x0, u_tm = scenarios(g, B, 43)
    plant = PlantModel(**PLANT_KW)
    A = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    rows = [['game', 'game'], ['pid', 'game'], ['game', 'pid'], ['game', 'replay'], ['pid', 'pid'], ['game', 'game']]
    rep = np.full_like(A['u_applied'], np.nan)                   # only chain 3's agent 1 is on replay: no other entry is read
    rep[3, :, 2:4] = 0.5 * A['u_applied'][3, :, 2:4] + 0.01
    refs = refs_around_x0(s, x0, [0.0, 0.2, 0.002, 0.0, -0.1, 0.0])
    refs[:, :, 0] += 0.1 * np.arange(B)[:, None]                 # and a speed reference of its own per chain
    drivers = Drivers(per_chain_kinds=rows, pid=[PidGains(ki_s=0.05, du_max=(0.5, 0.05)), PidGains(kp_s=0.8, ki_s=0.1, du_max=(10.0, 0.08))], refs=refs,
                      u_replay=rep)
    res, m = run_and_check(oracle, s, x0, u_tm, T, plant, drivers, 'kinds per chain')
    for b in (0, 5):
        for key in CHAIN:
            assert same(res[key][b], A[key][b]), (b, key)
        assert same(res['u_cmd'][b], A['u_applied'][b])
    assert (res['steps_done'] == T).all() and (A['steps_done'] == T).all()
    for b in (1, 2, 3, 4):
        assert np.abs(res['q'][b, 1:] - A['q'][b, 1:]).max() > 1e-6, b
    assert m['rate'] >= 1 and m['free'] >= 1, m
    assert same(res['u_cmd'][3, :, 2:4], rep[3, :, 2:4])


def test_no_pid_state_survives_beyond_the_grid(oracle, games, solver_of):
    """Case 5: one scenario copied to 600 chains (more than the grid: a workgroup starts a second chain after its first), agent 1 on PID
    with an integrator.  Every chain is chain 0 bit for bit."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(g, 4, 43)
    x0[0, qoff_of(s)[1] + 3] = 0.05                               # e_psi of agent 1: an error for the integrator at step 0
    x0, u_tm = np.repeat(x0[:1], 600, axis=0), np.repeat(u_tm[:1], 600, axis=0)
    refs = refs_around_x0(s, x0, [0.0] * 600)
    refs[:, :, 0] += 0.2                                          # (so that the previous u_a is not zero either)
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(ki_s=0.3, du_max=(10.0, 0.04)), refs=refs)
    plant = PlantModel(method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    res = s.step_batch(x0, u_tm, 2, keep_predictions=True, plant=plant, drivers=drivers)
    few = {k: v[:3] for k, v in res.items() if k in CHAIN + ('u_cmd', 'u_pred', 'msg', 'converged')}
    drivers = Drivers(kinds=['game', 'pid'], pid=drivers.pid, refs=refs[:3])
    check_chain(s, few, x0[:3], s._to_agent_major(u_tm[:3]))
    assert teacher_force(s, few) == 6
    check_plant(oracle, s, dict(few, u_applied=few['u_cmd']), plant, tag='beyond the grid, first 3 of 600')
    m = check_commands(s, few, drivers, 'beyond the grid, first 3 of 600')
    assert (m['state0'][:, 1] != 0).all(), m['state0']            # integrator and previous command are non-zero after step 0: a leak would show
    assert (res['steps_done'] == 2).all()
    for key in CHAIN + ('u_cmd',):
        assert same(res[key], np.broadcast_to(res[key][:1], res[key].shape)), key


def test_combined_with_the_further_settings(oracle, games, solver_of):
    """Case 6: per-chain vehicles, estimate noise and monitor='stop' with a PID opponent (references from x0): the PID command follows the
    mirror on the TRUE q[t] -- and not on q_est[t]."""
    from dgsqp_amd import closed_loop
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel, perturbed_configs
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 4, 3
    x0, u_tm = scenarios(g, B, 61)
    plant = PlantModel(per_chain_configs=perturbed_configs(configs_of(g), dict(mass=0.1), B, seed=1), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    v = 1e-2 * np.random.default_rng(3).standard_normal((B, T, s.n_q))
    drivers = Drivers(kinds=['game', 'pid'], pid=PidGains(ki_s=0.05, du_max=(10.0, 0.05)))
    res, m = run_and_check(oracle, s, x0, u_tm, T, plant, drivers, 'drivers with vehicles, estimates, monitor', min_done=0, estimate_noise=v, monitor='stop')
    assert {'q_est', 'clearance', 'box_excess', 'hit_step', 'u_plant', 'u_cmd'} <= set(res)
    assert (res['steps_done'] >= 1).all()
    ran = np.arange(T)[None, :] < res['steps_done'][:, None]
    assert same(res['q_est'][ran], (res['q'][:, :T] + v)[ran])
    # stepped from the estimates instead, the mirror is far from the device's commands: the check above tells the two apart
    qoff, gains = qoff_of(s), drivers.gains(s.M)
    far = 0.0
    for b in range(B):
        refs = [[x0[b, qoff[a] + 2], x0[b, qoff[a + 1] - 1]] for a in range(s.M)]
        want, _ = closed_loop.drive([0, 1], res['u_applied'][b, 0], res['q_est'][b, 0], gains, refs, closed_loop.new_pid_state((s.M,)), float(s._problem.dt), qoff)
        far = max(far, float(np.abs(want - res['u_cmd'][b, 0]).max()))
    assert far > 1e-4, far


def test_nan_replay_entry_ends_that_chain(oracle, games, solver_of):
    """Case 8: a NaN in u_replay of chain 2 at step 1 makes q[2] of that chain non-finite: the chain ends there, the others do not notice."""
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 4, 3
    x0, u_tm = scenarios(g, B, 43)
    plant = PlantModel(method='rk4', M=2, sim_steps=2)              # no delay: the entry is integrated in the step it is given
    rep = np.zeros((B, T, s.n_u))
    rep[:, :, 2:4] = [0.3, 0.02]
    clean, _ = run_and_check(oracle, s, x0, u_tm, T, plant, Drivers(kinds=['game', 'replay'], u_replay=rep), 'replay, clean')
    assert (clean['steps_done'] == T).all()
    rep2 = rep.copy()
    rep2[2, 1, 3] = np.nan
    res = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant, drivers=Drivers(kinds=['game', 'replay'], u_replay=rep2))
    teacher_force(s, res)
    assert res['steps_done'].tolist() == [T, T, 2, T]
    assert same(res['u_cmd'][2, 1, :2], res['u_applied'][2, 1, :2]) and same(res['u_plant'][2, 1], np.stack([res['u_cmd'][2, 1]] * 2))
    assert not np.isfinite(res['q'][2, 2]).all() and np.isnan(res['q'][2, 3]).all() and np.isnan(res['u_ws'][2, 2:]).all()
    assert (res['status'][2, 2:] == -1).all() and np.isnan(res['u_cmd'][2, 2:]).all() and np.isnan(res['u_plant'][2, 2:]).all()
    assert np.isnan(res['u_cmd'][2, 1, 3]) and same(res['u_cmd'][2, 1, :3], clean['u_cmd'][2, 1, :3])
    others = [0, 1, 3]
    for key in CHAIN + ('u_cmd',):
        assert same(res[key][others], clean[key][others]), key
        if key != 'steps_done':
            assert same(res[key][2, :1], clean[key][2, :1]), key


def test_coexistence(oracle, games, solver_of):
    """Case 9: after a driver launch, a plain-plant launch, a plant-less launch and solve_batch on the same handle give what they gave."""
    from dgsqp_amd.closed_loop import Drivers, PidGains, PlantModel
    g = games['kb_curve_N10'][0]
    s = solver_of('kb_curve_N10')
    B, T = 5, 3
    x0, u_tm = scenarios(g, B, 67)
    plant = PlantModel(dynamics_configs=configs_of(g, mass=1.2), method='rk4', M=2, sim_steps=2, delay_steps=DELAYS)
    sol_a = s.solve_batch(x0, u_tm)
    less_a = s.step_batch(x0, u_tm, T, keep_predictions=True)
    plain_a = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    res, _ = run_and_check(oracle, s, x0, u_tm, T, plant, Drivers(kinds=['pid', 'game'], pid=PidGains(du_max=(0.5, 0.05))), 'coexistence')
    assert not same(res['q'], plain_a['q'])
    plain_b = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    less_b = s.step_batch(x0, u_tm, T, keep_predictions=True)
    sol_b = s.solve_batch(x0, u_tm)
    for key in CHAIN:
        assert same(plain_a[key], plain_b[key]), key
        if key != 'u_plant':
            assert same(less_a[key], less_b[key]), key
    for key in DOUBLES + COUNTS:
        assert same(sol_a[key], sol_b[key]), key
    for out in (plain_b, less_b):
        assert 'u_cmd' not in out
    with pytest.raises(ValueError, match='u_replay'):              # what Drivers refuses never reaches the library, and leaves nothing behind
        s.step_batch(x0, u_tm, T, plant=plant, drivers=Drivers(kinds=['game', 'replay']))
    again = s.step_batch(x0, u_tm, T, keep_predictions=True, plant=plant)
    for key in CHAIN:
        assert same(again[key], plain_a[key]), key


def test_argument_errors_through_the_c_abi(games, solver_of):
    """Case 10: every refusal is DGSQP_E_ARG with a message starting 'drivers: ' and leaves the next launch clean."""
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import Drivers, PlantModel
    from dgsqp_amd.solver import DGSQP, _record_ptrs
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None)                  # a handle of its own: nothing has run on it
    lib, h = s._lib, s._h
    B, T, M = 2, 2, 2
    x0, u_tm = scenarios(g, B, 73)
    msg = lambda: lib.dgsqp_last_error(h).decode()
    d, _, _, _ = Drivers(kinds=['game', 'pid']).lower(s._problem, B, T)
    buf = np.empty(T * B * s.n_u)
    rep = np.zeros((T, B, s.n_u))
    assert lib.dgsqp_fetch_u_cmd(h, _ffi.dptr(buf), buf.size) == -1 and 'no closed-loop launch' in msg()
    # no plant set: switching on is refused, switching off is fine
    assert lib.dgsqp_set_drivers(h, ctypes.byref(d), T, B, None, None, None) == -1 and msg().startswith('drivers: ') and 'no plant' in msg()
    assert lib.dgsqp_set_drivers(h, None, 0, 0, None, None, None) == 0 and lib.dgsqp_set_drivers(None, None, 0, 0, None, None, None) == -1
    pt = PlantModel(sim_steps=2).lower(s._problem)
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0

    def launch(t=T, b=B):
        sm = dict(q=np.empty((t + 1, b, s.n_q)), u_ws=np.empty((t + 1, b, s.n)), **s._records((t, b), predictions=False))
        done = np.empty(b, np.int32)
        rc = lib.dgsqp_closed_loop_batch(h, b, t, _ffi.dptr(x0[:b]), _ffi.dptr(s._to_agent_major(u_tm[:b])), None, _ffi.dptr(sm['q']), _ffi.dptr(sm['u_ws']),
                                         *_record_ptrs(sm), _ffi.iptr(done), None)
        return rc, sm

    rc, plain = launch()
    assert rc == 0

    def refused(call, word):
        assert call() == -1
        assert msg().startswith('drivers: ') and word in msg(), msg()
        rc, sm = launch()                                               # the refusal left nothing behind
        assert rc == 0 and all(same(sm[k], plain[k]) for k in ('q', 'u', 'u_ws', 'status'))

    def with_kind(a, value):
        d2, _, _, _ = Drivers(kinds=['game', 'pid']).lower(s._problem, B, T)
        d2.kind[a] = value
        return lambda: lib.dgsqp_set_drivers(h, ctypes.byref(d2), T, B, None, None, _ffi.dptr(rep))

    def with_chain_kind(value, replay=rep):
        kind = np.zeros((B, M), np.int32)
        kind[1, 0] = value
        return lambda: lib.dgsqp_set_drivers(h, ctypes.byref(d), T, B, _ffi.iptr(kind), None, _ffi.dptr(replay))

    refused(with_kind(1, 3), 'kind')
    refused(with_kind(0, -1), 'kind')
    refused(with_chain_kind(3), 'kind')
    refused(with_chain_kind(-2), 'kind')
    refused(with_chain_kind(2, None), 'u_replay')
    d_rep, _, _, _ = Drivers(kinds=['game', 'replay'], u_replay=np.zeros((B, T, s.n_u))).lower(s._problem, B, T)
    refused(lambda: lib.dgsqp_set_drivers(h, ctypes.byref(d_rep), T, B, None, None, None), 'u_replay')
    refused(lambda: lib.dgsqp_set_drivers(h, ctypes.byref(d), 0, B, None, None, None), 'T')
    refused(lambda: lib.dgsqp_set_drivers(h, ctypes.byref(d), T, -1, None, None, None), 'negative')
    # a launch whose T or B differs from what the drivers were set for
    assert lib.dgsqp_set_drivers(h, ctypes.byref(d), T, B, None, None, None) == 0
    for t, b in ((T + 1, B), (T, B - 1)):
        rc, _ = launch(t, b)
        assert rc == -1 and msg().startswith('drivers: ') and f'T = {t}, B = {b}' in msg(), msg()
    # drivers that outlive their plant are refused by the launch
    assert lib.dgsqp_set_plant(h, None) == 0
    rc, _ = launch()
    assert rc == -1 and msg().startswith('drivers: ') and 'no plant' in msg()
    assert lib.dgsqp_set_plant(h, ctypes.byref(pt)) == 0
    # the fetcher after a launch with drivers
    rc, sm = launch()
    assert rc == 0
    assert lib.dgsqp_fetch_u_cmd(h, _ffi.dptr(buf), buf.size - 1) == -1 and 'too small' in msg()
    assert lib.dgsqp_fetch_u_cmd(h, None, buf.size) == -1
    assert lib.dgsqp_fetch_u_cmd(h, _ffi.dptr(buf), buf.size) == 0
    u_cmd = buf.reshape(T, B, s.n_u)
    stage0 = s._to_time_major(sm['u'])[:, :, 0]
    assert np.isfinite(u_cmd).all() and same(u_cmd[:, :, :2], stage0[:, :, :2]) and not same(u_cmd[:, :, 2:], stage0[:, :, 2:])
    assert lib.dgsqp_set_drivers(h, None, 0, 0, None, None, None) == 0
    rc, sm = launch()
    assert rc == 0 and all(same(sm[k], plain[k]) for k in ('q', 'u', 'u_ws', 'status'))
    # PID for a unicycle
    u = DGSQP(*games['merge_N8'][0].solver_args(), print_method=None)
    assert u._lib.dgsqp_set_plant(u._h, ctypes.byref(PlantModel().lower(u._problem))) == 0
    du = _ffi.DriversT()
    du.kind[1] = _ffi.DRIVER_PID
    assert u._lib.dgsqp_set_drivers(u._h, ctypes.byref(du), T, B, None, None, None) == -1
    err = u._lib.dgsqp_last_error(u._h).decode()
    assert err.startswith('drivers: ') and 'unicycle' in err, err
    kind = np.zeros((B, 3), np.int32)
    kind[0, 2] = _ffi.DRIVER_PID
    du.kind[1] = _ffi.DRIVER_GAME
    assert u._lib.dgsqp_set_drivers(u._h, ctypes.byref(du), T, B, _ffi.iptr(kind), None, None) == -1 and 'unicycle' in u._lib.dgsqp_last_error(u._h).decode()
    assert u._lib.dgsqp_set_drivers(u._h, ctypes.byref(du), T, B, None, None, None) == 0 and u._lib.dgsqp_set_drivers(u._h, None, 0, 0, None, None, None) == 0
