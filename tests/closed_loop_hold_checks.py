"""The checks the GPU tests of held plans share (tests/test_closed_loop_hold.py), on top of tests/closed_loop_checks.py.

* TEACHER FORCING (``teacher_force_solved``): every step that SOLVED (status >= 0) is re-solved in one ``solve_batch`` from its recorded
  start -- q_est[t] with estimates, q[t] otherwise --, u_ws[t] and, where the launch carried it, u_prev[t], bit for bit.  (``closed_loop_checks.teacher_force`` would include the held
  steps, which ran no solve.)
* THE HELD PLAN (``check_plan_chain``): ``closed_loop.hold_step`` replays the recorded statuses from (age, due) = (0, True); the device's
  u_game[t], u_ws[t+1], plan_stage[t] and "status == held exactly when no plan was due" must equal the mirror's bit for bit.  Held steps and
  steps that never ran carry exactly their fill values.
* THE PLANT (``closed_loop_checks.check_plant``): u_plant bit for bit against the delay-line mirror fed with the command that entered the
  plant -- u_game, or u_cmd with drivers -- and q[t+1] against the CPU oracle at its existing bar, 1e-12 relative to max(1, |q|_inf)."""
import numpy as np

from closed_loop_checks import COUNTS, DOUBLES, check_idle, check_monitor, check_plant, same

HELD = -2


def teacher_force_solved(s, res):
    """One solve_batch over every step that solved; returns how many that were."""
    T = res['status'].shape[1]
    ran = np.arange(T)[None, :] < res['steps_done'][:, None]
    assert (res['status'][ran] != -1).all() and (res['status'][~ran] == -1).all()
    bb, tt = np.nonzero(res['status'] >= 0)
    if len(bb) == 0:
        return 0
    start = res['q_est'] if 'q_est' in res else res['q']
    ref = s.solve_batch(start[bb, tt], res['u_ws'][bb, tt], u_prev=res['u_prev'][bb, tt] if 'u_prev' in res else None)
    for key in DOUBLES + COUNTS:
        got = res[key][bb, tt]
        bad = [(int(bb[i]), int(tt[i])) for i in range(len(bb)) if not same(got[i], ref[key][i])]
        assert not bad, f'{key}: closed-loop steps (scenario, step) {bad[:8]} differ from solve_batch on the same inputs'
    assert [res['msg'][b][t] for b, t in zip(bb, tt)] == ref['msg']
    assert same(res['converged'][bb, tt], ref['converged'])
    return len(bb)


def check_plan_chain(s, res, x0, u_am, hold, stopped=None, min_done=1):
    """The start of the chains, the held plan against ``hold_step``, steps_done, and the fill values of held and never-run steps.
    ``stopped`` as in ``closed_loop_checks.check_chain``.  Returns (solved, held): how many steps of each kind ran."""
    from dgsqp_amd import closed_loop
    B, T = res['status'].shape
    done = res['steps_done']
    stopped = np.full(B, -1) if stopped is None else np.asarray(stopped)
    assert same(res['q'][:, 0], x0) and same(res['u_ws'][:, 0], u_am)
    assert res['q'].shape == (B, T + 1, s.n_q) and res['u_ws'].shape == (B, T + 1, s.n) and res['u_pred'].shape == (B, T, s.N, s.n_u)
    assert res['u_game'].shape == (B, T, s.n_u) and res['plan_stage'].shape == (B, T) and res['plan_stage'].dtype == np.int32
    assert res['u_applied'] is res['u_game'] or same(res['u_applied'], res['u_game'])
    assert same(res['u_pred'], s._to_time_major(res['u']))
    n_solved = n_held = 0
    for b in range(B):
        age, due = 0, True
        for t in range(int(done[b])):
            status = int(res['status'][b, t])
            assert (status == HELD) == (not due), (b, t, status, due)                     # a chain solves exactly when a plan is due
            assert status == HELD or 0 <= status <= 5, (b, t, status)
            u_game, ws_next, age, due, stage = closed_loop.hold_step(None if status == HELD else status, res['u'][b, t], res['u_ws'][b, t], age, due,
                                                                     hold, s.N, s.num_ua_d)
            assert same(res['u_game'][b, t], u_game), (b, t, 'u_game')
            assert int(res['plan_stage'][b, t]) == stage, (b, t, int(res['plan_stage'][b, t]), stage)
            went_on = np.isfinite(res['q'][b, t + 1]).all() and stopped[b] != t
            assert (int(done[b]) == t + 1) or went_on, (b, t)                             # a chain ends at its first non-finite state or hit
            if went_on:
                assert same(res['u_ws'][b, t + 1], ws_next), (b, t, 'u_ws')
            else:
                assert np.isnan(res['u_ws'][b, t + 1]).all(), (b, t)
            if status == HELD:
                n_held += 1
                assert res['msg'][b][t] == 'held' and not res['converged'][b, t]
                assert res['num_iters'][b, t] == 0 and res['qp_solves'][b, t] == 0
                for key in DOUBLES:
                    assert np.isnan(res[key][b, t]).all(), (key, b, t)
                if 'q_est' in res:
                    assert np.isnan(res['q_est'][b, t]).all(), (b, t)
            else:
                n_solved += 1
                assert res['msg'][b][t] not in ('held', 'not_run')
    for t in range(T):
        idle = ~(t < done)
        ok = np.isfinite(res['q'][:, t + 1]).all(axis=-1) & (stopped != t)
        check_idle(res, t, idle, ok)
        assert (res['plan_stage'][idle, t] == -1).all() and np.isnan(res['u_game'][idle, t]).all(), t
        assert np.isnan(res['u_plant'][idle, t]).all() and np.isfinite(res['u_plant'][~idle, t]).all(), t
        for key in ('clearance', 'box_excess', 'q_est', 'u_cmd'):
            if key in res:
                assert np.isnan(res[key][idle, t]).all(), (key, t)
    assert ((done >= min_done) & (done <= T)).all()
    return n_solved, n_held


def check_all(oracle, s, res, x0, u_tm, hold, plant, tag='', w=None, stopped=None, min_done=1):
    """The checks common to every case.  Returns dict(solved, held, Z)."""
    n_solved, n_held = check_plan_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), hold, stopped=stopped, min_done=min_done)
    assert teacher_force_solved(s, res) == n_solved
    entered = res['u_cmd'] if 'u_cmd' in res else res['u_game']
    Z = check_plant(oracle, s, dict(res, u_applied=entered), plant, w, tag)
    if 'clearance' in res:
        check_monitor(s, res, Z, tag)
    print(f'{tag}: {n_solved} solved and {n_held} held steps')
    return dict(solved=n_solved, held=n_held, Z=Z)
