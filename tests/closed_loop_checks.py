"""The checks the closed-loop GPU tests share (tests/test_closed_loop.py and its _plant, _ensemble and _drivers siblings), one copy of each.

* TEACHER FORCING (``teacher_force``): every (state, warm start) pair a chain went through is stacked into ONE ``solve_batch`` call on the
  same solver, and u, l, x, cond, cost, status, num_iters and qp_solves of that call must equal the closed-loop records bit for bit -- the
  state is q_est[t] with estimates, q[t] otherwise.
* The feedback between two steps: without a plant exactly against the host mirror ``closed_loop.feedback`` (``check_feedback``); with one
  the warm-start chain and the records of steps that never ran (``check_chain``), and the plant itself (``check_plant``): ``q[t+1]``
  against the CPU oracle's next state, one control step at a time from the device's own ``q[t]`` and ``u_plant[t]`` with CHAIN b's vehicle
  record and delays, 1e-12 relative to max(1, |q|_inf) (``BAR``: the device-against-oracle bar for x), and
  ``u_plant`` bit for bit against the delay lines of ``closed_loop.plant_feedback``: it is data movement.
* The monitor (``check_monitor``) against ``closed_loop.monitor`` fed with the oracle's z_j.  With eps = 1e-12 max(1, |z|_inf) each position
  coordinate is within eps and a pair distance is 1-Lipschitz in each of its four coordinates, so clearance is held to 4 eps; a box excess
  is one difference of a state entry and a constant and is held to 2 eps.  A case is only valid when every monitored pairwise clearance is
  at least 1e-6 in magnitude by the oracle (else a hit could be decided by rounding): the check asserts that."""
import copy

import numpy as np
import pytest

DOUBLES = ('u', 'l', 'x', 'cond', 'cost')
COUNTS = ('status', 'num_iters', 'qp_solves')
CHAIN = DOUBLES + COUNTS + ('q', 'u_ws', 'u_applied', 'u_plant', 'steps_done')
BAR = 1e-12
DELAYS = [[2, 1], [0, 3]]
WORST = {}          # case -> largest relative deviation of q[t+1] from the oracle (printed by every case)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """Bit for bit (stricter than np.array_equal: NaN payloads and the sign of zero count)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))


@pytest.fixture(scope='module')
def solver_of(games):
    """name -> DGSQP of conftest's game of that name, built once per module (a test module imports this fixture by name)."""
    from dgsqp_amd.solver import DGSQP
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = DGSQP(*games[name][0].solver_args(), print_method=None, **kw)
        return cache[key]
    yield get
    cache.clear()


def scenarios(g, B, seed):
    from dgsqp_amd.montecarlo import sample_scenarios
    return sample_scenarios(g, B, seed=seed)


def configs_of(g, **scale):
    """Copies of the game's per-agent dynamics configs; ``scale``: field -> factor (every agent) or {agent: factor}."""
    cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
    for field, f in scale.items():
        for a, c in enumerate(cfgs):
            k = f.get(a, 1.0) if isinstance(f, dict) else f
            setattr(c, field, getattr(c, field) * k)
    return cfgs


def teacher_force(s, res):
    """One solve_batch over every step that ran, from the state its solve started from; returns how many steps that were."""
    bb, tt = np.nonzero(np.arange(res['status'].shape[1])[None, :] < res['steps_done'][:, None])
    start = res['q_est'] if 'q_est' in res else res['q']
    ref = s.solve_batch(start[bb, tt], res['u_ws'][bb, tt])
    for key in DOUBLES + COUNTS:
        got = res[key][bb, tt]
        bad = [(int(bb[i]), int(tt[i])) for i in range(len(bb)) if not same(got[i], ref[key][i])]
        assert not bad, f'{key}: closed-loop steps (scenario, step) {bad[:8]} differ from solve_batch on the same inputs'
    assert [res['msg'][b][t] for b, t in zip(bb, tt)] == ref['msg']
    assert same(res['converged'][bb, tt], ref['converged'])
    return len(bb)


def check_start(s, res, x0, u_am):
    """The start of the chains, the shapes, u_applied."""
    B, T = res['status'].shape
    assert same(res['q'][:, 0], x0) and same(res['u_ws'][:, 0], u_am)
    assert res['q'].shape == (B, T + 1, s.n_q) and res['u_ws'].shape == (B, T + 1, s.n) and res['u_pred'].shape == (B, T, s.N, s.n_u)
    assert same(res['u_applied'], res['u_pred'][:, :, 0]) and same(res['u_pred'], s._to_time_major(res['u']))


def check_idle(res, t, idle, ok):
    """The chains that did not run step t: status -1 / 'not_run', zero counts, NaN everywhere -- and no warm start after a step that ended
    its chain (``~ok``)."""
    assert (res['status'][idle, t] == -1).all() and (res['num_iters'][idle, t] == 0).all() and (res['qp_solves'][idle, t] == 0).all()
    assert all(res['msg'][b][t] == 'not_run' for b in np.nonzero(idle)[0]) and not res['converged'][idle, t].any()
    for key in DOUBLES:
        assert np.isnan(res[key][idle, t]).all(), (key, t)
    assert np.isnan(res['u_ws'][idle | ~ok, t + 1]).all() and np.isnan(res['q'][idle, t + 1]).all(), t


def check_feedback(s, res, x0, u_am, w=None):
    """Without a plant: q / u_ws chains, u_applied and the records of steps that never ran."""
    from dgsqp_amd import closed_loop
    T = res['status'].shape[1]
    done = res['steps_done']
    check_start(s, res, x0, u_am)
    for t in range(T):
        ran = t < done
        q_next, ws_next, ok = closed_loop.feedback(res['x'][:, t], res['u'][:, t], res['status'][:, t], res['u_ws'][:, t],
                                                   w=None if w is None else w[:, t], num_ua_d=s.num_ua_d)
        assert np.array_equal(res['q'][ran, t + 1], q_next[ran], equal_nan=True) and same(res['q'][ran & ok, t + 1], q_next[ran & ok]), t
        assert same(res['u_ws'][ran & ok, t + 1], ws_next[ran & ok]), t
        assert np.array_equal(done[ran], np.where(ok[ran], np.maximum(done[ran], t + 1), t + 1)), t      # a chain ends at its first non-finite state
        check_idle(res, t, ~ran, ok)            # ... and nothing was started from a non-finite state
    assert ((done >= 1) & (done <= T)).all()


def check_chain(s, res, x0, u_am, min_done=1, stopped=None):
    """With a plant: the warm-start chain, u_applied, steps_done and the records of steps that never ran (check_feedback without its q rule:
    the next state is checked against the oracle instead).  ``stopped`` [B]: the control step after which the monitor ended the chain, or
    -1 -- no warm start is written after it, as after a non-finite state."""
    from dgsqp_amd import closed_loop
    B, T = res['status'].shape
    done = res['steps_done']
    stopped = np.full(B, -1) if stopped is None else np.asarray(stopped)
    check_start(s, res, x0, u_am)
    for t in range(T):
        ran = t < done
        ok = np.isfinite(res['q'][:, t + 1]).all(axis=-1) & (stopped != t)
        _, ws_next, _ = closed_loop.feedback(res['x'][:, t], res['u'][:, t], res['status'][:, t], res['u_ws'][:, t], num_ua_d=s.num_ua_d)
        assert same(res['u_ws'][ran & ok, t + 1], ws_next[ran & ok]), t
        assert np.array_equal(done[ran], np.where(ok[ran], np.maximum(done[ran], t + 1), t + 1)), t      # a chain ends at its first non-finite state or hit
        check_idle(res, t, ~ran, ok)
        assert np.isnan(res['u_plant'][~ran, t]).all() and np.isfinite(res['u_plant'][ran, t]).all(), t
        for key in ('clearance', 'box_excess'):
            if key in res:
                assert np.isnan(res[key][~ran, t]).all(), (key, t)
    assert ((done >= min_done) & (done <= T)).all()


def plant_problem(P, pt, vehicles=None):
    """The game's POD as ONE simulation step of a chain's plant: dt / S, the plant's integrator and sub-steps, and the vehicle fields of
    ``vehicles`` (M records of the chain), else of the plant."""
    from dgsqp_amd import _ffi
    P2 = _ffi.ProblemT.from_buffer_copy(P)
    P2.dt = P.dt / pt.sim_steps
    P2.integrator, P2.substeps = pt.integrator, pt.substeps
    src = vehicles if vehicles is not None else (None if pt.use_game_agents else pt.agents)
    if src is not None:
        for a in range(P.M):
            for name, _ in _ffi.AgentT._fields_[:22]:               # model .. lin_Br
                setattr(P2.agents[a], name, getattr(src[a], name))
    return P2


def check_plant(oracle, s, res, plant, w=None, tag='', chains=None):
    """q[t+1] against the oracle with CHAIN b's vehicle record, u_plant against the host mirror's delay lines with chain b's delays.
    ``chains``: which chains of the ensemble the rows of ``res`` are (default: the first B).  Records the largest relative deviation in
    ``WORST[tag]`` and prints it.  Returns Z [B, T, S, n_q], the oracle's state after every simulation step (the last one with w: NaN
    where a step never ran), for the monitor's check."""
    from dgsqp_amd import closed_loop
    P = s._problem
    pt = plant.lower(P)
    B, T = res['status'].shape
    S, M = pt.sim_steps, s.M
    chains = np.arange(B) if chains is None else np.asarray(chains)
    vehicles, delays = (None, None)
    if plant.per_chain:
        n_all = len(plant.per_chain_configs) if plant.per_chain_configs is not None else len(plant.per_chain_delay_steps)
        vehicles, delays = plant.lower_ensemble(P, n_all)
    assert res['u_plant'].shape == (B, T, S, s.n_u)
    qoff = np.concatenate(([0], np.cumsum(s.num_qa_d)))
    Z = np.full((B, T, S, s.n_q), np.nan)
    worst = 0.0
    for b in range(B):
        c = int(chains[b])
        P2 = plant_problem(P, pt, None if vehicles is None else [vehicles[c * M + a] for a in range(M)])
        delay = delays[c] if delays is not None else [[pt.delay[a][j] for j in range(2)] for a in range(M)]
        lines = closed_loop.new_lines(delay)
        for t in range(int(res['steps_done'][b])):
            _, used, _ = closed_loop.plant_feedback(lambda q, u: q, res['q'][b, t], res['u_applied'][b, t], lines, sim_steps=S)
            assert same(res['u_plant'][b, t], used), f'{tag}: u_plant of chain {b}, step {t} is not what its delay lines deliver'
            q = res['q'][b, t].copy()
            for j in range(S):
                for a in range(M):
                    q[qoff[a]:qoff[a + 1]] = oracle.dynamics(P2, a, q[qoff[a]:qoff[a + 1]], res['u_plant'][b, t, j, 2 * a:2 * a + 2], derivs=False)[1]
                if j == S - 1 and w is not None:
                    q = q + w[b, t]
                Z[b, t, j] = q
            got = res['q'][b, t + 1]
            if not np.isfinite(q).all():
                assert np.array_equal(np.isfinite(got), np.isfinite(q)), (tag, b, t)
                continue
            worst = max(worst, float(np.abs(got - q).max() / max(1.0, np.abs(q).max())))
    WORST[tag] = worst
    print(f'{tag}: max |q[t+1] - oracle| / max(1, |q|_inf) = {worst:.3e} over {int(res["steps_done"].sum())} control steps (bar {BAR:g})')
    assert worst < BAR, (tag, worst)
    return Z


def game_bounds(s):
    """(radii [M], st_lb [n_q], st_ub [n_q], qoff [M+1]) of the solver's game."""
    P = s._problem
    qoff = np.concatenate(([0], np.cumsum(s.num_qa_d)))
    lb = np.concatenate([[P.agents[a].st_lb[i] for i in range(s.num_qa_d[a])] for a in range(s.M)])
    ub = np.concatenate([[P.agents[a].st_ub[i] for i in range(s.num_qa_d[a])] for a in range(s.M)])
    return np.array([P.agents[a].radius for a in range(s.M)]), lb, ub, qoff


def check_monitor(s, res, Z, tag=''):
    """clearance, box_excess and hit_step against closed_loop.monitor on the oracle's Z; asserts the validity condition of the case."""
    from dgsqp_amd import closed_loop
    radii, lb, ub, qoff = game_bounds(s)
    assert (radii > 0).all(), 'the monitor needs a game whose agents have a radius'
    B, T, S, _ = Z.shape
    worst_c = worst_b = 0.0
    closest = np.inf
    for b in range(B):
        first = -1
        for t in range(int(res['steps_done'][b])):
            z = Z[b, t]
            cl, bx, hit = closed_loop.monitor(z, radii, lb, ub, qoff)
            if not np.isfinite(z).all():
                assert np.isnan(res['clearance'][b, t]) and np.isnan(res['box_excess'][b, t]), (tag, b, t)
                continue
            for i in range(s.M):                                   # validity: no monitored pair is within 1e-6 of touching
                for k in range(i + 1, s.M):
                    d = np.hypot(z[:, qoff[i]] - z[:, qoff[k]], z[:, qoff[i] + 1] - z[:, qoff[k] + 1]) - (radii[i] + radii[k])
                    closest = min(closest, float(np.abs(d).min()))
            eps = BAR * max(1.0, float(np.abs(z).max()))
            dc, db = abs(res['clearance'][b, t] - cl), abs(res['box_excess'][b, t] - bx)
            worst_c, worst_b = max(worst_c, dc / eps), max(worst_b, db / eps)
            assert dc <= 4 * eps and db <= 2 * eps, (tag, b, t, dc, db, eps)
            if hit >= 0 and first < 0:
                first = t * S + int(hit)
        assert res['hit_step'][b] == first, (tag, b, int(res['hit_step'][b]), first)
    print(f'{tag}: |clearance - mirror| <= {worst_c:.2e} eps (bar 4 eps), |box_excess - mirror| <= {worst_b:.2e} eps (bar 2 eps), '
          f'eps = 1e-12 max(1, |z|_inf); closest monitored pair is {closest:.3e} from touching (validity: >= 1e-6)')
    assert closest >= 1e-6, (tag, closest)
