"""The checks the GPU tests of cross plants share (tests/test_closed_loop_cross.py), on top of tests/closed_loop_checks.py and
tests/closed_loop_hold_checks.py.  A cross plant (``PlantModel(own_class=True)``, ``dgsqp_set_cross_plant``) keeps a state z of its own and
the game sees the projection q = p(z).  ``check_cross``:

* TEACHER FORCING of every step that solved (``teacher_force_solved``) and the held plan -- u_game, u_ws[t+1], plan_stage -- bit for bit
  against ``closed_loop.hold_step`` (``check_plan_chain``; a launch without a hold runs the default one);
* q == p(z) bit for bit on every slice a chain wrote, NaN in both beyond;
* u_cmd of GAME and REPLAY agents bit for bit; u_plant bit for bit against the delay-line mirror fed with u_cmd;
* z[t+1] against ``oracle.dynamics`` on a PLANT GAME of the plant agent's class -- built by the package's constructors on the game's track,
  with dt / S, the plant's integrator and sub-steps and chain b's vehicle record --, one simulation step at a time from the device's own
  z[t] and u_plant[t]: 1e-12 relative to max(1, |z|_inf), row R1's bar, as for every plant.  The CPU oracle has no
  Frenet point mass; a plant agent of that class (the identity pair 3 -> 3 only) is advanced by the numpy model's ``fd`` at the same bar, as
  tests/test_point_mass.py does;
* track_ref against ``closed_loop.track_reference`` (the numpy model of the game's agent, the joint model's discretisation) from the
  device's z[t] and u_game[t], at the same bar;
* u_cmd of PID and TRACK agents against ``closed_loop.drive`` fed with the device's RECORDED track_ref, 1e-12 max(1, |z[t]|_inf): the law is
  a handful of fp64 operations on entries of z[t] and the references with gains kp_s ey_gain <= 10, kp_v <= 10 (the drivers' bound, f5).

Every figure is printed (pytest -s) before it is asserted; ``WORST[tag]`` keeps them."""
import numpy as np

from closed_loop_checks import BAR, same
from closed_loop_hold_checks import check_plan_chain, teacher_force_solved

WORST = {}
NQ = {0: 6, 1: 8, 2: 4, 3: 6}


def plant_bases(track='curve'):
    """class -> ProblemT of a game of that class on the game's track, from the package's constructors: what the oracle integrates a plant
    agent of that class with (its vehicle record, step and integrator are replaced per chain in ``agent_problem``)."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import build_problem
    if track == 'f1':
        games = {0: mc.f1_racing_game(N=10), 1: mc.f1_racing_game(N=10, model='dynamic')}
    else:
        games = {0: mc.kinematic_racing_game('curve', N=10), 1: mc.dynamic_racing_game(N=10, rk4_substeps=4, game_def='curve')}
    return {c: build_problem(*g.solver_args()) for c, g in games.items()}


def agent_problem(base, a, P, pt, vehicle):
    """``base`` with agent a's vehicle fields from ``vehicle``, ONE simulation step long, the plant's integrator and sub-steps."""
    from dgsqp_amd import _ffi
    P2 = _ffi.ProblemT.from_buffer_copy(base)
    P2.dt = P.dt / pt.sim_steps
    P2.integrator, P2.substeps = pt.integrator, pt.substeps
    for name, _ in _ffi.AgentT._fields_[:22]:               # model .. lin_Br
        setattr(P2.agents[a], name, getattr(vehicle, name))
    return P2


def point_mass_step(game, plant, pt, a):
    """One simulation step of a point-mass plant agent: the numpy model with the plant's config, dt / S, integrator and sub-steps."""
    import dataclasses
    jc = game.joint_model.model_config
    m = game.joint_model.dynamics_models[a]
    method = plant.method or jc.discretization_method
    cfg = plant.dynamics_configs[a] if plant.dynamics_configs is not None else m.model_config
    one = type(m)(0, dataclasses.replace(cfg, dt=jc.dt / pt.sim_steps, discretization_method=method, M=pt.substeps if method != 'euler' else 1), track=game.track)
    return one.fd


def check_cross(oracle, s, res, game, x0, u_tm, plant, bases, drivers=None, hold=None, z0=None, tag='', stopped=None, min_done=1):
    """Every check of the module's docstring.  ``game``: the Game the solver was built from; ``bases``: ``plant_bases``.  Returns
    dict(solved, held, Z): Z [B, T, S, n_q] the PROJECTED oracle states after every simulation step, for ``check_monitor``."""
    from test_closed_loop_drivers import chain_kinds
    from dgsqp_amd import closed_loop
    from dgsqp_amd.closed_loop import Drivers, PlanHold
    P = s._problem
    pt = plant.lower(P)
    B, T = res['status'].shape
    M, S, dt = s.M, pt.sim_steps, float(P.dt)
    gcls = [int(P.agents[a].model) for a in range(M)]
    pcls = plant.plant_classes(P)
    zoff = np.concatenate(([0], np.cumsum([NQ[c] for c in pcls])))
    qoff = np.concatenate(([0], np.cumsum(s.num_qa_d)))
    drivers = Drivers() if drivers is None else drivers
    hold = PlanHold() if hold is None else hold
    z = res['z']
    done = res['steps_done']
    assert z.shape == (B, T + 1, zoff[-1]) and res['u_plant'].shape == (B, T, S, s.n_u) and res['u_cmd'].shape == (B, T, s.n_u)
    assert same(z[:, 0], closed_loop.lift_state(gcls, pcls, x0) if z0 is None else np.asarray(z0, float))
    # a chain ends on a non-finite entry of z[t+1] (or a hit: ``stopped``)
    ended = np.full(B, -1) if stopped is None else np.array(stopped)
    for b in range(B):
        for t in range(int(done[b])):
            if not np.isfinite(z[b, t + 1]).all():
                assert int(done[b]) == t + 1, (tag, b, t)
                ended[b] = t
    n_solved, n_held = check_plan_chain(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), hold, stopped=ended, min_done=min_done)
    assert teacher_force_solved(s, res) == n_solved
    # q = p(z), bit for bit
    for b in range(B):
        d = int(done[b])
        assert same(res['q'][b, :d + 1], closed_loop.project_state(gcls, pcls, z[b, :d + 1])), (tag, b, 'q != p(z)')
        assert np.isnan(z[b, d + 1:]).all() and np.isnan(res['q'][b, d + 1:]).all(), (tag, b)
    kinds = chain_kinds(drivers, B, M)
    gains = drivers.gains(M)
    rep = None if drivers.u_replay is None else np.asarray(drivers.u_replay, float)
    tracked = any(k == 3 for row in kinds for k in row)
    assert ('track_ref' in res) == tracked
    vehicles = delays = None
    if plant.per_chain:
        n_all = len(plant.per_chain_configs) if plant.per_chain_configs is not None else len(plant.per_chain_delay_steps)
        vehicles, delays = plant.lower_ensemble(P, n_all)
    jc = game.joint_model.model_config
    Z = np.full((B, T, S, s.n_q), np.nan)
    worst = dict(z=0.0, track_ref=0.0, u_cmd=0.0)
    for b in range(B):
        veh = [vehicles[b * M + a] if vehicles is not None else (P.agents[a] if pt.use_game_agents else pt.agents[a]) for a in range(M)]
        for a in range(M):
            assert veh[a].model == pcls[a]
        assert vehicles is None or 3 not in pcls, 'no per-chain point-mass plants here: the oracle has no such model'
        step = [point_mass_step(game, plant, pt, a) if pcls[a] == 3 else
                (lambda q, u, a=a, P2=agent_problem(bases[pcls[a]], a, P, pt, veh[a]): oracle.dynamics(P2, a, q, u, derivs=False)[1]) for a in range(M)]
        delay = delays[b] if delays is not None else [[pt.delay[a][j] for j in range(2)] for a in range(M)]
        lines = closed_loop.new_lines(delay)
        refs = (np.array([[z[b, 0, zoff[a] + 2], z[b, 0, zoff[a + 1] - 1]] for a in range(M)]) if drivers.refs is None
                else np.asarray(drivers.refs, float)[b])
        states = closed_loop.new_pid_state((M,))
        if tracked:
            assert np.isnan(res['track_ref'][b, int(done[b]):]).all(), (tag, b)
        for t in range(int(done[b])):
            zt, g = z[b, t], res['u_game'][b, t]
            scale = max(1.0, float(np.abs(zt).max())) if np.isfinite(zt).all() else np.nan
            # the reference of every TRACK agent, from the device's z[t] and u_game[t]
            if tracked:
                for a in range(M):
                    got = res['track_ref'][b, t, a]
                    if kinds[b][a] != 3:
                        assert np.isnan(got).all(), (tag, b, t, a)
                        continue
                    qa = closed_loop.project_state([gcls[a]], [pcls[a]], zt[zoff[a]:zoff[a + 1]])
                    xr = closed_loop.track_reference(game.joint_model.dynamics_models[a], qa, g[2 * a:2 * a + 2],
                                                     method=jc.discretization_method, dt=jc.dt, M=jc.M)
                    want = np.array([xr[2], xr[-1], xr[5 if len(xr) == 8 else 3]])
                    if np.isfinite(want).all():
                        worst['track_ref'] = max(worst['track_ref'], float(np.abs(got - want).max() / scale))
            want, states = closed_loop.drive(kinds[b], g, zt, gains, refs, states, dt, zoff, u_replay=None if rep is None else rep[b, t],
                                             track_refs=res['track_ref'][b, t] if tracked else None)
            got = res['u_cmd'][b, t]
            for a in range(M):
                sl = slice(2 * a, 2 * a + 2)
                if kinds[b][a] in (0, 2):
                    assert same(got[sl], want[sl]), (tag, 'game / replay command', b, t, a)
                elif np.isfinite(want[sl]).all():
                    worst['u_cmd'] = max(worst['u_cmd'], float(np.abs(got[sl] - want[sl]).max() / scale))
            _, used, _ = closed_loop.plant_feedback(lambda q, u: q, zt, got, lines, sim_steps=S)
            assert same(res['u_plant'][b, t], used), f'{tag}: u_plant of chain {b}, step {t} is not what its delay lines deliver'
            zz = zt.copy()
            for j in range(S):
                for a in range(M):
                    zz[zoff[a]:zoff[a + 1]] = step[a](zz[zoff[a]:zoff[a + 1]], res['u_plant'][b, t, j, 2 * a:2 * a + 2])
                Z[b, t, j] = closed_loop.project_state(gcls, pcls, zz)
            got = z[b, t + 1]
            if not np.isfinite(zz).all():
                assert not np.isfinite(got).all(), (tag, b, t)
                continue
            worst['z'] = max(worst['z'], float(np.abs(got - zz).max() / max(1.0, np.abs(zz).max())))
    WORST[tag] = worst
    print(f'{tag}: max |z[t+1] - oracle| / max(1, |z|_inf) = {worst["z"]:.3e}, |track_ref - track_reference| / max(1, |z[t]|_inf) = '
          f'{worst["track_ref"]:.3e}, |u_cmd - drive| / max(1, |z[t]|_inf) = {worst["u_cmd"]:.3e} (bar {BAR:g} each) over '
          f'{int(done.sum())} control steps; {n_solved} solved, {n_held} held')
    assert worst['z'] < BAR and worst['track_ref'] < BAR and worst['u_cmd'] < BAR, (tag, worst)
    return dict(solved=n_solved, held=n_held, Z=Z)
