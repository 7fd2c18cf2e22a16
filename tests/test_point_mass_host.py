"""The Frenet point mass (``CasadiKinematicUnicycleCombined``, DGSQP_MODEL_UNICYCLE_COMBINED = 3) on the host: the enum, the class and
its module path, the lowering, the numpy mirror against the exact fixtures, the samplers' state layout, the plant's config
resolution and the refusals of ``plan``.  No GPU, no oracle (oracle/ has no model 3)."""
import dataclasses
import pathlib
import re

import numpy as np
import pytest

import point_mass_kat as pk

ROOT = pathlib.Path(__file__).resolve().parent.parent


def pm_game(kind='curve', **kw):
    from dgsqp_amd.montecarlo import point_mass_racing_game
    return point_mass_racing_game(kind, **kw)


def test_the_enum_is_in_the_header_and_in_the_ctypes_mirror():
    from dgsqp_amd import _ffi, dynamics
    header = (ROOT / 'include' / 'dgsqp.h').read_text()
    ids = {name: int(val) for name, val in re.findall(r'(DGSQP_MODEL_\w+)\s*=\s*(\d+)', header)}
    assert ids == {'DGSQP_MODEL_KIN_BICYCLE': 0, 'DGSQP_MODEL_DYN_BICYCLE': 1, 'DGSQP_MODEL_UNICYCLE': 2, 'DGSQP_MODEL_UNICYCLE_COMBINED': 3}
    assert (_ffi.MODEL_KIN_BICYCLE, _ffi.MODEL_DYN_BICYCLE, _ffi.MODEL_UNICYCLE, _ffi.MODEL_UNICYCLE_COMBINED) == (0, 1, 2, 3)
    assert dynamics.MODEL_UNICYCLE_COMBINED == 3 and dynamics.CasadiKinematicUnicycleCombined.model_id == 3
    assert (dynamics.CasadiKinematicUnicycleCombined.n_q, dynamics.CasadiKinematicUnicycleCombined.n_u) == (6, 2)


def test_the_reference_module_path_resolves_to_the_class():
    import dgsqp_amd
    from DGSQP.dynamics.dynamics_models import CasadiKinematicUnicycleCombined, CasadiDecoupledMultiAgentDynamicsModel  # noqa: F401  (game_setup_unicycle.py:8)
    from DGSQP.dynamics.model_types import UnicycleConfig
    assert CasadiKinematicUnicycleCombined is dgsqp_amd.CasadiKinematicUnicycleCombined is dgsqp_amd.dynamics.CasadiKinematicUnicycleCombined
    m = CasadiKinematicUnicycleCombined(0, UnicycleConfig(dt=0.1, mass=1.5, damping_coefficient=0.25), track=pm_game().track)
    assert (m.m, m.c_da, m.model_id) == (1.5, 0.25, 3)


def test_fill_vehicle_writes_mass_and_damping_and_defined_values_elsewhere():
    from dgsqp_amd import _ffi
    from dgsqp_amd.dynamics import UnicycleConfig
    from dgsqp_amd.solver import build_problem, fill_vehicle
    A = _ffi.AgentT()
    for name, _ in _ffi.AgentT._fields_[4:22]:
        setattr(A, name, np.nan)                         # whatever was there before
    fill_vehicle(A, 3, UnicycleConfig(mass=1.7, damping_coefficient=0.4, drag_coefficient=9.0, rolling_resistance=9.0))
    assert (A.model, A.mass, A.c_da) == (3, 1.7, 0.4)
    assert (A.c_dr, A.c_s, A.c_r) == (0.0, 0.0, 0.0)     # the reference's f_c reads neither drag nor rolling resistance: not passed on
    vehicle = [name for name, _ in _ffi.AgentT._fields_][:22]
    assert vehicle[0] == 'model' and vehicle[-1] == 'lin_Br'
    unread = [f for f in vehicle[4:] if f not in ('mass', 'c_da', 'pac_Bf', 'pac_Br', 'pac_Cf', 'pac_Cr', 'pac_Df', 'pac_Dr', 'lin_Bf', 'lin_Br')]
    assert all(np.isfinite(getattr(A, f)) for f in unread), [(f, getattr(A, f)) for f in unread]
    g = pm_game('barc')
    P = build_problem(*g.solver_args())
    assert (P.M, P.N, P.dt, P.integrator, P.substeps, P.obstacle_rows) == (2, 20, 0.1, 0, 1, 1)
    for a in range(2):
        B = P.agents[a]
        assert (B.model, B.mass, B.c_da, B.radius, B.has_rate, B.n_lane) == (3, 2.366, 0.0, 0.21, 0, 0)
        assert (tuple(B.w_in), tuple(B.w_rate), B.w_prog, B.w_comp, B.comp_type, B.w_block, B.w_obs) == ((0.1, 0.1), (0.0, 0.0), 1.0, 5.0, 0, 0.0, 0.0)
        assert (tuple(B.in_ub), tuple(B.in_lb)) == ((2.0, 2.0), (-2.0, -2.0))
        H = g.track.half_width
        assert list(B.st_ub[:6]) == [np.inf] * 5 + [H - 0.1] and list(B.st_lb[:6]) == [-np.inf] * 5 + [-(H - 0.1)]
    assert (g.params.reg, g.params.p_tol, g.params.d_tol, g.params.beta, g.params.tau, g.params.sqp_iters, g.params.line_search_iters,
            g.params.nonmono_ls, g.params.merit_function) == (0.0, 1e-3, 1e-3, 0.01, 0.5, 50, 50, True, 'stat_l1')


def test_qu2prediction_and_state_maps_field_for_field():
    from dgsqp_amd.types import VehiclePrediction, VehicleState
    m = pm_game().joint_model.dynamics_models[0]
    q = np.arange(18.0).reshape(3, 6)
    u = np.arange(4.0).reshape(2, 2) + 100
    pred = m.qu2prediction(None, q, u)
    assert isinstance(pred, VehiclePrediction)
    for name, col in (('x', 0), ('y', 1), ('v_long', 2), ('e_psi', 3), ('s', 4), ('x_tran', 5)):
        assert list(getattr(pred, name)) == list(q[:, col]), name
    assert list(pred.u_a) == list(u[:, 0]) and list(pred.u_steer) == list(u[:, 1])
    st = VehicleState()
    m.qu2state(st, q[1], u[0])
    assert (st.x.x, st.x.y, st.v.v_long, st.p.e_psi, st.p.s, st.p.x_tran, st.u.u_a, st.u.u_steer) == (*q[1], *u[0])
    assert np.array_equal(m.state2q(st), q[1])
    q2, u2 = m.state2qu(st)
    assert np.array_equal(q2, q[1]) and np.array_equal(u2, u[0])
    st2 = VehicleState()
    m.q2state(st2, q[2])
    assert np.array_equal(m.state2q(st2), q[2])


def test_fc_batch_is_fc_row_by_row():
    from dgsqp_amd.montecarlo import _fc_batch
    g = pm_game('chicane')
    m = type(g.joint_model.dynamics_models[0])(0, dataclasses.replace(g.joint_model.dynamics_models[0].model_config, mass=1.9, damping_coefficient=0.3),
                                                track=g.track)
    rng = np.random.default_rng(0)
    q = rng.standard_normal((40, 6))
    q[:, 2] += 2.0
    q[:, 4] = rng.uniform(0.0, g.track.track_length, 40)          # every segment of the chicane: c < 0, c = 0, c > 0
    q[:, 5] *= 0.3
    u = rng.standard_normal((40, 2))
    got = _fc_batch(m, q, u)
    want = np.stack([m.fc(q[i], u[i]) for i in range(40)])
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    curv = np.array([g.track.get_curvature(s) for s in q[:, 4]])
    assert (curv < 0).any() and (curv > 0).any() and (curv == 0).any()
    # the literal equations at one point (dynamics_models.py:536-541)
    (x, y, v, ep, s, xt), (Fx, wz) = q[0], u[0]
    c, pt = g.track.get_curvature(s), g.track.get_tangent_angle(s)
    lit = [v * np.cos(pt + ep), v * np.sin(pt + ep), (Fx - 0.3 * v) / 1.9, wz - c * (v * np.cos(ep)) / (1 - xt * c), v * np.cos(ep) / (1 - xt * c), v * np.sin(ep)]
    assert np.allclose(want[0], lit, rtol=1e-15, atol=0)


@pytest.mark.parametrize('case', pk.CASES)
def test_fixture_records_and_parameters(case):
    """The fixtures' own acc_* and margin records, their sens_* entries, and the game of the case field by field."""
    kat, g, P = pk.load(case)
    keys = ('x', 'g', 'q', 'Gv', 'Qv') if case in pk.DIRECTIONAL_CASES else ('x', 'g', 'q', 'G', 'Q')
    for k in keys:
        assert k in kat.files and float(kat['acc_' + k]) <= 1e-18 and 0.0 <= float(kat['sens_' + k]) < 1e-9, (case, k)
    assert float(kat['margin']) > 1e-3
    assert 2 <= len(kat['x0']) <= 3
    if case in pk.DIRECTIONAL_CASES:
        from dgsqp_amd.solver import build_params, plan
        assert plan(P, build_params(g.params, qp_method='active_set'))['layout'] == pk.DIRECTIONAL_CASES[case]
    if case == 'pm2_euler_N3':
        assert kat['x'][0, 0, 4] < 1.0 < kat['x'][0, 1, 4]       # car 1 crosses the segment boundary s = 1


@pytest.mark.parametrize('case', pk.CASES)
def test_host_fd_against_the_fixtures_stage_by_stage(case):
    """The numpy ``fd`` from the fixture's own x_k and u_k against its x_{k+1}, at the project's x bar.  Ties the numpy mirror to the
    mpmath transcription: the two were written from the reference separately.  (mix3: its point mass only.)"""
    kat, g, P = pk.load(case)
    rtol = max(pk.X_RTOL, 64.0 * float(kat['sens_x']))
    models, jc = g.joint_model.dynamics_models, g.joint_model.model_config
    qoff = np.concatenate(([0], np.cumsum([m.n_q for m in models])))
    N, worst, steps = P.N, 0.0, 0
    for b in range(len(kat['x0'])):
        x = kat['x'][b].reshape(N + 1, -1)
        assert np.array_equal(x[0], kat['x0'][b])
        for a, m in enumerate(models):
            if m.model_id != 3:
                continue
            ua = kat['u'][b][2 * N * a:2 * N * (a + 1)].reshape(N, 2)
            for k in range(N):
                got, want = pk.host_fd(m, jc, x[k, qoff[a]:qoff[a + 1]], ua[k]), x[k + 1, qoff[a]:qoff[a + 1]]
                worst = max(worst, float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()))
                np.testing.assert_allclose(got, want, rtol=rtol, atol=pk.X_ATOL, err_msg=f'{case} scenario {b} agent {a} stage {k}')
                steps += 1
    print(f'{case}: host fd against the exact x over {steps} steps, largest elementwise relative deviation {worst:.2e} (rtol {rtol:.1e})')
    assert steps > 0


def test_host_fd_integrators():
    """euler, rk2, rk3, rk4 with M sub-steps: each against its formula written out on fc (dynamics_models.py:88-99, :188-219)."""
    g = pm_game('curve')
    base = g.joint_model.dynamics_models[0]
    q, u = np.array([0.3, 0.1, 2.2, 0.05, 1.7, -0.2]), np.array([0.8, -0.6])
    for meth, M in (('euler', 1), ('euler', 3), ('rk2', 2), ('rk3', 2), ('rk4', 3)):
        m = type(base)(0, dataclasses.replace(base.model_config, discretization_method=meth, M=M, damping_coefficient=0.2), track=g.track)
        f, h, x = (lambda z: m.fc(z, u)), 0.1 / M, q.copy()
        if meth == 'euler':
            x = q + 0.1 * f(q)
        for _ in range(M if meth != 'euler' else 0):
            if meth == 'rk4':
                a1 = f(x); a2 = f(x + h / 2 * a1); a3 = f(x + h / 2 * a2); a4 = f(x + h * a3)
                x = x + h * (a1 + 2 * a2 + 2 * a3 + a4) / 6
            elif meth == 'rk3':
                a1 = h * f(x); a2 = h * f(x + a1 / 2); a3 = h * f(x - a1 + 2 * a2)
                x = x + (a1 + 4 * a2 + a3) / 6
            else:
                a1 = f(x); a2 = f(x + h * a1)
                x = x + h * (a1 + a2) / 2
        assert np.array_equal(m.fd(q, u), x), (meth, M)
    assert not np.array_equal(x, q)


def test_samplers_and_pid_warm_start_use_the_models_state_positions():
    """sample_scenarios / sample_scenarios_counter put s and x_tran at states 4, 5 and start with e_psi = 0 at state 3; the PID law steers
    on 5 (x_tran - x_tran0) + e_psi read from states 5 and 3: the first two steps by hand."""
    from dgsqp_amd import sampler as smp
    from dgsqp_amd.montecarlo import pid_warm_start, sample_scenarios
    g = pm_game('curve', N=6)
    m = g.joint_model.dynamics_models[0]
    assert (m.epsi_idx, m.s_idx, m.ey_idx) == (3, 4, 5)
    x0, u_ws = sample_scenarios(g, 6, seed=5)
    assert x0.shape == (6, 12) and u_ws.shape == (6, 6, 4)
    for a in range(2):
        q = x0[:, 6 * a:6 * a + 6]
        assert (q[:, 3] == 0).all() and (q[:, 2] >= 2).all() and (q[:, 2] <= 3).all() and (np.abs(q[:, 5]) <= g.half_width).all() and (q[:, 4] >= 0).all()
        xy = np.array([g.track.local_to_global((s, e, 0.0))[:2] for s, e in zip(q[:, 4], q[:, 5])])
        assert np.allclose(q[:, :2], xy, rtol=0, atol=1e-14)
    xc, uc, used = smp.sample_scenarios_counter(g, 6, seed=5, chunk=64)
    assert xc.shape == (6, 12) and (xc[:, 3] == 0).all() and (xc[:, 9] == 0).all() and used >= 6
    # circuit sampler (the race game's own track): e_psi is drawn, and lands in state 3
    gb = pm_game('barc', N=6)
    xb, _ = sample_scenarios(gb, 4, seed=2)
    assert (xb[:, 3] != 0).all() and (np.abs(xb[:, 3]) <= 5.0 * np.pi / 180).all() and (np.abs(xb[:, 5]) <= gb.half_width).all()
    # two steps of the lane follower by hand, from a state with e_psi and x_tran off their references
    q0 = np.array([[0.2, 0.3, 2.5, 0.07, 0.2, 0.3]])
    q0[0, :2] = g.track.local_to_global((0.2, 0.3, 0.0))[:2]
    q_ws, u = pid_warm_start(m, q0, 2, 0.1, du=(10.0, 4.5))
    rk4 = lambda q, uu: _rk4(m, q, uu, 0.1, 10)
    u0 = np.array([-(q0[0, 2] - q0[0, 2]), -(1.0 * q0[0, 3] + 0.005 * np.clip(q0[0, 3] * 0.1, -100, 100))])      # e = 5 (x_tran - x_tran0) + e_psi = e_psi
    u0 = np.clip(np.clip(u0, [-10.0, -4.5], [10.0, 4.5]), [-2.1, -0.436], [2.1, 0.436])
    q1 = rk4(q0[0], u0)
    e1 = 5.0 * (q1[5] - q0[0, 5]) + q1[3]
    ei = np.clip(q0[0, 3] * 0.1, -100, 100) + e1 * 0.1
    u1 = np.array([-(q1[2] - q0[0, 2]), -(e1 + 0.005 * ei)])
    u1 = np.clip(np.clip(u1 - u0, [-10.0, -4.5], [10.0, 4.5]) + u0, [-2.1, -0.436], [2.1, 0.436])
    q2 = rk4(q1, u1)
    assert np.allclose(u[0], [u0, u1], rtol=1e-13, atol=1e-15) and np.allclose(q_ws[0], [q0[0], q1, q2], rtol=1e-13, atol=1e-15)
    assert u0[1] < 0 and abs(u1[1]) > 0                  # it did steer on e_psi


def _rk4(m, q, u, dt, M):
    h = dt / M
    for _ in range(M):
        a1 = m.fc(q, u); a2 = m.fc(q + h / 2 * a1, u); a3 = m.fc(q + h / 2 * a2, u); a4 = m.fc(q + h * a3, u)
        q = q + h * (a1 + 2 * a2 + 2 * a3 + a4) / 6
    return q


def test_plant_resolves_a_unicycle_config_by_the_games_agent(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel, config_model_id
    from dgsqp_amd.dynamics import DynamicBicycleConfig, KinematicBicycleConfig, UnicycleConfig
    from dgsqp_amd.solver import build_problem
    assert [config_model_id(UnicycleConfig(), gm) for gm in (None, 0, 1, 2, 3)] == [2, 2, 2, 2, 3]
    assert config_model_id(KinematicBicycleConfig(), 3) == 0 and config_model_id(DynamicBicycleConfig(), 3) == 1
    g = pm_game('curve', N=5)
    P = build_problem(*g.solver_args())
    cfgs = [UnicycleConfig(dt=0.1, mass=2.0, damping_coefficient=0.1), UnicycleConfig(dt=0.1, mass=3.0, damping_coefficient=0.2)]
    pt = PlantModel(dynamics_configs=cfgs, method='rk4', M=2, sim_steps=2).lower(P)
    assert [(pt.agents[a].model, pt.agents[a].mass, pt.agents[a].c_da) for a in range(2)] == [(3, 2.0, 0.1), (3, 3.0, 0.2)]
    vehicles, delay = PlantModel(per_chain_configs=[cfgs, cfgs[::-1]]).lower_ensemble(P, 2)
    assert delay is None and [(v.model, v.mass) for v in vehicles] == [(3, 2.0), (3, 3.0), (3, 3.0), (3, 2.0)]
    for other in (KinematicBicycleConfig(), DynamicBicycleConfig()):
        with pytest.raises(ValueError, match='model class'):
            PlantModel(dynamics_configs=[cfgs[0], other]).lower(P)
        with pytest.raises(ValueError, match='model class'):
            PlantModel(per_chain_configs=[[cfgs[0], other]]).lower_ensemble(P, 1)
    # a bicycle game still refuses it, a merge game (class 2) still takes it as class 2
    with pytest.raises(ValueError, match='model class 2'):
        PlantModel(dynamics_configs=[KinematicBicycleConfig(), UnicycleConfig()]).lower(games['kb_curve_N10'][1])
    with pytest.raises(ValueError, match='model class 2'):
        PlantModel(dynamics_configs=[UnicycleConfig()] * 2).lower(games['dyn_curve_N15'][1])
    pm = PlantModel(dynamics_configs=[UnicycleConfig()] * 3).lower(games['merge_N8'][1])
    assert [pm.agents[a].model for a in range(3)] == [2, 2, 2]
    assert _ffi.VehicleT is not None


def test_plan_refuses_a_spline_track_and_allows_the_racing_costs():
    from dgsqp_amd.dynamics import CasadiDecoupledMultiAgentDynamicsModel
    from dgsqp_amd.solver import build_params, build_problem, plan
    from dgsqp_amd.tracks import get_track
    g = pm_game('curve', N=5)
    par = build_params(g.params)
    P = build_problem(*g.solver_args())
    d = plan(P, par)
    assert (d['n_q'], d['n_u'], d['n'], d['layout']) == (12, 4, 20, 0)
    # progress, competition and blocking costs are allowed (the unicycle of class 2 refuses them)
    P.agents[0].w_block = 0.5
    assert plan(P, par)['n'] == 20
    P.agents[0].model = 2
    with pytest.raises(ValueError, match='Frenet-frame model'):
        plan(P, par)
    # a spline track
    f1 = get_track('f1_austin_tenth_scale')
    models = [type(m)(0, m.model_config, track=f1) for m in g.joint_model.dynamics_models]
    gs = dataclasses.replace(g, joint_model=CasadiDecoupledMultiAgentDynamicsModel(0, models, g.joint_model.model_config), track=f1)
    Ps = build_problem(*gs.solver_args())
    assert Ps.track_kind == 1
    with pytest.raises(ValueError, match='arc tracks only'):
        plan(Ps, par)
    # ... also when only one of the agents is a point mass
    Ps.agents[0].model = 0
    with pytest.raises(ValueError, match='arc tracks only'):
        plan(Ps, par)
    Ps.agents[1].model = 0
    assert plan(Ps, par)['n'] == 20
    P4 = build_problem(*g.solver_args())
    P4.agents[1].model = 4
    with pytest.raises(ValueError, match='unsupported vehicle model'):
        plan(P4, par)
