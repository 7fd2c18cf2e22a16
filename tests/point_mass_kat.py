"""Helper of the known-answer tests of the Frenet point mass (``CasadiKinematicUnicycleCombined``, DGSQP_MODEL_UNICYCLE_COMBINED):
the ``pm*`` / ``mix*`` cases of tools/make_multistage_kats.py.  tests/multistage_kat.py has fixed model maps, so the games and the
parameter check of these cases live here; the comparison (``compare``, ``bar``, ``rel``) and the bars are that module's.

No oracle: oracle/ has no model 3 (it would run the kinematic bicycle in its place), so nothing here or in the tests that use this
helper evaluates a game that contains a point mass with it.  The answers are the generator's (mpmath, independent of oracle/ and of
dgsqp_amd/csrc); the numpy ``fd`` of dgsqp_amd/dynamics.py is tied to them by tests/test_point_mass_host.py."""
import dataclasses

import numpy as np

from multistage_kat import DEVICE_BAR, GOLD, X_ATOL, X_RTOL, bar, compare, rel  # noqa: F401

SMALL_CASES = ('pm2_euler_N3', 'pm2_rk4_N4', 'mix3_rk4m3_N3')
DIRECTIONAL_CASES = {'pm3_N20_dir': 1, 'pm3_N25_dir': 2}            # case -> the device layout it is there for (1 big, 2 XL)
CASES = SMALL_CASES + tuple(DIRECTIONAL_CASES)
PM_CASES = tuple(c for c in CASES if c.startswith('pm'))            # every agent a point mass

_MODEL_ID = {'kin': 0, 'dyn': 1, 'uni': 2, 'pm': 3}
_NQ = {'kin': 6, 'dyn': 8, 'uni': 4, 'pm': 6}


def _joint(models, method, substeps):
    from dgsqp_amd.dynamics import CasadiDecoupledMultiAgentDynamicsModel, MultiAgentModelConfig
    return CasadiDecoupledMultiAgentDynamicsModel(0, models, MultiAgentModelConfig(
        dt=0.1, discretization_method=method, use_mx=False, code_gen=False, verbose=False, compute_hessians=True, M=substeps))


def build_game(case):
    from dgsqp_amd.dynamics import CasadiDynamicBicycleCombined, CasadiKinematicBicycleCombined, CasadiKinematicUnicycleCombined
    from dgsqp_amd.game import CollisionAvoidance, InputRateLimits, RacingCost
    from dgsqp_amd.montecarlo import dynamic_racing_game, kinematic_racing_game, point_mass_racing_game
    if case == 'pm2_euler_N3':
        return point_mass_racing_game('curve', N=3)
    if case == 'pm2_rk4_N4':
        g = point_mass_racing_game('chicane', N=4)
        models = [CasadiKinematicUnicycleCombined(0, dataclasses.replace(m.model_config, discretization_method='rk4', M=2, mass=1.9,
                                                                         damping_coefficient=0.3), track=g.track)
                  for m in g.joint_model.dynamics_models]
        cost = lambda: RacingCost(input_weight=(0.1, 0.1), input_rate_weight=(0.3, 0.2), comp_weights=(1.0, 5.0), comp_type='linear',
                                  blocking_weight=0.7, obs_weight=3.0, obs_r=0.9)
        return dataclasses.replace(g, joint_model=_joint(models, 'rk4', 2), costs=[cost(), cost()],
                                   agent_constraints=[InputRateLimits((10.0, 4.5), (-10.0, -4.5)) for _ in range(2)])
    if case == 'mix3_rk4m3_N3':
        # (kinematic bicycle, point mass, dynamic bicycle): each agent as its own game has it, on the kinematic game's track object
        kin, pm, dyn = kinematic_racing_game('curve', N=3), point_mass_racing_game('curve', N=3), dynamic_racing_game(N=3, rk4_substeps=3)
        with_int = lambda cfg, **over: dataclasses.replace(cfg, discretization_method='rk4', M=3, **over)
        models = [CasadiKinematicBicycleCombined(0, with_int(kin.joint_model.dynamics_models[0].model_config), track=kin.track),
                  CasadiKinematicUnicycleCombined(0, with_int(pm.joint_model.dynamics_models[0].model_config, damping_coefficient=0.2), track=kin.track),
                  CasadiDynamicBicycleCombined(0, with_int(dyn.joint_model.dynamics_models[0].model_config), track=kin.track)]
        bounds = {k: [kin.bounds[k][0], pm.bounds[k][0], dyn.bounds[k][0]] for k in ('ub', 'lb')}
        return dataclasses.replace(kin, joint_model=_joint(models, 'rk4', 3), costs=[kin.costs[0], pm.costs[0], dyn.costs[0]],
                                   agent_constraints=[kin.agent_constraints[0], None, None], shared_constraints=CollisionAvoidance([0.2] * 3),
                                   bounds=bounds, name='mix3_rk4m3_N3')
    if case in DIRECTIONAL_CASES:
        return point_mass_racing_game('curve', N={'pm3_N20_dir': 20, 'pm3_N25_dir': 25}[case], M=3)
    raise ValueError(case)


_VEHICLE_FIELDS = {'wheel_dist_front': 'L_f', 'wheel_dist_rear': 'L_r', 'mass': 'mass', 'drag_coefficient': 'c_dr', 'damping_coefficient': 'c_da',
                   'slip_coefficient': 'c_s', 'rolling_resistance': 'c_r', 'rolling_resistance_exponent': 'p_r', 'yaw_inertia': 'I_z', 'gravity': 'gravity',
                   'simple_slip': 'simple_slip', 'tire_model': 'tire_model', 'drive_wheels': 'drive_wheels', 'pacejka_b_front': 'pac_Bf',
                   'pacejka_b_rear': 'pac_Br', 'pacejka_c_front': 'pac_Cf', 'pacejka_c_rear': 'pac_Cr', 'pacejka_d_front': 'pac_Df',
                   'pacejka_d_rear': 'pac_Dr', 'linear_bf': 'lin_Bf', 'linear_br': 'lin_Br'}
_CODES = {'tire_model': {'pacejka': 0, 'linear': 1}, 'drive_wheels': {'all': 0, 'rear': 1}}


def assert_same_parameters(kat, P):
    """Every ``p_*`` entry of the fixture against the problem record the package builds, field by field and exactly; a parameter of the
    fixture that nothing was compared with fails."""
    from dgsqp_amd.dynamics import INTEGRATORS
    same = lambda got, want, what: np.testing.assert_array_equal(np.asarray(got, float), np.asarray(want, float), err_msg=what)
    seen = set()

    def take(key):
        seen.add(key)
        v = kat[key]
        return v.item() if v.ndim == 0 else v
    M = take('p_M')
    assert (P.M, P.N, P.dt, P.substeps, P.obstacle_rows) == (M, take('p_N'), take('p_dt'), take('p_substeps'), take('p_obstacle_rows'))
    assert P.integrator == INTEGRATORS[take('p_method')]
    assert take('p_has_track') == 1
    n = len(take('p_track_seg_curv'))
    assert P.n_segs == n and P.track_L == take('p_track_L') and P.track_kind == 0
    same(P.seg_s[:n + 1], take('p_track_seg_s'), 'seg_s'); same(P.seg_curv[:n], kat['p_track_seg_curv'], 'seg_curv')
    same(P.seg_ang[:n + 1], take('p_track_seg_ang'), 'seg_ang')
    for a in range(M):
        A, pre = P.agents[a], f'p_a{a}_'
        model = take(pre + 'model')
        nq = _NQ[model]
        assert A.model == _MODEL_ID[model], (a, A.model, model)
        for name, field in _VEHICLE_FIELDS.items():
            if pre + 'vehicle_' + name in kat.files:
                want = take(pre + 'vehicle_' + name)
                assert getattr(A, field) == _CODES.get(name, {}).get(want, want), (a, name, getattr(A, field), want)
        same(A.w_in, take(pre + 'cost_input_weight'), 'w_in'); same(A.w_rate, take(pre + 'cost_input_rate_weight'), 'w_rate')
        assert take(pre + 'cost_kind') == 'racing'
        same([A.w_prog, A.w_comp], take(pre + 'cost_comp_weights'), 'comp_weights')
        assert A.comp_type == {'atan': 0, 'linear': 1}[take(pre + 'cost_comp_type')]
        assert (A.w_block, A.w_obs) == (take(pre + 'cost_blocking_weight'), take(pre + 'cost_obs_weight'))
        if A.w_obs != 0:
            assert A.obs_cost_r == take(pre + 'cost_obs_r')
        seen.add(pre + 'cost_obs_r')                    # (read only under a non-zero obstacle weight)
        assert not any(A.w_goal)
        assert A.has_rate == take(pre + 'has_rate')
        if A.has_rate:
            same([A.rate_ub, A.rate_lb], take(pre + 'rate'), 'rate')
        assert A.n_lane == take(pre + 'n_lane') == 0
        same(A.in_ub, take(pre + 'in_ub'), 'in_ub'); same(A.in_lb, take(pre + 'in_lb'), 'in_lb')
        same(A.st_ub[:nq], take(pre + 'st_ub'), 'st_ub'); same(A.st_lb[:nq], take(pre + 'st_lb'), 'st_lb')
        assert A.radius == take(pre + 'radius')
    left = {k for k in kat.files if k.startswith('p_')} - seen
    assert not left, f'parameters of the fixture that nothing was compared with: {sorted(left)}'


def load(case):
    """(fixture, Game, problem record) of a case, the parameters checked and the fixture's own records within the generator's rules."""
    from dgsqp_amd.solver import build_problem
    kat = np.load(GOLD / f'multistage_{case}.npz')
    g = build_game(case)
    P = build_problem(*g.solver_args())
    assert_same_parameters(kat, P)
    for k in kat.files:
        if k.startswith('acc_'):
            assert kat[k] <= 1e-18, (k, float(kat[k]))
    assert kat['margin'] > 1e-3
    return kat, g, P


def host_fd(model, joint_config, q, u):
    """One step of the numpy mirror ``model.fd`` under the JOINT model's discretisation (dynamics_models.py:2482-2530: the joint config
    fixes method, dt and sub-steps for every agent)."""
    m = type(model)(0, dataclasses.replace(model.model_config, dt=joint_config.dt, discretization_method=joint_config.discretization_method,
                                           M=joint_config.M if joint_config.discretization_method != 'euler' else 1), track=model.track)
    return m.fd(q, u)
