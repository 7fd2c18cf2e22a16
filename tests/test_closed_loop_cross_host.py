"""A plant of another model class, the host side (no GPU): the three C-ABI entries are declared, exported by both builds and bound;
``project_state`` / ``lift_state`` round-trip on every pair of the table; ``PlantModel(own_class=True)``, ``Drivers('track')`` and
``step_batch`` refuse what the library would refuse before they reach it; ``track_reference`` is the numpy model's ``fd``; the TRACK
driver through ``drive`` on hand-made arrays, clamp paths included; without ``own_class`` today's refusal is unchanged."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ('dgsqp_set_cross_plant', 'dgsqp_fetch_plant_state', 'dgsqp_fetch_track_ref')
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 0), (3, 1)]
NQ = {0: 6, 1: 8, 2: 4, 3: 6}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def dyn_config():
    from dgsqp_amd.dynamics import DynamicBicycleConfig
    return DynamicBicycleConfig(dt=0.1, discretization_method='rk4', tire_model='pacejka', mass=2.2187, yaw_inertia=0.02723, M=4)


def kin_config():
    from dgsqp_amd.dynamics import KinematicBicycleConfig
    return KinematicBicycleConfig(dt=0.1, discretization_method='rk4', code_gen=False)


def test_the_symbols_are_declared_exported_and_bound():
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc.build import OUT, OUT_B256, build
    build()
    header = (ROOT / 'include' / 'dgsqp.h').read_text()
    declared = set(re.findall(r'\b(dgsqp_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared, name
        assert name in _ffi.SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        for so in (OUT, OUT_B256):
            assert hasattr(ctypes.CDLL(str(so)), name), (so.name, name)
    for wg in (1, 2):
        lib = _ffi.load_library(wg)
        assert lib.dgsqp_set_cross_plant.argtypes[1] == ctypes.POINTER(_ffi.PlantT) and len(lib.dgsqp_set_cross_plant.argtypes) == 4
        assert len(lib.dgsqp_fetch_plant_state.argtypes) == 3 and len(lib.dgsqp_fetch_track_ref.argtypes) == 3
    assert re.search(r'DGSQP_DRIVER_TRACK\s*=\s*3\b', header) and _ffi.DRIVER_TRACK == 3
    from dgsqp_amd.closed_loop import DRIVER_KINDS
    assert DRIVER_KINDS['track'] == 3


@pytest.mark.parametrize('pair', PAIRS)
def test_project_and_lift_round_trip(pair):
    from dgsqp_amd.closed_loop import cross_projection, lift_state, project_state
    g, p = pair
    idx = cross_projection(g, p)
    assert idx == ((0, 1, 2, 5, 6, 7) if (NQ[g], NQ[p]) == (6, 8) else tuple(range(NQ[g])))
    rng = np.random.default_rng(3)
    # two agents of the pair, and the pair next to an identity agent: offsets of both layouts are exercised
    for gc, pc in (([g, g], [p, p]), ([0, g], [0, p])):
        nq, nz = sum(NQ[c] for c in gc), sum(NQ[c] for c in pc)
        x = rng.standard_normal((3, 2, nq))
        x[0, 0, 0] = -0.0
        z = lift_state(gc, pc, x)
        assert z.shape == (3, 2, nz) and np.array_equal(bits(project_state(gc, pc, z)), bits(x))
        assert np.count_nonzero(z) == np.count_nonzero(x)                    # vy = w = 0
        z2 = rng.standard_normal((4, nz))
        q = project_state(gc, pc, z2)
        back = lift_state(gc, pc, q)
        keep = np.array_equal(bits(back), bits(z2)) if nq == nz else True
        assert q.shape == (4, nq) and keep
        if NQ[pc[1]] == 8 and NQ[gc[1]] == 6:
            off = NQ[pc[0]]
            assert np.array_equal(bits(q[:, NQ[gc[0]]:]), bits(z2[:, [off + i for i in (0, 1, 2, 5, 6, 7)]]))
            assert (back[:, off + 3] == 0).all() and (back[:, off + 4] == 0).all()
    with pytest.raises(ValueError, match='entries per chain'):
        project_state([g], [p], np.zeros(NQ[p] + 1))
    with pytest.raises(ValueError, match='entries per chain'):
        lift_state([g], [p], np.zeros(NQ[g] + 1))


@pytest.mark.parametrize('pair', [(g, p) for g in range(4) for p in range(4) if (g, p) not in PAIRS] + [(0, 4), (-1, 0)])
def test_every_other_pair_is_refused(pair):
    from dgsqp_amd.closed_loop import cross_projection
    with pytest.raises(ValueError, match='not a supported pair'):
        cross_projection(*pair)


def test_plant_model_own_class_lowering_and_refusals(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel
    Pk, Pd, Pm = games['kb_curve_N10'][1], games['dyn_curve_N15'][1], games['merge_N8'][1]
    # without own_class: today's text, word for word
    with pytest.raises(ValueError) as e:
        PlantModel(dynamics_configs=[dyn_config(), dyn_config()]).lower(Pk)
    assert str(e.value) == ("plant config 0 is of model class 1, the game's agent is of class 0: a plant keeps the game's model class and state layout")
    with pytest.raises(ValueError, match="a plant keeps the game's model class and state layout"):
        PlantModel(per_chain_configs=[[dyn_config(), dyn_config()]]).lower_ensemble(Pk, 1)
    # with it: 0 -> 1 lowers, the record carries the plant's class
    plant = PlantModel(dynamics_configs=[dyn_config(), kin_config()], own_class=True, sim_steps=2, method='rk4', M=3)
    pt = plant.lower(Pk)
    assert isinstance(pt, _ffi.PlantT) and (pt.agents[0].model, pt.agents[1].model, pt.use_game_agents, pt.sim_steps) == (1, 0, 0, 2)
    assert pt.agents[0].pac_Cf == 2.28 and plant.plant_classes(Pk) == [1, 0]
    assert PlantModel(own_class=True).plant_classes(Pk) == [0, 0] and PlantModel(own_class=True).lower(Pk).use_game_agents == 1
    # an unsupported pair: a kinematic plant under a dynamic game, a bicycle under the merge game's unicycle
    with pytest.raises(ValueError, match='not a supported pair'):
        PlantModel(dynamics_configs=[kin_config(), kin_config()], own_class=True).lower(Pd)
    with pytest.raises(ValueError, match='not a supported pair'):
        PlantModel(dynamics_configs=[dyn_config()] * 3, own_class=True).lower(Pm)
    # per-chain vehicles are compared with the PLANT's class
    veh, _ = PlantModel(dynamics_configs=[dyn_config(), kin_config()], per_chain_configs=[[dyn_config(), kin_config()]] * 2, own_class=True).lower_ensemble(Pk, 2)
    assert [veh[i].model for i in range(4)] == [1, 0, 1, 0]
    with pytest.raises(ValueError, match="the plant's agent is of class 1"):
        PlantModel(dynamics_configs=[dyn_config(), kin_config()], per_chain_configs=[[kin_config(), kin_config()]], own_class=True).lower_ensemble(Pk, 1)


def test_drivers_track_lowering_and_refusals(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import Drivers
    from dgsqp_amd.montecarlo import point_mass_racing_game
    from dgsqp_amd.solver import build_problem
    Pk, Pm = games['kb_curve_N10'][1], games['merge_N8'][1]
    Pp = build_problem(*point_mass_racing_game('curve', N=10).solver_args())
    d, per_chain, ref, rep = Drivers(kinds=['track', 'game']).lower(Pk, 3, 2, plant_classes=[1, 0])
    assert (d.kind[0], d.kind[1]) == (_ffi.DRIVER_TRACK, _ffi.DRIVER_GAME) and per_chain is None and ref is None and rep is None
    assert Drivers(kinds=[3, 0]).lower(Pk, 3, 2, plant_classes=[0, 0])[0].kind[0] == 3
    with pytest.raises(ValueError, match='own_class'):
        Drivers(kinds=['track', 'game']).lower(Pk, 3, 2)                      # no cross plant
    with pytest.raises(ValueError, match='own_class'):
        Drivers(per_chain_kinds=[['game', 'track']]).lower(Pk, 1, 2)
    with pytest.raises(ValueError, match='unicycle'):
        Drivers(kinds=['track', 'game', 'game']).lower(Pm, 3, 2, plant_classes=[2, 2, 2])
    with pytest.raises(ValueError, match='not recognized'):
        Drivers(kinds=['tracker', 'game']).lower(Pk, 3, 2, plant_classes=[1, 0])
    with pytest.raises(ValueError, match='not recognized'):
        Drivers(kinds=[4, 0]).lower(Pk, 3, 2, plant_classes=[1, 0])
    # GAME needs inputs of the same meaning: a point mass on a bicycle plant is refused, by name
    with pytest.raises(ValueError, match='agent 0 is a point mass'):
        Drivers().lower(Pp, 3, 2, plant_classes=[1, 1])
    with pytest.raises(ValueError, match='agent 1 is a point mass'):
        Drivers(kinds=['track', 'game']).lower(Pp, 3, 2, plant_classes=[0, 0])
    with pytest.raises(ValueError, match='agent 1 is a point mass'):
        Drivers(kinds=['track', 'track'], per_chain_kinds=[['track', 'pid'], ['track', 'game']]).lower(Pp, 2, 2, plant_classes=[0, 1])
    Drivers(kinds=['track', 'pid']).lower(Pp, 3, 2, plant_classes=[1, 0])
    Drivers().lower(Pp, 3, 2, plant_classes=[3, 3])                           # the identity pair keeps GAME
    Drivers().lower(Pk, 3, 2, plant_classes=[1, 1])                           # and so does 0 -> 1


def host_solver(P, n_q, N):
    from dgsqp_amd import solver
    s = solver.DGSQP.__new__(solver.DGSQP)
    s.N, s.n_q, s.num_ua_d, s.M, s.n_u, s.n = N, n_q, [2, 2], 2, 4, N * 4
    s._lib, s._h, s._problem = None, None, P                                  # no handle, no library: anything beyond the checks would raise otherwise
    return s


def test_step_batch_refuses_before_the_library(games):
    from dgsqp_amd.closed_loop import PlantModel, lift_state
    P = games['kb_curve_N10'][1]
    s = host_solver(P, 12, 10)
    x0, u_ws = np.arange(24.0).reshape(2, 12), np.zeros((2, 10, 4))
    cross = PlantModel(dynamics_configs=[dyn_config(), dyn_config()], own_class=True)
    from dgsqp_amd.dynamics import UnicycleConfig
    with pytest.raises(ValueError, match='not a supported pair'):               # a unicycle under a kinematic bicycle's game
        s.step_batch(x0, u_ws, 2, plant=PlantModel(dynamics_configs=[dyn_config(), UnicycleConfig(dt=0.1)], own_class=True))
    with pytest.raises(ValueError, match='disturbance'):
        s.step_batch(x0, u_ws, 2, plant=cross, disturbance=np.zeros((2, 2, 12)))
    with pytest.raises(ValueError, match=r'z0 must be \[B, n_z\] = \(2, 16\)'):
        s.step_batch(x0, u_ws, 2, plant=cross, z0=np.zeros((2, 14)))
    with pytest.raises(ValueError, match=r'z0 must be \[B, n_z\] = \(2, 16\)'):
        s.step_batch(x0, u_ws, 2, plant=cross, z0=np.zeros((3, 16)))
    z0 = lift_state([0, 0], [1, 1], x0)
    z0[1, 8 + 5] = np.nextafter(z0[1, 8 + 5], np.inf)                          # e_psi of car 2, chain 1: one ulp off
    with pytest.raises(ValueError, match='projection of z0'):
        s.step_batch(x0, u_ws, 2, plant=cross, z0=z0)
    with pytest.raises(ValueError, match='own_class'):
        s.step_batch(x0, u_ws, 2, plant=PlantModel(), z0=np.zeros((2, 12)))
    with pytest.raises(ValueError, match='own_class'):
        s.step_batch(x0, u_ws, 2, z0=np.zeros((2, 12)))
    # what passes every check reaches the library (there is none here)
    z0 = lift_state([0, 0], [1, 1], x0)
    z0[:, 3] = 0.25                                                            # vy is the plant's own: x0 is still p(z0)
    with pytest.raises(AttributeError):
        s.step_batch(x0, u_ws, 2, plant=cross, z0=z0)


def test_track_reference_is_the_numpy_models_fd():
    from dgsqp_amd.closed_loop import track_reference
    from dgsqp_amd.montecarlo import kinematic_racing_game, point_mass_racing_game
    from dgsqp_amd.dynamics import CasadiKinematicUnicycle
    g = point_mass_racing_game('curve', N=10)
    m = g.joint_model.dynamics_models[0]
    q, u = np.array([0.3, -0.1, 1.2, 0.05, 0.31, -0.2]), np.array([0.7, -0.3])
    assert np.array_equal(bits(track_reference(m, q, u)), bits(m.fd(q, u)))
    jc = g.joint_model.model_config
    assert np.array_equal(bits(track_reference(m, q, u, method=jc.discretization_method, dt=jc.dt, M=jc.M)), bits(m.fd(q, u)))
    # euler by hand, and the joint model's discretisation in place of the model's own
    assert np.allclose(track_reference(m, q, u), q + 0.1 * m.fc(q, u), rtol=0, atol=1e-15)
    k = kinematic_racing_game('curve', N=10).joint_model.dynamics_models[1]
    two = track_reference(k, q, u, method='rk2', dt=0.1, M=2)
    x = q.copy()
    for _ in range(2):
        a1 = k.fc(x, u); a2 = k.fc(x + 0.05 * a1, u)
        x = x + 0.05 * (a1 + a2) / 2
    assert np.array_equal(bits(two), bits(x)) and not np.array_equal(bits(two), bits(CasadiKinematicUnicycle.fd(k, q, u)))
    assert k.dt == 0.1 and k.model_config.discretization_method != 'rk2'      # the model itself is not changed


def test_track_driver_through_drive_with_its_clamps():
    from dgsqp_amd.closed_loop import PidGains, drive, new_pid_state, next_u_prev, pid_driver_step
    gains = [PidGains(kp_v=2.0, kp_s=1.5, ki_s=0.1, ey_gain=4.0, ei_max=0.02, u_max=(1.0, 0.4), du_max=(0.5, 0.3)), PidGains()]
    z = np.concatenate([[1.0, 2.0, 1.5, 0.1, -0.2, 0.07, 3.0, -0.15], [0.5, 0.4, 1.1, 0.02, 2.5, 0.1]])      # an 8- and a 6-state block
    zoff = [0, 8, 14]
    u_game = np.array([0.3, -0.1, 0.2, 0.05])
    refs = np.zeros((2, 2))
    # (a) nothing saturates: the law by hand, with e_psi - epsi_ref
    tr = np.array([[1.45, -0.14, 0.06], [np.nan] * 3])
    u, st = drive(['track', 'game'], u_game, z, gains, refs, new_pid_state((2,)), 0.1, zoff, track_refs=tr)
    e = 4.0 * (-0.15 - -0.14) + (0.07 - 0.06)
    ei = e * 0.1
    assert np.array_equal(bits(u[2:]), bits(u_game[2:])) and np.array_equal(bits(st[1]), bits(np.zeros(3)))
    assert np.array_equal(bits(u[:2]), bits([-(2.0 * (1.5 - 1.45)), -(1.5 * e + 0.1 * ei)])) and np.array_equal(bits(st[0]), bits([ei, u[0], u[1]]))
    # it is pid_driver_step with the references and the heading error passed in
    w, _ = pid_driver_step(gains[0], z[:8], tr[0, :2], np.zeros(3), 0.1, epsi_ref=tr[0, 2])
    assert np.array_equal(bits(w), bits(u[:2]))
    same_ref, _ = pid_driver_step(gains[0], z[:8], tr[0, :2], np.zeros(3), 0.1)
    assert not np.array_equal(bits(same_ref), bits(w))                         # (e_psi alone is another command)
    # (b) the rate clamp, against the previous command; (c) the magnitude clamp; (d) the integrator clamp
    far = np.array([[0.2, 0.5, -0.5], [np.nan] * 3])
    u, st = drive([3, 0], u_game, z, gains, refs, new_pid_state((2,)), 0.1, zoff, track_refs=far)
    assert np.array_equal(bits(u[:2]), bits([-0.5, 0.3])) and st[0, 0] == -0.02                # both rate-limited from 0; ei clamped at -ei_max
    prev = np.array([[0.0, -0.9, 0.35], [0.0, 0.0, 0.0]])
    u, st = drive([3, 0], u_game, z, gains, refs, prev, 0.1, zoff, track_refs=far)
    assert np.array_equal(bits(u[:2]), bits([-1.0, 0.4]))                                        # -0.9 - 0.5 and 0.35 + 0.3 hit u_max
    assert np.array_equal(bits(prev), bits([[0.0, -0.9, 0.35], [0.0, 0.0, 0.0]]))               # the caller's state is not changed
    # a 6-state plant block: e_psi at 3, e_y last
    tr6 = np.array([[np.nan] * 3, [1.0, 0.08, 0.01]])
    u, _ = drive(['game', 'track'], u_game, z, [gains[1], PidGains(ki_s=0.0)], refs, new_pid_state((2,)), 0.1, zoff, track_refs=tr6)
    assert np.array_equal(bits(u[2:]), bits([-(1.0 * (1.1 - 1.0)), -(1.0 * (5.0 * (0.1 - 0.08) + (0.02 - 0.01)) + 0.0 * 0.0)]))
    with pytest.raises(ValueError, match='track_refs'):
        drive(['track', 'game'], u_game, z, gains, refs, new_pid_state((2,)), 0.1, zoff)
    # the carry: a TRACK agent's u_prev is the game's command, every other kind's its own
    u_cmd = np.array([9.0, 8.0, 7.0, 6.0])
    assert np.array_equal(bits(next_u_prev(u_game, u_cmd, kinds=['track', 'pid'])), bits([0.3, -0.1, 7.0, 6.0]))
    assert np.array_equal(bits(next_u_prev(u_game, u_cmd)), bits(u_cmd))
