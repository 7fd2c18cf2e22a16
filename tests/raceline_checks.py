"""Test infrastructure of the raceline warm starts (tests/test_raceline.py, tests/test_raceline_host.py): the fixture, the small games the
tests run on, and the HOST-LOOP composition of the warm-start program -- two tracker launches per car through the public
``CA_LTV_MPC.solve_batch`` with the chain of ``set_warm_start`` in numpy -- that the device program is held to bit for bit.  The product
never imports this."""
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
FIXTURE = ROOT / 'tests' / 'golden' / 'L_track_barc_raceline.npz'
TIME_SCALE = 1.7          # warm_start_dynamic.py:25


def raceline():
    from dgsqp_amd.montecarlo import Raceline
    return Raceline.from_file(FIXTURE, 'L_track_barc', TIME_SCALE)


def dynamic_game(N=4, rk4_substeps=2, solver='v1'):
    from dgsqp_amd.montecarlo import dynamic_racing_game
    return dynamic_racing_game(track_kind='barc', N=N, rk4_substeps=rk4_substeps, solver=solver, sampler='raceline', raceline=raceline())


def kinematic_game(N=3):
    """The kinematic circuit race with the raceline attached: the entry is not tied to the dynamic bicycle."""
    from dgsqp_amd.montecarlo import STUDY_COLLISION_D, barc_racing_game
    g = barc_racing_game(N=N, M=2)
    g.sampler, g.raceline, g.collision_d = 'raceline', raceline(), STUDY_COLLISION_D
    return g


def states_on_raceline(game, s, d_ey=0.0, d_v=0.0):
    """Joint states [B, n_q] with both cars at arclength s (car 2 0.4 behind), on the raceline up to the offsets."""
    rl = game.raceline
    models = game.joint_model.dynamics_models
    s = np.asarray(s, np.float64)
    out = []
    for a, mdl in enumerate(models):
        sa = s - 0.4 * a
        r = rl.eval(rl.s2t(sa))
        q = np.zeros((len(s), mdl.n_q))
        q[:, 2], q[:, mdl.epsi_idx], q[:, mdl.s_idx], q[:, mdl.ey_idx] = r[:, 3] + d_v, r[:, 6], sa, r[:, 8] + d_ey
        out.append(q)
    return np.concatenate(out, axis=1)


def lowered_tracker(game, tracker, device=0, workgroups_per_cu=1):
    """A ``CA_LTV_MPC`` whose record equals the program's: the study's cost and bounds with ``input_scaling`` already lowered by hand (rate
    weight w Tu^2, rate box / Tu) and no ``input_scaling`` left, so that its ``du_ws`` / ``du_pred`` are the device's own and the chain
    below feeds back exactly the bits the device chain does."""
    import copy
    from dgsqp_amd.ltv_mpc import CA_LTV_MPC, TrackingCost
    from dgsqp_amd.types import VehicleActuation, VehicleState
    p = copy.copy(tracker['params'])
    Tu = 1.0 / np.asarray(p.input_scaling, np.float64)
    p.input_scaling = None
    c = tracker['cost']
    cost = TrackingCost(state_weight=c.state_weight, input_weight=c.input_weight, rate_weight=tuple(float(w) * t * t for w, t in zip(c.rate_weight, Tu)))
    b = dict(tracker['bounds'])
    mdl = game.joint_model.dynamics_models[0]
    for key in ('du_ub', 'du_lb'):
        _, du = mdl.state2qu(b[key])
        b[key] = VehicleState(u=VehicleActuation(u_a=float(du[0]) / Tu[0], u_steer=float(du[1]) / Tu[1]))
    return CA_LTV_MPC(mdl, cost, None, b, p, print_method=None, device=device, workgroups_per_cu=workgroups_per_cu)


def host_loop(game, tracker, mpc, x0, q_ref):
    """warm_start_dynamic.py:156-165 for every car with two ``solve_batch`` calls: phase 1 (set_warm_start's loop: zero_du, init_iters,
    init_damping), the chain, phase 2.  q_ref [B, M, N + 1, n_qa].  Returns u_ws [B, N, n_u] time-major and ok [B]."""
    B, N = x0.shape[0], game.params.N
    models = game.joint_model.dynamics_models
    ok = np.ones(B, bool)
    us, off = [], 0
    for a, mdl in enumerate(models):
        q0 = np.ascontiguousarray(x0[:, off:off + mdl.n_q])
        off += mdl.n_q
        u_ws = np.full((B, N + 1, 2), tracker['u_init'])
        du_ws = np.full((B, N, 2), tracker['du_init'])
        qr = np.ascontiguousarray(q_ref[:, a])
        p1 = mpc.solve_batch(q0, u_ws, du_ws, qr, qp_iters=tracker['init_iters'], damping=tracker['init_damping'], zero_du=True)
        u_ws2 = np.concatenate((u_ws[:, :1], p1['u_pred']), axis=1)
        p2 = mpc.solve_batch(q0, u_ws2, p1['du_pred'], qr)
        ok &= p2['status'] == 0
        us.append(p2['u_pred'])
    return np.concatenate(us, axis=2), ok
