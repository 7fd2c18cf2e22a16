"""The circuit sampler on a spline track (dgsqp_sample_batch with n_key = 0: dg_sample_place_spline_kernel, csrc/dgsqp_track_frame.h)
against its numpy mirror (dgsqp_amd/sampler.py) on the F1 game, and the staged path."""
import ctypes as C

import numpy as np
import pytest

import track_frame_checks as tf

pytestmark = pytest.mark.gpu

SEED = 3


@pytest.fixture(scope='module')
def f1():
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=5)
    return g, DGSQP(*g.solver_args(), print_method=None)


def frenet_columns(g):
    """Columns of the joint state that the placement draws itself (v, e_psi, s, e_y of every car) and the ones it computes (x, y)."""
    drawn, xy, off = [], [], 0
    for m in g.joint_model.dynamics_models:
        drawn += [off + 2, off + m.epsi_idx, off + m.s_idx, off + m.ey_idx]
        xy += [off, off + 1]
        off += m.n_q
    return drawn, xy


def test_placement_of_the_first_round(f1):
    """B = 64: one round of 256 candidates (0 .. 255).  Every accepted row is found among the mirror's placements by the bits of car 1's
    arclength, in candidate order; s, e_y, v, e_psi carry the mirror's bits; x, y to 1e-12 (coordinates below 2^7 m, a handful of roundings
    of at most 2^-46 m each; the mirror runs the same operations, so the figure printed is usually 0)."""
    from dgsqp_amd import sampler as smp
    g, s = f1
    dev = s.sample_batch(g, 64, seed=SEED)
    assert dev['candidates'] <= 256
    q0, ok = smp.place(g, SEED, np.arange(256))
    host = np.concatenate(q0, axis=1)
    assert ok.all()
    drawn, xy = frenet_columns(g)
    s1 = g.joint_model.dynamics_models[0].s_idx
    where = {int(b): i for i, b in enumerate(tf.bits(host[:, s1]))}
    idx = np.array([where[int(b)] for b in tf.bits(dev['x0'][:, s1])])
    assert (np.diff(idx) > 0).all() and idx[-1] + 1 == dev['candidates']
    assert np.array_equal(tf.bits(dev['x0'][:, drawn]), tf.bits(host[idx][:, drawn]))
    d = np.abs(dev['x0'][:, xy] - host[idx][:, xy]).max()
    print(f'placement: {len(idx)} accepted of the first {dev["candidates"]} candidates, |dx|, |dy| <= {d:.2e}')
    assert d <= 1e-12
    L = g.track.track_length
    assert (host[:, s1] >= 0).all() and (host[:, s1] < L).all() and (np.abs(host[:, drawn[3]]) <= g.half_width).all()


def test_sample_batch_against_the_counter_mirror(f1):
    """DGSQP.sample_batch(game, 64, seed=3) against sampler.sample_scenarios_counter: the same candidates consumed, x0 at the bars of the
    placement test, u_ws to 1e-9 (the bar of test_device_sampler_matches_its_host_mirror).  Precondition, asserted first: among the
    consumed candidates the smallest |collision margin| along the warm start exceeds 1e-9, so that no decision can flip on rounding."""
    from dgsqp_amd import montecarlo as mc, sampler as smp
    g, s = f1
    x0, u_ws, used = smp.sample_scenarios_counter(g, 64, seed=SEED, chunk=256)
    q0, _ = smp.place(g, SEED, np.arange(used))
    models = g.joint_model.dynamics_models
    traj = [mc.pid_warm_start(m, q, g.params.N, g.params.dt, du=tuple(g.agent_constraints[0].rate_max))[0] for m, q in zip(models, q0)]
    r = g.shared_constraints.radii
    margin = np.linalg.norm(traj[0][:, :, :2] - traj[1][:, :, :2], axis=2) - (r[0] + r[1])
    closest = np.abs(margin).min()
    print(f'{used} candidates consumed for 64 scenarios, smallest |collision margin| {closest:.3e}')
    assert closest > 1e-9
    dev = s.sample_batch(g, 64, seed=SEED)
    assert dev['candidates'] == used
    drawn, xy = frenet_columns(g)
    assert np.array_equal(tf.bits(dev['x0'][:, drawn]), tf.bits(x0[:, drawn]))
    d, du = np.abs(dev['x0'][:, xy] - x0[:, xy]).max(), np.abs(dev['u_ws'] - u_ws).max()
    print(f'|dx|, |dy| <= {d:.2e}, |du_ws| <= {du:.2e}')
    assert d <= 1e-12 and du < 1e-9


def test_more_than_one_round_and_three_cars():
    """B = 200 (rounds of 400 candidates) with three cars: the rounds continue the candidate count as on arc tracks."""
    from dgsqp_amd import montecarlo as mc, sampler as smp
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=5, M=3)
    s = DGSQP(*g.solver_args(), print_method=None)
    dev = s.sample_batch(g, 200, seed=SEED)
    x0, u_ws, used = smp.sample_scenarios_counter(g, 200, seed=SEED, chunk=400)
    print(f'three cars: {used} candidates for 200 scenarios')
    assert dev['candidates'] == used and used > 400
    assert np.abs(dev['x0'] - x0).max() <= 1e-12 and np.abs(dev['u_ws'] - u_ws).max() < 1e-9


def test_staged_path(f1):
    """stage=True, then dgsqp_solve_staged, equals solve_batch on the fetched batch bit for bit."""
    from dgsqp_amd import _ffi
    g, s = f1
    B = 64
    dev = s.sample_batch(g, B, seed=SEED)
    ref = s.solve_batch(dev['x0'], dev['u_ws'])
    s.sample_batch(g, B, seed=SEED, stage=True, fetch=False)
    tm = _ffi.TimingT()
    assert s._lib.dgsqp_solve_staged(s._h, C.byref(tm)) == 0, s._lib.dgsqp_last_error(s._h)
    st, it, qp = (np.empty(B, np.int32) for _ in range(3))
    u = np.empty((B, s.n))
    assert s._lib.dgsqp_fetch_results(s._h, _ffi.dptr(u), None, None, _ffi.iptr(st), _ffi.iptr(it), _ffi.iptr(qp), None, None) == 0
    assert np.array_equal(st, ref['status']) and np.array_equal(it, ref['num_iters']) and np.array_equal(qp, ref['qp_solves'])
    assert np.array_equal(u, ref['u'], equal_nan=True)
