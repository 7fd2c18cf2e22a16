"""The raceline front end on a spline track (the F1 study's: comparison_study_f1/monte_carlo_sampler.py, warm_start.py) on the device:
the reference trajectories on a spline-track handle, dg_raceline_place_spline_kernel against ``sampler.place_raceline``, the sampler against
its mirror, the staged path and the refusals.  Dynamic F1 game, N = 10, the TUM line of tests/golden/f1_traj_race_cl.csv.gz.

Setting: the study's own, time_scale 1 and the [60, 80] m window (``s_range=(60, 80)``).  profiles/f1_raceline_acceptance.txt: of the first
1,024 candidates of seed 1 that setting accepts 723 (224 placements overlap, 77 warm starts fail); the other five settings measured accept
408 .. 745."""
import ctypes as C

import numpy as np
import pytest

import track_frame_checks as tf

pytestmark = pytest.mark.gpu

SEED = 1


@pytest.fixture(scope='module')
def f1dyn():
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=10, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=tf.f1_raceline(), s_range=(60, 80))
    s = DGSQP(*g.solver_args(), print_method=None)
    s.set_raceline(g.raceline)
    return g, s, mc.raceline_ws(g)


def states_on_line(g, B=16):
    """Both cars on the line up to small offsets, car 2 0.4 m ahead: s0 within 0.05 of the start line on both sides, in the second lap's
    first metres, the rest spread over the lap."""
    L = g.track.track_length
    rng = np.random.default_rng(2)
    s = np.concatenate(([0.03, -0.02, 0.0, L - 0.04, L + 0.01, 0.6 * L, 0.75 * L, 0.97 * L], rng.uniform(0.0, L, B - 8)))
    d_ey, d_v = rng.uniform(-0.05, 0.05, B), rng.uniform(-0.4, 0.4, B)
    out = []
    for a, mdl in enumerate(g.joint_model.dynamics_models):
        sa = s + 0.4 * a
        r = g.raceline.eval(g.raceline.s2t(sa))
        q = np.zeros((B, mdl.n_q))
        q[:, 2], q[:, mdl.epsi_idx], q[:, mdl.s_idx], q[:, mdl.ey_idx] = r[:, 3] + d_v, r[:, 6], sa, r[:, 8] + d_ey
        out.append(q)
    return np.concatenate(out, axis=1)


def test_reference_trajectories_on_a_spline_handle(f1dyn):
    """dg_raceline_ref_kernel reads the table and the states only: q_ref through dgsqp_fetch_raceline_ref against Raceline.q_ref on 16
    states, 0 ulp (the mirror runs the same operations, every one rounded once)."""
    g, s, W = f1dyn
    x0 = states_on_line(g)
    out = s.raceline_warm_start_batch(x0, W)
    assert out['u_ws'].shape == (16, 10, 4) and out['ok'].shape == (16,)
    ref = s.fetch_raceline_ref(16)
    for a in range(2):
        want = g.raceline.q_ref(x0[:, 8 * a:8 * (a + 1)], g.params.N, g.params.dt)
        assert np.array_equal(tf.bits(ref[:, a]), tf.bits(want)), np.abs(ref[:, a] - want).max()


def mirror_round(g, s, W, n):
    """The mirror's placement of candidates 0 .. n - 1, its collision margins, and the program's verdict on every one of them."""
    from dgsqp_amd import sampler as smp
    x0, margin = smp.place_raceline(g, SEED, np.arange(n))
    return x0, margin, s.raceline_warm_start_batch(x0, W)['ok']


def test_placement_against_the_mirror(f1dyn):
    """B = 64: one round of 256 candidates.  Every accepted row is found among the mirror's placements by the bits of car 1's arclength, in
    candidate order; s, e_y, e_psi and v carry the mirror's bits, x, y to 1e-12; and the candidates the device passed over are exactly
    those the mirror rejects (the cars overlap, or a warm start fails) -- under the precondition that no collision margin is within 1e-9
    of zero."""
    g, s, W = f1dyn
    dev = s.sample_raceline_batch(g, 64, seed=SEED, ws=W)
    x0, margin, ok = mirror_round(g, s, W, 256)
    assert np.abs(margin).min() > 1e-9
    where = {int(b): i for i, b in enumerate(tf.bits(x0[:, 6]))}
    idx = np.array([where[int(b)] for b in tf.bits(dev['x0'][:, 6])])
    used = dev['candidates']
    assert (np.diff(idx) > 0).all() and idx[-1] + 1 == used and used <= 256
    accepted = np.nonzero((margin[:used] < 0) & ok[:used])[0]
    print(f'{used} candidates for 64 scenarios: {int((margin[:used] >= 0).sum())} overlap, {int(((margin[:used] < 0) & ~ok[:used]).sum())} warm starts fail')
    assert np.array_equal(idx, accepted)
    drawn, xy = [2, 5, 6, 7, 10, 13, 14, 15], [0, 1, 8, 9]
    assert np.array_equal(tf.bits(dev['x0'][:, drawn]), tf.bits(x0[idx][:, drawn]))
    d = np.abs(dev['x0'][:, xy] - x0[idx][:, xy]).max()
    print(f'|dx|, |dy| <= {d:.2e}')
    assert d <= 1e-12
    gap = dev['x0'][:, 14] - dev['x0'][:, 6]
    assert (gap >= 0).all() and (gap <= 3 * 0.56).all() and (dev['x0'][:, 6] >= 60).all() and (dev['x0'][:, 6] <= 80).all()
    dd = dev['x0'][:, :2] - dev['x0'][:, 8:10]
    assert ((dd * dd).sum(axis=1) > g.collision_d ** 2).all()


def test_sampler_against_its_mirror(f1dyn):
    """sample_raceline_batch(game, 8, seed) against sampler.sample_raceline_counter (placement and collision check in numpy, the program per
    round through the same tracker kernel): the same candidates, x0 and u_ws bit for bit.  Condition, asserted first: at least 8 of the
    first 1,024 candidates are accepted (measured: 723)."""
    from dgsqp_amd import sampler as smp
    g, s, W = f1dyn
    _, margin, ok = mirror_round(g, s, W, 1024)
    n_acc = int(((margin < 0) & ok).sum())
    print(f'accepted {n_acc} of the first 1024 candidates')
    assert n_acc >= 8
    dev = s.sample_raceline_batch(g, 8, seed=SEED, ws=W)
    x0, u_ws, used, closest = smp.sample_raceline_counter(g, s, 8, SEED, ws=W)
    assert closest > 1e-9
    assert dev['candidates'] == used
    assert np.array_equal(tf.bits(dev['x0']), tf.bits(x0)) and np.array_equal(tf.bits(dev['u_ws']), tf.bits(u_ws))


def test_staged_path_and_the_whole_lap():
    """stage=True + dgsqp_solve_staged against solve_batch of the fetched batch, bit for bit (B = 16); here without s_range: car 1
    anywhere in [0, L - 10]."""
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=10, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=tf.f1_raceline())
    s = DGSQP(*g.solver_args(), print_method=None)
    B = 16
    dev = s.sample_raceline_batch(g, B, seed=5)
    assert (dev['x0'][:, 6] >= 0).all() and (dev['x0'][:, 6] <= g.track.track_length - 10).all() and np.ptp(dev['x0'][:, 6]) > 100
    ref = s.solve_batch(dev['x0'], dev['u_ws'])
    s.sample_raceline_batch(g, B, seed=5, stage=True, fetch=False)
    tm = _ffi.TimingT()
    assert s._lib.dgsqp_solve_staged(s._h, C.byref(tm)) == 0, s._lib.dgsqp_last_error(s._h)
    st, it, qp = (np.empty(B, np.int32) for _ in range(3))
    u = np.empty((B, s.n))
    assert s._lib.dgsqp_fetch_results(s._h, _ffi.dptr(u), None, None, _ffi.iptr(st), _ffi.iptr(it), _ffi.iptr(qp), None, None) == 0
    assert np.array_equal(st, ref['status']) and np.array_equal(it, ref['num_iters']) and np.array_equal(qp, ref['qp_solves'])
    assert np.array_equal(u, ref['u'], equal_nan=True)


def test_refusals_and_the_256_thread_build(f1dyn):
    from dgsqp_amd import _ffi, montecarlo as mc, sampler as smp
    from dgsqp_amd.solver import DGSQP
    import raceline_checks as rc
    g, s, W = f1dyn
    lib = s._lib
    spec = smp.raceline_spline_sampler_spec(g, SEED)

    def refused(handle, sp, B=4, word=''):
        assert lib.dgsqp_sample_raceline_spline_batch(handle._h, B, C.byref(sp) if sp is not None else None, C.byref(W), None, None, None, 0) == _ffi.E_ARG
        msg = lib.dgsqp_last_error(handle._h).decode()
        assert msg.startswith('raceline: ') and word in msg, msg
    refused(s, spec, B=-1)
    refused(s, None)
    for field, value in (('s_hi', 10.0), ('gap_hi', -1.0), ('ey_clip', -0.1), ('collision_d', np.nan), ('s_lo', np.inf)):
        bad = smp.raceline_spline_sampler_spec(g, SEED)
        setattr(bad, field, value)
        refused(s, bad, word='bad sampler description')
    arc_game = rc.dynamic_game(N=4, rk4_substeps=2)
    arc = DGSQP(*arc_game.solver_args(), print_method=None)
    arc.set_raceline(arc_game.raceline)
    refused(arc, spec, word='arc-track handle')
    s.set_raceline(None)
    refused(s, spec, word='no raceline set')
    s.set_raceline(g.raceline)
    assert lib.dgsqp_sample_raceline_spline_batch(s._h, 0, C.byref(spec), C.byref(W), None, None, None, 0) == 0
    ref = s.sample_raceline_batch(g, 8, seed=SEED, ws=W)          # the handle is fine after every refusal
    b = DGSQP(*g.solver_args(), print_method=None, workgroups_per_cu=2)
    out = b.sample_raceline_batch(g, 8, seed=SEED, ws=W)
    assert ref['x0'].shape == (8, 16) and out['x0'].shape == (8, 16) and out['u_ws'].shape == (8, 10, 4) and out['candidates'] >= 8


@pytest.mark.parametrize('front_end', ['raceline', 'circuit'])
def test_example_driver(tmp_path, monkeypatch, front_end):
    """examples/monte_carlo_f1.py: one sample_<i>.pkl per scenario with the keys the study's analysis reads, and the records are those of a
    plain solve_batch of the same sampled batch."""
    import pickle
    import sys
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    monkeypatch.syspath_prepend(str(tf.ROOT / 'examples'))
    sys.modules.pop('monte_carlo_f1', None)
    import monte_carlo_f1 as ex
    out = tmp_path / 'out'
    argv = ['--num-mc', '8', '--N', '6', '--rk4-substeps', '2', '--front-end', front_end, '--seed', '3', '--out', str(out)]
    if front_end == 'raceline':
        argv += ['--s-range', '60', '80']
    samples = ex.main(argv)
    files = sorted(out.glob('sample_*.pkl'), key=lambda p: int(p.stem.split('_')[1]))
    assert [p.name for p in files] == [f'sample_{i + 1}.pkl' for i in range(8)]
    d = pickle.load(open(files[4], 'rb'))
    assert set(d) == {'solver_result', 'initial_condition'} and {'msg', 'time', 'num_iters', 'status'} <= set(d['solver_result'])
    assert len(d['initial_condition']) == 2 and hasattr(d['initial_condition'][0].x, 'x')
    if front_end == 'raceline':
        g = mc.f1_racing_game(N=6, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=tf.f1_raceline(), s_range=(60, 80))
    else:
        g = mc.f1_racing_game(N=6, rk4_substeps=2)
    s = DGSQP(*g.solver_args(), print_method=None)
    batch = s.sample_raceline_batch(g, 8, seed=3) if front_end == 'raceline' else s.sample_batch(g, 8, seed=3)
    ref = s.solve_batch(batch['x0'], batch['u_ws'])
    assert [r['solver_result']['num_iters'] for r in samples] == list(ref['num_iters'])
    assert [r['solver_result']['msg'] for r in samples] == list(ref['msg'])
    s_col = g.joint_model.dynamics_models[0].n_q + g.joint_model.dynamics_models[1].s_idx
    assert abs(samples[4]['initial_condition'][1].p.s - batch['x0'][4, s_col]) < 1e-15
    if front_end == 'raceline':          # --host-sampler: sequential draws by the study's law, warm starts through the same program
        host = ex.main(['--num-mc', '8', '--N', '6', '--rk4-substeps', '2', '--front-end', 'raceline', '--seed', '0', '--s-range', '60', '80', '--host-sampler'])
        x0, u_ws = mc.sample_scenarios(g, 8, seed=0, solver=s)
        ref = s.solve_batch(x0, u_ws)
        assert [r['solver_result']['num_iters'] for r in host] == list(ref['num_iters'])
        assert ((x0[:, 14] - x0[:, 6]) >= 0).all() and (x0[:, 6] >= 60).all() and (x0[:, 6] <= 80).all()
