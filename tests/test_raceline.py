"""Raceline warm starts on the device (csrc/dgsqp_raceline.h): the look-ups and the reference trajectories against the numpy mirror, the
warm-start program against its host-loop composition bit for bit, the study's tracker parameters, the study's sampler against its mirror,
the staged path, the refusals, and the 256-thread build."""
import ctypes as C

import numpy as np
import pytest

import raceline_checks as rc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope='module')
def dyn4():
    """dynamic_racing_game(track_kind='barc', N=4, rk4_substeps=2) with the raceline set, its study tracker and the program's record."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = rc.dynamic_game(N=4, rk4_substeps=2)
    s = DGSQP(*g.solver_args(), print_method=None)
    s.set_raceline(g.raceline)
    return g, s, mc.study_tracker(g), mc.raceline_ws(g)


def edge_states(g, B=16):
    """s0 within 0.05 of the start line on both sides (car 2, 0.4 behind, is then at s < 0), s0 in the second half of the lap, the rest
    spread over the lap; lateral and speed offsets from the raceline (the raceline's |e_y| reaches 0.45 of the half width 0.55: the lateral
    offset stays below 0.05 so that every car starts inside the track)."""
    L = g.track.track_length
    rng = np.random.default_rng(2)
    s = np.concatenate(([0.03, -0.02, 0.0, L - 0.04, L + 0.01, 0.6 * L, 0.75 * L, 0.97 * L], rng.uniform(0.0, L, B - 8)))
    return rc.states_on_raceline(g, s, d_ey=rng.uniform(-0.05, 0.05, B), d_v=rng.uniform(-0.4, 0.4, B))


@pytest.mark.parametrize('kind', ['dynamic', 'kinematic'])
def test_device_lookups_and_reference_trajectories(dyn4, kind):
    """q_ref through dgsqp_fetch_raceline_ref against Raceline.q_ref: 1e-12 max(1, |value|) (t_k carries t0's rounding through slopes of
    order 10; the mirror runs the same operations, so the figure printed is usually 0)."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    if kind == 'dynamic':
        g, s, _, W = dyn4
    else:
        g = rc.kinematic_game(N=3)
        s = DGSQP(*g.solver_args(), print_method=None)
        s.set_raceline(g.raceline)
        W = mc.raceline_ws(g)
    x0 = edge_states(g)
    out = s.raceline_warm_start_batch(x0, W)
    assert out['u_ws'].shape == (16, g.params.N, 4) and out['ok'].shape == (16,)
    ref = s.fetch_raceline_ref(16)
    nqa = g.joint_model.dynamics_models[0].n_q
    worst = 0.0
    for a in range(2):
        want = g.raceline.q_ref(x0[:, a * nqa:(a + 1) * nqa], g.params.N, g.params.dt)
        err = np.abs(ref[:, a] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, float(err.max()))
    print(f'{kind}: q_ref device against mirror, worst relative difference {worst:.3e}')
    assert worst <= 1e-12


def test_program_equals_the_host_loop_bit_for_bit(dyn4):
    """Two CA_LTV_MPC.solve_batch calls per car with the chain on the host and q_ref from dgsqp_fetch_raceline_ref: the same kernel on the
    same inputs.  Scenario 2 starts at v_long = -1: its stage-1 box v_long >= 0.1 is out of reach with u_a <= 2 and dt = 0.1, so ok = 0; its
    neighbours are what a batch without it gives.  The handle's own tracker setting survives."""
    from dgsqp_amd import _ffi, ltv_mpc
    g, s, tracker, W = dyn4
    x0 = edge_states(g)[[0, 1, 5, 8, 9, 10]]
    x0[2, 2] = -1.0
    own = ltv_mpc.lower(1, 8, ltv_mpc.TrackingCost(state_weight=np.ones(8)), None, None, 1e10 * np.ones(8), -1e10 * np.ones(8), (1, 1), (-1, -1),
                        (3, 3), (-3, -3), 3, 3, 0.6)
    assert s._lib.dgsqp_set_mpc(s._h, C.byref(own)) == 0
    before = ltv_mpc.mpc_dims(s._lib, s._h)
    dev = s.raceline_warm_start_batch(x0, W)
    after = ltv_mpc.mpc_dims(s._lib, s._h)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    q_ref = s.fetch_raceline_ref(6)
    host_u, host_ok = rc.host_loop(g, tracker, rc.lowered_tracker(g, tracker), x0, q_ref)
    print('ok: device', dev['ok'].tolist(), 'host loop', host_ok.tolist())
    assert dev['ok'].tolist() == host_ok.tolist()
    assert dev['ok'].tolist() == [True, True, False, True, True, True]
    assert np.array_equal(bits(dev['u_ws']), bits(host_u))
    keep = [0, 1, 3, 4, 5]
    rest = s.raceline_warm_start_batch(x0[keep], W)
    assert rest['ok'].all() and np.array_equal(bits(rest['u_ws']), bits(dev['u_ws'][keep]))
    assert s._lib.dgsqp_set_mpc(s._h, None) == 0


def test_study_parameters_through_the_class_surface(dyn4):
    """input_scaling = [2, 0.45], state_scaling given, qp_iters = 5, N = 4 -- warm_start_dynamic.py's own CALTVMPCParams -- through
    CA_LTV_MPC.solve_batch: what the raw entry returns with the lowered record, du_ws / du_pred in the reference's scaled units."""
    from dgsqp_amd import ltv_mpc
    from dgsqp_amd.ltv_mpc import CA_LTV_MPC
    g, s, tracker, W = dyn4
    p = tracker['params']
    assert list(p.input_scaling) == [2, 0.45] and p.state_scaling is not None and p.qp_iters == 5 and p.N == 4
    mdl = g.joint_model.dynamics_models[0]
    mpc = CA_LTV_MPC(mdl, tracker['cost'], None, tracker['bounds'], p, print_method=None)
    x0 = edge_states(g)[:5]
    q0 = np.ascontiguousarray(x0[:, :8])
    q_ref = g.raceline.q_ref(q0, 4, 0.1)
    rng = np.random.default_rng(8)
    u_ws, du_ws = 0.05 * rng.standard_normal((5, 5, 2)), 0.2 * rng.standard_normal((5, 4, 2))
    got = mpc.solve_batch(q0, u_ws, du_ws, q_ref)
    Tu = 1.0 / np.asarray(p.input_scaling, np.float64)
    rec = W.mpc
    assert (rec.qp_iters, rec.N, rec.damping) == (5, 4, 0.75) and list(rec.w_du) == [0.1 * Tu[0] * Tu[0], 0.1 * Tu[1] * Tu[1]]
    raw = ltv_mpc.run_batch(mpc._solver._lib, mpc._solver._h, rec, 8, q0, u_ws, du_ws / Tu, q_ref)
    assert (raw['status'] == 0).all() and np.array_equal(got['status'], raw['status'])
    assert np.array_equal(bits(got['q_pred']), bits(raw['q_pred'])) and np.array_equal(bits(got['u_pred']), bits(raw['u_pred']))
    assert np.array_equal(bits(got['du_pred']), bits(raw['du_pred'] * Tu))


def tight_tracker(g):
    """The study's tracker with v_long >= 2 at every stage: more than half of the sampled cars cannot reach it, so the sampler needs more
    than one round (the study's own tracker accepts more than half of a round's 2 B candidates)."""
    from dgsqp_amd import montecarlo as mc
    t = mc.study_tracker(g)
    t['bounds']['qu_lb'].v.v_long = 2.0
    return t


@pytest.mark.parametrize('variant', ['study', 'tight'])
def test_sampler_against_its_mirror(dyn4, variant):
    """B = 300, seed 11: the same candidates accepted and the same count consumed as the numpy mirror (placement and collision check in
    numpy, the program per round through dgsqp_raceline_warm_start_batch); x0 to 1e-12; u_ws bit for bit what the program returns for the
    fetched x0.  Precondition: every candidate's collision margin in the mirror is above 1e-9 in magnitude.  'tight' is the same sampler
    with a tracker most cars fail, which makes it run more than one round."""
    from dgsqp_amd import montecarlo as mc, sampler as smp
    g, s, _, W = dyn4
    if variant == 'tight':
        W = mc.raceline_ws(g, tight_tracker(g))
    B, seed = 300, 11
    dev = s.sample_raceline_batch(g, B, seed=seed, ws=W)
    x0, u_ws, used, closest = smp.sample_raceline_counter(g, s, B, seed, ws=W)
    print(f'{variant}: candidates consumed {dev["candidates"]} (a round has {max(256, 2 * B)}), smallest |collision margin| {closest:.3e}')
    assert closest > 1e-9
    assert dev['candidates'] == used
    if variant == 'tight':
        assert used > max(256, 2 * B)
    assert dev['x0'].shape == x0.shape and np.abs(dev['x0'] - x0).max() <= 1e-12
    again = s.raceline_warm_start_batch(dev['x0'], W)
    assert again['ok'].all() and np.array_equal(bits(again['u_ws']), bits(dev['u_ws']))
    # every accepted warm start is inside the game's input boxes: the tracker's own boxes are inside them, and it accepts a row up to 1e-13
    # with one more rounding in the damped update (DG_MPC_UTOL = 1e-12 is the product's own figure for that)
    ub = np.tile([2.1, 0.436], 2)
    assert (np.abs(dev['u_ws']) <= ub * (1 + 1e-12)).all()
    d = dev['x0'][:, :2] - dev['x0'][:, 8:10]
    assert ((d * d).sum(axis=1) > g.collision_d ** 2).all()


def test_staged_path():
    """sample_raceline_batch(stage=True) + dgsqp_solve_staged against solve_batch from the fetched x0, u_ws: u, status, num_iters and
    qp_solves bit for bit (B = 32, N = 10); and the program on a staged batch (x0 = NULL) writes the staged warm start."""
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = rc.dynamic_game(N=10, rk4_substeps=2)
    s = DGSQP(*g.solver_args(), print_method=None)
    B = 32
    W = mc.raceline_ws(g)

    def staged_results():
        tm = _ffi.TimingT()
        assert s._lib.dgsqp_solve_staged(s._h, C.byref(tm)) == 0, s._lib.dgsqp_last_error(s._h)
        st, it, qp = (np.empty(B, np.int32) for _ in range(3))
        u = np.empty((B, s.n))
        assert s._lib.dgsqp_fetch_results(s._h, _ffi.dptr(u), None, None, _ffi.iptr(st), _ffi.iptr(it), _ffi.iptr(qp), None, None) == 0
        return u, st, it, qp
    dev = s.sample_raceline_batch(g, B, seed=5)
    ref = s.solve_batch(dev['x0'], dev['u_ws'])
    s.sample_raceline_batch(g, B, seed=5, stage=True, fetch=False)
    u, st, it, qp = staged_results()
    assert np.array_equal(st, ref['status']) and np.array_equal(it, ref['num_iters']) and np.array_equal(qp, ref['qp_solves'])
    assert np.array_equal(u, ref['u'], equal_nan=True)
    # x0 = NULL: the staged batch's own warm start is replaced by the program's
    x0 = np.ascontiguousarray(dev['x0'])
    assert s._lib.dgsqp_stage_inputs(s._h, B, _ffi.dptr(x0), _ffi.dptr(np.zeros((B, s.n)))) == 0
    out = s.raceline_warm_start_batch(None, W, B=B)
    assert out['ok'].all() and np.array_equal(bits(out['u_ws']), bits(dev['u_ws']))
    u2, st2, it2, qp2 = staged_results()
    assert np.array_equal(st2, st) and np.array_equal(it2, it) and np.array_equal(qp2, qp) and np.array_equal(u2, u, equal_nan=True)
    with pytest.raises(ValueError, match='raceline: .*staged'):
        s.raceline_warm_start_batch(None, W, B=B + 1)


def test_refusals(dyn4):
    from dgsqp_amd import _ffi, montecarlo as mc, sampler as smp
    from dgsqp_amd.solver import DGSQP
    g, s, _, W = dyn4
    x0 = edge_states(g)[:2]
    s.set_raceline(None)
    with pytest.raises(ValueError, match='raceline: no raceline set'):
        s.raceline_warm_start_batch(x0, W)
    spec = smp.raceline_sampler_spec(g, 1)
    assert s._lib.dgsqp_sample_raceline_batch(s._h, 4, C.byref(spec), C.byref(W), None, None, None, 0) == _ffi.E_ARG
    assert s._lib.dgsqp_last_error(s._h).startswith(b'raceline: no raceline set')
    for T, cols, word in ((np.arange(3.0), np.zeros((3, 9)), 'the s column is not strictly increasing'),(np.array([0.0]), np.zeros((1, 9)), 'knots'), (np.array([0.0, np.nan]), np.ones((2, 9)), 'not finite'),
                          (np.array([0.0, 0.0]), np.arange(18.0).reshape(2, 9), 'T is not strictly increasing')):
        with pytest.raises(ValueError, match='raceline: .*' + word):
            s.set_raceline((T, cols))
    s.set_raceline(g.raceline)
    assert s._lib.dgsqp_raceline_warm_start_batch(s._h, -1, _ffi.dptr(x0), C.byref(W), None, None) == _ffi.E_ARG
    assert s._lib.dgsqp_last_error(s._h).startswith(b'raceline: B < 0')
    assert s._lib.dgsqp_sample_raceline_batch(s._h, -1, C.byref(spec), C.byref(W), None, None, None, 0) == _ffi.E_ARG
    assert s.raceline_warm_start_batch(x0[:0], W)['ok'].shape == (0,)
    bad = mc.raceline_ws(g)
    bad.mpc.w_du[0] = 0.0
    with pytest.raises(ValueError, match='mpc: w_du'):          # what the tracker refuses
        s.raceline_warm_start_batch(x0, bad)
    bad = mc.raceline_ws(g)
    bad.mpc.N = 5
    with pytest.raises(ValueError, match="raceline: the tracker's N"):
        s.raceline_warm_start_batch(x0, bad)
    assert s.raceline_warm_start_batch(x0, W)['ok'].all()          # the handle is fine after every refusal
    m = mc.merge_game(N=4)
    u = DGSQP(*m.solver_args(), print_method=None)
    u.set_raceline(g.raceline)
    with pytest.raises(ValueError, match='raceline: agent 0 is no Frenet-frame bicycle'):
        u.raceline_warm_start_batch(np.zeros((2, u.n_q)), W)


def test_256_thread_build(dyn4):
    """libdgsqp_hip_b256.so exports the entries, runs the N = 4 case bit for bit like its own host loop, and refuses what its tracker refuses."""
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g, _, tracker, W = dyn4
    s = DGSQP(*g.solver_args(), print_method=None, workgroups_per_cu=2)
    for name in ('dgsqp_set_raceline', 'dgsqp_raceline_warm_start_batch', 'dgsqp_fetch_raceline_ref', 'dgsqp_sample_raceline_batch'):
        assert hasattr(s._lib, name)
    s.set_raceline(g.raceline)
    x0 = edge_states(g)[:6]
    dev = s.raceline_warm_start_batch(x0, W)
    host_u, host_ok = rc.host_loop(g, tracker, rc.lowered_tracker(g, tracker, workgroups_per_cu=2), x0, s.fetch_raceline_ref(6))
    assert dev['ok'].all() and host_ok.all() and np.array_equal(bits(dev['u_ws']), bits(host_u))
    out = s.sample_raceline_batch(g, 40, seed=3, ws=W)
    assert out['x0'].shape == (40, 16) and out['candidates'] >= 40
    bad = mc.raceline_ws(g)
    bad.mpc.n_soft = 2
    with pytest.raises(ValueError, match='mpc: n_soft'):
        s.raceline_warm_start_batch(x0, bad)


@pytest.mark.parametrize('front_end', ['raceline', 'circuit'])
def test_example_driver_writes_the_studys_records(tmp_path, monkeypatch, front_end):
    """examples/monte_carlo_barc_dynamic.py (the DG-SQP leg of comparison_study_barc/monte_carlo_main.py): one sample_<i>.pkl per scenario
    with the keys analyze_data.py reads, and the records are those of a plain solve_batch of the same sampled batch."""
    import pickle
    import sys
    from dgsqp_amd.solver import DGSQP
    monkeypatch.syspath_prepend(str(rc.ROOT / 'examples'))
    sys.modules.pop('monte_carlo_barc_dynamic', None)
    import monte_carlo_barc_dynamic as ex
    from dgsqp_amd.montecarlo import place_raceline_sequential as mc_place, raceline_ws as mc_ws
    out = tmp_path / 'out'
    samples = ex.main(['--num-mc', '12', '--N', '6', '--solver', 'v1', '--rk4-substeps', '2', '--front-end', front_end, '--seed', '3', '--out', str(out)])
    files = sorted(out.glob('sample_*.pkl'), key=lambda p: int(p.stem.split('_')[1]))
    assert [p.name for p in files] == [f'sample_{i + 1}.pkl' for i in range(12)]
    d = pickle.load(open(files[4], 'rb'))
    assert set(d) == {'solver_result', 'initial_condition'} and {'msg', 'time', 'num_iters', 'status'} <= set(d['solver_result'])
    assert len(d['initial_condition']) == 2 and hasattr(d['initial_condition'][0].x, 'x')
    g = rc.dynamic_game(N=6, rk4_substeps=2) if front_end == 'raceline' else None
    if g is None:
        from dgsqp_amd.montecarlo import dynamic_racing_game
        g = dynamic_racing_game(track_kind='barc', N=6, rk4_substeps=2)
    s = DGSQP(*g.solver_args(), print_method=None)
    batch = s.sample_raceline_batch(g, 12, seed=3) if front_end == 'raceline' else s.sample_batch(g, 12, seed=3)
    ref = s.solve_batch(batch['x0'], batch['u_ws'])
    assert [r['solver_result']['num_iters'] for r in samples] == list(ref['num_iters'])
    assert [r['solver_result']['msg'] for r in samples] == list(ref['msg'])
    assert abs(samples[4]['initial_condition'][1].p.s - batch['x0'][4, 14]) < 1e-15
    if front_end == 'raceline':          # --host-sampler: the script's sequential draws, warm starts through the same program
        from dgsqp_amd.montecarlo import sample_scenarios
        host = ex.main(['--num-mc', '12', '--N', '6', '--solver', 'v1', '--rk4-substeps', '2', '--seed', '0', '--host-sampler'])
        x0, u_ws = sample_scenarios(g, 12, seed=0, solver=s)
        ref = s.solve_batch(x0, u_ws)
        assert [r['solver_result']['num_iters'] for r in host] == list(ref['num_iters']) and [r['solver_result']['msg'] for r in host] == list(ref['msg'])
        rng = np.random.default_rng(0)
        first = None
        while first is None:
            q, margin = mc_place(g, rng)
            first = q if margin < 0 else None
        if s.raceline_warm_start_batch(first[None], mc_ws(g))['ok'][0]:
            assert np.array_equal(first, x0[0])
