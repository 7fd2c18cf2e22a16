"""Raceline warm starts, the host side (no GPU): the numpy look-ups of ``montecarlo.Raceline`` against ``np.interp`` and their linear
continuation; the refusals; the reference-trajectory mirror; ``input_scaling`` lowered as an exact change of variables, against the
reference's scaled QP restated in numpy; the sequential host sampler's draws; the public surface and the struct layouts."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import ltv_mpc_checks as chk
import raceline_checks as rc

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ('dgsqp_set_raceline', 'dgsqp_raceline_warm_start_batch', 'dgsqp_fetch_raceline_ref', 'dgsqp_sample_raceline_batch')


@pytest.fixture(scope='module')
def rl():
    return rc.raceline()


def test_table_is_the_two_lap_table_of_load_mpclab_raceline(rl):
    from dgsqp_amd.tracks import get_track
    f = np.load(rc.FIXTURE)
    n, L = len(f['t']), get_track('L_track_barc').track_length
    assert rl.T.shape == (2 * n - 1,) and rl.cols.shape == (2 * n - 1, 9) and rl.lap_mat.shape == (n, 9) and 2 * n - 1 == 4401
    assert np.array_equal(rl.T[:n], f['t'] * rc.TIME_SCALE) and np.array_equal(rl.T[n:], (f['t'] * rc.TIME_SCALE + f['t'][-1] * rc.TIME_SCALE)[1:])
    assert np.array_equal(rl.cols[:n, 3], f['v_long'] / rc.TIME_SCALE) and np.array_equal(rl.cols[:n, 5], f['psidot'] / rc.TIME_SCALE)
    assert np.array_equal(rl.cols[n:, 7], (f['s'] + L)[1:]) and np.array_equal(rl.cols[n:, 8], f['e_y'][1:])


def test_lookups_agree_with_numpy_interp(rl):
    """1e-13 max(1, |value|): the formula has four roundings; a neighbouring segment would be off by about 1e-5."""
    rng = np.random.default_rng(0)
    S, T = rl.cols[:, 7], rl.T
    n = (len(T) + 1) // 2
    L, T_lap = S[n - 1], T[n - 1]
    s = np.concatenate((rng.uniform(S[0], S[-1], 1000), S[::97], [L], rng.uniform(L, S[-1], 50)))
    t = np.concatenate((rng.uniform(T[0], T[-1], 1000), T[::97], [T_lap], rng.uniform(T_lap, T[-1], 50)))
    got, want = rl.s2t(s), np.interp(s, S, T)
    assert (np.abs(got - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
    ev = rl.eval(t)
    for c in range(9):
        want = np.interp(t, T, rl.cols[:, c])
        assert (np.abs(ev[:, c] - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all(), (c, np.abs(ev[:, c] - want).max())
    assert rl.s2t(L) == T_lap and np.array_equal(rl.eval(T_lap), rl.cols[n - 1])
    assert np.array_equal(rl.eval(T[::97]), rl.cols[::97])          # a knot exactly: its own row


def test_lookups_continue_the_end_segments_linearly(rl):
    S, T = rl.cols[:, 7], rl.T
    s = -0.3
    want = T[0] + (T[1] - T[0]) * (s - S[0]) / (S[1] - S[0])
    assert abs(rl.s2t(s) - want) <= 1e-13 * max(1.0, abs(want)) and rl.s2t(s) < T[0]
    t = T[-1] + 0.2
    want = rl.cols[-2] + (rl.cols[-1] - rl.cols[-2]) * (t - T[-2]) / (T[-1] - T[-2])
    assert (np.abs(rl.eval(t) - want) <= 1e-13 * np.maximum(1.0, np.abs(want))).all()
    assert rl.eval(t)[7] > S[-1]


def test_every_refusal_of_the_table():
    from dgsqp_amd.montecarlo import Raceline
    T, cols = np.arange(4.0), np.tile(np.arange(4.0)[:, None], (1, 9))
    Raceline(T, cols)
    with pytest.raises(ValueError, match='^raceline: '):
        Raceline(T[:1], cols[:1])
    for i, j, v in ((1, 2, np.nan), (2, 7, np.inf)):
        bad = cols.copy(); bad[i, j] = v
        with pytest.raises(ValueError, match='^raceline: a non-finite'):
            Raceline(T, bad)
    with pytest.raises(ValueError, match='^raceline: a non-finite'):
        Raceline(np.array([0, 1, np.nan, 3]), cols)
    with pytest.raises(ValueError, match='^raceline: T is not strictly increasing'):
        Raceline(np.array([0, 1, 1, 3.0]), cols)
    bad = cols.copy(); bad[2, 7] = bad[1, 7]
    with pytest.raises(ValueError, match='^raceline: the s column is not strictly increasing'):
        Raceline(T, bad)


@pytest.mark.parametrize('kind', ['dynamic', 'kinematic'])
def test_reference_mirror_starts_at_the_car_and_advances(rl, kind):
    g = rc.dynamic_game(N=6) if kind == 'dynamic' else rc.kinematic_game(N=6)
    rng = np.random.default_rng(4)
    L = g.track.track_length
    x0 = rc.states_on_raceline(g, rng.uniform(0.0, L, 64), d_ey=rng.uniform(-0.2, 0.2, 64), d_v=rng.uniform(-0.5, 0.5, 64))
    nqa = g.joint_model.dynamics_models[0].n_q
    for a in range(2):
        q0 = x0[:, a * nqa:(a + 1) * nqa]
        q = rl.q_ref(q0, 6, 0.1)
        assert q.shape == (64, 7, nqa)
        for i in (nqa - 2, nqa - 1, 2):            # s0, e_y0, v_long0
            assert (np.abs(q[:, 0, i] - q0[:, i]) <= 1e-12 * np.maximum(1.0, np.abs(q0[:, i]))).all(), i
        assert (np.diff(q[:, :, nqa - 2], axis=1) > 0).all()


def test_input_scaling_is_lowered_as_an_exact_change_of_variables(oracle, games):
    """The reference's QP in its scaled variables (x' = T x with Tu = 1 / input_scaling on u AND on du: u'_{k+1} = u'_k + dt du',
    CA_LTV_MPC.py:396-405; rate cost and rate box on du') against the unscaled QP built from the LOWERED record (w_du Tu^2, du box / Tu):
    kinematic bicycle, N = 3, with one active rate bound (stage 0) and an input bound active at the two stages after it.  The scaled QP is solved on the active set the unscaled
    one found and then CHECKED to be its own minimiser (its own bounds hold, its multipliers are non-negative); mapped back it equals the
    unscaled minimiser to 1e-9 relative.  The only term that is not invariant is the reference's 1e-10 I on the (q, u) blocks, which moves
    the minimiser by at most about 1e-10 / w_du = 1e-9 relative (w_du = 0.1): the bar.  Measured: printed below (1.7e-12 when this was
    written)."""
    from dgsqp_amd import ltv_mpc
    g, P, par = games['kb_curve_N10']
    N, scaling = 3, [2, 0.45]
    Tu = 1.0 / np.asarray(scaling)
    q0 = np.array([0.5, 0.1, 1.6, 0.03, 0.5, 0.1])
    u_ws = np.zeros((N + 1, 2)); u_ws[:, 0] = 0.1
    du_ws = np.zeros((N, 2))
    q_ref = np.zeros((N + 1, 6)); q_ref[:, 2] = 3.0; q_ref[:, 4] = 0.5 + 0.3 * np.arange(N + 1)
    cost = ltv_mpc.TrackingCost(state_weight=[0, 0, 1, 0.5, 2, 5], input_weight=(1e-2, 1e-2), rate_weight=(0.1, 0.1))
    q_ub, q_lb = 1e10 * np.ones(6), -1e10 * np.ones(6)
    b = (q_ub, q_lb, (0.25, 0.4), (-0.25, -0.4), (0.5, 2.0), (-0.5, -2.0))
    raw = chk.record_dict(ltv_mpc.lower(0, 6, cost, None, None, *b, N, 2, 0.75), 6)
    low = chk.record_dict(ltv_mpc.lower(0, 6, cost, None, None, *b, N, 2, 0.75, input_scaling=scaling), 6)
    assert np.array_equal(low['w_du'], raw['w_du'] * Tu * Tu) and np.array_equal(low['du_ub'], raw['du_ub'] / Tu) and np.array_equal(low['du_lb'], raw['du_lb'] / Tu)
    assert all(np.array_equal(low[k], raw[k]) for k in ('w_u', 'u_ub', 'u_lb', 'w_q', 'q_ub', 'q_lb'))       # input cost and box untouched
    dyn = chk.oracle_dyn(oracle, P, 0)
    nz = 8
    D = np.concatenate((np.hstack((chk.rollout(dyn, q0, u_ws[1:]), u_ws)).ravel(), du_ws.ravel()))
    rows = []
    for k in range(N):
        for j in range(2):
            rows += [(chk.RATE, k, j, 1), (chk.RATE, k, j, -1)]
    for k in range(1, N + 1):
        for j in range(2):
            rows += [(chk.INPUT, k, j, 1), (chk.INPUT, k, j, -1)]
    h = chk.solve_iteration(oracle, low, float(P.dt), dyn, rows, D, q0, u_ws[0], q_ref, None)
    assert h['flag'] == 0 and h['strict']
    act = np.nonzero(h['active'])[0]
    kinds = [rows[i][0] for i in act]
    print('active rows:', [rows[i] for i in act])
    assert chk.RATE in kinds and chk.INPUT in kinds
    # the reference's scaled QP from the RAW record, on that active set
    qs = chk.uncondensed_qp(raw, float(P.dt), dyn, D, q0, u_ws[0], q_ref, None, scale_u=Tu)
    nD = qs['nD']
    S = np.concatenate((qs['scal'][:(N + 1) * nz], np.tile(Tu, N)))          # x' = S x: the (q, u) blocks, then du' = Tu du
    As = np.vstack((qs['A_eq'], h['Ad'][act] / S[None, :]))
    K = np.block([[qs['H'], As.T], [As, np.zeros((As.shape[0],) * 2)]])
    sol = np.linalg.solve(K, np.concatenate((-qs['h'], qs['b_eq'], h['bd'][act])))
    xs, mult = sol[:nD], sol[nD + qs['A_eq'].shape[0]:]
    assert (mult > 0).all()                                                            # ... it is the scaled QP's minimiser: multipliers,
    tol = 1e-9 * np.maximum(1.0, np.abs(xs))
    assert (xs[nz:] <= qs['ub'][nz:] + tol[nz:]).all() and (xs[nz:] >= qs['lb'][nz:] - tol[nz:]).all()      # its own bounds,
    du_s = xs[(N + 1) * nz:]
    at = np.isclose(du_s, np.tile(raw['du_ub'], N), rtol=0, atol=1e-9) | np.isclose(du_s, np.tile(raw['du_lb'], N), rtol=0, atol=1e-9)
    assert at.sum() == kinds.count(chk.RATE)                                           # and its rate box active where the lowered one is
    dev = chk.rel(xs / S, h['D_bar'])
    print(f'scaled minimiser mapped back against the lowered record\'s minimiser (relative): {dev:.3e}')
    assert dev < 1e-9


def test_host_scaling_takes_input_scaling_out_before_the_device_check():
    """warm_start_dynamic.py's own CALTVMPCParams pass: host_scaling returns parameters without input_scaling (what check_params sees)
    and Tu = 1 / input_scaling; everything else still refused stays refused."""
    from dgsqp_amd import ltv_mpc, montecarlo as mc
    from dgsqp_amd.solver_types import CALTVMPCParams
    p = CALTVMPCParams(N=25, state_scaling=[10, 10, 7, np.pi / 2, 17.4, 1.0], input_scaling=[2, 0.45], damping=0.75, qp_iters=5, delay=None,
                       verbose=False, qp_interface='casadi')
    dev, Tu = ltv_mpc.host_scaling(p)
    ltv_mpc.check_params(dev)
    assert dev.input_scaling is None and p.input_scaling == [2, 0.45] and np.array_equal(Tu, 1.0 / np.array([2, 0.45]))
    assert (dev.N, dev.qp_iters, dev.damping, dev.state_scaling) == (25, 5, 0.75, p.state_scaling)
    q, none = ltv_mpc.host_scaling(CALTVMPCParams(N=7))
    assert none is None and q.N == 7
    for bad in ([2, 0.0], [2, -1], [2, np.nan], [2]):
        with pytest.raises(ValueError, match='input_scaling'):
            ltv_mpc.host_scaling(CALTVMPCParams(input_scaling=bad))
    with pytest.raises(NotImplementedError, match='delay'):
        ltv_mpc.check_params(ltv_mpc.host_scaling(CALTVMPCParams(input_scaling=[2, 0.45], delay=[1, 1]))[0])
    W = mc.raceline_ws(rc.dynamic_game(N=4))          # the study's tracker goes through the same step
    assert list(W.mpc.du_ub) == [10.0 / 0.5, 4.5 / (1.0 / 0.45)] and W.mpc.qp_iters == 5


def test_host_sampler_consumes_six_draws_per_candidate_in_the_scripts_order(rl):
    from dgsqp_amd import montecarlo as mc
    g = rc.dynamic_game()

    class Counting:
        def __init__(self, seed):
            self.rng, self.n = np.random.default_rng(seed), 0

        def random(self):
            self.n += 1
            return self.rng.random()
    cnt = Counting(0)
    L, H, obs_d = g.track.track_length, g.track.half_width, g.obs_d
    ref = np.random.default_rng(0)
    for i in range(20):
        x0, margin = mc.place_raceline_sequential(g, cnt)
        assert cnt.n == 6 * (i + 1)
        u = [ref.random() for _ in range(6)]
        s1 = L * u[0]
        r1 = rl.eval(rl.s2t(s1))
        s2 = s1 + 1.2 * obs_d * (2 * u[3] - 1)
        r2 = rl.eval(rl.s2t(s2))
        assert x0[6] == s1 and x0[14] == s2
        assert x0[7] == max(min(r1[8] + (2 * u[1] - 1), 0.9 * H), -0.9 * H) and x0[15] == max(min(r2[8] + (2 * u[4] - 1), 0.9 * H), -0.9 * H)
        assert x0[2] == r1[3] + (1.5 * u[2] - 0.75) and x0[10] == r2[3] + (1.5 * u[5] - 0.75)
        assert x0[5] == r1[6] and x0[13] == r2[6] and not x0[[3, 4, 11, 12]].any()
        d2 = (x0[0] - x0[8]) ** 2 + (x0[1] - x0[9]) ** 2
        assert margin == mc.STUDY_COLLISION_D ** 2 - d2
    with pytest.raises(ValueError, match='solver='):
        mc.sample_scenarios(g, 4, seed=0)
    assert mc.dynamic_racing_game(track_kind='barc', N=4).sampler == 'circuit'           # the default stays
    with pytest.raises(ValueError, match='raceline='):
        mc.dynamic_racing_game(track_kind='barc', N=4, sampler='raceline')
    with pytest.raises(ValueError, match='does not fit'):
        mc.dynamic_racing_game(track_kind='curve', N=4, sampler='raceline', raceline=rl)


def test_counter_based_placement_is_the_sequential_rule(rl):
    """The mirror of the device placement (six counter-based uniforms per candidate) and the sequential host rule are the same function
    of their six uniforms."""
    from dgsqp_amd import montecarlo as mc, sampler as smp
    g = rc.dynamic_game()
    cand = np.arange(40, dtype=np.uint64)
    x0, margin = smp.place_raceline(g, 11, cand)

    class Replay:
        def __init__(self, vals):
            self.vals = list(vals)

        def random(self):
            return self.vals.pop(0)
    for c in range(40):
        x, m = mc.place_raceline_sequential(g, Replay(float(smp.uniform(11, np.array([c], np.uint64), k)[0]) for k in range(6)))
        assert np.array_equal(x, x0[c]) and m == margin[c]


def test_surface_and_struct_layouts(tmp_path):
    import DGSQP.tracks.track_lib as tl
    import dgsqp_amd.tracks
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc.build import OUT, OUT_B256, build
    assert tl.load_mpclab_raceline is dgsqp_amd.tracks.load_mpclab_raceline
    raceline, s2t, mat = tl.load_mpclab_raceline(rc.FIXTURE, 'L_track_barc', time_scale=rc.TIME_SCALE)
    assert mat.shape == (2201, 9) and len(raceline(0.5)) == 9
    assert float(raceline(s2t(1.25))[7]) == pytest.approx(1.25, abs=1e-12)
    assert np.array(raceline(np.array([0.1, 0.2]))).squeeze().T.shape == (2, 9)           # the script's own call shape (warm_start_dynamic.py:151)
    build()
    header = (ROOT / 'include' / 'dgsqp.h').read_text()
    declared = set(re.findall(r'\b(dgsqp_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and name in _ffi.SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        for so in (OUT, OUT_B256):
            assert hasattr(ctypes.CDLL(str(so)), name), (so.name, name)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\nint main(){'
    want = []
    for cname, T in (('dgsqp_raceline_ws_t', _ffi.RacelineWsT), ('dgsqp_raceline_sampler_t', _ffi.RacelineSamplerT)):
        src += f'printf("%zu ", sizeof({cname}));'
        want.append(ctypes.sizeof(T))
        for f, _ in T._fields_:
            src += f'printf("%zu %zu ", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));'
            want += [getattr(T, f).offset, getattr(T, f).size]
    src += 'printf("%d\\n", DGSQP_RL_COLS);return 0;}\n'
    exe = tmp_path / 'raceline_layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [_ffi.RL_COLS]
