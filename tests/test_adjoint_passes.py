"""The three stage recursions over A_k, B_k -- sensitivity chains (G, q), costates (lam, trial merits) and the second-order adjoint
rows (Q) -- against the CPU oracle, at the smallest shapes at which each of their forms can go wrong:

* the forward tangent is propagated once, by the chains, and handed to the Hessian rows through the global scratch;
* only the own blocks H[a][k][a] of the contracted Taylor tensor are formed;
* a trial merit's costate sweep leaves the state-Hessian columns alone;
* uniform games of up to four agents run one lane per (row, block) of Q, so n = 100 needs more than 128 lanes and n = 150 more
  than 512 (a second pass of the strided loop); five and six agents stay on the one-lane-per-row kernel.

Bars: q, G, Q to the 1e-12 relative bar of tests/test_gpu.py::test_evaluate_parity (same definition of ``rel``); whole solves to the rule
of test_solve_matches_golden_fixtures (identical status / iterations / QP solves on the oracle-stable scenarios, iterates within 1e-5).

No public constructor of dgsqp_amd.montecarlo builds a game whose agents have different state sizes, so the one-lane-per-row
kernel is reached here through the six-agent case only (tests/test_point_mass.py holds a mixed three-car fixture of its own)."""
import numpy as np
import pytest

from conftest import assert_control_flow_parity, stable_mask, tight_lsqr

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def _game(name):
    from dgsqp_amd.montecarlo import dynamic_racing_game, kinematic_racing_game, merge_game
    return {'kb_curve_N2_M2': lambda: kinematic_racing_game('curve', N=2, M=2),         # rows with k0 = N - 1: no live tangent in the backward sweep
            'kb_curve_N3_M3': lambda: kinematic_racing_game('curve', N=3, M=3),         # three blocks
            'kb_curve_N3_M1': lambda: kinematic_racing_game('curve', N=3, M=1),         # one agent: the own block is the only one
            'dyn_N4_rk4x2': lambda: dynamic_racing_game(N=4, rk4_substeps=2),           # 8 states per agent
            'dyn_N4_rk4x4': lambda: dynamic_racing_game(N=4, rk4_substeps=4),
            'merge_N3_M3': lambda: merge_game(N=3, M=3),                                # 4 states per agent
            'merge_N3_M6': lambda: merge_game(N=3, M=6),                                # one lane per row, block a among six
            'kb_curve_N25_M2': lambda: kinematic_racing_game('curve', N=25, M=2),       # n = 100: 200 (row, block) items
            'kb_curve_N25_M3': lambda: kinematic_racing_game('curve', N=25, M=3),       # n = 150, XL layout: 450 items in 576 slots, a second pass
            'kb_chicane_N15': lambda: kinematic_racing_game('chicane', N=15)}[name]()


def _evaluate_against_oracle(oracle, g, B=4, **solver_kw):
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP, build_problem
    P = build_problem(*g.solver_args())
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13, **solver_kw)
    x0, u_tm = sample_scenarios(g, B, seed=21)
    rng = np.random.default_rng(0)
    u = s._to_agent_major(u_tm) + 0.01 * rng.standard_normal((B, s.n))
    l = np.maximum(0, rng.standard_normal((B, s.n_c_total)))
    ev = s.evaluate_batch(x0, u, l)
    worst = {}
    for b in range(B):
        o = oracle.evaluate(P, x0[b], u[b], l[b], 1)
        for key in ('q', 'G', 'Q'):
            worst[key] = max(worst.get(key, 0.0), rel(ev[key][b], o[key]))
    print(g.name, 'n', s.n, {k: f'{v:.1e}' for k, v in worst.items()})
    for key in ('q', 'G', 'Q'):
        assert worst[key] < 1e-12, (key, worst[key])


@pytest.mark.parametrize('name', ['kb_curve_N2_M2', 'kb_curve_N3_M3', 'kb_curve_N3_M1', 'dyn_N4_rk4x2', 'merge_N3_M3', 'merge_N3_M6',
                                  'kb_curve_N25_M2', 'kb_curve_N25_M3'])
def test_evaluate_batch_parity(oracle, name):
    """q, G and raw Q of ``evaluate_batch`` against the oracle on 4 sampled scenarios, multipliers max(0, N(0, 1))."""
    _evaluate_against_oracle(oracle, _game(name))


def test_evaluate_batch_parity_on_the_256_thread_build(oracle):
    """The same on the two-workgroups-per-CU build (256 threads): n = 60, 120 (row, block) items."""
    _evaluate_against_oracle(oracle, _game('kb_chicane_N15'), workgroups_per_cu=2)


def test_bit_reproducibility():
    """Two evaluations and two solves of the same 16 scenarios return identical bits (the hand-over of the tangents between lanes
    goes through a fence and a barrier; a race would show here)."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP
    g = _game('dyn_N4_rk4x4')
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = sample_scenarios(g, 16, seed=5)
    u = s._to_agent_major(u_tm)
    l = np.maximum(0, np.random.default_rng(2).standard_normal((16, s.n_c_total)))
    e1, e2 = s.evaluate_batch(x0, u, l), s.evaluate_batch(x0, u, l)
    for key in e1:
        assert np.array_equal(e1[key], e2[key], equal_nan=True), key
    r1, r2 = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm)
    for key in ('u', 'l', 'x', 'cond', 'cost', 'status', 'num_iters', 'qp_solves'):
        assert np.array_equal(r1[key], r2[key], equal_nan=True), key


@pytest.mark.parametrize('name', ['dyn_N4_rk4x4', 'kb_chicane_N15'])
def test_solves_match_the_oracle_through_the_trial_merits(oracle, name):
    """Whole solves of 16 scenarios against the oracle's: every line-search trial takes its merit from the costate sweep without the
    state-Hessian columns.  Rule and bars of test_solve_matches_golden_fixtures."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP, build_params, build_problem
    g = _game(name)
    P, par = build_problem(*g.solver_args()), tight_lsqr(build_params(g.params))
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    x0, u_tm = sample_scenarios(g, 16, seed=7)
    u = s._to_agent_major(u_tm)
    res = s.solve_batch(x0, u_tm)
    ref = oracle.solve_batch(P, par, x0, u, nthreads=8)
    stable = stable_mask(oracle, P, par, x0, u, ref)
    same = assert_control_flow_parity(res, ref, stable, name, min_stable_same=0.95, max_conv_gap=0.05)
    assert same.mean() >= 0.85
    for b in np.where(same & (ref['status'] <= 1))[0]:
        assert rel(res['u'][b], ref['u'][b]) < 1e-5, b
        if ref['status'][b] == 0:
            assert rel(res['l'][b], ref['l'][b]) < 1e-5, b
            assert rel(res['cost'][b], ref['cost'][b]) < 1e-8, b
