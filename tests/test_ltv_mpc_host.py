"""The LTV-MPC tracker, host side (no GPU): the five C-ABI entries are declared, exported by both builds and bound; dgsqp_mpc_t,
dgsqp_mpc_row_t and dgsqp_mpc_dims_t have one layout in C and in ctypes; CALTVMPCParams has the reference's fields and defaults; the alias
module resolves; every Python-side refusal fires; step()'s warm-start shift on hand-made arrays; the helper's condensed and uncondensed
minimisers agree on the CPU; the size of the scaling deviation is measured and printed."""
import ctypes
import dataclasses
import json
import pathlib
import re
import subprocess

import numpy as np
import pytest

import ltv_mpc_checks as chk

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ('dgsqp_set_mpc', 'dgsqp_mpc_dims', 'dgsqp_mpc_batch', 'dgsqp_set_mpc_log', 'dgsqp_fetch_mpc_log')


def test_symbols_are_declared_exported_and_bound():
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc.build import OUT, OUT_B256, build
    build()
    header = (ROOT / 'include' / 'dgsqp.h').read_text()
    declared = set(re.findall(r'\b(dgsqp_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and name in _ffi.SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        for so in (OUT, OUT_B256):
            assert hasattr(ctypes.CDLL(str(so)), name), (so.name, name)
    for wg in (1, 2):
        lib = _ffi.load_library(wg)
        assert lib.dgsqp_set_mpc.argtypes[1] == ctypes.POINTER(_ffi.MpcT) and len(lib.dgsqp_mpc_batch.argtypes) == 13
    assert re.search(r'#define\s+DGSQP_MPC_NMAX\s+128\s', header) and _ffi.MPC_NMAX == 128


@pytest.mark.parametrize('cname,T', [('dgsqp_mpc_t', 'MpcT'), ('dgsqp_mpc_row_t', 'MpcRowT'), ('dgsqp_mpc_dims_t', 'MpcDimsT')])
def test_struct_layouts_match_the_header(tmp_path, cname, T):
    from dgsqp_amd import _ffi
    S = getattr(_ffi, T)
    fields = [name for name, _ in S._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\n'
           f'int main(){{printf("%zu", sizeof({cname}));\n'
           + ''.join(f'printf(" %zu %zu", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));\n' for f in fields)
           + 'printf(" %d %d %d\\n", DGSQP_MPC_ROW_RATE, DGSQP_MPC_ROW_OBS, DGSQP_E_TOO_LARGE);return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(S)] + [v for f in fields for v in (getattr(S, f).offset, getattr(S, f).size)]
    assert got[:-3] == want
    assert got[-3:] == [_ffi.MPC_ROW_RATE, _ffi.MPC_ROW_OBS, _ffi.E_TOO_LARGE]


def _defaults(cls):
    return {f.name: f.default for f in dataclasses.fields(cls)}


def test_caltvmpc_param_defaults_match_reference_golden():
    from dgsqp_amd.solver_types import CALTVMPCParams
    gold = json.loads((ROOT / 'tests' / 'golden' / 'caltvmpc_params.json').read_text())
    mine = _defaults(CALTVMPCParams)
    assert sorted(mine) == sorted(gold)
    for k, v in gold.items():
        assert mine[k] == v and type(mine[k]) is type(v), (k, mine[k], v)


def test_caltvmpc_param_defaults_match_reference_live():
    import sys
    ref = pathlib.Path('/root/reference')
    if not (ref / 'DGSQP' / 'solvers' / 'solver_types.py').exists():
        pytest.skip('reference tree not present')
    code = ('import sys, json, dataclasses; sys.path.insert(0, sys.argv[1]); from DGSQP.solvers.solver_types import CALTVMPCParams as R; '
            'print(json.dumps({f.name: f.default for f in dataclasses.fields(R)}))')
    out = subprocess.run([sys.executable, '-c', code, str(ref)], capture_output=True, text=True, cwd='/')
    assert out.returncode == 0, out.stderr[-2000:]          # a missing tree skips (above); a tree that does not import fails
    from dgsqp_amd.solver_types import CALTVMPCParams
    assert json.loads(out.stdout) == json.loads(json.dumps(_defaults(CALTVMPCParams)))


def test_alias_module_resolves():
    import dgsqp_amd.ltv_mpc
    from DGSQP.solvers.CA_LTV_MPC import CA_LTV_MPC
    from DGSQP.solvers.solver_types import CALTVMPCParams
    assert CA_LTV_MPC is dgsqp_amd.ltv_mpc.CA_LTV_MPC and CALTVMPCParams is dgsqp_amd.solver_types.CALTVMPCParams


def test_every_python_side_refusal_fires():
    from dgsqp_amd import ltv_mpc
    from dgsqp_amd.solver_types import CALTVMPCParams
    for kw, word in ((dict(delay=[1, 1]), 'delay'), (dict(wrapped_state_idxs=[3], wrapped_state_periods=[6.28]), 'wrapped_state_idxs'),
                     (dict(soft_constraint_idxs=[[0]]), 'soft_constraint'), (dict(qp_interface='hpipm'), 'qp_interface'), (dict(qp_interface='cvxpy'), 'qp_interface'),
                     (dict(code_gen=True), 'code_gen'), (dict(jit=True), 'code_gen'), (dict(reg=1e-3), 'reg')):
        with pytest.raises(NotImplementedError, match=word):
            ltv_mpc.check_params(CALTVMPCParams(**kw))
    ltv_mpc.check_params(CALTVMPCParams(state_scaling=[1, 2, 3, 4, 5, 6]))        # accepted: a change of variables
    with pytest.raises(NotImplementedError, match='input_scaling'):      # not one in the reference (its du is in scaled units): refused
        ltv_mpc.check_params(CALTVMPCParams(input_scaling=[2, 0.45]))
    with pytest.raises(ValueError, match='state_scaling'):
        ltv_mpc.check_params(CALTVMPCParams(state_scaling=[1, 0, 3, 4, 5, 6]))
    cost = ltv_mpc.TrackingCost(state_weight=np.ones(6), rate_weight=(1.0, 0.0))
    b = (np.ones(6), -np.ones(6), (1, 1), (-1, -1), (1, 1), (-1, -1))
    with pytest.raises(ValueError, match='rate_weight must be positive'):
        ltv_mpc.lower(0, 6, cost, None, None, *b, 5, 2, 0.75)
    ok = ltv_mpc.TrackingCost(state_weight=np.ones(6))
    with pytest.raises(NotImplementedError, match='one soft state'):
        ltv_mpc.lower(0, 6, ok, ltv_mpc.SoftStateBounds([4, 5], [1, 1], [1, 1]), None, *b, 5, 2, 0.75)
    with pytest.raises(ValueError, match='state_weight needs 6'):
        ltv_mpc.lower(0, 6, ltv_mpc.TrackingCost(state_weight=np.ones(5)), None, None, *b, 5, 2, 0.75)
    for costs, constraints, word in (('casadi function', None, 'TrackingCost'), (ok, dict(rate=[object()]), 'rate-constraint'), (ok, object(), 'ObstacleAvoidance')):
        with pytest.raises(NotImplementedError, match=word):
            ltv_mpc.CA_LTV_MPC(None, costs, constraints, {}, CALTVMPCParams())
    r = ltv_mpc.lower(1, 6, ok, ltv_mpc.SoftStateBounds([5], [5.0], [25.0]), ltv_mpc.ObstacleAvoidance(0.21), *b, 7, 3, 0.5, True)
    assert (r.agent, r.N, r.qp_iters, r.zero_du, r.damping, r.n_soft, r.soft_idx[0], r.soft_quad[0], r.soft_lin[0], r.obs_r) == (1, 7, 3, 1, 0.5, 1, 5, 5.0, 25.0, 0.21)
    assert r.q_ub[6] == np.inf and r.q_lb[7] == -np.inf


def test_step_warm_start_shift():
    from dgsqp_amd.ltv_mpc import shift_warm_start
    u = np.arange(8.0).reshape(4, 2)
    du = 10 + np.arange(8.0).reshape(4, 2)
    uw, dw = shift_warm_start(u, du)
    assert uw.tolist() == [[0, 1], [2, 3], [4, 5], [6, 7], [6, 7]]          # row 0, the next u_prev, is the input just applied
    assert dw.tolist() == [[12, 13], [14, 15], [16, 17], [16, 17]]


def _cpu_case(games, N=4, seed=5):
    from dgsqp_amd import _ffi, ltv_mpc
    g, P, par = games['kb_curve_N10']
    rng = np.random.default_rng(seed)
    q0 = np.array([0.5, 0.1, 1.6, 0.03, 0.5, 0.1])
    u_ws = np.stack([0.3 * rng.standard_normal(N + 1), 0.05 * rng.standard_normal(N + 1)], axis=1)
    du_ws = 0.1 * rng.standard_normal((N, 2))
    q_ref = np.zeros((N + 1, 6)); q_ref[:, 2] = 1.8; q_ref[:, 4] = 0.5 + 0.18 * np.arange(N + 1)
    cost = ltv_mpc.TrackingCost(state_weight=[0, 0, 1, 0.5, 2, 5], input_weight=(1e-2, 1e-2), rate_weight=(0.01, 1.0))
    q_ub, q_lb = 1e10 * np.ones(6), -1e10 * np.ones(6)
    q_ub[5], q_lb[5] = 0.2, -0.2
    rec = ltv_mpc.lower(0, 6, cost, None, None, q_ub, q_lb, (0.5, 0.1), (-0.5, -0.1), (1.5, 0.6), (-1.5, -0.6), N, 2, 0.75)
    return P, rec, q0, u_ws, du_ws, q_ref


def _rows(R):
    """The row table dgsqp_set_mpc builds (dgsqp_api.hip: mpc_plan), restated."""
    N, nq, ns = R['N'], R['n_q'], len(R['soft_idx'])
    fin = lambda v: int(abs(v) < 1e9)
    rows = []
    for k in range(N):
        for j in range(2):
            rows += [(chk.RATE, k, j, 1)] * fin(R['du_ub'][j]) + [(chk.RATE, k, j, -1)] * fin(R['du_lb'][j])
    rows += [(chk.SLACK, 0, i, -1) for i in range(2 * ns)]
    for k in range(1, N + 1):
        for j in range(2):
            rows += [(chk.INPUT, k, j, 1)] * fin(R['u_ub'][j]) + [(chk.INPUT, k, j, -1)] * fin(R['u_lb'][j])
    for k in range(1, N + 1):
        for i in range(nq):
            if i not in R['soft_idx']:
                rows += [(chk.STATE, k, i, 1)] * fin(R['q_ub'][i]) + [(chk.STATE, k, i, -1)] * fin(R['q_lb'][i])
    for s in range(ns):
        for k in range(1, N + 1):
            rows += [(chk.SOFT, k, s, 1), (chk.SOFT, k, s, -1)]
    if R['obs_r'] > 0:
        rows += [(chk.OBS, k, 0, 1) for k in range(1, N + 1)]
    return rows


def test_condensed_and_uncondensed_minimisers_agree_and_scaling_deviation(oracle, games):
    """The helper's condensed answer satisfies the uncondensed KKT conditions (asserted inside solve_iteration) and equals a direct
    KKT solve of the uncondensed QP on its active set; the reference's scaled QP (state_scaling / input_scaling) has the same minimiser up
    to the 1e-10 I term: the difference is printed."""
    P, rec, q0, u_ws, du_ws, q_ref = _cpu_case(games)
    R = chk.record_dict(rec, 6)
    dyn = chk.oracle_dyn(oracle, P, 0)
    N, nz = R['N'], 8
    D = np.concatenate((np.hstack((chk.rollout(dyn, q0, u_ws[1:]), u_ws)).ravel(), du_ws.ravel()))
    rows = _rows(R)
    h = chk.solve_iteration(oracle, R, float(P.dt), dyn, rows, D, q0, u_ws[0], q_ref, None)
    assert h['flag'] == 0 and h['strict'] and h['active'].any()
    qp = h['qp']
    act = np.nonzero(h['active'])[0]
    Aa = np.vstack((qp['A_eq'], h['Ad'][act]))
    K = np.block([[qp['H'], Aa.T], [Aa, np.zeros((Aa.shape[0],) * 2)]])
    sol = np.linalg.solve(K, np.concatenate((-qp['h'], qp['b_eq'], h['bd'][act])))
    assert chk.rel(sol[:qp['nD']], h['D_bar']) < 1e-9
    # scaled: x_scaled = T x; same active set, minimiser mapped back
    # (state scaling only: with input_scaling the reference leaves the rows u_{k+1} = u_k + dt du unscaled, CA_LTV_MPC.py:398-405, so its du --
    # rate cost and rate box with it -- is measured in scaled units: another problem, not a change of variables)
    sq, su = 1 / np.array([1, 1, 3.0, 0.5, 10.0, 0.5]), np.ones(2)
    qs = chk.uncondensed_qp(R, float(P.dt), dyn, D, q0, u_ws[0], q_ref, None, scale_q=sq, scale_u=su)
    As = np.vstack((qs['A_eq'], h['Ad'][act] / qs['scal'][None, :]))
    Ks = np.block([[qs['H'], As.T], [As, np.zeros((As.shape[0],) * 2)]])
    ss = np.linalg.solve(Ks, np.concatenate((-qs['h'], qs['b_eq'], h['bd'][act])))
    dev = chk.rel(ss[:qs['nD']] / qs['scal'], h['D_bar'])
    print(f'scaling deviation of the minimiser (relative): {dev:.3e}')
    assert dev < 1e-6
