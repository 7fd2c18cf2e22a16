"""The input before stage 0 (u_prev), the host side (no GPU): the three C-ABI entries (dgsqp_set_u_prev, dgsqp_set_closed_loop_u_prev,
dgsqp_fetch_u_prev) are declared, exported by both builds and bound; solver.coerce_u_prev and closed_loop.next_u_prev on hand-made
arrays; and the two known-answer fixtures multistage_<parent>_uprev.npz against their parents.

The fixture checks.  The answers of tools/make_multistage_kats.py are 60-digit values good to 1e-18 (the tool's acceptance, ``acc_*``); a
fixture stores each of them ROUNDED to fp64.  With p = u_prev, exact arithmetic gives: x, G, Q unchanged; the k = 0 rate rows of g changed
by -p_j (ub) and +p_j (lb), no other row; q changed by -w_rate[j] p_j in each agent's stage-0 columns, no other column.

* On the stored doubles: x, G, Q, every other g row and q column are held to 1e-17 of the array's largest entry (they are equal, or
  differ where two 60-digit runs round a value next to zero differently); the CHANGED entries of the stored g and q can only be held to the
  rounding of the two stored doubles and of the expected difference, one half ulp each (``_rounding``) -- a difference of two rounded
  numbers carries no more.
* On the generator's unrounded values (hi + lo, ~32 digits), every scenario: the same deltas to 1e-17 relative -- the tool's 1e-18
  plus one 60-digit operation --, and with u_prev = 0 the parent fixture's x, g, q (and G, Q for scenario 0 of each case) are reproduced to
  1e-17 (the stored doubles are the roundings of those values: every entry must be the fp64 nearest to the regenerated one)."""
import ctypes
import importlib.util
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLD = ROOT / 'tests' / 'golden'
NEW = ('dgsqp_set_u_prev', 'dgsqp_set_closed_loop_u_prev', 'dgsqp_fetch_u_prev')
PAIRS = ('kin2_rk4_N4', 'dyn2_rk4m3_N3')
REL = 1e-17


def test_the_three_symbols_are_declared_exported_and_bound():
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
        assert [len(getattr(lib, name).argtypes) for name in NEW] == [3, 4, 3]
        assert lib.dgsqp_set_u_prev.argtypes[1] == ctypes.c_int64 and lib.dgsqp_set_closed_loop_u_prev.argtypes[1] == ctypes.c_int


def test_coerce_u_prev_accepts_B_by_n_u_and_refuses_the_rest():
    from dgsqp_amd.solver import coerce_u_prev
    B, n_u = 3, 4
    p = np.arange(12, dtype=np.float32).reshape(B, n_u)
    out = coerce_u_prev(p[:, ::-1], B, n_u)              # neither fp64 nor contiguous
    assert out.dtype == np.float64 and out.flags['C_CONTIGUOUS'] and np.array_equal(out, p[:, ::-1])
    assert coerce_u_prev([[0.0, -0.0, 1.0, 2.0]] * 3, B, n_u).shape == (B, n_u)
    for bad in (np.zeros(n_u), np.zeros((B, n_u + 1)), np.zeros((B + 1, n_u)), np.zeros((B, 1, n_u)), np.zeros((n_u, B))):
        with pytest.raises(ValueError, match='u_prev must be'):
            coerce_u_prev(bad, B, n_u)
    for v in (np.nan, np.inf, -np.inf):
        p = np.zeros((B, n_u))
        p[2, 1] = v
        with pytest.raises(ValueError, match='not finite'):
            coerce_u_prev(p, B, n_u)


def test_next_u_prev_is_the_command_that_entered_the_plant():
    from dgsqp_amd.closed_loop import next_u_prev
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    u0 = np.array([[0.3, -0.0, 1.5, -0.2], [2.1, 0.436, -2.1, 1e-300]])
    got = next_u_prev(u0)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(u0))          # the sign of zero included
    got[0, 0] = 9.0
    assert u0[0, 0] == 0.3                                                           # a copy
    cmd = np.array([[0.3, -0.0, 0.7, 0.1], [2.1, 0.436, -1.0, 0.0]])                 # agent 1 is driven by something else
    assert np.array_equal(bits(next_u_prev(u0, cmd)), bits(cmd))
    assert np.array_equal(next_u_prev(u0[0], cmd[0]), cmd[0])                        # a single chain
    with pytest.raises(ValueError):
        next_u_prev(u0, cmd[:, :2])


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location('make_multistage_kats', ROOT / 'tools' / 'make_multistage_kats.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _pair(case):
    return np.load(GOLD / f'multistage_{case}.npz'), np.load(GOLD / f'multistage_{case}_uprev.npz')


def _layout(kat):
    """(stage-0 columns [M, 2], w_rate [M, 2], k = 0 rate rows [M, 2, 2] (ub, lb) or -1) from the fixture's parameters and the row order of
    DGSQP.py:730-821: at k = 0 no shared rows; per agent rate rows (ub, lb per channel), lane rows, input ub, input lb."""
    M, N = int(kat['p_M']), int(kat['p_N'])
    cols = np.array([[2 * N * a + j for j in range(2)] for a in range(M)])
    w = np.array([kat[f'p_a{a}_cost_input_rate_weight'] for a in range(M)], float)
    rate = -np.ones((M, 2, 2), int)
    r = 0
    for a in range(M):
        if int(kat[f'p_a{a}_has_rate']):
            for j in range(2):
                rate[a, j] = (r, r + 1)
                r += 2
        r += int(kat[f'p_a{a}_n_lane']) + int(np.isfinite(kat[f'p_a{a}_in_ub']).sum()) + int(np.isfinite(kat[f'p_a{a}_in_lb']).sum())
    return cols, w, rate


def _expected_deltas(kat, p):
    """(dg [n_c], dq [n]) that u_prev = p adds, in exact arithmetic."""
    cols, w, rate = _layout(kat)
    dg, dq = np.zeros(kat['g'].shape[1]), np.zeros(kat['q'].shape[1])
    for a in range(len(cols)):
        for j in range(2):
            dq[cols[a, j]] = -w[a, j] * p[2 * a + j]
            if rate[a, j, 0] >= 0:
                dg[rate[a, j, 0]], dg[rate[a, j, 1]] = -p[2 * a + j], p[2 * a + j]
    return dg, dq


def _rounding(*terms):
    """Half an ulp of each stored double that enters a difference."""
    return sum(0.5 * np.spacing(np.abs(t)) for t in terms)


@pytest.mark.parametrize('case', PAIRS)
def test_uprev_fixture_differs_from_its_parent_in_the_stage_0_rate_terms_only(case):
    par, up = _pair(case)
    for k in ('x0', 'u', 'l'):
        assert np.array_equal(par[k], up[k]), k                                      # the parent's scenarios
    for k in [k for k in par.files if k.startswith('p_')]:
        assert np.array_equal(par[k], up[k]), k                                      # ... and game
    p = up['u_prev']
    B = len(par['x0'])
    M = int(par['p_M'])
    assert p.shape == (B, 2 * M) and np.isfinite(p).all() and (p != 0).all()
    lb = np.concatenate([par[f'p_a{a}_in_lb'] for a in range(M)])
    ub = np.concatenate([par[f'p_a{a}_in_ub'] for a in range(M)])
    assert ((p > lb) & (p < ub)).all()                                               # inside the input box
    for k in up.files:
        if k.startswith('acc_'):
            assert up[k] <= 1e-18, (k, float(up[k]))
    assert up['margin'] > 1e-3
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for k in ('x', 'G', 'Q'):
        print(f'{case} {k}: stored doubles differ by {rel(up[k], par[k]):.1e} of the largest entry')
        assert rel(up[k], par[k]) <= REL, k
    cols, w, rate = _layout(par)
    touched_q = np.zeros(par['q'].shape[1], bool)
    touched_q[cols[w != 0]] = True
    touched_g = np.zeros(par['g'].shape[1], bool)
    touched_g[rate[rate >= 0]] = True
    assert touched_q.sum() == 2 * M and touched_g.sum() == (4 * M if int(par['p_a0_has_rate']) else 0)
    assert rel(up['g'][:, ~touched_g], par['g'][:, ~touched_g]) <= REL and rel(up['q'][:, ~touched_q], par['q'][:, ~touched_q]) <= REL
    for b in range(B):
        dg, dq = _expected_deltas(par, p[b])
        for key, d, touched in (('g', dg, touched_g), ('q', dq, touched_q)):
            got = up[key][b] - par[key][b]
            tol = _rounding(up[key][b], par[key][b], d)
            print(f'{case} scenario {b} {key}: changed entries off the exact delta by at most {np.abs(got - d)[touched].max() if touched.any() else 0.0:.1e} '
                  f'(rounding of the stored doubles allows {tol[touched].max() if touched.any() else 0.0:.1e})')
            assert (np.abs(got - d)[touched] <= tol[touched]).all(), (key, b)
            assert (got[touched] != 0).all(), (key, b)                                # ... and they did change


@pytest.mark.parametrize('case', PAIRS)
def test_generator_reproduces_the_parent_with_zero_u_prev_and_the_exact_deltas_with_one(case):
    """Every scenario of each pair from the generator itself, the game rebuilt from the parent fixture's own parameters
    (``unflatten_spec``).  Scenario 0 runs the whole answer, G and Q included; scenarios 1 and 2 run x, g, q (a full answer takes seconds,
    and the deltas live in g and q)."""
    gen = _generator()
    par, up = _pair(case)
    spec = gen.unflatten_spec(par)
    assert all(np.array_equal(np.asarray(v), np.asarray(gen.flatten_spec(spec)[k])) for k, v in ((k, par[k]) for k in par.files if k.startswith('p_')))
    val = lambda a: a[0].astype(np.longdouble) + a[1].astype(np.longdouble)           # hi + lo
    for b in range(len(par['x0'])):
        full = b == 0
        p = up['u_prev'][b]
        zero, margin = gen.answers(spec, par['x0'][b], par['u'][b], par['l'][b], 60, 20, full=full, up=np.zeros_like(p))
        assert margin[0] > gen.MARGIN
        for k in ('x', 'g', 'q') + (('G', 'Q') if full else ()):
            want = par[k][b].reshape(zero[k][0].shape)
            err = float(np.abs(val(zero[k]) - want).max() / np.abs(want).max())
            print(f'{case} scenario {b} {k}: parent fixture against the regenerated value, {err:.1e} of the largest entry (one fp64 rounding: 1.1e-16)')
            assert np.array_equal(zero[k][0], want) or float(np.abs(zero[k][0] - want).max() / np.abs(want).max()) <= REL, (b, k)
        with_p, _ = gen.answers(spec, par['x0'][b], par['u'][b], par['l'][b], 60, 20, full=False, up=p)
        dg, dq = _expected_deltas(par, p)
        assert float(np.abs(val(with_p['x']) - val(zero['x'])).max()) == 0.0
        for k, d in (('g', dg), ('q', dq)):
            got = val(with_p[k]) - val(zero[k])
            err = float(np.abs(got - d.astype(np.longdouble)).max() / np.abs(val(zero[k])).max())
            print(f'{case} scenario {b} {k}: delta of the unrounded answers off the exact one by {err:.1e} of the largest entry (bar {REL:g})')
            assert err <= REL, (b, k, err)
