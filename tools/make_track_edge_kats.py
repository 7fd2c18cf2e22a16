"""Known-answer vectors for games with TRACK-EDGE rows: tools/make_multistage_kats.py (imported; its defaults and its cases are untouched)
with ``rows()`` extended by the two rows per agent and stage of ``game.TrackEdges``, as plain 60-digit functions of the input sequence:

    right  -(w_R(sbar_k) - margin) - e_y,k        left  e_y,k - (w_L(sbar_k) - margin)          k = 1..N, after the agent's rate and lane rows
    w(sbar) = pw_lin(sbar, knots, widths),  sbar = fmod(fmod(s, L) + L, L)        (casadi_bspline_track.py:61-64)

pw_lin's slopes are doubles, as in ``track_fn``; the table sits in ``spec['track']['widths']`` ([n, 3]: knot, left, right) and an
agent's margin in ``ag['edges']`` (None: no rows).  Every evaluated s stays 1e-3 m from every knot of the table (the generator's Margin),
and the tool asserts that the stages of a case fall into at least two different pieces.  Writes tests/golden/multistage_<case>.npz.

    usage: python tools/make_track_edge_kats.py [--reference DIR] [--jobs J] [case ...]
"""
import argparse
import os
import pathlib
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_multistage_kats as base          # noqa: E402
from make_multistage_kats import F, INF, MARGIN, NQ      # noqa: E402

# four pieces on the curve track (L = 14), slopes between -0.25 and +0.25, left != right
TABLE = np.array([[0.0, 1.0, 0.8], [0.5, 0.9, 0.7], [1.1, 0.75, 0.85], [2.0, 0.95, 0.7], [14.0, 1.0, 0.8]])
EDGE_MARGIN = 0.05
CASES = ('kin2_edges_euler_N3', 'dyn2_edges_rk4m3_N3')


def widths(tr, s, mg):
    """(w_L, w_R) at s: pw_lin over the table on the wrapped s, the slopes doubles."""
    tab = np.asarray(tr['widths'], float)
    L = F(tr['L'])
    sbar = s - L * mp.floor(s / L)
    for kn in tab[:, 0]:
        mg.see(sbar - F(kn), f'knot of the width table s = {kn:g}')
    i = 0
    while i + 2 < len(tab) and sbar >= F(tab[i + 1, 0]):
        i += 1
    dk = tab[i + 1, 0] - tab[i, 0]
    return tuple(F(tab[i, c]) + F((tab[i + 1, c] - tab[i, c]) / dk) * (sbar - F(tab[i, 0])) for c in (1, 2))


def rows(spec, traj, ua, mg, up=None):
    """``make_multistage_kats.rows`` with the edge rows in their place (its text otherwise; DGSQP.py:730-821)."""
    up = base.zero_up(spec['M']) if up is None else up
    N, M = spec['N'], spec['M']
    dt = spec['dt']
    C = []
    for k in range(N + 1):
        if spec['obstacle_rows'] and k >= 1:
            for i in range(M):
                for j in range(i + 1, M):
                    r = F(spec['agents'][i]['radius'] + spec['agents'][j]['radius'])
                    C.append(r ** 2 - ((traj[i][k][0] - traj[j][k][0]) ** 2 + (traj[i][k][1] - traj[j][k][1]) ** 2))
        for a in range(M):
            ag = spec['agents'][a]
            if k < N and ag['rate'] is not None:
                um = ua[a][k - 1] if k > 0 else up[a]
                for j in range(2):
                    C.append((ua[a][k][j] - um[j]) - F(dt * ag['rate'][0][j]))
                    C.append(F(dt * ag['rate'][1][j]) - (ua[a][k][j] - um[j]))
            for ln in ag['lanes']:
                px, py = traj[a][k][0], traj[a][k][1]
                if ln['brk'] < INF:
                    mg.see(px - F(ln['brk']), 'brk of a lane normal')
                n = ln['n_lo'] if px < F(ln['brk']) else ln['n_hi']
                C.append(F(n[0]) * (px - (F(ln['anchor'][0]) - F(ln['r']) * F(n[0]))) + F(n[1]) * (py - (F(ln['anchor'][1]) - F(ln['r']) * F(n[1]))))
            if ag.get('edges') is not None and k >= 1:            # vertcat(right, left)
                nq = NQ[ag['model']]
                wL, wR = widths(spec['track'], traj[a][k][nq - 2], mg)
                ey, m = traj[a][k][nq - 1], F(ag['edges'])
                C.append(-(wR - m) - ey)
                C.append(ey - (wL - m))
            if k < N:
                C += [ua[a][k][j] - F(ag['in_ub'][j]) for j in range(2) if ag['in_ub'][j] < INF]
                C += [F(ag['in_lb'][j]) - ua[a][k][j] for j in range(2) if ag['in_lb'][j] > -INF]
            if k > 0:
                C += [traj[a][k][i] - F(ag['st_ub'][i]) for i in range(NQ[ag['model']]) if ag['st_ub'][i] < INF]
                C += [F(ag['st_lb'][i]) - traj[a][k][i] for i in range(NQ[ag['model']]) if ag['st_lb'][i] > -INF]
    return C


base.rows = rows          # GameMP.at and n_rows call the module's ``rows``; a spec without 'edges' / 'widths' gives the rows it always gave


def with_edges(spec, table, margin, box=False):
    """``spec`` racing on ``table``: the e_y box of every agent replaced by edge rows with ``margin`` -- or, ``box``: the box kept, no rows."""
    spec = dict(spec, track=dict(spec['track'], widths=np.asarray(table, float)), agents=[dict(ag) for ag in spec['agents']])
    for ag in spec['agents']:
        nq = NQ[ag['model']]
        if not box:
            ag['st_ub'], ag['st_lb'] = list(ag['st_ub']), list(ag['st_lb'])
            ag['st_ub'][nq - 1], ag['st_lb'][nq - 1] = INF, -INF
            ag['edges'] = float(margin)
    return spec


def edge_row_index(spec):
    """Positions of the edge rows in C (the order of ``rows``)."""
    marks, n = [], 0
    for k in range(spec['N'] + 1):
        if spec['obstacle_rows'] and k >= 1:
            n += spec['M'] * (spec['M'] - 1) // 2
        for ag in spec['agents']:
            n += (4 if (k < spec['N'] and ag['rate'] is not None) else 0) + len(ag['lanes'])
            if ag.get('edges') is not None and k >= 1:
                marks += [n, n + 1]
                n += 2
            if k < spec['N']:
                n += sum(v < INF for v in ag['in_ub']) + sum(v > -INF for v in ag['in_lb'])
            if k > 0:
                n += sum(v < INF for v in ag['st_ub']) + sum(v > -INF for v in ag['st_lb'])
    assert n == base.n_rows(spec)
    return marks


def flatten_spec(spec):
    out = base.flatten_spec(spec)
    for a, ag in enumerate(spec['agents']):
        out[f'p_a{a}_edge_margin'] = np.nan if ag.get('edges') is None else float(ag['edges'])
    return out


def case_inputs(case, defaults, shift=0):
    sys.path.insert(0, str(base.ROOT / 'tests'))
    sys.path.insert(0, str(base.ROOT))
    import track_width_checks as tw
    game = tw.build_edge_case(case)
    if case == 'kin2_edges_euler_N3':
        spec = with_edges(base.kinematic_game(defaults, base.curve_track(), 3), TABLE, EDGE_MARGIN)
        seed = 31
    elif case == 'dyn2_edges_rk4m3_N3':
        spec = with_edges(base.dynamic_game(defaults, 3, 'rk4', 3), TABLE, EDGE_MARGIN)
        seed = 32
    else:
        raise ValueError(case)
    x0, u, l = base.draw(case, game, 2, seed + 100 * shift, base.n_rows(spec))
    ie = edge_row_index(spec)
    l[:, ie] = 0.1 + np.abs(np.random.default_rng(seed + 7).standard_normal((len(x0), len(ie))))      # every edge row carries a multiplier

    def checks(x):
        nqa = x.shape[2] // 2
        s = x[:, 1:, [nqa - 2, 2 * nqa - 2]]
        kn = TABLE[:, 0]
        pieces = {int(p) for p in (np.searchsorted(kn, np.fmod(np.fmod(s, 14.0) + 14.0, 14.0), side='right') - 1).ravel()}
        assert len(pieces) >= 2, f'{case}: the stages fall into the pieces {sorted(pieces)} only'
        assert np.abs(np.fmod(np.fmod(s, 14.0) + 14.0, 14.0)[..., None] - kn).min() >= MARGIN
    return spec, x0, u, l, checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=None, help='the reference tree (for the defaults of DGSQP/dynamics/model_types.py)')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('cases', nargs='*', default=list(CASES))
    args = ap.parse_args()
    if args.reference is None:
        raise SystemExit('--reference DIR: the reference tree is needed for the vehicle defaults')
    defaults = base.reference_defaults(args.reference)
    with ProcessPoolExecutor(args.jobs) as pool:
        for case in args.cases:
            t = time.time()
            for shift in range(50):
                spec, x0, u, l, checks = case_inputs(case, defaults, shift)
                mp.mp.dps = 30
                gms = [base.GameMP(spec, x0[b], u[b], l[b], mp.mpf(0)) for b in range(len(x0))]
                if all(gm.at() and gm.mg.m > 1.1 * MARGIN for gm in gms):
                    try:
                        checks(np.array([[[float(e) for a in range(spec['M']) for e in gm.agent(a, (), 0)[0][k]] for k in range(spec['N'] + 1)] for gm in gms]))
                        break
                    except AssertionError as e:
                        print(f'{case}: seed shift {shift}: {e}, next', flush=True)
                        continue
                print(f'{case}: seed shift {shift} comes within {min(gm.mg.m for gm in gms):.2e} of a breakpoint, next', flush=True)
            else:
                raise SystemExit(f'{case}: no seed keeps the margin')
            out, acc, sens, margin = base.solve_case(spec, x0, u, l, (), True, pool)
            assert margin[0] > MARGIN, f'{case}: a state comes within {margin[0]:.2e} of a breakpoint ({margin[1]})'
            checks(out['x'].reshape(len(x0), spec['N'] + 1, -1))
            worst = max(acc.values())
            print(f'{case}: B {len(x0)}, n {u.shape[1]}, rows {l.shape[1]}, {time.time() - t:.1f} s, breakpoint margin {margin[0]:.3g} ({margin[1]}), '
                  f'accuracy record {worst:.1e}; sensitivity ' + ', '.join(f'{k} {v:.1e}' for k, v in sens.items()), flush=True)
            if worst > 1e-18:
                raise SystemExit(f'{case}: the 60- and the 90-digit answers disagree by {worst:.1e} > 1e-18, not written')
            data = dict(flatten_spec(spec), x0=x0, u=u, l=l, margin=margin[0], edge_rows=np.array(edge_row_index(spec)), **out)
            data.update({'acc_' + k: v for k, v in acc.items()})
            data.update({'sens_' + k: v for k, v in sens.items()})
            np.savez_compressed(base.GOLD / f'multistage_{case}.npz', **data)


if __name__ == '__main__':
    main()
