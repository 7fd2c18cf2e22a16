#!/usr/bin/env python3
"""The ``--game_type exact --dynamics_type dynamic --solver dgsqp`` leg of scripts/comparison_study_barc/monte_carlo_main.py on the MI355X
library: cars drawn around the raceline (monte_carlo_sampler_dynamic.py), warm-started by the LTV-MPC tracker following it
(warm_start_dynamic.py), the dynamic-bicycle game of exact_dynamic_game_dynamic.py solved by DG-SQP v2 (the study) or v1.  Sampling, warm
starts and the solve stay on the device (``sample_raceline_batch(stage=True)`` -> ``dgsqp_solve_staged``).  The script writes one
``sample_<i>.pkl`` = ``dict(solver_result=<solve() info>, initial_condition=<joint VehicleStates>)`` per sample (:110-117), the keys
analyze_data.py reads (``solver_result['msg' | 'time' | 'num_iters']``, ``initial_condition``), and so does this driver.

    python examples/monte_carlo_barc_dynamic.py --num-mc 1024 --out /tmp/barc_dynamic
    python examples/monte_carlo_barc_dynamic.py --front-end circuit        # the PID front end of DGSQP_comp_monte_carlo.py, side by side
"""
import argparse
import ctypes
import pathlib
import time

import numpy as np

from _driver import ROOT, dump
from dgsqp_amd import _ffi
from dgsqp_amd.montecarlo import dynamic_racing_game, sample_scenarios
from dgsqp_amd.results import solve_infos
from dgsqp_amd.solver import DGSQP

FIXTURE = ROOT / 'tests' / 'golden' / 'L_track_barc_raceline.npz'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-mc', type=int, default=100, help='samples (monte_carlo_main.py --samples)')
    ap.add_argument('--N', type=int, default=25, help='horizon')
    ap.add_argument('--solver', choices=('v1', 'v2'), default='v2', help='DG-SQP v2 (the study, globals.py:27-55) or v1')
    ap.add_argument('--front-end', choices=('circuit', 'raceline'), default='raceline',
                    help="'raceline': the study's sampler and tracker warm starts; 'circuit': DGSQP_comp_monte_carlo.py's sampler with PID warm starts")
    ap.add_argument('--raceline', default=str(FIXTURE), help="the study's L_track_barc_raceline.npz")
    ap.add_argument('--seed', type=int, default=0, help='seed of the counter-based sampler (the script seeds its generator with 0)')
    ap.add_argument('--rk4-substeps', type=int, default=10, help='globals.py:18: M = 10')
    ap.add_argument('--host-sampler', action='store_true',
                    help="the script's own sequential np.random.default_rng(seed) draws (montecarlo.sample_scenarios) instead of the counter-based device sampler")
    ap.add_argument('--out', default=None, help='directory of the sample_<i>.pkl files')
    args = ap.parse_args(argv)
    raceline = args.front_end == 'raceline'
    game = dynamic_racing_game(track_kind='barc', N=args.N, rk4_substeps=args.rk4_substeps, solver=args.solver,
                               sampler=args.front_end, raceline=args.raceline if raceline else None)
    solver = DGSQP(*game.solver_args(), print_method=None)
    B = args.num_mc
    t0 = time.time()
    if args.host_sampler:
        x0, u_ws = sample_scenarios(game, B, seed=args.seed, solver=solver if raceline else None)      # (the tracker's warm starts still run on the device)
        x0, u_am = np.ascontiguousarray(x0), np.ascontiguousarray(solver._to_agent_major(u_ws))
        if solver._lib.dgsqp_stage_inputs(solver._h, B, _ffi.dptr(x0), _ffi.dptr(u_am)) != 0:
            raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
        smp = dict(x0=x0, u_ws=u_ws, candidates=float('nan'))
    else:
        smp = (solver.sample_raceline_batch if raceline else solver.sample_batch)(game, B, seed=args.seed, stage=True)
    t1 = time.time()
    tm = _ffi.TimingT()
    if solver._lib.dgsqp_solve_staged(solver._h, ctypes.byref(tm)) != 0:
        raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
    res = solver._records((B,))
    if solver._lib.dgsqp_fetch_results(solver._h, _ffi.dptr(res['u']), _ffi.dptr(res['l']), _ffi.dptr(res['x']), _ffi.iptr(res['status']),
                                       _ffi.iptr(res['num_iters']), _ffi.iptr(res['qp_solves']), _ffi.dptr(res['cond']), _ffi.dptr(res['cost'])) != 0:
        raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
    wall = time.time() - t1
    res['msg'] = [_ffi.STATUS_NAMES[int(s)] for s in res['status']]
    infos = solve_infos(res, wall)
    samples = [dict(solver_result=si, initial_condition=game.joint_model.qu2state(None, smp['x0'][b], np.zeros(game.joint_model.n_u)))
               for b, si in enumerate(infos)]
    conv = res['status'] <= 1
    print(f'{game.name} [{args.front_end} front end]: {B} samples; front end {t1 - t0:.2f} s ({smp["candidates"]} candidates, '
          f'{smp["candidates"] / B:.2f} per accepted), solve {wall:.2f} s ({B / max(wall, 1e-9):.0f} scenarios/s); converged {conv.mean():.3f}, '
          f'mean iterations (converged) {res["num_iters"][conv].mean() if conv.any() else float("nan"):.1f}, qp_fail {np.mean(res["status"] == 4):.3f}')
    if args.out:
        for i, s in enumerate(samples):
            dump(pathlib.Path(args.out) / f'sample_{i + 1}.pkl', s)
    return samples


if __name__ == '__main__':
    main()
