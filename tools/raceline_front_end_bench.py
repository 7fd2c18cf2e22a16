#!/usr/bin/env python3
"""Front end of the BARC study, B accepted scenarios at horizon N: the device program (``DGSQP.sample_raceline_batch``: placement, reference
trajectories, the tracker's two phases per car, assembly, compaction -- nothing through the host) against the HOST-LOOP composition of the
same tree (placement and references in numpy, one ``CA_LTV_MPC.solve_batch`` per car and phase with host copies in between, the mirror's
rounds).  One process = one timing of each, after a warm-up of each; prints one JSON line.

    python tools/raceline_front_end_bench.py --B 1024 --N 25
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dgsqp_amd import montecarlo as mc, sampler as smp                  # noqa: E402
from dgsqp_amd.ltv_mpc import CA_LTV_MPC                                # noqa: E402
from dgsqp_amd.solver import DGSQP                                      # noqa: E402


def host_loop_sampler(game, mpc, tracker, B, seed):
    """The mirror's rounds with every piece composed on the host: numpy placement and q_ref, two solve_batch calls per car."""
    N, dt = game.params.N, game.params.dt
    nround = max(256, min(2 * B, 1 << 16))
    Tu = 1.0 / np.asarray(tracker['params'].input_scaling, np.float64)
    x0s, uws, have, c0 = [], [], 0, 0
    while have < B:
        x0, margin = smp.place_raceline(game, seed, np.arange(c0, c0 + nround, dtype=np.uint64))
        ok = margin < 0
        us = []
        for a in range(2):
            q0 = np.ascontiguousarray(x0[:, 8 * a:8 * a + 8])
            q_ref = game.raceline.q_ref(q0, N, dt)
            u_ws, du_ws = np.full((nround, N + 1, 2), tracker['u_init']), np.full((nround, N, 2), tracker['du_init']) * Tu
            p1 = mpc.solve_batch(q0, u_ws, du_ws, q_ref, qp_iters=tracker['init_iters'], damping=tracker['init_damping'], zero_du=True)
            p2 = mpc.solve_batch(q0, np.concatenate((u_ws[:, :1], p1['u_pred']), axis=1), p1['du_pred'], q_ref)
            ok &= p2['status'] == 0
            us.append(p2['u_pred'])
        take = np.nonzero(ok)[0][:B - have]
        x0s.append(x0[take]); uws.append(np.concatenate(us, axis=2)[take])
        have += len(take)
        used = c0 + int(take[-1]) + 1 if len(take) else c0
        c0 += nround
    return np.concatenate(x0s), np.concatenate(uws), used


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1024)
    ap.add_argument('--N', type=int, default=25)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--raceline', default=str(ROOT / 'tests' / 'golden' / 'L_track_barc_raceline.npz'))
    args = ap.parse_args(argv)
    game = mc.dynamic_racing_game(track_kind='barc', N=args.N, sampler='raceline', raceline=args.raceline)
    solver = DGSQP(*game.solver_args(), print_method=None)
    tracker = mc.study_tracker(game)
    mpc = CA_LTV_MPC(game.joint_model.dynamics_models[0], tracker['cost'], None, tracker['bounds'], tracker['params'], print_method=None)
    out = {}
    for name, fn in (('device_program', lambda: solver.sample_raceline_batch(game, args.B, seed=args.seed, fetch=False)),
                     ('host_loop', lambda: host_loop_sampler(game, mpc, tracker, args.B, args.seed))):
        fn()                                                # warm-up: allocations, module load
        t0 = time.perf_counter()
        r = fn()
        out[name + '_ms'] = 1e3 * (time.perf_counter() - t0)
        out[name + '_candidates'] = int(r['candidates'] if isinstance(r, dict) else r[2])
    out.update(B=args.B, N=args.N, candidates_per_accepted=out['device_program_candidates'] / args.B,
               speedup=out['host_loop_ms'] / out['device_program_ms'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
