#!/usr/bin/env python3
"""Front end of BASELINE configs[3]'s batch (kb_f1 N = 50, B = 16,384): the device sampler (``DGSQP.sample_batch``: placement on the spline,
PID warm starts, collision check, compaction -- nothing through the host) against the host sampler of the same tree
(``montecarlo.sample_scenarios``: a Python loop over ``track.local_to_global``, numpy PID warm starts).  Also ``global_to_local_batch`` on the
device for the TUM raceline's 2,721 poses and for 2^20 poses.  One process = one timing of each after a warm-up of each; one JSON line.

    python tools/spline_front_end_bench.py --B 16384 --N 50
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dgsqp_amd import montecarlo as mc, tracks                           # noqa: E402
from dgsqp_amd.solver import DGSQP                                      # noqa: E402


def timed(fn):
    fn()                                                    # warm-up: allocations, module load
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=16384)
    ap.add_argument('--N', type=int, default=50)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args(argv)
    game = mc.f1_racing_game(N=args.N)
    solver = DGSQP(*game.solver_args(), print_method=None)
    out = dict(game=game.name, B=args.B, N=args.N)
    out['device_sampler_ms'], r = timed(lambda: solver.sample_batch(game, args.B, seed=args.seed, fetch=False))
    out['device_sampler_candidates'] = r['candidates']
    out['device_sampler_fetch_ms'], _ = timed(lambda: solver.sample_batch(game, args.B, seed=args.seed))
    if not args.skip_host:
        mc.sample_scenarios(game, 256, seed=args.seed)              # (warm-up of the host path: a small batch, it has nothing to allocate)
        t0 = time.perf_counter()
        mc.sample_scenarios(game, args.B, seed=args.seed)
        out['host_sampler_ms'] = 1e3 * (time.perf_counter() - t0)
        out['speedup'] = out['host_sampler_ms'] / out['device_sampler_fetch_ms']
    rl = mc.Raceline.from_tum(ROOT / 'tests' / 'golden' / 'f1_traj_race_cl.csv.gz', 'f1_austin_tenth_scale', tenth_scale=True)
    xy = np.ascontiguousarray(rl.lap_mat[:, :3])
    out['g2l_2721_device_ms'], dev = timed(lambda: solver.global_to_local_batch(xy))
    out['g2l_2721_mirror_ms'], mir = timed(lambda: tracks.global_to_local_batch(game.track, xy))
    out['g2l_2721_max_diff'] = float(np.abs(dev[0][:, :2] - mir[0][:, :2]).max())
    rng = np.random.default_rng(0)
    n = 1 << 20
    cl = np.stack([rng.random(n) * game.track.track_length, (2 * rng.random(n) - 1) * game.track.half_width, rng.random(n) - 0.5], axis=1)
    big = tracks.local_to_global_batch(game.track, cl)
    out['l2g_1M_device_ms'], _ = timed(lambda: solver.local_to_global_batch(cl))
    out['g2l_1M_device_ms'], dev = timed(lambda: solver.global_to_local_batch(big))
    ds = np.abs(dev[0][:, 0] - cl[:, 0])
    far = np.minimum(ds, game.track.track_length - ds) > 1e-6           # (the start line's kink: a point there may be named by its other foot point)
    out['g2l_1M_status0'] = int((dev[2] == 0).sum())
    out['g2l_1M_max_ds'] = float(np.minimum(ds, game.track.track_length - ds)[~far].max())
    out['g2l_1M_other_foot_point'] = int(far.sum())
    out['g2l_1M_max_resid'] = float(np.abs(dev[1]).max())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
