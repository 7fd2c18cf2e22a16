"""Accepted share of the F1 study's raceline front end on this project's dynamic F1 game (needs the GPU: the tracker runs there).

    python tools/f1_raceline_acceptance.py [--N 10] [--rk4-substeps 2] [--candidates 1024] [--seed 1] [--out profiles/f1_raceline_acceptance.txt]

For time_scale in {1, 1.5, 2} x s_range in {None, (60, 80)}: the first ``--candidates`` candidates of ``sampler.place_raceline`` through
``DGSQP.raceline_warm_start_batch`` with ``montecarlo.study_tracker``; a candidate is accepted when the two cars do not overlap and both
trackers report success.  Nobody has run the study's tracker on this game before: dt, tyres and mass are the BARC car's and the line's speeds
are 1.3 - 6.3 m/s at time_scale 1, above the tracker's v_long <= 5 box."""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FIXTURE = ROOT / 'tests' / 'golden' / 'f1_traj_race_cl.csv.gz'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10)
    ap.add_argument('--rk4-substeps', type=int, default=2)
    ap.add_argument('--candidates', type=int, default=1024)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from dgsqp_amd import montecarlo as mc, sampler as smp
    from dgsqp_amd.solver import DGSQP
    lines = [f'F1 raceline front end: accepted share of the first {a.candidates} candidates (seed {a.seed}); dynamic F1 game N = {a.N}, '
             f'rk4 sub-steps {a.rk4_substeps}; tracker montecarlo.study_tracker',
             f'{"time_scale":>10} {"s_range":>10} {"collide":>8} {"ws fails":>9} {"accepted":>9} {"share":>7}  line v_long (m/s)']
    for ts in (1.0, 1.5, 2.0):
        rl = mc.Raceline.from_tum(FIXTURE, 'f1_austin_tenth_scale', tenth_scale=True, time_scale=ts)
        for sr in (None, (60.0, 80.0)):
            g = mc.f1_racing_game(N=a.N, model='dynamic', rk4_substeps=a.rk4_substeps, sampler='raceline', raceline=rl, s_range=sr)
            s = DGSQP(*g.solver_args(), print_method=None)
            s.set_raceline(g.raceline)
            x0, margin = smp.place_raceline(g, a.seed, np.arange(a.candidates))
            out = s.raceline_warm_start_batch(x0, mc.raceline_ws(g))
            free = margin < 0
            acc = free & out['ok']
            v = rl.lap_mat[:, 3] if sr is None else rl.lap_mat[(rl.lap_mat[:, 7] >= sr[0]) & (rl.lap_mat[:, 7] <= sr[1] + 3 * mc.F1_STUDY_VL), 3]
            lines.append(f'{ts:>10.1f} {str(sr) if sr else "lap":>10} {int((~free).sum()):>8} {int((free & ~out["ok"]).sum()):>9} {int(acc.sum()):>9} '
                         f'{acc.mean():>7.3f}  {v.min():.2f} .. {v.max():.2f}')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
