#!/usr/bin/env python3
"""Run the random sweeps of tests/test_device_math.py through two builds of the device-math probe -- the in-tree one and one built from
another revision of csrc/ -- and compare every output array bit by bit (needs a GPU).

    python tools/compare_math_probe.py --csrc DIR     # DIR: dgsqp_amd/csrc of a checkout of the other revision (a git worktree)
    python tools/compare_math_probe.py --lib FILE     # a probe library already built from it

Each library runs in a fresh child process (``DGSQP_MATH_PROBE_LIB`` selects it).  Points where both atan2 arguments are zero are
reported apart: there the two revisions are meant to differ (pi/2 before the fix, 0 after it).  Exit status 1 on any other difference."""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]


def dump(path):
    import device_math_probe as dmp
    import test_device_math as t
    from dgsqp_amd.montecarlo import kinematic_racing_game
    p = dmp.Probe(kinematic_racing_game('curve', N=3))
    out = {}

    def put(name, res):
        for j, a in enumerate(res if isinstance(res, tuple) else (res,)):
            out[f'{name}.{j}'] = a

    for chunk in range(t.CHUNKS):
        put(f'rcp{chunk}', p.run('rcp', t._rcp_inputs(chunk)))
        x, n_tan = t._sincos_inputs(chunk)
        for op in ('sincos', 'roll_sincos', 'roll_sin'):
            put(f'{op}{chunk}', p.run(op, x))
        put(f'tan{chunk}', p.run('tan', x[:n_tan]))
        x = t._atan_inputs(chunk)
        for op in ('atan', 'roll_atan'):
            put(f'{op}{chunk}', p.run(op, x))
        y, x = t._atan2_sweep(chunk)
        # ... and the axes and the origin, whole wavefronts of them (the fast path of roll_atan2) and mixed into the sweep
        y[:256:4], x[1:256:4] = 0.0, 0.0
        y[2:256:4], x[2:256:4] = 0.0, 0.0
        y[256:320], x[256:320] = 0.0, np.abs(x[256:320])
        y[320:384], x[320:384] = 0.0, 0.0
        for op in ('atan2', 'roll_atan2'):
            put(f'{op}{chunk}', p.run(op, y, x))
        out[f'atan2_origin{chunk}'] = (y == 0) & (x == 0)
        rng = np.random.default_rng(650 + chunk)
        jets = [rng.uniform(-4, 4, 4096) for _ in range(6)]
        put(f'ty_atan2{chunk}', p.run('ty_atan2', *jets))
    p.close()
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--csrc', help='directory with the other revision of dgsqp_amd/csrc')
    ap.add_argument('--lib', help='probe library built from the other revision')
    ap.add_argument('--dump', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    import device_math_probe as dmp
    here = dmp.build()
    with tempfile.TemporaryDirectory() as tmp:
        other = pathlib.Path(a.lib).resolve() if a.lib else dmp.build(force=True, csrc=pathlib.Path(a.csrc).resolve(), out=pathlib.Path(tmp) / 'other.so')
        res = []
        for tag, lib in (('tree', here), ('other', other)):
            f = pathlib.Path(tmp) / f'{tag}.npz'
            subprocess.check_call([sys.executable, __file__, '--dump', str(f)], env=dict(os.environ, DGSQP_MATH_PROBE_LIB=str(lib)))
            res.append(dict(np.load(f)))
    mine, theirs = res
    n = n_diff = n_origin = n_origin_diff = 0
    for k in sorted(mine):
        if k.startswith('atan2_origin'):
            continue
        a_, b_ = mine[k].view(np.int64), theirs[k].view(np.int64)
        origin = np.zeros(len(a_), dtype=bool)
        if 'atan2' in k and not k.startswith('ty_'):
            origin = mine['atan2_origin' + k.split('.')[0][-1]]
        d = (a_ != b_) & ~(np.isnan(mine[k]) & np.isnan(theirs[k]))
        n += int((~origin).sum()); n_diff += int((d & ~origin).sum())
        n_origin += int(origin.sum()); n_origin_diff += int((d & origin).sum())
        if (d & ~origin).any():
            i = int(np.flatnonzero(d & ~origin)[0])
            print(f'{k}: {int((d & ~origin).sum())} results differ, first at element {i}: {mine[k][i]!r} / {theirs[k][i]!r}')
        if origin.any():
            print(f'{k}: at (0, 0) this tree gives {sorted(set(mine[k][origin].tolist()))}, the other {sorted(set(theirs[k][origin].tolist()))}')
    print(f'{n} results away from atan2(0, 0): {n_diff} differ; {n_origin} at atan2(0, 0): {n_origin_diff} differ')
    return 1 if n_diff else 0


if __name__ == '__main__':
    sys.exit(main())
