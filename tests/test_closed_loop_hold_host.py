"""Holding a plan across control steps, the host side (no GPU): the two C-ABI entries (dgsqp_set_plan_hold, dgsqp_fetch_plan_hold) are
declared, exported by both builds and bound; dgsqp_hold_t has one layout in C and in ctypes; closed_loop.PlanHold refuses what the library
would refuse; closed_loop.hold_step implements the table of include/dgsqp.h -- all four rows, for R = 1, 2, 3 --, is the reference's
warm-start rule (closed_loop.feedback) bit for bit at R = 1 / 'reference' / the default mask, and repeats the last row of a plan older than N
stages; step_batch refuses a hold of the wrong type before it touches the library."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ('dgsqp_set_plan_hold', 'dgsqp_fetch_plan_hold')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_both_symbols_are_declared_exported_and_bound():
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
        assert lib.dgsqp_set_plan_hold.argtypes[1] == ctypes.POINTER(_ffi.HoldT) and len(lib.dgsqp_set_plan_hold.argtypes) == 2
        assert len(lib.dgsqp_fetch_plan_hold.argtypes) == 4 and lib.dgsqp_fetch_plan_hold.argtypes[2] == ctypes.POINTER(ctypes.c_int32)
    for name, value in (('DGSQP_HELD', r'\(-2\)'), ('DGSQP_HOLD_REFERENCE', '0'), ('DGSQP_HOLD_HOLD', '1')):
        assert re.search(rf'#define\s+{name}\s+{value}\s', header), name
    assert (_ffi.HELD, _ffi.HOLD_REFERENCE, _ffi.HOLD_HOLD) == (-2, 0, 1)
    assert _ffi.STATUS_NAMES[_ffi.HELD] == 'held' and _ffi.STATUS_NAMES[_ffi.NOT_RUN] == 'not_run'
    assert [_ffi.STATUS_NAMES[s] for s in range(6)] == _ffi.STATUS_MSG


def test_hold_struct_layout_matches_the_header(tmp_path):
    from dgsqp_amd import _ffi
    fields = [name for name, _ in _ffi.HoldT._fields_]
    assert fields == ['replan_every', 'on_fail', 'fail_mask', 'reserved']
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\n'
           'int main(){printf("%zu", sizeof(dgsqp_hold_t));\n'
           + ''.join(f'printf(" %zu %zu", offsetof(dgsqp_hold_t, {f}), sizeof(((dgsqp_hold_t*)0)->{f}));\n' for f in fields)
           + 'dgsqp_hold_t h; h.fail_mask = 0; h.fail_mask -= 1; printf(" %d %d %d\\n", h.fail_mask > 0, DGSQP_DIVERGED, DGSQP_QP_FAIL);return 0;}\n')
    exe = tmp_path / 'hold_layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    H = _ffi.HoldT
    want = [ctypes.sizeof(H)] + [v for f in fields for v in (getattr(H, f).offset, getattr(H, f).size)]
    assert got[:-3] == want and ctypes.sizeof(H) == 16
    assert got[-3] == 1                                               # the mask is unsigned in C as in ctypes
    from dgsqp_amd import closed_loop
    assert closed_loop.REFERENCE_FAIL_MASK == (1 << got[-2]) | (1 << got[-1]) == 0b011000


def test_plan_hold_lowering_and_every_refusal(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlanHold
    P = games['kb_curve_N10'][1]
    N = int(P.N)
    h = PlanHold().lower(P)
    assert isinstance(h, _ffi.HoldT) and (h.replan_every, h.on_fail, h.fail_mask, h.reserved) == (1, 0, 0b011000, 0)
    h = PlanHold(replan_every=N, on_fail='hold', accept='converged').lower(P)
    assert (h.replan_every, h.on_fail, h.fail_mask) == (N, 1, 0b111100)               # statuses 2 .. 5
    assert PlanHold(accept='converged').mask == sum(1 << s for s in (2, 3, 4, 5))
    assert PlanHold(accept=0).lower(P).fail_mask == 0 and PlanHold(accept=63).lower(P).fail_mask == 63
    assert PlanHold(replan_every=np.int64(3)).lower(P).replan_every == 3
    for kw, word in ((dict(replan_every=0), 'replan_every'), (dict(replan_every=-1), 'replan_every'), (dict(replan_every=1.5), 'replan_every'),
                     (dict(replan_every=True), 'replan_every'), (dict(on_fail='keep'), 'on_fail'), (dict(on_fail=1), 'on_fail'),
                     (dict(accept='all'), 'accept'), (dict(accept=64), 'bits 0 .. 5'), (dict(accept=-1), 'bits 0 .. 5'), (dict(accept=1.5), 'bits 0 .. 5')):
        with pytest.raises(ValueError, match=word):
            PlanHold(**kw)
    with pytest.raises(ValueError, match=f'1 .. N = {N}'):
        PlanHold(replan_every=N + 1).lower(P)


NUM_UA = [2, 2]
N_ST = 4


def plan(seed):
    """A random agent-major vector [n] for two agents of two inputs and N_ST stages."""
    return np.random.default_rng(seed).standard_normal(N_ST * sum(NUM_UA))


def stage0(u):
    return np.concatenate([u[0:2], u[2 * N_ST:2 * N_ST + 2]])


@pytest.mark.parametrize('R', [1, 2, 3])
def test_hold_step_walks_all_four_rows_of_the_table(R):
    """A hand-made status sequence: accepted, (held ...), failed (qp_fail) twice, accepted, (held ...), failed (diverged), accepted.  Under
    'reference' a failure keeps the warm start and the state; under 'hold' it consumes one more stage and is retried."""
    from dgsqp_amd.closed_loop import PlanHold, hold_step, shift_warm_start
    shift = lambda u: shift_warm_start(u, N_ST, NUM_UA)
    for on_fail in ('reference', 'hold'):
        hold = PlanHold(replan_every=R, on_fail=on_fail)
        solved = iter([0, 4, 4, 1, 3, 0, 2, 0, 0, 0, 0, 0])            # the statuses of the solves, in the order they happen
        ws, age, due = plan(0), 0, True
        rows = set()
        for t in range(12):
            u_t = plan(100 + t)
            status = next(solved) if due else None
            before = (ws.copy(), age, due)
            u_game, ws_next, age2, due2, stage = hold_step(status, u_t if due else None, ws, age, due, hold, N_ST, NUM_UA)
            assert np.array_equal(bits(ws), bits(before[0]))                         # the caller's arrays are not changed
            if status is None:
                rows.add('held')
                assert not due and np.array_equal(bits(u_game), bits(stage0(ws))) and np.array_equal(bits(ws_next), bits(shift(ws)))
                assert (age2, due2, stage) == (age + 1, age + 1 >= R, age)
            elif status in (3, 4) and on_fail == 'reference':
                rows.add('reference')
                assert np.array_equal(bits(u_game), bits(stage0(u_t))) and np.array_equal(bits(ws_next), bits(ws))
                assert (age2, due2, stage) == (age, True, 0)
            elif status in (3, 4):
                rows.add('hold')
                assert np.array_equal(bits(u_game), bits(stage0(ws))) and np.array_equal(bits(ws_next), bits(shift(ws)))
                assert (age2, due2, stage) == (age + 1, True, age)
            else:
                rows.add('accepted')                                                  # (max_it, status 2, is accepted by the default mask)
                assert np.array_equal(bits(u_game), bits(stage0(u_t))) and np.array_equal(bits(ws_next), bits(shift(u_t)))
                assert (age2, due2, stage) == (1, 1 >= R, 0)
            ws, age, due = ws_next, age2, due2
        assert rows == ({'accepted', on_fail} | ({'held'} if R > 1 else set())), (R, on_fail, rows)
    # the state machine itself, spelled out for R = 3 with an accepted plan: solve, held, held, solve
    hold = PlanHold(replan_every=3)
    ws, age, due, seen = plan(1), 0, True, []
    for t in range(7):
        _, ws, age, due, stage = hold_step(0 if due else None, plan(t), ws, age, due, hold, N_ST, NUM_UA)
        seen.append((stage, age, due))
    assert seen == [(0, 1, False), (1, 2, False), (2, 3, True), (0, 1, False), (1, 2, False), (2, 3, True), (0, 1, False)]
    with pytest.raises(ValueError, match='due'):
        hold_step(None, None, ws, 0, True, hold, N_ST, NUM_UA)
    with pytest.raises(ValueError, match='due'):
        hold_step(0, plan(2), ws, 1, False, hold, N_ST, NUM_UA)


def test_mask_decides_what_fails():
    from dgsqp_amd.closed_loop import PlanHold, hold_step
    ws, u_t = plan(3), plan(4)
    for status in range(6):
        for accept, fails in (('reference', status in (3, 4)), ('converged', status >= 2), (0, False), (63, True), (1 << status, True)):
            u_game, _, age, due, stage = hold_step(status, u_t, ws, 2, True, PlanHold(replan_every=2, on_fail='hold', accept=accept), N_ST, NUM_UA)
            assert np.array_equal(bits(u_game), bits(stage0(ws if fails else u_t))), (status, accept)
            assert (age, due, stage) == ((3, True, 2) if fails else (1, False, 0)), (status, accept)


def test_default_hold_is_the_reference_warm_start_rule_bit_for_bit():
    from dgsqp_amd.closed_loop import PlanHold, feedback, hold_step
    rng = np.random.default_rng(11)
    N, num_ua = 5, [2, 2, 2]
    n, nq = N * 6, 7
    hold = PlanHold()
    for status in range(6):
        u, ws, x = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((N + 1, nq))
        u[3] = -0.0
        _, want, _ = feedback(x, u, np.int32(status), ws, num_ua_d=num_ua)
        u_game, got, age, due, stage = hold_step(status, u, ws, 0, True, hold, N, num_ua)
        assert np.array_equal(bits(got), bits(want)), status
        assert np.array_equal(bits(u_game), bits(np.concatenate([u[a * N * 2:a * N * 2 + 2] for a in range(3)]))) and stage == 0 and due
        assert age == (0 if status in (3, 4) else 1)


def test_a_plan_older_than_its_horizon_repeats_its_last_row():
    from dgsqp_amd.closed_loop import PlanHold, hold_step
    hold = PlanHold(replan_every=1, on_fail='hold', accept=63)              # nothing is ever accepted: the initial plan is consumed for ever
    ws0 = plan(7)
    ws, age, due = ws0, 0, True
    rows = lambda u, k: np.concatenate([u[2 * k:2 * k + 2], u[2 * N_ST + 2 * k:2 * N_ST + 2 * k + 2]])
    for t in range(N_ST + 3):
        u_game, ws, age, due, stage = hold_step(4, plan(50 + t), ws, age, due, hold, N_ST, NUM_UA)
        assert np.array_equal(bits(u_game), bits(rows(ws0, min(t, N_ST - 1)))), t
        assert (stage, age, due) == (t, t + 1, True)
    for k in range(N_ST):
        assert np.array_equal(bits(rows(ws, k)), bits(rows(ws0, N_ST - 1)))


def test_step_batch_refuses_a_hold_of_the_wrong_type_before_the_library():
    from dgsqp_amd import solver
    from dgsqp_amd.closed_loop import PlanHold
    s = solver.DGSQP.__new__(solver.DGSQP)
    s.N, s.n_q, s.num_ua_d, s._lib, s._h = 15, 12, [2, 2], None, None          # no handle, no library: anything beyond the check would raise otherwise
    x0, u_ws = np.zeros((2, 12)), np.zeros((2, 15, 4))
    for bad in (2, 'hold', dict(replan_every=2), PlanHold):
        with pytest.raises(TypeError, match='PlanHold'):
            s.step_batch(x0, u_ws, 2, hold=bad)
