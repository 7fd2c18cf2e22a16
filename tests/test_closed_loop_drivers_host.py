"""Drivers of closed-loop batches, the host side (no GPU): the two C-ABI entries (dgsqp_set_drivers, dgsqp_fetch_u_cmd) are declared,
exported by both builds and bound; dgsqp_drivers_t has one layout in C and in ctypes; closed_loop.pid_driver_step is, bit for bit, the
reference controller's mirror pid.PID / pid.PIDLaneFollower; closed_loop.drive selects per agent; closed_loop.Drivers refuses what the
library would refuse."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ('dgsqp_set_drivers', 'dgsqp_fetch_u_cmd')


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
        assert lib.dgsqp_set_drivers.argtypes[1] == ctypes.POINTER(_ffi.DriversT) and len(lib.dgsqp_set_drivers.argtypes) == 7
        assert len(lib.dgsqp_fetch_u_cmd.argtypes) == 3
    assert (_ffi.DRIVER_GAME, _ffi.DRIVER_PID, _ffi.DRIVER_REPLAY) == (0, 1, 2)
    for name, value in (('DGSQP_DRIVER_GAME', 0), ('DGSQP_DRIVER_PID', 1), ('DGSQP_DRIVER_REPLAY', 2)):
        assert re.search(rf'\b{name} = {value}\b', header), name


def test_drivers_struct_layout_matches_the_header(tmp_path):
    from dgsqp_amd import _ffi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(dgsqp_drivers_t), offsetof(dgsqp_drivers_t, kind), offsetof(dgsqp_drivers_t, pid), '
           'sizeof(((dgsqp_drivers_t*)0)->kind), sizeof(((dgsqp_drivers_t*)0)->pid[0]));return 0;}\n')
    exe = tmp_path / 'drivers_layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _ffi.DriversT
    assert got == [ctypes.sizeof(D), D.kind.offset, D.pid.offset, D.kind.size, ctypes.sizeof(_ffi.PidT)]
    assert D.kind.size == 4 * _ffi.MAX_AGENTS and D.pid.size == _ffi.MAX_AGENTS * ctypes.sizeof(_ffi.PidT)


def hand_made_sequence():
    """(v, e_y, e_psi) per step for refs (2.0, 0.1) and the gains below: built so that each of the four clamps is reached."""
    return np.array([
        [2.05, 0.11, 0.01],       # small errors: nothing saturates
        [2.03, 0.12, -0.02],
        [0.50, 0.90, 0.30],       # large speed error: speed RATE; large lateral error: steering RATE
        [0.50, 0.90, 0.30],
        [0.50, 0.90, 0.30],
        [0.50, 0.90, 0.30],       # ... until the steering MAGNITUDE is reached; the INTEGRATOR has hit its clamp on the way
        [0.50, 0.90, 0.30],
        [2.00, 0.10, 0.00],       # back on the reference: rate-limited return
        [2.10, -0.40, -0.20],
        [1.95, 0.05, 0.015],
    ])


def test_pid_driver_step_is_the_reference_controller_bit_for_bit():
    from dgsqp_amd.closed_loop import PidGains, new_pid_state, pid_driver_step
    from dgsqp_amd.pid import PID, PIDLaneFollower
    from dgsqp_amd.solver_types import PIDParams
    from dgsqp_amd.types import BodyLinearVelocity, ParametricPose, VehicleActuation, VehicleState
    dt, refs = 0.1, (2.0, 0.1)
    seq = hand_made_sequence()
    for ey_gain, nqa in ((5.0, 6), (5.0, 8), (3.0, 6)):
        g = PidGains(kp_v=1.5, kp_s=0.8, ki_s=0.4, ey_gain=ey_gain, ei_max=0.5, u_max=(2.1, 0.436), du_max=(0.9, 0.15))
        steer = PID(PIDParams(dt=dt, Kp=g.kp_s, Ki=g.ki_s, Kd=0, x_ref=0.0, int_e_max=g.ei_max, int_e_min=-g.ei_max, u_max=g.u_max[1], u_min=-g.u_max[1],
                              du_max=g.du_max[1], du_min=-g.du_max[1]))
        speed = PID(PIDParams(dt=dt, Kp=g.kp_v, Ki=0, Kd=0, x_ref=refs[0], u_max=g.u_max[0], u_min=-g.u_max[0], du_max=g.du_max[0], du_min=-g.du_max[0]))
        follower = None
        if ey_gain == 5.0:          # PIDLaneFollower's own error: 5 (x_tran - lat_ref) + e_psi
            follower = PIDLaneFollower(dt, PIDParams(dt=dt, Kp=g.kp_s, Ki=g.ki_s, x_ref=refs[1], int_e_max=g.ei_max, int_e_min=-g.ei_max, u_max=g.u_max[1],
                                                     u_min=-g.u_max[1], du_max=g.du_max[1], du_min=-g.du_max[1]),
                                       PIDParams(dt=dt, Kp=g.kp_v, x_ref=refs[0], u_max=g.u_max[0], u_min=-g.u_max[0], du_max=g.du_max[0], du_min=-g.du_max[0]))
        state = new_pid_state()
        reached = dict(steer_rate=0, steer_mag=0, speed_rate=0, integrator=0, free=0)
        for k, (v, ey, epsi) in enumerate(seq):
            q = np.zeros(nqa)
            q[2], q[5 if nqa == 8 else 3], q[-1] = v, epsi, ey
            prev = state.copy()
            u, new = pid_driver_step(g, q, refs, state, dt)
            assert np.array_equal(bits(state), bits(prev))                       # the state handed in is not changed
            state = new
            ua, _ = speed.solve(v)
            us, _ = steer.solve(ey_gain * (ey - refs[1]) + epsi)
            assert np.array_equal(bits(u), bits([ua, us])), (ey_gain, nqa, k, u, ua, us)
            assert np.array_equal(bits(state), bits([steer.ei, ua, us])), (ey_gain, nqa, k)
            if follower is not None:
                st = VehicleState(p=ParametricPose(x_tran=ey, e_psi=epsi), v=BodyLinearVelocity(v_long=v), u=VehicleActuation())
                follower.step(st)
                assert np.array_equal(bits(u), bits([st.u.u_a, st.u.u_steer])), (nqa, k)
            raw_s = -(g.kp_s * (ey_gain * (ey - refs[1]) + epsi) + g.ki_s * state[0])
            reached['steer_rate'] += int(abs(raw_s - prev[2]) > g.du_max[1] and abs(u[1] - prev[2]) == pytest.approx(g.du_max[1], rel=1e-12))
            reached['steer_mag'] += int(abs(u[1]) == g.u_max[1])
            reached['speed_rate'] += int(abs(-(g.kp_v * (v - refs[0])) - prev[1]) > g.du_max[0] and abs(u[0] - prev[1]) == pytest.approx(g.du_max[0], rel=1e-12))
            reached['integrator'] += int(abs(state[0]) == g.ei_max)
            reached['free'] += int(abs(raw_s - prev[2]) < g.du_max[1] and abs(u[1]) < g.u_max[1])
        assert all(n >= 1 for n in reached.values()), (ey_gain, nqa, reached)
    with pytest.raises(ValueError, match='e_y and e_psi'):
        pid_driver_step(PidGains(), np.zeros(4), refs, new_pid_state(), dt)


def test_drive_selects_per_agent():
    from dgsqp_amd.closed_loop import PidGains, drive, new_pid_state, pid_driver_step
    qoff = [0, 6, 14, 20]
    rng = np.random.default_rng(5)
    q = rng.standard_normal(20)
    u_game, u_rep = rng.standard_normal(6), rng.standard_normal(6)
    gains = [PidGains(), PidGains(kp_s=0.7, ki_s=0.2), PidGains()]
    refs = np.array([[1.0, 0.0], [2.0, 0.1], [3.0, -0.1]])
    states = new_pid_state((3,))
    states[1] = [0.01, 0.2, -0.05]
    before = states.copy()
    u, out = drive(['game', 'pid', 'replay'], u_game, q, gains, refs, states, 0.1, qoff, u_replay=u_rep)
    want, st1 = pid_driver_step(gains[1], q[6:14], refs[1], before[1], 0.1)
    assert np.array_equal(bits(u[0:2]), bits(u_game[0:2])) and np.array_equal(bits(u[2:4]), bits(want)) and np.array_equal(bits(u[4:6]), bits(u_rep[4:6]))
    assert np.array_equal(bits(out[1]), bits(st1)) and np.array_equal(bits(out[[0, 2]]), bits(before[[0, 2]]))
    assert np.array_equal(bits(states), bits(before))                            # the caller's array is not changed
    assert out[1, 0] != before[1, 0]
    u2, out2 = drive([0, 0, 0], u_game, q, gains, refs, states, 0.1, qoff)       # all game: the solution's stage 0, no state touched
    assert np.array_equal(bits(u2), bits(u_game)) and np.array_equal(bits(out2), bits(before))
    u3, _ = drive([1, 1, 2], u_game, q, gains, refs, states, 0.1, qoff, u_replay=u_rep)
    assert np.array_equal(bits(u3[0:2]), bits(pid_driver_step(gains[0], q[0:6], refs[0], before[0], 0.1)[0]))
    with pytest.raises(ValueError, match='u_replay'):
        drive([0, 2, 0], u_game, q, gains, refs, states, 0.1, qoff)
    with pytest.raises(ValueError, match='not recognized'):
        drive([0, 3, 0], u_game, q, gains, refs, states, 0.1, qoff)


def test_drivers_lowering_and_every_validation_error(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import Drivers, PidGains
    P, U = games['kb_curve_N10'][1], games['merge_N8'][1]
    M, B, T = int(P.M), 3, 2
    assert M == 2 and int(U.M) == 3 and U.agents[0].model == 2
    g1 = PidGains(kp_s=0.7, ki_s=0.2, du_max=(1.0, 0.05))
    rep = np.arange(B * T * 2 * M, dtype=float).reshape(B, T, 2 * M)
    d, kind, ref, u_rep = Drivers(kinds=['game', 'pid'], pid=[PidGains(), g1]).lower(P, B, T)
    assert isinstance(d, _ffi.DriversT) and kind is None and ref is None and u_rep is None
    assert list(d.kind)[:M] == [0, 1] and d.pid[1].kp_s == 0.7 and d.pid[1].ki_s == 0.2 and list(d.pid[1].du_max) == [1.0, 0.05]
    assert d.pid[0].ey_gain == 5.0 and d.pid[0].ei_max == 100.0 and list(d.pid[0].u_max) == [2.1, 0.436]
    d, kind, ref, u_rep = Drivers(per_chain_kinds=[[0, 0], ['pid', 2], [1, 'game']], refs=np.ones((B, M, 2)), u_replay=rep, pid=g1).lower(P, B, T)
    assert list(d.kind)[:M] == [0, 0] and kind.dtype == np.int32 and kind.tolist() == [[0, 0], [1, 2], [1, 0]]
    assert ref.shape == (B, M, 2) and ref.flags.c_contiguous and u_rep.shape == (T, B, 2 * M) and u_rep.flags.c_contiguous
    assert np.array_equal(u_rep[1, 2], rep[2, 1]) and d.pid[0].kp_s == 0.7 and d.pid[1].kp_s == 0.7
    assert list(Drivers().lower(P, B, T)[0].kind)[:M] == [0, 0]                   # the default: every agent plays the game
    refusals = [
        (Drivers(kinds=['game']), P, B, T, 'Number of agents'),
        (Drivers(kinds=['game', 'lane']), P, B, T, 'not recognized'),
        (Drivers(kinds=[0, 3]), P, B, T, 'not recognized'),
        (Drivers(kinds=[0, 0.5]), P, B, T, 'not recognized'),
        (Drivers(kinds=[0, 0], per_chain_kinds=[[0, 0]] * B + [[0, 0]]), P, B, T, r'\[B\]\[M\]'),
        (Drivers(per_chain_kinds=[[0, 0], [0, 7], [0, 0]]), P, B, T, 'not recognized'),
        (Drivers(kinds=['pid', 'game', 'game']), U, B, T, 'unicycle'),
        (Drivers(per_chain_kinds=[[0, 0, 0], [0, 0, 1], [0, 0, 0]]), U, B, T, 'unicycle'),
        (Drivers(kinds=['game', 'replay']), P, B, T, 'u_replay'),
        (Drivers(per_chain_kinds=[[0, 0], [0, 0], [2, 0]]), P, B, T, 'u_replay'),
        (Drivers(kinds=['game', 'replay'], u_replay=rep[:, :1]), P, B, T, 'u_replay must be'),
        (Drivers(kinds=['game', 'pid'], refs=np.ones((B, M))), P, B, T, 'refs must be'),
        (Drivers(kinds=['game', 'pid'], pid=[PidGains()]), P, B, T, 'PidGains'),
        (Drivers(kinds=['game', 'pid'], pid=[PidGains(), 1.0]), P, B, T, 'PidGains'),
        (Drivers(kinds=['game', 'pid']), P, B, 0, 'T must be'),
        (Drivers(kinds=['game', 'pid']), P, -1, T, 'negative'),
    ]
    for drivers, problem, b, t, word in refusals:
        with pytest.raises(ValueError, match=word):
            drivers.lower(problem, b, t)
    # replay entries of agents that are not on replay may be anything; a unicycle may replay and play
    assert Drivers(kinds=['replay', 'game', 'game'], u_replay=np.zeros((B, T, 6))).lower(U, B, T)[3].shape == (T, B, 6)
