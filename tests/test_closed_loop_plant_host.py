"""A plant of its own for closed-loop batches (closed_loop.PlantModel / dgsqp_set_plant), the parts that need no GPU: the new symbols are
declared, exported by both builds and bound; the ctypes mirror of dgsqp_plant_t has the header's layout; the host mirror of the plant's
feedback rule (closed_loop.plant_feedback) is the delay rule of the reference's simulator (dynamics_simulator.py:33-40); PlantModel refuses
what the library would refuse."""
import copy
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_symbols_are_declared_exported_by_both_builds_and_bound():
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc import build
    text = (ROOT / 'include' / 'dgsqp.h').read_text()
    assert re.search(r'int\s+dgsqp_set_plant\s*\(\s*dgsqp_handle_t\s+h\s*,\s*const\s+dgsqp_plant_t\s*\*\s*plant\s*\)\s*;', text)
    assert re.search(r'int\s+dgsqp_fetch_u_plant\s*\(\s*dgsqp_handle_t\s+h\s*,\s*double\s*\*\s*out\s*,\s*int64_t\s+capacity_doubles\s*\)\s*;', text)
    m = re.search(r'#define\s+DGSQP_MAX_DELAY\s+(\d+)', text)
    assert m and int(m.group(1)) == _ffi.MAX_DELAY >= 16
    build.build()
    for wg in (1, 2):
        raw = ctypes.CDLL(str(_ffi.library_path(wg)))                     # loads without a GPU
        bound = _ffi.load_library(wg)
        for name, n_args in (('dgsqp_set_plant', 2), ('dgsqp_fetch_u_plant', 3)):
            assert name in _ffi.EXPORTED_SYMBOLS and getattr(raw, name) is not None
            fn = getattr(bound, name)
            assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int
    # the signature of the launch itself has not changed
    args = re.search(r'int\s+dgsqp_closed_loop_batch\s*\((.*?)\)\s*;', text, re.S).group(1)
    assert len([a for a in re.sub(r'/\*.*?\*/', '', args, flags=re.S).split(',') if a.strip()]) == 18 == len(_ffi.SIGNATURES['dgsqp_closed_loop_batch'][1])


def test_plant_struct_layout_matches_the_header(tmp_path):
    """Size and the offset of every field of dgsqp_plant_t, from a tiny C program."""
    from dgsqp_amd import _ffi
    fields = [name for name, _ in _ffi.PlantT._fields_]
    assert fields == ['integrator', 'substeps', 'sim_steps', 'use_game_agents', 'delay', 'agents']
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\nint main(){printf("%zu %zu %zu"' +
           ''.join(' " %zu"' for _ in fields) + ', sizeof(dgsqp_plant_t), sizeof(((dgsqp_plant_t*)0)->delay), sizeof(((dgsqp_plant_t*)0)->delay[0])' +
           ''.join(f', offsetof(dgsqp_plant_t, {f})' for f in fields) + ');return 0;}\n')
    exe = tmp_path / 'dgsqp_plant_layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(_ffi.PlantT)
    assert got[1] == 4 * _ffi.MAX_AGENTS * _ffi.NUA and got[2] == 4 * _ffi.NUA            # delay[agent][channel], int32
    assert got[3:] == [getattr(_ffi.PlantT, f).offset for f in fields]
    pt = _ffi.PlantT()
    pt.delay[3][1] = 7                                                                      # ... and ctypes indexes it the same way
    assert np.frombuffer(bytes(pt), np.int32, count=4 + 2 * _ffi.MAX_AGENTS)[4 + 3 * 2 + 1] == 7


def _toy_fd(q, u):
    """One 'simulation step' that makes every input and every step visible in the state: q <- 2 q + sum of the inputs, last state counts."""
    q = np.asarray(q, float)
    out = 2.0 * q
    out[..., 0] += u[..., 0] + 10.0 * u[..., 1]
    out[..., -1] = q[..., -1] + 1.0
    return out


def test_plant_feedback_on_hand_made_arrays():
    from dgsqp_amd import closed_loop
    # one scenario, two channels: channel 0 delayed by d = 3 simulation steps, channel 1 not delayed; S = 2 steps per control step
    lines = closed_loop.new_lines([3, 0])
    assert [ln.shape for ln in lines] == [(3,), (0,)] and not lines[0].any()
    q = np.array([0.0, 0.0])
    seen = []
    for t in range(4):
        u_new = np.array([1.0 + t, 100.0 + t])
        q, used, ok = closed_loop.plant_feedback(_toy_fd, q, u_new, lines, sim_steps=2)
        assert used.shape == (2, 2) and bool(ok) is True
        seen.append(used)
    seen = np.concatenate(seen)                                             # [8 simulation steps, 2 channels]
    # the line delivers zeros for its first d = 3 simulation steps, then the inputs in the order they were appended (each twice: S = 2);
    # it persists across control steps: steps 3, 4 of control steps 1, 2 see control step 0's input
    assert seen[:, 0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 2.0, 3.0]
    assert seen[:, 1].tolist() == [100.0, 100.0, 101.0, 101.0, 102.0, 102.0, 103.0, 103.0]      # d = 0 passes through
    assert lines[0].tolist() == [3.0, 4.0, 4.0]                            # oldest first
    assert q[-1] == 8.0                                                     # S steps were taken every time
    # the state saw exactly those inputs
    want = np.zeros(2)
    for u in seen:
        want = _toy_fd(want, u)
    assert np.array_equal(q, want)
    # batched, with a disturbance and a non-finite state; every scenario has lines of its own
    B = 3
    lines = closed_loop.new_lines([[1, 2], [0, 1]], lead=(B,))
    assert [ln.shape for ln in lines] == [(B, 1), (B, 2), (B, 0), (B, 1)]
    u_new = np.arange(1.0, 1.0 + B * 4).reshape(B, 4)
    w = np.zeros((B, 3))
    w[1, 1] = np.inf
    q1, used, ok = closed_loop.plant_feedback(lambda q, u: q + u[..., :3], np.zeros((B, 3)), u_new, lines, sim_steps=3, w=w)
    assert used.shape == (B, 3, 4) and ok.tolist() == [True, False, True]
    for b in range(B):
        assert used[b, :, 0].tolist() == [0.0, u_new[b, 0], u_new[b, 0]]
        assert used[b, :, 1].tolist() == [0.0, 0.0, u_new[b, 1]]
        assert used[b, :, 2].tolist() == [u_new[b, 2]] * 3
        assert used[b, :, 3].tolist() == [0.0, u_new[b, 3], u_new[b, 3]]
        assert np.array_equal(lines[1][b], [u_new[b, 1]] * 2)
    assert np.array_equal(q1[0], used[0].sum(axis=0)[:3]) and np.isinf(q1[1, 1])
    with pytest.raises(ValueError):
        closed_loop.plant_feedback(_toy_fd, np.zeros(2), np.zeros(2), closed_loop.new_lines([1]))


def test_plant_feedback_is_the_simulators_deque():
    """The rule of dynamics_simulator.py:33-40 written with its own deque, against plant_feedback, on random inputs."""
    from collections import deque
    from dgsqp_amd import closed_loop
    rng = np.random.default_rng(7)
    d, S = [2, 5, 1], 3
    buf = [deque([0 for _ in range(n)], maxlen=n) for n in d]
    lines = closed_loop.new_lines(d)
    for _ in range(6):
        u_new = rng.standard_normal(3)
        want = []
        for _ in range(S):
            want.append([buf[i][0] for i in range(3)])
            for i in range(3):
                buf[i].append(u_new[i])
        _, used, _ = closed_loop.plant_feedback(lambda q, u: q, np.zeros(1), u_new, lines, sim_steps=S)
        assert np.array_equal(used, np.array(want))


def test_plant_model_validation(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel
    from dgsqp_amd.dynamics import DynamicBicycleConfig, KinematicBicycleConfig, UnicycleConfig
    g, P, _ = games['kb_curve_N10']
    cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
    # the default plant is the game's model
    pt = PlantModel().lower(P)
    assert (pt.integrator, pt.substeps, pt.sim_steps, pt.use_game_agents) == (P.integrator, P.substeps, 1, 1)
    assert not np.frombuffer(bytes(pt), np.int32, count=4 + 2 * _ffi.MAX_AGENTS)[4:].any()
    # own parameters go through the code build_problem uses: the game's own configs give the game's own vehicle fields
    pt = PlantModel(dynamics_configs=cfgs, method='rk4', M=3, sim_steps=2, delay_steps=[[2, 1], [0, 3]]).lower(P)
    assert (pt.integrator, pt.substeps, pt.sim_steps, pt.use_game_agents) == (1, 3, 2, 0)
    assert [[pt.delay[a][j] for j in range(2)] for a in range(2)] == [[2, 1], [0, 3]]
    vehicle = [name for name, _ in _ffi.AgentT._fields_][:22]
    assert vehicle[0] == 'model' and vehicle[-1] == 'lin_Br'
    for a in range(2):
        assert all(getattr(pt.agents[a], f) == getattr(P.agents[a], f) for f in vehicle), a
    cfgs[1].mass *= 1.2
    pt = PlantModel(dynamics_configs=cfgs).lower(P)
    assert pt.agents[1].mass == P.agents[1].mass * 1.2 and pt.agents[0].mass == P.agents[0].mass
    # what is refused
    with pytest.raises(ValueError, match='plant configs'):
        PlantModel(dynamics_configs=cfgs[:1]).lower(P)
    for other in (DynamicBicycleConfig(), UnicycleConfig()):
        with pytest.raises(ValueError, match='model class'):
            PlantModel(dynamics_configs=[cfgs[0], other]).lower(P)
    with pytest.raises(ValueError, match='model class'):
        PlantModel(dynamics_configs=[KinematicBicycleConfig()] * 3).lower(games['merge_N8'][1])
    for S in (0, -1, 1.5):
        with pytest.raises(ValueError, match='sim_steps'):
            PlantModel(sim_steps=S).lower(P)
    with pytest.raises(ValueError, match='M must be'):
        PlantModel(M=0).lower(P)
    with pytest.raises(ValueError, match='not recognized'):
        PlantModel(method='rk45').lower(P)
    for bad in (_ffi.MAX_DELAY + 1, [[0, 0], [0, -1]], 1.5):
        with pytest.raises(ValueError, match='delay'):
            PlantModel(delay_steps=bad).lower(P)
    assert PlantModel(delay_steps=_ffi.MAX_DELAY).lower(P).delay[1][1] == _ffi.MAX_DELAY
    with pytest.raises(ValueError, match='not both'):
        PlantModel(delay_steps=1, delay=0.1).lower(P)
    # seconds -> simulation steps as the reference's simulator does: int(d / model.dt), the simulation model's dt being dt / S
    dt = float(P.dt)
    for S in (1, 2, 3):
        sec = [[0.0, 0.05], [0.1, 0.26]]
        pt = PlantModel(sim_steps=S, delay=sec).lower(P)
        assert [[pt.delay[a][j] for j in range(2)] for a in range(2)] == [[int(d / (dt / S)) for d in row] for row in sec], S
    with pytest.raises(ValueError, match='delay'):
        PlantModel(sim_steps=4, delay=0.5).lower(P)                        # 20 simulation steps
