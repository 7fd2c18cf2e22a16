"""Per-chain plants, state estimates and the safety monitor of closed-loop batches (dgsqp_set_plant_ensemble, dgsqp_set_estimate_noise,
dgsqp_set_monitor), the parts that need no GPU: the new symbols are declared, exported by both builds and bound; dgsqp_vehicle_t is the
vehicle prefix of dgsqp_agent_t; closed_loop.perturbed_configs draws an ensemble that does not depend on its size; closed_loop.monitor is
the documented formula on hand-made states; PlantModel refuses what the library would refuse."""
import copy
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

NEW = (('dgsqp_set_plant_ensemble', 4), ('dgsqp_set_estimate_noise', 4), ('dgsqp_fetch_q_est', 3), ('dgsqp_set_monitor', 2), ('dgsqp_fetch_monitor', 4))


def test_symbols_are_declared_exported_by_both_builds_and_bound():
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc import build
    text = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / 'dgsqp.h').read_text(), flags=re.S)
    for name, n_args in NEW:
        m = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', text, re.S)
        assert m, name
        assert len([a for a in m.group(1).split(',') if a.strip()]) == n_args, name
    build.build()
    for wg in (1, 2):
        raw = ctypes.CDLL(str(_ffi.library_path(wg)))                     # loads without a GPU
        bound = _ffi.load_library(wg)
        for name, n_args in NEW:
            assert name in _ffi.EXPORTED_SYMBOLS and getattr(raw, name) is not None
            fn = getattr(bound, name)
            assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int
    # what the earlier tests pin has not moved
    args = re.search(r'int\s+dgsqp_closed_loop_batch\s*\((.*?)\)\s*;', text, re.S).group(1)
    assert len([a for a in args.split(',') if a.strip()]) == 18 == len(_ffi.SIGNATURES['dgsqp_closed_loop_batch'][1])
    assert len(_ffi.SIGNATURES['dgsqp_set_plant'][1]) == 2 and len(_ffi.SIGNATURES['dgsqp_fetch_u_plant'][1]) == 3


def test_vehicle_struct_is_the_prefix_of_the_agent_struct(tmp_path):
    """Size and the offset of every field of dgsqp_vehicle_t, from a tiny C program, against AgentT's first 22 fields."""
    from dgsqp_amd import _ffi
    fields = [name for name, _ in _ffi.VehicleT._fields_]
    assert fields == [name for name, _ in _ffi.AgentT._fields_[:22]] and fields[0] == 'model' and fields[-1] == 'lin_Br'
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\nint main(){printf("%zu %zu"' + ''.join(' " %zu %zu"' for _ in fields) +
           ', sizeof(dgsqp_vehicle_t), offsetof(dgsqp_agent_t, w_in)' +
           ''.join(f', offsetof(dgsqp_vehicle_t, {f}), offsetof(dgsqp_agent_t, {f})' for f in fields) + ');return 0;}\n')
    exe = tmp_path / 'dgsqp_vehicle_layout'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == got[1] == ctypes.sizeof(_ffi.VehicleT) == 160
    want = [getattr(_ffi.AgentT, f).offset for f in fields]
    assert got[2::2] == want and got[3::2] == want and want == [getattr(_ffi.VehicleT, f).offset for f in fields]


SPREAD = dict(mass=0.1, drag_coefficient=0.2, wheel_dist_front=0.05)


def test_perturbed_configs(games):
    from dgsqp_amd import closed_loop, sampler
    g = games['kb_curve_N10'][0]
    cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
    before = copy.deepcopy(cfgs)
    few = closed_loop.perturbed_configs(cfgs, SPREAD, 4, seed=11)
    many = closed_loop.perturbed_configs(cfgs, SPREAD, 600, seed=11)
    again = closed_loop.perturbed_configs(cfgs, SPREAD, 4, seed=11)
    other = closed_loop.perturbed_configs(cfgs, SPREAD, 4, seed=12)
    assert len(few) == 4 and len(many) == 600 and all(len(row) == len(cfgs) for row in many)
    assert all(vars(c) == vars(c0) for c, c0 in zip(cfgs, before))                      # the nominal configs are left alone
    for b in range(4):
        for a in range(len(cfgs)):
            assert vars(few[b][a]) == vars(many[b][a]) == vars(again[b][a]), (b, a)      # reproducible; chain b does not depend on B
            assert any(getattr(few[b][a], f) != getattr(other[b][a], f) for f in SPREAD)
    seen = {f: [] for f in SPREAD}
    for b, row in enumerate(many):
        for a, c in enumerate(row):
            for i, (f, s) in enumerate(SPREAD.items()):
                nom, val = getattr(cfgs[a], f), getattr(c, f)
                assert nom * (1 - s) <= val <= nom * (1 + s), (b, a, f)
                U = float(sampler.uniform(11, np.array([b]), a * len(SPREAD) + i)[0])    # the documented key: (seed, chain, (agent, field))
                assert val == nom * (1.0 + s * (2.0 * U - 1.0))
                seen[f].append(val / nom - 1.0)
            untouched = [k for k in vars(c) if k not in SPREAD]
            assert all(getattr(c, k) == getattr(cfgs[a], k) for k in untouched)
    for f, s in SPREAD.items():                                                          # ... and the spread is used: both halves, near both ends
        assert min(seen[f]) < -0.9 * s and max(seen[f]) > 0.9 * s
    zero = closed_loop.perturbed_configs(cfgs, {f: 0.0 for f in SPREAD}, 3, seed=5)
    for row in zero:
        for a, c in enumerate(row):
            for f in SPREAD:
                assert np.float64(getattr(c, f)).tobytes() == np.float64(getattr(cfgs[a], f)).tobytes()      # the nominal, bit for bit
    with pytest.raises(ValueError, match='no field'):
        closed_loop.perturbed_configs(cfgs, dict(no_such_field=0.1), 2, seed=1)
    with pytest.raises(ValueError, match='half-width'):
        closed_loop.perturbed_configs(cfgs, dict(mass=1.5), 2, seed=1)


def test_monitor_on_hand_made_states():
    from dgsqp_amd.closed_loop import monitor
    inf = np.inf
    # two agents with three states each (x, y, v), S = 3 simulation steps; radii 0.5 and 0.25
    qoff, radii = [0, 3, 6], [0.5, 0.25]
    lb = np.array([-inf, -inf, 0.0, -inf, -inf, -inf])
    ub = np.array([inf, inf, 2.0, inf, inf, 1.0])
    z = np.array([[0.0, 0.0, 1.0, 3.0, 4.0, 0.5],           # distance 5
                  [0.0, 0.0, 1.5, 0.0, 2.0, 0.5],           # distance 2
                  [1.0, 1.0, 1.0, 4.0, 5.0, 0.25]])         # distance 5
    cl, bx, hit = monitor(z, radii, lb, ub, qoff)
    assert cl == 2.0 - 0.75 and bx == -0.5 and hit == -1      # closest to a bound: v_0 = 1.5 under its upper bound 2, v_1 = 0.5 under 1
    # one bound exceeded, from below and from above
    z2 = z.copy(); z2[2, 2] = -0.125
    assert monitor(z2, radii, lb, ub, qoff)[1] == 0.125
    z2 = z.copy(); z2[0, 5] = 1.75
    assert monitor(z2, radii, lb, ub, qoff)[1] == 0.75
    # a contact in simulation step 1 of 3: clearance < 0, first_hit = 1; the later steps do not hide it
    z3 = z.copy(); z3[1, 3:5] = [0.0, 0.5]
    cl, bx, hit = monitor(z3, radii, lb, ub, qoff)
    assert cl == 0.5 - 0.75 and hit == 1
    z3[0, 3:5] = [0.0, 0.75]                                  # touching exactly is no hit (clearance 0 is not < 0); step 1 still is the first
    assert monitor(z3, radii, lb, ub, qoff)[2] == 1 and monitor(z3[:1], radii, lb, ub, qoff)[2] == -1 and monitor(z3[:1], radii, lb, ub, qoff)[0] == 0.0
    # no finite bound at all
    assert monitor(z, radii, np.full(6, -inf), np.full(6, inf), qoff)[1] == -inf
    # M = 1
    cl, bx, hit = monitor(z[:, :3], [0.5], lb[:3], ub[:3], [0, 3])
    assert cl == inf and bx == -0.5 and hit == -1
    # a non-finite state anywhere: both NaN
    for bad in (np.nan, inf):
        z4 = z.copy(); z4[2, 4] = bad
        cl, bx, hit = monitor(z4, radii, lb, ub, qoff)
        assert np.isnan(cl) and np.isnan(bx)
    # batched, three agents: min over the three pairs; leading axes are kept
    zz = np.zeros((2, 4, 1, 6))
    zz[..., 0, :] = [0.0, 0.0, 3.0, 0.0, 0.0, 1.0]
    zz[1, 2, 0, 4:6] = [0.0, 0.5]
    cl, bx, hit = monitor(zz, [0.1, 0.1, 0.1], np.full(6, -inf), np.full(6, inf), [0, 2, 4, 6])
    assert cl.shape == bx.shape == hit.shape == (2, 4)
    want = np.full((2, 4), 1.0 - 0.2); want[1, 2] = 0.5 - 0.2
    assert np.array_equal(cl, want) and (hit == -1).all() and (bx == -inf).all()


def test_plant_model_validation_of_the_per_chain_fields(games):
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import PlantModel, perturbed_configs
    from dgsqp_amd.dynamics import DynamicBicycleConfig
    g, P, _ = games['kb_curve_N10']
    cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
    B = 3
    ens = perturbed_configs(cfgs, dict(mass=0.1), B, seed=3)
    assert not PlantModel().per_chain and PlantModel(per_chain_configs=ens).per_chain and PlantModel(per_chain_delay_steps=np.zeros((B, 2, 2))).per_chain
    veh, delay = PlantModel(per_chain_configs=ens).lower_ensemble(P, B)
    assert len(veh) == B * 2 and delay is None and ctypes.sizeof(veh) == B * 2 * 160
    names = [n for n, _ in _ffi.VehicleT._fields_]
    for b in range(B):
        for a in range(2):
            assert veh[b * 2 + a].mass == ens[b][a].mass and veh[b * 2 + a].model == P.agents[a].model
            assert all(getattr(veh[b * 2 + a], f) == getattr(P.agents[a], f) for f in names if f != 'mass')
    # delays: [B][M][2] simulation steps, or seconds converted as `delay`
    d = np.arange(B * 4).reshape(B, 2, 2) % 5
    veh, delay = PlantModel(per_chain_configs=ens, per_chain_delay_steps=d).lower_ensemble(P, B)
    assert delay.dtype == np.int32 and delay.flags.c_contiguous and np.array_equal(delay, d)
    dt = float(P.dt)
    sec = np.array([[[0.0, 0.05], [0.1, 0.26]]] * B)
    for S in (1, 2):
        _, delay = PlantModel(sim_steps=S, per_chain_delay=sec).lower_ensemble(P, B)
        assert delay.tolist() == [[[int(v / (dt / S)) for v in row] for row in sec[0]]] * B
    # per-chain delays alone: every chain has the shared plant's vehicles (its own configs, or the game's)
    heavy = copy.deepcopy(cfgs); heavy[1].mass *= 1.5
    veh, _ = PlantModel(dynamics_configs=heavy, per_chain_delay_steps=d).lower_ensemble(P, B)
    assert all(veh[b * 2 + 1].mass == P.agents[1].mass * 1.5 and veh[b * 2].mass == P.agents[0].mass for b in range(B))
    veh, _ = PlantModel(per_chain_delay_steps=d).lower_ensemble(P, B)
    assert all(bytes(veh[b * 2 + a]) == bytes(P.agents[a])[:160] for b in range(B) for a in range(2))
    # what is refused
    with pytest.raises(ValueError, match=r'\[B\]\[M\]'):
        PlantModel(per_chain_configs=ens).lower_ensemble(P, B + 1)
    with pytest.raises(ValueError, match=r'\[B\]\[M\]'):
        PlantModel(per_chain_configs=[row[:1] for row in ens]).lower_ensemble(P, B)
    wrong = [list(row) for row in ens]; wrong[2][1] = DynamicBicycleConfig()
    with pytest.raises(ValueError, match='model class'):
        PlantModel(per_chain_configs=wrong).lower_ensemble(P, B)
    with pytest.raises(ValueError, match=r'\[B\]\[M\]\[2\]'):
        PlantModel(per_chain_delay_steps=np.zeros((B, 2))).lower_ensemble(P, B)
    for bad in (_ffi.MAX_DELAY + 1, -1, 1.5):
        dd = d.astype(float); dd[1, 0, 1] = bad
        with pytest.raises(ValueError, match='delay'):
            PlantModel(per_chain_delay_steps=dd).lower_ensemble(P, B)
    with pytest.raises(ValueError, match='not both'):
        PlantModel(per_chain_delay_steps=d, per_chain_delay=sec).lower_ensemble(P, B)
    with pytest.raises(ValueError, match='delay'):
        PlantModel(sim_steps=4, per_chain_delay=np.full((B, 2, 2), 0.5)).lower_ensemble(P, B)      # 20 simulation steps
    with pytest.raises(ValueError, match='sim_steps'):
        PlantModel(sim_steps=0, per_chain_configs=ens).lower_ensemble(P, B)
