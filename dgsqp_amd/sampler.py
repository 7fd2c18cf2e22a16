"""Counter-based rejection samplers: the host mirror of ``dgsqp_sample_batch`` (csrc/dgsqp_sampler.h).

The Monte-Carlo scripts of the reference draw from ``np.random.default_rng(seed)`` in a sequential loop
(scripts/DGSQP_ALGAMES_monte_carlo_chicane.py:384-404, DGSQP_monte_carlo_agents.py:262-308, DGSQP_comp_monte_carlo.py:365-382,
DGSQP_merge_monte_carlo.py:429-473); ``dgsqp_amd.montecarlo.sample_scenarios`` reproduces those draws on the host.  On the device
the candidates of a round are drawn by thousands of lanes at once, so the stream has to be a pure function of (seed, candidate,
draw): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  This module restates the
generator and the placement rules in numpy -- the same 53-bit uniforms bit for bit, the same accept / reject decisions, initial
states equal to rounding of sin / cos -- and is what the tests compare the device against.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .game import InputRateLimits, record_of
from . import _ffi
from .tracks import local_to_global_batch

FIRST_SEGMENT, INDEPENDENT, CIRCUIT, MERGE = 0, 1, 2, 3
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4] uint32, key (k0, k1) -> [..., 4] uint32 (ten rounds)."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(seed: int, cand, k: int):
    """Uniform k of the candidates ``cand`` (array of indices): 53 random bits, ((a >> 5) 2^26 + (b >> 6)) / 2^53."""
    cand = np.asarray(cand, dtype=np.uint64)
    ctr = np.stack([cand & _MASK, cand >> np.uint64(32), np.full(cand.shape, k >> 1, np.uint64), np.zeros(cand.shape, np.uint64)], axis=-1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    a, b = r[..., (k & 1) * 2].astype(np.uint64), r[..., (k & 1) * 2 + 1].astype(np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


class SamplerT(C.Structure):
    _fields_ = [('kind', C.c_int32), ('n_key', C.c_int32), ('seed', C.c_uint64), ('half_width', C.c_double), ('obs_d', C.c_double),
                ('seg0_len', C.c_double), ('x_nom', C.c_double * _ffi.MAX_AGENTS), ('key_pts', (C.c_double * 6) * (_ffi.MAX_SEGS + 1))]


def sampler_kind(game) -> int:
    if game.sampler == 'merge':
        return MERGE
    if game.sampler == 'circuit':
        return CIRCUIT
    return FIRST_SEGMENT if game.joint_model.n_a == 2 else INDEPENDENT


def sampler_spec(game, seed: int) -> SamplerT:
    """The C-ABI description of the game's sampler (include/dgsqp.h: dgsqp_sampler_t)."""
    from .montecarlo import _MERGE_X_NOM
    if getattr(game, 'second_car_ahead', False):
        raise ValueError("the device sampler has no 'car 2 ahead of car 1' rule (DGSQP_monte_carlo_ablation.py:387): sample this game on the host (montecarlo.sample_scenarios)")
    S = SamplerT()
    S.kind, S.seed = sampler_kind(game), int(seed)
    S.half_width, S.obs_d = float(game.half_width), float(game.obs_d)
    for a in range(_ffi.MAX_AGENTS):
        S.x_nom[a] = _MERGE_X_NOM[a]
    if S.kind != MERGE and getattr(game.track, 'kind', 'arcs') == 'spline':
        if S.kind != CIRCUIT:
            raise ValueError("on a spline track the device sampler places cars with the 'circuit' rule only (the others need the first segment of an arc track)")
        S.n_key = 0                  # the handle's spline (dg_sample_place_spline_kernel)
    elif S.kind != MERGE:
        kp = np.asarray(game.track.key_pts, dtype=float)
        if not hasattr(game.track, 'key_pts') or kp.shape[0] > _ffi.MAX_SEGS + 1:
            raise ValueError('the device sampler places cars on arc tracks (key points); spline tracks are sampled on the host')
        S.n_key = kp.shape[0]
        S.seg0_len = float(game.track.cl_segs[0, 0])
        for i in range(kp.shape[0]):
            for j in range(6):
                S.key_pts[i][j] = float(kp[i, j])
    return S


def place(game, seed: int, cand):
    """Placement of the candidates ``cand`` -> (q0 list per agent [n, n_q^a], ok [n]): the arithmetic of dg_sample_place_kernel."""
    cand = np.asarray(cand, dtype=np.uint64)
    n = len(cand)
    U = lambda k: uniform(seed, cand, k)
    models = game.joint_model.dynamics_models
    M = len(models)
    kind = sampler_kind(game)
    ok = np.ones(n, bool)
    if kind == MERGE:
        from .montecarlo import _MERGE_X_NOM
        mw, mp, th = 0.3, 1.5, np.pi / 12
        x5, x7 = mp, mp + mw / np.sin(th)
        q0 = []
        for a in range(M):
            xn = _MERGE_X_NOM[a]
            q = np.zeros((n, 4))
            if a % 3 != 2:
                q[:, 0] = xn + 0.5 * U(4 * a) - 0.25
                q[:, 1] = 0.15 + 0.1 * U(4 * a + 1) - 0.05
                q[:, 2] = 0.3 * (1 + 0.06 * U(4 * a + 2) - 0.03)
                q[:, 3] = (5 * U(4 * a + 3) - 2.5) * np.pi / 180
            else:
                yn = -((x7 + x5) / 2 - xn) * np.tan(th)
                sr, er = 0.5 * U(4 * a) - 0.25, 0.1 * U(4 * a + 1) - 0.05
                q[:, 0] = xn + sr * np.cos(th) - er * np.sin(th)
                q[:, 1] = yn + sr * np.sin(th) + er * np.cos(th)
                q[:, 2] = 0.3 * (1 + 0.06 * U(4 * a + 2) - 0.03)
                q[:, 3] = np.pi / 12 + (5 * U(4 * a + 3) - 2.5) * np.pi / 180
            q0.append(q)
        return q0, ok
    track, hw, obs_d = game.track, game.half_width, game.obs_d

    def put(mdl, s, ey, v, epsi):
        xy = local_to_global_batch(track, np.stack([s, ey, np.zeros(n)], axis=1))
        q = np.zeros((n, mdl.n_q))
        q[:, 0], q[:, 1], q[:, 2] = xy[:, 0], xy[:, 1], v
        q[:, mdl.epsi_idx] = epsi
        q[:, mdl.s_idx], q[:, mdl.ey_idx] = s, ey
        return q
    if kind == FIRST_SEGMENT:
        seg0 = track.cl_segs[0, 0]
        s1, ey1, v1 = np.maximum(0.1, U(0) * seg0), U(1) * hw * 2 - hw, U(2) + 2
        d = 2 * np.pi * U(3)
        s2, ey2, v2 = s1 + 1.2 * obs_d * np.cos(d), ey1 + 1.2 * obs_d * np.sin(d), U(4) + 2
        ok = (s2 >= 0) & (np.abs(ey2) <= hw)
        s2s, ey2s = np.where(ok, s2, s1), np.where(ok, ey2, ey1)           # (rejected placements are never used)
        return [put(models[0], s1, ey1, v1, 0.0), put(models[1], s2s, ey2s, v2, 0.0)], ok
    if kind == INDEPENDENT:
        seg0 = track.cl_segs[0, 0]
        return [put(m, np.maximum(0.1, U(3 * a) * seg0), U(3 * a + 1) * hw * 2 - hw, U(3 * a + 2) + 2, 0.0) for a, m in enumerate(models)], ok
    L = track.track_length
    s1, v1 = L * U(0), 2.0 + (U(2) - 0.5)
    q0 = [put(models[0], s1, hw * (2 * U(1) - 1), v1, 5.0 * (2 * U(3) - 1) * np.pi / 180)]
    for a in range(1, M):
        q0.append(put(models[a], s1 + 1.2 * obs_d * (2 * U(4 * a) - 1), hw * (2 * U(4 * a + 1) - 1), (1 + 0.25 * (2 * U(4 * a + 2) - 1)) * v1,
                      5.0 * (2 * U(4 * a + 3) - 1) * np.pi / 180))
    return q0, ok


def sample_scenarios_counter(game, B: int, seed: int = 1, chunk: int = 512, max_candidates: int = 10_000_000):
    """Host mirror of ``dgsqp_sample_batch``: the first B accepted candidates in candidate order.
    Returns x0 [B, n_q], u_ws [B, N, n_u] (time-major) and the number of candidates consumed."""
    from .montecarlo import pid_warm_start
    models = game.joint_model.dynamics_models
    M, N, dt = len(models), game.params.N, game.params.dt
    kind = sampler_kind(game)
    radii = list(game.shared_constraints.radii) if game.shared_constraints is not None else [game.obs_d / 2] * M
    rl = record_of(game.agent_constraints[0], InputRateLimits) if game.agent_constraints else None
    du = (10.0, 4.5) if rl is None else tuple(rl.rate_max)
    x0s, uws, have, c0, used = [], [], 0, 0, 0
    while have < B:
        if c0 >= max_candidates:
            raise RuntimeError('sampler did not produce enough collision-free scenarios')
        cand = np.arange(c0, c0 + chunk, dtype=np.uint64)
        q0, ok = place(game, seed, cand)
        if kind == MERGE:
            traj = []
            for a, mdl in enumerate(models):
                qa = [np.zeros((chunk, 4)) if (M == 3 and a == 2) else q0[a].copy()]
                for _ in range(N):
                    qa.append(np.array([mdl.fd(q, np.zeros(2)) for q in qa[-1]]))
                traj.append(np.stack(qa, axis=1))
            u_ws = [np.zeros((chunk, N, 2)) for _ in range(M)]
        else:
            traj, u_ws = zip(*[pid_warm_start(m, q, N, dt, du=du) for m, q in zip(models, q0)])
        keep = ok.copy()
        for i in range(M):
            for j in range(i + 1, M):
                dist = np.linalg.norm(traj[i][:, :, :2] - traj[j][:, :, :2], axis=2)
                keep &= ~(dist < radii[i] + radii[j]).any(axis=1)
        idx = np.nonzero(keep)[0]
        take = idx[:B - have]
        x0s.append(np.concatenate([q[take] for q in q0], axis=1))
        uws.append(np.concatenate([u[take] for u in u_ws], axis=2))
        have += len(take)
        if have >= B:
            used = c0 + int(take[-1]) + 1
        c0 += chunk
    return np.ascontiguousarray(np.concatenate(x0s)), np.ascontiguousarray(np.concatenate(uws)), used


# ---- the BARC study's sampler (dgsqp_sample_raceline_batch, csrc/dgsqp_raceline.h: dg_raceline_place_kernel) ----
def raceline_sampler_spec(game, seed: int) -> _ffi.RacelineSamplerT:
    """The C-ABI description of the study's placement (include/dgsqp.h: dgsqp_raceline_sampler_t)."""
    kp = np.asarray(game.track.key_pts, dtype=float)
    if kp.shape[0] > _ffi.MAX_SEGS + 1:
        raise ValueError('the device sampler places cars on arc tracks of at most %d segments' % _ffi.MAX_SEGS)
    S = _ffi.RacelineSamplerT()
    S.n_key, S.seed = kp.shape[0], int(seed)
    S.half_width, S.obs_d, S.collision_d = float(game.track.half_width), float(game.obs_d), float(game.collision_d)
    for i in range(kp.shape[0]):
        for j in range(6):
            S.key_pts[i][j] = float(kp[i, j])
    return S


def raceline_spline_sampler_spec(game, seed: int) -> _ffi.RacelineSplineSamplerT:
    """The C-ABI description of the F1 study's placement (include/dgsqp.h: dgsqp_raceline_spline_sampler_t).  Defaults as the study
    (comparison_study_f1/monte_carlo_sampler.py): s1 in [0, L - 10] -- ``game.s_range`` overrides --, gap in [0, 3 * 0.56], collision
    distance ``game.collision_d``.  ``game.clip_widths``: the study's clip of e_y with 0.9 x the track's width functions at the car's own s;
    otherwise e_y is clipped to 0.9 x the game's one constant lateral bound."""
    from .montecarlo import F1_STUDY_VL
    if getattr(game.track, 'kind', 'arcs') != 'spline':
        raise ValueError('the spline-track raceline sampler needs a game on a spline track (raceline_sampler_spec places cars on arc tracks)')
    S = _ffi.RacelineSplineSamplerT()
    S.seed = int(seed)
    S.s_lo, S.s_hi = (0.0, float(game.track.track_length) - 10.0) if game.s_range is None else (float(game.s_range[0]), float(game.s_range[1]))
    S.gap_lo, S.gap_hi = 0.0, 3 * F1_STUDY_VL
    S.ey_clip, S.collision_d = 0.9 * float(game.half_width), float(game.collision_d)
    return S


RACELINE_CLIP_SCALE = 0.9            # comparison_study_f1/monte_carlo_sampler.py:29,38


def raceline_clip(game):
    """(clip_widths, clip_scale) of dgsqp_set_raceline_clip for ``game``."""
    return (1, RACELINE_CLIP_SCALE) if getattr(game, 'clip_widths', False) else (0, 0.0)


def _place_raceline_spline(game, seed: int, cand):
    """comparison_study_f1/monte_carlo_sampler.py:25-55 with the counter-based uniforms: the arithmetic of dg_raceline_place_spline_kernel."""
    U = lambda k: uniform(seed, cand, k)
    S = raceline_spline_sampler_spec(game, seed)
    widths, scale = raceline_clip(game)
    rl, track = game.raceline, game.track
    models = game.joint_model.dynamics_models
    s1 = S.s_lo + (S.s_hi - S.s_lo) * U(0)
    q0, xy = [], []
    for a, mdl in enumerate(models[:2]):
        s = s1 if a == 0 else s1 + S.gap_lo + (S.gap_hi - S.gap_lo) * U(3)
        r = rl.eval(rl.s2t(s))
        hi, lo = (scale * track.left_width(s), -scale * track.right_width(s)) if widths else (S.ey_clip, -S.ey_clip)
        ey = np.maximum(np.minimum(r[:, 8] + (2 * U(3 * a + 1) - 1), hi), lo)
        v = r[:, 3] + (1.5 * U(3 * a + 2) - 0.75)
        p = local_to_global_batch(track, np.stack([s, ey, np.zeros(len(cand))], axis=1))[:, :2]
        q = np.zeros((len(cand), mdl.n_q))
        q[:, 0], q[:, 1], q[:, 2] = p[:, 0], p[:, 1], v
        q[:, mdl.epsi_idx], q[:, mdl.s_idx], q[:, mdl.ey_idx] = r[:, 6], s, ey
        q0.append(q); xy.append(p)
    d = xy[0] - xy[1]
    return np.concatenate(q0, axis=1), S.collision_d ** 2 - (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def place_raceline(game, seed: int, cand):
    """monte_carlo_sampler_dynamic.py:27-57 for the candidates ``cand`` with the counter-based uniforms, six per candidate in the script's
    order (s1, e_y1, v1, s2, e_y2, v2) -> (x0 [n, n_q], margin [n]); a candidate is in collision when margin >= 0.  A game on a spline
    track is placed by the F1 study's law instead (``raceline_spline_sampler_spec``)."""
    cand = np.asarray(cand, dtype=np.uint64)
    if getattr(game.track, 'kind', 'arcs') == 'spline':
        return _place_raceline_spline(game, seed, cand)
    U = lambda k: uniform(seed, cand, k)
    rl, track = game.raceline, game.track
    L, lim = track.track_length, 0.9 * track.half_width
    models = game.joint_model.dynamics_models
    s1 = L * U(0)
    q0, xy = [], []
    for a, mdl in enumerate(models[:2]):
        s = s1 if a == 0 else s1 + 1.2 * game.obs_d * (2 * U(3) - 1)
        r = rl.eval(rl.s2t(s))
        ey = np.maximum(np.minimum(r[:, 8] + (2 * U(3 * a + 1) - 1), lim), -lim)
        v = r[:, 3] + (1.5 * U(3 * a + 2) - 0.75)
        p = np.array([track.local_to_global((si, ei, 0.0))[:2] for si, ei in zip(s, ey)]).reshape(-1, 2)
        q = np.zeros((len(cand), mdl.n_q))
        q[:, 0], q[:, 1], q[:, 2] = p[:, 0], p[:, 1], v
        q[:, mdl.epsi_idx], q[:, mdl.s_idx], q[:, mdl.ey_idx] = r[:, 6], s, ey
        q0.append(q); xy.append(p)
    d = xy[0] - xy[1]
    return np.concatenate(q0, axis=1), game.collision_d ** 2 - (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def sample_raceline_counter(game, solver, B: int, seed: int = 1, ws=None, max_candidates: int = 10_000_000):
    """Host mirror of ``dgsqp_sample_raceline_batch``: placement and collision check in numpy, the warm-start program through
    ``solver.raceline_warm_start_batch`` (the tracker has no host form), the first B accepted candidates in candidate order, in the device's
    rounds.  Returns x0 [B, n_q], u_ws [B, N, n_u] (time-major), the candidates consumed and the smallest |margin| seen."""
    from .montecarlo import raceline_ws
    W = raceline_ws(game) if ws is None else ws
    nround = max(256, min(2 * B, 1 << 16))
    x0s, uws, have, c0, used, closest = [], [], 0, 0, 0, np.inf
    while have < B:
        if c0 >= max_candidates:
            raise RuntimeError('sampler did not produce enough scenarios')
        x0, margin = place_raceline(game, seed, np.arange(c0, c0 + nround, dtype=np.uint64))
        closest = min(closest, float(np.abs(margin).min()))
        out = solver.raceline_warm_start_batch(x0, W)
        idx = np.nonzero((margin < 0) & out['ok'])[0]
        take = idx[:B - have]
        x0s.append(x0[take]); uws.append(out['u_ws'][take])
        have += len(take)
        if have >= B:
            used = c0 + int(take[-1]) + 1
        c0 += nround
    return np.ascontiguousarray(np.concatenate(x0s)), np.ascontiguousarray(np.concatenate(uws)), used, closest
