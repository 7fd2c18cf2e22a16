"""Track width functions on the device: dev_track_width (csrc/dgsqp_track_width.h) through the F1 study's raceline sampler with the e_y clip
by ``left_width(s)`` / ``right_width(s)`` (dgsqp_set_raceline_clip), against the numpy mirror; the setting's refusals; the 256-thread
build; and coexistence: a handle that carries a width table and does not use it computes what a handle without one computes.
Dynamic F1 game, N = 10, the study's [60, 80] m window, the TUM line of tests/golden/f1_traj_race_cl.csv.gz."""
import ctypes as C

import numpy as np
import pytest

import track_frame_checks as tf

pytestmark = pytest.mark.gpu

SEED, B = 11, 300


def make(clip, table=True, **kw):
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=10, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=tf.f1_raceline(), s_range=(60, 80), edges=clip)
    if not table:
        g.track.clear_width_table()          # build_problem then passes n_width = 0: the handle of the parent commit
    s = DGSQP(*g.solver_args(), print_method=None, **kw)
    assert s._problem.n_width == (1103 if table else 0)
    s.set_raceline(g.raceline)
    return g, s, mc.raceline_ws(g)


@pytest.fixture(scope='module')
def widths():
    return make('track')


@pytest.fixture(scope='module')
def constant():
    return make('constant')


@pytest.fixture(scope='module')
def drawn(widths):
    """The device's B = 300, seed 11 batch with the width clip, drawn once."""
    g, s, W = widths
    return s.sample_raceline_batch(g, B, seed=SEED, ws=W)


def test_sampler_with_the_width_clip_against_its_mirror(widths, drawn):
    """The batch against sampler.sample_raceline_counter (placement, clip and collision check in numpy -- tracks.left_width /
    right_width --, the warm-start program per round through the same tracker kernel): the same candidates, x0 -- s, e_y, x, y, v, e_psi of
    both cars -- and u_ws bit for bit.  Precondition: no collision margin within 1e-9 of zero."""
    from dgsqp_amd import sampler as smp
    g, s, W = widths
    x0, u_ws, used, closest = smp.sample_raceline_counter(g, s, B, SEED, ws=W)
    print(f'{used} candidates for {B} scenarios, closest collision margin {closest:.2e}')
    assert closest > 1e-9
    assert drawn['candidates'] == used
    for name, cols in (('s', [6, 14]), ('e_y', [7, 15]), ('x', [0, 8]), ('y', [1, 9])):
        d = np.abs(drawn['x0'][:, cols] - x0[:, cols]).max()
        print(f'{name}: max |device - mirror| {d:.2e}')
    assert np.array_equal(tf.bits(drawn['x0']), tf.bits(x0))
    assert np.array_equal(tf.bits(drawn['u_ws']), tf.bits(u_ws))


def test_the_clip_is_the_tracks(widths, constant, drawn):
    """Every accepted e_y lies within 0.9 x the widths at its own s (the numpy functions, which carry the device's bits); at least one sits
    exactly on a scaled width that differs from 0.9 x the constant bound; and the constant clip's batch of the same seed, drawn on a handle
    that carries the table too, is the mirror's and another one."""
    from dgsqp_amd import sampler as smp
    g, s, W = widths
    t, lim = g.track, 0.9 * g.half_width
    on = 0
    for a in range(2):
        sa, ey = drawn['x0'][:, 8 * a + 6], drawn['x0'][:, 8 * a + 7]
        hi, lo = 0.9 * t.left_width(sa), -0.9 * t.right_width(sa)
        assert (ey <= hi).all() and (ey >= lo).all()
        on += int((((ey == hi) & (np.abs(hi - lim) > 1e-3)) | ((ey == lo) & (np.abs(lo + lim) > 1e-3))).sum())
        print(f'car {a + 1}: e_y {ey.min():.3f} .. {ey.max():.3f}; beyond the constant clip {lim:.3f}: {int((np.abs(ey) > lim).sum())}')
    print(f'{on} accepted placements sit on a scaled width')
    assert on >= 1
    g0, s0, W0 = constant
    dev0 = s0.sample_raceline_batch(g0, B, seed=SEED, ws=W0)
    x0, u_ws, used, closest = smp.sample_raceline_counter(g0, s0, B, SEED, ws=W0)
    assert closest > 1e-9 and dev0['candidates'] == used
    assert np.array_equal(tf.bits(dev0['x0']), tf.bits(x0)) and np.array_equal(tf.bits(dev0['u_ws']), tf.bits(u_ws))
    assert (np.abs(dev0['x0'][:, [7, 15]]) <= lim).all()
    assert not np.array_equal(dev0['x0'], drawn['x0'])


def test_staged_path(widths):
    """stage=True + dgsqp_solve_staged against solve_batch of the fetched batch, bit for bit (the first 16 scenarios)."""
    from dgsqp_amd import _ffi
    g, s, W = widths
    n = 16
    dev = s.sample_raceline_batch(g, n, seed=SEED, ws=W)
    ref = s.solve_batch(dev['x0'], dev['u_ws'])
    s.sample_raceline_batch(g, n, seed=SEED, ws=W, stage=True, fetch=False)
    tm = _ffi.TimingT()
    assert s._lib.dgsqp_solve_staged(s._h, C.byref(tm)) == 0, s._lib.dgsqp_last_error(s._h)
    st, it, qp = (np.empty(n, np.int32) for _ in range(3))
    u = np.empty((n, s.n))
    assert s._lib.dgsqp_fetch_results(s._h, _ffi.dptr(u), None, None, _ffi.iptr(st), _ffi.iptr(it), _ffi.iptr(qp), None, None) == 0
    assert np.array_equal(st, ref['status']) and np.array_equal(it, ref['num_iters']) and np.array_equal(qp, ref['qp_solves'])
    assert np.array_equal(u, ref['u'], equal_nan=True)


def test_refusals_and_the_setting_is_sticky(widths):
    """dgsqp_set_raceline_clip through the raw ABI: every refusal with its message, the setting in force survives a refusal, 0 restores the
    constant clip, and a table is refused at create with its 'widths: ' message."""
    from dgsqp_amd import _ffi, sampler as smp
    from dgsqp_amd.solver import DGSQP, build_problem
    g, s, W = widths
    lib = s._lib
    g_bare, bare, W_bare = make('constant', table=False)

    def refused(handle, mode, scale, word):
        assert lib.dgsqp_set_raceline_clip(handle._h, mode, scale) == _ffi.E_ARG
        msg = lib.dgsqp_last_error(handle._h).decode()
        assert msg.startswith('raceline: ') and word in msg, msg
    assert lib.dgsqp_set_raceline_clip(None, 0, 0.0) == _ffi.E_ARG
    assert lib.dgsqp_set_raceline_clip(s._h, 1, 0.9) == 0
    for mode, scale, word in ((2, 0.9, '0 or 1'), (-1, 0.9, '0 or 1'), (1, -0.1, 'clip_scale'), (1, np.nan, 'clip_scale'), (1, np.inf, 'clip_scale')):
        refused(s, mode, scale, word)
    refused(bare, 1, 0.9, 'without a width table')
    assert lib.dgsqp_set_raceline_clip(bare._h, 0, np.nan) == 0                     # off: the scale is not read
    spec = smp.raceline_spline_sampler_spec(g, SEED)

    def raw(handle, ws=W_bare, n=8):          # (the warm-start program with the e_y box: a handle without a table refuses the edge rows)
        x0 = np.empty((n, handle.n_q))
        assert lib.dgsqp_sample_raceline_spline_batch(handle._h, n, C.byref(spec), C.byref(ws), _ffi.dptr(x0), None, None, 0) == 0, lib.dgsqp_last_error(handle._h)
        return x0
    assert lib.dgsqp_sample_raceline_spline_batch(bare._h, 8, C.byref(spec), C.byref(W), None, None, None, 0) == _ffi.E_ARG
    assert lib.dgsqp_last_error(bare._h).decode().startswith('mpc: edge_rows on a handle without a width table')
    with_widths = raw(s)                                                             # still 1, 0.9 after the refusals
    assert lib.dgsqp_set_raceline_clip(s._h, 0, 0.0) == 0
    with_constant = raw(s)
    assert np.array_equal(tf.bits(with_constant), tf.bits(raw(bare)))               # the handle without a table: the parent's draw
    assert (np.abs(with_constant[:, [7, 15]]) <= spec.ey_clip).all() and not np.array_equal(with_widths, with_constant)
    assert lib.dgsqp_set_raceline_clip(s._h, 1, 0.0) == 0                            # scale 0: every car on the centre line
    assert (raw(s)[:, [7, 15]] == 0.0).all()
    assert np.array_equal(tf.bits(s.sample_raceline_batch(g, 8, seed=SEED, ws=W_bare)['x0']), tf.bits(with_widths))      # the wrapper states the game's setting
    # create
    P = build_problem(*g.solver_args())
    bad = P._widths_keepalive.copy()
    bad[5, 1] = -1.0
    P.widths = bad.ctypes.data
    h = C.c_void_p()
    assert lib.dgsqp_create(C.byref(P), C.byref(s._cparams), 0, C.byref(h)) == _ffi.E_ARG
    assert lib.dgsqp_last_error(None).decode().startswith('widths: ')


def test_256_thread_build(widths, drawn):
    g, s, W = widths
    _, b, _ = make('track', workgroups_per_cu=2)
    out = b.sample_raceline_batch(g, 64, seed=SEED, ws=W)
    assert out['candidates'] >= 64
    for a in range(2):
        sa, ey = out['x0'][:, 8 * a + 6], out['x0'][:, 8 * a + 7]
        assert (ey <= 0.9 * g.track.left_width(sa)).all() and (ey >= -0.9 * g.track.right_width(sa)).all()
    where = {int(v): i for i, v in enumerate(tf.bits(drawn['x0'][:, 6]))}
    both = [(i, where[int(v)]) for i, v in enumerate(tf.bits(out['x0'][:, 6])) if int(v) in where]
    print(f'{len(both)} of 64 scenarios also in the product build\'s batch')
    assert len(both) >= 32          # (a warm start may succeed on one build and fail on the other; the placements are the same)
    i, j = np.array(both).T
    assert np.array_equal(tf.bits(out['x0'][i]), tf.bits(drawn['x0'][j]))


def test_a_table_nobody_reads_changes_nothing(constant):
    """Coexistence: the handle with the table (constant clip, so nothing reads it) against a handle of the same game without one:
    the sampler's batch, the warm-start program (the tracker's kernel) and solve_batch, bit for bit."""
    g, s, W = constant
    g0, s0, W0 = make('constant', table=False)
    a, b = s.sample_raceline_batch(g, 16, seed=3, ws=W), s0.sample_raceline_batch(g0, 16, seed=3, ws=W0)
    assert a['candidates'] == b['candidates']
    assert np.array_equal(tf.bits(a['x0']), tf.bits(b['x0'])) and np.array_equal(tf.bits(a['u_ws']), tf.bits(b['u_ws']))
    wa, wb = s.raceline_warm_start_batch(a['x0'], W), s0.raceline_warm_start_batch(a['x0'], W0)
    assert np.array_equal(wa['ok'], wb['ok']) and np.array_equal(tf.bits(wa['u_ws']), tf.bits(wb['u_ws']))
    ra, rb = s.solve_batch(a['x0'], a['u_ws']), s0.solve_batch(a['x0'], a['u_ws'])
    for key in ('status', 'num_iters', 'qp_solves'):
        assert np.array_equal(ra[key], rb[key]), key
    for key in ('u', 'l', 'x', 'cond'):
        assert np.array_equal(ra[key], rb[key], equal_nan=True), key
