"""The hand-written fp64 device primitives of csrc/dgsqp_device.h and csrc/dgsqp_eval.h, one at a time, against plain mpmath references
(60 digits), on a real MI355X through the probe library (tests/device_math_probe.py, tests/csrc/device_math_probe.hip).

Error in ulp: |got - exact| / ulp(exact), exact kept as an unevaluated sum of two doubles (never rounded to one first).  The caps are
conditions (the algorithms' own maxima from a CPU emulation with exact fma, rounded up), not measurements; every test prints what it
measured and the argument that attains it before it asserts (pytest -s).  The caps and conventions: DESIGN.md section 2, item 5.

The random sweeps come in four chunks of 5 x 10^4 points (2 x 10^5 per function in all): the references cost ~30 us a point."""
import fractions
import math

import mpmath
import numpy as np
import pytest

import device_math_probe as dmp

pytestmark = pytest.mark.gpu

MP = mpmath.MPContext()
MP.prec = 200                                   # 60 digits
CHUNKS, CHUNK_N = 4, 50000
CAPS = {'rcp': 1.0, 'atan': 1.0, 'roll_atan': 1.0, 'sin': 2.0, 'cos': 2.0, 'roll_atan2': 2.0, 'atan2': 2.5, 'tan': 4.0}      # ulp
BIG_K_ABS = 2.0 ** -52                          # sin, cos at x ~ k pi / 2, 8 < |k| <= 2e6: absolute
JET_BAR, TRACK_BAR, SPLINE_BAR = 1e-11, 1e-13, 1e-11
THRESHOLDS = (7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16)
PI, PIO2 = math.pi, math.pi / 2


# ---------------------------------------------------------------------------------------------------------------------------------
# handles (one arc-track game for everything but the spline look-up) and reference plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def probe():
    from dgsqp_amd.montecarlo import kinematic_racing_game
    p = dmp.Probe(kinematic_racing_game('curve', N=3))
    yield p
    p.close()


def mpf(v):
    return MP.mpf(float(v))                     # a double, exactly


def split(vals):
    """list of mpf -> (hi, lo) arrays with hi + lo = value to ~2^-106"""
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - MP.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(vals, hi.tolist())])
    return hi, lo


def ulp_of(hi, lo):
    """ulp(exact) for exact = hi + lo: 2^(e - 52) with 2^e <= |exact| < 2^(e + 1) (the spacing of doubles just below a power of two
    where exact sits below one that hi was rounded up to)"""
    a = np.abs(hi)
    m, e = np.frexp(a)
    u = np.ldexp(1.0, np.maximum(e - 53, -1074))
    below = (m == 0.5) & (np.sign(lo) == -np.sign(hi)) & (lo != 0)
    return np.where(below, 0.5 * u, u)


def ulp_err(got, ref):
    hi, lo = ref
    return np.abs((got - hi) - lo) / ulp_of(hi, lo)


def report(name, err, *args, unit='ulp'):
    i = int(np.nanargmax(err))
    at = ', '.join(f'{float(a[i])!r}' for a in args)
    print(f'{name}: max error {err[i]:.3g} {unit} at ({at})')
    return float(err[i])


def check_cap(name, cap_key, got, ref, *args):
    err = ulp_err(got, ref)
    assert np.isfinite(got).all(), (name, 'non-finite result')
    worst = report(name, err, *args)
    assert worst <= CAPS[cap_key], (name, worst, CAPS[cap_key])
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def ordinal_distance(a, b):
    """how many doubles apart (monotone integer image of the doubles)"""
    def key(v):
        i = bits(v).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(key(a) - key(b))


def step(x, k):
    """x moved by k ulp (k steps of nextafter)"""
    x = np.asarray(x, dtype=np.float64).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def around(x, reach=2):
    return np.concatenate([step(x, k) for k in range(-reach, reach + 1)])


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# fast_rcp
# ---------------------------------------------------------------------------------------------------------------------------------
def _rcp_inputs(chunk):
    rng = np.random.default_rng(100 + chunk)
    x = rng.choice((-1.0, 1.0), CHUNK_N) * 2.0 ** rng.uniform(-30, 30, CHUNK_N)
    x[:8] = (1.0, -1.0, 2.0 ** -30, 2.0 ** 30, 3.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, -0.75)
    return x


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_fast_rcp(probe, chunk):
    x = _rcp_inputs(chunk)
    ref = split([1 / mpf(v) for v in x])
    check_cap('fast_rcp', 'rcp', probe.run('rcp', x), ref, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# sin, cos, tan
# ---------------------------------------------------------------------------------------------------------------------------------
def _sincos_inputs(chunk):
    """(x, n_tan): the first n_tan points lie in |x| < 1.5, dev_tan's domain"""
    rng = np.random.default_rng(200 + chunk)
    n_tan, n_mid = 2 * CHUNK_N // 5, CHUNK_N // 5
    return np.concatenate([rng.uniform(-1.5, 1.5, n_tan), rng.uniform(-4, 4, n_mid), rng.uniform(-2.0 ** 20, 2.0 ** 20, CHUNK_N - n_tan - n_mid)]), n_tan


def _sincos_sweep(chunk):
    def make():
        x, n_tan = _sincos_inputs(chunk)
        s, c = [MP.sin(mpf(v)) for v in x], [MP.cos(mpf(v)) for v in x]
        return x, n_tan, split(s), split(c), split([a / b for a, b in zip(s[:n_tan], c[:n_tan])])
    return cached(('sincos', chunk), make)


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_sincos_tan_sweep(probe, chunk):
    """dev_sincos, roll_sincos, roll_sin on |x| < 4 and |x| < 2^20, dev_tan on |x| < 1.5; sin odd and cos even to the bit."""
    x, n_tan, rs, rc, rt = _sincos_sweep(chunk)
    s, c = probe.run('sincos', x)
    check_cap('dev_sincos sin', 'sin', s, rs, x)
    check_cap('dev_sincos cos', 'cos', c, rc, x)
    s2, c2 = probe.run('roll_sincos', x)
    check_cap('roll_sincos sin', 'sin', s2, rs, x)
    check_cap('roll_sincos cos', 'cos', c2, rc, x)
    check_cap('roll_sin', 'sin', probe.run('roll_sin', x), rs, x)
    check_cap('dev_tan', 'tan', probe.run('tan', x[:n_tan]), rt, x[:n_tan])
    sm, cm = probe.run('sincos', -x)
    assert same_bits(sm, -s) and same_bits(cm, c)
    sm, cm = probe.run('roll_sincos', -x)
    assert same_bits(sm, -s2) and same_bits(cm, c2)
    assert same_bits(probe.run('roll_sin', -x), -probe.run('roll_sin', x))


def test_sincos_near_multiples_of_half_pi(probe):
    """x = fl(k pi / 2) +- 0, 1, 2 ulp, where the two-term Cody-Waite reduction leaves ~|k| 1e-33 absolute: the ulp caps for |k| <= 8,
    2^-52 absolute for 8 < |k| <= 2 x 10^6 (the result is tiny there and an ulp of it means nothing)."""
    def points(ks):
        k = np.array(ks, dtype=np.float64)
        return around(np.concatenate([k, -k]) * PIO2)
    small, big = points(range(0, 9)), points(list(range(9, 2000001, 997)) + [2000000])
    for name, x, big_k in (('|k| <= 8', small, False), ('8 < |k| <= 2e6', big, True)):
        rs, rc = split([MP.sin(mpf(v)) for v in x]), split([MP.cos(mpf(v)) for v in x])
        for op in ('sincos', 'roll_sincos'):
            s, c = probe.run(op, x)
            if big_k:
                for what, got, ref in (('sin', s, rs), ('cos', c, rc)):
                    err = np.abs((got - ref[0]) - ref[1])
                    report(f'{op} {what} {name} (also {ulp_err(got, ref).max():.3g} ulp)', err, x, unit='absolute')
                    assert err.max() <= BIG_K_ABS, (op, what, err.max())
            else:
                check_cap(f'{op} sin {name}', 'sin', s, rs, x)
                check_cap(f'{op} cos {name}', 'cos', c, rc, x)
            # quadrant: the sign of every result that is not the tiny one
            for got, ref in ((s, rs), (c, rc)):
                firm = np.abs(ref[0]) > 0.5
                assert np.array_equal(np.sign(got[firm]), np.sign(ref[0][firm]))


def test_roll_sin_fast_path_edge(probe):
    """|x| = 0.78 +- 1 ulp, whole wavefronts of one value: just inside the fast path of roll_sin / roll_sincos, on its edge, just outside."""
    v = np.concatenate([around(np.array([0.78]), 1), around(np.array([-0.78]), 1)])
    x = np.repeat(v, 64)
    rs, rc = split([MP.sin(mpf(t)) for t in x]), split([MP.cos(mpf(t)) for t in x])
    s, c = probe.run('sincos', x)
    s2, c2 = probe.run('roll_sincos', x)
    assert same_bits(s, s2) and same_bits(c, c2) and same_bits(probe.run('roll_sin', x), s)
    check_cap('sin at the edge of the fast path', 'sin', s2, rs, x)
    check_cap('cos at the edge of the fast path', 'cos', c2, rc, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# atan
# ---------------------------------------------------------------------------------------------------------------------------------
def _atan_inputs(chunk):
    rng = np.random.default_rng(300 + chunk)
    h = CHUNK_N // 2
    return np.concatenate([rng.choice((-1.0, 1.0), h) * 2.0 ** rng.uniform(-20, 10, h), rng.uniform(-4, 4, CHUNK_N - h)])


def _atan_sweep(chunk):
    def make():
        x = _atan_inputs(chunk)
        return x, split([MP.atan(mpf(v)) for v in x])
    return cached(('atan', chunk), make)


def _atan_pair(probe, x, ref, tag):
    """dev_atan and roll_atan share the reduction but associate the tail differently (atan_poly_tail / roll_atan_core): both under the
    cap, hence at most 2 ulp = 4 doubles (across a binade edge) apart."""
    a, b = probe.run('atan', x), probe.run('roll_atan', x)
    check_cap(f'dev_atan {tag}', 'atan', a, ref, x)
    check_cap(f'roll_atan {tag}', 'roll_atan', b, ref, x)
    d = ordinal_distance(a, b)
    print(f'dev_atan / roll_atan {tag}: {int((d != 0).sum())} of {len(x)} differ, at most {int(d.max())} doubles apart')
    assert d.max() <= 4
    assert same_bits(probe.run('atan', -x), -a) and same_bits(probe.run('roll_atan', -x), -b)
    assert np.array_equal(np.sign(a), np.sign(x)) and np.array_equal(np.sign(b), np.sign(x))


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_atan_sweep(probe, chunk):
    x, ref = _atan_sweep(chunk)
    _atan_pair(probe, x, ref, 'sweep')


def test_atan_thresholds(probe):
    """The four range-reduction thresholds 7/16, 11/16, 19/16, 39/16, each +- 0, 1, 2 ulp, both signs; and the ends of the domain."""
    t = around(np.array(THRESHOLDS))
    x = np.concatenate([t, -t, [2.0 ** -20, 2.0 ** 10, -2.0 ** -20, -2.0 ** 10, 1.0, -1.0]])
    _atan_pair(probe, x, split([MP.atan(mpf(v)) for v in x]), 'thresholds')


# ---------------------------------------------------------------------------------------------------------------------------------
# atan2
# ---------------------------------------------------------------------------------------------------------------------------------
def _quadrant(r):
    return np.sign(r), np.abs(r) > PIO2


def _atan2_pair(probe, y, x, tag):
    ref = split([MP.atan2(mpf(a), mpf(b)) for a, b in zip(y, x)])
    out = {}
    for op, key in (('atan2', 'atan2'), ('roll_atan2', 'roll_atan2')):
        r = probe.run(op, y, x)
        out[key] = check_cap(f'{op} {tag}', key, r, ref, y, x)
        for got_q, want_q in zip(_quadrant(r), _quadrant(ref[0])):
            assert np.array_equal(got_q, want_q), (op, tag, 'quadrant')
        assert same_bits(probe.run(op, -y, x), -r), (op, tag, 'not antisymmetric in y')
        out[op + '_values'] = r
    d = ordinal_distance(out['atan2_values'], out['roll_atan2_values'])
    print(f'dev_atan2 / roll_atan2 {tag}: {int((d != 0).sum())} of {len(x)} differ, at most {int(d.max())} doubles apart')
    assert d.max() <= 9                          # 2.5 + 2 ulp, doubled across a binade edge
    return out


def _atan2_sweep(chunk):
    rng = np.random.default_rng(400 + chunk)
    mag = lambda: 2.0 ** rng.uniform(-10, 10, CHUNK_N)
    return rng.choice((-1.0, 1.0), CHUNK_N) * mag(), rng.choice((-1.0, 1.0), CHUNK_N) * mag()


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_atan2_sweep(probe, chunk):
    y, x = _atan2_sweep(chunk)
    _atan2_pair(probe, y, x, 'sweep')


def test_atan2_rays(probe):
    """The rays 16 |y| = c |x|, c in {7, 11, 19, 39}, where the range index changes: on them (x with few mantissa bits, so that c x / 16 is
    exact) and 1 ulp to either side, in all four quadrants."""
    xs = np.array([1.0, 3.0, 0.15625, 1000.0, 2.0 ** -10, 2.0 ** 10 * 0.875, 0.3125, 17.0])
    ys, xx = [], []
    for c in (7.0, 11.0, 19.0, 39.0):
        y0 = c * xs / 16.0
        assert all(fractions.Fraction(v) * 16 == fractions.Fraction(c) * fractions.Fraction(w) for v, w in zip(y0.tolist(), xs.tolist()))
        for k in (-1, 0, 1):
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    ys.append(sy * step(y0, k)); xx.append(sx * xs)
    _atan2_pair(probe, np.concatenate(ys), np.concatenate(xx), 'rays')
    # with x = 1 dev_atan2 / roll_atan2 are dev_atan / roll_atan operation by operation: the same range index at and around every threshold
    t = around(np.array(THRESHOLDS))
    t = np.concatenate([t, -t])
    one = np.ones(len(t))
    assert same_bits(probe.run('atan2', t, one), probe.run('atan', t))
    assert same_bits(probe.run('roll_atan2', t, one), probe.run('roll_atan', t))


def test_atan2_axes_and_origin(probe):
    """The axes (+-0, +-x), (+-y, +-0) and the pinned conventions: atan2(0, x < 0) = fl(pi); atan2(-0.0, x < 0) = +pi (IEEE 754: -pi;
    `y < 0.0` is false for -0.0 -- no game can tell, recorded on dev_atan2); atan2(+-0, +-0) = 0 for x >= 0 as std::atan2 and CasADi."""
    mags = np.array([2.0 ** -10, 0.3, 1.0, 7.5, 2.0 ** 10])
    for op in ('atan2', 'roll_atan2'):
        for z in (0.0, -0.0):
            zz = np.full(len(mags), z)
            assert np.array_equal(probe.run(op, zz, mags), np.zeros(len(mags))), (op, z, 'positive x axis')
            assert same_bits(probe.run(op, zz, -mags), np.full(len(mags), PI)), (op, z, 'negative x axis')
            for sy in (1.0, -1.0):
                r = probe.run(op, sy * mags, zz)
                ref = split([MP.atan2(mpf(v), mpf(0.0)) for v in sy * mags])
                check_cap(f'{op} y axis (x = {z!r}, sign {sy:+.0f})', 'roll_atan2', r, ref, sy * mags)
                assert np.array_equal(np.sign(r), np.full(len(mags), sy))
        y0 = np.array([0.0, -0.0, 0.0, -0.0]); x0 = np.array([0.0, 0.0, -0.0, -0.0])
        r = probe.run(op, y0, x0)
        print(op, 'at (+-0, +-0):', r)
        assert np.array_equal(r, np.zeros(4)), (op, r)
    # ... and hence the value of ty_atan2 (its derivative coefficients are 1 / 0 there)
    z = np.zeros(1)
    assert probe.run('ty_atan2', z, z, z, z, z, z)[0][0] == 0.0


def test_specials(probe):
    """2^-1022 (the smallest normal double), +-inf and NaN as arguments: the results are recorded (pytest -s); required is only that the
    kernels complete and that NaN in gives NaN out."""
    v = np.array([2.0 ** -1022, -2.0 ** -1022, np.inf, -np.inf, np.nan])
    for op in ('rcp', 'sincos', 'tan', 'atan', 'roll_atan', 'roll_sin', 'roll_sincos'):
        r = probe.run(op, v)
        r = r if isinstance(r, tuple) else (r,)
        print(op, [a.tolist() for a in r])
        assert all(np.isnan(a[4]) for a in r), op
    pairs = [(a, b) for a in v for b in (1.0, 2.0 ** -1022, np.inf, np.nan)] + [(b, a) for a in v for b in (1.0, np.nan)]
    y, x = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    for op in ('atan2', 'roll_atan2'):
        r = probe.run(op, y, x)
        print(op, list(zip(y.tolist(), x.tolist(), r.tolist())))
        nan_in = np.isnan(y) | np.isnan(x)
        assert np.isnan(r[nan_in]).all(), op


# ---------------------------------------------------------------------------------------------------------------------------------
# the wave-uniform fast paths of the rollout's functions against their general paths
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fast_path_is_the_general_path(probe):
    """Groups of 64 in-range inputs take the fast path; the same groups with lane 63 replaced by an out-of-range value take the general
    one: lanes 0 .. 62 must not change by a bit.  roll_sincos / roll_sin share dev_sincos's arithmetic on both paths: bit-identical to it."""
    rng = np.random.default_rng(500)
    G = 48
    n = 64 * G
    last = np.arange(n) % 64 == 63

    def both(op, ins, out_of_range):
        a = probe.run(op, *ins)
        ins2 = [np.where(last, o, v) for v, o in zip(ins, out_of_range)]
        b = probe.run(op, *ins2)
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        for p, q in zip(a, b):
            assert same_bits(p[~last], q[~last]), op
        return a, b

    x = rng.uniform(-0.4375, 0.4375, n); x[:64:7] = step(np.array([0.4375]), -1)[0]
    (fa,), _ = both('roll_atan', [x], [3.0])
    ref = split([MP.atan(mpf(v)) for v in x])
    check_cap('roll_atan fast path', 'roll_atan', fa, ref, x)
    d = ordinal_distance(fa, probe.run('atan', x))
    print('roll_atan fast path / dev_atan: at most', int(d.max()), 'doubles apart')
    assert d.max() <= 4

    xx = 2.0 ** rng.uniform(-10, 10, n)
    y = xx * rng.uniform(-0.4375, 0.4375, n)
    y = np.where(16.0 * np.abs(y) < 7.0 * xx, y, 0.0)
    (fa,), _ = both('roll_atan2', [y, xx], [1.0, -1.0])
    check_cap('roll_atan2 fast path', 'roll_atan2', fa, split([MP.atan2(mpf(a), mpf(b)) for a, b in zip(y, xx)]), y, xx)

    x = rng.uniform(-0.78, 0.78, n); x[5] = step(np.array([0.78]), -1)[0]
    s0, c0 = probe.run('sincos', x)
    (fs,), (gs,) = both('roll_sin', [x], [2.0])
    (s1, c1), (s2, c2) = both('roll_sincos', [x], [2.0])
    assert same_bits(fs, s0) and same_bits(s1, s0) and same_bits(c1, c0)
    xg = np.where(last, 2.0, x)
    sg, cg = probe.run('sincos', xg)
    assert same_bits(gs, sg) and same_bits(s2, sg) and same_bits(c2, cg)
    check_cap('roll_sincos fast path sin', 'sin', s1, split([MP.sin(mpf(v)) for v in x]), x)
    check_cap('roll_sincos fast path cos', 'cos', c1, split([MP.cos(mpf(v)) for v in x]), x)


# ---------------------------------------------------------------------------------------------------------------------------------
# Ty<2>: truncated Taylor arithmetic against mpmath.taylor of f(c0 + c1 t + c2 t^2) at t = 0
# ---------------------------------------------------------------------------------------------------------------------------------
N_JET = 384


def _away(rng, n, lo, hi):
    """+-[lo, hi]"""
    return rng.choice((-1.0, 1.0), n) * rng.uniform(lo, hi, n)


def _jet_inputs(rng, c0):
    return [c0, rng.uniform(-2, 2, len(c0)), rng.uniform(-2, 2, len(c0))]


def _poly(c):
    a, b, d = (mpf(v) for v in c)
    return lambda t: a + b * t + d * t * t


def _jet_check(name, got, f_of_polys, *jets):
    """got: three arrays; jets: per argument the three input arrays"""
    worst = 0.0
    for i in range(len(got[0])):
        polys = [_poly([j[0][i], j[1][i], j[2][i]]) for j in jets]
        want = MP.taylor(lambda t: f_of_polys(*[p(t) for p in polys]), 0, 2)
        scale = max(abs(w) for w in want)
        err = max(abs(mpf(got[k][i]) - want[k]) for k in range(3)) / scale
        worst = max(worst, float(err))
    print(f'{name}: max error {worst:.2e} of the largest coefficient')
    assert worst < JET_BAR, (name, worst)


JET_OPS = {
    'ty_recip': (lambda rng, n: [_jet_inputs(rng, _away(rng, n, 1e-2, 4))], lambda a: 1 / a),
    'ty_mul': (lambda rng, n: [_jet_inputs(rng, rng.uniform(-4, 4, n)), _jet_inputs(rng, rng.uniform(-4, 4, n))], lambda a, b: a * b),
    'ty_div': (lambda rng, n: [_jet_inputs(rng, rng.uniform(-4, 4, n)), _jet_inputs(rng, _away(rng, n, 1e-2, 4))], lambda a, b: a / b),
    'ty_tan': (lambda rng, n: [_jet_inputs(rng, rng.uniform(-1.5, 1.5, n))], lambda a: MP.tan(a)),
    'ty_atan': (lambda rng, n: [_jet_inputs(rng, rng.uniform(-8, 8, n))], lambda a: MP.atan(a)),
    'ty_atan2': (lambda rng, n: [_jet_inputs(rng, _away(rng, n, 1e-2, 4)), _jet_inputs(rng, _away(rng, n, 1e-2, 4))], lambda y, x: MP.atan2(y, x)),
    'ty_sqrt': (lambda rng, n: [_jet_inputs(rng, rng.uniform(1e-2, 4, n))], lambda a: MP.sqrt(a)),
}


@pytest.mark.parametrize('op', sorted(JET_OPS))
def test_taylor_jets(probe, op):
    gen, f = JET_OPS[op]
    jets = gen(np.random.default_rng(600 + sorted(JET_OPS).index(op)), N_JET)
    got = probe.run(op, *[a for j in jets for a in j])
    _jet_check(op, got, f, *jets)


def test_taylor_sincos(probe):
    rng = np.random.default_rng(620)
    jet = _jet_inputs(rng, rng.uniform(-4, 4, N_JET))
    out = probe.run('ty_sincos', *jet)
    _jet_check('ty_sincos sin', out[:3], lambda a: MP.sin(a), jet)
    _jet_check('ty_sincos cos', out[3:], lambda a: MP.cos(a), jet)


@pytest.mark.parametrize('p', [1.5, 2.0, 0.7])
def test_taylor_pow(probe, p):
    rng = np.random.default_rng(630)
    jet = _jet_inputs(rng, rng.uniform(1e-2, 4, N_JET))
    _jet_check(f'ty_pow {p}', probe.run('ty_pow', *jet, p=p), lambda a: a ** mpf(p), jet)


def test_taylor_abs(probe):
    """ty_abs is the jet itself or its negation, exactly; at the kink c0 = 0 it takes the -x branch, as ca.if_else(x > 0, x, -x)."""
    rng = np.random.default_rng(640)
    jet = _jet_inputs(rng, _away(rng, N_JET, 1e-2, 4))
    jet[0][:4] = (0.0, -0.0, 0.0, 2.0 ** -1022)
    got = probe.run('ty_abs', *jet)
    pos = jet[0] > 0
    for k in range(3):
        assert same_bits(got[k], np.where(pos, jet[k], -jet[k])), k
    assert not pos[0] and same_bits(got[1][:3], -jet[1][:3]) and same_bits(got[2][:3], -jet[2][:3]) and (got[0][:3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# track look-up
# ---------------------------------------------------------------------------------------------------------------------------------
def _track_points(rng, L, breaks, n_random):
    """random s in [-3 L, 3 L]; every breakpoint of every lap k in {-2 .. 2} +- 0, 1, 2 ulp (the seam s = k L among them)"""
    edges = np.array(sorted({float(k * L + b) for k in range(-2, 3) for b in breaks}))
    return np.concatenate([rng.uniform(-3 * L, 3 * L, n_random)] + [step(edges, k) for k in range(-2, 3)])


def _wrap(s, L):
    return mpf(s) - mpf(L) * MP.floor(mpf(s) / mpf(L))


def _near_break(s, sbar, breaks, L):
    """index of the breakpoint (breaks[0] = 0 .. breaks[-1] = L) the wrapped argument sits within one ulp of, else None.  The ulp is
    the spacing of doubles at max(|s|, L): wrap_s returns a double in [0, L) and cannot place s = -1e-323 (exactly: L - 1e-323) or
    s = 3 L - ulp(3 L) any finer than that, so there either neighbouring segment is a correct answer."""
    d, j = min((abs(sbar - mpf(b)), j) for j, b in enumerate(breaks))
    return j if d <= mpf(np.spacing(max(abs(float(s)), L))) else None


def _arc_truth(P, s, seg=None):
    """(sbar, segment, curvature, psi and its slope) of the plain piecewise function (radius_arclength_track.py:199-225): curvature
    piecewise constant, tangent piecewise linear with slopes that are doubles, sbar = s - L floor(s / L)"""
    L, n = mpf(P.track_L), P.n_segs
    sbar = mpf(s) - L * MP.floor(mpf(s) / L)
    if seg is None:
        seg = 0
        while seg + 1 < n and sbar >= mpf(P.seg_s[seg + 1]):
            seg += 1
    slope = (P.seg_ang[seg + 1] - P.seg_ang[seg]) / (P.seg_s[seg + 1] - P.seg_s[seg])
    return sbar, seg, P.seg_curv[seg], mpf(P.seg_ang[seg]) + mpf(slope) * (sbar - mpf(P.seg_s[seg])), slope


def _track_game(name):
    from dgsqp_amd import montecarlo as mc
    return {'curve': lambda: mc.kinematic_racing_game('curve', N=3), 'chicane': lambda: mc.kinematic_racing_game('chicane', N=3),
            'barc': lambda: mc.barc_racing_game(N=3)}[name]()


@pytest.mark.parametrize('name', ['curve', 'chicane', 'barc'])
def test_arc_track_lookup(name):
    """wrap_s and dev_track<2>.  Bars: curvature exact (a table entry); psi and its two coefficients to 1e-13 of the largest coefficient.
    Within 1 ulp of a breakpoint either neighbouring segment is accepted (_near_break; the quotient of wrap_s may be one ulp off at
    the seam)."""
    p = dmp.Probe(_track_game(name))
    try:
        P = p.problem
        L = P.track_L
        rng = np.random.default_rng(700)
        s = _track_points(rng, L, [P.seg_s[i] for i in range(P.n_segs)], 2000)
        c1, c2 = rng.uniform(-2, 2, len(s)), rng.uniform(-2, 2, len(s))
        w = p.run('wrap_s', s)
        curv, p0, p1, p2 = p.run('track', s, c1, c2)
    finally:
        p.close()
    assert (w >= 0).all() and (w < L).all(), (w.min(), w.max())
    n = P.n_segs
    breaks = [P.seg_s[i] for i in range(n + 1)]
    assert breaks[0] == 0.0 and breaks[-1] == L
    worst = wrap_worst = 0.0
    n_near = 0
    for i in range(len(s)):
        sbar, seg, *_ = _arc_truth(P, s[i])
        j = _near_break(s[i], sbar, breaks, L)
        cands = {seg} if j is None else {(j - 1) % n, j % n}
        n_near += j is not None
        wrap_err = min(abs(mpf(w[i]) - sbar - k * mpf(L)) for k in (-1, 0, 1))
        wrap_worst = max(wrap_worst, float(wrap_err / mpf(np.spacing(max(abs(s[i]), L)))))
        errs = []
        for sg in cands:
            # a neighbouring segment continues its own line: across the seam, sbar -+ L from the segment's start
            sb = sbar
            if sg == n - 1 and sbar < mpf(L) / 2:
                sb = sbar + mpf(L)
            if sg == 0 and sbar > mpf(L) / 2:
                sb = sbar - mpf(L)
            slope = (P.seg_ang[sg + 1] - P.seg_ang[sg]) / (P.seg_s[sg + 1] - P.seg_s[sg])
            want = [mpf(P.seg_ang[sg]) + mpf(slope) * (sb - mpf(P.seg_s[sg])), mpf(c1[i]) * mpf(slope), mpf(c2[i]) * mpf(slope)]
            tol = TRACK_BAR * max(abs(v) for v in want)
            e = max(abs(mpf(g) - v) for g, v in zip((p0[i], p1[i], p2[i]), want))
            ok = curv[i] == P.seg_curv[sg] and e <= tol
            errs.append((ok, float(e / tol) if tol else (0.0 if e == 0 else math.inf)))
        assert any(ok for ok, _ in errs), (name, s[i], j, curv[i], (p0[i], p1[i], p2[i]), sorted(cands), errs)
        worst = max(worst, min(r for ok, r in errs if ok))
    print(f'{name}: psi jet at most {worst:.3f} of its bar, wrap_s at most {wrap_worst:.3f} ulp of max(|s|, L) off, {n_near} of {len(s)} arguments on a breakpoint')
    assert wrap_worst <= 2.0 and n_near >= 5 * (n + 1)


def _spline_closed_form(coef, t0, c1, c2):
    """Taylor coefficients at t = 0 of the curvature kappa(u) = n / d^1.5 and the tangent angle psi(u) = atan2(y', x') of one cubic piece
    along u = t0 + c1 t + c2 t^2, by the chain rule (g0 = F, g1 = F' c1, g2 = F' c2 + F'' c1^2 / 2) from the derivatives written out:
    n = x' y'' - y' x'', d = x'^2 + y'^2, psi' = n / d.  Cheap enough for every knot; checked against mpmath.taylor in the test."""
    x1, x2, x3, y1, y2, y3 = coef                     # of u, u^2, u^3 in x and y, as mpf
    dx, dy = (3 * x3 * t0 + 2 * x2) * t0 + x1, (3 * y3 * t0 + 2 * y2) * t0 + y1
    ddx, ddy, d3x, d3y = 6 * x3 * t0 + 2 * x2, 6 * y3 * t0 + 2 * y2, 6 * x3, 6 * y3
    n, n1, n2 = dx * ddy - dy * ddx, dx * d3y - dy * d3x, ddx * d3y - ddy * d3x
    d, d1, d2 = dx * dx + dy * dy, 2 * (dx * ddx + dy * ddy), 2 * (ddx * ddx + dx * d3x + ddy * ddy + dy * d3y)
    r = MP.sqrt(d)
    k0 = n / (d * r)
    k1 = n1 / (d * r) - mpf(1.5) * n * d1 / (d * d * r)
    k2 = n2 / (d * r) - 3 * n1 * d1 / (d * d * r) - mpf(1.5) * n * d2 / (d * d * r) + mpf(3.75) * n * d1 * d1 / (d * d * d * r)
    p0, p1, p2 = MP.atan2(dy, dx), n / d, (n1 * d - n * d1) / (d * d)
    a, b = mpf(c1), mpf(c2)
    return [k0, k1 * a, k1 * b + k2 * a * a / 2], [p0, p1 * a, p1 * b + p2 * a * a / 2]


def test_spline_track_lookup():
    """dev_track_spline<2> on the F1 table: curvature (x' y'' - y' x'') / (x'^2 + y'^2)^1.5 and tangent atan2(y', x') of the piecewise
    cubics, both as jets, to 1e-11 of the largest coefficient.  300 random s in [-3 L, 3 L] against mpmath.taylor; every 32nd knot of
    the laps -2 .. 2, the seams and EVERY knot of lap 0 (the proportional-guess interval search of dev_track_spline has to land on
    each of them), each +- 0, 1, 2 ulp, against the derivatives written out (_spline_closed_form: mpmath.taylor costs a millisecond
    a point), which the random points tie to mpmath.taylor at 1e-40."""
    from dgsqp_amd.montecarlo import f1_racing_game
    p = dmp.Probe(f1_racing_game(N=5))
    try:
        P = p.problem
        tab, nk, L = P._spline_keepalive, P.n_knots, P.track_L
        kn, cx, cy = tab[:nk], tab[nk:nk + 4 * (nk - 1)].reshape(nk - 1, 4), tab[nk + 4 * (nk - 1):].reshape(nk - 1, 4)
        rng = np.random.default_rng(710)
        n_taylor = 300
        s = _track_points(rng, L, kn[:-1:32].tolist(), n_taylor)
        s = np.concatenate([s] + [step(kn, k) for k in range(-2, 3)])
        c1, c2 = rng.uniform(-2, 2, len(s)), rng.uniform(-2, 2, len(s))
        w = p.run('wrap_s', s)
        out = p.run('track_spline', s, c1, c2)
    finally:
        p.close()
    assert (w >= 0).all() and (w < L).all()

    assert kn[0] == 0.0 and kn[-1] == L

    worst = closed_worst = 0.0
    n_near = 0
    coefs = {}
    for j in range(len(s)):
        sbar = _wrap(s[j], L)
        i0 = min(max(int(np.searchsorted(kn, float(sbar), side='right')) - 1, 0), nk - 2)
        while i0 > 0 and sbar < mpf(kn[i0]):
            i0 -= 1
        while i0 < nk - 2 and sbar >= mpf(kn[i0 + 1]):
            i0 += 1
        lo = max(i0 - 1, 0)
        jb = _near_break(s[j], sbar, kn[lo:i0 + 3].tolist(), L)
        cands = {i0} if jb is None else {(lo + jb - 1) % (nk - 1), (lo + jb) % (nk - 1)}
        n_near += jb is not None
        best = math.inf
        for i in sorted(cands, key=lambda i: i != i0):      # the plain function's own segment first; the neighbour only if that fails
            if best <= 1.0:
                break
            sb = sbar
            if i == nk - 2 and sbar < mpf(L) / 2:
                sb = sbar + mpf(L)
            if i == 0 and sbar > mpf(L) / 2:
                sb = sbar - mpf(L)
            t0 = sb - mpf(kn[i])
            if i not in coefs:
                coefs[i] = [mpf(v) for v in (*cx[i][1:], *cy[i][1:])]
            wants = _spline_closed_form(coefs[i], t0, c1[j], c2[j])
            if j < n_taylor:
                x1, x2, x3, y1, y2, y3 = coefs[i]

                def derivs(t):
                    u = t0 + mpf(c1[j]) * t + mpf(c2[j]) * t * t
                    return (3 * x3 * u + 2 * x2) * u + x1, (3 * y3 * u + 2 * y2) * u + y1, 6 * x3 * u + 2 * x2, 6 * y3 * u + 2 * y2

                def curvature(t):
                    dx, dy, ddx, ddy = derivs(t)
                    return (dx * ddy - dy * ddx) / (dx * dx + dy * dy) ** mpf(1.5)

                def tangent(t):
                    dx, dy, _, _ = derivs(t)
                    return MP.atan2(dy, dx)

                taylor = [MP.taylor(curvature, 0, 2), MP.taylor(tangent, 0, 2)]
                for a, b in zip(wants, taylor):
                    closed_worst = max(closed_worst, float(max(abs(u - v) for u, v in zip(a, b)) / max(abs(v) for v in b)))
                wants = taylor
            rel = 0.0
            for want, got in zip(wants, (out[:3], out[3:])):
                tol = SPLINE_BAR * max(abs(v) for v in want)
                rel = max(rel, float(max(abs(mpf(g[j]) - v) for g, v in zip(got, want)) / tol))
            best = min(best, rel)
        assert best <= 1.0, (s[j], jb, sorted(cands), best)
        worst = max(worst, best)
    print(f'spline curvature and tangent jets: at most {worst:.3g} of their bar, {n_near} of {len(s)} arguments on a knot; '
          f'derivatives written out / mpmath.taylor: {closed_worst:.1e}')
    assert closed_worst < 1e-40 and n_near >= 3 * nk


# ---------------------------------------------------------------------------------------------------------------------------------
# DPP reductions
# ---------------------------------------------------------------------------------------------------------------------------------
def _tree_sum(v):
    """wave_sum's fixed tree on [.., 64] lanes, in its association order"""
    lane = np.arange(64)
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    v = v + v[..., (lane & ~7) | (7 - (lane & 7))]
    v = v + v[..., (lane & ~15) | (15 - (lane & 15))]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _block_tree_sum(v, block):
    r = _tree_sum(v.reshape(-1, block // 64, 64))
    t = np.zeros(len(r))
    for w in range(block // 64):
        t = t + r[:, w]
    return t


def _reduction_inputs(rng, groups, width):
    v = rng.choice((-1.0, 1.0), (groups, width)) * 2.0 ** rng.uniform(-30, 30, (groups, width))
    eq = np.full((1, width), -3.7)
    single = np.zeros((64, width))                     # one nonzero value in each of the 64 lane positions (block: in wavefront g % n_waves)
    for g in range(64):
        single[g, (64 * (g % (width // 64)) + g) % width] = -(1.0 + g) if g % 2 else 1.0 + g
    return np.concatenate([v, eq, single])


def _argmin_ref(v, idx):
    """lowest value, lowest index among equals"""
    out_v, out_i = np.empty(len(v)), np.empty(len(v))
    for g in range(len(v)):
        m = v[g].min()
        out_v[g], out_i[g] = m, idx[g][v[g] == m].min()
    return out_v, out_i


@pytest.mark.parametrize('scope', ['wave', 'block'])
def test_reductions(probe, scope):
    """sum: bit-identical to the fixed tree restated in numpy, within n 2^-53 sum|v| of math.fsum, uniform; max and argmin exact, lowest
    index on ties (2 and 64 equal minima, in different 16-lane rows and wavefronts).  NaN contract: one NaN lane makes the sums NaN,
    the max ignores it."""
    width = 64 if scope == 'wave' else probe.block
    rng = np.random.default_rng(800 + width)
    v = _reduction_inputs(rng, 40, width)
    G = len(v)
    uniform = lambda r: (bits(r.reshape(G, width)) == bits(r.reshape(G, width))[:, :1]).all()
    s = probe.run(f'{scope}_sum', v.ravel())
    assert uniform(s)
    want = _tree_sum(v) if scope == 'wave' else _block_tree_sum(v, width)
    assert same_bits(s.reshape(G, width)[:, 0], want)
    for g in range(G):
        assert abs(want[g] - math.fsum(v[g])) <= width * 2.0 ** -53 * np.abs(v[g]).sum()
    m = probe.run(f'{scope}_max', v.ravel())
    assert uniform(m) and same_bits(m.reshape(G, width)[:, 0], v.max(axis=1))
    # argmin: indices are the positions, then a permutation of them (the index travels with the value)
    ties = v[:40].copy()
    for g in range(40):
        lo = ties[g].min() - 1.0
        where = {0: [5, 37], 1: [17, 16], 2: [63, 0], 3: [width - 1, width // 2 + 3], 4: [width - 64 + 9, 70 % width]}.get(g % 8)
        if where is not None:
            ties[g, where] = lo
        elif g % 8 == 5:
            ties[g, rng.choice(width, 64, replace=False) if width > 64 else np.arange(64)] = lo
    va = np.concatenate([v, ties])
    for idx in (np.tile(np.arange(width, dtype=float), (len(va), 1)), np.array([rng.permutation(width) for _ in range(len(va))], dtype=float)):
        gv, gi = probe.run(f'{scope}_argmin', va.ravel(), idx.ravel())
        wv, wi = _argmin_ref(va, idx)
        gv, gi = gv.reshape(len(va), width), gi.reshape(len(va), width)
        if scope == 'wave':                                  # wave-uniform; block_argmin returns to every thread as well
            assert (gv == gv[:, :1]).all() and (gi == gi[:, :1]).all()
        assert same_bits(gv[:, 0], wv) and np.array_equal(gi[:, 0], wi), (scope, np.flatnonzero(gi[:, 0] != wi))
        assert (gv == gv[:, :1]).all() and (gi == gi[:, :1]).all()
    # NaN
    vn = v[:8].copy()
    pos = [0, 1, 15, 16, 31, 32, 47, width - 1]
    for g in range(8):
        vn[g, pos[g]] = np.nan
    clean = np.where(np.isnan(vn), -np.inf, vn).max(axis=1)
    assert np.isnan(probe.run(f'{scope}_sum', vn.ravel())).all()
    mn = probe.run(f'{scope}_max', vn.ravel()).reshape(8, width)
    assert same_bits(mn, np.repeat(clean[:, None], width, axis=1))
    assert np.isnan(probe.run(f'{scope}_max', np.full(width, np.nan))).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# DYN_BOTH: the single-wavefront mode of dev_rollout_dyn, which no game of the package reaches
# ---------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    F = fractions.Fraction
    return float(F(a) * F(b) + F(c))            # one rounding


@pytest.mark.parametrize('name', ['dyn_curve_N15', 'dyn_rk3_N10', 'dyn_rk2_N10'])
def test_single_wavefront_rollout_is_the_split_one(name):
    """dev_rollout_dyn<DYN_BOTH> against evaluate_batch's trajectory (the split modes DYN_VEL + DYN_POSE) on the four slow-branch
    scenarios of tests/test_split_rollout.py, rk4 (N = 15), rk3 and rk2 (N = 10): bit-identical, also at fma(0.37, du, u)."""
    import test_split_rollout as tsr
    from dgsqp_amd.solver import DGSQP, build_problem
    g = tsr._games()[name]()
    P = build_problem(*g.solver_args())
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u = tsr._slow_branch_points(g, P, s)
    rng = np.random.default_rng(900)
    du = 0.3 * rng.standard_normal(u.shape)
    alpha = 0.37
    ustep = np.array([[_fma(alpha, d, v) for v, d in zip(ub, db)] for ub, db in zip(u.tolist(), du.tolist())])
    ev, ev_step = s.evaluate_batch(x0, u), s.evaluate_batch(x0, ustep)
    p = dmp.Probe(g)
    try:
        for b in range(len(x0)):
            xb = p.rollout_both(x0[b], u[b])
            assert same_bits(xb.ravel(), np.asarray(ev['x'][b]).ravel()), (name, b, np.abs(xb.ravel() - np.asarray(ev['x'][b]).ravel()).max())
            xs = p.rollout_both(x0[b], u[b], du[b], alpha)
            assert same_bits(xs.ravel(), np.asarray(ev_step['x'][b]).ravel()), (name, b, 'stepped')
            assert not same_bits(xs, xb)
    finally:
        p.close()


def test_single_wavefront_rollout_known_answer():
    """... and against the exact trajectory of tests/golden/multistage_dyn2_rk4m3_N3.npz at the fixture's own tolerance."""
    import multistage_kat as mk
    kat, g, P = mk.load('dyn2_rk4m3_N3')
    p = dmp.Probe(g)
    try:
        for b in range(len(kat['x0'])):
            x = p.rollout_both(kat['x0'][b], kat['u'][b])
            want = kat['x'][b].reshape(x.shape)
            print('DYN_BOTH scenario', b, 'x', f'{mk.rel(x, want):.2e}')
            np.testing.assert_allclose(x, want, rtol=max(mk.X_RTOL, 64.0 * float(kat['sens_x'])), atol=mk.X_ATOL)
    finally:
        p.close()
