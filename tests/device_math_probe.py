"""Helper of tests/test_device_math.py: builds and drives the probe library tests/csrc/libdgsqp_math_probe.so (test infrastructure,
never loaded by the product).

The probe (tests/csrc/device_math_probe.hip) is the product's own dgsqp_api.hip plus one-workgroup kernels that apply one device
primitive of csrc/dgsqp_device.h / csrc/dgsqp_eval.h elementwise.  ``Probe(game)`` makes a handle with the library's own
``dgsqp_create`` from the problem record the package builds for that game, so the constant block, the atan table and the track tables
the primitives read are written by the product's code.

Element e of an array runs on lane ``e % 64`` of some wavefront together with the other elements of its aligned group of 64: callers
that care which inputs share a wavefront (the wave-uniform fast paths, the reductions) lay their arrays out in groups of 64."""
import ctypes as C
import os
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent
SRC = HERE / 'csrc' / 'device_math_probe.hip'
OUT = HERE / 'csrc' / 'libdgsqp_math_probe.so'
PRODUCT_CSRC = ROOT / 'dgsqp_amd' / 'csrc'

# op codes and (planes in, planes out) of tests/csrc/device_math_probe.hip
OPS = {name: (i, nin, nout) for i, (name, nin, nout) in enumerate([
    ('rcp', 1, 1), ('sincos', 1, 2), ('tan', 1, 1), ('atan', 1, 1), ('atan2', 2, 1), ('roll_atan', 1, 1), ('roll_atan2', 2, 1),
    ('roll_sin', 1, 1), ('roll_sincos', 1, 2),
    ('ty_recip', 3, 3), ('ty_mul', 6, 3), ('ty_div', 6, 3), ('ty_sincos', 3, 6), ('ty_tan', 3, 3), ('ty_atan', 3, 3), ('ty_atan2', 6, 3),
    ('ty_sqrt', 3, 3), ('ty_pow', 3, 3), ('ty_abs', 3, 3),
    ('wrap_s', 1, 1), ('track', 3, 4), ('track_spline', 3, 6),
    ('wave_sum', 1, 1), ('wave_max', 1, 1), ('wave_argmin', 2, 2), ('block_sum', 1, 1), ('block_max', 1, 1), ('block_argmin', 2, 2)])}


def _deps(csrc):
    from dgsqp_amd.csrc.build import DEPS
    return [SRC] + [pathlib.Path(csrc) / d.name if d.parent == PRODUCT_CSRC else d for d in DEPS]


def build(force=False, csrc=PRODUCT_CSRC, out=OUT):
    """Compile the probe for gfx950 with the flags of dgsqp_amd/csrc/build.py (cross-compiles without a GPU); nothing to do when the
    library is newer than the probe source and every header the product library depends on.  ``csrc``: the directory dgsqp_api.hip
    and its headers are taken from (another revision's, to compare two revisions of a primitive bit by bit)."""
    out = pathlib.Path(out)
    if not force and out.exists() and out.stat().st_mtime >= max(d.stat().st_mtime for d in _deps(csrc)):
        return out
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC', '-I', str(csrc), '-I', str(ROOT / 'include'),
           '-o', str(out), str(SRC)]
    subprocess.check_call(cmd, cwd=str(SRC.parent))
    return out


_LIBS = {}


def load(path=None):
    """The probe library: ``path``, else the file ``DGSQP_MATH_PROBE_LIB`` names (a probe built from another revision of the headers),
    else the in-tree build, refreshed when stale."""
    env = os.environ.get('DGSQP_MATH_PROBE_LIB')
    path = pathlib.Path(path) if path else (pathlib.Path(env).resolve() if env else build())
    if path in _LIBS:
        return _LIBS[path]
    from dgsqp_amd import _ffi
    lib = C.CDLL(str(path))
    H, PD = C.c_void_p, C.POINTER(C.c_double)
    lib.dgsqp_create.argtypes = [C.POINTER(_ffi.ProblemT), C.POINTER(_ffi.ParamsT), C.c_int, C.POINTER(H)]
    lib.dgsqp_create.restype = C.c_int
    lib.dgsqp_destroy.argtypes = [H]
    lib.dgsqp_destroy.restype = None
    lib.dgsqp_last_error.argtypes = [H]
    lib.dgsqp_last_error.restype = C.c_char_p
    lib.dgsqp_probe_block.argtypes = []
    lib.dgsqp_probe_block.restype = C.c_int
    lib.dgsqp_probe_run.argtypes = [H, C.c_int, C.c_int64, C.c_int, PD, C.c_int, PD, C.c_double]
    lib.dgsqp_probe_run.restype = C.c_int
    lib.dgsqp_probe_rollout_both.argtypes = [H, PD, PD, PD, C.c_double, PD]
    lib.dgsqp_probe_rollout_both.restype = C.c_int
    _LIBS[path] = lib
    return lib


class Probe:
    """A handle of the probe library for ``game`` (a dgsqp_amd.game.Game)."""

    def __init__(self, game, lib_path=None):
        from dgsqp_amd.solver import build_params, build_problem
        self.lib = load(lib_path)
        self.problem = build_problem(*game.solver_args())
        self.params = build_params(game.params, qp_method='active_set')
        self.block = int(self.lib.dgsqp_probe_block())
        self._h = C.c_void_p()
        rc = self.lib.dgsqp_create(C.byref(self.problem), C.byref(self.params), 0, C.byref(self._h))
        if rc != 0:
            msg = self.lib.dgsqp_last_error(None)
            raise RuntimeError(f'dgsqp_create (probe library) failed ({rc}): {msg.decode() if msg else ""}')

    def close(self):
        if self._h:
            self.lib.dgsqp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fail(self, what, rc):
        raise RuntimeError(f'{what} failed ({rc}): {self.lib.dgsqp_last_error(self._h).decode()}')

    def run(self, op, *inputs, p=0.0):
        """Apply ``op`` to the equally long 1-d arrays ``inputs``; returns the tuple of output arrays (one array where the op has one
        output).  Arrays whose length is no multiple of 64 are padded with copies of their last element (block reductions: the
        length must be a multiple of ``self.block``)."""
        code, nin, nout = OPS[op]
        assert len(inputs) == nin, (op, len(inputs), nin)
        arrs = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in inputs]
        n = len(arrs[0])
        assert n > 0 and all(len(a) == n for a in arrs)
        npad = -n % 64
        buf = np.empty((nin, n + npad))
        for j, a in enumerate(arrs):
            buf[j, :n] = a
            buf[j, n:] = a[-1]
        out = np.empty((nout, n + npad))
        PD = C.POINTER(C.c_double)
        rc = self.lib.dgsqp_probe_run(self._h, code, n + npad, nin, buf.ctypes.data_as(PD), nout, out.ctypes.data_as(PD), float(p))
        if rc != 0:
            self._fail(f'probe op {op}', rc)
        res = tuple(out[j, :n].copy() for j in range(nout))
        return res[0] if nout == 1 else res

    def rollout_both(self, x0, u, du=None, alpha=0.0):
        """Trajectory [(N + 1), n_q] of dev_rollout_dyn<DYN_BOTH> from ``x0`` under the agent-major inputs ``u`` (or fma(alpha, du, u))."""
        PD = C.POINTER(C.c_double)
        P = self.problem
        nq = 8 * P.M
        x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
        u = np.ascontiguousarray(u, dtype=np.float64).ravel()
        assert len(x0) == nq and len(u) == 2 * P.M * P.N
        if du is not None:
            du = np.ascontiguousarray(du, dtype=np.float64).ravel()
            assert len(du) == len(u)
        x = np.empty((P.N + 1, nq))
        rc = self.lib.dgsqp_probe_rollout_both(self._h, x0.ctypes.data_as(PD), u.ctypes.data_as(PD),
                                               du.ctypes.data_as(PD) if du is not None else None, float(alpha), x.ctypes.data_as(PD))
        if rc != 0:
            self._fail('probe rollout', rc)
        return x
