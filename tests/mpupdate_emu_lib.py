"""ctypes binding of tests/mpupdate_emu (TEST-ONLY host build of rsc_mpupdate.h: the sequential restatement, and the
kernels' lane decompositions with the lanes run one after another)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import mpupdate_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "mpupdate_emu")
LIB = os.path.join(DIR, "build", "libmpupdate_emu.so")
_lib = None


class KF(C.Structure):
    """mpue_kf (mpupdate_emu.cpp)."""
    _fields_ = [("n", C.c_int32), ("desc", C.c_void_p), ("octave", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32), ("Ow", C.c_float * 3)]


class Problem(C.Structure):
    """mpue_problem (mpupdate_emu.cpp)."""
    _fields_ = [("n_kfs", C.c_int32), ("kfs", C.POINTER(KF)), ("kf_bad", C.c_void_p), ("n_points", C.c_int32),
                ("skip", C.c_void_p), ("pos", C.c_void_p), ("obs_begin", C.c_void_p), ("obs_kf", C.c_void_p),
                ("obs_idx", C.c_void_p), ("ref_kf", C.c_void_p), ("ref_idx", C.c_void_p)]


class Out(C.Structure):
    """mpue_out (mpupdate_emu.cpp)."""
    _fields_ = [("desc", C.c_void_p), ("best_obs", C.c_void_p), ("normal", C.c_void_p), ("dmax", C.c_void_p),
                ("dmin", C.c_void_p), ("updated", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB)
        L.mpue_update.argtypes = [C.POINTER(Problem), C.c_int, C.c_int, C.POINTER(Out)]
        L.mpue_medians.argtypes = [C.POINTER(Problem), C.c_int, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
        _lib = L
    return _lib


def pack(problem):
    """(mpue_problem, keep-alive objects)."""
    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    u = problem.upd
    keep = []
    kfs = (KF * max(len(problem.kfs), 1))()
    for k, v in enumerate(problem.kfs):
        a = [arr(v.desc, np.uint8, 32), arr(v.octave, np.int32, 1), arr(v.scale, np.float32, 1)]
        keep += a
        kfs[k].n, kfs[k].n_levels = int(v.n), len(v.scale)
        kfs[k].desc, kfs[k].octave, kfs[k].scale = (x.ctypes.data for x in a)
        kfs[k].Ow[:] = [float(x) for x in np.asarray(v.Ow, np.float32)]
    m = max(int(u.n_points), 1)
    a = [arr(u.skip, np.uint8, m), arr(u.pos, np.float32, 3 * m), arr(u.obs_begin, np.int32, m + 1),
         arr(u.obs_kf, np.int32, 1), arr(u.obs_idx, np.int32, 1), arr(u.ref_kf, np.int32, m), arr(u.ref_idx, np.int32, m)]
    p = Problem()
    p.n_kfs, p.kfs, p.n_points = len(problem.kfs), kfs, int(u.n_points)
    p.skip, p.pos, p.obs_begin, p.obs_kf, p.obs_idx, p.ref_kf, p.ref_idx = (x.ctypes.data for x in a)
    if u.kf_bad is not None:
        bad = arr(u.kf_bad, np.uint8, 1)
        a.append(bad)
        p.kf_bad = bad.ctypes.data
    return p, keep + a + [kfs]


def update(problem, what: int = 3, mode: int = 1):
    """mpue_update: the result dict of mpupdate_ref.update (unwritten entries hold its FILL), or None when the call
    is refused (a list longer than the limit)."""
    p, keep = pack(problem)
    n = max(p.n_points, 1)
    F = mr.FILL
    res = dict(desc=np.full((n, 32), F["desc"], np.uint8), best_obs=np.full(n, F["best_obs"], np.int32),
               normal=np.full((n, 3), F["normal"], np.float32), dmax=np.full(n, F["dmax"], np.float32),
               dmin=np.full(n, F["dmin"], np.float32), updated=np.full(n, 0xFF, np.uint8))
    o = Out()
    for k, a in res.items():
        setattr(o, k, a.ctypes.data)
    if lib().mpue_update(C.byref(p), what, mode, C.byref(o)) != 0:
        assert (res["updated"] == 0xFF).all()
        return None
    return {k: a[:p.n_points] for k, a in res.items()}


def medians(problem, point: int):
    """mpu_row_median of the kept rows of one point."""
    p, keep = pack(problem)
    out = np.zeros(max(int(problem.upd.obs_begin[point + 1] - problem.upd.obs_begin[point]), 1), np.int32)
    n = lib().mpue_medians(C.byref(p), point, out)
    return out[:n].tolist()
