"""ctypes binding of tests/stereo_emu (TEST-ONLY host build of rsc_stereo.h: the sequential path written like the
reference, and the kernels' tile / wave / lane / chunk decomposition with the lanes run one after another)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "stereo_emu")
LIB = os.path.join(DIR, "build", "libstereo_emu.so")
MAIN = os.path.join(DIR, "build", "stereo_emu_main")
MAIN_SAN = os.path.join(DIR, "build", "stereo_emu_main_san")
_lib = None


class Frame(C.Structure):
    """stme_frame (stereo_emu.cpp)."""
    _fields_ = [("n_left", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p),
                ("scale", C.c_void_p), ("n_levels", C.c_int32), ("n_right", C.c_int32), ("r_kp", C.c_void_p),
                ("r_octave", C.c_void_p), ("r_desc", C.c_void_p), ("mbf", C.c_float), ("mb", C.c_float)]


class Result(C.Structure):
    """StereoOut (rsc_stereo.h) = rsc_stereo_result."""
    _fields_ = [("n_candidates", C.c_int32), ("n_removed", C.c_int32), ("median", C.c_int32), ("th_dist", C.c_float)]


class Out(C.Structure):
    """stme_out (stereo_emu.cpp)."""
    _fields_ = [("u_right", C.c_void_p), ("depth", C.c_void_p), ("best_right", C.c_void_p), ("best_dist", C.c_void_p),
                ("result", C.POINTER(Result))]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB)
        L.stme_compute.argtypes = [C.POINTER(Frame), C.c_int, C.POINTER(Out)]
        L.stme_order.argtypes = [C.c_float]
        L.stme_order.restype = C.c_uint32
        _lib = L
    return _lib


def pack(fr):
    """(stme_frame, keep-alive arrays) of a stereo_ref frame."""
    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    keep = [arr(fr.kp, np.float32, 2), arr(fr.octave, np.int32, 1), arr(fr.desc, np.uint8, 32),
            arr(fr.scale, np.float32, 1), arr(fr.r_kp, np.float32, 2), arr(fr.r_octave, np.int32, 1),
            arr(fr.r_desc, np.uint8, 32)]
    f = Frame()
    f.n_left, f.n_levels, f.n_right = len(fr.kp), len(fr.scale), len(fr.r_kp)
    f.kp, f.octave, f.desc, f.scale, f.r_kp, f.r_octave, f.r_desc = (a.ctypes.data for a in keep)
    f.mbf, f.mb = float(fr.mbf), float(fr.mb)
    return f, keep


def compute(fr, mode: int = 1, repeat: int = 1):
    """stme_compute: the result dict of stereo_ref.compute, or None when the frame is refused."""
    f, keep = pack(fr)
    n = max(f.n_left, 1)
    u, z = np.full(n, -77.0, np.float32), np.full(n, -77.0, np.float32)
    br, bd = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    res = Result(-9, -9, -9, -9.0)
    o = Out(u.ctypes.data, z.ctypes.data, br.ctypes.data, bd.ctypes.data, C.pointer(res))
    L = lib()
    for _ in range(repeat):
        if L.stme_compute(C.byref(f), mode, C.byref(o)) != 0:
            assert (u == -77.0).all() and res.median == -9
            return None
    k = f.n_left
    return dict(u_right=u[:k], depth=z[:k], best_right=br[:k], best_dist=bd[:k], n_candidates=res.n_candidates,
                n_removed=res.n_removed, median=res.median, th_dist=np.float32(res.th_dist))
