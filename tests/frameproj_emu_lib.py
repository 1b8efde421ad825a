"""ctypes binding of tests/frameproj_emu (TEST-ONLY host build of rsc_frameproj.h: the sequential loop
and the kernel's fixed-point rounds over the same per-MapPoint functions)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "frameproj_emu", "build", "libframeproj_emu.so")
_lib = None
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class Problem(C.Structure):
    """fpe_problem (frameproj_emu.cpp)."""
    _fields_ = [("nf", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("desc", C.c_void_p), ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32)] + \
               [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "gw_inv", "gh_inv", "fx", "fy", "cx",
                                         "cy", "log_sf")] + \
               [("nk", C.c_int32), ("mp_state", C.c_void_p), ("mp_pos", C.c_void_p), ("mp_dmax", C.c_void_p),
                ("mp_dmin", C.c_void_p), ("mp_desc", C.c_void_p), ("kf_angle", C.c_void_p), ("Tcw", C.c_void_p),
                ("already", C.c_void_p), ("frame_mp", C.c_void_p), ("th", C.c_float), ("orb_dist", C.c_int32),
                ("check_orientation", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "frameproj_emu")])
        L = C.CDLL(LIB)
        L.fpe_search_sequential.argtypes = [C.POINTER(Problem), i32p]
        L.fpe_search_fixed_point.argtypes = [C.POINTER(Problem), i32p, C.POINTER(C.c_int32)]
        _lib = L
    return _lib


def pack(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation=True):
    """(fpe_problem, keep-alive arrays)."""
    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    keep = [arr(F.kp, np.float32, 2), arr(F.octave, np.int32, 1), arr(F.angle, np.float32, 1),
            arr(F.desc, np.uint8, 32), arr(F.cell_begin, np.int32, 1), arr(F.cell_feat, np.int32, 1),
            synth.scale_factors(), arr(kf.mp_state, np.uint8, 1), arr(kf.mp_pos, np.float32, 3),
            arr(kf.mp_dmax, np.float32, 1), arr(kf.mp_dmin, np.float32, 1), arr(kf.mp_desc, np.uint8, 32),
            arr(kf.angle, np.float32, 1), arr(Tcw, np.float32, 16), arr(already, np.uint8, 1),
            arr(frame_mp, np.int32, 1)]
    p = Problem()
    p.nf, p.nk = int(F.n), int(kf.n)
    (p.kp, p.octave, p.angle, p.desc, p.cell_begin, p.cell_feat, p.scale, p.mp_state, p.mp_pos, p.mp_dmax,
     p.mp_dmin, p.mp_desc, p.kf_angle, p.Tcw, p.already, p.frame_mp) = (a.ctypes.data for a in keep)
    p.n_levels = len(keep[6])
    p.min_x, p.max_x, p.min_y, p.max_y = F.min_x, F.max_x, F.min_y, F.max_y
    p.gw_inv, p.gh_inv = float(synth.GRID_W_INV), float(synth.GRID_H_INV)
    p.fx, p.fy, p.cx, p.cy = F.fx, F.fy, F.cx, F.cy
    p.log_sf = float(synth.LOG_SCALE_FACTOR)
    p.th, p.orb_dist, p.check_orientation = float(th), int(orb_dist), int(bool(check_orientation))
    return p, keep


def search_sequential(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation=True):
    """(nmatches, out int32[F.n]) of the literal sequential loop over the kernel's per-point functions."""
    p, keep = pack(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation)
    out = np.full(max(F.n, 1), -7, np.int32)
    n = lib().fpe_search_sequential(C.byref(p), out)
    return n, out[:F.n]


def search_fixed_point(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation=True):
    """(nmatches, out int32[F.n], rounds) of the rounds as the kernel runs them."""
    p, keep = pack(F, kf, Tcw, already, frame_mp, th, orb_dist, check_orientation)
    out = np.full(max(F.n, 1), -7, np.int32)
    r = C.c_int32()
    n = lib().fpe_search_fixed_point(C.byref(p), out, C.byref(r))
    return n, out[:F.n], r.value
