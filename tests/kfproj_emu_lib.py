"""ctypes binding of tests/kfproj_emu (TEST-ONLY host build of rsc_kfproj.h and rsc_sim3compose.h: the
sequential loop and the kernel's fixed-point rounds over the same per-point functions, Fuse, and the Sim3
composition of LoopClosing.cpp:318-320)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "kfproj_emu")
LIB = os.path.join(DIR, "build", "libkfproj_emu.so")
_lib = None
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


class Problem(C.Structure):
    """kfpe_problem (kfproj_emu.cpp)."""
    _fields_ = [("nk", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p),
                ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32)] + \
               [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "gw_inv", "gh_inv", "fx", "fy", "cx",
                                         "cy", "log_sf")] + \
               [("np", C.c_int32), ("state", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("dmax", C.c_void_p), ("dmin", C.c_void_p), ("pdesc", C.c_void_p), ("Scw", C.c_void_p),
                ("skip", C.c_void_p), ("occupied", C.c_void_p), ("th", C.c_float)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB)
        L.kfpe_search_sequential.argtypes = [C.POINTER(Problem), i32p]
        L.kfpe_search_fixed_point.argtypes = [C.POINTER(Problem), i32p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.kfpe_fuse.argtypes = [C.POINTER(Problem), i32p]
        L.kfpe_compose.argtypes = [C.c_int, f64p, f32p, f32p, f64p, f32p]
        L.kfpe_compose.restype = None
        _lib = L
    return _lib


def pack(kf, pts, Scw, skip, occupied, th):
    """(kfpe_problem, keep-alive arrays)."""
    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    keep = [arr(kf.kp, np.float32, 2), arr(kf.octave, np.int32, 1), arr(kf.desc, np.uint8, 32),
            arr(kf.cell_begin, np.int32, 1), arr(kf.cell_feat, np.int32, 1), synth.scale_factors(),
            arr(pts.state, np.uint8, 1), arr(pts.pos, np.float32, 3), arr(pts.normal, np.float32, 3),
            arr(pts.dmax, np.float32, 1), arr(pts.dmin, np.float32, 1), arr(pts.desc, np.uint8, 32),
            arr(Scw, np.float32, 16), arr(skip, np.uint8, 1),
            arr(occupied if occupied is not None else np.zeros(kf.n, np.uint8), np.uint8, 1)]
    p = Problem()
    p.nk, p.np = int(kf.n), int(pts.n)
    (p.kp, p.octave, p.desc, p.cell_begin, p.cell_feat, p.scale, p.state, p.pos, p.normal, p.dmax, p.dmin, p.pdesc,
     p.Scw, p.skip, p.occupied) = (a.ctypes.data for a in keep)
    p.n_levels = len(keep[5])
    p.min_x, p.max_x, p.min_y, p.max_y = kf.min_x, kf.max_x, kf.min_y, kf.max_y
    p.gw_inv, p.gh_inv = float(synth.GRID_W_INV), float(synth.GRID_H_INV)
    p.fx, p.fy, p.cx, p.cy = kf.fx, kf.fy, kf.cx, kf.cy
    p.log_sf = float(synth.LOG_SCALE_FACTOR)
    p.th = float(th)
    return p, keep


def search_sequential(kf, pts, Scw, already, occupied, th):
    """(nmatches, out int32[kf.n]) of the literal sequential loop over the kernel's per-point functions."""
    p, keep = pack(kf, pts, Scw, already, occupied, th)
    out = np.full(max(kf.n, 1), -7, np.int32)
    n = lib().kfpe_search_sequential(C.byref(p), out)
    return n, out[:kf.n]


def search_fixed_point(kf, pts, Scw, already, occupied, th):
    """(nmatches, out int32[kf.n], rounds, fallback window walks) of the rounds as the kernel runs them."""
    p, keep = pack(kf, pts, Scw, already, occupied, th)
    out = np.full(max(kf.n, 1), -7, np.int32)
    r, w = C.c_int32(), C.c_int32()
    n = lib().kfpe_search_fixed_point(C.byref(p), out, C.byref(r), C.byref(w))
    return n, out[:kf.n], r.value, w.value


def fuse(kf, pts, Scw, in_kf, th):
    """(nfused, best_idx int32[pts.n])."""
    p, keep = pack(kf, pts, Scw, in_kf, None, th)
    best = np.full(max(pts.n, 1), -7, np.int32)
    n = lib().kfpe_fuse(C.byref(p), best)
    return n, best[:pts.n]


def compose(S_cm, R_mw, t_mw):
    """(S_cw float64 [count,8], T float32 [count,16]) of the host build of rsc_sim3compose.h."""
    S_cm = np.ascontiguousarray(S_cm, np.float64).reshape(-1, 8)
    c = len(S_cm)
    R = np.ascontiguousarray(R_mw, np.float32).reshape(c, 9)
    t = np.ascontiguousarray(t_mw, np.float32).reshape(c, 3)
    S_cw = np.zeros((c, 8), np.float64)
    T = np.zeros((c, 16), np.float32)
    lib().kfpe_compose(c, S_cm, R, t, S_cw, T)
    return S_cw, T
