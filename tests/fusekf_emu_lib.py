"""ctypes binding of tests/fusekf_emu (TEST-ONLY host build of rsc_fusekf.h: the sequential loop over the kernel's
per-pair function, and the 16-lane window walk restated lane after lane)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "fusekf_emu")
LIB = os.path.join(DIR, "build", "libfusekf_emu.so")
_lib = None
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


class Problem(C.Structure):
    """fkfe_problem (fusekf_emu.cpp)."""
    _fields_ = [("nk", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p),
                ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32)] + \
               [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "gw_inv", "gh_inv", "fx", "fy", "cx",
                                         "cy", "log_sf")] + \
               [("u_right", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("mbf", C.c_float), ("np", C.c_int32), ("state", C.c_void_p), ("pos", C.c_void_p),
                ("normal", C.c_void_p), ("dmax", C.c_void_p), ("dmin", C.c_void_p), ("pdesc", C.c_void_p),
                ("skip", C.c_void_p), ("th", C.c_float)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB)
        L.fkfe_fuse.argtypes = [C.POINTER(Problem), i32p]
        L.fkfe_fuse_coop.argtypes = [C.POINTER(Problem), C.c_int, i32p]
        L.fkfe_inv_sigma2.argtypes = [f32p, C.c_int, f32p]
        L.fkfe_inv_sigma2.restype = None
        _lib = L
    return _lib


def pack(kf, pts, skip, th):
    """(fkfe_problem, keep-alive arrays)."""
    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    sf, log_sf, gw, gh = synth.kf_geometry(kf)
    keep = [arr(kf.kp, np.float32, 2), arr(kf.octave, np.int32, 1), arr(kf.desc, np.uint8, 32),
            arr(kf.cell_begin, np.int32, 1), arr(kf.cell_feat, np.int32, 1), sf, arr(kf.u_right, np.float32, 1),
            arr(pts.state, np.uint8, 1), arr(pts.pos, np.float32, 3), arr(pts.normal, np.float32, 3),
            arr(pts.dmax, np.float32, 1), arr(pts.dmin, np.float32, 1), arr(pts.desc, np.uint8, 32),
            arr(skip, np.uint8, 1)]
    p = Problem()
    p.nk, p.np = int(kf.n), int(pts.n)
    (p.kp, p.octave, p.desc, p.cell_begin, p.cell_feat, p.scale, p.u_right, p.state, p.pos, p.normal, p.dmax, p.dmin,
     p.pdesc, p.skip) = (a.ctypes.data for a in keep)
    p.n_levels = len(sf)
    p.min_x, p.max_x, p.min_y, p.max_y = kf.min_x, kf.max_x, kf.min_y, kf.max_y
    p.gw_inv, p.gh_inv = float(gw), float(gh)
    p.fx, p.fy, p.cx, p.cy = kf.fx, kf.fy, kf.cx, kf.cy
    p.log_sf = float(log_sf)
    p.Rcw[:] = [float(v) for v in np.asarray(kf.Rcw, np.float32).reshape(9)]
    p.tcw[:] = [float(v) for v in np.asarray(kf.tcw, np.float32).reshape(3)]
    p.Ow[:] = [float(v) for v in np.asarray(kf.Ow, np.float32).reshape(3)]
    p.mbf = float(kf.mbf)
    p.th = float(th)
    return p, keep


def fuse(kf, pts, skip, th, lanes: int = 0):
    """(nfused, best_idx int32[pts.n]) of the sequential loop (lanes = 0) or of the `lanes`-lane window walk."""
    p, keep = pack(kf, pts, skip, th)
    best = np.full(max(pts.n, 1), -7, np.int32)
    n = lib().fkfe_fuse_coop(C.byref(p), lanes, best) if lanes else lib().fkfe_fuse(C.byref(p), best)
    return n, best[:pts.n]


def inv_sigma2(sf):
    sf = np.ascontiguousarray(sf, np.float32)
    out = np.zeros(len(sf), np.float32)
    lib().fkfe_inv_sigma2(sf, len(sf), out)
    return out
