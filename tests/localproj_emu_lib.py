"""ctypes binding of tests/localproj_emu (TEST-ONLY host build of rsc_localproj.h: the sequential loop and the
kernel's fixed-point rounds over the same per-point functions, and the pieces the proofs of
tests/test_cpu_localproj.py enumerate)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import localproj_ref as lr
from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "localproj_emu")
LIB = os.path.join(DIR, "build", "liblocalproj_emu.so")
LIB_O3 = os.path.join(DIR, "build", "liblocalproj_emu_o3.so")
_libs = {}
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class Problem(C.Structure):
    """lpe_problem (localproj_emu.cpp)."""
    _fields_ = [("nf", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p),
                ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32)] + \
               [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "gw_inv", "gh_inv", "fx", "fy", "cx",
                                         "cy", "log_sf")] + \
               [("u_right", C.c_void_p), ("mbf", C.c_float),
                ("np", C.c_int32), ("state", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("dmax", C.c_void_p), ("dmin", C.c_void_p), ("pdesc", C.c_void_p), ("Tcw", C.c_void_p),
                ("skip", C.c_void_p), ("has_obs", C.c_void_p), ("frame_occ", C.c_void_p), ("track_in", C.c_void_p),
                ("cos_limit", C.c_float), ("th", C.c_float), ("nn_ratio", C.c_float), ("fused", C.c_int32)]


def lib(o3: bool = False):
    if o3 not in _libs:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB_O3 if o3 else LIB)
        L.lpe_search_sequential.argtypes = [C.POINTER(Problem), i32p, C.c_void_p, i32p]
        L.lpe_search_sequential.restype = None
        L.lpe_search_fixed_point.argtypes = [C.POINTER(Problem), i32p, C.c_void_p, i32p, C.POINTER(C.c_int32)]
        L.lpe_search_fixed_point.restype = None
        L.lpe_search_fixed_point_walks.argtypes = [C.POINTER(Problem), i32p, C.c_void_p, i32p, i32p]
        L.lpe_search_fixed_point_walks.restype = None
        L.lpe_top2.argtypes = [C.c_int, i32p, i32p, i32p]
        L.lpe_top2.restype = None
        L.lpe_accepts.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
        L.lpe_veto_bound.argtypes = [C.c_float]
        L.lpe_keep_max.argtypes = [C.c_float]
        L.lpe_radius.argtypes = [C.c_float]
        L.lpe_radius.restype = C.c_float
        _libs[o3] = L
    return _libs[o3]


def pack(p, track=None):
    """(lpe_problem, keep-alive arrays) for a problem namespace (tests/localproj_cases.py); with `track` the
    matcher-only mode on those records."""
    fr, pts = p.frame, p.pts

    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    keep = [arr(fr.kp, np.float32, 2), arr(fr.octave, np.int32, 1), arr(fr.desc, np.uint8, 32),
            arr(fr.cell_begin, np.int32, 1), arr(fr.cell_feat, np.int32, 1), synth.scale_factors(),
            arr(fr.u_right, np.float32, 1),
            arr(pts.state, np.uint8, 1), arr(pts.pos, np.float32, 3), arr(pts.normal, np.float32, 3),
            arr(pts.dmax, np.float32, 1), arr(pts.dmin, np.float32, 1), arr(pts.desc, np.uint8, 32),
            arr(p.Tcw, np.float32, 16), arr(p.skip, np.uint8, 1), arr(p.has_obs, np.uint8, 1),
            arr(p.frame_occ, np.uint8, 1)]
    q = Problem()
    q.nf, q.np = int(fr.n), int(pts.n)
    (q.kp, q.octave, q.desc, q.cell_begin, q.cell_feat, q.scale, q.u_right, q.state, q.pos, q.normal, q.dmax, q.dmin,
     q.pdesc, q.Tcw, q.skip, q.has_obs, q.frame_occ) = (a.ctypes.data for a in keep)
    q.n_levels = len(keep[5])
    q.min_x, q.max_x, q.min_y, q.max_y = fr.min_x, fr.max_x, fr.min_y, fr.max_y
    q.gw_inv, q.gh_inv = float(synth.GRID_W_INV), float(synth.GRID_H_INV)
    q.fx, q.fy, q.cx, q.cy = fr.fx, fr.fy, fr.cx, fr.cy
    q.log_sf = float(synth.LOG_SCALE_FACTOR)
    q.mbf = float(fr.mbf)
    q.cos_limit, q.th, q.nn_ratio = float(p.cos_limit), float(p.th), float(p.nn_ratio)
    q.fused = 1
    if track is not None:
        t = np.ascontiguousarray(track, lr.TRACK) if pts.n else np.zeros(1, lr.TRACK)
        keep.append(t)
        q.track_in = t.ctypes.data
        q.fused = 0
    return q, keep


def _run(p, track, fixed_point: bool, o3: bool = False):
    q, keep = pack(p, track)
    out = np.full(max(p.frame.n, 1), -7, np.int32)
    tr = np.zeros(max(p.pts.n, 1), lr.TRACK)
    counts = np.zeros(3, np.int32)
    walks = np.zeros(2, np.int32)  # all window walks, the most in one round
    if fixed_point:
        lib(o3).lpe_search_fixed_point_walks(C.byref(q), out, tr.ctypes.data, counts, walks)
    else:
        lib(o3).lpe_search_sequential(C.byref(q), out, tr.ctypes.data, counts)
    return dict(out=out[:p.frame.n], track=tr[:p.pts.n], nmatches=int(counts[0]), n_to_match=int(counts[1]),
                rounds=int(counts[2]), walks=int(walks[0]), max_round_walks=int(walks[1]))


def search_sequential(p, track=None, o3: bool = False):
    """The literal sequential loop over the kernel's per-point functions (fused, or matcher-only on `track`)."""
    return _run(p, track, False, o3)


def search_fixed_point(p, track=None):
    """The rounds as the kernel runs them."""
    return _run(p, track, True)


def top2(dist, level):
    res = np.zeros(5, np.int32)
    lib().lpe_top2(len(dist), np.ascontiguousarray(dist, np.int32).reshape(-1) if len(dist) else np.zeros(1, np.int32),
                   np.ascontiguousarray(level, np.int32).reshape(-1) if len(dist) else np.zeros(1, np.int32), res)
    return tuple(int(v) for v in res)
