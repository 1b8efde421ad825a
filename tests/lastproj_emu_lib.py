"""ctypes binding of tests/lastproj_emu (TEST-ONLY host build of rsc_lastproj.h: the sequential loop and the
kernel's fixed-point rounds over the same per-point functions)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from rsc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "lastproj_emu")
LIB = os.path.join(DIR, "build", "liblastproj_emu.so")
LIB_O3 = os.path.join(DIR, "build", "liblastproj_emu_o3.so")
MAIN = os.path.join(DIR, "build", "lastproj_emu_main")
MAIN_SAN = os.path.join(DIR, "build", "lastproj_emu_main_san")
_libs = {}
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


class Problem(C.Structure):
    """lse_problem (lastproj_emu.cpp)."""
    _fields_ = [("nf", C.c_int32), ("kp", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("desc", C.c_void_p), ("cell_begin", C.c_void_p), ("cell_feat", C.c_void_p), ("scale", C.c_void_p),
                ("n_levels", C.c_int32)] + \
               [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "gw_inv", "gh_inv", "fx", "fy", "cx",
                                         "cy", "log_sf")] + \
               [("u_right", C.c_void_p), ("mbf", C.c_float),
                ("nl", C.c_int32), ("l_octave", C.c_void_p), ("l_angle", C.c_void_p), ("mp_state", C.c_void_p),
                ("mp_pos", C.c_void_p), ("mp_desc", C.c_void_p), ("mp_has_obs", C.c_void_p),
                ("Tcw_cur", C.c_void_p), ("Tcw_last", C.c_void_p), ("mb", C.c_float), ("frame_occ", C.c_void_p),
                ("th", C.c_float), ("check_ori", C.c_int32)]


def build():
    subprocess.check_call(["make", "-s", "-C", DIR])


def lib(o3: bool = False):
    if o3 not in _libs:
        build()
        L = C.CDLL(LIB_O3 if o3 else LIB)
        L.lse_search_sequential.argtypes = [C.POINTER(Problem), i32p, i32p]
        L.lse_search_sequential.restype = None
        L.lse_search_fixed_point.argtypes = [C.POINTER(Problem), i32p, i32p, C.POINTER(C.c_int32)]
        L.lse_search_fixed_point.restype = None
        L.lse_search_fixed_point_walks.argtypes = [C.POINTER(Problem), i32p, i32p, i32p]
        L.lse_search_fixed_point_walks.restype = None
        L.lse_mode.argtypes = [f32p, f32p, C.c_float]
        _libs[o3] = L
    return _libs[o3]


def pack(p):
    """(lse_problem, keep-alive arrays) for a problem namespace (tests/lastproj_cases.py)."""
    fr, last = p.frame, p.last

    def arr(a, dt, pad):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        return a if a.size else np.zeros(pad, dt)
    keep = [arr(fr.kp, np.float32, 2), arr(fr.octave, np.int32, 1), arr(fr.angle, np.float32, 1),
            arr(fr.desc, np.uint8, 32), arr(fr.cell_begin, np.int32, 1), arr(fr.cell_feat, np.int32, 1),
            synth.scale_factors(), arr(fr.u_right, np.float32, 1),
            arr(last.octave, np.int32, 1), arr(last.angle, np.float32, 1), arr(last.mp_state, np.uint8, 1),
            arr(last.mp_pos, np.float32, 3), arr(last.mp_desc, np.uint8, 32), arr(last.mp_has_obs, np.uint8, 1),
            arr(p.Tcw_cur, np.float32, 16), arr(p.Tcw_last, np.float32, 16), arr(p.frame_occ, np.uint8, 1)]
    q = Problem()
    q.nf, q.nl = int(fr.n), int(last.n)
    (q.kp, q.octave, q.angle, q.desc, q.cell_begin, q.cell_feat, q.scale, q.u_right, q.l_octave, q.l_angle,
     q.mp_state, q.mp_pos, q.mp_desc, q.mp_has_obs, q.Tcw_cur, q.Tcw_last, q.frame_occ) = (a.ctypes.data for a in keep)
    q.n_levels = len(keep[6])
    q.min_x, q.max_x, q.min_y, q.max_y = fr.min_x, fr.max_x, fr.min_y, fr.max_y
    q.gw_inv, q.gh_inv = float(synth.GRID_W_INV), float(synth.GRID_H_INV)
    q.fx, q.fy, q.cx, q.cy = fr.fx, fr.fy, fr.cx, fr.cy
    q.log_sf = float(synth.LOG_SCALE_FACTOR)
    q.mbf, q.mb, q.th, q.check_ori = float(fr.mbf), float(p.mb), float(p.th), int(p.check_ori)
    return q, keep


def _run(p, fixed_point: bool, o3: bool = False, packed=None):
    q, keep = pack(p) if packed is None else packed
    out = np.full(max(p.frame.n, 1), -7, np.int32)
    counts = np.zeros(4, np.int32)
    walks = np.zeros(2, np.int32)  # all window walks, the most in one round
    if fixed_point:
        lib(o3).lse_search_fixed_point_walks(C.byref(q), out, counts, walks)
    else:
        lib(o3).lse_search_sequential(C.byref(q), out, counts)
    return dict(out=out[:p.frame.n], nmatches=int(counts[0]), mode=int(counts[1]), rounds=int(counts[2]),
                claims=int(counts[3]), walks=int(walks[0]), max_round_walks=int(walks[1]))


def search_sequential(p, o3: bool = False, packed=None):
    """The literal sequential loop over the kernel's per-point functions."""
    return _run(p, False, o3, packed)


def search_fixed_point(p):
    """The rounds and the finish as the kernel runs them."""
    return _run(p, True)
