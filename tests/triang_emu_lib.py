"""ctypes binding of tests/triang_emu (TEST-ONLY host build of rsc_triang.h: the literal sequential loop and the
kernels' own item / reduction order over the same per-candidate and per-pair functions), and the case file of its
stand-alone program."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "triang_emu")
LIB = os.path.join(DIR, "build", "libtriang_emu.so")
LIB_O3 = os.path.join(DIR, "build", "libtriang_emu_o3.so")
MAIN = os.path.join(DIR, "build", "triang_emu_main")
MAIN_SAN = os.path.join(DIR, "build", "triang_emu_main_san")
_libs = {}
f32 = np.float32


class KF(C.Structure):
    """tse_kf (triang_emu.cpp)."""
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in ("kp", "kp_raw", "octave", "desc", "angle", "u_right",
                                                                "depth", "cos_stereo", "mp_state")] + \
               [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_begin", C.c_void_p), ("feat", C.c_void_p),
                ("scale", C.c_void_p), ("n_levels", C.c_int32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf", "scale_factor")] + \
               [("Kinv", C.c_float * 9)]


def build():
    subprocess.check_call(["make", "-s", "-C", DIR])


def lib(o3: bool = False):
    if o3 not in _libs:
        build()
        L = C.CDLL(LIB_O3 if o3 else LIB)
        for f in ("tse_search_sequential", "tse_search_kernel_order", "tse_triangulate", "tse_compute_f12",
                  "tse_svd_last_v", "tse_create_new_map_points"):
            getattr(L, f).restype = None
        _libs[o3] = L
    return _libs[o3]


def _arrays(k):
    pad = lambda a, dt, m: (np.ascontiguousarray(a, dt).reshape(-1) if np.size(a) else np.zeros(m, dt))
    return [pad(k.kp, f32, 2), pad(k.kp_raw, f32, 2), pad(k.octave, np.int32, 1), pad(k.desc, np.uint8, 32),
            pad(k.angle, f32, 1), pad(k.u_right, f32, 1), pad(k.depth, f32, 1), pad(k.cos_parallax_stereo, f32, 1),
            pad(k.mp_state, np.uint8, 1), pad(k.node_id, np.uint32, 1), pad(k.node_begin, np.int32, 1),
            pad(k.feat, np.uint32, 1), pad(k.scale_factors, f32, 1)]


def _scalars(k):
    return np.concatenate([np.asarray(k.Rcw, f32).reshape(9), np.asarray(k.tcw, f32).reshape(3),
                           np.asarray(k.Rwc, f32).reshape(9), np.asarray(k.Ow, f32).reshape(3),
                           np.array([k.fx, k.fy, k.cx, k.cy, k.invfx, k.invfy, k.mb, k.mbf, k.scale_factor], f32),
                           np.asarray(k.Kinv, f32).reshape(9)]).astype(f32)


def pack(k):
    """(tse_kf, keep-alive arrays) of a KeyFrame namespace (tests/triang_cases.py)."""
    keep = _arrays(k)
    q = KF()
    q.n, q.n_nodes, q.n_levels = int(k.n), len(k.node_id), len(k.scale_factors)
    (q.kp, q.kp_raw, q.octave, q.desc, q.angle, q.u_right, q.depth, q.cos_stereo, q.mp_state, q.node_id,
     q.node_begin, q.feat, q.scale) = (a.ctypes.data for a in keep)
    s = _scalars(k)
    q.Rcw[:], q.tcw[:], q.Rwc[:], q.Ow[:] = s[0:9].tolist(), s[9:12].tolist(), s[12:21].tolist(), s[21:24].tolist()
    (q.fx, q.fy, q.cx, q.cy, q.invfx, q.invfy, q.mb, q.mbf, q.scale_factor) = s[24:33].tolist()
    q.Kinv[:] = s[33:42].tolist()
    return q, keep


def _flags(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8)


def search(k1, k2, F12, only_stereo=False, check_ori=False, has1=None, has2=None, kernel_order=False, o3=False,
           packed=None):
    (q1, _a), (q2, _b) = packed or (pack(k1), pack(k2))
    n = max(int(k1.n), 1)
    m, counts, dzs = np.full(n, -7, np.int32), np.zeros(2, np.int32), np.zeros(n, np.uint8)
    F = np.ascontiguousarray(F12, f32).reshape(9)
    h1, h2 = _flags(has1), _flags(has2)
    fn = lib(o3).tse_search_kernel_order if kernel_order else lib(o3).tse_search_sequential
    fn(C.byref(q1), C.byref(q2), F.ctypes.data_as(C.c_void_p), int(only_stereo), int(check_ori),
       None if h1 is None else h1.ctypes.data_as(C.c_void_p), None if h2 is None else h2.ctypes.data_as(C.c_void_p),
       m.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), dzs.ctypes.data_as(C.c_void_p))
    return dict(matches12=m[:k1.n], nmatches=int(counts[0]), den_zero=int(counts[1]), den_zero_slot=dzs[:k1.n])


def triangulate(k1, k2, pairs, o3=False, packed=None):
    (q1, _a), (q2, _b) = packed or (pack(k1), pack(k2))
    p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = max(len(p), 1)
    st, x = np.full(m, -7, np.int32), np.zeros((m, 3), f32)
    pp = p if len(p) else np.zeros((1, 2), np.int32)
    lib(o3).tse_triangulate(C.byref(q1), C.byref(q2), len(p), pp.ctypes.data_as(C.c_void_p),
                            st.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    return st[:len(p)], x[:len(p)]


def compute_f12(k1, k2):
    (q1, _a), (q2, _b) = pack(k1), pack(k2)
    F = np.zeros(9, f32)
    lib().tse_compute_f12(C.byref(q1), C.byref(q2), F.ctypes.data_as(C.c_void_p))
    return F.reshape(3, 3)


def svd_last_v(A):
    a, v = np.ascontiguousarray(A, f32).reshape(16), np.zeros(4, f32)
    lib().tse_svd_last_v(a.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
    return v


def create_new_map_points(cur, neighbours, o3=False, packed=None):
    """The literal neighbour loop over the sequential matcher (the one-core baseline of tools/triang_bench.py)."""
    qc, qn = packed or (pack(cur), [pack(k) for k in neighbours])
    n = max(int(cur.n), 1)
    nn, i2, pos, nnew = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.zeros((n, 3), f32), C.c_int32()
    ptrs = (C.c_void_p * max(len(qn), 1))(*[C.addressof(q[0]) for q in qn])
    lib(o3).tse_create_new_map_points(C.byref(qc[0]), ptrs, len(qn), nn.ctypes.data_as(C.c_void_p),
                                      i2.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), C.byref(nnew))
    return dict(new_neighbour=nn[:cur.n], new_idx2=i2[:cur.n], new_pos=pos[:cur.n], nnew=nnew.value)


def _blob(a):
    b = np.ascontiguousarray(a).tobytes()
    return b + b"\0" * (-len(b) % 8)


def _dump_kf(k):
    arrs = _arrays(k)
    n, nn = int(k.n), len(k.node_id)
    sizes = [2 * n, 2 * n, n, 32 * n, n, n, n, n, n, nn, nn + 1, len(np.asarray(k.feat)), len(k.scale_factors)]
    out = b"".join(_blob(np.int32(v)) for v in (n, nn, len(k.scale_factors), len(np.asarray(k.feat))))
    for a, s in zip(arrs, sizes):
        out += _blob(a[:s])
    return out + _blob(_scalars(k))


def write_cases(cases, path):
    """The case file of the stand-alone programs (this one's and tests/cpp/facade_triang_test.cpp): int32 words and
    raw arrays, each padded to 8 bytes."""
    with open(path, "wb") as f:
        f.write(_blob(np.int32(len(cases))))
        for k1, k2, F, os_, co, pairs in cases:
            p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            f.write(_dump_kf(k1) + _dump_kf(k2) + _blob(np.asarray(F, f32).reshape(9)))
            f.write(_blob(np.int32(os_)) + _blob(np.int32(co)) + _blob(np.int32(len(p))) + _blob(p))


def run_main(cases, path_in, path_out, sanitized=False):
    """cases: (kf1, kf2, F12, only_stereo, check_ori, pairs int32 [np,2]).  Runs the stand-alone program (plain or
    under the host sanitizers) and returns per case (sequential, kernel order, status, x3d)."""
    build()
    write_cases(cases, path_in)
    subprocess.run([MAIN_SAN if sanitized else MAIN, path_in, path_out], check=True, capture_output=True, timeout=300)
    raw = np.fromfile(path_out, np.int32)
    out, o = [], 0
    for k1, k2, F, os_, co, pairs in cases:
        n, npairs = int(k1.n), len(np.asarray(pairs).reshape(-1, 2))
        res = []
        for _ in range(2):
            res.append(dict(nmatches=int(raw[o]), den_zero=int(raw[o + 1]), matches12=raw[o + 2:o + 2 + n].copy()))
            o += 2 + n
        st = raw[o:o + npairs].copy()
        x = raw[o + npairs:o + 4 * npairs].copy().view(f32).reshape(-1, 3)
        o += 4 * npairs
        out.append((res[0], res[1], st, x))
    assert o == len(raw)
    return out
