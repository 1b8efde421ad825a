"""rsc_local_bundle_adjustment_many at the drop-in boundary, without a GPU.

What runs on the real symbol in librsc.so here: the prototype against a C compiler, the NULL-context and negative-count
refusals, and every argument and size refusal (test_real_symbol_refusals) — the entry point checks all problems
before it reads its context, so those calls are made with a zeroed stand-in for the context, which a refused call
never touches; each must return its code with the outputs and the result record untouched.  The same refusals also
go through the host build (lbae_run), which runs the same lba_check first.  What needs a device is in
tests/test_gpu_localba.py: the refusals on a live context with the context used again afterwards."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import localba_cases as lc
import localba_emu_lib as le
from rsc import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def test_prototype_compiles_and_symbol_is_exported():
    src = r'''
#include <stdio.h>
#include "rsc.h"
int main(void) {
    int (*f)(rsc_context*, const rsc_localba_problem*, int, const rsc_localba_out*, rsc_localba_result*) =
        &rsc_local_bundle_adjustment_many; /* a mismatch is a compile error (-Werror) */
    printf("%zu %zu %zu %zu %d\n", sizeof(f), sizeof(rsc_localba_problem), sizeof(rsc_localba_out),
           sizeof(rsc_localba_result), RSC_LOCALBA_MAX_FREE_KFS);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        exe = os.path.join(d, "t")
        lib = os.path.dirname(engine.LIB_PATH)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(d, "t.c"), "-L", lib, "-lrsc", "-Wl,-rpath," + lib])
        out = subprocess.check_output([exe], text=True).split()
    assert int(out[1]) == C.sizeof(engine.LocalBAProblem)
    assert int(out[2]) == C.sizeof(engine.LocalBAOut)
    assert int(out[3]) == C.sizeof(engine.LocalBAResult)
    assert int(out[4]) == engine.LOCALBA_MAX_FREE_KFS
    assert engine.EXPORTED.count("rsc_local_bundle_adjustment_many") == 1


def test_null_context_and_null_problems_are_refused_before_any_hip_call():
    L = engine.load_library()
    p = lc.build("small_mixed")
    q, keep = engine.localba_pack(p)
    assert L.rsc_local_bundle_adjustment_many(None, C.byref(q), 1, None, None) == ERR_ARG
    assert L.rsc_local_bundle_adjustment_many(None, None, 0, None, None) == ERR_ARG
    assert L.rsc_local_bundle_adjustment_many(None, C.byref(q), -1, None, None) == ERR_ARG


def _refused(p):
    """The status of the argument check (the entry point's first step) and whether the outputs were left alone."""
    q, keep = engine.localba_pack(p)
    arrays = engine.localba_outputs(p)
    before = {k: v.copy() for k, v in arrays.items()}
    o = engine.LocalBAOut()
    for k, v in arrays.items():
        setattr(o, k, v.ctypes.data)
    r = engine.LocalBAResult()
    r.n_erase = -5
    st = le.lib().lbae_run(C.byref(q), 1, C.byref(o), C.byref(r))
    untouched = all(np.array_equal(v.view(np.uint8), before[k].view(np.uint8)) for k, v in arrays.items())
    return st, untouched and r.n_erase == -5


def _refused_real(p, null=None):
    """rsc_local_bundle_adjustment_many itself with a zeroed stand-in context."""
    q, keep = engine.localba_pack(p)
    if null:
        setattr(q, null, None)
    arrays = engine.localba_outputs(p)
    before = {k: v.copy() for k, v in arrays.items()}
    o = engine.LocalBAOut()
    for k, v in arrays.items():
        setattr(o, k, v.ctypes.data)
    r = engine.LocalBAResult()
    r.n_erase = -5
    stand_in = C.create_string_buffer(1 << 20)
    st = engine.load_library().rsc_local_bundle_adjustment_many(C.cast(stand_in, C.c_void_p), C.byref(q), 1, C.byref(o),
                                                                 C.byref(r))
    untouched = all(np.array_equal(v.view(np.uint8), before[k].view(np.uint8)) for k, v in arrays.items())
    assert bytes(stand_in) == bytes(1 << 20)  # the context was not written either
    return st, untouched and r.n_erase == -5


def _mutations():
    base = lc.build("small_mixed")

    def m(**kw):
        p = dict(base)
        p.update(kw)
        return p
    dup_kf = base["kf_id"].copy()
    dup_kf[-1] = dup_kf[0]
    dup_mp = base["mp_id"].copy()
    dup_mp[-1] = dup_mp[0]
    bad_begin = base["obs_begin"].copy()
    bad_begin[2] = bad_begin[1] - 1
    first = base["obs_begin"].copy()
    first[0] = 1
    oob = base["obs_kf"].copy()
    oob[3] = len(base["kf_id"])
    neg = base["obs_kf"].copy()
    neg[0] = -1
    twice = base["obs_kf"].copy()
    twice[1] = twice[0]
    assert base["obs_begin"][1] >= 2
    yield "kf_id twice", m(kf_id=dup_kf), ERR_ARG
    yield "mp_id twice", m(mp_id=dup_mp), ERR_ARG
    yield "obs_begin descending", m(obs_begin=bad_begin), ERR_ARG
    yield "obs_begin[0] != 0", m(obs_begin=first), ERR_ARG
    yield "obs_kf too large", m(obs_kf=oob), ERR_ARG
    yield "obs_kf negative", m(obs_kf=neg), ERR_ARG
    yield "a KeyFrame twice in one point", m(obs_kf=twice), ERR_ARG


@pytest.mark.parametrize("what,p,code", list(_mutations()), ids=[w for w, _, _ in _mutations()])
def test_argument_refusals(what, p, code):
    st, untouched = _refused(p)
    assert st == code, what
    assert untouched, what


NULLABLE = ("kf_id", "fixed", "Tcw", "cam", "mp_id", "pos", "bad", "obs_begin", "obs_kf", "uv", "u_right", "inv_sigma2")


@pytest.mark.parametrize("field", NULLABLE)
def test_null_arrays_are_refused(field):
    p = lc.build("small_mixed")
    assert _refused_real(p, null=field) == (ERR_ARG, True)
    q, keep = engine.localba_pack(p)
    setattr(q, field, None)
    assert le.lib().lbae_run(C.byref(q), 1, None, None) == ERR_ARG


@pytest.mark.parametrize("what,p,code", list(_mutations()), ids=[w for w, _, _ in _mutations()])
def test_real_symbol_refusals(what, p, code):
    assert _refused_real(p) == (code, True), what


def test_real_symbol_size_limits():
    E = engine
    assert _refused_real(_sized(E.LOCALBA_MAX_FREE_KFS + 1, 1, 4, 4)) == (ERR_UNSUPPORTED, True)
    assert _refused_real(_sized(2, E.LOCALBA_MAX_KFS - 1, 4, 4)) == (ERR_UNSUPPORTED, True)
    assert _refused_real(_sized(2, 2, E.LOCALBA_MAX_POINTS + 1, 4)) == (ERR_UNSUPPORTED, True)


def _sized(n_free, n_fixed, n_points, n_edges):
    """A problem of the given sizes (contents irrelevant: it is refused by its counts)."""
    K = n_free + n_fixed
    begin = np.minimum(np.arange(n_points + 1, dtype=np.int64), n_edges).astype(np.int32)
    return dict(kf_id=np.arange(K, dtype=np.int64), fixed=(np.arange(K) >= n_free).astype(np.uint8),
                Tcw=np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (K, 1)), cam=np.ones((K, 5), np.float32),
                mp_id=np.arange(n_points, dtype=np.int64), pos=np.ones((n_points, 3), np.float32),
                bad=np.zeros(n_points, np.uint8), obs_begin=begin, obs_kf=np.zeros(n_edges, np.int32),
                uv=np.zeros((n_edges, 2), np.float32), u_right=np.zeros(n_edges, np.float32),
                inv_sigma2=np.ones(n_edges, np.float32))


def test_size_limits():
    E = engine
    assert _refused(_sized(E.LOCALBA_MAX_FREE_KFS + 1, 1, 4, 4)) == (ERR_UNSUPPORTED, True)
    assert _refused(_sized(2, E.LOCALBA_MAX_KFS - 1, 4, 4)) == (ERR_UNSUPPORTED, True)
    assert _refused(_sized(2, 2, E.LOCALBA_MAX_POINTS + 1, 4)) == (ERR_UNSUPPORTED, True)
    # one edge per point and one more than the limit on the last point would name a KeyFrame twice: spread over KeyFrames
    p = _sized(2, 30, E.LOCALBA_MAX_POINTS, 0)
    per = 9
    ne = E.LOCALBA_MAX_POINTS * per
    assert ne > E.LOCALBA_MAX_EDGES
    p["obs_begin"] = (np.arange(E.LOCALBA_MAX_POINTS + 1, dtype=np.int64) * per).astype(np.int32)
    p["obs_kf"] = np.tile(np.arange(per, dtype=np.int32), E.LOCALBA_MAX_POINTS)
    p["uv"], p["u_right"], p["inv_sigma2"] = np.zeros((ne, 2), np.float32), np.zeros(ne, np.float32), np.ones(ne, np.float32)
    assert _refused(p) == (ERR_UNSUPPORTED, True)
    assert _refused_real(p) == (ERR_UNSUPPORTED, True)
    # at the limits the check passes (64 free KeyFrames, the reduced system of 384 unknowns)
    q, keep = engine.localba_pack(lc.build("limit_free64"))
    assert int((lc.build("limit_free64")["fixed"] == 0).sum()) == E.LOCALBA_MAX_FREE_KFS
