"""rsc_compute_stereo_matches_many at the drop-in boundary, without a GPU: librsc.so exports it, the ctypes
structures of the binding have the sizes and offsets a C compiler gives the header's, and the limit agrees."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from rsc import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "rsc.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(rsc_right_features), offsetof(rsc_right_features, kp),
           offsetof(rsc_right_features, octave), offsetof(rsc_right_features, desc), sizeof(rsc_stereo_result),
           offsetof(rsc_stereo_result, n_removed), offsetof(rsc_stereo_result, median),
           offsetof(rsc_stereo_result, th_dist), sizeof(&rsc_compute_stereo_matches_many), RSC_STEREO_MAX_RIGHT);
    return 0;
}
"""


def test_symbol_is_exported():
    L = engine.load_library()
    assert hasattr(L, "rsc_compute_stereo_matches_many")
    assert "rsc_compute_stereo_matches_many" in engine.EXPORTED
    out = subprocess.run(["nm", "-D", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rsc_compute_stereo_matches_many" in out


def test_struct_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, S = engine.RightFeatures, engine.StereoResult
    want = [C.sizeof(R), R.kp.offset, R.octave.offset, R.desc.offset, C.sizeof(S), S.n_removed.offset, S.median.offset,
            S.th_dist.offset, C.sizeof(C.c_void_p), engine.STEREO_MAX_RIGHT]
    assert got == want, (got, want)
    assert C.sizeof(R) == 32 and C.sizeof(S) == 16
