"""rsc_diag_fill_staging at the drop-in boundary, without a GPU: librsc.so exports it once, a C compiler reads the
header's declaration as the binding declares it (a 64-bit return value, a context and an int), and a NULL
context is an error, not a count."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from rsc import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rsc_diag_fill_staging"

PROBE = r"""
#include <stdint.h>
#include <stdio.h>
#include "rsc.h"
int main(void) {
    int64_t (*f)(rsc_context*, int) = &rsc_diag_fill_staging; /* a mismatch is a compile error (-Werror) */
    printf("%zu %zu\n", sizeof(f), sizeof(rsc_diag_fill_staging((rsc_context*)0, 0)));
    return 0;
}
"""


def test_symbol_is_exported_once():
    L = engine.load_library()
    assert hasattr(L, NAME)
    assert engine.EXPORTED.count(NAME) == 1
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert len(re.findall(rf" T {NAME}$", out, flags=re.M)) == 1
    header = open(os.path.join(ROOT, "include", "rsc.h")).read()
    assert len(re.findall(rf"\b{NAME}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) == 1


def test_binding_matches_the_header(tmp_path):
    L = engine.load_library()
    assert L.rsc_diag_fill_staging.restype is C.c_int64
    assert list(L.rsc_diag_fill_staging.argtypes) == [C.c_void_p, C.c_int]
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src, obj = tmp_path / "probe.c", tmp_path / "probe.o"
    src.write_text(PROBE)
    # compiled, not linked: the call inside sizeof is not evaluated and the address needs no library here
    subprocess.check_call([cc, "-std=c99", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj),
                           str(src)])


def test_null_context_and_bad_byte_are_errors():
    L = engine.load_library()
    assert L.rsc_diag_fill_staging(None, 0) == -1   # RSC_ERR_ARG, before any HIP call
    assert L.rsc_diag_fill_staging(None, 255) == -1
    assert L.rsc_diag_fill_staging(None, 256) == -1
    assert hasattr(engine.Context, "fill_staging")
