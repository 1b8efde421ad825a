"""ctypes binding of tests/bowvoc_emu (TEST-ONLY single-core sequential vocabulary transform in C++:
the CPU baseline of tools/bowvoc_bench.py and a second restatement beside tests/bowvoc_ref.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "bowvoc_emu")
LIB = os.path.join(DIR, "build", "libbowvoc_emu.so")
MAIN = os.path.join(DIR, "build", "bowvoc_emu_main")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = C.CDLL(LIB)
        L.bve_create.restype = C.c_void_p
        L.bve_create.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        L.bve_destroy.argtypes = [C.c_void_p]
        L.bve_destroy.restype = None
        L.bve_transform.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib = L
    return _lib


class EmuVocabulary:
    def __init__(self, voc):
        self._keep = [np.ascontiguousarray(voc.parent, np.int32), np.ascontiguousarray(voc.is_leaf, np.uint8),
                      np.ascontiguousarray(voc.desc, np.uint8), np.ascontiguousarray(voc.weight, np.float64)]
        self.h = lib().bve_create(int(voc.L), len(self._keep[0]), *[a.ctypes.data for a in self._keep])
        self._n = 0

    def _room(self, n):
        if n > self._n or not self._n:
            m = max(n, 1)
            self._out = [np.zeros(m, np.uint32), np.zeros(m, np.float64), np.zeros(m, np.uint32),
                         np.zeros(m + 1, np.int32), np.zeros(m, np.uint32), np.zeros(2, np.int32)]
            self._n = m

    def transform_raw(self, desc: np.ndarray, levelsup: int = 4) -> int:
        """The bare C call on a contiguous uint8 [n,32] array (what the benchmark times)."""
        self._room(len(desc))
        return lib().bve_transform(self.h, len(desc), desc.ctypes.data, int(levelsup),
                                   *[a.ctypes.data for a in self._out])

    def transform(self, desc, levelsup: int = 4) -> dict:
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if self.transform_raw(d, levelsup) != 0:
            raise ValueError("a descent ended above nid_level")
        wid, wv, nid, nb, feat, cnt = self._out
        nw, nn = int(cnt[0]), int(cnt[1])
        return dict(word_id=wid[:nw].copy(), word_value=wv[:nw].copy(), node_id=nid[:nn].copy(),
                    node_begin=nb[:nn + 1].copy(), feat=feat[:int(nb[nn])].copy())

    def close(self):
        if self.h:
            lib().bve_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
