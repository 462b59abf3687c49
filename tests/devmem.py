"""Plain device memory for the tests of the library's ``*_device`` entries, through the HIP runtime the product library is linked
against (ctypes; no torch): upload a NumPy array, download into one, fill with a byte, free everything at the end."""
from __future__ import annotations

import ctypes as C

import numpy as np


class DevMem:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self._ptrs = []

    def alloc(self, nbytes: int, fill: int | None = None) -> int:
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(int(nbytes), 8))) == 0
        self._ptrs.append(p)
        if fill is not None:
            assert self.hip.hipMemset(p, C.c_int(fill), C.c_size_t(int(nbytes))) == 0
            assert self.hip.hipDeviceSynchronize() == 0
        return p.value

    def up(self, a) -> int:
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 4) == 0      # hipMemcpyDefault
        return p

    def down(self, p: int, shape, dtype=np.float64):
        """The caller has synchronised the stream that wrote p."""
        a = np.empty(shape, dtype=dtype)
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), C.c_size_t(a.nbytes), 4) == 0
        return a

    def free(self):
        for p in self._ptrs:
            assert self.hip.hipFree(p) == 0
        self._ptrs = []
