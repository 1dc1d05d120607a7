"""Raw copies to and from device memory for the tests that read or write what a kernel wrote or will read, without another kernel
of the library in between (test_gpu_multi_merge.py, test_gpu_position_passes.py).  They go through the HIP runtime the library is
linked to, reached through the library's own handle: the suite's process cannot also start torch's copy of the runtime once the
library's is in use."""
import ctypes as C

import numpy as np

from gfasort_amd import hip

H2D, D2H = 1, 2


def rt():
    """The HIP runtime the library is linked to, through the library's own handle (a symbol lookup on it searches its
    dependencies): the copies below go through the same runtime as the kernels."""
    L = hip.lib()
    if not getattr(L, "_merge_test_rt", False):
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        L.hipDeviceSynchronize.argtypes = []
        L._merge_test_rt = True
    return L


def sync():
    assert rt().hipDeviceSynchronize() == 0


def download(ptr, count, dtype):
    host = np.empty(int(count), dtype=dtype)
    assert rt().hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), host.nbytes, D2H) == 0
    return host


def upload(ptr, host):
    host = np.ascontiguousarray(host)
    assert rt().hipMemcpy(C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), host.nbytes, H2D) == 0


class Dev:
    """`count` elements of `dtype` in device memory, zeroed; a caller's buffer that a rank or a context is bound to."""

    def __init__(self, count, dtype):
        self.count, self.dtype = int(count), np.dtype(dtype)
        p = C.c_void_p()
        assert self.count > 0 and rt().hipMalloc(C.byref(p), self.count * self.dtype.itemsize) == 0
        self.ptr = p.value
        upload(self.ptr, np.zeros(self.count, dtype=self.dtype))

    def host(self):
        return download(self.ptr, self.count, self.dtype)

    def set(self, host):
        assert host.dtype == self.dtype and host.shape == (self.count,)
        upload(self.ptr, host)

    def free(self):
        if self.ptr:
            assert rt().hipFree(C.c_void_p(self.ptr)) == 0
            self.ptr = None
