"""Device memory for the tests without torch: a few calls of the HIP runtime that this process has ALREADY mapped (a ``Context`` loads
it with the library), bound with ctypes.  Its path is read from /proc/self/maps and that very file is opened again, so the process
never gets a second runtime."""
import ctypes

import numpy as np

H2D, D2H, D2D = 1, 2, 3
_hip = None


def runtime_path():
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64" in path.rsplit("/", 1)[-1]:
                return path
    raise RuntimeError("no HIP runtime is mapped yet: make a pyrodigal_amd Context first")


def hip():
    global _hip
    if _hip is None:
        L = ctypes.CDLL(runtime_path())
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        for name, args in (("hipMalloc", [ctypes.POINTER(vp), sz]), ("hipFree", [vp]), ("hipMemcpy", [vp, vp, sz, i]),
                           ("hipMemcpyAsync", [vp, vp, sz, i, vp]), ("hipMemsetAsync", [vp, i, sz, vp]),
                           ("hipHostMalloc", [ctypes.POINTER(vp), sz, ctypes.c_uint]), ("hipHostFree", [vp]),
                           ("hipStreamCreate", [ctypes.POINTER(vp)]), ("hipStreamDestroy", [vp]), ("hipStreamSynchronize", [vp])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = i, args
        _hip = L
    return _hip


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (hipError_t %d)" % (what, rc))


class DeviceArray:
    """``nbytes`` of device memory with a ``__cuda_array_interface__``: ``shape`` / ``typestr`` / ``strides`` describe what it holds."""

    def __init__(self, nbytes, shape=None, typestr="|u1", strides=None):
        p = ctypes.c_void_p()
        check(hip().hipMalloc(ctypes.byref(p), max(int(nbytes), 1)), "hipMalloc")
        self.ptr, self.nbytes = int(p.value), int(nbytes)
        self.shape = (self.nbytes,) if shape is None else tuple(shape)
        self.typestr, self.strides = typestr, strides

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.nbytes, a.shape, a.dtype.str if a.dtype.itemsize > 1 else ("|i1" if a.dtype.kind == "i" else "|u1"))
        if a.nbytes:
            check(hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, H2D), "hipMemcpy")
        return d

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.typestr, "data": (self.ptr, False), "version": 3, "strides": self.strides}

    def to_numpy(self, dtype=np.uint8):
        out = np.empty(self.nbytes, np.uint8)
        if self.nbytes:
            check(hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, D2H), "hipMemcpy")
        return out.view(dtype)

    def close(self):
        if self.ptr and _hip is not None:         # (not while the interpreter takes the module apart)
            _hip.hipFree(self.ptr)
        self.ptr = 0

    def __del__(self):
        self.close()


class PinnedArray:
    """A numpy uint8 array over pinned host memory."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        check(hip().hipHostMalloc(ctypes.byref(p), max(int(nbytes), 1), 0), "hipHostMalloc")
        self.ptr = int(p.value)
        self.array = np.frombuffer((ctypes.c_uint8 * int(nbytes)).from_address(self.ptr), np.uint8)

    def close(self):
        if self.ptr:
            self.array = None
            hip().hipHostFree(self.ptr)
            self.ptr = 0


class Stream:
    def __init__(self):
        p = ctypes.c_void_p()
        check(hip().hipStreamCreate(ctypes.byref(p)), "hipStreamCreate")
        self.cuda_stream = int(p.value)

    def synchronize(self):
        check(hip().hipStreamSynchronize(self.cuda_stream), "hipStreamSynchronize")

    def close(self):
        if self.cuda_stream:
            hip().hipStreamDestroy(self.cuda_stream)
            self.cuda_stream = 0
