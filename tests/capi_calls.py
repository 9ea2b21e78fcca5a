"""Arguments for calling the C entry points without a GPU: dummy non-null pointers that are never dereferenced (every such call fails
argument validation before any HIP call) and the all-zero argument list of a binding row."""
import ctypes as C

_D = 4096


def _d(k=0):
    return C.c_void_p(_D * (k + 1))


def _zero(argtypes):
    """every pointer NULL, every number 0"""
    return [t(0) if t in (C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double) else None for t in argtypes]
