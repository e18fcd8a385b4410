"""CPU-side check of g2g_batch_paths (include/g2g.h): without a device -- no batch can exist -- it answers with the library's
argument / no-device errors and does not crash.  No GPU compute here."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    from prrn_aln_amd import build
    return build.build_lib()


def test_batch_paths_without_a_batch(built):
    L = C.CDLL(built)
    L.g2g_create.restype = C.c_void_p
    L.g2g_create.argtypes = [C.c_int]
    L.g2g_destroy.argtypes = [C.c_void_p]
    L.g2g_batch_prepare.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.g2g_batch_paths.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.g2g_batch_free.argtypes = [C.c_void_p]
    L.g2g_last_error.restype = C.c_char_p
    gen = (C.c_int32 * 4)(9, 9, 9, 9)
    assert L.g2g_batch_paths(None, gen) == -1                      # G2G_ERR_ARG
    assert L.g2g_batch_paths(None, None) == -1
    assert b"g2g_batch_paths" in L.g2g_last_error()
    assert list(gen) == [9, 9, 9, 9]
    h = L.g2g_create(-1)
    if not h:
        return                                                      # (no context at all without a device: nothing more to ask)
    try:
        b = C.c_void_p()
        rc = L.g2g_batch_prepare(h, 0, None, C.byref(b))
        if rc == 0:                                                 # a device is present: an empty batch reports nothing
            assert L.g2g_batch_paths(b, None) == -1
            assert L.g2g_batch_paths(b, gen) == 0 and list(gen) == [9, 9, 9, 9]
            L.g2g_batch_free(b)
        else:
            assert rc == -3 and not b.value                         # G2G_ERR_NODEVICE, and no batch to ask about
            assert L.g2g_batch_paths(b, gen) == -1
    finally:
        L.g2g_destroy(h)


def test_bonus_cells_restatement_matches_the_library(built):
    """tests/intronlib.bonus_cells (the walk restated in Python; the coverage assertions of tests/test_gpu_intron_strips.py rest
    on it) against the table the library itself builds at pack time (g2g_bonus_cells: host only) -- the seven annotated
    goldens and every synthetic annotation.  If the two drift apart this fails, not nothing."""
    import numpy as np
    import intronlib as il
    from prrn_aln_amd import _abi
    L = C.CDLL(built)
    L.g2g_bonus_cells.argtypes = [C.POINTER(_abi.Problem), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _abi.c_f64p, _abi.c_f64p]
    assert L.g2g_bonus_cells(None, 0, None, None, None, None) == -1
    inputs = [dict(np.load(f)) for f in il.INTRON] + [il.annotate(il.load(n), v) for n, v in il.SYNTH]
    assert len(inputs) == 12
    for d in inputs:
        want = il.bonus_cells(d)
        h = _abi.problem_from_arrays(d)
        cap = len(want) + 8
        m, n, bh, bx = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        cnt = L.g2g_bonus_cells(C.byref(h.c), cap, m, n, bh, bx)
        assert cnt == len(want) and cnt > 0
        assert [(m[k], n[k], bh[k], bx[k]) for k in range(cnt)] == want
        assert L.g2g_bonus_cells(C.byref(h.c), 0, None, None, None, None) == cnt      # counting only
    plain = _abi.problem_from_arrays(il.unannotated(il.load(il.SYNTH[0][0])))
    assert L.g2g_bonus_cells(C.byref(plain.c), 0, None, None, None, None) == 0
