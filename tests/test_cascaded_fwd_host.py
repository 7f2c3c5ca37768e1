"""CPU-only checks of the cascaded forward entries: sc_cosine_refine_masked in header, library and ctypes table, and the argument rules of sc_vq_fwd and
sc_cosine_refine_masked -- codes with a message, nothing enqueued (no GPU is needed to be refused)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_is_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in ("sc_cosine_refine", "sc_cosine_refine_masked"):
        assert n in _lib.exported_symbols() and hasattr(L, n), n
        params = re.search(rf"^int {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
    assert L.sc_abi_version() == 1


def test_argument_errors_need_no_gpu_and_launch_nothing():
    """sc_vq_fwd refuses a mask that covers every id of [0, V) (nothing would compare: the arg-max has no answer) before anything is enqueued; ids outside [0, V) and
    repeats do not count towards the cover.  sc_cosine_refine_masked: at most 8 ids, R = 0 is a no-op."""
    from speechclip_amd import _lib
    L = _lib.lib()
    F = ctypes.c_float

    def ids(*v):
        arr = (ctypes.c_int32 * max(1, len(v)))(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p), len(v)
    keep, p, n = ids(0)
    assert L.sc_vq_fwd(None, None, None, None, None, 4, 1, 1, p, n, None) == -1 and b"every id" in L.sc_last_error()
    keep, p, n = ids(2, 0, 1, 1, 7)
    assert L.sc_vq_fwd(None, None, None, None, None, 4, 1, 3, p, n, None) == -1 and b"every id" in L.sc_last_error()
    keep, p, n = ids(0, 1, 2, 3, 4, 5, 6, 7)
    assert L.sc_vq_fwd(None, None, None, None, None, 4, 1, 8, p, n, None) == -1 and b"every id" in L.sc_last_error()
    assert L.sc_vq_fwd(None, None, None, None, None, 4, 1, 8, p, 9, None) == -1 and b"at most 8" in L.sc_last_error()
    assert L.sc_vq_fwd(None, None, None, None, None, 4, 1, 8, None, 3, None) == -1 and b"null mask" in L.sc_last_error()
    assert L.sc_vq_fwd(None, None, None, None, None, 5, 2, 8, None, 0, None) == -1 and b"bad sizes" in L.sc_last_error()
    assert L.sc_cosine_refine_masked(None, None, None, 4, 8, 64, F(1e-3), F(1e-8), p, 9, None) == -1 and b"n_mask=9" in L.sc_last_error()
    assert L.sc_cosine_refine_masked(None, None, None, 4, 8, 64, F(1e-3), F(1e-8), None, 2, None) == -1
    assert L.sc_cosine_refine_masked(None, None, None, 4, 8, 64, F(-1.0), F(1e-8), None, 0, None) == -1 and b"bad arguments" in L.sc_last_error()
    assert L.sc_cosine_refine_masked(None, None, None, 0, 8, 64, F(1e-3), F(1e-8), p, 8, None) == 0
    assert L.sc_cosine_refine(None, None, None, 0, 8, 64, F(1e-3), F(1e-8), None) == 0
