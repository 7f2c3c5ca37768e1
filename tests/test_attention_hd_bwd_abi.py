"""CPU-only: sc_attention_hd_bwd in the header, the library's exports and the ctypes table together, and its argument errors as codes (no launch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_attention_hd_bwd", "sc_attention_hd_bwd_workspace_bytes")


def _call(L, B, H, Tq, Tk, hd, drop_p=0.0, stride=None):
    D = H * hd if stride is None else stride
    return L.sc_attention_hd_bwd(None, None, None, None, None, None, B, H, Tq, Tk, hd, Tq * D, D, Tk * D, D, Tq * D, D, None, Tq * D, D, None, None, Tk * D, D,
                                 ctypes.c_float(1.0), ctypes.c_float(drop_p), 0, None, None)


def test_entry_is_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n)
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", text).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
    assert L.sc_attention_hd_bwd.restype is ctypes.c_int and L.sc_attention_hd_bwd_workspace_bytes.restype is ctypes.c_int64
    assert L.sc_attention_hd_bwd_workspace_bytes(2, 8, 500) == 2 * 4 * 2 * 8 * 500
    assert L.sc_attention_hd_bwd_workspace_bytes(2, 8, 1) == 2 * 4 * 2 * 8
    assert L.sc_attention_hd_bwd_workspace_bytes(0, 8, 500) == 0


def test_argument_errors_are_codes_with_a_message():
    from speechclip_amd import _lib
    L = _lib.lib()
    assert _call(L, 1, 2, 8, 8, 80) < 0 and b"head_dim=80" in L.sc_last_error()
    assert _call(L, 1, 2, 7, 40, 96) < 0 and b"Tq=7 Tk=40" in L.sc_last_error()
    assert _call(L, 1, 2, 8, 8, 96, stride=196) < 0 and b"multiples of 8" in L.sc_last_error()
    assert _call(L, 1, 2, 8, 8, 96, drop_p=1.0) < 0 and b"drop_p" in L.sc_last_error()
    assert _call(L, 1, 2, 8, 8, 96) < 0 and b"null operand" in L.sc_last_error()        # served sizes, no operands
    assert _call(L, 0, 2, 8, 8, 96) == 0 and _call(L, 2, 2, 0, 0, 128) == 0               # nothing to do: no launch, no look at the operands
