"""No GPU: the deterministic-reduction entries (sc_sgemm_batched_det, sc_colsum_det, sc_cls_pool_bwd_det and their size functions) in header, library and
ctypes table; the workspace sizes against the split / chunk rules restated in tests/tail_kernels_ref.py on both sides of every threshold; the host switch."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import tail_kernels_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_ENTRIES = ("sc_sgemm_batched_det", "sc_sgemm_det", "sc_colsum_det", "sc_cls_pool_bwd_det", "sc_sgemm_det_slices", "sc_colsum_det_chunks")
SIZE_ENTRIES = ("sc_sgemm_det_workspace_bytes", "sc_colsum_det_workspace_bytes")

# (M, N, K, batch): K = 2047 / 2048 (the length threshold), tiles = 127 / 128 (the tile threshold: 127 x 1 and 128 x 1 tiles of 64, and 3 x 42 + 1 / 4 x 32 over a
# batch), K / split around 256 (the slice-length floor), ragged sizes, the shapes of tests/test_deterministic_kernels_gpu.py
SGEMM_SHAPES = ((64, 64, 2047, 1), (64, 64, 2048, 1), (64, 64, 2049, 1), (64 * 127, 64, 2048, 1), (64 * 127 + 1, 64, 2048, 1), (64 * 128, 64, 2048, 1),
                (64, 64 * 127, 4096, 1), (64, 64 * 42, 2048, 3), (64, 64 * 43, 2048, 3), (128, 64 * 32, 2048, 2), (33, 70, 4099, 1), (16, 64, 2304, 3),
                (1, 1, 1, 1), (5, 65, 19, 3), (768, 768, 127744, 1), (64, 64, 16384, 1), (64, 64, 16383, 1), (65, 64, 65536, 1), (64, 64, 2560, 1))
# (rows, cols): rows = 255 / 256, 511 / 512 column blocks of 64, the shapes of the GPU test
COLSUM_SHAPES = ((255, 64), (256, 64), (257, 64), (1000, 70), (256, 64 * 511), (256, 64 * 511 + 1), (256, 64 * 512), (256, 64 * 512 - 63), (1, 1), (127744, 768),
                 (4096, 64 * 100), (300, 64 * 17 + 5))


def test_new_entries_are_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in INT_ENTRIES + SIZE_ENTRIES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is (ctypes.c_int64 if n in SIZE_ENTRIES else ctypes.c_int), n
    # the pooling entry takes sc_cls_pool_bwd's arguments, the other two their default's plus (workspace, workspace_bytes) in front of the stream
    assert L.sc_cls_pool_bwd_det.argtypes == L.sc_cls_pool_bwd.argtypes
    for det, base in (("sc_sgemm_batched_det", "sc_sgemm_batched"), ("sc_sgemm_det", "sc_sgemm"), ("sc_colsum_det", "sc_colsum")):
        a, b = getattr(L, det).argtypes, getattr(L, base).argtypes
        assert a[:len(b) - 1] == b[:-1] and a[len(b) - 1:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p], det
    assert L.sc_abi_version() == 1


@pytest.mark.parametrize("M,N,K,batch", SGEMM_SHAPES)
def test_sgemm_workspace_is_slices_of_the_restated_split_rule(M, N, K, batch):
    from speechclip_amd import _lib
    L = _lib.lib()
    slices, _ = T.gemm_split(M, N, K, batch)
    assert L.sc_sgemm_det_slices(M, N, K, batch) == slices
    assert L.sc_sgemm_det_workspace_bytes(M, N, K, batch) == slices * M * N * batch * 4


def test_sgemm_shape_list_is_on_both_sides_of_the_thresholds():
    s = {sh: T.gemm_split(*sh)[0] for sh in SGEMM_SHAPES}
    assert s[(64, 64, 2047, 1)] == 1 and s[(64, 64, 2048, 1)] == 8                                  # K
    assert s[(64 * 127, 64, 2048, 1)] > 1 and s[(64 * 127 + 1, 64, 2048, 1)] == 1 and s[(64 * 128, 64, 2048, 1)] == 1          # tiles 127 | 128
    assert s[(64, 64 * 42, 2048, 3)] > 1 and s[(64, 64 * 43, 2048, 3)] == 1                         # tiles 126 | 129 over a batch
    assert s[(128, 64 * 32, 2048, 2)] == 1                                                          # tiles 128 over a batch
    assert s[(64, 64, 16384, 1)] == 64 and s[(768, 768, 127744, 1)] == 1 and s[(33, 70, 4099, 1)] > 1 and s[(16, 64, 2304, 3)] > 1


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES)
def test_colsum_workspace_is_chunks_of_the_restated_chunk_rule(rows, cols):
    from speechclip_amd import _lib
    L = _lib.lib()
    chunks, _ = T.cs_chunks(rows, cols)
    assert L.sc_colsum_det_chunks(rows, cols) == chunks
    assert L.sc_colsum_det_workspace_bytes(rows, cols) == chunks * cols * 4


def test_colsum_shape_list_is_on_both_sides_of_the_thresholds():
    c = {sh: T.cs_chunks(*sh)[0] for sh in COLSUM_SHAPES}
    assert c[(255, 64)] == 1 and c[(256, 64)] == 4 and c[(1000, 70)] > 1
    assert c[(256, 64 * 511)] > 1 and c[(256, 64 * 511 + 1)] == 1 and c[(256, 64 * 512)] == 1


def test_empty_problems_have_no_slices_and_no_workspace():
    from speechclip_amd import _lib
    L = _lib.lib()
    assert L.sc_sgemm_det_slices(0, 4, 4, 1) == 0 and L.sc_sgemm_det_workspace_bytes(4, 4, 0, 1) == 0
    assert L.sc_colsum_det_chunks(0, 4) == 0 and L.sc_colsum_det_workspace_bytes(4, 0) == 0


def test_argument_errors_are_codes_with_a_message_and_no_launch():
    from speechclip_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) // 16 * 16 + 16          # an aligned, non-null host address: never dereferenced, every call below returns before a launch
    need = L.sc_sgemm_det_workspace_bytes(64, 64, 2048, 1)
    assert L.sc_sgemm_batched_det(0, 0, 64, 64, 2048, 1.0, p, 2048, 0, p, 64, 0, 0.0, p, 64, 0, None, 0, 1, p, need - 4, None) < 0
    assert "sc_sgemm_batched_det: workspace" in L.sc_last_error().decode()
    assert L.sc_sgemm_batched_det(0, 0, 64, 64, 2048, 1.0, p, 2048, 0, p, 64, 0, 0.0, p, 64, 0, None, 0, 1, None, need, None) < 0
    assert L.sc_sgemm_det(0, 0, 64, 64, 2048, 1.0, p, 2047, p, 64, 0.0, p, 64, None, p, need, None) < 0
    assert "leading dimension" in L.sc_last_error().decode()
    assert L.sc_colsum_det(p, 64, 256, 64, p, 0, p, L.sc_colsum_det_workspace_bytes(256, 64) - 4, None) < 0
    assert "sc_colsum_det: workspace" in L.sc_last_error().decode()
    assert L.sc_cls_pool_bwd_det(p, 768, p, None, 0, 0, 0, 0, p, p, p, None, p, p, p, p, None, 2, 10, 1, 8, 768, 65, 0.0, 0, None) < 0
    assert "nsplit=65" in L.sc_last_error().decode()


# ------------------------------------------------------------------------------------------------ the switch
def test_env_values_parse():
    from speechclip_amd import ops
    for v in ("1", "true", "TRUE", "on", "yes", " 1 "):
        assert ops._env_flag(v) is True, v
    for v in (None, "", "0", "false", "off", "no", "2", "deterministic"):
        assert ops._env_flag(v) is False, v


@pytest.mark.parametrize("value,want", [("1", True), (None, False)])
def test_sc_deterministic_is_read_once_at_import(value, want):
    env = {k: v for k, v in os.environ.items() if k != "SC_DETERMINISTIC"}
    if value is not None:
        env["SC_DETERMINISTIC"] = value
    code = ("import os; from speechclip_amd import ops; a = ops.deterministic(); os.environ['SC_DETERMINISTIC'] = '1' if not a else '0'; "
            "print(int(a), int(ops.deterministic()))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(int(want))] * 2


def test_set_deterministic_round_trips_and_torchs_flag_is_read_not_set():
    import torch
    from speechclip_amd import ops
    before, torch_before = ops._DETERMINISTIC[0], torch.are_deterministic_algorithms_enabled()
    try:
        ops.set_deterministic(True)
        assert ops.deterministic() is True and torch.are_deterministic_algorithms_enabled() == torch_before
        ops.set_deterministic(False)
        assert ops.deterministic() is torch_before
        torch.use_deterministic_algorithms(True)
        assert ops.deterministic() is True and ops._DETERMINISTIC[0] is False
        torch.use_deterministic_algorithms(False)
        assert ops.deterministic() is False
        ops.set_deterministic(1)
        assert ops._DETERMINISTIC[0] is True
    finally:
        torch.use_deterministic_algorithms(torch_before)
        ops.set_deterministic(before)


def test_counters_start_at_zero_and_reset():
    from speechclip_amd import ops
    assert sorted(ops.det_counters()) == ["cls_pool_bwd", "colsum_chunks", "sgemm_split"]
    ops._DET_COUNTERS["sgemm_split"] += 2
    try:
        assert ops.det_counters(reset=True)["sgemm_split"] >= 2
        assert ops.det_counters() == {"sgemm_split": 0, "colsum_chunks": 0, "cls_pool_bwd": 0}
    finally:
        ops.det_counters(reset=True)
