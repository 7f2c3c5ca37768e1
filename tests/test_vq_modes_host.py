"""CPU-only checks of the quantizer's soft / gumbel modes: the constructor, the noise contract restated in float64 (tests/vq_modes_ref.py), the fixture written
by tests/golden/make_golden_vq.py from the reference's own SimpleVectorQuantizer, and the new C entries in header, library and ctypes table."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_modes_ref as R  # noqa: E402

NAMES = ("sc_vq_gumbel_noise", "sc_vq_noisy_argmax", "sc_vq_probs", "sc_vq_soft_table_bytes", "sc_vq_soft_table", "sc_vq_soft_embed_workspace_bytes",
         "sc_vq_soft_embed", "sc_vq_mode_bwd")


def test_constructor_takes_every_mode_and_still_refuses_time_first_false():
    from speechclip_amd.module.speechclip_c_modules.vector_quantizers import SimpleVectorQuantizer
    for use_gumbel in (False, True):
        for hard in (False, True):
            vq = SimpleVectorQuantizer("fixed=0.1", use_gumbel=use_gumbel, hard=hard)
            assert (vq.use_gumbel, vq.hard, vq.groundTruthPerplexity) == (use_gumbel, hard, None)
    assert SimpleVectorQuantizer("learnable=0.2", groundTruthPerplexity=30.0, use_gumbel=True, hard=False).groundTruthPerplexity == 30.0
    with pytest.raises(NotImplementedError, match="time_first"):
        SimpleVectorQuantizer("fixed=0.1", time_first=False)


def test_make_config_carries_the_quantizer_switches():
    from speechclip_amd.util.shipped_configs import make_config
    shipped = make_config(cascaded=True, parallel=False).model_settings.cascaded_branch.vq.args
    assert (shipped.use_gumbel, shipped.hard) == (False, True)
    args = make_config(cascaded=True, parallel=False, vq_args={"use_gumbel": True, "hard": False}).model_settings.cascaded_branch.vq.args
    assert (args.use_gumbel, args.hard, args.temp) == (True, False, "fixed=0.1")


def test_noise_restatement_is_a_gumbel_sample():
    """2^20 draws: mean = Euler's constant, variance = pi^2 / 6 (sigma of the sample mean 1.25e-3, of the sample variance ~3.4e-3: the bounds are 8-9 sigma),
    every value inside the range the 23-bit uniform allows, the uniform itself exact in fp32."""
    idx = np.arange(1 << 20, dtype=np.uint64)
    g = R.gumbel(1234567, idx)
    assert abs(g.mean() - 0.57722) < 0.01
    assert abs(g.var() - np.pi ** 2 / 6) < 0.03
    assert g.min() >= -2.82 and g.max() <= 16.64
    u = R.uniform(1234567, idx)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert -np.log(-np.log(2.0 ** -24)) > -2.82 and -np.log(-np.log(1 - 2.0 ** -24)) < 16.64          # the two extreme draws
    assert not np.array_equal(R.hash_draw(1, idx[:64]), R.hash_draw(2, idx[:64]))
    assert int(R.hash32(np.uint64(0))) == 0                                                           # the dropout hash of csrc/common.h fixes 0
    assert bin(int(R.hash32(np.uint64(1))) ^ int(R.hash32(np.uint64(3)))).count("1") >= 8


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "vq_modes.npz"))
    x = g["x_q"].astype(np.float32) / 2 ** 10
    emb = g["emb_q"].astype(np.float32) / 2 ** 6
    return g, x, emb


def test_fixture_is_small_and_drew_the_restated_noise(fixture):
    g, x, emb = fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vq_modes.npz")) <= 200 * 1024
    assert x.shape == (12, 331) and emb.shape == (331, 64) and np.abs(x).max() < 1
    e = R.unpack_f32(g["e"], x.shape)
    assert np.array_equal(e, R.exponential(int(g["seed"]), np.arange(x.size, dtype=np.uint64)).reshape(x.shape).astype(np.float32))


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("temp", [0.1, 0.5])
def test_float64_restatement_reproduces_the_reference_class(fixture, mode, temp):
    """my_vector_quantizer.py:124-131 + kwClip.py:909 restated (vq_modes_ref.mode_forward / mode_dx) against what the reference class returned."""
    g, x, emb = fixture
    use_gumbel, hard = R.MODES[mode]
    tag = f"{mode}/T{temp}/"
    prob, targets, kw, y = R.mode_forward(x, emb, temp, use_gumbel, hard, int(g["seed"]), f32_points=True)
    assert np.array_equal(targets, R.mode_forward(x, emb, temp, use_gumbel, hard, int(g["seed"]))[1])          # the plain float64 form picks the same sub-words
    assert np.array_equal(targets, g[tag + "targets"])
    ref_prob = R.unpack_f32(g[tag + "subword_prob"], x.shape)
    assert np.abs(prob - ref_prob).max() < 1e-6
    assert (ref_prob[:, list(R.MASK)] == 0).all()
    assert np.abs(kw - g[tag + "keywords"]).max() < 1e-6
    dprob = np.broadcast_to(g["w"].astype(np.float64), (x.shape[0], emb.shape[1])) @ emb.astype(np.float64).T
    ref_dx = R.unpack_f32(g[tag + "dx"], x.shape)
    assert np.abs(R.mode_dx(y, dprob, temp) - ref_dx).max() < 1e-6, np.abs(R.mode_dx(y, dprob, temp) - ref_dx).max()


def test_new_entries_are_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is (ctypes.c_int64 if n.endswith("_bytes") else ctypes.c_int)
    assert "NOISE CONTRACT" in text and "0x9e3779b9" in text
    assert L.sc_vq_soft_table_bytes(331, 64) == 2 * 352 * 64 * 2 and L.sc_vq_soft_table_bytes(331, 48) == 0
    assert L.sc_vq_soft_embed_workspace_bytes(16, 49408, 512, 5) == 5 * 16 * 512 * 4
    assert L.sc_vq_soft_embed_workspace_bytes(16, 49408, 512, 1) == 0
    assert L.sc_vq_soft_embed_workspace_bytes(7, 333, 64, 0) == 11 * 7 * 64 * 4            # auto never exceeds the 11 steps of 32 sub-words


def test_argument_errors_are_codes_with_a_message_and_uncovered_shapes_say_so():
    from speechclip_amd import _lib
    L = _lib.lib()
    F = ctypes.c_float
    assert L.sc_vq_gumbel_noise(None, 1 << 16, 1 << 16, 1, None) < 0 and b"2^32" in L.sc_last_error()
    assert L.sc_vq_noisy_argmax(None, None, 4, 100, 1, 1, None, 9, None) < 0 and b"n_mask=9" in L.sc_last_error()
    assert L.sc_vq_probs(None, None, 4, 100, F(0.0), 1, 1, None, 0, None) < 0 and b"temperature" in L.sc_last_error()
    assert L.sc_vq_mode_bwd(None, None, None, None, 4, 100, F(0.1), 1, 1, None, 0, None) < 0 and b"null operand" in L.sc_last_error()
    assert L.sc_vq_soft_embed(None, None, None, None, None, None, 4, 100, 48, F(0.1), 1, 1, None, 0, 0, None) == 1      # E % 64: not covered, no launch
    assert L.sc_vq_soft_embed(None, None, None, None, None, None, 4, 4, 64, F(0.1), 1, 1, None, 0, 0, None) == 1        # V < 5
    assert L.sc_vq_soft_embed(None, None, None, None, None, None, 4, 100, 64, F(0.1), 1, 1, None, 0, 0, None) < 0 and b"null operand" in L.sc_last_error()
    assert L.sc_vq_soft_embed(None, None, None, None, None, None, 0, 100, 64, F(0.1), 1, 1, None, 0, 0, None) == 0      # nothing to do
