"""Host half of the on-device image hand-over (data/image_transforms.py: resample_coeffs, clip_window_plan, load_images_raw; the sc_image_prep_* ABI).

The plan is a restatement of Pillow's 8-bit bicubic resampler (22-bit fixed-point tables, int32 accumulate from 2^21, arithmetic shift, clamp) and of the
geometry of clip_resize_center_crop_u8.  This file executes it in numpy, independently of the module's own executor, and demands EQUALITY with the installed
Pillow on every byte of every case -- and that five plausible mis-statements of the algorithm are each caught by that comparison."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from image_prep_cases import CASES_CPU, case_image, pil_crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- an independent restatement with switches for the mutants -------------------------------------------------------------------------------------------
def _filter(x):
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _coeffs(in_size, out_size, neg_round_up=False, center_outside=False):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    coef, bounds = np.zeros((out_size, ksize), np.int64), np.zeros((out_size, 2), np.int64)
    for xx in range(out_size):
        center = xx * scale + 0.5 if center_outside else (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_filter((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            coef[xx, x] = int(0.5 + v * (1 << 22)) if (v >= 0 or neg_round_up) else int(-0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def _run(img, n, acc0=1 << 21, clamp=True, floor_margin=False, tables=None, plan=None, **mut):
    """img uint8 [h, w, 3] or [h, w] -> uint8 [n, n, 3] by the stated algorithm: window only, horizontal pass on the needed rows, then vertical."""
    tables = tables or (lambda i, o: _coeffs(i, o, **mut))
    h, w = img.shape[:2]
    x = img.reshape(h, w, -1).astype(np.int64)

    def fin(acc):
        acc = acc >> 22
        return np.clip(acc, 0, 255) if clamp else acc & 255          # without the clamp: what a bare store of the low byte keeps

    if not (w == h == n):
        nw, nh = (n, int(n * h / w)) if w <= h else (int(n * w / h), n)
        top, left = ((nh - n) // 2, (nw - n) // 2) if floor_margin else (int(round((nh - n) / 2.0)), int(round((nw - n) / 2.0)))
        if plan is not None:
            assert (plan.nw, plan.nh, plan.left, plan.top, plan.hpass, plan.vpass) == (nw, nh, left, top, nw != w, nh != h)
        vt = tables(h, nh) if nh != h else None
        r0, r1 = (int(vt[1][top, 0]), int(vt[1][top + n - 1].sum()) - 1) if vt else (top, top + n - 1)
        if plan is not None:
            assert (plan.row0, plan.row1) == (r0, r1)
        x = x[r0:r1 + 1]
        if nw != w:
            coef, bounds = tables(w, nw)
            cols = []
            for xx in range(left, left + n):
                b0, c = int(bounds[xx, 0]), int(bounds[xx, 1])
                cols.append(fin(acc0 + np.tensordot(x[:, b0:b0 + c], np.asarray(coef[xx, :c], np.int64), axes=([1], [0]))))
            x = np.stack(cols, axis=1)
        else:
            x = x[:, left:left + n]
        if vt:
            coef, bounds = vt
            rows = []
            for yy in range(top, top + n):
                b0, c = int(bounds[yy, 0]), int(bounds[yy, 1])
                rows.append(fin(acc0 + np.tensordot(np.asarray(coef[yy, :c], np.int64), x[b0 - r0:b0 - r0 + c], axes=([0], [0]))))
            x = np.stack(rows, axis=0)
    return np.ascontiguousarray(np.broadcast_to(x.astype(np.uint8), (n, n, 3)))


@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("w,h,n", CASES_CPU)
def test_plan_executed_in_numpy_equals_pil_on_every_byte(w, h, n, mode):
    from speechclip_amd.data import image_transforms as T
    img = case_image(w, h, mode)
    want = pil_crop(img, n)
    plan = T.clip_window_plan(w, h, n)
    got = _run(img, n, tables=T.resample_coeffs, plan=plan)          # the module's tables and plan, this file's executor
    assert got.shape == want.shape == (n, n, 3) and np.array_equal(got, want)
    assert np.array_equal(T.execute_plan_numpy(img, n), want)       # the module's own executor
    assert np.array_equal(_run(img, n), want)                       # this file's tables too
    for i, o in ((w, plan.nw), (h, plan.nh)):
        coef, bounds = T.resample_coeffs(i, o)
        c2, b2 = _coeffs(i, o)
        assert coef.dtype == np.int32 and bounds.dtype == np.int32 and np.array_equal(coef, c2) and np.array_equal(bounds, b2)
        assert T.resample_coeffs(i, o)[0] is coef                      # cached per size pair


def test_coefficient_count_is_not_capped():
    from speechclip_amd.data import image_transforms as T
    coef, bounds = T.resample_coeffs(600, 16)
    assert coef.shape == (16, 151) and bounds[:, 1].max() == 150 and (coef[np.arange(16), bounds[:, 1] - 1] != 0).all()


MUTANTS = {
    "accumulator starts at 0": dict(acc0=0),
    "negative coefficients rounded with +0.5": dict(neg_round_up=True),
    "shift without clamp": dict(clamp=False),
    "center = xx * scale + 0.5": dict(center_outside=True),
    "crop margin by floor division": dict(floor_margin=True),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_mutant_of_the_algorithm_differs_from_pil(name):
    """The comparison above is sharp: each of these mis-statements changes at least one byte of at least one case."""
    small = [c for c in CASES_CPU if max(c[:2]) <= 100]
    differs = [(w, h, n, mode) for (w, h, n) in small for mode in ("RGB", "L")
               if not np.array_equal(_run(case_image(w, h, mode), n, **MUTANTS[name]), pil_crop(case_image(w, h, mode), n))]
    assert differs, name


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_shipped_tables_and_plan_are_not_a_mutant(name):
    """The same five mis-statements against the MODULE: the executor mutants run on the module's own tables and still differ from PIL (so the tables do not
    compensate for them), and the module's tables / crop origin differ from the mutated ones on a case where the mutation shows."""
    from speechclip_amd.data import image_transforms as T
    mut = MUTANTS[name]
    small = [(w, h, n, mode) for (w, h, n) in CASES_CPU if max(w, h) <= 100 for mode in ("RGB", "L")]
    if name in ("accumulator starts at 0", "shift without clamp", "crop margin by floor division"):
        assert any(not np.array_equal(_run(case_image(w, h, mode), n, tables=T.resample_coeffs, **mut), pil_crop(case_image(w, h, mode), n))
                   for (w, h, n, mode) in small), name
        if name == "crop margin by floor division":          # (19, 16, 16): margin 3, half-to-even gives 2 and floor 1
            assert T.clip_window_plan(19, 16, 16).left == 2 and (19 - 16) // 2 == 1
    else:
        shows = []
        for (w, h, n, mode) in small:
            p = T.clip_window_plan(w, h, n)
            for i, o in ((w, p.nw), (h, p.nh)):
                good, bad = _coeffs(i, o), _coeffs(i, o, **mut)
                if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                    shows.append((i, o))
                    coef, bounds = T.resample_coeffs(i, o)
                    assert not (np.array_equal(coef, bad[0]) and np.array_equal(bounds, bad[1])), (name, i, o)
        assert shows, name


def test_workspace_bytes_refuses_what_the_entry_refuses():
    from speechclip_amd import _lib
    from speechclip_amd.data import image_transforms as T
    L = _lib.lib()
    bp = T.plan_image_batch([case_image(100, 60, "RGB"), case_image(19, 16, "L")], 16)
    g = np.ascontiguousarray(bp.geom)
    assert L.sc_image_prep_workspace_bytes(g.ctypes.data, 2, 16) == bp.workspace_bytes > 0
    assert L.sc_image_prep_workspace_bytes(g.ctypes.data, 0, 16) == 0 and L.sc_image_prep_workspace_bytes(None, 0, 16) == 0
    for args in ((None, 2, 16), (g.ctypes.data, -1, 16), (g.ctypes.data, 2, 0), (g.ctypes.data, 2, -5)):
        assert L.sc_image_prep_workspace_bytes(*args) == -1, args
    for field, value in ((2, 2), (2, 0), (6, -1)):          # C = 2, C = 0, row1 < row0
        bad = g.copy()
        bad[0, field] = value
        assert L.sc_image_prep_workspace_bytes(bad.ctypes.data, 2, 16) == -1, (field, value)


def test_entries_are_declared_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in ("sc_image_prep_workspace_bytes", "sc_image_prep_u8"):
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
    assert L.sc_image_prep_workspace_bytes.restype is ctypes.c_int64 and L.sc_image_prep_u8.restype is ctypes.c_int
    from speechclip_amd.data import image_transforms as T
    assert f"#define SC_IMAGE_PREP_GEOM {T.GEOM_FIELDS}" in text and f"#define SC_IMAGE_PREP_HPASS {T.HPASS}" in text and f"#define SC_IMAGE_PREP_VPASS {T.VPASS}" in text
    assert "BYTE-EXACTNESS CONTRACT" in text


def test_batch_plan_and_workspace_bytes():
    """Tables once per distinct size pair, shares of the workspace back to back, and the library's size rule equal to the plan's."""
    from speechclip_amd import _lib
    from speechclip_amd.data import image_transforms as T
    imgs = [case_image(100, 60, "RGB"), case_image(100, 60, "L"), case_image(16, 16, "RGB"), case_image(60, 100, "RGB")]
    bp = T.plan_image_batch(imgs, 16, pad_bytes=7)
    assert bp.offsets[0].tolist() == [7, 7 + 18000 + 7, 2 * 7 + 24000 + 7, 3 * 7 + 24000 + 768 + 7] and bp.packed_bytes == 4 * 7 + 24000 + 768 + 18000 + 7
    rows = [int(g[6] - g[5] + 1) for g in bp.geom]
    assert bp.offsets[1].tolist() == [0, rows[0] * 16 * 3, rows[0] * 16 * 4, rows[0] * 16 * 4] and bp.workspace_bytes == rows[0] * 16 * 4 + rows[3] * 16 * 3
    assert bp.geom[0, 8] == bp.geom[1, 8] == bp.geom[3, 9] and bp.geom[0, 9] == bp.geom[1, 9] == bp.geom[3, 8]       # (100 -> 26) and (60 -> 16): stored once
    assert bp.geom[2, 7] == 0 and bp.tables.size == 2 * 3 + 26 * (2 + 17) + 16 * (2 + 17)          # ksize = 2 * ceil(2 * 100 / 26) + 1 = 17, both pairs
    g = np.ascontiguousarray(bp.geom)
    assert _lib.lib().sc_image_prep_workspace_bytes(g.ctypes.data, 4, 16) == bp.workspace_bytes
    with pytest.raises(ValueError):
        T.plan_image_batch([np.zeros((4, 4, 4), np.uint8)], 16)
    with pytest.raises(ValueError):
        T.plan_image_batch([np.zeros((4, 4, 3), np.float32)], 16)


def test_load_images_raw_keeps_rgb_and_l_and_resizes_other_modes_on_the_host(tmp_path):
    from PIL import Image
    from speechclip_amd.data import image_transforms as T
    rng = np.random.default_rng(5)
    rgb, lum = rng.integers(0, 256, (30, 41, 3), dtype=np.uint8), rng.integers(0, 256, (23, 19), dtype=np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "rgb.png")
    Image.fromarray(lum, "L").save(tmp_path / "l.png")
    Image.fromarray(rgb, "RGB").convert("P", palette=Image.ADAPTIVE, colors=17).save(tmp_path / "p.png")
    Image.fromarray(rng.integers(0, 256, (27, 35, 4), dtype=np.uint8), "RGBA").save(tmp_path / "rgba.png")
    paths = [str(tmp_path / f) for f in ("rgb.png", "l.png", "p.png", "rgba.png")]
    raw = T.load_images_raw(paths, 16)
    assert np.array_equal(raw[0], rgb) and np.array_equal(raw[1], lum)
    host = T.load_images_u8(paths, 16).numpy()
    for i in (2, 3):
        assert Image.open(paths[i]).mode in ("P", "RGBA")
        assert raw[i].shape == (16, 16, 3) and np.array_equal(raw[i], host[i])
        assert not (T.clip_window_plan(16, 16, 16).hpass or T.clip_window_plan(16, 16, 16).vpass)
    for i in range(4):          # decode + plan == the host path, all four modes
        assert np.array_equal(T.execute_plan_numpy(raw[i], 16), host[i])


def _tiny_model():
    import dataclasses
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from helpers import make_config
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.hubert import HubertConfig
    torch.manual_seed(0)
    return KWClip_GeneralTransformer(make_config(d_model=128, branch_heads=4, hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())),
                                                 clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))).eval()


def test_forward_image_refuses_a_list_that_mixes_paths_and_arrays(tmp_path):
    from PIL import Image
    model = _tiny_model()
    arr = np.zeros((20, 30, 3), np.uint8)
    Image.fromarray(arr, "RGB").save(tmp_path / "a.png")
    with pytest.raises(TypeError, match="mix"):
        model.forward_image([str(tmp_path / "a.png"), arr])
    with pytest.raises(TypeError, match="mix"):
        model.forward_image([torch.from_numpy(arr), str(tmp_path / "a.png")])
    with pytest.raises(ValueError):
        model.forward_image(torch.zeros(2, 1, 8, 8))
    with pytest.raises(TypeError):
        model.forward_image("a.png")


def test_sc_image_prep_env_values_are_checked(tmp_path, monkeypatch):
    from PIL import Image
    from speechclip_amd.data.image_transforms import load_images_u8, normalize_u8
    model = _tiny_model()
    n = model.clip.model.cfg.image_resolution
    Image.fromarray(case_image(37, 91, "RGB"), "RGB").save(tmp_path / "a.png")
    paths = [str(tmp_path / "a.png")]
    want = normalize_u8(load_images_u8(paths, n))
    for mode in ("host", "device", "auto"):          # a CPU model keeps the host path whatever the variable says
        monkeypatch.setenv("SC_IMAGE_PREP", mode)
        assert torch.equal(model.clip.prep_image(paths), want)
    assert torch.equal(model.clip.prep_image_arrays([case_image(37, 91, "RGB")]), want)
    monkeypatch.setenv("SC_IMAGE_PREP", "gpu")
    with pytest.raises(ValueError, match="SC_IMAGE_PREP"):
        model.clip.prep_image(paths)
