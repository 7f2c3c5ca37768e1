"""sc_image_prep_u8 / ops.image_prep on the device: CLIP's bicubic resize + centre crop + normalise of a ragged batch of decoded images.

Everything here is EQUALITY: the uint8 crop against PIL (clip_resize_center_crop_u8 of the same image), the f32 output against sc_image_normalize_u8 of
that crop, the device path of prep_image / forward_image against the host path.  The case list (image_prep_cases.py) is shared with the host test."""
import ctypes

import numpy as np
import pytest
import torch

from image_prep_cases import CASES_16, CASES_32, CASES_224, case_image, pil_crop

pytestmark = pytest.mark.gpu

GUARD = 4096          # sentinel elements in front of and behind every buffer the entry writes
PAD = 64              # bytes of value 255 around every image in the packed input


def _batch(cases):
    imgs = [case_image(w, h, mode) for (w, h, n) in cases for mode in ("RGB", "L")]
    return imgs, cases[0][2]


def _guarded(numel, dtype, sentinel):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, numel, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + numel:] == sentinel).all())


def _run_guarded(imgs, n, plans=None):
    """ops.image_prep (through its internal form, which takes caller-owned buffers) with outputs and workspace inside sentinel-filled guard regions and the packed input padded with 255 -> (f32, u8) on the host."""
    from speechclip_amd import ops
    from speechclip_amd.data.image_transforms import plan_image_batch
    B = len(imgs)
    ws_bytes = plan_image_batch(imgs, n, plans=plans).workspace_bytes
    fbuf, f = _guarded(B * 3 * n * n, torch.float32, 12345.0)
    ubuf, u = _guarded(B * n * n * 3, torch.uint8, 0xA5)
    wbuf, ws = _guarded(ws_bytes, torch.uint8, 0x5A)
    f32, u8 = ops._image_prep(imgs, n, return_u8=True, out=f.view(B, 3, n, n), out_u8=u.view(B, n, n, 3), workspace=ws, pad_bytes=PAD, plans=plans)
    torch.cuda.synchronize()
    assert f32.data_ptr() == f.data_ptr() and u8.data_ptr() == u.data_ptr()
    assert _intact(fbuf, f.numel(), 12345.0) and _intact(ubuf, u.numel(), 0xA5) and _intact(wbuf, ws_bytes, 0x5A)
    return f32.cpu(), u8.cpu()


@pytest.mark.parametrize("cases", [CASES_16, CASES_32, CASES_224], ids=["n16", "n32", "n224"])
def test_bytes_equal_pil_and_f32_equals_image_normalize_u8(cases):
    """The whole case list of one n_px as ONE ragged batch, and again one image per call."""
    from speechclip_amd import ops
    imgs, n = _batch(cases)
    want_u8 = torch.from_numpy(np.stack([pil_crop(im, n) for im in imgs]))
    want_f32 = ops.image_normalize_u8(want_u8.cuda()).cpu()
    f32, u8 = _run_guarded(imgs, n)
    assert torch.equal(u8, want_u8)
    assert torch.equal(f32, want_f32)
    for i, im in enumerate(imgs):
        f1, u1 = _run_guarded([im], n)
        assert torch.equal(u1[0], want_u8[i]), (im.shape, n)
        assert torch.equal(f1[0], want_f32[i]), (im.shape, n)
    # the plain call (buffers from torch's allocator, no padding, tensors instead of arrays) gives the same
    f32b = ops.image_prep([torch.from_numpy(im.copy()) for im in imgs], n)
    assert f32b.shape == (len(imgs), 3, n, n) and torch.equal(f32b.cpu(), want_f32)


def test_result_does_not_depend_on_the_order_within_the_batch():
    """Offsets, workspace shares and table indices follow the images: a permuted batch gives the permuted result."""
    imgs, n = _batch(CASES_32)
    f32, u8 = _run_guarded(imgs, n)
    perm = np.random.default_rng(3).permutation(len(imgs)).tolist()
    assert perm != sorted(perm)
    f32p, u8p = _run_guarded([imgs[i] for i in perm], n)
    assert torch.equal(u8p, u8[perm]) and torch.equal(f32p, f32[perm])


def test_one_pass_geometries_and_far_edge_windows():
    """Geometries CLIP's rule never produces (its resize always changes both sides or none) but the entry supports: one pass only, and windows at the far corner
    of the resized image.  Reference: PIL's resize of the same image to (nw, nh) and the same crop box."""
    from PIL import Image
    from speechclip_amd.data.image_transforms import ClipWindowPlan, resample_coeffs
    n = 16
    todo = []          # (w, h, nw, nh, left, top)
    for mode in ("RGB", "L"):
        todo += [(mode, 40, 20, 23, 20, 3, 2), (mode, 20, 40, 20, 23, 2, 3), (mode, 40, 20, 23, 20, 7, 4), (mode, 50, 70, 21, 29, 5, 13), (mode, 9, 11, 31, 37, 15, 21),
                 (mode, 300, 30, 17, 30, 0, 14)]
    imgs, plans, want = [], [], []
    for mode, w, h, nw, nh, left, top in todo:
        im = case_image(w, h, mode)
        row0, row1 = top, top + n - 1
        if nh != h:
            vb = resample_coeffs(h, nh)[1]
            row0, row1 = int(vb[top, 0]), int(vb[top + n - 1].sum()) - 1
        imgs.append(im)
        plans.append(ClipWindowPlan(w, h, n, nw, nh, left, top, nw != w, nh != h, row0, row1))
        ref = Image.fromarray(im, mode).resize((nw, nh), Image.BICUBIC).crop((left, top, left + n, top + n)).convert("RGB")
        want.append(np.asarray(ref, dtype=np.uint8))
    f32, u8 = _run_guarded(imgs, n, plans=plans)
    for i, t in enumerate(todo):
        assert np.array_equal(u8[i].numpy(), want[i]), t


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
                                                 clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))).cuda().eval()


def _write_pngs(tmp_path):
    from PIL import Image
    rgb = case_image(100, 60, "RGB")
    Image.fromarray(rgb, "RGB").save(tmp_path / "a.png")
    Image.fromarray(case_image(37, 91, "L"), "L").save(tmp_path / "b.png")
    Image.fromarray(case_image(33, 47, "RGB"), "RGB").convert("P", palette=Image.ADAPTIVE, colors=31).save(tmp_path / "c.png")
    Image.fromarray(case_image(225, 224, "RGB"), "RGB").save(tmp_path / "d.png")
    return [str(tmp_path / f) for f in ("a.png", "b.png", "c.png", "d.png")]


def test_prep_image_device_equals_host(tmp_path, monkeypatch):
    """SC_IMAGE_PREP is read at every call; the device path (decode on the host, geometry on the device) gives the host path's bits -- RGB, L and a mode-P file
    (resized by PIL on the host, identity plan on the device)."""
    from speechclip_amd import ops
    model = _tiny_model()
    model.clip.update_device(model.device)
    paths = _write_pngs(tmp_path)
    calls = []
    real = ops.image_prep
    monkeypatch.setattr(ops, "image_prep", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("SC_IMAGE_PREP", "host")
    host = model.clip.prep_image(paths)
    assert not calls
    monkeypatch.setenv("SC_IMAGE_PREP", "device")
    dev = model.clip.prep_image(paths)
    assert len(calls) == 1
    n = model.clip.model.cfg.image_resolution
    assert dev.is_cuda and dev.shape == (4, 3, n, n) and dev.dtype == torch.float32 and torch.equal(dev, host)
    for mode in ("auto", None):          # the default is `auto` = the device for a GPU model (profiles/image_prep_bench.txt)
        monkeypatch.setenv("SC_IMAGE_PREP", mode) if mode else monkeypatch.delenv("SC_IMAGE_PREP")
        assert torch.equal(model.clip.prep_image(paths), host)
    assert len(calls) == 3


def test_forward_image_of_decoded_arrays_equals_forward_image_of_paths(tmp_path, monkeypatch):
    from speechclip_amd.data.image_transforms import load_images_raw
    model = _tiny_model()
    paths = [p for i, p in enumerate(_write_pngs(tmp_path)) if i != 2]          # RGB, L, RGB
    arrays = load_images_raw(paths, model.clip.model.cfg.image_resolution)
    assert [a.ndim for a in arrays] == [3, 2, 3]
    from speechclip_amd import ops
    calls = []
    real = ops.image_prep
    monkeypatch.setattr(ops, "image_prep", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setenv("SC_IMAGE_PREP", "host")
        want = model.forward_image(paths)
        want_a = model.forward_image(arrays)          # PIL on the arrays
        assert not calls
        monkeypatch.setenv("SC_IMAGE_PREP", "device")
        got = model.forward_image(arrays)
        got_t = model.forward_image([torch.from_numpy(a.copy()) for a in arrays])
        got_p = model.forward_image(paths)
        assert len(calls) == 3
    assert got.shape == want.shape and all(torch.equal(x, want) for x in (want_a, got, got_t, got_p))
    with pytest.raises(TypeError):
        model.forward_image([paths[0], arrays[1]])


def test_argument_rules_give_a_code_and_a_message_without_a_launch():
    """Every rule is checked on the host copies before anything is launched.  The device arguments are real, generously sized and zero-filled device
    allocations (the tables inside a larger zero buffer), so that a rule that stops refusing makes this test FAIL on `rc` instead of launching on bad addresses."""
    from speechclip_amd import _lib
    from speechclip_amd.data.image_transforms import plan_image_batch
    L = _lib.lib()
    imgs = [case_image(100, 60, "RGB"), case_image(19, 16, "L")]
    n = 16
    bp = plan_image_batch(imgs, n)
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    packed_d, ws_d = (torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") for _ in range(2))
    out_d = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    keep = []

    def dev(a, pad_to=0):
        t = torch.zeros(max(a.size, pad_to), dtype=torch.from_numpy(a).dtype, device="cuda")
        t[:a.size] = torch.from_numpy(a.reshape(-1))
        keep.append(t)
        return t.data_ptr()

    def call(geom=bp.geom, offsets=bp.offsets, tables=bp.tables, n_px=n, packed_bytes=bp.packed_bytes, ws_bytes=bp.workspace_bytes, std=m, no_tables=False):
        g, o, t = np.ascontiguousarray(geom, np.int32), np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(tables, np.int32)
        keep.extend([g, o, t])
        rc = L.sc_image_prep_u8(packed_d.data_ptr(), packed_bytes, o.ctypes.data, dev(o), g.ctypes.data, dev(g), None if no_tables else t.ctypes.data,
                                None if no_tables else dev(t, 1 << 16), t.size, 2, n_px, ctypes.addressof(m), ctypes.addressof(std), ws_d.data_ptr(), ws_bytes,
                                out_d.data_ptr(), None, _lib.stream())
        return rc, L.sc_last_error().decode()

    def with_geom(b, field, value):
        g = bp.geom.copy()
        g[b, field] = value
        return g

    W, H, C, LEFT, TOP, ROW0, ROW1, PASSES, HTAB, VTAB = range(10)
    refused = [          # (what the message must name, the call)
        ("C=2", call(geom=with_geom(0, C, 2))),
        ("C=4", call(geom=with_geom(1, C, 4))),
        ("n_px=0", call(n_px=0)),
        ("n_px=-3", call(n_px=-3)),
        ("window", call(geom=with_geom(0, LEFT, bp.geom[0, LEFT] + 11))),          # 100 -> 26 columns: [left + 11, left + 27) leaves them
        ("window", call(geom=with_geom(1, LEFT, 4))),                              # crop only: [4, 20) of 19 columns
        ("window", call(geom=with_geom(0, TOP, -1))),
        ("needed rows", call(geom=with_geom(0, ROW1, 60))),
        ("needed rows", call(geom=with_geom(1, ROW0, -1))),
        ("needed rows", call(geom=with_geom(1, ROW0, 1))),                         # crop only: the window's rows start at 0
        ("bounds", call(geom=with_geom(0, ROW0, 1))),                              # the first window row's taps start at input row 0
        ("workspace", call(ws_bytes=bp.workspace_bytes - 1)),
        ("tables is null", call(no_tables=True)),
        ("table index", call(geom=with_geom(0, HTAB, bp.tables.size))),
        ("outside packed", call(packed_bytes=bp.packed_bytes - 1)),
        ("workspace offset", call(offsets=np.array([bp.offsets[0], bp.offsets[1] + 1]))),
        ("std", call(std=(ctypes.c_float * 3)(0.5, 0.0, 0.5))),
    ]
    for what, (rc, msg) in refused:
        assert rc != 0 and what in msg and "sc_image_prep_u8" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert not bool(out_d.any()) and not bool(ws_d.any())          # nothing ran
    assert call()[0] == 0                                          # the unmodified arguments are accepted (zero pixels in, one launch)
    torch.cuda.synchronize()
    assert bool(out_d[:2 * 3 * n * n].any()) and not bool(out_d[2 * 3 * n * n:].any())


def test_no_host_fallback(monkeypatch):
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    img = case_image(31, 17, "RGB")
    with pytest.raises(SpeechClipHipError):
        ops._image_prep([img], 16, device="cpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SpeechClipHipError, match="no CPU fallback"):
        ops.image_prep([img], 16)


def test_a_cuda_device_without_an_index_is_the_current_device(tmp_path, monkeypatch):
    """`ClipModel(name, device="cuda").cuda()` (the reference's constructor form; nn.Module.cuda() does not pass through ClipModel.to) and
    `update_device("cuda")` leave `clip.device` the bare string: prep_image works for it on the device path as it does on the host path, with equal bits."""
    from speechclip_amd import ops
    n = 16
    imgs = [case_image(31, 17, "RGB"), case_image(19, 16, "L")]
    want = ops.image_normalize_u8(torch.from_numpy(np.stack([pil_crop(im, n) for im in imgs])).cuda())
    for spelling in ("cuda", torch.device("cuda"), "cuda:0", torch.device("cuda", 0)):
        got, got_u8 = ops._image_prep(imgs, n, return_u8=True, device=spelling)
        assert got.device == want.device and got_u8.device == want.device and torch.equal(got, want), spelling
    model = _tiny_model()
    paths = _write_pngs(tmp_path)
    monkeypatch.setenv("SC_IMAGE_PREP", "host")
    model.clip.update_device(model.device)
    host = model.clip.prep_image(paths)
    for device in ("cuda", torch.device("cuda")):
        model.clip.update_device(device)
        for mode in ("host", "device", "auto"):
            monkeypatch.setenv("SC_IMAGE_PREP", mode)
            pix = model.clip.prep_image(paths)
            assert pix.device == host.device and torch.equal(pix, host), (device, mode)
        monkeypatch.delenv("SC_IMAGE_PREP")
        assert torch.equal(model.clip.prep_image(paths), host)
        assert torch.equal(model.clip.prep_image_arrays([case_image(100, 60, "RGB")]), host[:1])
