"""GPU: every GEMM kernel of csrc/gemm.hip and csrc/gemm8p.hip against the plain fp64 statement of tests/gemm_ref.py, on every dispatch path, through the C ABI
(sc_gemm_bf16, sc_gemm_bf16_batched, sc_gemm_bf16_batched2).  tools/gemm_bounds.py is the CPU self-check of statements, rounding model, bounds and mutants.

    exact     integer inputs whose fp32 accumulation is exact in any order: fp32 outputs bit-equal to the reference, 16-bit outputs bit-equal to the reference
              rounded to nearest-even once or twice, as gemm_ref.rounding_points states for the path
    bounded   real inputs: every element inside its derived bound; act = 0 and at least 4096 outputs: both 6 / sqrt(n) statistics of the signed ratio
    then      repeatability per path, mode 16 against mode 26, the scalar-fallback against the vector epilogue of gemm256_kernel, and the argument rules

Every operand lies inside a flat buffer of NaN (in front, behind, and in the gaps of lda > K, ldw > K, ldr > N): a read of anything the operation does not own
poisons an output.  Every output lies in a sentinel-filled window: everything outside [M, :N] must still hold the sentinel -- ldc padding and the gaps between
batched products included -- and everything inside must have been written.  Every operand is sized so that what the operation owns is mapped; nothing here
relies on a fault.  The kernel each case must reach is asserted through sc_gemm_last_path() and the restated dispatcher (tests/test_gemm_bounds_cpu.py).
The limit of that assertion: sc_gemm_last_path() tells gemm8p (3) and the vendor comparator (1) from the kernels of gemm.hip (0), and is set by sc_gemm_bf16 only.
WHICH kernel of gemm.hip ran -- gemm256_kernel, its BATCH variant or gemm_bf16_kernel, and every batched call -- rests on the Python restatement of gemm_dispatch
with the library's constants (100 tiles; the batched entries never consult the vendor path).  The dispatcher reads nothing from the environment any more (the
PROBES build of earlier revisions read SC_GEMM_MIN_TILES, SC_GEMM_V1 and SC_GEMM_NOBATCH256 and would choose differently, so a run against such a library still
asserts that they are unset); the comparator switch SC_GEMM_VENDOR must be unset.
Each test prints its figures (-s); profiles/gemm_parity.txt holds the table of one run."""
import os

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu
F64, F32 = G.F64, G.F32
NAN = float("nan")
DISPATCH_KNOBS = ("SC_GEMM_MIN_TILES", "SC_GEMM_V1", "SC_GEMM_NOBATCH256", "SC_GEMM_VENDOR")

CASES = G.all_cases()
EXACT = [c for c in CASES if c.kind == "exact"]
REAL = [c for c in CASES if c.kind == "real"]


def _flat(n, dt):
    return torch.full((2 * G.PAD + n,), NAN, dtype=dt, device="cuda")


def _put(flat, off, vals, ld, dt):
    """vals fp64 [rows, cols] -> rows of pitch ld, the first at element PAD + off"""
    rows, cols = vals.shape
    torch.as_strided(flat, (rows, cols), (ld, 1), G.PAD + off).copy_(vals.to(F32).to(dt))


def _ptr(flat):
    return flat.data_ptr() + G.PAD * flat.element_size()


class Call:
    """the device operands of one case, built once; run() launches into a fresh guarded output"""

    def __init__(self, c, inp):
        self.c, L = c, G.layout(c)
        self.L, Z, odt, rdt = L, G.nprod(c), G.op_dt(c), G.out_dt(c)
        M, N, K = c.M, c.N, c.K
        rowsA = (M - 1) * c.lda
        if c.api == "gemm":
            if "Aflat" in inp:
                self.A = _flat(inp["Aflat"].numel(), odt)
                self.A[G.PAD:G.PAD + inp["Aflat"].numel()] = inp["Aflat"].to(F32).to(odt)
            else:
                self.A = _flat(rowsA + K, odt)
                _put(self.A, 0, inp["A"][0], c.lda, odt)
            self.W = _flat((N - 1) * c.ldw + K, odt)
            _put(self.W, 0, inp["W"][0], c.ldw, odt)
        elif c.api == "batched":
            self.A = _flat((Z - 1) * L["strideA"] + rowsA + K, odt)
            self.W = _flat((c.w_mod - 1) * L["strideW"] + (N - 1) * c.ldw + K, odt)
            for z in range(Z):
                _put(self.A, z * L["strideA"], inp["A"][z], c.lda, odt)
            for z in range(c.w_mod):
                _put(self.W, z * L["strideW"], inp["W"][z], c.ldw, odt)
        else:
            self.A = _flat((c.S - 1) * L["strideA"] + rowsA + c.inner * K, odt)
            self.W = _flat((c.S - 1) * L["strideW"] + (c.inner - 1) * L["strideW2"] + (N - 1) * c.ldw + K, odt)
            for z in range(Z):
                zo, zi = divmod(z, c.inner)
                _put(self.A, zo * L["strideA"] + zi * L["strideA2"], inp["A"][z], c.lda, odt)
                _put(self.W, zo * L["strideW"] + zi * L["strideW2"], inp["W"][z], c.ldw, odt)
        self.bias = self.res = None
        if inp["bias"] is not None:
            self.bias = _flat(inp["bias"].numel(), F32)
            self.bias[G.PAD:G.PAD + inp["bias"].numel()] = inp["bias"].reshape(-1).to(F32)
        if inp["res"] is not None:
            self.res = _flat((M - 1) * c.ldr + N, rdt)
            _put(self.res, 0, inp["res"], c.ldr, rdt)

    def run(self, mode=None, check_path=True):
        """-> (outputs fp64 [Z, M, N], the whole guarded buffer as left by the kernel)"""
        from speechclip_amd import ops
        from speechclip_amd._lib import GEMM_F16, GEMM_OUT_F32, lib, stream
        c, L, dt = self.c, self.L, G.out_dt(self.c)
        Z, M, N, K = G.nprod(c), c.M, c.N, c.K
        if c.api == "gemm":
            go = G.Guarded(M, c.ldc, dt, N)
        elif c.api == "batched":
            go = G.Guarded(1, (Z - 1) * L["strideC"] + M * c.ldc, dt)
        else:
            go = G.Guarded(c.S * M, c.ldc, dt, c.inner * N)
        flags = c.act | (GEMM_OUT_F32 if c.out == 32 else 0) | (GEMM_F16 if c.f16 else 0)
        bias, res = (0 if self.bias is None else _ptr(self.bias)), (0 if self.res is None else _ptr(self.res))
        mode = c.mode if mode is None else mode
        knobs = [k for k in DISPATCH_KNOBS if os.environ.get(k)]
        assert not knobs and not ops.vendor_gemm_enabled(), (knobs, "the restated dispatcher holds for the product library's constants only")
        try:
            lib().sc_debug_set_gemm_mode(mode)
            if c.api == "gemm":
                rc = lib().sc_gemm_bf16(_ptr(self.A), c.lda, _ptr(self.W), c.ldw, go.win.data_ptr(), c.ldc, bias, res, c.ldr, M, N, K, flags, stream())
                path = lib().sc_gemm_last_path()
            elif c.api == "batched":
                rc = lib().sc_gemm_bf16_batched(_ptr(self.A), c.lda, L["strideA"], _ptr(self.W), c.ldw, L["strideW"], c.w_mod, go.win.data_ptr(), c.ldc, L["strideC"],
                                                bias, M, N, K, Z, flags, stream())
                path = 0
            else:
                rc = lib().sc_gemm_bf16_batched2(_ptr(self.A), c.lda, L["strideA"], L["strideA2"], _ptr(self.W), c.ldw, L["strideW"], L["strideW2"], go.win.data_ptr(),
                                                 c.ldc, L["strideC"], L["strideC2"], M, N, K, c.S, c.inner, flags, stream())
                path = 0
        finally:
            lib().sc_debug_set_gemm_mode(-1)
        assert rc == 0, (c.id, rc, lib().sc_last_error().decode())
        torch.cuda.synchronize()
        if check_path:
            d = G.dispatch(c._replace(mode=mode))
            assert d["path"] == c.path and path == d["last_path"], (c.id, mode, d, path)
        win = go.check(c.id)
        if c.api == "gemm":
            got = win.unsqueeze(0)
        elif c.api == "batched":
            flat = win.reshape(-1)
            owned = torch.zeros(flat.numel(), dtype=torch.bool)
            for z in range(Z):
                torch.as_strided(owned, (M, N), (c.ldc, 1), z * L["strideC"]).fill_(True)
            assert bool((flat[~owned] == go.sent).all()), (c.id, "wrote between the products or into the ldc padding")
            got = torch.stack([torch.as_strided(flat, (M, N), (c.ldc, 1), z * L["strideC"]).clone() for z in range(Z)])
        else:
            got = torch.stack([win[(z // c.inner) * M:(z // c.inner + 1) * M, (z % c.inner) * N:(z % c.inner + 1) * N] for z in range(Z)])
        assert not bool((got == go.sent).any()), (c.id, "an element of the output was not written", int((got == go.sent).sum()))
        return got, go.buf


def _first_diff(a, b):
    ne = (a != b) | (torch.isnan(a) != torch.isnan(b))
    if not bool(ne.any()):
        return None
    i = int(ne.reshape(-1).to(torch.uint8).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape))
    return idx, float(a[idx]), float(b[idx]), int(ne.sum())


def _check_exact(c, got, r):
    dt = G.out_dt(c)
    want = G.expected_bits(c, r)
    gb = got.to(F32).to(dt)
    d = _first_diff(gb, want)
    print(f"{c.id:44s} {c.path:14s} exact   {G.rounding_points(c):5s} {'bit-equal' if d is None else 'DIFFERS'}   {got.numel()} outputs")
    assert torch.equal(gb, want), (c.id, "first difference at", d[0], "got", d[1], "want", d[2], "differing", d[3], "pre-residual", float(r["val"][d[0]]),
                                   "residual", float(r["res"][d[0][1:]]))
    if c.out == 16 and c.res:      # the case must be able to tell the two rounding models apart, or its bit-equality says nothing about the rounding points
        other = "once" if G.rounding_points(c) == "twice" else "twice"
        assert torch.equal(G.model_bits(c, r, G.rounding_points(c)), want) and not torch.equal(G.model_bits(c, r, other), want), (c.id, "`once` and `twice` give the same bits")


def _check_bounded(c, got, inp, r):
    bd, _ = G.bound(c, inp, r)
    ratio = G.judge(c.id, got, r["out"], bd)
    line = f"{c.id:44s} {c.path:14s} bounded {G.rounding_points(c):5s} worst err/bound {ratio:7.4f}"
    if G.wants_stats(c):
        n, s1, s2, lim = G.stats(got, r["out"], bd)
        print(f"{line}   n {n:9d}  |mean r| {s1:.5f}  |mean sign(ref) r| {s2:.5f}  limit {lim:.5f}")
        assert s1 <= lim and s2 <= lim, (c.id, "statistics of the signed ratio", n, s1, s2, lim)
    else:
        print(line)


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.id)
def test_exact(c):
    inp = G.inputs(c)
    got, _ = Call(c, inp).run()
    _check_exact(c, got, G.ref(c, inp))


@pytest.mark.parametrize("c", REAL, ids=lambda c: c.id)
def test_bounded(c):
    inp = G.inputs(c)
    got, _ = Call(c, inp).run()
    _check_bounded(c, got, inp, G.ref(c, inp))


def _one_per_path():
    seen, out = set(), []
    for c in CASES:
        key = (c.path, c.api)
        if key not in seen and c.kind == "real" and G.nprod(c) * c.M * c.N >= 4096:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _one_per_path(), ids=lambda c: c.id)
def test_repeatable(c):
    """the same call twice: the same bits, guards included (K rotation and the dynamic tile order change the order of tiles, never of a sum)"""
    call = Call(c, G.inputs(c))
    _, a = call.run()
    _, b = call.run()
    assert torch.equal(a.view(torch.int32 if a.dtype == F32 else torch.int16), b.view(torch.int32 if b.dtype == F32 else torch.int16)), c.id


def test_dynamic_and_static_tile_order_give_the_same_bits():
    """mode 16 (tiles from the per-XCD counters) against mode 26 (the static stride order) on the shape with more tiles than blocks"""
    pair = [c for c in CASES if c.also == "switch" and c.kind == "real"]
    assert {c.mode for c in pair} == {16, 26}
    c = [k for k in pair if k.mode == 16][0]
    assert G.dispatch(c)["order"] == "dyn" and G.dispatch(c._replace(mode=26))["order"] == "static"
    call = Call(c, G.inputs(c))
    _, dyn = call.run(16)
    _, static = call.run(26)
    assert torch.equal(dyn.view(torch.int16), static.view(torch.int16)), _first_diff(dyn.float(), static.float())


def test_scalar_fallback_and_vector_epilogue_agree_without_residual():
    """gemm256_kernel, one exact-integer problem (non-symmetric W: a transposed fragment or store shows), no residual: the vector epilogue (ldc = N) and the scalar
    fallback (ldc = N + 4) round once each and must give the same bits."""
    c = G._c("g256-x-2560x2560x256-fallback", "g256", 0, "exact", 2560, 2560, 256)
    inp = G.inputs(c)
    assert G.epilogue256(c) == "vector" and G.epilogue256(c._replace(ldc=c.N + 4)) == "scalar"
    vec, _ = Call(c, inp).run()
    sca, _ = Call(c._replace(ldc=c.N + 4), inp).run()
    assert torch.equal(vec, sca), _first_diff(vec, sca)
    _check_exact(c, vec, G.ref(c, inp))


BAD_ARGS = (("K % 64 != 0", dict(K=96), "K=96"), ("N % 4 != 0", dict(N=62), "N=62"), ("M = 0", dict(M=0), "empty problem"), ("lda % 8 != 0", dict(lda=68), "lda"),
            ("null A", dict(null="A"), "null operand"), ("null W", dict(null="W"), "null operand"), ("null C", dict(null="C"), "null operand"))


@pytest.mark.parametrize("what,change,msg", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
def test_argument_rules_refuse_and_launch_nothing(what, change, msg):
    from speechclip_amd._lib import lib, stream
    M, N, K, lda = (change.get(k, v) for k, v in (("M", 64), ("N", 64), ("K", 64), ("lda", 64)))
    a = torch.ones(64 * 128, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(64 * 128, dtype=torch.bfloat16, device="cuda")
    go = G.Guarded(64, 64, torch.bfloat16)
    null = change.get("null")
    for mode in (-1, 0, 16):
        try:
            lib().sc_debug_set_gemm_mode(mode)
            rc = lib().sc_gemm_bf16(0 if null == "A" else a.data_ptr(), lda, 0 if null == "W" else w.data_ptr(), 128, 0 if null == "C" else go.win.data_ptr(), 64,
                                    0, 0, 0, M, N, K, 0, stream())
        finally:
            lib().sc_debug_set_gemm_mode(-1)
        err = lib().sc_last_error().decode()
        assert rc < 0 and msg in err, (what, mode, rc, err)
    torch.cuda.synchronize()
    assert bool((go.buf == go.sent).all()), what


def test_two_level_batch_refuses_more_than_65535_products():
    from speechclip_amd._lib import lib, stream
    a = torch.ones(64 * 64, dtype=torch.bfloat16, device="cuda")
    go = G.Guarded(64, 64, torch.bfloat16)
    rc = lib().sc_gemm_bf16_batched2(a.data_ptr(), 64, 0, 0, a.data_ptr(), 64, 0, 0, go.win.data_ptr(), 64, 0, 0, 64, 64, 64, 256, 256, 0, stream())
    err = lib().sc_last_error().decode()
    assert rc < 0 and "outer*inner=65536" in err, (rc, err)
    torch.cuda.synchronize()
    assert bool((go.buf == go.sent).all())
