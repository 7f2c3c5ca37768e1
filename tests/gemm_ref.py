"""Plain fp64 statements, case lists per dispatch path, deterministic inputs, the per-path rounding model and DERIVED per-element bounds of the 16-bit GEMM kernels
(csrc/gemm.hip: gemm_bf16_kernel<128,64 / 128,128, F16>, gemm256_kernel and its BATCH variant; csrc/gemm8p.hip: gemm8p_pers_kernel) for
tests/test_gemm_parity_gpu.py and tools/gemm_bounds.py.  A helper module, not a test; no kernel runs here.  The constants, the generator, the rounding helper, the
guarded window and the judge are those of tests/row_kernels_ref.py and are imported, not restated.

The operation:  C[M, N] = act(A[M, K] W[N, K]^T + bias) + residual, fp64 torch on the CPU (the largest reference, 8525 x 2048 x 384, is 6.7 GFLOP and about a second with its magnitude
product: the device's fp64 matmul would be faster but is not needed, and the CPU product shares nothing with the kernels under test).

Two kinds of inputs, both from gen(case id):
    exact   A, W integers in [-3, 3], bias integers in [-16, 16], residual integers in [-64, 64]; act = 0 only.  Every product and every partial sum is an integer
            below 2^24 (9 K + 16 + 64 <= 4112), so the fp32 accumulation is exact in ANY order, under any K rotation, whatever the matrix core's adders round
            like, and started from the bias or not: the stores are the only inexact operations.  fp32 outputs must equal the reference bit for bit, 16-bit
            outputs the reference rounded to nearest-even once or twice (rounding_points).  For a 16-bit output A and W are drawn from [0, 3] and the bias
            from [-12, 16]: every output is then >= -76 and the sentinel -77 of the guarded window is not a legal output (fp32 outputs: sentinel -7777, out of
            reach of any sum); the mean 2.25 K of such a sum also puts it above 256 from K = 128 on, where bf16 has to round and `once` and `twice` part ways
            (IEEE half is exact up to 2048, which no sum here reaches: its 16-bit exact cases check placement and accumulation, its real cases the store).
            The price: EVERY exact case with a 16-bit output has non-negative operands.  Exactness with signed operands is proven through the fp32-output
            exact cases alone -- the same k-loops, the output type changes only the epilogue -- and signed values meet the 16-bit stores in the real cases.
    real    0.5 randn for A, K^-0.5 randn for W, randn for bias and residual, each rounded to the type the kernel reads before the reference sees it.

The bound of a real case, per element (U = 2^-24, TR = 2^-22, BF_STORE, H16_STORE: row_kernels_ref.py):
    products        two 8-bit (bf16) or 11-bit (half) significands: exact in fp32
    accumulation    K u_acc sum_k |a_k w_k| with u_acc = 2^-23, the sum through a second fp64 product of the absolute values.  The chain is taken as K additions;
                    no ISA document is on hand for the rounding of the matrix core's internal adds, so one factor 2 over U is BUDGETED, as TR was.
                    gemm8p_pers_kernel starts its accumulators FROM the bias (its init_q): the bias then sits in each of the K / 32
                    accumulator updates, (K / 32) u_acc |bias| on top.
    bias, residual  one U |result| each
    activation      the pre-activation's error through |gelu'| <= GELU_LIP (1.13; QuickGELU's largest slope is 1.10), plus the form's own constant:
                      gelu_erf          GELU_ERF_FIT + (2 TR + 8 U) |want|        the 16-bit bf16 outputs of gemm_bf16_kernel          (its epilogue)
                      gelu_erf_precise  GELU_PRECISE (1 + |u|)                     its fp32 and IEEE-half outputs                       (its epilogue)
                      gelu_poly2_f32    1.7e-5 on [-4.25, 4.25]; beyond, Phi is held at 1 - 7e-6 / 7e-6: 7e-6 |u| on top  (common.h)    fp32 outputs of gemm256 / gemm8p
                      gelu_poly2[_x8]   GELU_POLY2_ABS + GELU_POLY2_REL |want|, which already holds the 16-bit store      16-bit outputs of gemm256 / gemm8p
                      quick_gelu        x rcp(1 + exp(-1.702 x)): the argument's two products reach the result as 1.702 |x| 2^-23, one exp and one rcp at TR,
                                        the add and the last product at U:  (2 TR + 2 U + 1.702 |u| 2^-23) |want|
    stores          fp32: none beyond the operations above.  16 bit: one store term of the result, and -- `twice` -- one more of the pre-residual value.

rounding_points(case) states where a 16-bit result is rounded; dispatch(case) restates the host's kernel choice.  The two-statistic check of the signed ratio
r = (got - ref) / bound (stats): |mean r| and |mean sign(ref) r| each within 6 / sqrt(n) -- Hoeffding for n values in [-1, 1], below 1e-7 per case under
independence; the second is what a store that truncates moves (to about 0.7: half an ulp toward zero on average).  Its expectation under exact round-to-nearest is not quite zero: the error of a
rounding is uniform in x, the ratio divides it by a bound proportional to |x|, and the smaller |x| of a rounding interval weigh more -- ideal bf16 stores of 1.8e7
normal values give -5.8e-4 (once) and -8.8e-4 (twice) on the CPU.  That stays inside 6 / sqrt(n) up to n of about 4e7; the largest case here has 1.84e7 outputs
(asserted in tests/test_gemm_bounds_cpu.py), and a case list that grows past that has to subtract this expectation first.

Mutants (MUTANTS): wrong kernels stated in fp64; every one must leave its bound or break bit-equality on a case it applies to (tools/gemm_bounds.py)."""
import collections

import torch

from row_kernels_ref import (BF, BF_STORE, F32, F64, GELU_ERF_FIT, GELU_LIP, GELU_POLY2_ABS, GELU_POLY2_REL, GELU_PRECISE, H16, H16_STORE, SENT16, SENT32,  # noqa: F401
                             TR, U, Guarded, gelu64, gen, judge, rnd, store_bound, worst)

U_ACC = 2.0 ** -23
GELU_POLY2_F32, GELU_POLY2_F32_CLAMP, GELU_POLY2_F32_TAIL = 1.7e-5, 4.25, 7e-6
N_CU = 256                                  # compute units of the MI355X: grid of the persistent kernels = min(tiles, N_CU)
PAD = 4096                                  # NaN elements in front of and behind every operand
ORDERS = ("seq", "rot32")

GemmCase = collections.namedtuple("GemmCase", "id path mode api kind M N K lda ldw ldc ldr act bias res out f16 S w_mod inner also")
PATHS = ("bf128x64", "bf128x128", "h128x64", "h128x128", "g256", "g256_batch", "bf128_batched", "g8p_pers")
ROWS128 = ("bf128x64", "bf128x128", "h128x64", "h128x128", "bf128_batched")


def _c(cid, path, mode, kind, M, N, K, api="gemm", lda=0, ldw=0, ldc=0, ldr=0, act=0, bias=True, res=False, out=16, f16=False, S=1, w_mod=1, inner=0, also=""):
    """leading dimensions 0: tight (K, K, N, ldc).  `also`: what else the case is in the list for (asserted by the case-count test)."""
    if api == "batched2":       # two-level batch: an A row holds `inner` K-slices, a C row `inner` N-slices and 4 columns of padding
        lda, ldc = inner * K, inner * N + 4
    lda, ldw = lda or K, ldw or K
    ldc = ldc or N
    ldr = (ldr or ldc) if res else 0
    return GemmCase(cid, path, mode, api, kind, M, N, K, lda, ldw, ldc, ldr, act, bias, res, out, f16, S, w_mod, inner, also)


def op_dt(c):
    return H16 if c.f16 else BF


def out_dt(c):
    return F32 if c.out == 32 else op_dt(c)


def nprod(c):
    return c.S * c.inner if c.api == "batched2" else c.S


# ================================================================================================ the dispatcher, restated
def gemm8p_try(c, mode):
    """sc_gemm8p_try (gemm8p.hip): None where it declines, else (path, tile order, column band)"""
    f32 = c.out == 32
    if c.N % 256 or c.N > 8192 or c.K % 64 or c.M < 256:
        return None
    nk = c.K // 64
    if nk < 2:
        return None
    al = 4 if f32 else 8
    if c.ldc % al or (c.res and c.ldr % al) or c.lda % 8 or c.ldw % 8:
        return None
    tiles = -(-c.M // 256) * (c.N // 256)
    band = 4 if (mode == -1 and c.N // 256 >= 16) else 0
    pg = min(tiles, N_CU)
    dyn = mode != 26 and nk >= 6 and c.N < 8192 and pg >= 8
    return "g8p_pers", ("dyn" if dyn else "static"), band


def gemm_dispatch(c, batch):
    """gemm_dispatch (gemm.hip) -> path"""
    if c.f16:
        return "h128x64" if c.N <= 64 else "h128x128"
    t256 = -(-c.M // 256) * -(-c.N // 256)
    if batch == 1 and c.N >= 256 and c.M >= 256 and t256 >= 100:
        return "g256"
    if batch > 1 and c.inner == 0 and not c.bias and not c.res and c.act == 0 and c.N >= 256 and c.M >= 256 and t256 * batch >= 100:
        return "g256_batch"
    if batch > 1 or c.api != "gemm":
        return "bf128_batched"
    return "bf128x64" if c.N <= 64 else "bf128x128"


def arg_error(c):
    """the argument rules of sc_gemm_bf16 / gemm_dispatch / the batched entries: a message where the call must be refused, else None"""
    if c.api == "batched2" and not (c.S > 0 and c.inner > 0 and c.S * c.inner <= 65535):
        return "outer*inner"
    if c.api == "batched" and c.S > 65535:
        return "batch"
    if not (c.K > 0 and c.K % 64 == 0):
        return "K"
    if not (c.N > 0 and c.N % 4 == 0):
        return "N"
    if not (c.M > 0 and nprod(c) > 0):
        return "M"
    if c.lda % 8 or c.ldw % 8 or c.ldc % 4:
        return "ld"
    return None


def dispatch(c):
    """-> dict(path, last_path (sc_gemm_last_path: 3 gemm8p, 0 the kernels of gemm.hip), order, band, kpair, epilogue).  The `dflt_ok` / `aligned` rule of
    sc_gemm_bf16 (every operand of this suite is 16-byte aligned), the refusals and the `dyn` rule of sc_gemm8p_try, gemm_dispatch."""
    assert arg_error(c) is None, (c.id, arg_error(c))
    d = dict(order=None, band=0, kpair=0, last_path=0)
    if c.api == "gemm":
        if c.mode != 0:
            dflt_ok = c.N % 256 == 0 and c.N <= 8192 and -(-c.M // 256) * (c.N // 256) >= 128
            if c.mode > 0 or dflt_ok:
                t = gemm8p_try(c, c.mode)
                if t is not None:
                    d.update(path=t[0], order=t[1], band=t[2], last_path=3, epilogue="f32" if c.out == 32 else "vector")
                    return d
        d["path"] = gemm_dispatch(c, 1)
        if c.lda < c.K and c.K == 3 * (c.lda // 2) and (c.lda // 2) % 64 == 0:
            d["kpair"] = c.lda // 2 // 64
    else:
        d["path"] = gemm_dispatch(c, nprod(c))
    if d["path"] == "g256":
        tn = -(-c.N // 256)
        d["band"] = 4 if tn >= 16 else 0
    d["epilogue"] = epilogue256(c) if d["path"] in ("g256", "g256_batch") else ("f32" if c.out == 32 else "direct")
    return d


def epilogue256(c):
    """which epilogue of gemm256_kernel a call takes (its vec_ok / f32_ok): "vector" (fast or predicated), "f32", or the "scalar" fallback"""
    if c.out == 16 and c.N % 8 == 0 and c.ldc % 8 == 0 and (not c.res or c.ldr % 8 == 0):
        return "vector"
    if c.out == 32 and c.N % 4 == 0 and c.ldc % 4 == 0 and (not c.res or c.ldr % 4 == 0):
        return "f32"
    return "scalar"


def fast_epilogue_runs(c):
    """gemm256_kernel's fast epilogue (its fast_epi): no residual operand, vector stores, at least two k-steps, an interior tile of a block that has a NEXT tile --
    so more tiles than blocks.  True where some tile of the case takes it."""
    tiles = -(-c.M // 256) * -(-c.N // 256)
    return c.path == "g256" and not c.res and epilogue256(c) == "vector" and c.K >= 128 and tiles > N_CU and c.M >= 512 and c.N >= 512


def rounding_points(c):
    """Where a 16-bit result with a residual is rounded -> "once" or "twice".

    twice: act(y + bias) is rounded to the output type, the residual (read in that type) is added in fp32 and the sum is rounded again --
        gemm256_kernel, vector epilogue      gemm.hip: epi_bf16 (pack2bf), then the residual add of the predicated vector epilogue (the fast epilogue takes no residual)
        gemm8p_pers_kernel                   gemm8p.hip: `shuffled` (pack2x) of the 16-bit epilogue, then add_packed behind the explicit residual loads
    once: the residual is added to the fp32 value and the sum is rounded --
        gemm_bf16_kernel                     gemm.hip: the residual branch of its epilogue
        gemm256_kernel, scalar fallback      gemm.hip: the residual branch of the scalar epilogue (N % 8 != 0, ldc % 8 != 0 or ldr % 8 != 0)
    fp32 outputs are never rounded to 16 bits (gemm.hip: the out_f32 stores of gemm_bf16_kernel and of gemm256_kernel's fp32 and scalar epilogues; gemm8p.hip: both arms of the F32 epilogue), and without a residual there is one store: once."""
    if c.out == 32 or not c.res:
        return "once"
    if c.path == "g8p_pers":
        return "twice"
    if c.path == "g256" and epilogue256(c) == "vector":
        return "twice"
    return "once"


def gelu_form(c):
    if c.path in ROWS128:
        return "erf_precise" if (c.out == 32 or c.f16) else "erf_fit"
    return "poly2_f32" if c.out == 32 else "poly2_half"


# ================================================================================================ case lists
M128 = (1, 15, 16, 17, 127, 128, 129)
N64, K64 = (4, 8, 60, 64), (64, 128, 448)
N128 = (68, 128, 132, 252, 260)
# (out, bias, res, act) rotations: exact cases take act 0 only; a 16-bit exact case with a residual needs roundings to tell `once` from `twice` (K >= 128, >= 4096 outputs)
_EXACT_OPTS = ((32, True, True), (16, True, False), (32, False, False), (16, False, False), (32, True, False))
_REAL_OPTS = ((16, True, True, 0), (32, True, True, 1), (16, True, False, 1), (32, False, True, 0), (16, True, True, 2), (32, True, False, 2), (16, False, False, 0),
              (16, True, True, 1), (32, True, True, 0))


def _grid128(path, Ns, Ms, f16):
    out, i = [], 0
    for ni, N in enumerate(Ns):
        for mi, M in enumerate(Ms):
            K = K64[(ni + mi) % 3]
            eo, eb, er = _EXACT_OPTS[i % len(_EXACT_OPTS)]
            ro, rb, rr, ra = _REAL_OPTS[i % len(_REAL_OPTS)]
            pre = "h" if f16 else "bf"
            out.append(_c(f"{pre}-x-{M}x{N}x{K}-o{eo}{'-b' if eb else ''}{'-r' if er else ''}", path, -1, "exact", M, N, K, out=eo, bias=eb, res=er, f16=f16))
            out.append(_c(f"{pre}-r-{M}x{N}x{K}-o{ro}{'-b' if rb else ''}{'-r' if rr else ''}-a{ra}", path, -1, "real", M, N, K, out=ro, bias=rb, res=rr, act=ra, f16=f16))
            i += 1
    return out


def cases_bf128x64():
    out = _grid128("bf128x64", N64, M128, False)
    out += [_c("bf-x-129x64x448-o16-b-r", "bf128x64", -1, "exact", 129, 64, 448, res=True, also="once"),
            _c("bf-x-64x64x64-o32-square", "bf128x64", -1, "exact", 64, 64, 64, out=32, also="square"),
            _c("bf-r-129x60x128-ldw", "bf128x64", -1, "real", 129, 60, 128, ldw=136, lda=144, res=True, ldc=68, ldr=76, also="ldw")]
    return out


def cases_bf128x128():
    out = _grid128("bf128x128", N128, M128 + (257,), False)
    out += [_c("bf-x-257x260x448-o16-b-r", "bf128x128", -1, "exact", 257, 260, 448, res=True, also="once"),
            _c("bf-r-2400x2304x64-below100", "bf128x128", -1, "real", 2400, 2304, 64, res=True, also="below100"),
            _c("bf-x-2400x2304x128-below100", "bf128x128", -1, "exact", 2400, 2304, 128, out=32, res=True, also="below100"),
            _c("bf-r-257x132x128-ldw", "bf128x128", -1, "real", 257, 132, 128, ldw=136, lda=136, res=True, ldc=140, ldr=136, also="ldw"),
            _c("bf-r-300x260x192-conv", "bf128x128", -1, "real", 300, 260, 192, lda=64, also="overlap"),
            # mode 16 and N > 8192: sc_gemm8p_try declines (the bias vector of gemm8p_pers_kernel sits in LDS), 33 tiles go to this kernel.  (The ids, and with
            # them the inputs, are those the cases had when a per-tile ping-pong kernel answered for them.)
            _c("g8p-tile-x-256x8448x128", "bf128x128", 16, "exact", 256, 8448, 128, also="declined8p"),
            _c("g8p-tile-r-256x8448x128", "bf128x128", 16, "real", 256, 8448, 128, res=True, also="declined8p")]
    return out


def cases_f16():
    out = _grid128("h128x64", N64, (1, 17, 129), True) + _grid128("h128x128", N128, (1, 16, 129, 257), True)
    out += [_c("h-r-4096x256x128-big", "h128x128", -1, "real", 4096, 256, 128, f16=True, res=True, also="stats"),
            _c("h-r-129x64x128-ldw", "h128x64", -1, "real", 129, 64, 128, f16=True, ldw=136, also="ldw")]
    return out


def cases_g256():
    C, out, i = _c, [], 0
    ks = (64, 128, 192, 448)
    for mi, M in enumerate((2560, 2561, 2815)):
        for ni, N in enumerate((2560, 2312, 2308)):
            K = ks[(mi + 2 * ni) % 4]
            if i % 2 == 0:
                eo, eb, er = _EXACT_OPTS[(i // 2) % len(_EXACT_OPTS)]
                out.append(C(f"g256-x-{M}x{N}x{K}-o{eo}{'-b' if eb else ''}{'-r' if er else ''}", "g256", 0, "exact", M, N, K, out=eo, bias=eb, res=er))
            else:
                ro, rb, rr, ra = _REAL_OPTS[(i // 2) % len(_REAL_OPTS)]
                out.append(C(f"g256-r-{M}x{N}x{K}-o{ro}{'-b' if rb else ''}{'-r' if rr else ''}-a{ra}", "g256", 0, "real", M, N, K, out=ro, bias=rb, res=rr, act=ra))
            i += 1
    out += [C("g256-x-2561x2560x448-o16-b-r-twice", "g256", 0, "exact", 2561, 2560, 448, res=True, also="twice"),
            C("g256-x-2560x2308x448-o16-b-r-once", "g256", 0, "exact", 2560, 2308, 448, res=True, also="once"),
            C("g256-r-2815x2560x448-o16-b-r", "g256", 0, "real", 2815, 2560, 448, res=True, also="largest"),
            C("g256-r-2560x2560x64-nk1", "g256", 0, "real", 2560, 2560, 64, also="nk1"),
            C("g256-r-2561x2312x128-gelu16", "g256", 0, "real", 2561, 2312, 128, act=1, also="gelu16"),
            C("g256-r-2561x2308x128-gelu16-scalar", "g256", 0, "real", 2561, 2308, 128, act=1, res=True, also="gelu16"),
            C("g256-r-2560x2312x128-qgelu32", "g256", 0, "real", 2560, 2312, 128, act=2, out=32, res=True),
            C("g256-r-1793x4104x128-band", "g256", 0, "real", 1793, 4104, 128, also="band"),
            C("g256-x-1793x4104x128-band", "g256", 0, "exact", 1793, 4104, 128, out=32, also="band"),
            C("g256-x-2560x2560x192-lda128-pair", "g256", 0, "exact", 2560, 2560, 192, lda=128, out=32, also="kpair"),
            C("g256-r-2561x2560x384-lda256-pair", "g256", 0, "real", 2561, 2560, 384, lda=256, res=True, also="kpair"),
            C("g256-x-2561x2560x192-lda64-overlap", "g256", 0, "exact", 2561, 2560, 192, lda=64, out=32, also="overlap"),
            C("g256-r-2560x2560x128-ldaK+8", "g256", 0, "real", 2560, 2560, 128, lda=136, also="lda>K"),
            C("g256-r-2561x2560x128-ldcN+8", "g256", 0, "real", 2561, 2560, 128, ldc=2568, res=True, also="ldc+8"),
            C("g256-x-2561x2560x128-ldcN+4", "g256", 0, "exact", 2561, 2560, 128, ldc=2564, res=True, also="ldc+4"),
            C("g256-r-2560x2560x128-ldcN+4", "g256", 0, "real", 2560, 2560, 128, ldc=2564, act=2, also="ldc+4"),
            C("g256-r-2561x2560x128-ldr", "g256", 0, "real", 2561, 2560, 128, res=True, ldr=2576, also="ldr"),
            C("g256-x-2560x2312x128-ldr32", "g256", 0, "exact", 2560, 2312, 128, out=32, res=True, ldr=2316, ldc=2320, also="ldr"),
            C("g256-r-2560x2560x128-ldw", "g256", 0, "real", 2560, 2560, 128, ldw=136, also="ldw"),
            # more tiles than blocks: the only shapes on which a block has a NEXT tile, i.e. the fast epilogue and the counted tile-start wait run
            C("g256-r-7168x2560x128-fast", "g256", 0, "real", 7168, 2560, 128, also="fast"),
            C("g256-x-7168x2560x192-fast", "g256", 0, "exact", 7168, 2560, 192, also="fast"),
            C("g256-r-7169x2560x128-next-res", "g256", 0, "real", 7169, 2560, 128, res=True, also="next")]
    return out


def cases_g256_batch():
    C = _c
    kw = dict(api="batched", S=25, bias=False)
    return [C("b256-x-25x300x260x64-o32-w1", "g256_batch", -1, "exact", 300, 260, 64, out=32, w_mod=1, **kw),
            C("b256-r-25x300x260x192-o16-w25", "g256_batch", -1, "real", 300, 260, 192, out=16, w_mod=25, **kw),
            C("b256-x-25x300x260x192-o16-w1", "g256_batch", -1, "exact", 300, 260, 192, out=16, w_mod=1, **kw),
            C("b256-r-25x300x260x64-o32-w25", "g256_batch", -1, "real", 300, 260, 64, out=32, w_mod=25, **kw)]


def cases_batched128():
    C, out = _c, []
    for S, w_mod, o, kind, N in ((1, 1, 16, "real", 64), (3, 1, 32, "exact", 64), (3, 2, 16, "real", 132), (3, 2, 32, "real", 64), (1, 1, 32, "exact", 132),
                                 (3, 2, 16, "exact", 64)):
        out.append(C(f"b128-{kind[0]}-{S}x70x{N}x128-o{o}-w{w_mod}", "bf128_batched", -1, kind, 70, N, 128, api="batched", S=S, w_mod=w_mod, out=o))
    for inner, o, kind in ((1, 32, "exact"), (4, 16, "real"), (4, 32, "exact"), (1, 16, "real")):
        out.append(C(f"b2-{kind[0]}-3x{inner}x70x64x64-o{o}", "bf128_batched", -1, kind, 70, 64, 64, api="batched2", S=3, inner=inner, out=o, bias=False))
    return out


def cases_g8p():
    C, out, i = _c, [], 0
    ks = (128, 192, 320, 384, 448)
    keys = [(a, r, f, h) for h in (False, True) for f in (False, True) for r in (False, True) for a in (0, 1, 2)]      # every key of the switch in sc_gemm8p_try
    for mi, M in enumerate((256, 257, 511, 589)):
        for ni, N in enumerate((256, 512, 1280)):
            for rep in range(2):
                a, r, f, h = keys[i]
                K = ks[(mi + ni + 2 * rep) % 5]
                kind = "exact" if (a == 0 and not (r and not f) and i % 2 == 0) else "real"
                out.append(C(f"g8p-{kind[0]}-{M}x{N}x{K}-a{a}{'-r' if r else ''}-o{32 if f else 16}{'-h' if h else ''}", "g8p_pers", 16, kind, M, N, K, act=a, res=r,
                             out=32 if f else 16, f16=h))
                i += 1
    out += [C("g8p-x-589x1280x448-o16-b-r-twice", "g8p_pers", 16, "exact", 589, 1280, 448, res=True, also="twice"),
            C("g8p-r-8525x2048x384-switch-dyn", "g8p_pers", 16, "real", 8525, 2048, 384, res=True, also="switch"),
            C("g8p-r-8525x2048x384-switch-static", "g8p_pers", 26, "real", 8525, 2048, 384, res=True, also="switch"),
            C("g8p-x-8525x2048x384-switch-dyn", "g8p_pers", 16, "exact", 8525, 2048, 384, out=32, also="switch"),
            C("g8p-r-2125x4096x384-default-band", "g8p_pers", -1, "real", 2125, 4096, 384, also="band"),
            C("g8p-x-2125x4096x384-default-band", "g8p_pers", -1, "exact", 2125, 4096, 384, out=32, res=True, also="band"),
            C("g8p-r-589x512x192-lda128", "g8p_pers", 16, "real", 589, 512, 192, lda=128, also="lda<K"),
            C("g8p-x-589x512x192-lda128", "g8p_pers", 16, "exact", 589, 512, 192, lda=128, out=32, also="lda<K"),
            C("g8p-r-257x512x128-ldaK+8", "g8p_pers", 16, "real", 257, 512, 128, lda=136, res=True, also="lda>K"),
            C("g8p-r-511x512x128-ldcN+8", "g8p_pers", 16, "real", 511, 512, 128, ldc=520, res=True, ldr=528, also="ldc+8"),
            C("g8p-x-511x512x128-ldcN+8", "g8p_pers", 16, "exact", 511, 512, 128, ldc=520, also="ldc+8"),
            C("g8p-r-589x512x128-ldw", "g8p_pers", 16, "real", 589, 512, 128, ldw=136, also="ldw"),
            C("g8p-r-4096x256x128-h-stats", "g8p_pers", 16, "real", 4096, 256, 128, f16=True, res=True, also="stats")]
    return out


CASE_LISTS = collections.OrderedDict((("bf128x64", cases_bf128x64), ("bf128x128", cases_bf128x128), ("f16", cases_f16), ("g256", cases_g256),
                                      ("g256_batch", cases_g256_batch), ("batched128", cases_batched128), ("g8p", cases_g8p)))


def all_cases():
    return [c for f in CASE_LISTS.values() for c in f()]


def shrunk_cases():
    """One case per path of the 256-row kernels at a size the CPU self-check can emulate: the SAME fields feed the reference, the rounding model and the bound; only
    the dispatcher would not send such a shape there (tools/gemm_bounds.py does not ask it to)."""
    C = _c
    return [C("s-g256-x-513x264x448-twice", "g256", 0, "exact", 513, 264, 448, res=True, ldr=272), C("s-g256-x-300x260x448-once", "g256", 0, "exact", 300, 260, 448, res=True, ldr=264),
            C("s-g256-r-513x264x192-twice", "g256", 0, "real", 513, 264, 192, res=True, ldr=272), C("s-g256-r-300x260x128-scalar", "g256", 0, "real", 300, 260, 128, res=True, act=1),
            C("s-g256-r-300x264x128-gelu32", "g256", 0, "real", 300, 264, 128, out=32, act=1, res=True), C("s-g256-r-300x264x128-qgelu", "g256", 0, "real", 300, 264, 128, act=2, res=True),
            C("s-g256-x-300x264x192-kpair", "g256", 0, "exact", 300, 264, 192, lda=128, out=32), C("s-g256-r-300x264x128-plain", "g256", 0, "real", 300, 264, 128, bias=False),
            C("s-b256-r-3x300x260x64", "g256_batch", -1, "real", 300, 260, 64, api="batched", S=3, w_mod=3, bias=False),
            C("s-b256-x-3x300x260x64", "g256_batch", -1, "exact", 300, 260, 64, api="batched", S=3, w_mod=1, bias=False, out=32),
            C("s-g8p-x-300x256x448-twice", "g8p_pers", 16, "exact", 300, 256, 448, res=True), C("s-g8p-r-300x256x128-twice", "g8p_pers", 16, "real", 300, 256, 128, res=True),
            C("s-g8p-r-300x256x128-gelu-h", "g8p_pers", 16, "real", 300, 256, 128, act=1, f16=True), C("s-g8p-r-300x256x128-qgelu32", "g8p_pers", 16, "real", 300, 256, 128, act=2, out=32, res=True)]


# ================================================================================================ layout and inputs
def layout(c):
    """strides (elements) of the operands of a batched call; every one keeps 16-byte alignment; C leaves a gap of sentinels between products"""
    Z = nprod(c)
    L = dict(Z=Z)
    if c.api == "gemm":
        L.update(strideA=0, strideW=0, strideC=0, nw=1)
    elif c.api == "batched":
        L.update(strideA=c.M * c.lda + 64, strideW=c.N * c.ldw + 64, strideC=c.M * c.ldc + 128, nw=c.w_mod)
    else:   # batched2: A [outer][M][inner K], W [outer][inner][N][K], C [outer][M][inner N (+ padding)]: the heads of one packed row side by side
        L.update(strideA=c.M * c.lda + 64, strideA2=c.K, strideW2=c.N * c.ldw + 8, strideC=c.M * c.ldc, strideC2=c.N, nw=Z)
        L["strideW"] = c.inner * L["strideW2"] + 64
    return L


def w_index(c, z):
    return z % c.w_mod if c.api == "batched" else (z if c.api == "batched2" else 0)


def inputs(c):
    """-> dict of fp64 tensors: A [Z, M, K] (lda < K: rows of one flat vector `Aflat`, A[m, k] = Aflat[m lda + k]), W [nw, N, K], bias [nw, N] or None, res [M, N] or None"""
    g = gen("gemm", c.id)
    Z, nw = nprod(c), layout(c)["nw"]
    odt, rdt = op_dt(c), out_dt(c)
    inp = {}
    if c.kind == "exact":
        assert c.act == 0
        lo = 0 if c.out == 16 else -3
        draw = lambda *s: torch.randint(lo, 4, s, generator=g).to(F64)      # noqa: E731
        scale_w = 1.0
    else:
        draw = lambda *s: 0.5 * torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
        scale_w = 2.0 * c.K ** -0.5
    if c.lda < c.K:
        assert c.api == "gemm"
        flat = rnd(draw((c.M - 1) * c.lda + c.K), odt)
        inp["Aflat"] = flat
        inp["A"] = torch.as_strided(flat, (c.M, c.K), (c.lda, 1)).clone().unsqueeze(0)
    else:
        inp["A"] = rnd(draw(Z, c.M, c.K), odt)
    inp["W"] = rnd(draw(nw, c.N, c.K) * scale_w, odt)
    if c.kind == "exact":
        inp["bias"] = torch.randint(-12 if c.out == 16 else -16, 17, (nw, c.N), generator=g).to(F64) if c.bias else None
        inp["res"] = torch.randint(-64, 65, (c.M, c.N), generator=g).to(F64) if c.res else None
    else:
        inp["bias"] = rnd(torch.randn(nw, c.N, generator=g, dtype=F64), F32) if c.bias else None
        inp["res"] = rnd(torch.randn(c.M, c.N, generator=g, dtype=F64), rdt) if c.res else None
    return inp


# ================================================================================================ the statement, its mutants, the rounding model
MUTANTS = ("drop_k", "drop_last_chunk", "chunk_twice", "clamp_off_by_one", "overlap_wrong_tile", "bias_shift4", "bias_product0", "res_ldc", "res_skip_ragged",
           "act_after_res", "store_trunc", "once_for_twice", "twice_for_once", "stridec2_for_stridec", "col_past_n", "w_not_transposed")


def act64(y, act):
    return gelu64(y) if act == 1 else (y * torch.sigmoid(1.702 * y) if act == 2 else y)


def q(t, dt, trunc=False):
    """fp64 values stored to dt (fp32 first: the kernels hold fp32) and read back; trunc: toward zero, the store a mutant makes"""
    if dt == F32:
        return t.to(F32).to(F64)
    if not trunc:
        return t.to(F32).to(dt).to(F64)
    r = t.to(F32).to(dt).to(F64)
    bits = r.to(dt).view(torch.int16)
    over = r.abs() > t.abs()
    return torch.where(over, (bits - 1).view(dt).to(F64), r)      # sign-magnitude: one step toward zero


def ref(c, inp, mutant=None):
    """-> dict(pre [Z, M, N] = A W^T, mag = |A| |W|^T, u = pre + bias, val = act(u), out = val + residual, got = `out` after the stores of rounding_points(c)), all fp64.
    With a mutant: the statement of that wrong kernel, or None where it cannot apply to the case."""
    A, W, bias, res = inp["A"], inp["W"], inp["bias"], inp["res"]
    Z, M, N, K = nprod(c), c.M, c.N, c.K
    wz = torch.tensor([w_index(c, z) for z in range(Z)])
    model, dt = rounding_points(c), out_dt(c)
    if mutant == "drop_k":
        A = A.clone(); A[..., 5] = 0
    elif mutant == "drop_last_chunk":
        A = A.clone(); A[..., K - 64:] = 0
    elif mutant == "chunk_twice":              # the first chunk of the walk read again in place of its partner (the last chunk)
        if K < 128:
            return None
        A, W = A.clone(), W.clone()
        A[..., K - 64:], W[..., K - 64:] = A[..., :64], W[..., :64]
    elif mutant == "clamp_off_by_one":
        if M < 2:
            return None
        A = A.clone(); A[:, M - 2] = A[:, M - 1]
    elif mutant == "w_not_transposed":
        if N != K:
            return None
        W = W.transpose(-1, -2)
    elif mutant in ("once_for_twice", "twice_for_once"):
        if dt == F32 or not c.res or model != ("twice" if mutant == "once_for_twice" else "once"):
            return None
        model = "once" if mutant == "once_for_twice" else "twice"
    elif mutant == "store_trunc" and dt == F32:
        return None
    Ww = W[wz]
    pre = torch.matmul(A, Ww.transpose(-1, -2))
    r = dict(pre=pre)
    if mutant is None:
        r["mag"] = torch.matmul(A.abs(), Ww.abs().transpose(-1, -2))
    b = torch.zeros(Z, 1, N, dtype=F64) if bias is None else bias[wz].unsqueeze(1)
    if mutant == "bias_shift4":
        if bias is None:
            return None
        b = torch.roll(b, 4, -1)
    elif mutant == "bias_product0":
        if bias is None or c.w_mod < 2:
            return None
        b = bias[0].reshape(1, 1, N).expand(Z, 1, N)
    u = pre + b
    rr = torch.zeros(M, N, dtype=F64) if res is None else res
    if mutant == "res_ldc":
        if res is None or c.ldr == c.ldc:
            return None
        flat = torch.zeros(M * max(c.ldr, c.ldc) + N, dtype=F64)
        flat[:M * c.ldr].view(M, c.ldr)[:, :N] = res
        rr = torch.as_strided(flat, (M, N), (c.ldc, 1)).clone()
    elif mutant == "res_skip_ragged":
        bn = 64 if c.path in ("bf128x64", "h128x64") else (128 if c.path in ROWS128 else 256)
        if res is None or N % bn == 0 or N < bn:
            return None
        rr = rr.clone(); rr[:, N // bn * bn:] = 0
    if mutant == "act_after_res":
        if res is None or c.act == 0:
            return None
        val, out = act64(u + rr, c.act), None
    else:
        val = act64(u, c.act)
        out = val + rr
    r.update(u=u, val=val, b=b)
    if dt == F32 or model == "once" or out is None:
        out = val if out is None else out
        got = q(out, dt, trunc=mutant == "store_trunc")
    else:
        got = q(q(val, dt) + rr, dt, trunc=mutant == "store_trunc")
    if mutant == "overlap_wrong_tile":      # the shifted-back last tile stores its overlap rows with the unshifted row index: what belongs to tile 0
        lo = M // 256 * 256
        if M <= 256 or M == lo or c.path in ROWS128:
            return None
        got = got.clone(); got[:, M - 256:lo] = got[:, 0:lo - (M - 256)].clone()
    elif mutant == "col_past_n":             # every store one column to the right: column 0 keeps the sentinel, column N lands in the padding / the next row
        got = torch.cat([torch.full_like(got[..., :1], SENT32 if dt == F32 else SENT16), got[..., :-1]], -1)
    elif mutant == "stridec2_for_stridec":
        if c.api != "batched2" or c.inner < 2:
            return None
        L = layout(c)
        flat = torch.full((Z * L["strideC"] + c.M * c.ldc,), SENT32 if dt == F32 else SENT16, dtype=F64)
        for z in range(Z):
            zo, zi = divmod(z, c.inner)
            torch.as_strided(flat, (M, N), (c.ldc, 1), zo * L["strideC2"] + zi * L["strideC"]).copy_(got[z])
        got = torch.stack([torch.as_strided(flat, (M, N), (c.ldc, 1), (z // c.inner) * L["strideC"] + (z % c.inner) * L["strideC2"]).clone() for z in range(Z)])
    r.update(out=out, got=got, res=rr)
    return r


def bound(c, inp, r):
    """-> (bound, store): fp64 [Z, M, N]; `store` is the part the attained roundings of the 16-bit stores take (0 for fp32 outputs and for the packed-half GELU
    form, whose constant holds its store)."""
    dt, model = out_dt(c), rounding_points(c)
    u, val, out = r["u"], r["val"], r["out"]
    e = c.K * U_ACC * r["mag"]
    if c.bias:
        e = e + U * u.abs()
        if c.path == "g8p_pers":
            e = e + (c.K // 32) * U_ACC * r["b"].abs()
    store = torch.zeros_like(out)
    form_holds_store = False
    if c.act == 1:
        form = gelu_form(c)
        e = GELU_LIP * e
        if form == "erf_fit":
            e = e + GELU_ERF_FIT + (2 * TR + 8 * U) * val.abs()
        elif form == "erf_precise":
            e = e + GELU_PRECISE * (1 + u.abs())
        elif form == "poly2_f32":
            e = e + GELU_POLY2_F32 + torch.where(u.abs() > GELU_POLY2_F32_CLAMP, GELU_POLY2_F32_TAIL * u.abs(), torch.zeros_like(u))
        else:
            e = e + GELU_POLY2_ABS + GELU_POLY2_REL * val.abs()
            form_holds_store = True
    elif c.act == 2:
        e = GELU_LIP * e + (2 * TR + 2 * U + 1.702 * u.abs() * U_ACC) * val.abs()
    if c.res:
        if dt != F32 and model == "twice" and not form_holds_store:
            store = store + store_bound(val, dt)
        e = e + U * out.abs()
    if dt != F32 and not (form_holds_store and not c.res):
        store = store + store_bound(out, dt)
    return e + store, store


def expected_bits(c, r):
    """the exact case's expected output in the output type"""
    return r["got"].to(F32).to(out_dt(c))


def model_bits(c, r, model):
    """the 16-bit output of a case with a residual under the given rounding model ("once" / "twice"), from the parts of ref(): no second product"""
    dt = out_dt(c)
    v = q(r["out"], dt) if model == "once" else q(q(r["val"], dt) + r["res"], dt)
    return v.to(F32).to(dt)


def stats(got, ref_, bd):
    """-> (n, |mean r|, |mean sign(ref) r|, 6 / sqrt(n)) over the elements with a positive bound"""
    ok = bd > 0
    rr = ((got - ref_) / bd.clamp_min(1e-300))[ok]
    n = int(rr.numel())
    return n, abs(float(rr.mean())), abs(float((torch.sign(ref_[ok]) * rr).mean())), 6.0 / max(n, 1) ** 0.5


def wants_stats(c):
    return c.kind == "real" and c.act == 0 and nprod(c) * c.M * c.N >= 4096


# ================================================================================================ fp32 emulation (CPU self-check)
def emulate(c, inp, order):
    """torch fp32 emulation of the path: the K sum "seq" (one addition per k, left to right) or "rot32" (32-deep dot products formed exactly and added to the
    accumulator one at a time, the walk started at chunk 1 and wrapped: the K rotation), accumulators started from the bias where the kernel does; bias, activation
    (the exact erf / sigmoid forms in fp32: the forms' own errors are constants of the bound) and residual in fp32; stores at the rounding points.  -> fp64 [Z, M, N]"""
    A, W, bias, res = inp["A"], inp["W"], inp["bias"], inp["res"]
    Z, K = nprod(c), c.K
    wz = torch.tensor([w_index(c, z) for z in range(Z)])
    Ww = W[wz]
    dt, model = out_dt(c), rounding_points(c)
    b32 = None if bias is None else bias[wz].unsqueeze(1).to(F32)
    init = c.path == "g8p_pers" and b32 is not None
    acc = torch.zeros(Z, c.M, c.N, dtype=F32) + (b32 if init else 0)
    if order == "seq":
        a32, w32 = A.to(F32), Ww.to(F32)
        for k in range(K):
            acc = acc + a32[:, :, k:k + 1] * w32[:, :, k].unsqueeze(1)
    else:
        nch = K // 32
        for j in range(nch):
            k0 = ((j + 2) % nch) * 32
            part = torch.matmul(A[:, :, k0:k0 + 32], Ww[:, :, k0:k0 + 32].transpose(-1, -2))
            acc = (acc.to(F64) + part).to(F32)
    if b32 is not None and not init:
        acc = acc + b32
    if c.act == 1:
        acc = torch.nn.functional.gelu(acc)
    elif c.act == 2:
        acc = acc * torch.sigmoid(torch.tensor(1.702, dtype=F32) * acc)
    if res is None:
        return acc.to(dt).to(F64)
    r32 = res.to(F32)
    if dt != F32 and model == "twice":
        return (acc.to(dt).to(F32) + r32).to(dt).to(F64)
    return (acc + r32).to(dt).to(F64)
