// Backward of the HuBERT FRONT END for `audio_encoder.trainable: true` without layer lists (avssl/module/speech_encoder_plus.py:399-401: nothing
// is frozen, so the conv feature extractor, post_extract_proj, layer_norm and the positional conv train too; [3P fairseq] scales the feature
// extractor's gradient by feature_grad_mult).  The GEMM-shaped parts run on sc_gemm_bf16 / sc_gemm_bf16_batched / sc_posconv_conv from Python
// (speechclip_amd/train_front.py); this file holds what they cannot do:
//   sc_posconv_finish_train   training forward of the positional-conv tail: u = conv + bias (regrouped to [B*Tp, D]) and s = mask(x) + gelu(u),
//                             both kept for the backward (the eval kernel fuses them with the LayerNorm and keeps neither)
//   sc_posconv_dgrad_finish   dx = mask(ds + time-reversed regroup of the transposed conv): the input gradient of the grouped conv is the SAME
//                             "pad Kw/2, drop the last output" conv applied to the time-reversed gradient with in/out channels swapped
//   sc_reverse_rows_bf16      out[b, t, :] = in[b, T-1-t, :]
//   sc_conv0_bwd              conv layer 0 (Conv1d(1 -> C, k=10, s=5, no bias) -> GroupNorm(C groups) over time -> GELU) backward from the wave:
//                             per-(b, c) partial gradients of the conv weight [10], gamma and beta (summed over b by sc_colsum)
// Packed (padding-free) batches -- utterance b owns rows [row_off[b], row_off[b + 1]) at transformer level and row_scale times that range at conv
// layer 0 (module/hubert.py: packed_geometry) -- run on the SAME kernels: the padded layout is the packed one with row_off[b] = b * Tp and rows_b = Tp, so
// every operation is one kernel and one host _impl, and its two entries (uniform / *_packed, which takes row_off) are thin forwards into it.  Every
// GEMM-shaped part is row-wise and runs as it is.
//   sc_conv0_bwd_packed / sc_conv0_wgrad_packed   dy / du read at rows row_scale * row_off[b] + t, zero for frames the layout does not materialise
//                             (the GroupNorm sums still run over all T0 frames of the padded length); uniform: rows b * P + t, all T0 frames
//   sc_posconv_finish_train_packed / sc_posconv_dgrad_finish_packed / sc_reverse_rows_packed_bf16   over sc_posconv_conv_packed's slab layout
//                             ([G][rows_b][cg] at element row_off[b] * D, = [B, G, Tp, cg] on uniform rows), time reversed inside each utterance's own rows
//   sc_posconv_pack_gapped    (packed only) the window slab of the weight gradient with Kw zero rows between utterances, so that dW stays ONE [rows, cols] product
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

__device__ __forceinline__ float gelu_grad(float x) {
    return 0.5f * (1.0f + fast_erf(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// ------------------------------------------------------------------------------------------------ row-streaming kernels, padded and packed rows
// One kernel per operation.  A thread owns V adjacent channels of one row (V = 8: one 16-byte load / store per tensor, when the group width D/G is a
// multiple of 8; else V = 4; either way the V channels lie in one group).  The row's utterance b, its first row r0 and its row count rows_b come from
// row_off by binary search on packed rows and from b = row / Tp, r0 = b * Tp, rows_b = Tp on uniform rows (the packed layout with row_off[b] = b * Tp);
// everything after that is one body.  The conv slab of utterance b is [G][rows_b][cg] at element r0 * D, which is [B, G, Tp, cg] on uniform rows.
__device__ __forceinline__ int pk_find(const int32_t* __restrict__ off, int B, int64_t row) {
    int lo = 0, hi = B;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)off[mid] <= row) lo = mid; else hi = mid; }
    return lo;
}
template <bool PACKED>
__device__ __forceinline__ int row_owner(const int32_t* __restrict__ off, int B, int Tp, int64_t row, int64_t& r0, int& rows_b) {
    if (PACKED) { const int b = pk_find(off, B, row); r0 = off[b]; rows_b = off[b + 1] - off[b]; return b; }
    const int b = (int)(row / Tp);
    r0 = (int64_t)b * Tp; rows_b = Tp;
    return b;
}
template <int V> struct alignas(2 * V) bfv { uint32_t w[V / 2]; };      // V bf16 values: uint2 / uint4
template <int V> __device__ __forceinline__ bfv<V> ld_bfv(const bf16_t* p) { return *(const bfv<V>*)p; }
template <int V> __device__ __forceinline__ void unpack_bfv(const bfv<V> v, float (&f)[V]) {
#pragma unroll
    for (int i = 0; i < V / 2; ++i) { f[2 * i] = lo2f(v.w[i]); f[2 * i + 1] = hi2f(v.w[i]); }
}
template <int V> __device__ __forceinline__ bfv<V> pack_bfv(const float (&f)[V]) {
    bfv<V> v;
#pragma unroll
    for (int i = 0; i < V / 2; ++i) v.w[i] = pack2bf(f[2 * i], f[2 * i + 1]);
    return v;
}

// u[row, e] = conv[b][g][t][ci] + bias[e];  s[row, e] = (t < valid[b] ? x[row, e] : 0) + gelu(u)
template <int V, bool PACKED>
__global__ __launch_bounds__(256) void posconv_finish_train_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ valid, const bf16_t* __restrict__ conv,
                                                                   const float* __restrict__ bias, bf16_t* __restrict__ u, bf16_t* __restrict__ s,
                                                                   const int32_t* __restrict__ row_off, int B, int Tp, int64_t rows, int D, int G) {
    const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (idx >= rows * D) return;
    const int64_t row = idx / D;
    const int e = (int)(idx - row * D);
    int64_t r0;
    int rows_b;
    const int b = row_owner<PACKED>(row_off, B, Tp, row, r0, rows_b);
    const int t = (int)(row - r0);
    const int cg = D / G, g = e / cg, ci = e - g * cg;
    float cv[V], xv[V], uv[V], ur[V], sv[V];
    unpack_bfv<V>(ld_bfv<V>(conv + (r0 * G + (int64_t)g * rows_b + t) * cg + ci), cv);
    bfv<V> xx = {};
    if (t < valid[b]) xx = ld_bfv<V>(x + idx);
    unpack_bfv<V>(xx, xv);
#pragma unroll
    for (int i = 0; i < V; i += 4) {
        const f32x4_t bv = *(const f32x4_t*)(bias + e + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) uv[i + j] = cv[i + j] + bv[j];
    }
    const bfv<V> uo = pack_bfv<V>(uv);
    unpack_bfv<V>(uo, ur);              // gelu of the bf16-ROUNDED pre-activation: the backward differentiates gelu at exactly the value it is handed
#pragma unroll
    for (int i = 0; i < V; ++i) sv[i] = xv[i] + gelu_erf_precise(ur[i]);
    *(bfv<V>*)(u + idx) = uo;
    *(bfv<V>*)(s + idx) = pack_bfv<V>(sv);
}

// dx[row, e] = t < valid[b] ? ds[row, e] + convT[b][g][rows_b - 1 - t][ci] : 0  (convT: the grouped conv of the time-reversed du)
template <int V, bool PACKED>
__global__ __launch_bounds__(256) void posconv_dgrad_finish_kernel(const bf16_t* __restrict__ convT, const bf16_t* __restrict__ ds, const int32_t* __restrict__ valid,
                                                                   bf16_t* __restrict__ dx, const int32_t* __restrict__ row_off, int B, int Tp, int64_t rows,
                                                                   int D, int G) {
    const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (idx >= rows * D) return;
    const int64_t row = idx / D;
    const int e = (int)(idx - row * D);
    int64_t r0;
    int rows_b;
    const int b = row_owner<PACKED>(row_off, B, Tp, row, r0, rows_b);
    const int t = (int)(row - r0);
    bfv<V> o = {};
    if (t < valid[b]) {
        const int cg = D / G, g = e / cg, ci = e - g * cg;
        float cv[V], dv[V], ov[V];
        unpack_bfv<V>(ld_bfv<V>(convT + (r0 * G + (int64_t)g * rows_b + (rows_b - 1 - t)) * cg + ci), cv);
        unpack_bfv<V>(ld_bfv<V>(ds + idx), dv);
#pragma unroll
        for (int i = 0; i < V; ++i) ov[i] = cv[i] + dv[i];
        o = pack_bfv<V>(ov);
    }
    *(bfv<V>*)(dx + idx) = o;
}

// out[r0 + rows_b - 1 - t, :] = in[r0 + t, :]: time reversal inside every utterance's own rows
template <int V, bool PACKED>
__global__ __launch_bounds__(256) void reverse_rows_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, const int32_t* __restrict__ row_off, int B,
                                                           int Tp, int64_t rows, int D) {
    const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (idx >= rows * D) return;
    const int64_t row = idx / D;
    const int e = (int)(idx - row * D);
    int64_t r0;
    int rows_b;
    row_owner<PACKED>(row_off, B, Tp, row, r0, rows_b);
    const int t = (int)(row - r0);
    *(bfv<V>*)(out + (r0 + (rows_b - 1 - t)) * D + e) = ld_bfv<V>(in + idx);
}

// conv layer 0 backward.  Block = (b, 64 channels); lane = channel, the 4 waves split the frames.  Three sweeps over the T0 frames, the conv
// recomputed from the wave each time (10 FMAs): (A) mean / variance of u over time, (B) S1 = sum dzhat, S2 = sum dzhat uhat, dgamma, dbeta,
// (C) du = rstd (dzhat - S1/T - uhat S2/T) and dw[j] += du wav[5 t + j].  dy rows >= T0 of an utterance do not exist in the reference (alignment
// padding of the channels-last buffer) and are not read.
// PACKED: utterance b's dy rows start at row_scale * row_off[b] and only row_scale * rows_b of them exist; later frames carry no gradient (dz = 0) but still
// take part in the two mean-subtraction terms of sweep (C): a frame the layout does not materialise can still see non-zero samples near the utterance's end.
constexpr int C0_K = 10, C0_S = 5;
template <bool PACKED>
__global__ __launch_bounds__(256) void conv0_bwd_kernel(const float* __restrict__ wav, int64_t ld, const float* __restrict__ w, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const bf16_t* __restrict__ dy, float* __restrict__ part, int C, int T0,
                                                        int P, float eps, const int32_t* __restrict__ row_off, int row_scale) {
    __shared__ float red[4][64][12];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the frame index below is wave-uniform,
    const int b = blockIdx.y, c = blockIdx.x * 64 + lane;                                            // so the ten wave samples of a frame are scalar loads
    const float* wv = wav + (int64_t)b * ld;
    float wk[C0_K];
#pragma unroll
    for (int j = 0; j < C0_K; ++j) wk[j] = w[c * C0_K + j];
    auto conv_at = [&](int t, float (&x)[C0_K]) -> float {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < C0_K; ++j) { x[j] = wv[t * C0_S + j]; a = fmaf(wk[j], x[j], a); }     // wave-uniform address: scalar loads
        return a;
    };
    auto block_sum = [&](float (&v)[12], int n) {      // sums v[0..n) over the 4 waves; result in every thread
        __syncthreads();
        for (int i = 0; i < n; ++i) red[wave][lane][i] = v[i];
        __syncthreads();
        for (int i = 0; i < n; ++i) v[i] = (red[0][lane][i] + red[1][lane][i]) + (red[2][lane][i] + red[3][lane][i]);
    };
    float x[C0_K];
    float acc[12];
    // (A) statistics in ONE sweep: sum and sum of squares in fp64 (the frames of a 10 s wave are ~3e4 terms; E[u^2] - E[u]^2 in fp32 would
    // lose the variance of a channel with a DC offset)
    double su = 0.0, sq = 0.0;
    for (int t = wave; t < T0; t += 4) { const double v = (double)conv_at(t, x); su += v; sq += v * v; }
    {
        __shared__ double dred[4][64][2];
        dred[wave][lane][0] = su; dred[wave][lane][1] = sq;
        __syncthreads();
        su = (dred[0][lane][0] + dred[1][lane][0]) + (dred[2][lane][0] + dred[3][lane][0]);
        sq = (dred[0][lane][1] + dred[1][lane][1]) + (dred[2][lane][1] + dred[3][lane][1]);
    }
    const double mean_d = su / (double)T0;
    const float mean = (float)mean_d;
    const float rstd = rsqrtf((float)(sq / (double)T0 - mean_d * mean_d) + eps);
    const float gm = gamma[c], bt = beta[c];
    const bf16_t* dyb = dy + (PACKED ? (int64_t)row_scale * row_off[b] : (int64_t)b * P) * C + c;
    const int tlim = PACKED ? min(T0, row_scale * (row_off[b + 1] - row_off[b])) : T0;      // frames with a gradient
    // (B)
    float s1 = 0.f, s2 = 0.f, dg = 0.f, db = 0.f;
    for (int t = wave; t < tlim; t += 4) {
        const float uh = (conv_at(t, x) - mean) * rstd;
        const float dz = bf2f(dyb[(int64_t)t * C]) * gelu_grad(fmaf(gm, uh, bt));
        dg = fmaf(dz, uh, dg);
        db += dz;
        const float dzh = dz * gm;
        s1 += dzh;
        s2 = fmaf(dzh, uh, s2);
    }
    acc[0] = s1; acc[1] = s2; acc[2] = dg; acc[3] = db;
    block_sum(acc, 4);
    const float m1 = acc[0] / (float)T0, m2 = acc[1] / (float)T0;
    dg = acc[2]; db = acc[3];
    // (C)
    float dw[C0_K];
#pragma unroll
    for (int j = 0; j < C0_K; ++j) dw[j] = 0.f;
    for (int t = wave; t < T0; t += 4) {
        const float uh = (conv_at(t, x) - mean) * rstd;
        const float dz = (!PACKED || t < tlim) ? bf2f(dyb[(int64_t)t * C]) * gelu_grad(fmaf(gm, uh, bt)) : 0.f;
        const float du = rstd * (dz * gm - m1 - uh * m2);
#pragma unroll
        for (int j = 0; j < C0_K; ++j) dw[j] = fmaf(du, x[j], dw[j]);
    }
#pragma unroll
    for (int j = 0; j < C0_K; ++j) acc[j] = dw[j];
    block_sum(acc, C0_K);
    if (wave == 0) {
        float* o = part + ((int64_t)b * C + c) * 12;
#pragma unroll
        for (int j = 0; j < C0_K; ++j) o[j] = acc[j];
        o[10] = dg;
        o[11] = db;
    }
}

// conv layer 0 of the LayerNorm extractor (HuBERT-large: Conv1d(1 -> C, k 10, s 5, bias) -> LayerNorm(C) -> GELU): the LayerNorm / GELU part of the
// backward runs on the row kernels, which leaves dw[c, j] = sum_t du[t, c] wav[5 t + j] and dbias[c] = sum_t du[t, c] per utterance.
template <bool PACKED>      // du rows of utterance b at row_scale * row_off[b] .., zero beyond the row_scale * rows_b the layout holds
__global__ __launch_bounds__(256) void conv0_wgrad_kernel(const float* __restrict__ wav, int64_t ld, const bf16_t* __restrict__ du, float* __restrict__ part,
                                                          int C, int T0, int P, const int32_t* __restrict__ row_off, int row_scale) {
    __shared__ float red[4][64][12];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
    const float* wv = wav + (int64_t)b * ld;
    const bf16_t* dub = du + (PACKED ? (int64_t)row_scale * row_off[b] : (int64_t)b * P) * C + c;
    const int tlim = PACKED ? min(T0, row_scale * (row_off[b + 1] - row_off[b])) : T0;
    float acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.f;
    for (int t = wave; t < tlim; t += 4) {
        const float g = bf2f(dub[(int64_t)t * C]);
#pragma unroll
        for (int j = 0; j < C0_K; ++j) acc[j] = fmaf(g, wv[t * C0_S + j], acc[j]);
        acc[10] += g;
    }
    for (int i = 0; i < 11; ++i) red[wave][lane][i] = acc[i];
    __syncthreads();
    if (wave == 0) {
        float* o = part + ((int64_t)b * C + c) * 12;
        for (int i = 0; i < 11; ++i) o[i] = (red[0][lane][i] + red[1][lane][i]) + (red[2][lane][i] + red[3][lane][i]);
        o[11] = 0.f;
    }
}

// out[g][lead + row_off[b] + b * gap + t][c] = t < min(lim[b], rows_b) ? x[row_off[b] + t][g * cg + c] : 0; every other row of the [G][slab_rows][cg] slab is zero.
// Utterance b starts at gapped row row_off[b] + b * gap: with gap = Kw zero rows between neighbours a window of Kw rows never sees two utterances.
__global__ __launch_bounds__(256) void posconv_pack_gapped_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lim, const int32_t* __restrict__ row_off,
                                                                  bf16_t* __restrict__ out, int B, int D, int G, int gap, int lead, int64_t slab_rows) {
    const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (idx >= slab_rows * D) return;
    const int64_t r = idx / D;
    const int e = (int)(idx - r * D);
    const int cg = D / G, g = e / cg, ci = e - g * cg;
    const int64_t p = r - lead;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p >= 0) {
        int lo = 0, hi = B;          // the last utterance whose gapped start is <= p
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)row_off[mid] + (int64_t)mid * gap <= p) lo = mid; else hi = mid; }
        const int r0 = row_off[lo], rows_b = row_off[lo + 1] - r0;
        const int64_t t = p - r0 - (int64_t)lo * gap;
        if (t < rows_b && t < lim[lo]) v = *(const uint4*)(x + ((int64_t)r0 + t) * D + e);
    }
    *(uint4*)(out + ((int64_t)g * slab_rows + r) * cg + ci) = v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entries
// Every operation has one _impl; its uniform and its packed entry forward into it (row_off == nullptr: uniform rows).  row_off: B + 1 device ints in
// transformer rows (row_off[B] = total_rows); the callers' buffers hold row_scale * total_rows rows at conv layer 0.
static int conv0_bwd_impl(const char* name, const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, const void* dy, float* part, int B,
                          int C, int T0, int P, float eps, void* stream, const int32_t* row_off, int row_scale) {
    SC_CHECK_ARG(wav && w && gamma && beta && dy && part, "%s: null operand", name);
    SC_CHECK_ARG(C % 64 == 0 && B <= 65535, "%s: C must be a multiple of 64, B <= 65535", name);
    SC_CHECK_ARG(T0 >= 1 && (row_off ? row_scale >= 1 : P >= T0) && ld >= (int64_t)(T0 - 1) * C0_S + C0_K, "%s: T0=%d P=%d row_scale=%d ld=%lld inconsistent", name,
                 T0, P, row_scale, (long long)ld);
    if (B <= 0) return 0;
#define C0_LAUNCH(PK_) hipLaunchKernelGGL(conv0_bwd_kernel<PK_>, dim3(C / 64, B), dim3(256), 0, (hipStream_t)stream, wav, ld, w, gamma, beta, (const bf16_t*)dy, part, C, T0, P, eps, row_off, row_scale)
    if (row_off) C0_LAUNCH(true); else C0_LAUNCH(false);
#undef C0_LAUNCH
    SC_CHECK_LAUNCH();
    return 0;
}

static int conv0_wgrad_impl(const char* name, const float* wav, int64_t ld, const void* du, float* part, int B, int C, int T0, int P, void* stream,
                            const int32_t* row_off, int row_scale) {
    SC_CHECK_ARG(wav && du && part, "%s: null operand", name);
    SC_CHECK_ARG(C % 64 == 0 && B <= 65535, "%s: C must be a multiple of 64, B <= 65535", name);
    SC_CHECK_ARG(T0 >= 1 && (row_off ? row_scale >= 1 : P >= T0) && ld >= (int64_t)(T0 - 1) * C0_S + C0_K, "%s: T0=%d P=%d row_scale=%d ld=%lld inconsistent", name,
                 T0, P, row_scale, (long long)ld);
    if (B <= 0) return 0;
#define C0_LAUNCH(PK_) hipLaunchKernelGGL(conv0_wgrad_kernel<PK_>, dim3(C / 64, B), dim3(256), 0, (hipStream_t)stream, wav, ld, (const bf16_t*)du, part, C, T0, P, row_off, row_scale)
    if (row_off) C0_LAUNCH(true); else C0_LAUNCH(false);
#undef C0_LAUNCH
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_conv0_bwd(const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, const void* dy, float* part, int B, int C, int T0,
                            int P, float eps, void* stream) {
    return conv0_bwd_impl("sc_conv0_bwd", wav, ld, w, gamma, beta, dy, part, B, C, T0, P, eps, stream, nullptr, 0);
}

extern "C" int sc_conv0_bwd_packed(const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, const void* dy, float* part, int B, int C,
                                   int T0, const int32_t* row_off, int row_scale, float eps, void* stream) {
    SC_CHECK_ARG(row_off, "sc_conv0_bwd_packed: null operand");
    return conv0_bwd_impl("sc_conv0_bwd_packed", wav, ld, w, gamma, beta, dy, part, B, C, T0, 0, eps, stream, row_off, row_scale);
}

extern "C" int sc_conv0_wgrad(const float* wav, int64_t ld, const void* du, float* part, int B, int C, int T0, int P, void* stream) {
    return conv0_wgrad_impl("sc_conv0_wgrad", wav, ld, du, part, B, C, T0, P, stream, nullptr, 0);
}

extern "C" int sc_conv0_wgrad_packed(const float* wav, int64_t ld, const void* du, float* part, int B, int C, int T0, const int32_t* row_off, int row_scale,
                                     void* stream) {
    SC_CHECK_ARG(row_off, "sc_conv0_wgrad_packed: null operand");
    return conv0_wgrad_impl("sc_conv0_wgrad_packed", wav, ld, du, part, B, C, T0, 0, stream, row_off, row_scale);
}

#define SC_PACKED_ROWS_CHECK(name) \
    SC_CHECK_ARG(B > 0 && total_rows > 0 && total_rows * D < (int64_t)0x7fffffff * 8, "%s: B=%d total_rows=%lld out of range", name, B, (long long)total_rows)

// The row-streaming kernels' shared checks -> elements per thread (8 or 4), 0 when there is nothing to do, -1 on a bad argument.  The uniform entries accept a
// group width that is a multiple of 4 and any row count (none: no launch); the packed entries need a multiple of 8, B > 0 and total_rows > 0.
static int rows_vec(const char* name, int D, int G, const int32_t* row_off, int B, int64_t total_rows) {
    const int need = row_off ? 8 : 4;
    SC_CHECK_ARG(G > 0 && D % G == 0 && (D / G) % need == 0, "%s: D/G must be a multiple of %d", name, need);
    if (row_off) SC_PACKED_ROWS_CHECK(name);
    else if (total_rows <= 0 || D <= 0) return 0;
    return (D / G) % 8 == 0 ? 8 : 4;
}
#define ROWS_LAUNCH(kernel, v, ...)                                                                                                 \
    do {                                                                                                                            \
        const dim3 grid_((unsigned)((rows * D / (v) + 255) / 256));                                                                 \
        if (row_off) hipLaunchKernelGGL((kernel<8, true>), grid_, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                  \
        else if ((v) == 8) hipLaunchKernelGGL((kernel<8, false>), grid_, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<4, false>), grid_, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                         \
        SC_CHECK_LAUNCH();                                                                                                          \
    } while (0)

static int posconv_finish_train_impl(const char* name, const void* x, const int32_t* valid, const void* conv, const float* bias, void* u, void* s, int B, int Tp,
                                     int D, int G, void* stream, const int32_t* row_off, int64_t rows) {
    SC_CHECK_ARG(x && valid && conv && bias && u && s, "%s: null operand", name);
    const int v = rows_vec(name, D, G, row_off, B, rows);
    if (v <= 0) return v;
    ROWS_LAUNCH(posconv_finish_train_kernel, v, (const bf16_t*)x, valid, (const bf16_t*)conv, bias, (bf16_t*)u, (bf16_t*)s, row_off, B, Tp, rows, D, G);
    return 0;
}

static int posconv_dgrad_finish_impl(const char* name, const void* convT, const void* ds, const int32_t* valid, void* dx, int B, int Tp, int D, int G, void* stream,
                                     const int32_t* row_off, int64_t rows) {
    SC_CHECK_ARG(convT && ds && valid && dx, "%s: null operand", name);
    const int v = rows_vec(name, D, G, row_off, B, rows);
    if (v <= 0) return v;
    ROWS_LAUNCH(posconv_dgrad_finish_kernel, v, (const bf16_t*)convT, (const bf16_t*)ds, valid, (bf16_t*)dx, row_off, B, Tp, rows, D, G);
    return 0;
}

static int reverse_rows_impl(const char* name, const void* in, void* out, int B, int T, int D, void* stream, const int32_t* row_off, int64_t rows) {
    SC_CHECK_ARG(in && out && in != out, "%s: null operand or in-place", name);
    const int v = rows_vec(name, D, 1, row_off, B, rows);
    if (v <= 0) return v;
    ROWS_LAUNCH(reverse_rows_kernel, v, (const bf16_t*)in, (bf16_t*)out, row_off, B, T, rows, D);
    return 0;
}
#undef ROWS_LAUNCH

extern "C" int sc_posconv_finish_train(const void* x, const int32_t* valid, const void* conv, const float* bias, void* u, void* s, int B, int Tp, int D, int G,
                                       void* stream) {
    return posconv_finish_train_impl("sc_posconv_finish_train", x, valid, conv, bias, u, s, B, Tp, D, G, stream, nullptr, (int64_t)B * Tp);
}

extern "C" int sc_posconv_finish_train_packed(const void* x, const int32_t* valid, const int32_t* row_off, const void* conv, const float* bias, void* u, void* s,
                                              int B, int64_t total_rows, int D, int G, void* stream) {
    SC_CHECK_ARG(row_off, "sc_posconv_finish_train_packed: null operand");
    return posconv_finish_train_impl("sc_posconv_finish_train_packed", x, valid, conv, bias, u, s, B, 0, D, G, stream, row_off, total_rows);
}

extern "C" int sc_posconv_dgrad_finish(const void* convT, const void* ds, const int32_t* valid, void* dx, int B, int Tp, int D, int G, void* stream) {
    return posconv_dgrad_finish_impl("sc_posconv_dgrad_finish", convT, ds, valid, dx, B, Tp, D, G, stream, nullptr, (int64_t)B * Tp);
}

extern "C" int sc_posconv_dgrad_finish_packed(const void* convT, const void* ds, const int32_t* valid, const int32_t* row_off, void* dx, int B, int64_t total_rows,
                                              int D, int G, void* stream) {
    SC_CHECK_ARG(row_off, "sc_posconv_dgrad_finish_packed: null operand");
    return posconv_dgrad_finish_impl("sc_posconv_dgrad_finish_packed", convT, ds, valid, dx, B, 0, D, G, stream, row_off, total_rows);
}

extern "C" int sc_reverse_rows_bf16(const void* in, void* out, int B, int T, int D, void* stream) {
    return reverse_rows_impl("sc_reverse_rows_bf16", in, out, B, T, D, stream, nullptr, (int64_t)B * T);
}

extern "C" int sc_reverse_rows_packed_bf16(const void* in, const int32_t* row_off, void* out, int B, int64_t total_rows, int D, void* stream) {
    SC_CHECK_ARG(row_off, "sc_reverse_rows_packed_bf16: null operand");
    return reverse_rows_impl("sc_reverse_rows_packed_bf16", in, out, B, 0, D, stream, row_off, total_rows);
}

// out bf16 [G][slab_rows][D/G]: row lead + row_off[b] + b * gap + t of group g = row row_off[b] + t of x (columns of group g) for t < min(lim[b], rows_b), zeros
// everywhere else; every row of the slab is written.  slab_rows >= lead + row_off[B] + B * gap.  The weight gradient of the positional conv uses it twice:
// (x, lim = valid, G groups, lead = Kw / 2) is the sliding-window operand, (du, lim = rows, G = 1, lead = 0) the gradient in the same row numbering.
extern "C" int sc_posconv_pack_gapped(const void* x, const int32_t* lim, const int32_t* row_off, void* out, int B, int64_t total_rows, int D, int G, int gap,
                                      int lead, int64_t slab_rows, void* stream) {
    SC_CHECK_ARG(x && lim && row_off && out, "sc_posconv_pack_gapped: null operand");
    SC_CHECK_ARG(G > 0 && D % G == 0 && (D / G) % 8 == 0, "sc_posconv_pack_gapped: D/G must be a multiple of 8");
    SC_CHECK_ARG(gap >= 0 && lead >= 0 && slab_rows >= lead + total_rows + (int64_t)B * gap, "sc_posconv_pack_gapped: slab_rows=%lld too small", (long long)slab_rows);
    SC_PACKED_ROWS_CHECK("sc_posconv_pack_gapped");
    SC_CHECK_ARG(slab_rows * D < (int64_t)0x7fffffff * 8, "sc_posconv_pack_gapped: slab too large");
    const int64_t n8 = slab_rows * D / 8;
    hipLaunchKernelGGL(posconv_pack_gapped_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, lim, row_off,
                       (bf16_t*)out, B, D, G, gap, lead, slab_rows);
    SC_CHECK_LAUNCH();
    return 0;
}
