// SimpleVectorQuantizer, the modes beside the shipped one (my_vector_quantizer.py:124-139 in train mode): soft (hard: false), Gumbel hard and Gumbel soft.
//   y = softmax((x + g) / T) over the unmasked sub-words, x = cosine scores f32 [R, V], g = Gumbel(0, 1) noise or 0, T = temperature.
// The noise is a pure function of (seed, r * V + v) -- the dropout masks' hash (common.h) -- so the backward regenerates it instead of storing it:
//   h = hash32(seed ^ hash32(idx + 0x9e3779b9)), u = ((h >> 9) + 0.5) 2^-23 (exact in fp32, in [2^-24, 1 - 2^-24]), e = -log u (the Exponential(1) draw of
//   F.gumbel_softmax), g = -log e in [-2.82, 16.64]; both logarithms are the accurate logf (near u = 1, e ~ 6e-8: an absolute error of the fast log there
//   is an order-one relative error of e).
// sc_vq_soft_embed is the hot path: keywords = y @ emb without an [R, V] image of y.  It is a flash-attention forward with one "head", scores given
// instead of computed and the sub-words in the role of the keys: a pre-pass (one block per row) leaves row_max = max_v (x + g) and
// row_den = sum_v exp((x + g - row_max) / T); the main kernel forms P = exp(..) / row_den for a 128 x 32 tile, splits it into (hi, lo) bf16 in LDS, and
// accumulates P_hi E_hi + P_lo E_hi + P_hi E_lo on v_mfma_f32_16x16x32_bf16 against the table in MFMA-fragment order (sc_vq_soft_table).  V is split over
// `nsplit` chunks (grid.z); since P is already normalised the partial products simply add, in a fixed order (vq_soft_finish_kernel): no atomics, bitwise
// run-to-run.
#include "common.h"

namespace {

struct MaskIds { int n; int id[8]; };

__device__ __forceinline__ bool masked(int v, const MaskIds& m) {
    for (int i = 0; i < m.n; ++i)
        if (m.id[i] == v) return true;
    return false;
}

__device__ __forceinline__ float gumbel_noise(uint32_t seed, uint32_t idx) {
    const uint32_t h = hash32(seed ^ hash32(idx + 0x9e3779b9U));
    const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;        // 24 significant bits: exact
    return -logf(-logf(u));
}

__device__ __forceinline__ float block_sum(float v, float* s_red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
__device__ __forceinline__ float block_max(float v, float* s_red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

__global__ __launch_bounds__(256) void vq_gumbel_noise_kernel(float* __restrict__ out, int64_t n, uint32_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gumbel_noise(seed, (uint32_t)i);
}

// one block per row: arg-max of x + g over the unmasked sub-words, the lowest index on ties (torch.max)
template <bool NOISE>
__global__ __launch_bounds__(256) void vq_noisy_argmax_kernel(const float* __restrict__ x, int64_t* __restrict__ targets, int V, uint32_t seed, MaskIds mk) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* row = x + (int64_t)r * V;
    const uint32_t base = (uint32_t)r * (uint32_t)V;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = tid; v < V; v += 256) {
        if (masked(v, mk)) continue;
        float t = row[v];
        if (NOISE) t += gumbel_noise(seed, base + (uint32_t)v);
        if (t > best || (t == best && v < bi)) { best = t; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_val[wv] = best; s_idx[wv] = bi; }
    __syncthreads();
    if (tid == 0) {
        best = s_val[0]; bi = s_idx[0];
        for (int w = 1; w < 4; ++w)
            if (s_val[w] > best || (s_val[w] == best && s_idx[w] < bi)) { best = s_val[w]; bi = s_idx[w]; }
        targets[r] = bi == 0x7fffffff ? 0 : bi;
    }
}

// one block per row: row_max = max_v (x + g), row_den = sum_v exp((x + g - row_max) / T) over the unmasked sub-words
template <bool NOISE>
__device__ __forceinline__ void row_stats(const float* __restrict__ row, uint32_t base, int V, float inv_temp, uint32_t seed, const MaskIds& mk, float* s_red,
                                          float& mx, float& den) {
    const int tid = threadIdx.x;
    mx = -INFINITY;
    for (int v = tid; v < V; v += 256)
        if (!masked(v, mk)) mx = fmaxf(mx, NOISE ? row[v] + gumbel_noise(seed, base + (uint32_t)v) : row[v]);
    mx = block_max(mx, s_red);
    den = 0.f;
    for (int v = tid; v < V; v += 256)
        if (!masked(v, mk)) den += __expf(((NOISE ? row[v] + gumbel_noise(seed, base + (uint32_t)v) : row[v]) - mx) * inv_temp);
    den = block_sum(den, s_red);
}

template <bool NOISE>
__global__ __launch_bounds__(256) void vq_row_stats_kernel(const float* __restrict__ x, float* __restrict__ row_max, float* __restrict__ row_den, int V,
                                                           float inv_temp, uint32_t seed, MaskIds mk) {
    __shared__ float s_red[4];
    const int r = blockIdx.x;
    float mx, den;
    row_stats<NOISE>(x + (int64_t)r * V, (uint32_t)r * (uint32_t)V, V, inv_temp, seed, mk, s_red, mx, den);
    if (threadIdx.x == 0) { row_max[r] = mx; row_den[r] = den; }
}

// y = softmax((x + g) / T) as a dense image (the lazy `subword_prob`, and the product path of shapes sc_vq_soft_embed does not cover)
template <bool NOISE>
__global__ __launch_bounds__(256) void vq_probs_kernel(const float* __restrict__ x, float* __restrict__ out, int V, float inv_temp, uint32_t seed, MaskIds mk) {
    __shared__ float s_red[4];
    const int r = blockIdx.x;
    const float* row = x + (int64_t)r * V;
    float* o = out + (int64_t)r * V;
    const uint32_t base = (uint32_t)r * (uint32_t)V;
    float mx, den;
    row_stats<NOISE>(row, base, V, inv_temp, seed, mk, s_red, mx, den);
    for (int v = threadIdx.x; v < V; v += 256) {
        float p = 0.f;
        if (!masked(v, mk)) p = __expf(((NOISE ? row[v] + gumbel_noise(seed, base + (uint32_t)v) : row[v]) - mx) * inv_temp) / den;
        o[v] = p;
    }
}

// Backward through y = softmax((cos + g) / T): vq_st_bwd_kernel (train_cascaded.hip) with the noise regenerated.  Without noise the instruction sequence is
// that kernel's (tests/test_vq_modes_gpu.py compares the bits), and rowdot_z = rowdot_cos.
template <bool NOISE>
__global__ __launch_bounds__(256) void vq_mode_bwd_kernel(const float* __restrict__ cosv, float* __restrict__ dprob, float* __restrict__ rowdot,
                                                          float* __restrict__ rowdot_z, int V, float inv_temp, uint32_t seed, MaskIds mk) {
    __shared__ float s_red[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* c = cosv + (int64_t)r * V;
    float* g = dprob + (int64_t)r * V;
    const uint32_t base = (uint32_t)r * (uint32_t)V;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256)
        if (!masked(v, mk)) mx = fmaxf(mx, NOISE ? c[v] + gumbel_noise(seed, base + (uint32_t)v) : c[v]);
    mx = block_max(mx, s_red);
    float den = 0.f, num = 0.f;
    for (int v = tid; v < V; v += 256)
        if (!masked(v, mk)) { const float e = __expf(((NOISE ? c[v] + gumbel_noise(seed, base + (uint32_t)v) : c[v]) - mx) * inv_temp); den += e; num += e * g[v]; }
    den = block_sum(den, s_red);
    num = block_sum(num, s_red);
    const float dot = num / den;
    float rd = 0.f, rz = 0.f;
    for (int v = tid; v < V; v += 256) {
        float d = 0.f;
        if (!masked(v, mk)) {
            const float s = NOISE ? c[v] + gumbel_noise(seed, base + (uint32_t)v) : c[v];
            const float p = __expf((s - mx) * inv_temp) / den;
            d = p * (g[v] - dot) * inv_temp;
            rd += d * c[v];
            if (NOISE) rz += d * s;
        }
        g[v] = d;
    }
    rd = block_sum(rd, s_red);
    if (NOISE) rz = block_sum(rz, s_red);
    if (tid == 0) { rowdot[r] = rd; rowdot_z[r] = NOISE ? rz : rd; }
}

// The sub-word table in the B-operand order of v_mfma_f32_16x16x32_bf16: table[half][vb][et][lane][j] = half(emb[32 vb + 8 (lane >> 4) + j][16 et + (lane & 15)]),
// half 0 = bf16(emb), half 1 = bf16(emb - hi); rows beyond V are zero.  One wave reads a fragment as 1 KiB of consecutive bytes.
__global__ __launch_bounds__(256) void vq_soft_table_kernel(const float* __restrict__ emb, bf16_t* __restrict__ table, int V, int E, int64_t nvec, int64_t half_elems) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one 8-element vector (a lane's fragment) per thread
    if (i >= nvec) return;
    const int lane = (int)(i & 63), ET = E >> 4;
    const int64_t t = i >> 6;
    const int et = (int)(t % ET);
    const int64_t vb = t / ET;
    const int col = et * 16 + (lane & 15);
    bf16_t hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t v = vb * 32 + (lane >> 4) * 8 + j;
        const float x = v < V ? emb[v * E + col] : 0.f;
        hi[j] = f2bf(x);
        lo[j] = f2bf(x - bf2f(hi[j]));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { table[i * 8 + j] = hi[j]; table[half_elems + i * 8 + j] = lo[j]; }
}

constexpr int SE_BM = 128;       // rows per block (two wave rows of 64)
constexpr int SE_BK = 32;        // sub-words per step (one MFMA depth)
constexpr int SE_PITCH = 40;     // bf16 per LDS row of the P tile: 80 bytes (16-byte aligned, rows 20 banks apart)

// grid (row tiles, E / (64 NE), nsplit), 512 threads = 8 waves as 2 (rows) x 4 (columns): a wave owns 64 rows x 16 NE columns of the output tile.
// Thread t forms P for row t >> 2, sub-words 8 (t & 3) .. + 7 of the step -- exactly one lane's A fragment -- and stores it as 16 bytes of hi and of lo.
// The P tile is double-buffered, so one barrier per step separates its writers from its readers.
template <int NE, bool NOISE>
__global__ __launch_bounds__(512) void vq_soft_embed_kernel(const float* __restrict__ scores, const bf16_t* __restrict__ table, int64_t half_elems,
                                                            const float* __restrict__ row_max, const float* __restrict__ row_den, float* __restrict__ out,
                                                            int R, int V, int E, float inv_temp, uint32_t seed, MaskIds mk, int steps_per_split, int nsteps) {
    __shared__ __attribute__((aligned(16))) bf16_t s_p[2][2][SE_BM * SE_PITCH];     // [buffer][hi / lo]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 2, wn = w & 3;
    const int r0 = blockIdx.x * SE_BM, ez = blockIdx.y, sp = blockIdx.z;
    const int s_begin = sp * steps_per_split, s_end = min(s_begin + steps_per_split, nsteps);
    const int ET = E >> 4, et0 = (ez * 4 + wn) * NE;

    const int prow = tid >> 2, kg = tid & 3, pr = r0 + prow;
    const bool prow_ok = pr < R;
    const float p_mx = prow_ok ? row_max[pr] : 0.f, p_den = prow_ok ? row_den[pr] : 0.f, p_inv = p_den > 0.f ? 1.0f / p_den : 0.f;   // a row with every column masked: P = 0
    const float* srow = scores + (int64_t)(prow_ok ? pr : 0) * V;
    const uint32_t pbase = (uint32_t)pr * (uint32_t)V;

    f32x4_t acc[4][NE];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int s = s_begin; s < s_end; ++s) {
        const int buf = (s - s_begin) & 1;
        {
            uint32_t hi[4], lo[4];
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = s * SE_BK + kg * 8 + j;
                p[j] = 0.f;
                if (prow_ok && v < V && !masked(v, mk)) {
                    float x = srow[v];
                    if (NOISE) x += gumbel_noise(seed, pbase + (uint32_t)v);
                    p[j] = __expf((x - p_mx) * inv_temp) * p_inv;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                hi[j] = pack2bf(p[2 * j], p[2 * j + 1]);
                lo[j] = pack2bf(p[2 * j] - lo2f(hi[j]), p[2 * j + 1] - hi2f(hi[j]));
            }
            *reinterpret_cast<uint4*>(&s_p[buf][0][prow * SE_PITCH + kg * 8]) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            *reinterpret_cast<uint4*>(&s_p[buf][1][prow * SE_PITCH + kg * 8]) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        }
        __syncthreads();
        bf16x8_t ahi[4], alo[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int off = (wm * 64 + mt * 16 + (lane & 15)) * SE_PITCH + (lane >> 4) * 8;
            ahi[mt] = *reinterpret_cast<const bf16x8_t*>(&s_p[buf][0][off]);
            alo[mt] = *reinterpret_cast<const bf16x8_t*>(&s_p[buf][1][off]);
        }
        const bf16_t* tb = table + (((int64_t)s * ET + et0) * 64 + lane) * 8;
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
            const bf16x8_t bhi = *reinterpret_cast<const bf16x8_t*>(tb + (int64_t)nt * 512);
            const bf16x8_t blo = *reinterpret_cast<const bf16x8_t*>(tb + half_elems + (int64_t)nt * 512);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[mt], bhi, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo[mt], bhi, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[mt], blo, acc[mt][nt], 0, 0, 0);
            }
        }
    }
    // C layout: column = lane & 15, row = 4 (lane >> 4) + register
    float* o = out + (int64_t)sp * R * E;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + wm * 64 + mt * 16 + (lane >> 4) * 4 + i;
            if (r < R) {
#pragma unroll
                for (int nt = 0; nt < NE; ++nt) o[(int64_t)r * E + (et0 + nt) * 16 + (lane & 15)] = acc[mt][nt][i];
            }
        }
}

__global__ __launch_bounds__(256) void vq_soft_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a = part[i];
    for (int s = 1; s < nsplit; ++s) a += part[(int64_t)s * n + i];
    out[i] = a;
}

int soft_ne(int E) {
    const int n = E / 64;
    const int cand[6] = {8, 6, 4, 3, 2, 1};
    for (int c : cand)
        if (n % c == 0) return c;
    return 1;
}
int device_cus() {       // compute units of the current device, asked once
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus = n;
    }
    return cus;
}
// auto: about one 512-thread block per compute unit (measured at R = 2048, E = 512: profiles/vq_soft_embed_bench.txt, the nsplit sweep)
int soft_nsplit(int R, int V, int E, int nsplit) {
    const int nsteps = (V + SE_BK - 1) / SE_BK;
    if (nsplit <= 0) {
        const int tiles = ((R + SE_BM - 1) / SE_BM) * (E / (64 * soft_ne(E)));
        nsplit = device_cus() / (tiles > 0 ? tiles : 1);
        if (nsplit > 64) nsplit = 64;
    }
    if (nsplit > nsteps) nsplit = nsteps;
    return nsplit < 1 ? 1 : nsplit;
}
bool fill_mask(MaskIds& mk, const int* ids, int n) {
    if (n < 0 || n > 8 || (n > 0 && ids == nullptr)) return false;
    mk.n = n;
    for (int i = 0; i < n; ++i) mk.id[i] = ids[i];
    return true;
}

template <int NE>
void launch_soft(dim3 grid, hipStream_t s, bool noise, const float* scores, const bf16_t* table, int64_t half_elems, const float* row_max, const float* row_den,
                 float* out, int R, int V, int E, float inv_temp, uint32_t seed, MaskIds mk, int sps, int nsteps) {
    if (noise)
        hipLaunchKernelGGL((vq_soft_embed_kernel<NE, true>), grid, dim3(512), 0, s, scores, table, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps);
    else
        hipLaunchKernelGGL((vq_soft_embed_kernel<NE, false>), grid, dim3(512), 0, s, scores, table, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps);
}

}  // namespace

#define VQ_SIZES_OK(name) SC_CHECK_ARG(R >= 0 && V >= 1 && (int64_t)R * V < ((int64_t)1 << 32), name ": R=%d V=%d (R * V must stay below 2^32: the noise index is 32 bits)", R, V)

extern "C" int sc_vq_gumbel_noise(float* out, int R, int V, uint32_t seed, void* stream) {
    VQ_SIZES_OK("sc_vq_gumbel_noise");
    if (R == 0) return 0;
    SC_CHECK_ARG(out != nullptr, "sc_vq_gumbel_noise: null operand");
    const int64_t n = (int64_t)R * V;
    hipLaunchKernelGGL(vq_gumbel_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n, seed);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_vq_noisy_argmax(const float* scores, int64_t* targets, int R, int V, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, void* stream) {
    VQ_SIZES_OK("sc_vq_noisy_argmax");
    MaskIds mk;
    SC_CHECK_ARG(fill_mask(mk, mask_ids, n_mask), "sc_vq_noisy_argmax: n_mask=%d out of range", n_mask);
    if (R == 0) return 0;
    SC_CHECK_ARG(scores != nullptr && targets != nullptr, "sc_vq_noisy_argmax: null operand");
    if (seed_on) hipLaunchKernelGGL(vq_noisy_argmax_kernel<true>, dim3(R), dim3(256), 0, (hipStream_t)stream, scores, targets, V, seed, mk);
    else hipLaunchKernelGGL(vq_noisy_argmax_kernel<false>, dim3(R), dim3(256), 0, (hipStream_t)stream, scores, targets, V, seed, mk);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_vq_probs(const float* scores, float* out, int R, int V, float temp, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, void* stream) {
    VQ_SIZES_OK("sc_vq_probs");
    MaskIds mk;
    SC_CHECK_ARG(fill_mask(mk, mask_ids, n_mask), "sc_vq_probs: n_mask=%d out of range", n_mask);
    SC_CHECK_ARG(temp > 0.f, "sc_vq_probs: temperature %g must be positive", (double)temp);
    if (R == 0) return 0;
    SC_CHECK_ARG(scores != nullptr && out != nullptr, "sc_vq_probs: null operand");
    if (seed_on) hipLaunchKernelGGL(vq_probs_kernel<true>, dim3(R), dim3(256), 0, (hipStream_t)stream, scores, out, V, 1.0f / temp, seed, mk);
    else hipLaunchKernelGGL(vq_probs_kernel<false>, dim3(R), dim3(256), 0, (hipStream_t)stream, scores, out, V, 1.0f / temp, seed, mk);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_vq_mode_bwd(const float* cos_scores, float* dprob_inout, float* rowdot_cos, float* rowdot_z, int R, int V, float temp, uint32_t seed, int seed_on,
                              const int* mask_ids, int n_mask, void* stream) {
    VQ_SIZES_OK("sc_vq_mode_bwd");
    MaskIds mk;
    SC_CHECK_ARG(fill_mask(mk, mask_ids, n_mask), "sc_vq_mode_bwd: n_mask=%d out of range", n_mask);
    SC_CHECK_ARG(temp > 0.f, "sc_vq_mode_bwd: temperature %g must be positive", (double)temp);
    if (R == 0) return 0;
    SC_CHECK_ARG(cos_scores != nullptr && dprob_inout != nullptr && rowdot_cos != nullptr && rowdot_z != nullptr, "sc_vq_mode_bwd: null operand");
    if (seed_on)
        hipLaunchKernelGGL(vq_mode_bwd_kernel<true>, dim3(R), dim3(256), 0, (hipStream_t)stream, cos_scores, dprob_inout, rowdot_cos, rowdot_z, V, 1.0f / temp, seed, mk);
    else
        hipLaunchKernelGGL(vq_mode_bwd_kernel<false>, dim3(R), dim3(256), 0, (hipStream_t)stream, cos_scores, dprob_inout, rowdot_cos, rowdot_z, V, 1.0f / temp, seed, mk);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t sc_vq_soft_table_bytes(int V, int E) {
    if (V < 1 || E < 64 || E % 64) return 0;
    return (int64_t)2 * ((V + SE_BK - 1) / SE_BK) * SE_BK * E * 2;
}

extern "C" int sc_vq_soft_table(const float* emb, void* table, int V, int E, void* stream) {
    SC_CHECK_ARG(V >= 1 && E >= 64 && E % 64 == 0, "sc_vq_soft_table: V=%d E=%d (E must be a multiple of 64)", V, E);
    SC_CHECK_ARG(emb != nullptr && table != nullptr, "sc_vq_soft_table: null operand");
    const int64_t half_elems = (int64_t)((V + SE_BK - 1) / SE_BK) * SE_BK * E, nvec = half_elems / 8;
    hipLaunchKernelGGL(vq_soft_table_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, (hipStream_t)stream, emb, (bf16_t*)table, V, E, nvec, half_elems);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t sc_vq_soft_embed_workspace_bytes(int R, int V, int E, int nsplit) {
    if (R < 1 || V < 5 || E < 64 || E % 64) return 0;
    const int ns = soft_nsplit(R, V, E, nsplit);
    return ns > 1 ? (int64_t)ns * R * E * 4 : 0;
}

extern "C" int sc_vq_soft_embed(const float* scores, const void* table, float* keywords, float* row_max, float* row_den, void* workspace, int R, int V, int E,
                                float temp, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, int nsplit, void* stream) {
    VQ_SIZES_OK("sc_vq_soft_embed");
    MaskIds mk;
    SC_CHECK_ARG(fill_mask(mk, mask_ids, n_mask), "sc_vq_soft_embed: n_mask=%d out of range", n_mask);
    SC_CHECK_ARG(temp > 0.f, "sc_vq_soft_embed: temperature %g must be positive", (double)temp);
    SC_CHECK_ARG(nsplit >= 0, "sc_vq_soft_embed: nsplit=%d (0 = auto)", nsplit);
    if (E < 64 || E % 64 || V < 5) return 1;      // not covered: the caller composes sc_vq_probs + a GEMM
    if (R == 0) return 0;
    const int ns = soft_nsplit(R, V, E, nsplit);
    SC_CHECK_ARG(scores != nullptr && table != nullptr && keywords != nullptr && row_max != nullptr && row_den != nullptr && (ns == 1 || workspace != nullptr),
                 "sc_vq_soft_embed: null operand");
    hipStream_t s = (hipStream_t)stream;
    const float inv_temp = 1.0f / temp;
    if (seed_on) hipLaunchKernelGGL(vq_row_stats_kernel<true>, dim3(R), dim3(256), 0, s, scores, row_max, row_den, V, inv_temp, seed, mk);
    else hipLaunchKernelGGL(vq_row_stats_kernel<false>, dim3(R), dim3(256), 0, s, scores, row_max, row_den, V, inv_temp, seed, mk);
    SC_CHECK_LAUNCH();
    const int nsteps = (V + SE_BK - 1) / SE_BK, sps = (nsteps + ns - 1) / ns, ne = soft_ne(E);
    const int64_t half_elems = (int64_t)nsteps * SE_BK * E;
    float* out = ns > 1 ? (float*)workspace : keywords;
    const dim3 grid((R + SE_BM - 1) / SE_BM, E / (64 * ne), ns);
    const bf16_t* tab = (const bf16_t*)table;
    const bool noise = seed_on != 0;
    switch (ne) {
        case 8: launch_soft<8>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
        case 6: launch_soft<6>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
        case 4: launch_soft<4>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
        case 3: launch_soft<3>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
        case 2: launch_soft<2>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
        default: launch_soft<1>(grid, s, noise, scores, tab, half_elems, row_max, row_den, out, R, V, E, inv_temp, seed, mk, sps, nsteps); break;
    }
    SC_CHECK_LAUNCH();
    if (ns > 1) {
        const int64_t n = (int64_t)R * E;
        hipLaunchKernelGGL(vq_soft_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)workspace, keywords, n, ns);
        SC_CHECK_LAUNCH();
    }
    return 0;
}
