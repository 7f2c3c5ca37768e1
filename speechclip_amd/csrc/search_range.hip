// Gallery search by threshold (include/speechclip_hip.h, "Gallery search by threshold"): every gallery row whose score reaches the query's threshold, in
// ascending row order, WITHOUT the [Q, N] score image and without atomics.  Two passes over the same scores:
//   range_count_kernel  one block per (query tile, gallery range): the number of hits of every query row in the range -> counts[i, s].
//   range_fill_kernel   the same walk again; the hits of (i, s) are written from offs[i, s] on, which the caller derived from the counts by an exclusive scan.
// Both are range_block below.  The stage loop is search_core.h's search_block restated (256 threads, waves 2 x 2 over 64 WQ query rows x 128 gallery rows,
// KC = 64, the next stage's loads in flight during the multiply), with F32Rows / Bf16Rows (search_rows.h) as loading, staging and product: the scores are
// those of sc_search_topk / sc_search_topk_bf16 bit for bit.  There is no K-list and no candidate buffer, so the wide query tile is used whenever Q > 64.
// Where a hit goes: for a fixed accumulator (a, b, x) the 64-bit ballot of "is a hit" holds two query rows (lane half h) x 32 gallery columns (lane r), so
// popcounts of its halves count a row's hits in one 32-column group, and the bits below lane r give a hit's place inside its group.  A tile has four column
// groups (wave column wg, accumulator b); their counts go through a [rows][4] table in LDS, and a per-row running position carries across the tiles.
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

// `old` with the wave-uniform value v in lane l (a compile-time constant below 64 at every call)
__device__ __forceinline__ int put_lane(int v, int l, int old) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(v), "n"(l));
#endif
    return old;
}

// FILL == false: counts[(q0 + i) * ld_tab + s] (int32) = the hits of row i in range s; offs / out_v / out_i are not touched.
// FILL == true:  the hits are written from offs[(q0 + i) * ld_tab + s] (int64) on, ascending j; counts is not touched.
template <class OP, int WQ, bool FILL>
__device__ __forceinline__ void range_block(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g, int64_t ld_g, int Q,
                                            int N, int E, const float* __restrict__ thresh, int per, const int32_t* __restrict__ g_item,
                                            const int32_t* __restrict__ q_skip, int64_t idx_base, int32_t* __restrict__ counts,
                                            const int64_t* __restrict__ offs, int64_t ld_tab, float* __restrict__ out_v, int64_t* __restrict__ out_i) {
    using elem = typename OP::elem;
    constexpr int LDT = OP::LDT;
    constexpr int BQ = 64 * WQ;
    constexpr int RW = 32 * WQ;                            // query rows of one wave
    constexpr int NQU = 2 * WQ, NGU = 4;                   // a thread's load units per stage: (row, group of 8) of the [BQ][64] and [128][64] stage images
    __shared__ __attribute__((aligned(16))) elem sQ[BQ * LDT];
    __shared__ __attribute__((aligned(16))) elem sG[BN * LDT];
    __shared__ float th[BQ];                               // the row's threshold; NaN for a row beyond Q: nothing reaches it
    __shared__ int skips[BQ];                              // the row's skip code, -1: none
    __shared__ __attribute__((aligned(16))) int grp[FILL ? 2 * BQ * 4 : BQ * 2];   // fill: hits per (row, column group) of a tile, two tiles deep; count: per (wave column, row)
    __shared__ int64_t run[FILL ? BQ : 1];                 // fill: where the row's next hit goes

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wq = wave >> 1, wg = wave & 1;
    const int q0 = blockIdx.x * BQ, s = blockIdx.y;
    const int jbeg = (int)min((int64_t)N, (int64_t)s * per), jend = (int)min((int64_t)N, (int64_t)jbeg + per);
    const bool has_skip = q_skip != nullptr;

    for (int x = tid; x < BQ; x += 256) {
        const bool ok = q0 + x < Q;
        th[x] = ok ? thresh[q0 + x] : NAN;
        skips[x] = has_skip && ok ? q_skip[q0 + x] : -1;
        if constexpr (FILL) run[x] = ok ? offs[(int64_t)(q0 + x) * ld_tab + s] : 0;
    }
    // (the first __syncthreads of the tile loop orders these writes; without a tile nothing reads them)

    const int nchunk = (E + KC - 1) / KC;
    const int ntiles = (jend - jbeg + BN - 1) / BN;
    const int total = ntiles * nchunk;
    const int urow = tid >> 3, uc8 = (tid & 7) * 8;          // unit u of a thread: row urow + 32 u, elements uc8 .. uc8 + 7 of the stage
    typename OP::unit pq[NQU], pg[NGU];
    auto prefetch = [&](int it) {
        const int tile = it / nchunk, e = (it - tile * nchunk) * KC + uc8;
#pragma unroll
        for (int u = 0; u < NQU; ++u) {
            const int row = q0 + urow + 32 * u;
            OP::load(q + (int64_t)row * ld_q, row < Q, e, E, pq[u]);
        }
#pragma unroll
        for (int u = 0; u < NGU; ++u) {
            const int row = jbeg + tile * BN + urow + 32 * u;
            OP::load(g + (int64_t)row * ld_g, row < jend, e, E, pg[u]);
        }
    };
    if (total > 0) prefetch(0);

    int mine = 0;                                            // count: the hits so far of wave row `lane` in this wave's 64 columns
    f32x16_t acc[WQ][2];
    for (int tile = 0, it = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[a][b][x] = 0.f;
        int jc[2] = {-1, -1};                                // item codes of this lane's two gallery rows, in flight during the multiply
        if (has_skip) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                if (j < jend) jc[b] = g_item[j];
            }
        }
        for (int chunk = 0; chunk < nchunk; ++chunk, ++it) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NQU; ++u) OP::store(sQ + (urow + 32 * u) * LDT + uc8, pq[u]);
#pragma unroll
            for (int u = 0; u < NGU; ++u) OP::store(sG + (urow + 32 * u) * LDT + uc8, pg[u]);
            __syncthreads();
            if (it + 1 < total) prefetch(it + 1);            // the next stage's global loads are in flight during the multiply
            OP::template stage<WQ>(acc, sQ + (wq * RW + r) * LDT, sG + (wg * 64 + r) * LDT, h, chunk * KC, E);
        }
        // ---- hits: accumulator (a, b, x) of this lane is query row i = wq*RW + 32a + (x&3) + 8(x>>2) + 4h, gallery row j = jbeg + tile*128 + wg*64 + 32b + r
        [[maybe_unused]] int* tab = grp;
        if constexpr (FILL) {
            // the row's position moves past the tile before: its four counts are complete since that tile's barrier, its readers are behind this tile's
            // stage barriers, and this tile's counts go to the other half of the table
            if (tile > 0 && tid < BQ) {
                const int4 c = *(const int4*)(grp + (((tile - 1) & 1) * BQ + tid) * 4);
                run[tid] += c.x + c.y + c.z + c.w;
            }
            tab = grp + (tile & 1) * BQ * 4;
        }
        uint64_t hit = 0;                                    // bit (a*2 + b)*16 + x
        int gc[2] = {0, 0};                                  // the hits of wave row `lane` in this tile's column groups 2 wg and 2 wg + 1
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int il = a * 32 + (x & 3) + 8 * (x >> 2);          // wave row of lane half 0; half 1 holds il + 4
                const int i = wq * RW + il + 4 * h;
                const float t = th[i];
                const int skip = skips[i];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                    const bool is = j < jend && (skip < 0 || jc[b] != skip) && acc[a][b][x] >= t;    // (a NaN score or threshold reaches nothing)
                    if (is) hit |= 1ull << ((a * 2 + b) * 16 + x);
                    const uint64_t bal = __ballot(is);               // bits 0..31: wave row il, bits 32..63: wave row il + 4; each row once per tile and b
                    gc[b] = put_lane(__popc((uint32_t)bal), il, gc[b]);
                    gc[b] = put_lane(__popc((uint32_t)(bal >> 32)), il + 4, gc[b]);
                }
            }
        if constexpr (!FILL) {
            mine += gc[0] + gc[1];
        } else {
            if (lane < RW) *(int2*)(tab + (wq * RW + lane) * 4 + wg * 2) = int2{gc[0], gc[1]};
            __syncthreads();
            if (__ballot(hit != 0)) {
#pragma unroll
                for (int a = 0; a < WQ; ++a)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int i = wq * RW + a * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
                        const int4 c = *(const int4*)(tab + i * 4);
                        const int64_t at = run[i];
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const bool is = (hit >> ((a * 2 + b) * 16 + x)) & 1;
                            const uint64_t bal = __ballot(is);
                            const uint32_t half = h ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                            if (is) {
                                const int before_group = wg ? c.x + c.y + (b ? c.z : 0) : (b ? c.x : 0);
                                const int64_t o = at + before_group + __popc(half & ((1u << r) - 1u));
                                out_v[o] = acc[a][b][x];
                                out_i[o] = idx_base + (jbeg + tile * BN + wg * 64 + b * 32 + r);
                            }
                        }
                    }
            }
        }
    }
    if constexpr (!FILL) {
        __syncthreads();                                     // (also orders th / skips / the stage images of a block without tiles: nothing to order there)
        if (lane < RW) grp[wg * BQ + wq * RW + lane] = mine;
        __syncthreads();
        if (tid < BQ && q0 + tid < Q) counts[(int64_t)(q0 + tid) * ld_tab + s] = grp[tid] + grp[BQ + tid];
    }
}

template <class OP, int WQ>
__global__ __launch_bounds__(256) void range_count_kernel(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g,
                                                           int64_t ld_g, int Q, int N, int E, const float* __restrict__ thresh, int per,
                                                           const int32_t* __restrict__ g_item, const int32_t* __restrict__ q_skip, int32_t* __restrict__ counts,
                                                           int64_t ld_counts) {
    range_block<OP, WQ, false>(q, ld_q, g, ld_g, Q, N, E, thresh, per, g_item, q_skip, 0, counts, nullptr, ld_counts, nullptr, nullptr);
}

template <class OP, int WQ>
__global__ __launch_bounds__(256) void range_fill_kernel(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g,
                                                          int64_t ld_g, int Q, int N, int E, const float* __restrict__ thresh, int per,
                                                          const int32_t* __restrict__ g_item, const int32_t* __restrict__ q_skip, int64_t idx_base,
                                                          const int64_t* __restrict__ offs, int64_t ld_offs, float* __restrict__ out_v,
                                                          int64_t* __restrict__ out_i) {
    range_block<OP, WQ, true>(q, ld_q, g, ld_g, Q, N, E, thresh, per, g_item, q_skip, idx_base, nullptr, offs, ld_offs, out_v, out_i);
}

// The host side of the four entries: the argument rules of sc_search_topk[_bf16] (e_mul / ld_mul as in search_core.h's search_host) and those of the two
// tables, the split rule, the launch.  counts != null: the count pass; else the fill pass.
template <class OP>
int range_host(const char* name, int e_mul, int ld_mul, const typename OP::elem* q, int64_t ld_q, const typename OP::elem* g, int64_t ld_g, int Q, int64_t N, int E,
               const float* thresh, int n_split, const int32_t* g_item, const int32_t* q_skip, bool fill, int64_t idx_base, int32_t* counts, const int64_t* offs,
               int64_t ld_tab, float* vals, int64_t* idx, void* stream) {
    SC_CHECK_ARG(E >= e_mul && E <= 1024 && E % e_mul == 0, "%s: E=%d must be a multiple of %d in [%d, 1024]", name, E, e_mul, e_mul);
    SC_CHECK_ARG(ld_q >= E && ld_g >= E && ld_q % ld_mul == 0 && ld_g % ld_mul == 0, "%s: ld_q=%lld / ld_g=%lld must be multiples of %d and >= E=%d", name,
                 (long long)ld_q, (long long)ld_g, ld_mul, E);
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)g) & 15) == 0, "%s: q and g must be 16-byte aligned", name);
    SC_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "%s: N=%lld must be in [0, 2^31)", name, (long long)N);
    SC_CHECK_ARG(n_split >= 0 && n_split <= 1024, "%s: n_split=%d must be in [0, 1024] (0 = auto)", name, n_split);
    SC_CHECK_ARG(Q >= 0, "%s: Q=%d is negative", name, Q);
    const int S = n_split ? n_split : sc_search_splits(Q, N, 1);
    SC_CHECK_ARG(ld_tab >= S, "%s: %s=%lld is below the %d splits", name, fill ? "ld_offs" : "ld_counts", (long long)ld_tab, S);
    if (Q == 0) return 0;
    SC_CHECK_ARG(q && g && (fill ? offs && vals && idx : counts != nullptr), "%s: null operand", name);
    SC_CHECK_ARG(thresh, "%s: null thresh (an fp32 threshold per query is required)", name);
    SC_CHECK_ARG(!q_skip || g_item, "%s: q_skip without g_item (an int32 item code per gallery row is required)", name);
    const int per = (int)((N + S - 1) / S);
    const bool wide = Q > 64;
    const int bq = wide ? 128 : 64;
    const dim3 grid((unsigned)((Q + bq - 1) / bq), (unsigned)S);
    if (fill) {
        auto* const k = wide ? range_fill_kernel<OP, 2> : range_fill_kernel<OP, 1>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, q, ld_q, g, ld_g, Q, (int)N, E, thresh, per, g_item, q_skip, idx_base, offs, ld_tab, vals,
                           idx);
    } else {
        auto* const k = wide ? range_count_kernel<OP, 2> : range_count_kernel<OP, 1>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, q, ld_q, g, ld_g, Q, (int)N, E, thresh, per, g_item, q_skip, counts, ld_tab);
    }
    SC_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int sc_search_range_count(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                                     const int32_t* g_item, const int32_t* q_skip, int32_t* counts, int64_t ld_counts, void* stream) {
    return range_host<F32Rows>("sc_search_range_count", 4, 4, q, ld_q, g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip, false, 0, counts, nullptr, ld_counts,
                               nullptr, nullptr, stream);
}

extern "C" int sc_search_range_fill(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                                    const int32_t* g_item, const int32_t* q_skip, int64_t idx_base, const int64_t* offs, int64_t ld_offs, float* vals,
                                    int64_t* idx, void* stream) {
    return range_host<F32Rows>("sc_search_range_fill", 4, 4, q, ld_q, g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip, true, idx_base, nullptr, offs, ld_offs,
                               vals, idx, stream);
}

extern "C" int sc_search_range_count_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                                          const int32_t* g_item, const int32_t* q_skip, int32_t* counts, int64_t ld_counts, void* stream) {
    return range_host<Bf16Rows>("sc_search_range_count_bf16", 16, 8, (const bf16_t*)q, ld_q, (const bf16_t*)g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip,
                                false, 0, counts, nullptr, ld_counts, nullptr, nullptr, stream);
}

extern "C" int sc_search_range_fill_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                                         const int32_t* g_item, const int32_t* q_skip, int64_t idx_base, const int64_t* offs, int64_t ld_offs, float* vals,
                                         int64_t* idx, void* stream) {
    return range_host<Bf16Rows>("sc_search_range_fill_bf16", 16, 8, (const bf16_t*)q, ld_q, (const bf16_t*)g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip,
                                true, idx_base, nullptr, offs, ld_offs, vals, idx, stream);
}
