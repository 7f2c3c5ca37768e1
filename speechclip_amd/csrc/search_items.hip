// Gallery search by item (include/speechclip_hip.h, "Gallery search by item"): the K nearest DISTINCT item codes of every query row, a query's own item left
// out -- sc_search_topk / sc_search_topk_bf16 with a predicate and a tie rule inside the selection, no new score.
//   search_items_kernel      search_core.h's search_block under the selection by item (eligibility filter, dominance inside the rank fold, item codes as a
//                            third output), for both operand formats of search_rows.h: loading, staging and the product are the ones of the plain kernels,
//                            so the scores are theirs bit for bit.
//   topk_merge_items_kernel  L candidates per row -> the first K, or with `distinct` the first K whose item codes differ: K rounds of a block-wide arg-max; the
//                            candidates of a picked item are retired in an LDS bitmap.
// The host side of both entries is search_core.h's search_host.  Every output element is written once.
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

constexpr int MERGE_MAX_L = 1024 * 128;      // the dead bitmap of topk_merge_items_kernel: one bit per candidate, 16 KB

template <class OP, int WQ, int KL>
__global__ __launch_bounds__(256) void search_items_kernel(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g,
                                                            int64_t ld_g, int Q, int N, int E, int K, int per, int S, int64_t idx_base,
                                                            const int32_t* __restrict__ g_item, const int32_t* __restrict__ q_skip, int distinct,
                                                            float* __restrict__ out_v, int64_t* __restrict__ out_i, int32_t* __restrict__ out_c) {
    search_block<OP, true, WQ, KL>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, g_item, q_skip, distinct, out_v, out_i, out_c);
}

// topk_merge_kernel (search.hip) with the item code carried along.  distinct == 0: round p picks the first (value, id) pair strictly after round p-1's pick.
// distinct != 0: a round picks the first live pair and the next round's scan retires every candidate that carries the picked item code (the pick itself among
// them) in `dead`: candidate x = t + 256 m is bit (m & 31) of word (m >> 5) * 256 + t, so a thread reads and writes its own words only -- no atomics, no
// barrier for the bitmap, no bank conflict.  Pairs with id < 0 or a NaN value take no part.  Of equal (value, id) pairs the one with the lower item code is
// picked (and, without `distinct`, emitted once, as sc_topk_merge does).
__global__ __launch_bounds__(256) void topk_merge_items_kernel(const float* __restrict__ vin, const int64_t* __restrict__ iin, const int32_t* __restrict__ cin,
                                                                int L, int K, int distinct, float* __restrict__ vals, int64_t* __restrict__ idx,
                                                                int32_t* __restrict__ items) {
    __shared__ float sv[4];
    __shared__ int64_t si[4];
    __shared__ int sc[4];
    __shared__ uint32_t dead[(MERGE_MAX_L / 256 / 32) * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* rv = vin + (int64_t)blockIdx.x * L;
    const int64_t* ri = iin + (int64_t)blockIdx.x * L;
    const int32_t* rc = cin + (int64_t)blockIdx.x * L;
    constexpr int64_t NONE = INT64_MAX;
    if (distinct)
        for (int w = 0; w * 32 * 256 < L; ++w) dead[w * 256 + tid] = 0;
    float pv = INFINITY;
    int64_t pi = -1;
    int pc = 0;
    bool picked = false;
    for (int p = 0; p < K; ++p) {
        float bv = -INFINITY;
        int64_t bi = NONE;
        int bc = INT_MAX;
        for (int x = tid, m = 0; x < L; x += 256, ++m) {
            const float v = rv[x];
            const int64_t id = ri[x];
            const int c = rc[x];
            bool eligible;
            if (distinct) {
                uint32_t w = dead[(m >> 5) * 256 + tid];
                const uint32_t bit = 1u << (m & 31);
                if (picked && c == pc && !(w & bit)) { w |= bit; dead[(m >> 5) * 256 + tid] = w; }
                eligible = id >= 0 && !(w & bit);
            } else {
                eligible = id >= 0 && (v < pv || (v == pv && id > pi));
            }
            if (eligible && (v > bv || (v == bv && (id < bi || (id == bi && c < bc))))) { bv = v; bi = id; bc = c; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int64_t oi = __shfl_xor((long long)bi, off, 64);
            const int oc = __shfl_xor(bc, off, 64);
            if (ov > bv || (ov == bv && (oi < bi || (oi == bi && oc < bc)))) { bv = ov; bi = oi; bc = oc; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; sc[wave] = bc; }
        __syncthreads();
        bv = sv[0]; bi = si[0]; bc = sc[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && (si[w] < bi || (si[w] == bi && sc[w] < bc)))) { bv = sv[w]; bi = si[w]; bc = sc[w]; }
        __syncthreads();
        const bool none = bi == NONE;
        if (tid == 0) {
            vals[(int64_t)blockIdx.x * K + p] = none ? -INFINITY : bv;
            idx[(int64_t)blockIdx.x * K + p] = none ? (int64_t)-1 : bi;
            items[(int64_t)blockIdx.x * K + p] = none ? -1 : bc;
        }
        pv = none ? -INFINITY : bv; pi = bi; pc = none ? INT_MAX : bc;
        picked = !none;
    }
}

}  // namespace

// 16 bytes (i64 index + f32 value + i32 item code) per (query, split, slot); one split writes the result directly and needs none.
extern "C" int64_t sc_search_items_workspace_bytes(int Q, int64_t N, int K, int n_split) {
    if (Q <= 0 || N <= 0 || K <= 0 || n_split < 0) return 0;
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    return S <= 1 ? 0 : (int64_t)Q * S * K * 16;
}

extern "C" int sc_topk_merge_items(const float* vals_in, const int64_t* idx_in, const int32_t* items_in, int Q, int L, int K, int distinct, float* vals,
                                   int64_t* idx, int32_t* items, void* stream) {
    SC_CHECK_ARG(K >= 1 && K <= 128, "sc_topk_merge_items: K=%d must be in [1, 128]", K);
    SC_CHECK_ARG(K <= L, "sc_topk_merge_items: K=%d exceeds L=%d", K, L);
    SC_CHECK_ARG(!distinct || L <= MERGE_MAX_L, "sc_topk_merge_items: L=%d exceeds %d (distinct)", L, MERGE_MAX_L);
    SC_CHECK_ARG(Q >= 0, "sc_topk_merge_items: Q=%d is negative", Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(vals_in && idx_in && items_in && vals && idx && items, "sc_topk_merge_items: null operand");
    hipLaunchKernelGGL(topk_merge_items_kernel, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, vals_in, idx_in, items_in, L, K, distinct, vals, idx,
                       items);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_search_items(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                               const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace,
                               void* stream) {
    using OP = F32Rows;
    return search_host<OP, true>("sc_search_items", 4, 4,
                                 {search_items_kernel<OP, 2, 16>, search_items_kernel<OP, 2, 64>, search_items_kernel<OP, 1, 16>, search_items_kernel<OP, 1, 128>}, q,
                                 ld_q, g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip, distinct, vals, idx, items, workspace, stream);
}

extern "C" int sc_search_items_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                    const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace,
                                    void* stream) {
    using OP = Bf16Rows;
    return search_host<OP, true>("sc_search_items_bf16", 16, 8,
                                 {search_items_kernel<OP, 2, 16>, search_items_kernel<OP, 2, 64>, search_items_kernel<OP, 1, 16>, search_items_kernel<OP, 1, 128>},
                                 (const bf16_t*)q, ld_q, (const bf16_t*)g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip, distinct, vals, idx, items,
                                 workspace, stream);
}
