// Gallery search (include/speechclip_hip.h, "Gallery search"): the K nearest gallery rows of every query row WITHOUT the [Q, N] score image.
//   search_kernel      one block per (query tile, gallery split): fp32 scores on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per (i, j), E walked in
//                      ascending order, one accumulator chain, no split over E), kept in accumulators and selected inside the block.  The block body is
//                      search_core.h's search_block under the plain selection, with F32Rows (search_rows.h) as loading, staging and product.
//   topk_merge_kernel  L candidates per row -> the first K of that order (the partial lists of the splits, of gallery segments, of ranks).
// The split rule and the workspace size of all four search entries are here; the entries' host side is search_core.h's search_host.
// No global atomics; the LDS counters only hand out buffer slots.  Every output element is written once.
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

constexpr int MIN_SPLIT_ROWS = 256;
constexpr int TARGET_BLOCKS = 512;

template <int WQ, int KL>
__global__ __launch_bounds__(256) void search_kernel(const float* __restrict__ q, int64_t ld_q, const float* __restrict__ g, int64_t ld_g, int Q, int N,
                                                      int E, int K, int per, int S, int64_t idx_base, float* __restrict__ out_v,
                                                      int64_t* __restrict__ out_i) {
    search_block<F32Rows, false, WQ, KL>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, nullptr, nullptr, 0, out_v, out_i, nullptr);
}

// K rounds of a block-wide arg-max over L (value, id) pairs; round p picks the first pair strictly after round p-1's pick in (value descending, id
// ascending) order -- topk_rows_kernel's scheme (analysis.hip) with the 64-bit id in place of the position.  Pairs with id < 0 or a NaN value take no part.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ vin, const int64_t* __restrict__ iin, int L, int K, float* __restrict__ vals,
                                                          int64_t* __restrict__ idx) {
    __shared__ float sv[4];
    __shared__ int64_t si[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* rv = vin + (int64_t)blockIdx.x * L;
    const int64_t* ri = iin + (int64_t)blockIdx.x * L;
    constexpr int64_t NONE = INT64_MAX;
    float pv = INFINITY;
    int64_t pi = -1;
    for (int p = 0; p < K; ++p) {
        float bv = -INFINITY;
        int64_t bi = NONE;
        for (int x = threadIdx.x; x < L; x += 256) {
            const float v = rv[x];
            const int64_t id = ri[x];
            const bool eligible = id >= 0 && (v < pv || (v == pv && id > pi));
            if (eligible && (v > bv || (v == bv && id < bi))) { bv = v; bi = id; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int64_t oi = __shfl_xor((long long)bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
        __syncthreads();
        if (threadIdx.x == 0) {
            vals[(int64_t)blockIdx.x * K + p] = bi == NONE ? -INFINITY : bv;
            idx[(int64_t)blockIdx.x * K + p] = bi == NONE ? (int64_t)-1 : bi;
        }
        pv = bi == NONE ? -INFINITY : bv; pi = bi;
    }
}

}  // namespace

// The auto rule: enough blocks for two per CU (256 CUs), no split shorter than 256 gallery rows, at most 1024 splits.
extern "C" int sc_search_splits(int Q, int64_t N, int K) {
    if (Q <= 0 || N <= 0 || K <= 0) return 1;
    const int bq = query_rows_per_block(Q, K);
    const int64_t qtiles = ((int64_t)Q + bq - 1) / bq;
    int64_t s = (TARGET_BLOCKS + qtiles - 1) / qtiles;
    s = s < N / MIN_SPLIT_ROWS ? s : N / MIN_SPLIT_ROWS;
    return (int)(s < 1 ? 1 : s > 1024 ? 1024 : s);
}

// 12 bytes (f32 value + i64 index) per (query, split, slot); one split writes the result directly and needs none.
extern "C" int64_t sc_search_workspace_bytes(int Q, int64_t N, int K, int n_split) {
    if (Q <= 0 || N <= 0 || K <= 0 || n_split < 0) return 0;
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    return S <= 1 ? 0 : (int64_t)Q * S * K * 12;
}

extern "C" int sc_topk_merge(const float* vals_in, const int64_t* idx_in, int Q, int L, int K, float* vals, int64_t* idx, void* stream) {
    SC_CHECK_ARG(K >= 1 && K <= 128, "sc_topk_merge: K=%d must be in [1, 128]", K);
    SC_CHECK_ARG(K <= L, "sc_topk_merge: K=%d exceeds L=%d", K, L);
    SC_CHECK_ARG(Q >= 0, "sc_topk_merge: Q=%d is negative", Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(vals_in && idx_in && vals && idx, "sc_topk_merge: null operand");
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, vals_in, idx_in, L, K, vals, idx);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_search_topk(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                              float* vals, int64_t* idx, void* workspace, void* stream) {
    return search_host<F32Rows, false>("sc_search_topk", 4, 4, {search_kernel<2, 16>, search_kernel<2, 64>, search_kernel<1, 16>, search_kernel<1, 128>}, q, ld_q,
                                       g, ld_g, Q, N, E, K, n_split, idx_base, nullptr, nullptr, 0, vals, idx, nullptr, workspace, stream);
}
