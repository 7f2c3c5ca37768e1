// Gallery search inside a subset (include/speechclip_hip.h, "Gallery search by subset"): sc_search_items / sc_search_items_bf16 with two more conjuncts in
// eligible(i, j) -- a row mask shared by all queries (one bit per gallery row) and a per-query group code that a row must carry -- and a scan that skips the
// gallery tiles in which the mask allows nothing.
//   search_select_kernel     search_core.h's search_block under the selection by subset (SELECT on top of ITEMS), for both operand formats of search_rows.h:
//                            loading, staging, the product, the candidate buffer and the rank fold are the ones of the kernels by item, so scores and order are
//                            theirs bit for bit.  The block walks the LIVE tiles of its range only (search_block's next_live): a dead tile costs neither global
//                            loads of its rows, nor an LDS stage, nor an MFMA.
//   pack_row_mask_kernel     one byte per row -> one bit per row: a wave ballots 64 bytes into two words.
// The host side of both search entries is search_core.h's search_host; the partial lists of the splits are joined by sc_topk_merge_items.
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

template <class OP, int WQ, int KL>
__global__ __launch_bounds__(256) void search_select_kernel(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g,
                                                             int64_t ld_g, int Q, int N, int E, int K, int per, int S, int64_t idx_base,
                                                             const int32_t* __restrict__ g_item, const int32_t* __restrict__ q_skip, int distinct,
                                                             float* __restrict__ out_v, int64_t* __restrict__ out_i, int32_t* __restrict__ out_c,
                                                             const uint32_t* __restrict__ g_allow, const int32_t* __restrict__ g_group,
                                                             const int32_t* __restrict__ q_group) {
    search_block<OP, true, WQ, KL, true>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, g_item, q_skip, distinct, out_v, out_i, out_c, g_allow, g_group, q_group);
}

// Thread t of the grid owns row t; lane 0 of a wave writes the word of the wave's rows 0 .. 31, lane 32 that of rows 32 .. 63.  A word is written iff it holds
// a row below N; rows at or above N ballot 0, so the unused high bits of the last word are 0.
__global__ __launch_bounds__(256) void pack_row_mask_kernel(const uint8_t* __restrict__ mask, int64_t N, uint32_t* __restrict__ words) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t bits = __ballot(j < N && mask[j] != 0);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && j < N) words[j >> 5] = (uint32_t)(bits >> lane);
}

}  // namespace

extern "C" int sc_pack_row_mask(const uint8_t* mask, int64_t N, uint32_t* words, void* stream) {
    SC_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "sc_pack_row_mask: N=%lld must be in [0, 2^31)", (long long)N);
    if (N == 0) return 0;
    SC_CHECK_ARG(mask && words, "sc_pack_row_mask: null operand");
    hipLaunchKernelGGL(pack_row_mask_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, N, words);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_search_select(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                const uint32_t* g_allow, const int32_t* g_group, const int32_t* q_group, const int32_t* g_item, const int32_t* q_skip,
                                int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream) {
    using OP = F32Rows;
    return search_host<OP, true, true>(
        "sc_search_select", 4, 4, {search_select_kernel<OP, 2, 16>, search_select_kernel<OP, 2, 64>, search_select_kernel<OP, 1, 16>, search_select_kernel<OP, 1, 128>},
        q, ld_q, g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip, distinct, vals, idx, items, workspace, stream, g_allow, g_group, q_group);
}

extern "C" int sc_search_select_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                     const uint32_t* g_allow, const int32_t* g_group, const int32_t* q_group, const int32_t* g_item, const int32_t* q_skip,
                                     int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream) {
    using OP = Bf16Rows;
    return search_host<OP, true, true>(
        "sc_search_select_bf16", 16, 8,
        {search_select_kernel<OP, 2, 16>, search_select_kernel<OP, 2, 64>, search_select_kernel<OP, 1, 16>, search_select_kernel<OP, 1, 128>}, (const bf16_t*)q, ld_q,
        (const bf16_t*)g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip, distinct, vals, idx, items, workspace, stream, g_allow, g_group, q_group);
}
