// Gallery search on bf16 rows (include/speechclip_hip.h, "Gallery search, bf16 storage"): sc_search_topk with q and g stored in bf16 -- half the gallery bytes,
// the product on v_mfma_f32_32x32x16_bf16.
//   search_bf16_kernel  search_core.h's search_block under the plain selection, with Bf16Rows (search_rows.h) as loading, staging and product: a lane holds 8
//                       consecutive k of its row, one ds_read_b128 supplies its k-group of a 16-wide MFMA step, stage rows are 128 bytes.  The bf16 products
//                       are exact in fp32; each (i, j) has one fp32 accumulator, E is walked in ascending groups of 16 and never split over blocks.
// The host side is search_core.h's search_host; splits, workspace and the merge of the partial lists are those of search.hip (sc_search_splits,
// sc_search_workspace_bytes, sc_topk_merge).
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

template <int WQ, int KL>
__global__ __launch_bounds__(256) void search_bf16_kernel(const bf16_t* __restrict__ q, int64_t ld_q, const bf16_t* __restrict__ g, int64_t ld_g, int Q, int N,
                                                           int E, int K, int per, int S, int64_t idx_base, float* __restrict__ out_v,
                                                           int64_t* __restrict__ out_i) {
    search_block<Bf16Rows, false, WQ, KL>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, nullptr, nullptr, 0, out_v, out_i, nullptr);
}

}  // namespace

extern "C" int sc_search_topk_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                   float* vals, int64_t* idx, void* workspace, void* stream) {
    return search_host<Bf16Rows, false>("sc_search_topk_bf16", 16, 8,
                                        {search_bf16_kernel<2, 16>, search_bf16_kernel<2, 64>, search_bf16_kernel<1, 16>, search_bf16_kernel<1, 128>},
                                        (const bf16_t*)q, ld_q, (const bf16_t*)g, ld_g, Q, N, E, K, n_split, idx_base, nullptr, nullptr, 0, vals, idx, nullptr,
                                        workspace, stream);
}
