// Gallery search on bf16 rows (include/speechclip_hip.h, "Gallery search, bf16 storage"): sc_search_topk with q and g stored in bf16 -- half the gallery bytes,
// the product on v_mfma_f32_32x32x16_bf16.
//   search_bf16_kernel  search_core.h's search_block (one block per (query tile, gallery split), scores kept in accumulators, per-row candidate buffers folded
//                       into sorted lists by rank) with Bf16Rows (search_rows.h) as loading, staging and product: a lane holds 8 consecutive k of its row, one
//                       ds_read_b128 supplies its k-group of a 16-wide MFMA step, stage rows are 128 bytes.  The bf16 products are exact in fp32; each (i, j)
//                       has one fp32 accumulator, E is walked in ascending groups of 16 and never split over blocks.
// Splits, workspace and the merge of the partial lists are those of search.hip (sc_search_splits, sc_search_workspace_bytes, sc_topk_merge).
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
    search_block<Bf16Rows, WQ, KL>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, out_v, out_i);
}

}  // namespace

extern "C" int sc_search_topk_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                   float* vals, int64_t* idx, void* workspace, void* stream) {
    SC_CHECK_ARG(E >= 16 && E <= 1024 && E % 16 == 0, "sc_search_topk_bf16: E=%d must be a multiple of 16 in [16, 1024]", E);
    SC_CHECK_ARG(ld_q >= E && ld_g >= E && ld_q % 8 == 0 && ld_g % 8 == 0, "sc_search_topk_bf16: ld_q=%lld / ld_g=%lld must be multiples of 8 and >= E=%d",
                 (long long)ld_q, (long long)ld_g, E);
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)g) & 15) == 0, "sc_search_topk_bf16: q and g must be 16-byte aligned");
    SC_CHECK_ARG(K >= 1 && K <= 128, "sc_search_topk_bf16: K=%d must be in [1, 128]", K);
    SC_CHECK_ARG(N < ((int64_t)1 << 31), "sc_search_topk_bf16: N=%lld must be below 2^31", (long long)N);
    SC_CHECK_ARG(K <= N, "sc_search_topk_bf16: K=%d exceeds N=%lld", K, (long long)N);
    SC_CHECK_ARG(n_split >= 0 && n_split <= 1024, "sc_search_topk_bf16: n_split=%d must be in [0, 1024] (0 = auto)", n_split);
    SC_CHECK_ARG(Q >= 0, "sc_search_topk_bf16: Q=%d is negative", Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(q && g && vals && idx, "sc_search_topk_bf16: null operand");
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    SC_CHECK_ARG(S == 1 || workspace, "sc_search_topk_bf16: %d splits need a workspace (sc_search_workspace_bytes)", S);
    const int per = (int)((N + S - 1) / S);
    int64_t* wi = (int64_t*)workspace;                       // [Q][S][K] i64, then [Q][S][K] f32
    float* wv = (float*)(wi + (int64_t)Q * S * K);
    float* ov = S == 1 ? vals : wv;
    int64_t* oi = S == 1 ? idx : wi;
    const int bq = query_rows_per_block(Q, K);
    const dim3 grid((unsigned)((Q + bq - 1) / bq), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* q16 = (const bf16_t*)q;
    const bf16_t* g16 = (const bf16_t*)g;
#define SC_SEARCH_LAUNCH(WQ, KL) \
    hipLaunchKernelGGL((search_bf16_kernel<WQ, KL>), grid, dim3(256), 0, st, q16, ld_q, g16, ld_g, Q, (int)N, E, K, per, S, idx_base, ov, oi)
    if (bq == 128) { if (K <= 16) SC_SEARCH_LAUNCH(2, 16); else SC_SEARCH_LAUNCH(2, 64); }
    else           { if (K <= 16) SC_SEARCH_LAUNCH(1, 16); else SC_SEARCH_LAUNCH(1, 128); }
#undef SC_SEARCH_LAUNCH
    SC_CHECK_LAUNCH();
    if (S > 1) return sc_topk_merge(wv, wi, Q, S * K, K, vals, idx, stream);
    return 0;
}
