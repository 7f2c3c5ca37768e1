// Gallery search, second stage (include/speechclip_hip.h, "Gallery search, fp32 re-score of a shortlist"): the R rows that a bf16 search shortlisted for a
// query are scored again on the fp32 rows with sc_search_topk's arithmetic, the first K of them in sc_search_topk's order are the result, and a flag per
// query says whether the caller's error bound PROVES that no row outside the shortlist can be among the first K of the whole gallery.
//   search_rescore_kernel   one 128-thread block per query, thread t = shortlist slot t.  The query row sits in LDS; the R candidate rows are GATHERED in
//                           stages of KC = 64 elements by the whole block -- 16 lanes read 256 consecutive bytes of one row, 16-byte loads, the next stage in
//                           flight in registers while the current one is multiplied -- into a [128][68] image (F32Rows' row stride: 68 t mod 64 = 4 t, so the
//                           sixteen lanes of a ds_read_b128 group hit sixteen different 4-bank slots), and thread t walks row t of the image with plain fmaf:
//                           ONE accumulator, e ascending, the chain of sc_search_topk in every bit.  Then every slot's rank among the R (score, j) pairs is
//                           COUNTED in LDS with search_core.h's before(), ranks below K fill the output list, and thread 0 evaluates the certificate on it.
// A slot that is -1 or names no row of [idx_base, idx_base + N) is never dereferenced: its units load nothing and it enters the ranking as NaN, which is
// before nothing and which nothing is before.  No atomics; every output element is written once.
#include "common.h"
#include "search_core.h"
#include "../../include/speechclip_hip.h"
#include <math.h>

namespace {

using namespace search_core;

constexpr int RT = 128;              // threads per block = shortlist slots (R <= 128)
constexpr int LDT = KC + 4;          // LDS row stride of the stage image in floats (see above)
constexpr int NU = KC / 4;           // 16-byte units of one stage per thread: 128 rows x 16 units / 128 threads
constexpr int EMAX = 1024;

__global__ __launch_bounds__(RT) void search_rescore_kernel(const float* __restrict__ q, int64_t ld_q, const float* __restrict__ g, int64_t ld_g, int N, int E,
                                                             const int64_t* __restrict__ cand_idx, const float* __restrict__ short_vals, int R,
                                                             const float* __restrict__ eps, int K, int64_t idx_base, float* __restrict__ vals,
                                                             int64_t* __restrict__ idx, int32_t* __restrict__ certified) {
    __shared__ __attribute__((aligned(16))) float sQ[EMAX];
    __shared__ __attribute__((aligned(16))) float sG[RT * LDT];
    __shared__ int sJ[RT];           // slot -> gallery row, -1: the slot names none
    __shared__ float sV[RT];         // slot -> score, NaN: takes no part
    __shared__ float oV[RT];         // the list by rank
    __shared__ int oJ[RT];

    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    int j = -1;
    if (tid < R) {
        const int64_t c = cand_idx[i * R + tid];
        const uint64_t off = (uint64_t)c - (uint64_t)idx_base;
        if (c != -1 && off < (uint64_t)N) j = (int)off;
    }
    sJ[tid] = j;
    oV[tid] = -INFINITY;
    oJ[tid] = -1;
    for (int e = tid * 4; e < E; e += RT * 4) *(f32x4_t*)(sQ + e) = *(const f32x4_t*)(q + i * ld_q + e);
    const int in_range = __syncthreads_count(j >= 0);

    // unit u of a thread: elements uc4 .. uc4 + 3 of the stage, row urow + 8 u of the image (rows >= R and slots that name no row load nothing)
    const int urow = tid >> 4, uc4 = (tid & 15) * 4;
    const int nu = (R + 7) >> 3;
    int ju[NU];                      // the gallery row of unit u, -1: none (rows >= R hold -1 too)
#pragma unroll
    for (int u = 0; u < NU; ++u) ju[u] = sJ[urow + 8 * u];
    f32x4_t pg[NU];
    auto prefetch = [&](int chunk) {
        const int e = chunk * KC + uc4;
        const unsigned lim = e < E ? (unsigned)N : 0u;       // one unsigned compare per unit says "a row, and inside it": -1 is above every N
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
            pg[u] = (unsigned)ju[u] < lim ? *(const f32x4_t*)(g + (int64_t)ju[u] * ld_g + e) : z;
        }
    };
    const int nchunk = (E + KC - 1) / KC;
    prefetch(0);

    float acc = 0.f;
    const float* rg = sG + tid * LDT;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NU; ++u)
            if (u < nu) *(f32x4_t*)(sG + (urow + 8 * u) * LDT + uc4) = pg[u];
        __syncthreads();
        if (chunk + 1 < nchunk) prefetch(chunk + 1);         // the next stage's gather is in flight during the multiply
        const float* rq = sQ + chunk * KC;
        if ((chunk + 1) * KC <= E) {
#pragma unroll
            for (int x = 0; x < KC / 4; ++x) {
                const f32x4_t a = *(const f32x4_t*)(rq + 4 * x), b = *(const f32x4_t*)(rg + 4 * x);
                acc = fmaf(a[0], b[0], acc);
                acc = fmaf(a[1], b[1], acc);
                acc = fmaf(a[2], b[2], acc);
                acc = fmaf(a[3], b[3], acc);
            }
        } else {                                             // the last stage of a row: E % 4 == 0, whole units only
            const int n4 = (E - chunk * KC) >> 2;
            for (int x = 0; x < n4; ++x) {
                const f32x4_t a = *(const f32x4_t*)(rq + 4 * x), b = *(const f32x4_t*)(rg + 4 * x);
                acc = fmaf(a[0], b[0], acc);
                acc = fmaf(a[1], b[1], acc);
                acc = fmaf(a[2], b[2], acc);
                acc = fmaf(a[3], b[3], acc);
            }
        }
    }

    const float v = j >= 0 ? acc : __builtin_nanf("");
    sV[tid] = v;
    __syncthreads();
    if (v == v) {                                            // rank = the slots before this one in (score descending, j ascending)
        int rank = 0;
        for (int u = 0; u < R; ++u) rank += before(sV[u], sJ[u], v, j) ? 1 : 0;
        if (rank < K) { oV[rank] = v; oJ[rank] = j; }
    }
    __syncthreads();
    if (tid < K) {
        const int oj = oJ[tid];
        vals[i * K + tid] = oj < 0 ? -INFINITY : oV[tid];
        idx[i * K + tid] = oj < 0 ? (int64_t)-1 : idx_base + oj;
    }
    if (tid == 0) {
        const float last = short_vals[i * R + R - 1];
        const float kth = oJ[K - 1] < 0 ? -INFINITY : oV[K - 1];
        const bool proven = R == N || (double)kth > (double)last + (double)eps[i];
        certified[i] = in_range == R && last == last && proven ? 1 : 0;
    }
}

}  // namespace

extern "C" int sc_search_rescore(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const int64_t* cand_idx,
                                 const float* short_vals, int R, const float* eps, int K, int64_t idx_base, float* vals, int64_t* idx, int32_t* certified,
                                 void* stream) {
    SC_CHECK_ARG(E >= 4 && E <= EMAX && E % 4 == 0, "sc_search_rescore: E=%d must be a multiple of 4 in [4, 1024]", E);
    SC_CHECK_ARG(ld_q >= E && ld_g >= E && ld_q % 4 == 0 && ld_g % 4 == 0, "sc_search_rescore: ld_q=%lld / ld_g=%lld must be multiples of 4 and >= E=%d",
                 (long long)ld_q, (long long)ld_g, E);
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)g) & 15) == 0, "sc_search_rescore: q and g must be 16-byte aligned");
    SC_CHECK_ARG(K >= 1 && K <= 128, "sc_search_rescore: K=%d must be in [1, 128]", K);
    SC_CHECK_ARG(R >= K && R <= RT, "sc_search_rescore: R=%d must be in [K=%d, 128]", R, K);
    SC_CHECK_ARG(N >= 1 && N < ((int64_t)1 << 31), "sc_search_rescore: N=%lld must be in [1, 2^31)", (long long)N);
    SC_CHECK_ARG(Q >= 0, "sc_search_rescore: Q=%d is negative", Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(q && g && cand_idx && short_vals && eps && vals && idx && certified, "sc_search_rescore: null operand");
    hipLaunchKernelGGL(search_rescore_kernel, dim3((unsigned)Q), dim3(RT), 0, (hipStream_t)stream, q, ld_q, g, ld_g, (int)N, E, cand_idx, short_vals, R, eps, K,
                       idx_base, vals, idx, certified);
    SC_CHECK_LAUNCH();
    return 0;
}
