// Gallery search by item (include/speechclip_hip.h, "Gallery search by item"): the K nearest DISTINCT item codes of every query row, a query's own item left
// out -- sc_search_topk / sc_search_topk_bf16 with a predicate and a tie rule inside the selection, no new score.
//   search_items_kernel      search_core.h's search_block with three changes (search_items_block below): a score is pushed only if it is ELIGIBLE (its row's
//                            item code differs from the query's skip code) and before its row's K-th entry; with `distinct` the rank fold first drops every
//                            entry of list + buffer that is DOMINATED (another entry with the same item code is before it) and ranks the survivors among the
//                            survivors; the output carries the item codes.  Loading, staging and the product are search_rows.h's F32Rows / Bf16Rows, the ones
//                            of the plain kernels, so the scores are theirs bit for bit.  The list and the buffer hold (score, j) as before: an entry's item
//                            code is g_item[j], read from global memory (N * 4 bytes, L2-resident) only inside a `distinct` fold and for the output, so the
//                            four (WQ, list capacity) instantiations of the plain kernels and their LDS sizes carry over (+ 4 bytes per query row).
//   topk_merge_items_kernel  L candidates per row -> the first K, or with `distinct` the first K whose item codes differ: K rounds of a block-wide arg-max; the
//                            candidates of a picked item are retired in an LDS bitmap.
// No global atomics; the LDS counters only hand out buffer slots.  Every output element is written once.
#include "common.h"
#include "search_core.h"
#include "search_rows.h"
#include "../../include/speechclip_hip.h"

namespace {

using namespace search_core;

constexpr int MERGE_MAX_L = 1024 * 128;      // the dead bitmap of topk_merge_items_kernel: one bit per candidate, 16 KB

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1; }

// search_block (search_core.h) with the eligibility filter, the dominance fold and the item output.  g_item: int32 [N]; q_skip: int32 [Q] or null.
template <class OP, int WQ, int KL>
__device__ __forceinline__ void search_items_block(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g, int64_t ld_g,
                                                   int Q, int N, int E, int K, int per, int S, int64_t idx_base, const int32_t* __restrict__ g_item,
                                                   const int32_t* __restrict__ q_skip, int distinct, float* __restrict__ out_v, int64_t* __restrict__ out_i,
                                                   int32_t* __restrict__ out_c) {
    using elem = typename OP::elem;
    constexpr int LDT = OP::LDT;
    constexpr int BQ = 64 * WQ;
    constexpr int CB = WQ == 2 && KL == 64 ? 16 : 32;      // candidate buffer entries per row, as search_block
    constexpr int NQU = 2 * WQ, NGU = 4;
    __shared__ __attribute__((aligned(16))) elem sQ[BQ * LDT];
    __shared__ __attribute__((aligned(16))) elem sG[BN * LDT];
    __shared__ float lv[BQ * KL];      // sorted top list of every row, slots >= count hold (-inf, NO_J); with `distinct` its item codes are all different
    __shared__ int lj[BQ * KL];
    __shared__ float cv[BQ * CB];      // candidate buffer, any order
    __shared__ int cj[BQ * CB];
    __shared__ int cnt[BQ];
    __shared__ int sk[BQ];             // the row's skip code, -1: none

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wq = wave >> 1, wg = wave & 1;
    const int q0 = blockIdx.x * BQ, s = blockIdx.y;
    const int jbeg = (int)min((int64_t)N, (int64_t)s * per), jend = (int)min((int64_t)N, (int64_t)jbeg + per);
    const bool has_skip = q_skip != nullptr;

    for (int x = tid; x < BQ * KL; x += 256) { lv[x] = -INFINITY; lj[x] = NO_J; }
    for (int x = tid; x < BQ; x += 256) { cnt[x] = 0; sk[x] = has_skip && q0 + x < Q ? q_skip[q0 + x] : -1; }
    // (the first __syncthreads of the tile loop, or the one before the output, orders these writes)

    // fold the buffer of the rows that are full (or, at the end, non-empty) into their lists; wave w owns rows w, w + 4, ...
    auto compact = [&](bool final) {
        const int myc = lane < BQ / 4 ? cnt[wave + 4 * lane] : 0;
        uint64_t todo = __ballot(final ? myc > 0 : myc >= CB);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int i = wave + 4 * l;
            const int c = min(__builtin_amdgcn_readlane(myc, l), CB);
            float* Lv = lv + i * KL; int* Lj = lj + i * KL;
            const float* Cv = cv + i * CB; const int* Cj = cj + i * CB;
            constexpr int NU = KL > 64 ? 2 : 1;
            float ev[NU]; int ej[NU], rk[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int p = lane + 64 * u;
                const bool ok = p < K;
                ev[u] = ok ? Lv[p] : -INFINITY; ej[u] = ok ? Lj[p] : NO_J; rk[u] = ok ? p : KL;
            }
            const bool mine = lane < c;
            const float mv = mine ? Cv[lane] : -INFINITY;
            const int mj = mine ? Cj[lane] : NO_J;
            // ---- dominance: an entry goes if another entry of list + buffer with its item code is before it.  The list's codes are all different, so only
            // buffer entries can dominate a list entry; a buffer entry falls to a list entry or to another buffer entry.  An empty slot (-inf, NO_J, code -1)
            // is before nothing, so it dominates nothing.
            uint64_t bdom = 0, dm[NU];                       // dominated buffer entries / list entries (bit = lane of chunk u)
#pragma unroll
            for (int u = 0; u < NU; ++u) dm[u] = 0;
            if (distinct) {
                int ec[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) ec[u] = ej[u] != NO_J ? g_item[ej[u]] : -1;
                const int mc = mine ? g_item[mj] : -1;
                bool ld[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) ld[u] = false;
#pragma unroll
                for (int x = 0; x < CB; ++x) {
                    const float xv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mv), x));
                    const int xj = __builtin_amdgcn_readlane(mj, x);
                    const int xc = __builtin_amdgcn_readlane(mc, x);
                    bool d = mc == xc && before(mv, mj, xv, xj);             // this lane's buffer entry dominates x (strict order: never itself)
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const bool same = ec[u] == xc;
                        ld[u] |= same && before(xv, xj, ev[u], ej[u]);
                        d |= same && before(ev[u], ej[u], xv, xj);
                    }
                    if (__ballot(d)) bdom |= 1ull << x;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) dm[u] = __ballot(ld[u]);
            }
            // ---- ranks among the survivors: list entry p = the surviving list entries above it + the surviving buffer entries before it; buffer entry =
            // the surviving list entries before it (binary search, minus the dominated ones among those) + the surviving buffer entries before it
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                int gone = __popcll(dm[u] & low_bits(lane));
#pragma unroll
                for (int w = 0; w < u; ++w) gone += __popcll(dm[w]);
                if (rk[u] < KL) rk[u] -= gone;
                if ((dm[u] >> lane) & 1) rk[u] = KL;
            }
            int lo = 0, hi = K;
            for (int step = 32 - __builtin_clz(K); step > 0; --step) {
                const int mid = (lo + hi) >> 1;
                if (lo < hi) { if (before(Lv[mid], Lj[mid], mv, mj)) lo = mid + 1; else hi = mid; }
            }
            int mr = lo;
#pragma unroll
            for (int u = 0; u < NU; ++u) mr -= __popcll(dm[u] & low_bits(lo - 64 * u));
            if ((bdom >> lane) & 1) mr = KL;
#pragma unroll
            for (int x = 0; x < CB; ++x) {
                if ((bdom >> x) & 1) continue;                                  // wave-uniform
                const float xv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mv), x));
                const int xj = __builtin_amdgcn_readlane(mj, x);
#pragma unroll
                for (int u = 0; u < NU; ++u) rk[u] += before(xv, xj, ev[u], ej[u]) ? 1 : 0;
                mr += before(xv, xj, mv, mj) ? 1 : 0;
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every lane of the wave has its reads before any slot is rewritten
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (rk[u] < K) { Lv[rk[u]] = ev[u]; Lj[rk[u]] = ej[u]; }
            if (mine && mr < K) { Lv[mr] = mv; Lj[mr] = mj; }
            if (lane == 0) cnt[i] = 0;
        }
    };

    const int nchunk = (E + KC - 1) / KC;
    const int ntiles = (jend - jbeg + BN - 1) / BN;
    const int total = ntiles * nchunk;
    const int urow = tid >> 3, uc8 = (tid & 7) * 8;
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

    f32x16_t acc[WQ][2];
    for (int tile = 0, it = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[a][b][x] = 0.f;
        int jc[2] = {-1, -1};                                    // item codes of this lane's two gallery rows: in flight during the multiply
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
            if (it + 1 < total) prefetch(it + 1);
            OP::template stage<WQ>(acc, sQ + (wq * 32 * WQ + r) * LDT, sG + (wg * 64 + r) * LDT, h, chunk * KC, E);
        }
        // ---- selection: accumulator (a, b, x) of this lane is query row i = wq*32*WQ + 32a + (x&3) + 8(x>>2) + 4h, gallery row j below
        uint64_t pend = 0;
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int i = wq * 32 * WQ + a * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
                const float tv = lv[i * KL + K - 1];
                const int tj = lj[i * KL + K - 1];
                const int skip = sk[i];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                    const bool eligible = skip < 0 || jc[b] != skip;           // (a NaN score is before nothing)
                    if (j < jend && q0 + i < Q && eligible && before(acc[a][b][x], j, tv, tj)) pend |= 1ull << ((a * 2 + b) * 16 + x);
                }
            }
        while (__syncthreads_or(pend != 0)) {
#pragma unroll
            for (int a = 0; a < WQ; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const uint64_t bit = 1ull << ((a * 2 + b) * 16 + x);
                        if (pend & bit) {
                            const int i = wq * 32 * WQ + a * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
                            const int pos = atomicAdd(&cnt[i], 1);
                            if (pos < CB) {
                                cv[i * CB + pos] = acc[a][b][x];
                                cj[i * CB + pos] = jbeg + tile * BN + wg * 64 + b * 32 + r;
                                pend &= ~bit;
                            }
                        }
                    }
            __syncthreads();
            compact(false);
            __syncthreads();
            if (pend) {                                      // a score that found its row's buffer full: is it still ahead of the new K-th entry?
#pragma unroll
                for (int a = 0; a < WQ; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int x = 0; x < 16; ++x) {
                            const uint64_t bit = 1ull << ((a * 2 + b) * 16 + x);
                            if (pend & bit) {
                                const int i = wq * 32 * WQ + a * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
                                const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                                if (!before(acc[a][b][x], j, lv[i * KL + K - 1], lj[i * KL + K - 1])) pend &= ~bit;
                            }
                        }
            }
        }
    }
    __syncthreads();
    compact(true);
    __syncthreads();
    for (int x = tid; x < BQ * K; x += 256) {
        const int i = x / K, p = x - i * K;
        if (q0 + i >= Q) continue;
        const int j = lj[i * KL + p];
        const int64_t o = ((int64_t)(q0 + i) * S + s) * K + p;
        out_v[o] = j == NO_J ? -INFINITY : lv[i * KL + p];
        out_i[o] = j == NO_J ? (int64_t)-1 : idx_base + j;
        out_c[o] = j == NO_J ? -1 : g_item[j];
    }
}

template <class OP, int WQ, int KL>
__global__ __launch_bounds__(256) void search_items_kernel(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g,
                                                            int64_t ld_g, int Q, int N, int E, int K, int per, int S, int64_t idx_base,
                                                            const int32_t* __restrict__ g_item, const int32_t* __restrict__ q_skip, int distinct,
                                                            float* __restrict__ out_v, int64_t* __restrict__ out_i, int32_t* __restrict__ out_c) {
    search_items_block<OP, WQ, KL>(q, ld_q, g, ld_g, Q, N, E, K, per, S, idx_base, g_item, q_skip, distinct, out_v, out_i, out_c);
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

// The argument rules, split rule, workspace and launch of both entries; `name` is the entry's, for the messages.  e_mul / ld_mul: what E and the row strides
// must be multiples of in this operand format (sc_search_topk: 4 / 4, sc_search_topk_bf16: 16 / 8).
template <class OP>
int search_items(const char* name, int e_mul, int ld_mul, const typename OP::elem* q, int64_t ld_q, const typename OP::elem* g, int64_t ld_g, int Q, int64_t N,
                 int E, int K, int n_split, int64_t idx_base, const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx,
                 int32_t* items, void* workspace, void* stream) {
    SC_CHECK_ARG(E >= e_mul && E <= 1024 && E % e_mul == 0, "%s: E=%d must be a multiple of %d in [%d, 1024]", name, E, e_mul, e_mul);
    SC_CHECK_ARG(ld_q >= E && ld_g >= E && ld_q % ld_mul == 0 && ld_g % ld_mul == 0, "%s: ld_q=%lld / ld_g=%lld must be multiples of %d and >= E=%d", name,
                 (long long)ld_q, (long long)ld_g, ld_mul, E);
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)g) & 15) == 0, "%s: q and g must be 16-byte aligned", name);
    SC_CHECK_ARG(K >= 1 && K <= 128, "%s: K=%d must be in [1, 128]", name, K);
    SC_CHECK_ARG(N < ((int64_t)1 << 31), "%s: N=%lld must be below 2^31", name, (long long)N);
    SC_CHECK_ARG(K <= N, "%s: K=%d exceeds N=%lld", name, K, (long long)N);
    SC_CHECK_ARG(n_split >= 0 && n_split <= 1024, "%s: n_split=%d must be in [0, 1024] (0 = auto)", name, n_split);
    SC_CHECK_ARG(Q >= 0, "%s: Q=%d is negative", name, Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(q && g && vals && idx, "%s: null operand", name);
    SC_CHECK_ARG(g_item, "%s: null g_item (an int32 item code per gallery row is required)", name);
    SC_CHECK_ARG(items, "%s: null items", name);
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    SC_CHECK_ARG(S == 1 || workspace, "%s: %d splits need a workspace (sc_search_items_workspace_bytes)", name, S);
    const int per = (int)((N + S - 1) / S);
    int64_t* wi = (int64_t*)workspace;                       // [Q][S][K] i64, then [Q][S][K] f32, then [Q][S][K] i32
    float* wv = (float*)(wi + (int64_t)Q * S * K);
    int32_t* wc = (int32_t*)(wv + (int64_t)Q * S * K);
    float* ov = S == 1 ? vals : wv;
    int64_t* oi = S == 1 ? idx : wi;
    int32_t* oc = S == 1 ? items : wc;
    const int bq = query_rows_per_block(Q, K);
    const dim3 grid((unsigned)((Q + bq - 1) / bq), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
#define SC_SEARCH_LAUNCH(WQ, KL)                                                                                                                            \
    hipLaunchKernelGGL((search_items_kernel<OP, WQ, KL>), grid, dim3(256), 0, st, q, ld_q, g, ld_g, Q, (int)N, E, K, per, S, idx_base, g_item, q_skip, distinct, \
                       ov, oi, oc)
    if (bq == 128) { if (K <= 16) SC_SEARCH_LAUNCH(2, 16); else SC_SEARCH_LAUNCH(2, 64); }
    else           { if (K <= 16) SC_SEARCH_LAUNCH(1, 16); else SC_SEARCH_LAUNCH(1, 128); }
#undef SC_SEARCH_LAUNCH
    SC_CHECK_LAUNCH();
    if (S > 1) return sc_topk_merge_items(wv, wi, wc, Q, S * K, K, distinct, vals, idx, items, stream);
    return 0;
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
    return search_items<F32Rows>("sc_search_items", 4, 4, q, ld_q, g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip, distinct, vals, idx, items, workspace,
                                 stream);
}

extern "C" int sc_search_items_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                                    const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace,
                                    void* stream) {
    return search_items<Bf16Rows>("sc_search_items_bf16", 16, 8, (const bf16_t*)q, ld_q, (const bf16_t*)g, ld_g, Q, N, E, K, n_split, idx_base, g_item, q_skip,
                                  distinct, vals, idx, items, workspace, stream);
}
