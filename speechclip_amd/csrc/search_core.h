// Gallery search, the part that does not depend on the operand format (include/speechclip_hip.h, "Gallery search" and "Gallery search, bf16 storage"):
// the block of search_kernel (search.hip, fp32 rows) and of search_bf16_kernel (search_bf16.hip, bf16 rows).  One 256-thread block per (query tile, gallery
// split), waves 2 x 2 over 64 WQ query rows x 128 gallery rows; scores stay in the 32 x 32 MFMA accumulators; every score is filtered against its row's
// current K-th entry, survivors go to a per-row LDS candidate buffer, and a full buffer is folded into the row's sorted top-K list by RANK in the total order
// (score descending, j ascending) -- the buffer may fill in any order, the list cannot tell.  No global atomics; the LDS counters only hand out buffer slots.
//
// The operand format OP supplies what differs -- loading, staging and the product:
//   elem                   storage type of a q / g element
//   LDT                    LDS row stride of a stage image, in elements, chosen so that the fragment reads (ds_read_b128) are conflict-free
//   unit, load, store      8 consecutive elements of one row: global -> registers (an absent row or e >= E reads nothing and holds zeros) -> stage image
//   stage<WQ>              acc[a][b] += the products of one staged chunk of KC elements (only those below E), k ascending, one accumulator per (i, j)
// Both MFMAs used (32x32x2_f32, 32x32x16_bf16) leave accumulator x of lane (r, h) = (lane & 31, lane >> 5) at (row (x & 3) + 8 (x >> 2) + 4 h, column r).
#pragma once
#include "common.h"
#include <limits.h>

namespace search_core {

constexpr int BN = 128;          // gallery rows per tile
constexpr int KC = 64;           // elements of E per LDS stage (32 measured the same within 3 % on fp32 rows: DESIGN.md 3.10)
constexpr int NO_J = INT_MAX;    // empty list slot: (-inf, NO_J) comes after every real pair, a real -inf score included

// (av, aj) strictly before (bv, bj) in (score descending, j ascending).  A NaN score is before nothing and nothing is before it.
__device__ __forceinline__ bool before(float av, int aj, float bv, int bj) { return av > bv || (av == bv && aj < bj); }

// query rows per block: the wide tile wherever its list fits (K <= 64) and there is more than one narrow tile of queries
static inline int query_rows_per_block(int Q, int K) { return K <= 64 && Q > 64 ? 128 : 64; }

// WQ: 32-row query tiles per wave (block = 64 WQ query rows x 128 gallery rows, waves 2 x 2); KL: list capacity (K <= KL).
template <class OP, int WQ, int KL>
__device__ __forceinline__ void search_block(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g, int64_t ld_g, int Q,
                                             int N, int E, int K, int per, int S, int64_t idx_base, float* __restrict__ out_v, int64_t* __restrict__ out_i) {
    using elem = typename OP::elem;
    constexpr int LDT = OP::LDT;
    constexpr int BQ = 64 * WQ;
    constexpr int CB = WQ == 2 && KL == 64 ? 16 : 32;      // candidate buffer entries per row (the widest instantiation has 160 KB of LDS to fit)
    constexpr int NQU = 2 * WQ, NGU = 4;                   // a thread's load units per stage: (row, group of 8) of the [BQ][64] and [128][64] stage images
    __shared__ __attribute__((aligned(16))) elem sQ[BQ * LDT];
    __shared__ __attribute__((aligned(16))) elem sG[BN * LDT];
    __shared__ float lv[BQ * KL];      // sorted top list of every row, slots >= count hold (-inf, NO_J)
    __shared__ int lj[BQ * KL];
    __shared__ float cv[BQ * CB];      // candidate buffer, any order
    __shared__ int cj[BQ * CB];
    __shared__ int cnt[BQ];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wq = wave >> 1, wg = wave & 1;
    const int q0 = blockIdx.x * BQ, s = blockIdx.y;
    const int jbeg = (int)min((int64_t)N, (int64_t)s * per), jend = (int)min((int64_t)N, (int64_t)jbeg + per);

    for (int x = tid; x < BQ * KL; x += 256) { lv[x] = -INFINITY; lj[x] = NO_J; }
    for (int x = tid; x < BQ; x += 256) cnt[x] = 0;
    // (the first __syncthreads of the tile loop, or the one before the output, orders these writes)

    // fold the buffer of the rows that are full (or, at the end, non-empty) into their lists; wave w owns rows w, w + 4, ...
    auto compact = [&](bool final) {
        const int myc = lane < BQ / 4 ? cnt[wave + 4 * lane] : 0;        // one read for the wave's rows, then only the rows that have work
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
            for (int u = 0; u < NU; ++u) {                   // list entry p: rank = p + the buffer entries before it
                const int p = lane + 64 * u;
                const bool ok = p < K;
                ev[u] = ok ? Lv[p] : -INFINITY; ej[u] = ok ? Lj[p] : NO_J; rk[u] = ok ? p : KL;
            }
            const bool mine = lane < c;                      // buffer entry: rank = the list entries before it + the buffer entries before it
            const float mv = mine ? Cv[lane] : -INFINITY;
            const int mj = mine ? Cj[lane] : NO_J;
            int lo = 0, hi = K;
            for (int step = 32 - __builtin_clz(K); step > 0; --step) {   // bit_length(K) halvings empty [0, K]
                const int mid = (lo + hi) >> 1;
                if (lo < hi) { if (before(Lv[mid], Lj[mid], mv, mj)) lo = mid + 1; else hi = mid; }
            }
            int mr = lo;
            // buffer entry x sits in lane x's registers: broadcast it from there (lanes >= c hold (-inf, NO_J), which is before nothing)
#pragma unroll
            for (int x = 0; x < CB; ++x) {
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

    f32x16_t acc[WQ][2];
    for (int tile = 0, it = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[a][b][x] = 0.f;
        for (int chunk = 0; chunk < nchunk; ++chunk, ++it) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NQU; ++u) OP::store(sQ + (urow + 32 * u) * LDT + uc8, pq[u]);
#pragma unroll
            for (int u = 0; u < NGU; ++u) OP::store(sG + (urow + 32 * u) * LDT + uc8, pg[u]);
            __syncthreads();
            if (it + 1 < total) prefetch(it + 1);            // the next stage's global loads are in flight during the multiply
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
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                    if (j < jend && q0 + i < Q && before(acc[a][b][x], j, tv, tj)) pend |= 1ull << ((a * 2 + b) * 16 + x);
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
    }
}

}  // namespace search_core
