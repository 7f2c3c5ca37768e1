// Gallery search, everything that does not depend on the operand format (include/speechclip_hip.h, "Gallery search", "Gallery search, bf16 storage" and
// "Gallery search by item"): ONE block body and ONE host driver for the four entries.
//   search_block      the block of search_kernel (search.hip, fp32 rows), search_bf16_kernel (search_bf16.hip, bf16 rows) and search_items_kernel
//                     (search_items.hip, both formats).  One 256-thread block per (query tile, gallery split), waves 2 x 2 over 64 WQ query rows x 128 gallery
//                     rows; scores stay in the 32 x 32 MFMA accumulators; every score is filtered against its row's current K-th entry, survivors go to a
//                     per-row LDS candidate buffer, and a full buffer is folded into the row's sorted top-K list by RANK in the total order (score descending,
//                     j ascending) -- the buffer may fill in any order, the list cannot tell.  No global atomics; the LDS counters only hand out buffer slots.
//   search_host       argument rules, split and workspace arithmetic, launch and merge of sc_search_topk, sc_search_topk_bf16, sc_search_items and
//                     sc_search_items_bf16.
// Two SELECTIONS, chosen at compile time by ITEMS:
//   ITEMS == false    the plain one: the first K (score, j) pairs.
//   ITEMS == true     by item: a score is pushed only if it is ELIGIBLE (its row's item code g_item[j] differs from the query's skip code) and before its row's
//                     K-th entry; with `distinct` the rank fold first drops every entry of list + buffer that is DOMINATED (another entry with the same item
//                     code is before it) and ranks the survivors among the survivors; a third output carries the item codes.  The list and the buffer hold
//                     (score, j) either way: an entry's item code is g_item[j], read from global memory (N * 4 bytes, L2-resident) only inside a `distinct`
//                     fold and for the output, so both selections have the same four (WQ, list capacity) instantiations and LDS sizes (+ 4 bytes of skip
//                     code per query row by item).
// Everything by item stands under `if constexpr (ITEMS)`, its LDS array included: the plain instantiations hold none of it.
// A third selection, BY SUBSET (SELECT, on top of ITEMS; search_select.hip, "Gallery search by subset"), adds two conjuncts to eligibility -- the row's bit in
// a mask shared by all queries, and a group code the row must share with the query -- and walks only the LIVE tiles of the block's range, those with an
// allowed row (next_live below): the mask words of a range are the same for every thread of the block, so every wave finds the same next tile by a ballot,
// with no LDS list, no barrier and no atomics.  Everything by subset stands under `if constexpr (SELECT)`, its LDS array (a group code per query row) and
// its loop control included: the other instantiations compile to what they compiled to without it.
//
// The operand format OP (search_rows.h) supplies what differs between fp32 and bf16 rows -- loading, staging and the product:
//   elem                   storage type of a q / g element
//   LDT                    LDS row stride of a stage image, in elements, chosen so that the fragment reads (ds_read_b128) are conflict-free
//   unit, load, store      8 consecutive elements of one row: global -> registers (an absent row or e >= E reads nothing and holds zeros) -> stage image
//   stage<WQ>              acc[a][b] += the products of one staged chunk of KC elements (only those below E), k ascending, one accumulator per (i, j)
// Both MFMAs used (32x32x2_f32, 32x32x16_bf16) leave accumulator x of lane (r, h) = (lane & 31, lane >> 5) at (row (x & 3) + 8 (x >> 2) + 4 h, column r).
#pragma once
#include "common.h"
#include "../../include/speechclip_hip.h"
#include <limits.h>

namespace search_core {

constexpr int BN = 128;          // gallery rows per tile
constexpr int KC = 64;           // elements of E per LDS stage (32 measured the same within 3 % on fp32 rows: DESIGN.md 3.10)
constexpr int NO_J = INT_MAX;    // empty list slot: (-inf, NO_J) comes after every real pair, a real -inf score included

// (av, aj) strictly before (bv, bj) in (score descending, j ascending).  A NaN score is before nothing and nothing is before it.
__device__ __forceinline__ bool before(float av, int aj, float bv, int bj) { return av > bv || (av == bv && aj < bj); }

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1; }

// query rows per block: the wide tile wherever its list fits (K <= 64) and there is more than one narrow tile of queries
static inline int query_rows_per_block(int Q, int K) { return K <= 64 && Q > 64 ? 128 : 64; }

// WQ: 32-row query tiles per wave (block = 64 WQ query rows x 128 gallery rows, waves 2 x 2); KL: list capacity (K <= KL).
// By item only (the plain kernels pass null / 0): g_item int32 [N], q_skip int32 [Q] or null, distinct, out_c.
// By subset only (SELECT, on top of ITEMS): g_allow uint32 [ceil(N / 32)] or null, g_group int32 [N] and q_group int32 [Q] or both null.
template <class OP, bool ITEMS, int WQ, int KL, bool SELECT = false>
__device__ __forceinline__ void search_block(const typename OP::elem* __restrict__ q, int64_t ld_q, const typename OP::elem* __restrict__ g, int64_t ld_g, int Q,
                                             int N, int E, int K, int per, int S, int64_t idx_base, const int32_t* __restrict__ g_item,
                                             const int32_t* __restrict__ q_skip, int distinct, float* __restrict__ out_v, int64_t* __restrict__ out_i,
                                             int32_t* __restrict__ out_c, const uint32_t* __restrict__ g_allow = nullptr,
                                             const int32_t* __restrict__ g_group = nullptr, const int32_t* __restrict__ q_group = nullptr) {
    static_assert(ITEMS || !SELECT, "the selection by subset extends the selection by item");
    using elem = typename OP::elem;
    constexpr int LDT = OP::LDT;
    constexpr int BQ = 64 * WQ;
    constexpr int CB = WQ == 2 && KL == 64 ? 16 : 32;      // candidate buffer entries per row (the widest instantiation has 160 KB of LDS to fit)
    constexpr int NQU = 2 * WQ, NGU = 4;                   // a thread's load units per stage: (row, group of 8) of the [BQ][64] and [128][64] stage images
    __shared__ __attribute__((aligned(16))) elem sQ[BQ * LDT];
    __shared__ __attribute__((aligned(16))) elem sG[BN * LDT];
    __shared__ float lv[BQ * KL];      // sorted top list of every row, slots >= count hold (-inf, NO_J); with `distinct` its item codes are all different
    __shared__ int lj[BQ * KL];
    __shared__ float cv[BQ * CB];      // candidate buffer, any order
    __shared__ int cj[BQ * CB];
    __shared__ int cnt[BQ];
    int* skips = nullptr;              // by item: the row's skip code, -1: none
    if constexpr (ITEMS) {
        __shared__ int sk[BQ];         // (hipcc orders a kernel's LDS by the arrays' names: renaming one moves the others)
        skips = sk;
    }
    int* groups = nullptr;             // by subset: the row's group code, -1: no restriction
    if constexpr (SELECT) {
        __shared__ int sg_q[BQ];
        groups = sg_q;
    }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wq = wave >> 1, wg = wave & 1;
    const int q0 = blockIdx.x * BQ, s = blockIdx.y;
    const int jbeg = (int)min((int64_t)N, (int64_t)s * per), jend = (int)min((int64_t)N, (int64_t)jbeg + per);
    const bool has_skip = ITEMS && q_skip != nullptr;
    const bool has_group = SELECT && q_group != nullptr;

    for (int x = tid; x < BQ * KL; x += 256) { lv[x] = -INFINITY; lj[x] = NO_J; }
    for (int x = tid; x < BQ; x += 256) {
        cnt[x] = 0;
        if constexpr (ITEMS) skips[x] = has_skip && q0 + x < Q ? q_skip[q0 + x] : -1;
        if constexpr (SELECT) groups[x] = has_group && q0 + x < Q ? q_group[q0 + x] : -1;
    }
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
            uint64_t bdom = 0, dm[NU];                       // by item: dominated buffer entries / list entries (bit = lane of chunk u)
            if constexpr (ITEMS) {
                // ---- dominance: an entry goes if another entry of list + buffer with its item code is before it.  The list's codes are all different, so
                // only buffer entries can dominate a list entry; a buffer entry falls to a list entry or to another buffer entry.  An empty slot (-inf, NO_J,
                // code -1) is before nothing, so it dominates nothing.
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
                // ---- ranks among the survivors: list entry p = the surviving list entries above it + the surviving buffer entries before it (below)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    int gone = __popcll(dm[u] & low_bits(lane));
#pragma unroll
                    for (int w = 0; w < u; ++w) gone += __popcll(dm[w]);
                    if (rk[u] < KL) rk[u] -= gone;
                    if ((dm[u] >> lane) & 1) rk[u] = KL;
                }
            }
            int lo = 0, hi = K;
            for (int step = 32 - __builtin_clz(K); step > 0; --step) {   // bit_length(K) halvings empty [0, K]
                const int mid = (lo + hi) >> 1;
                if (lo < hi) { if (before(Lv[mid], Lj[mid], mv, mj)) lo = mid + 1; else hi = mid; }
            }
            int mr = lo;
            if constexpr (ITEMS) {                           // buffer entry: the surviving list entries before it = those before it minus the dominated ones
#pragma unroll
                for (int u = 0; u < NU; ++u) mr -= __popcll(dm[u] & low_bits(lo - 64 * u));
                if ((bdom >> lane) & 1) mr = KL;
            }
            // buffer entry x sits in lane x's registers: broadcast it from there (lanes >= c hold (-inf, NO_J), which is before nothing)
#pragma unroll
            for (int x = 0; x < CB; ++x) {
                if constexpr (ITEMS) {
                    if ((bdom >> x) & 1) continue;           // wave-uniform
                }
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
    // by subset: the first LIVE tile at or after `from` -- a tile with an allowed row inside the block's range; ntiles if there is none.  Lane l of every
    // wave tests tile from + l (the words that hold its rows, the first and the last masked to the rows), a ballot names the first: wave-uniform, the same
    // in all four waves, no LDS and no atomics.  Only words [jbeg >> 5, (jend - 1) >> 5] are read.
    auto next_live = [&](int from) {
        if (g_allow == nullptr) return from;
        for (int base = from; base < ntiles; base += 64) {
            const int t = base + lane;
            bool live = false;
            if (t < ntiles) {
                const int a = jbeg + t * BN, b = min(a + BN, jend) - 1;      // rows a .. b, a <= b < jend
                for (int w = a >> 5; w <= b >> 5; ++w) {
                    uint32_t bits = g_allow[w];
                    if (w == a >> 5) bits &= ~0u << (a & 31);
                    if (w == b >> 5) bits &= ~0u >> (31 - (b & 31));
                    live |= bits != 0;
                }
            }
            const uint64_t any = __ballot(live);
            if (any) return base + (int)__builtin_ctzll(any);
        }
        return ntiles;
    };
    int first = 0, nxt = 0;                                  // by subset: the first live tile and the live tile after the current one
    if constexpr (SELECT) {
        first = next_live(0);
        if (first < ntiles) prefetch(first * nchunk);
    } else {
        if (total > 0) prefetch(0);
    }

    f32x16_t acc[WQ][2];
    for (int tile = first, it = first * nchunk; tile < ntiles; ++tile) {
        if constexpr (SELECT) nxt = next_live(tile + 1);     // its first chunk is prefetched during this tile's last multiply
#pragma unroll
        for (int a = 0; a < WQ; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[a][b][x] = 0.f;
        int jc[2] = {-1, -1};                                // by item: item codes of this lane's two gallery rows, in flight during the multiply
        if constexpr (ITEMS) {
            if (has_skip) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                    if (j < jend) jc[b] = g_item[j];
                }
            }
        }
        int jg[2] = {-1, -1};                                // by subset: group codes and allow bits of the same two rows
        bool ja[2] = {true, true};
        if constexpr (SELECT) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                if (j < jend) {
                    if (has_group) jg[b] = g_group[j];
                    if (g_allow != nullptr) ja[b] = (g_allow[j >> 5] >> (j & 31)) & 1;
                }
            }
        }
        for (int chunk = 0; chunk < nchunk; ++chunk, ++it) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NQU; ++u) OP::store(sQ + (urow + 32 * u) * LDT + uc8, pq[u]);
#pragma unroll
            for (int u = 0; u < NGU; ++u) OP::store(sG + (urow + 32 * u) * LDT + uc8, pg[u]);
            __syncthreads();
            if constexpr (SELECT) {                          // the next stage's global loads are in flight during the multiply
                const int ahead = chunk + 1 == nchunk ? nxt * nchunk : it + 1;
                if (ahead < total) prefetch(ahead);
            } else {
                if (it + 1 < total) prefetch(it + 1);        // the next stage's global loads are in flight during the multiply
            }
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
                int skip = -1;
                if constexpr (ITEMS) skip = skips[i];
                int group = -1;
                if constexpr (SELECT) group = groups[i];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int j = jbeg + tile * BN + wg * 64 + b * 32 + r;
                    bool eligible = true;                    // (a NaN score is before nothing)
                    if constexpr (ITEMS) eligible = skip < 0 || jc[b] != skip;
                    if constexpr (SELECT) eligible = eligible && ja[b] && (group < 0 || jg[b] == group);
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
        if constexpr (SELECT) { tile = nxt - 1; it = nxt * nchunk; }     // on to the next live tile (the loop adds the 1)
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
        if constexpr (ITEMS) out_c[o] = j == NO_J ? -1 : g_item[j];
    }
}

// The host side of the four search entries: argument rules, split rule, workspace layout, launch, and the merge of the splits' partial lists.
//   name             the entry's, for the messages
//   e_mul / ld_mul   what E and the row strides must be multiples of in this operand format (fp32 rows: 4 / 4, bf16 rows: 16 / 8)
//   kern             the entry's score kernel at (WQ, KL) = (2, 16) (2, 64) (1, 16) (1, 128): the wide tile where query_rows_per_block says so, the short
//                    list for K <= 16
// The plain entries (ITEMS == false) pass null g_item / q_skip / items and distinct = 0; nothing reads them.  The entries by subset (SELECT, search_select.hip)
// add g_allow / g_group / q_group, each of which may be null; the groups are given together or not at all.
template <class OP, bool ITEMS, bool SELECT = false, class KERN>
int search_host(const char* name, int e_mul, int ld_mul, KERN* const (&kern)[4], const typename OP::elem* q, int64_t ld_q, const typename OP::elem* g,
                int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base, const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals,
                int64_t* idx, int32_t* items, void* workspace, void* stream, const uint32_t* g_allow = nullptr, const int32_t* g_group = nullptr,
                const int32_t* q_group = nullptr) {
    static_assert(ITEMS || !SELECT, "the selection by subset extends the selection by item");
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
    if constexpr (ITEMS) {
        SC_CHECK_ARG(g_item, "%s: null g_item (an int32 item code per gallery row is required)", name);
        SC_CHECK_ARG(items, "%s: null items", name);
    }
    if constexpr (SELECT)
        SC_CHECK_ARG((g_group == nullptr) == (q_group == nullptr), "%s: g_group and q_group are given together or not at all (%s is null)", name,
                     g_group ? "q_group" : "g_group");
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    SC_CHECK_ARG(S == 1 || workspace, "%s: %d splits need a workspace (%s)", name, S, ITEMS ? "sc_search_items_workspace_bytes" : "sc_search_workspace_bytes");
    const int per = (int)((N + S - 1) / S);
    int64_t* wi = (int64_t*)workspace;                       // [Q][S][K] i64, then [Q][S][K] f32 and, by item, [Q][S][K] i32
    float* wv = (float*)(wi + (int64_t)Q * S * K);
    int32_t* wc = (int32_t*)(wv + (int64_t)Q * S * K);
    float* ov = S == 1 ? vals : wv;
    int64_t* oi = S == 1 ? idx : wi;
    const int bq = query_rows_per_block(Q, K);
    const dim3 grid((unsigned)((Q + bq - 1) / bq), (unsigned)S);
    KERN* const k = kern[(bq == 128 ? 0 : 2) + (K <= 16 ? 0 : 1)];
    if constexpr (SELECT)
        hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, q, ld_q, g, ld_g, Q, (int)N, E, K, per, S, idx_base, g_item, q_skip, distinct, ov, oi,
                           S == 1 ? items : wc, g_allow, g_group, q_group);
    else if constexpr (ITEMS)
        hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, q, ld_q, g, ld_g, Q, (int)N, E, K, per, S, idx_base, g_item, q_skip, distinct, ov, oi,
                           S == 1 ? items : wc);
    else
        hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, q, ld_q, g, ld_g, Q, (int)N, E, K, per, S, idx_base, ov, oi);
    SC_CHECK_LAUNCH();
    if (S == 1) return 0;
    if constexpr (ITEMS) return sc_topk_merge_items(wv, wi, wc, Q, S * K, K, distinct, vals, idx, items, stream);
    else return sc_topk_merge(wv, wi, Q, S * K, K, vals, idx, stream);
}

}  // namespace search_core
