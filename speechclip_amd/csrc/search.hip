// Gallery search (include/speechclip_hip.h, "Gallery search"): the K nearest gallery rows of every query row WITHOUT the [Q, N] score image.
//   search_kernel      one block per (query tile, gallery split): fp32 scores on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per (i, j), E walked in
//                      ascending order, one accumulator chain, no split over E), kept in accumulators; every score is filtered against its row's current
//                      K-th entry, survivors go to a per-row LDS candidate buffer, and a full buffer is folded into the row's sorted top-K list by RANK in
//                      the total order (score descending, j ascending) -- the buffer may fill in any order, the list cannot tell.
//   topk_merge_kernel  L candidates per row -> the first K of that order (the partial lists of the splits, of gallery segments, of ranks).
// No global atomics; the LDS counters only hand out buffer slots.  Every output element is written once.
#include "common.h"
#include "../../include/speechclip_hip.h"
#include <limits.h>

namespace {

constexpr int BN = 128;          // gallery rows per tile
constexpr int KC = 64;           // elements of E per LDS stage (32 measured the same within 3 %: DESIGN.md 3.10)
constexpr int LDT = KC + 4;      // LDS row stride in floats: 68 r mod 64 = 4 r walks all sixteen 4-bank slots over 16 rows: ds_read_b128 is conflict-free
constexpr int NO_J = INT_MAX;    // empty list slot: (-inf, NO_J) comes after every real pair, a real -inf score included
constexpr int MIN_SPLIT_ROWS = 256;
constexpr int TARGET_BLOCKS = 512;

// (av, aj) strictly before (bv, bj) in (score descending, j ascending).  A NaN score is before nothing and nothing is before it.
__device__ __forceinline__ bool before(float av, int aj, float bv, int bj) { return av > bv || (av == bv && aj < bj); }

// 8 consecutive floats of one row from e (a multiple of 8), only those below E (E % 4 == 0: whole 16-byte halves); an absent row reads nothing
__device__ __forceinline__ void load8(const float* __restrict__ row, bool row_ok, int e, int E, f32x4_t& x0, f32x4_t& x1) {
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    x0 = row_ok && e < E ? *(const f32x4_t*)(row + e) : z;
    x1 = row_ok && e + 4 < E ? *(const f32x4_t*)(row + e + 4) : z;
}
// The 32x32x2 MFMA takes k = 2t from lanes 0..31 and k = 2t + 1 from lanes 32..63, so a group of 8 is stored even elements first: lane half h then reads
// its four k-steps (e = 2t + h, t = 0..3) with one ds_read_b128 at offset 4h.
__device__ __forceinline__ void store8(float* dst, const f32x4_t& x0, const f32x4_t& x1) {
    *(f32x4_t*)dst = f32x4_t{x0[0], x0[2], x1[0], x1[2]};
    *(f32x4_t*)(dst + 4) = f32x4_t{x0[1], x0[3], x1[1], x1[3]};
}

// WQ: 32-row query tiles per wave (block = 64 WQ query rows x 128 gallery rows, waves 2 x 2); KL: list capacity (K <= KL).
template <int WQ, int KL>
__global__ __launch_bounds__(256) void search_kernel(const float* __restrict__ q, int64_t ld_q, const float* __restrict__ g, int64_t ld_g, int Q, int N,
                                                      int E, int K, int per, int S, int64_t idx_base, float* __restrict__ out_v,
                                                      int64_t* __restrict__ out_i) {
    constexpr int BQ = 64 * WQ;
    constexpr int CB = WQ == 2 && KL == 64 ? 16 : 32;      // candidate buffer entries per row (the widest instantiation has 160 KB of LDS to fit)
    constexpr int NQU = 2 * WQ, NGU = 4;                   // a thread's load units per stage: (row, group of 8) of the [BQ][64] and [128][64] stage images
    __shared__ __attribute__((aligned(16))) float sQ[BQ * LDT];
    __shared__ __attribute__((aligned(16))) float sG[BN * LDT];
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
    f32x4_t pq[NQU][2], pg[NGU][2];
    auto prefetch = [&](int it) {
        const int tile = it / nchunk, e = (it - tile * nchunk) * KC + uc8;
#pragma unroll
        for (int u = 0; u < NQU; ++u) {
            const int row = q0 + urow + 32 * u;
            load8(q + (int64_t)row * ld_q, row < Q, e, E, pq[u][0], pq[u][1]);
        }
#pragma unroll
        for (int u = 0; u < NGU; ++u) {
            const int row = jbeg + tile * BN + urow + 32 * u;
            load8(g + (int64_t)row * ld_g, row < jend, e, E, pg[u][0], pg[u][1]);
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
            for (int u = 0; u < NQU; ++u) store8(sQ + (urow + 32 * u) * LDT + uc8, pq[u][0], pq[u][1]);
#pragma unroll
            for (int u = 0; u < NGU; ++u) store8(sG + (urow + 32 * u) * LDT + uc8, pg[u][0], pg[u][1]);
            __syncthreads();
            if (it + 1 < total) prefetch(it + 1);
            const int e0 = chunk * KC;
            const float* aq = sQ + (wq * 32 * WQ + r) * LDT + 4 * h;
            const float* bg = sG + (wg * 64 + r) * LDT + 4 * h;
            if (e0 + KC <= E) {                              // a whole stage: straight-line code, the fragment reads run ahead of the MFMAs
                f32x4_t a4[KC / 8][WQ], b4[KC / 8][2];
#pragma unroll
                for (int g8 = 0; g8 < KC / 8; ++g8) {
#pragma unroll
                    for (int a = 0; a < WQ; ++a) a4[g8][a] = *(const f32x4_t*)(aq + a * 32 * LDT + 8 * g8);
#pragma unroll
                    for (int b = 0; b < 2; ++b) b4[g8][b] = *(const f32x4_t*)(bg + b * 32 * LDT + 8 * g8);
                }
#pragma unroll
                for (int g8 = 0; g8 < KC / 8; ++g8)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int a = 0; a < WQ; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[g8][a][t], b4[g8][b][t], acc[a][b], 0, 0, 0);
            } else {                                         // the last stage of a row: E % 4 == 0, so a group of 8 has 4 k-steps or 2
#pragma unroll
                for (int g8 = 0; g8 < KC / 8; ++g8) {
                    if (e0 + 8 * g8 < E) {
                        f32x4_t a4[WQ], b4[2];
#pragma unroll
                        for (int a = 0; a < WQ; ++a) a4[a] = *(const f32x4_t*)(aq + a * 32 * LDT + 8 * g8);
#pragma unroll
                        for (int b = 0; b < 2; ++b) b4[b] = *(const f32x4_t*)(bg + b * 32 * LDT + 8 * g8);
                        const bool whole = e0 + 8 * g8 + 4 < E;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            if (t < 2 || whole) {
#pragma unroll
                                for (int a = 0; a < WQ; ++a)
#pragma unroll
                                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[a][t], b4[b][t], acc[a][b], 0, 0, 0);
                            }
                        }
                    }
                }
            }
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

int query_rows_per_block(int Q, int K) { return K <= 64 && Q > 64 ? 128 : 64; }

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
    SC_CHECK_ARG(E >= 4 && E <= 1024 && E % 4 == 0, "sc_search_topk: E=%d must be a multiple of 4 in [4, 1024]", E);
    SC_CHECK_ARG(ld_q >= E && ld_g >= E && ld_q % 4 == 0 && ld_g % 4 == 0, "sc_search_topk: ld_q=%lld / ld_g=%lld must be multiples of 4 and >= E=%d",
                 (long long)ld_q, (long long)ld_g, E);
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)g) & 15) == 0, "sc_search_topk: q and g must be 16-byte aligned");
    SC_CHECK_ARG(K >= 1 && K <= 128, "sc_search_topk: K=%d must be in [1, 128]", K);
    SC_CHECK_ARG(N < ((int64_t)1 << 31), "sc_search_topk: N=%lld must be below 2^31", (long long)N);
    SC_CHECK_ARG(K <= N, "sc_search_topk: K=%d exceeds N=%lld", K, (long long)N);
    SC_CHECK_ARG(n_split >= 0 && n_split <= 1024, "sc_search_topk: n_split=%d must be in [0, 1024] (0 = auto)", n_split);
    SC_CHECK_ARG(Q >= 0, "sc_search_topk: Q=%d is negative", Q);
    if (Q == 0) return 0;
    SC_CHECK_ARG(q && g && vals && idx, "sc_search_topk: null operand");
    const int S = n_split ? n_split : sc_search_splits(Q, N, K);
    SC_CHECK_ARG(S == 1 || workspace, "sc_search_topk: %d splits need a workspace (sc_search_workspace_bytes)", S);
    const int per = (int)((N + S - 1) / S);
    int64_t* wi = (int64_t*)workspace;                       // [Q][S][K] i64, then [Q][S][K] f32
    float* wv = (float*)(wi + (int64_t)Q * S * K);
    float* ov = S == 1 ? vals : wv;
    int64_t* oi = S == 1 ? idx : wi;
    const int bq = query_rows_per_block(Q, K);
    const dim3 grid((unsigned)((Q + bq - 1) / bq), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
#define SC_SEARCH_LAUNCH(WQ, KL) hipLaunchKernelGGL((search_kernel<WQ, KL>), grid, dim3(256), 0, st, q, ld_q, g, ld_g, Q, (int)N, E, K, per, S, idx_base, ov, oi)
    if (bq == 128) { if (K <= 16) SC_SEARCH_LAUNCH(2, 16); else SC_SEARCH_LAUNCH(2, 64); }
    else           { if (K <= 16) SC_SEARCH_LAUNCH(1, 16); else SC_SEARCH_LAUNCH(1, 128); }
#undef SC_SEARCH_LAUNCH
    SC_CHECK_LAUNCH();
    if (S > 1) return sc_topk_merge(wv, wi, Q, S * K, K, vals, idx, stream);
    return 0;
}
