// Gallery search, the two operand formats of search_core.h's block bodies ("what an operand format supplies"): F32Rows is the loading, staging and product of
// search.hip (fp32 rows, sc_search_topk), Bf16Rows that of search_bf16.hip (bf16 rows, sc_search_topk_bf16); search_items.hip runs both under the id-aware
// selection (sc_search_items, sc_search_items_bf16).  One definition each, so that the three files form the same scores bit for bit.
#pragma once
#include "search_core.h"

namespace search_core {

// fp32 rows on v_mfma_f32_32x32x2_f32 (search_core.h: what an operand format supplies)
struct F32Rows {
    using elem = float;
    static constexpr int LDT = KC + 4;   // LDS row stride in floats: 68 r mod 64 = 4 r walks all sixteen 4-bank slots over 16 rows: ds_read_b128 is conflict-free
    struct unit { f32x4_t x0, x1; };
    // 8 consecutive floats of one row from e (a multiple of 8), only those below E (E % 4 == 0: whole 16-byte halves); an absent row reads nothing
    static __device__ __forceinline__ void load(const float* __restrict__ row, bool row_ok, int e, int E, unit& u) {
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        u.x0 = row_ok && e < E ? *(const f32x4_t*)(row + e) : z;
        u.x1 = row_ok && e + 4 < E ? *(const f32x4_t*)(row + e + 4) : z;
    }
    // The 32x32x2 MFMA takes k = 2t from lanes 0..31 and k = 2t + 1 from lanes 32..63, so a group of 8 is stored even elements first: lane half h then reads
    // its four k-steps (e = 2t + h, t = 0..3) with one ds_read_b128 at offset 4h.
    static __device__ __forceinline__ void store(float* dst, const unit& u) {
        *(f32x4_t*)dst = f32x4_t{u.x0[0], u.x0[2], u.x1[0], u.x1[2]};
        *(f32x4_t*)(dst + 4) = f32x4_t{u.x0[1], u.x0[3], u.x1[1], u.x1[3]};
    }
    // rq / rg: this lane's row of the wave's first query / gallery tile in the stage images; e0: the stage's first element
    template <int WQ>
    static __device__ __forceinline__ void stage(f32x16_t (&acc)[WQ][2], const float* rq, const float* rg, int h, int e0, int E) {
        const float* aq = rq + 4 * h;
        const float* bg = rg + 4 * h;
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
};

// bf16 rows on v_mfma_f32_32x32x16_bf16: lane (r, h) supplies A[row r][k = 8 h + 0..7] and B[k = 8 h + 0..7][column r] of a 16-wide step
struct Bf16Rows {
    using elem = bf16_t;
    // LDS row stride in elements: 72 = 144 bytes = 9 sixteen-byte slots.  A ds_read_b128 is served in groups of 16 lanes whose rows cover every residue mod 16
    // ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, the same for the upper half), and 9 r mod 16 is a bijection of them: sixteen distinct slots, conflict-free.
    static constexpr int LDT = KC + 8;
    struct unit { bf16x8_t x; };
    // 8 consecutive elements of one row from e (a multiple of 8; E % 16 == 0: whole 16-byte units); an absent row reads nothing
    static __device__ __forceinline__ void load(const bf16_t* __restrict__ row, bool row_ok, int e, int E, unit& u) {
        const bf16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
        u.x = row_ok && e < E ? *(const bf16x8_t*)(row + e) : z;
    }
    static __device__ __forceinline__ void store(bf16_t* dst, const unit& u) { *(bf16x8_t*)dst = u.x; }
    // rq / rg: this lane's row of the wave's first query / gallery tile in the stage images; e0: the stage's first element
    template <int WQ>
    static __device__ __forceinline__ void stage(f32x16_t (&acc)[WQ][2], const bf16_t* rq, const bf16_t* rg, int h, int e0, int E) {
        const bf16_t* aq = rq + 8 * h;
        const bf16_t* bg = rg + 8 * h;
        if (e0 + KC <= E) {                              // a whole stage: straight-line code, the fragment reads run ahead of the MFMAs
            bf16x8_t a8[KC / 16][WQ], b8[KC / 16][2];
#pragma unroll
            for (int g16 = 0; g16 < KC / 16; ++g16) {
#pragma unroll
                for (int a = 0; a < WQ; ++a) a8[g16][a] = *(const bf16x8_t*)(aq + a * 32 * LDT + 16 * g16);
#pragma unroll
                for (int b = 0; b < 2; ++b) b8[g16][b] = *(const bf16x8_t*)(bg + b * 32 * LDT + 16 * g16);
            }
#pragma unroll
            for (int g16 = 0; g16 < KC / 16; ++g16)
#pragma unroll
                for (int a = 0; a < WQ; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8[g16][a], b8[g16][b], acc[a][b], 0, 0, 0);
        } else {                                         // the last stage of a row: E % 16 == 0, so only whole groups of 16, and none beyond E
#pragma unroll
            for (int g16 = 0; g16 < KC / 16; ++g16) {
                if (e0 + 16 * g16 < E) {
                    bf16x8_t a8[WQ], b8[2];
#pragma unroll
                    for (int a = 0; a < WQ; ++a) a8[a] = *(const bf16x8_t*)(aq + a * 32 * LDT + 16 * g16);
#pragma unroll
                    for (int b = 0; b < 2; ++b) b8[b] = *(const bf16x8_t*)(bg + b * 32 * LDT + 16 * g16);
#pragma unroll
                    for (int a = 0; a < WQ; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8[a], b8[b], acc[a][b], 0, 0, 0);
                }
            }
        }
    }
};

}  // namespace search_core
