// CLIP text tower on packed (padding-free) rows: the embedding kernel.  Caption b owns rows [row_off[b], row_off[b + 1]) -- SOT .. EOT, nothing
// behind the EOT: under the causal mask no later position can reach the EOT feature.  The attention over these rows is sc_attention_fwd_text
// (attention.hip: attn_fwd_kernel with row_off and the causal bit); GEMMs and LayerNorms take the packed rows as they are.
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

// One block per caption: out[row_off[b] + t] = tok[ids[b, t]] + pos[t], t < rows_b; float4 loads and stores, one fp32 add per element.
__global__ __launch_bounds__(256) void text_embed_packed_kernel(const int64_t* __restrict__ ids, int64_t ld_ids, const float* __restrict__ tok,
                                                                const float* __restrict__ pos, const int32_t* __restrict__ row_off,
                                                                float* __restrict__ out, int rows_cap, int V, int W4, int64_t total_rows) {
    const int b = blockIdx.x;
    const int64_t r0 = row_off[b];
    int rows = row_off[b + 1] - row_off[b];
    rows = rows < rows_cap ? rows : rows_cap;                  // never past the id row or the positional table
    if (r0 < 0 || r0 + rows > total_rows) return;              // a row_off that breaks its contract writes nothing
    const f32x4_t* tok4 = (const f32x4_t*)tok;
    const f32x4_t* pos4 = (const f32x4_t*)pos;
    f32x4_t* out4 = (f32x4_t*)out;
    const int n = rows * W4;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = i / W4, c = i - t * W4;
        int64_t id = ids[(int64_t)b * ld_ids + t];
        id = id < 0 ? 0 : (id >= V ? V - 1 : id);              // the wrapper refuses such ids; the kernel never reads outside the table
        out4[(r0 + t) * W4 + c] = tok4[id * W4 + c] + pos4[(int64_t)t * W4 + c];
    }
}

// ------------------------------------------------------------------------------------------------ short-row causal attention
// Captions are 10 to 20 rows long: attn_fwd_kernel gives a (caption, head) unit a 256-thread block of 128 query rows, this kernel gives it ONE wave (four units
// share a block, no unit waits for another beyond one barrier).  Per unit: V is transposed once into the wave's own LDS slice (V^T [64 d][keys], keys T .. next
// multiple of 32 zero-filled), then per 16-query block
//   S^T = K.Q^T  on v_mfma_f32_16x16x32_bf16, operands straight from global memory (A = 16 keys x 32 dims, B = 16 queries x 32 dims, two k-steps per key block):
//                the lane (query l & 15, g = l >> 4) holds keys 16 kb + 4 g + i of its query -- row maximum and sum are in-lane plus two cross-lane steps;
//   softmax      fp32 in registers over the whole key range (at most NKB x 16 keys: no K/V ring, no online rescale);
//   O^T += V^T.P^T  the exponentiated registers of key blocks 2p, 2p + 1 ARE the B fragment of k-step p (k-slot 8 g + j = key 32 p + 16 (j >> 2) + 4 g + (j & 3)),
//                the A fragment is two 8-byte reads of the V^T image at the same keys.
// Every output row is written once, no atomics.  NKB (key blocks of 16, even): 2 / 4 / 6 / 8 = captions of up to 32 / 64 / 96 / 128 rows.
template <int NKB>
__global__ __launch_bounds__(256) void text_attn_short_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                              bf16_t* __restrict__ out, const int32_t* __restrict__ row_off, int64_t ld_qkv, int64_t ld_out,
                                                              float scale_log2e, int n_units, int H, int64_t total_rows) {
    constexpr int KS = NKB * 16 + 8;                               // V^T row pitch in elements: (KS / 2) % 64 in {20, 36, 52, 4}: 16 d rows x 4 dwords on distinct banks
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 4 waves x [64 d][KS] bf16
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bf16_t* vt = (bf16_t*)smem + wave * (64 * KS);
    const int unit = blockIdx.x * 4 + wave;
    int T = 0;
    int64_t row_base = 0;
    int hoff = 0;
    if (unit < n_units) {
        const int b = unit / H;
        hoff = (unit - b * H) * 64;
        row_base = row_off[b];
        T = row_off[b + 1] - row_off[b];
        T = T > NKB * 16 ? NKB * 16 : T;                           // rows per caption <= Tmax is the caller's contract; never past the LDS image
        if (row_base < 0 || row_base + T > total_rows) T = 0;      // a row_off that breaks its contract computes nothing
    }
    if (T > 0) {
        const bf16_t* vb = v + row_base * ld_qkv + hoff;
        for (int i = lane; i < T * 8; i += 64) {                   // 16-byte chunk (i & 7) of key row i >> 3 -> column of V^T
            const int key = i >> 3, c = i & 7;
            const uint4 u = *(const uint4*)(vb + (int64_t)key * ld_qkv + c * 8);
            bf16_t* dst = vt + (c * 8) * KS + key;
            dst[0 * KS] = (bf16_t)(u.x & 0xffffu); dst[1 * KS] = (bf16_t)(u.x >> 16);
            dst[2 * KS] = (bf16_t)(u.y & 0xffffu); dst[3 * KS] = (bf16_t)(u.y >> 16);
            dst[4 * KS] = (bf16_t)(u.z & 0xffffu); dst[5 * KS] = (bf16_t)(u.z >> 16);
            dst[6 * KS] = (bf16_t)(u.w & 0xffffu); dst[7 * KS] = (bf16_t)(u.w >> 16);
        }
        const int Tpad = (T + 31) & ~31;                           // <= NKB * 16 (NKB even)
        for (int i = lane; i < (Tpad - T) * 64; i += 64) vt[(i & 63) * KS + T + (i >> 6)] = 0;
    }
    __syncthreads();                                               // the one barrier: every wave reaches it exactly once
    if (T <= 0) return;

    const int ql = lane & 15, g = lane >> 4;
    const bf16_t* qb_ = q + row_base * ld_qkv + hoff + g * 8;
    const bf16_t* kb_ = k + row_base * ld_qkv + hoff + g * 8;
    const int nqb = (T + 15) >> 4;
    for (int qb = 0; qb < nqb; ++qb) {
        const int qrow = qb * 16 + ql;
        const int qc = qrow < T ? qrow : T - 1;
        const bf16x8_t q0 = *(const bf16x8_t*)(qb_ + (int64_t)qc * ld_qkv);
        const bf16x8_t q1 = *(const bf16x8_t*)(qb_ + (int64_t)qc * ld_qkv + 32);
        const int ngrp = (qb >> 1) + 1;                            // 32-key groups up to the block's diagonal
        f32x4_t s[NKB];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            s[kb] = (f32x4_t){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (kb < 2 * ngrp) {
                const int kr = kb * 16 + ql;
                const int kc = kr < T ? kr : T - 1;                // rows past the caption are masked below: any row of the caption will do
                const bf16x8_t k0 = *(const bf16x8_t*)(kb_ + (int64_t)kc * ld_qkv);
                const bf16x8_t k1 = *(const bf16x8_t*)(kb_ + (int64_t)kc * ld_qkv + 32);
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, q0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, q1, acc, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kb * 16 + g * 4 + i;
                    const float t = (key <= qrow && key < T) ? acc[i] * scale_log2e : -INFINITY;
                    s[kb][i] = t;
                    mx = fmaxf(mx, t);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));                        // key 0 is visible to every query: finite
        float lsum = 0.f;
        uint32_t pk[NKB][2];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            float p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[i] = __builtin_amdgcn_exp2f(s[kb][i] - mx);      // exp2(-inf) = 0 on masked and skipped keys
                lsum += p[i];
            }
            pk[kb][0] = pack2bf(p[0], p[1]);
            pk[kb][1] = pack2bf(p[2], p[3]);
        }
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        f32x4_t o[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) o[db] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
#pragma unroll
        for (int p = 0; p < NKB / 2; ++p) {
            if (p < ngrp && p * 32 < T) {
                const u32x4_t pu = {pk[2 * p][0], pk[2 * p][1], pk[2 * p + 1][0], pk[2 * p + 1][1]};
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    const bf16_t* vr = vt + (db * 16 + ql) * KS + p * 32 + g * 4;
                    const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 16);
                    const u32x4_t vu = {lo.x, lo.y, hi.x, hi.y};
                    o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vu), __builtin_bit_cast(bf16x8_t, pu), o[db], 0, 0, 0);
                }
            }
        }
        if (qrow < T) {
            const float inv = 1.0f / lsum;
            bf16_t* orow = out + (row_base + qrow) * ld_out + hoff + g * 4;
#pragma unroll
            for (int db = 0; db < 4; ++db)
                *(uint2*)(orow + db * 16) = make_uint2(pack2bf(o[db][0] * inv, o[db][1] * inv), pack2bf(o[db][2] * inv, o[db][3] * inv));
        }
    }
}

}  // namespace

// The short-row form of sc_attention_fwd_text (attention.hip holds the entry and its argument checks).  Tmax <= SC_TEXT_ATTN_SHORT_MAX.
int text_attn_short_launch(const void* q, const void* k, const void* v, void* out, const int32_t* row_off, int B, int H, int Tmax, int64_t total_rows,
                           int64_t ld_qkv, int64_t ld_out, float scale, void* stream) {
    const int64_t n_units = (int64_t)B * H;
    SC_CHECK_ARG(Tmax >= 1 && Tmax <= 128, "sc_attention_fwd_text: short-row form takes Tmax in [1, 128], got %d", Tmax);
    SC_CHECK_ARG(n_units < 0x7fffffffLL, "sc_attention_fwd_text: grid too large");
    const dim3 grid((unsigned)((n_units + 3) / 4));
#define TEXT_ATTN_LAUNCH(NKB_)                                                                                                                         \
    do {                                                                                                                                               \
        const int lds = 4 * 64 * (NKB_ * 16 + 8) * 2;                                                                                                  \
        (void)hipFuncSetAttribute((const void*)text_attn_short_kernel<NKB_>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);                         \
        hipLaunchKernelGGL((text_attn_short_kernel<NKB_>), grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k,             \
                           (const bf16_t*)v, (bf16_t*)out, row_off, ld_qkv, ld_out, scale * 1.44269504088896341f, (int)n_units, H, total_rows);         \
    } while (0)
    if (Tmax <= 32) TEXT_ATTN_LAUNCH(2);
    else if (Tmax <= 64) TEXT_ATTN_LAUNCH(4);
    else if (Tmax <= 96) TEXT_ATTN_LAUNCH(6);
    else TEXT_ATTN_LAUNCH(8);
#undef TEXT_ATTN_LAUNCH
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int sc_text_embed_packed(const int64_t* ids, int64_t ld_ids, const float* tok, const float* pos, const int32_t* row_off, float* out,
                                    int B, int L, int V, int ctx, int W, int64_t total_rows, void* stream) {
    SC_CHECK_ARG(W > 0 && W % 4 == 0, "sc_text_embed_packed: W=%d must be a positive multiple of 4 (float4 rows)", W);
    SC_CHECK_ARG(ids != nullptr && tok != nullptr && pos != nullptr && row_off != nullptr && out != nullptr,
                 "sc_text_embed_packed: ids, tok, pos, row_off and out are required");
    SC_CHECK_ARG(L > 0 && L <= ctx, "sc_text_embed_packed: L=%d must be in [1, ctx=%d]", L, ctx);
    SC_CHECK_ARG(ld_ids >= L, "sc_text_embed_packed: ld_ids=%lld < L=%d", (long long)ld_ids, L);
    SC_CHECK_ARG(V > 0, "sc_text_embed_packed: V=%d", V);
    SC_CHECK_ARG((((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15) == 0, "sc_text_embed_packed: tok, pos and out must be 16-byte aligned");
    if (B <= 0 || total_rows <= 0) return 0;
    hipLaunchKernelGGL(text_embed_packed_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, ids, ld_ids, tok, pos, row_off, out, L, V, W / 4,
                       total_rows);
    SC_CHECK_LAUNCH();
    return 0;
}
