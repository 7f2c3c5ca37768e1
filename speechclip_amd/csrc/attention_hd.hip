// Flash-style attention forward for head_dim 64 / 96 / 128 (sc_attention_hd_fwd): the full-row layers of a parallel branch deeper than one
// layer (8 heads: head_dim 96 at d = 768, 128 at d = 1024), and the CLS-row attention of its last layer (Tq = 1, per-utterance query).
//  Block = 4 waves x 32 query rows of one (utterance, head); 64-key tiles.  S^T = K.Q^T with the operands swapped (mfma(K, Q), as attn_fwd_kernel),
//  so a lane holds 16 keys of ONE query: the row max is in-lane plus one v_permlane32_swap, and the exponentiated scores are already the B operand
//  of O^T += V^T.P^T.  K is stored row-major in LDS (pitch HD + 8: conflict-free ds_read_b128 fragments), V is transposed on its way into LDS
//  (V^T pitch 68: conflict-free ds_read_b64 fragments).  The next tile's K / V are loaded into registers while the current one is computed; tiles
//  past the utterance's key length are skipped, and V rows past it are written as zeros (a masked key contributes exactly 0, whatever the row holds).
//  Dropout on the probabilities uses attn_fwd_kernel's mask (hash_pair over key pairs of row (b*H + h)*Tk + query), so a CPU restatement of one
//  serves both.
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

constexpr int HD_KV = 64;       // keys per tile
constexpr int HD_ROWS = 128;    // query rows per block (4 waves x 32)
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;     // (HIP's uint4 struct kept the prefetch registers in scratch)

template <int HD>
struct HdTile {
    static constexpr int KP = HD + 8;                   // K tile row pitch (elements)
    static constexpr int VP = HD_KV + 4;                // V^T tile row pitch (elements): Vt[d][key]
    static constexpr int CH = HD / 8;                   // 16-byte chunks per K / V row
    static constexpr int NLD = HD_KV * CH / 256;        // chunks per thread per operand and tile
    static constexpr int LDS = (HD_KV * KP + HD * VP) * 2;
};

template <int HD, bool DROP, bool OUT_F32>
__global__ __launch_bounds__(256) void attn_hd_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          void* __restrict__ out, const int32_t* __restrict__ klens, int H, int Tq, int Tk,
                                                          int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs,
                                                          float scale_log2e, uint32_t drop_seed, uint32_t drop_thresh_, float drop_keep_scale) {
    using TL = HdTile<HD>;
    constexpr int NC = HD / 16;     // 16-dim k-steps of S^T = K.Q^T
    constexpr int ND = HD / 32;     // 32-dim row blocks of O^T
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* Ks = (bf16_t*)smem;                     // [64 keys][KP]
    bf16_t* Vt = Ks + HD_KV * TL::KP;               // [HD][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, ql = lane & 31;
    const int qblk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    int klen = klens ? klens[b] : Tk;
    klen = klen < 0 ? 0 : (klen > Tk ? Tk : klen);
    const int nkv = (klen + HD_KV - 1) / HD_KV;
    const int qrow = qblk * HD_ROWS + wave * 32 + ql;
    const int qrow_c = qrow < Tq ? qrow : Tq - 1;
    const bool active = qblk * HD_ROWS + wave * 32 < Tq;           // wave-uniform: a wave without valid rows only helps to load

    bf16x8_t qf[NC];                                                // B operand of S^T: col = query, k-slots = 8 dims
    const bf16_t* qp = q + (int64_t)b * q_bs + (int64_t)qrow_c * q_rs + h * HD + g * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = *(const bf16x8_t*)(qp + c * 16);

    f32x16_t o[ND];
#pragma unroll
    for (int db = 0; db < ND; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const uint32_t drop_pairs = (uint32_t)((Tk + 1) >> 1);
    const uint32_t drop_row = DROP ? (uint32_t)(((int64_t)b * H + h) * Tk + qrow_c) : 0u;

    const bf16_t* kbase = k + (int64_t)b * kv_bs + h * HD;
    const bf16_t* vbase = v + (int64_t)b * kv_bs + h * HD;
    u32x4_t kr[TL::NLD], vr[TL::NLD];
#define SC_HD_LOAD(tile)                                                                 \
    _Pragma("unroll") for (int i = 0; i < TL::NLD; ++i) {                                \
        const int idx = i * 256 + tid, key = idx & 63, c = idx >> 6;                     \
        int kk = (tile) * HD_KV + key;                                                   \
        kk = kk < Tk ? kk : Tk - 1;                                                      \
        kr[i] = *(const u32x4_t*)(kbase + (int64_t)kk * kv_rs + c * 8);                    \
        vr[i] = *(const u32x4_t*)(vbase + (int64_t)kk * kv_rs + c * 8);                    \
    }
    if (nkv > 0) { SC_HD_LOAD(0) }
    for (int j = 0; j < nkv; ++j) {
        const int kv0 = j * HD_KV;
        __syncthreads();                                            // every wave is done with tile j - 1
#pragma unroll
        for (int i = 0; i < TL::NLD; ++i) {
            const int idx = i * 256 + tid, key = idx & 63, c = idx >> 6;
            *(u32x4_t*)(Ks + key * TL::KP + c * 8) = kr[i];
            const bool valid = kv0 + key < klen;
            const u32x4_t w = valid ? vr[i] : (u32x4_t){0u, 0u, 0u, 0u};
            bf16_t* vt = Vt + c * 8 * TL::VP + key;
            vt[0 * TL::VP] = (bf16_t)(w.x & 0xffffu); vt[1 * TL::VP] = (bf16_t)(w.x >> 16);
            vt[2 * TL::VP] = (bf16_t)(w.y & 0xffffu); vt[3 * TL::VP] = (bf16_t)(w.y >> 16);
            vt[4 * TL::VP] = (bf16_t)(w.z & 0xffffu); vt[5 * TL::VP] = (bf16_t)(w.z >> 16);
            vt[6 * TL::VP] = (bf16_t)(w.w & 0xffffu); vt[7 * TL::VP] = (bf16_t)(w.w >> 16);
        }
        __syncthreads();
        if (j + 1 < nkv) { SC_HD_LOAD(j + 1) }                      // in flight while tile j is computed
#undef SC_HD_LOAD
        if (!active) continue;

        f32x16_t s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bf16x8_t kf = *(const bf16x8_t*)(Ks + (kb * 32 + ql) * TL::KP + c * 16 + g * 8);
                s[kb] = mfma_32x32x16<false>(kf, qf[c], s[kb]);
            }
        }
        // lane (g, ql), register r of key block kb: key kv0 + kb*32 + (r & 3) + 8*(r >> 2) + 4*g of query ql
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                const float t = key < klen ? s[kb][r] * scale_log2e : -INFINITY;
                s[kb][r] = t;
                mx = fmaxf(mx, t);
            }
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        const float m_new = fmaxf(m_run, mx);                      // finite: key kv0 < klen is in every processed tile
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new); // 0 on the first tile
        m_run = m_new;
        float psum = 0.f;
        uint32_t ppk[2][8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[kb][r] - m_new), p1 = __builtin_amdgcn_exp2f(s[kb][r + 1] - m_new);
                psum += p0;
                psum += p1;
                if (DROP) {
                    const uint32_t key = (uint32_t)(kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g);     // even
                    const uint32_t hbits = hash_pair(drop_seed, drop_row * drop_pairs + (key >> 1));
                    const float d0 = (hbits & 0xffffu) >= drop_thresh_ ? p0 * drop_keep_scale : 0.f;
                    const float d1 = (hbits >> 16) >= drop_thresh_ ? p1 * drop_keep_scale : 0.f;
                    ppk[kb][r >> 1] = pack2bf(d0, d1);
                } else {
                    ppk[kb][r >> 1] = pack2bf(p0, p1);
                }
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int db = 0; db < ND; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
        // O^T[d][q] += sum_k V^T[d][k] P^T[k][q]; k-slot s = 8g + e of the 16-key chunk (kb, hb) is key kb*32 + hb*16 + 4g + (e & 3) + 8*(e >> 2)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                const uint4 pu = make_uint4(ppk[kb][hb * 4 + 0], ppk[kb][hb * 4 + 1], ppk[kb][hb * 4 + 2], ppk[kb][hb * 4 + 3]);
                const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pu);
#pragma unroll
                for (int db = 0; db < ND; ++db) {
                    const bf16_t* vp = Vt + (db * 32 + ql) * TL::VP + kb * 32 + hb * 16 + 4 * g;
                    const uint2 lo = *(const uint2*)vp, hi = *(const uint2*)(vp + 8);
                    const bf16x8_t vf = __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
                    o[db] = mfma_32x32x16<false>(vf, pf, o[db]);
                }
            }
    }
    if (!active || qrow >= Tq) return;
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_run = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    // O^T register r of block db: d = db*32 + (r >> 2)*8 + 4g + (r & 3)
#pragma unroll
    for (int db = 0; db < ND; ++db)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int d = h * HD + db * 32 + r4 * 8 + 4 * g;
            const float a0 = o[db][4 * r4] * inv, a1 = o[db][4 * r4 + 1] * inv, a2 = o[db][4 * r4 + 2] * inv, a3 = o[db][4 * r4 + 3] * inv;
            const int64_t off = (int64_t)b * o_bs + (int64_t)qrow * o_rs + d;
            if (OUT_F32) *(f32x4_t*)((float*)out + off) = (f32x4_t){a0, a1, a2, a3};
            else *(uint2*)((bf16_t*)out + off) = make_uint2(pack2bf(a0, a1), pack2bf(a2, a3));
        }
}

}  // namespace

extern "C" int sc_attention_hd_fwd(const void* q, const void* k, const void* v, void* out, const int32_t* klens, int B, int H, int Tq, int Tk,
                                   int head_dim, int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs,
                                   float scale, float drop_p, uint32_t seed, int flags, void* stream) {
    const bool f32 = (flags & SC_ATTN_HD_OUT_F32) != 0;
    SC_CHECK_ARG((flags & ~SC_ATTN_HD_OUT_F32) == 0, "sc_attention_hd_fwd: unknown flag bits 0x%x", flags);
    SC_CHECK_ARG(head_dim == 64 || head_dim == 96 || head_dim == 128, "sc_attention_hd_fwd: head_dim=%d unsupported (64, 96, 128)", head_dim);
    SC_CHECK_ARG(B >= 0 && H >= 1 && B <= 65535 && H <= 65535 && Tq >= 0 && Tk >= 1, "sc_attention_hd_fwd: bad sizes B=%d H=%d Tq=%d Tk=%d", B, H, Tq, Tk);
    SC_CHECK_ARG(q_bs % 8 == 0 && q_rs % 8 == 0 && kv_bs % 8 == 0 && kv_rs % 8 == 0,
                 "sc_attention_hd_fwd: q / kv strides must be multiples of 8 elements (16-byte rows)");
    SC_CHECK_ARG(o_bs % 4 == 0 && o_rs % 4 == 0, "sc_attention_hd_fwd: out strides must be multiples of 4 elements");
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "sc_attention_hd_fwd: misaligned pointers");
    SC_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "sc_attention_hd_fwd: drop_p=%f must be in [0, 1)", (double)drop_p);
    SC_CHECK_ARG(drop_p == 0.f || (int64_t)B * H * Tk * ((Tk + 1) / 2) < 0xffffffffLL, "sc_attention_hd_fwd: B*H*Tk*Tk/2 must fit 32 bits (dropout pair index)");
    if (B == 0 || Tq == 0) return 0;
    const uint32_t th = drop_thresh16(drop_p);
    const float ks = 1.0f / (1.0f - drop_p);
    const dim3 grid((unsigned)((Tq + HD_ROWS - 1) / HD_ROWS), (unsigned)H, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
#define SC_HD_LAUNCH(HD_, DR_, F32_)                                                                                                        \
    do {                                                                                                                                    \
        constexpr int lds_ = HdTile<HD_>::LDS;                                                                                              \
        hipLaunchKernelGGL((attn_hd_fwd_kernel<HD_, DR_, F32_>), grid, dim3(256), lds_, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, \
                           out, klens, H, Tq, Tk, q_bs, q_rs, kv_bs, kv_rs, o_bs, o_rs, scale * 1.44269504088896341f, seed, th, ks);         \
    } while (0)
#define SC_HD_BY_MODE(HD_)                                      \
    do {                                                        \
        if (th) { if (f32) SC_HD_LAUNCH(HD_, true, true); else SC_HD_LAUNCH(HD_, true, false); }   \
        else { if (f32) SC_HD_LAUNCH(HD_, false, true); else SC_HD_LAUNCH(HD_, false, false); }    \
    } while (0)
    if (head_dim == 64) SC_HD_BY_MODE(64);
    else if (head_dim == 96) SC_HD_BY_MODE(96);
    else SC_HD_BY_MODE(128);
#undef SC_HD_BY_MODE
#undef SC_HD_LAUNCH
    SC_CHECK_LAUNCH();
    return 0;
}
