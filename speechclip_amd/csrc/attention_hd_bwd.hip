// Fused attention backward for head_dim 64 / 96 / 128 (sc_attention_hd_bwd), gfx950: the backward of sc_attention_hd_fwd, addressed exactly as it addresses
// its operands (element (b, t, h, e) at b*bs + t*rs + h*head_dim + e), for the full-row layers of a parallel branch deeper than one layer (Tq == Tk) and
// for the CLS query of its last layer (Tq == 1).  Structure of attention_bwd.hip with the head dim as a template parameter.  Three kernels:
//   attn_hd_bwd_stats_kernel  per (b, h, query): lse = log2 sum_k exp2(s_k) (s in log2 units) and delta = dO . O -> the fp32 workspace [2][B*H][Tq]
//                             (with dropout, delta is the same number taken before O's rounding: sum_k P_dropped dP, see the kernel)
//   attn_hd_bwd_dkv_kernel    key-tile-stationary sweep over the query tiles:  dV^T += dO^T P_dropped,  dK^T += Q^T dS
//   attn_hd_bwd_dq_kernel     query-tile-stationary sweep over the key tiles:  dQ^T += K^T dS^T
// S = Q K^T and dP = dO V^T are recomputed on v_mfma_f32_16x16x32_bf16 in both sweeps (HD / 32 k-steps each); the softmax arithmetic is fp32 in registers;
// nothing of size Tq x Tk reaches memory.  Every output element is produced by exactly one wave in a fixed order (no atomics): bitwise reproducible.
// The streamed 64-row tiles are staged row-major in LDS and read twice: row-wise (ds_read_b128, the product that contracts along the head dim) and through
// ds_read_b64_tr_b16 (the product that contracts along the tile's ROW index: its 4 x 16 blocks deliver rows 4g .. 4g+3 to lane group g, the order in which
// the 16x16 accumulator of S / dP holds them, so P and dS go from the accumulators straight into the next MFMA's operand registers).
// LDS row pitch = HD + 16 elements = 8 * odd dwords for 64 / 96 / 128 (40, 56, 72): the 8 rows that one 32-lane half of a transposed read touches start
// 8 banks apart (each covers 8), and the 16 rows of one ds_read_b128 lane group -- rows r and r + 8 fall on the same even 16-byte slot, and exactly one of
// the two belongs to the lane group's g = 1 lanes, which read 16 bytes further on -- cover the 16 slots of the 256-byte bank row once each.
// Rows that take no part are zeroed ON THEIR WAY INTO LDS (keys >= klens[b] of the K / V tiles, queries >= klens[b] of the Q / dO tiles): a zero P / dS
// times whatever such a row holds must add exactly 0, so there is no finiteness precondition on them (the forward zeroes V the same way).
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;     // (HIP's uint4 struct kept attention_hd.hip's prefetch registers in scratch)

constexpr int TILE = 64;       // streamed rows per tile; rows a block owns (16 per wave)

template <int HD>
struct BwdTile {
    static constexpr int LDR = HD + 16;                 // LDS row pitch (elements)
    static constexpr int CH = HD / 8;                   // 16-byte chunks per row
    static constexpr int NLD = TILE * CH / 256;         // chunks per thread per operand and tile
    static constexpr int NC = HD / 32;                  // 32-dim k-steps of S / dP
    static constexpr int ND = HD / 16;                  // 16-dim blocks of the dQ / dK / dV accumulators
    static_assert(HD % 32 == 0 && (TILE * CH) % 256 == 0 && (LDR / 2) % 16 == 8, "tile geometry");
};

// rows k0 .. k0+3 (this lane group's) x 16 columns of a row-major LDS image, column (lane & 15) delivered to the lane
__device__ __forceinline__ s16x4_t lds_tr(const bf16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}
// MFMA operand with k-slots 0-3 = rows r0 + 4g .. + 3 and 4-7 = rows r0 + 16 + 4g .. + 3 of the image (column d0 + (lane & 15))
template <int LDR>
__device__ __forceinline__ bf16x8_t lds_tr_frag(const bf16_t* img, int r0, int d0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const bf16_t* p = img + (r0 + 4 * g + (i >> 2)) * LDR + d0 + 4 * (i & 3);
    const s16x4_t lo = lds_tr(p), hi = lds_tr(p + 16 * LDR);
    const s16x8_t both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, both);
}
__device__ __forceinline__ bf16x8_t frag_of(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint4 u = make_uint4(a, b, c, d);
    return __builtin_bit_cast(bf16x8_t, u);
}
// sum / max over the four 16-lane groups of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) with the VALU lane swaps
__device__ __forceinline__ float groups_sum(float x) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float groups_max(float x) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

__device__ __forceinline__ int clamped_klen(const int32_t* klens, int b, int Tk) {
    const int kl = klens ? klens[b] : Tk;
    return kl < 0 ? 0 : (kl > Tk ? Tk : kl);
}

// rows r0 .. r0 + 63 (< T) of one head's column block <- 0
template <int HD>
__device__ __forceinline__ void zero_rows(bf16_t* base, int64_t rs, int r0, int T, int tid) {
    using TL = BwdTile<HD>;
#pragma unroll
    for (int i = 0; i < TL::NLD; ++i) {
        const int idx = i * 256 + tid, r = r0 + idx / TL::CH, c = idx % TL::CH;
        if (r < T) *(u32x4_t*)(base + (int64_t)r * rs + c * 8) = (u32x4_t){0u, 0u, 0u, 0u};
    }
}

// 64 rows of a [rows][head] operand (row t0 + r, clamped to the T rows there are; rows >= nvalid as zeros) -> registers -> the LDS image
template <int HD>
struct Stage {
    using TL = BwdTile<HD>;
    u32x4_t v[TL::NLD];
    __device__ __forceinline__ void load(const bf16_t* base, int64_t rs, int t0, int T, int nvalid, int tid) {
#pragma unroll
        for (int i = 0; i < TL::NLD; ++i) {
            const int idx = i * 256 + tid, r = t0 + idx / TL::CH, c = idx % TL::CH;
            const int rc = r < T ? r : T - 1;
            const u32x4_t w = *(const u32x4_t*)(base + (int64_t)rc * rs + c * 8);
            v[i] = r < nvalid ? w : (u32x4_t){0u, 0u, 0u, 0u};
        }
    }
    __device__ __forceinline__ void store(bf16_t* img, int tid) const {
#pragma unroll
        for (int i = 0; i < TL::NLD; ++i) {
            const int idx = i * 256 + tid;
            *(u32x4_t*)(img + (idx / TL::CH) * TL::LDR + (idx % TL::CH) * 8) = v[i];
        }
    }
};

// ---- statistics: one wave per 16 queries; K fragments are single 16-byte global loads (the product contracts along the head dimension)
// Without dropout delta = dO . O from the stored output.  With dropout the stored O = bf16(P_dropped V) no longer cancels against the recomputed
// sum_k P_dropped dP: with ONE kept key P_dropped = 1 / (1 - p), O = bf16(v / (1 - p)) is off v / (1 - p) by a bf16 ulp per element, and dS = P (m dP - delta),
// which is 0 analytically, keeps dO . (O - o) ~ sqrt(head_dim) 2^-9 |dO| |v|.  So the dropout form takes delta = sum_k P_dropped,k dP_k from the same MFMA
// products and the same mask the sweeps recompute (the online sum carried beside l), and the cancellation is exact in fp32.
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void attn_hd_bwd_stats_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                                const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO,
                                                                const int32_t* __restrict__ klens, int H, int Tq, int Tk, int64_t q_bs, int64_t q_rs,
                                                                int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs, float scale_log2e, uint32_t seed,
                                                                uint32_t thresh, float keep_scale, float* __restrict__ lse, float* __restrict__ delta) {
    constexpr int NC = BwdTile<HD>::NC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const int klen = clamped_klen(klens, b, Tk);
    const int i0 = (blockIdx.y * 4 + wave) * 16;
    if (i0 >= Tq) return;
    const int qi = lane & 15, g = lane >> 4;
    const int i = i0 + qi, ic = i < Tq ? i : Tq - 1;
    const bf16_t* qr = q + (int64_t)b * q_bs + (int64_t)ic * q_rs + h * HD + g * 8;
    const bf16_t* orow = O + (int64_t)b * o_bs + (int64_t)ic * o_rs + h * HD + g * 8;
    const bf16_t* drow = dO + (int64_t)b * o_bs + (int64_t)ic * o_rs + h * HD + g * 8;
    bf16x8_t qf[NC], dof[NC];
    float dpart = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        qf[c] = *(const bf16x8_t*)(qr + c * 32);
        if (DROP) {
            dof[c] = *(const bf16x8_t*)(drow + c * 32);
        } else {
            const u32x4_t du = *(const u32x4_t*)(drow + c * 32), ou = *(const u32x4_t*)(orow + c * 32);
#pragma unroll
            for (int e = 0; e < 4; ++e) dpart += lo2f(du[e]) * lo2f(ou[e]) + hi2f(du[e]) * hi2f(ou[e]);
        }
    }
    const uint32_t drow_id = DROP ? (uint32_t)(((int64_t)b * H + h) * Tk + ic) * (uint32_t)((Tk + 1) >> 1) : 0u;      // the forward's pair index base
    // lane-local online max / sum over this lane's keys (4 g + r of every 16-key block); the four groups are combined once at the end
    float m = -INFINITY, l = 0.f, da = 0.f;
    const int nkb = (klen + 15) / 16;
    const bf16_t* kb_ = k + (int64_t)b * kv_bs + h * HD + g * 8;
    const bf16_t* vb_ = v + (int64_t)b * kv_bs + h * HD + g * 8;
    for (int kb = 0; kb < nkb; ++kb) {
        int key = kb * 16 + qi;
        key = key < Tk ? key : Tk - 1;
        const bf16_t* kr = kb_ + (int64_t)key * kv_rs;
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(kr + c * 32), qf[c], s, 0, 0, 0);
        float pm[4] = {0.f, 0.f, 0.f, 0.f};      // m dP of this lane's keys (0 for a dropped key and for keys >= klen, whatever V holds there)
        if (DROP) {
            const bf16_t* vr = vb_ + (int64_t)key * kv_rs;
            f32x4_t pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(vr + c * 32), dof[c], pa, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const int kk = kb * 16 + 4 * g + r;      // even: registers r, r + 1 are one mask pair
                const uint32_t hb = hash_pair(seed, drow_id + ((uint32_t)kk >> 1));
                pm[r] = kk < klen && (hb & 0xffffu) >= thresh ? pa[r] * keep_scale : 0.f;
                pm[r + 1] = kk + 1 < klen && (hb >> 16) >= thresh ? pa[r + 1] * keep_scale : 0.f;
            }
        }
        float bm = m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (kb * 16 + 4 * g + r) < klen ? s[r] * scale_log2e : -INFINITY;
            bm = fmaxf(bm, s[r]);
        }
        if (bm > -INFINITY) {
            float ps = 0.f, pd = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[r] - bm);
                ps += e;
                pd += e * pm[r];
            }
            const float resc = __builtin_amdgcn_exp2f(m - bm);
            l = l * resc + ps;
            da = da * resc + pd;
            m = bm;
        }
    }
    const float mt = groups_max(m);
    const float lt = groups_sum(m > -INFINITY ? l * __builtin_amdgcn_exp2f(m - mt) : 0.f);
    const float dd = DROP ? groups_sum(m > -INFINITY ? da * __builtin_amdgcn_exp2f(m - mt) : 0.f) / lt : groups_sum(dpart);
    if (g == 0 && i < Tq) {
        const bool ok = i < klen && lt > 0.f;
        lse[(int64_t)z * Tq + i] = ok ? mt + __builtin_amdgcn_logf(lt) : 0.f;      // v_log_f32: log2
        delta[(int64_t)z * Tq + i] = ok ? dd : 0.f;
    }
}

// ---- dQ: a block owns 64 queries (16 per wave) of one (b, h) and walks the key tiles
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void attn_hd_bwd_dq_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                             const bf16_t* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
                                                             const int32_t* __restrict__ klens, int H, int Tq, int Tk, int64_t q_bs, int64_t q_rs,
                                                             int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs, float scale, float scale_log2e,
                                                             uint32_t seed, uint32_t thresh, float keep_scale, bf16_t* __restrict__ dq, int64_t dq_bs,
                                                             int64_t dq_rs) {
    using TL = BwdTile<HD>;
    constexpr int LDR = TL::LDR, NC = TL::NC, ND = TL::ND;
    __shared__ __attribute__((aligned(16))) bf16_t ks[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t vs[TILE * LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const int klen = clamped_klen(klens, b, Tk);
    const int nq = klen < Tq ? klen : Tq;                // queries that take part
    const int q0 = blockIdx.y * TILE;
    if (q0 >= Tq) return;
    bf16_t* dq_u = dq + (int64_t)b * dq_bs + h * HD;
    if (q0 >= nq) { zero_rows<HD>(dq_u, dq_rs, q0, Tq, tid); return; }
    const int qi = lane & 15, g = lane >> 4;
    const int i = q0 + wave * 16 + qi, ic = i < Tq ? i : Tq - 1;
    const bool q_ok = i < nq;
    const bf16_t* qr = q + (int64_t)b * q_bs + (int64_t)ic * q_rs + h * HD + g * 8;
    const bf16_t* drow = dO + (int64_t)b * o_bs + (int64_t)ic * o_rs + h * HD + g * 8;
    bf16x8_t qf[NC], dof[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        qf[c] = *(const bf16x8_t*)(qr + c * 32);
        dof[c] = *(const bf16x8_t*)(drow + c * 32);
    }
    const float lse_i = lse[(int64_t)z * Tq + ic], del_i = delta[(int64_t)z * Tq + ic];
    const uint32_t drow_id = DROP ? (uint32_t)(((int64_t)b * H + h) * Tk + ic) * (uint32_t)((Tk + 1) >> 1) : 0u;      // the forward's pair index base
    const bf16_t* k_u = k + (int64_t)b * kv_bs + h * HD;
    const bf16_t* v_u = v + (int64_t)b * kv_bs + h * HD;
    f32x4_t acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int nt = (klen + TILE - 1) / TILE;
    Stage<HD> sk, sv;
    sk.load(k_u, kv_rs, 0, Tk, klen, tid);
    sv.load(v_u, kv_rs, 0, Tk, klen, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                     // every wave is done with the previous tile
        sk.store(ks, tid);
        sv.store(vs, tid);
        __syncthreads();
        if (t + 1 < nt) {
            sk.load(k_u, kv_rs, (t + 1) * TILE, Tk, klen, tid);
            sv.load(v_u, kv_rs, (t + 1) * TILE, Tk, klen, tid);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {        // 32 keys: one k-step of dQ^T += K^T dS^T
            uint32_t dsp[4];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int kb = 2 * s + sub;
                f32x4_t sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(ks + (kb * 16 + qi) * LDR + c * 32 + g * 8), qf[c], sa, 0, 0, 0);
                    pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(vs + (kb * 16 + qi) * LDR + c * 32 + g * 8), dof[c], pa, 0, 0, 0);
                }
                float ds[4];
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const int key = t * TILE + kb * 16 + 4 * g + r;      // even: registers r, r + 1 are one mask pair
                    float m0 = 1.f, m1 = 1.f;
                    if (DROP) {
                        const uint32_t hb = hash_pair(seed, drow_id + ((uint32_t)key >> 1));
                        m0 = (hb & 0xffffu) >= thresh ? keep_scale : 0.f;
                        m1 = (hb >> 16) >= thresh ? keep_scale : 0.f;
                    }
                    const bool ok0 = q_ok && key < klen, ok1 = q_ok && key + 1 < klen;
                    const float p0 = __builtin_amdgcn_exp2f(sa[r] * scale_log2e - lse_i), p1 = __builtin_amdgcn_exp2f(sa[r + 1] * scale_log2e - lse_i);
                    ds[r] = ok0 ? p0 * (pa[r] * m0 - del_i) * scale : 0.f;
                    ds[r + 1] = ok1 ? p1 * (pa[r + 1] * m1 - del_i) * scale : 0.f;
                }
                dsp[2 * sub] = pack2bf(ds[0], ds[1]);
                dsp[2 * sub + 1] = pack2bf(ds[2], ds[3]);
            }
            const bf16x8_t dsf = frag_of(dsp[0], dsp[1], dsp[2], dsp[3]);
#pragma unroll
            for (int d = 0; d < ND; ++d)
                acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag<LDR>(ks, s * 32, d * 16, lane), dsf, acc[d], 0, 0, 0);
        }
    }
    if (i < Tq) {       // lane: query qi, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < ND; ++d)
            *(uint2*)(dq_u + (int64_t)i * dq_rs + d * 16 + 4 * g) = make_uint2(pack2bf(acc[d][0], acc[d][1]), pack2bf(acc[d][2], acc[d][3]));
    }
}

// ---- dK, dV: a block owns 64 keys (16 per wave) of one (b, h) and walks the query tiles
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void attn_hd_bwd_dkv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                              const bf16_t* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
                                                              const int32_t* __restrict__ klens, int H, int Tq, int Tk, int64_t q_bs, int64_t q_rs,
                                                              int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs, float scale, float scale_log2e,
                                                              uint32_t seed, uint32_t thresh, float keep_scale, bf16_t* __restrict__ dk,
                                                              bf16_t* __restrict__ dv, int64_t dkv_bs, int64_t dkv_rs) {
    using TL = BwdTile<HD>;
    constexpr int LDR = TL::LDR, NC = TL::NC, ND = TL::ND;
    __shared__ __attribute__((aligned(16))) bf16_t qs[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t os[TILE * LDR];
    __shared__ __attribute__((aligned(16))) float st[2 * TILE];      // lse | delta of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const int klen = clamped_klen(klens, b, Tk);
    const int nq = klen < Tq ? klen : Tq;                // queries that take part
    const int k0 = blockIdx.y * TILE;
    if (k0 >= Tk) return;
    bf16_t* dk_u = dk + (int64_t)b * dkv_bs + h * HD;
    bf16_t* dv_u = dv + (int64_t)b * dkv_bs + h * HD;
    if (k0 >= klen) { zero_rows<HD>(dk_u, dkv_rs, k0, Tk, tid); zero_rows<HD>(dv_u, dkv_rs, k0, Tk, tid); return; }
    const int ki = lane & 15, g = lane >> 4;
    const int j = k0 + wave * 16 + ki, jc = j < Tk ? j : Tk - 1;
    const bool k_ok = j < klen;
    const bf16_t* kr = k + (int64_t)b * kv_bs + (int64_t)jc * kv_rs + h * HD + g * 8;
    const bf16_t* vr = v + (int64_t)b * kv_bs + (int64_t)jc * kv_rs + h * HD + g * 8;
    bf16x8_t kf[NC], vf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        kf[c] = *(const bf16x8_t*)(kr + c * 32);
        vf[c] = *(const bf16x8_t*)(vr + c * 32);
    }
    const uint32_t kpair = (uint32_t)jc >> 1, drop_pairs = (uint32_t)((Tk + 1) >> 1);
    const bool khigh = (jc & 1) != 0;
    const uint32_t drow0 = (uint32_t)(((int64_t)b * H + h) * Tk);      // the forward's mask row of query 0
    const bf16_t* q_u = q + (int64_t)b * q_bs + h * HD;
    const bf16_t* o_u = dO + (int64_t)b * o_bs + h * HD;
    const float* lse_u = lse + (int64_t)z * Tq;
    const float* del_u = delta + (int64_t)z * Tq;
    f32x4_t ak[ND], av[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { ak[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; av[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
    const int nt = (nq + TILE - 1) / TILE;
    Stage<HD> sq, so;
    float sreg = 0.f;
    auto load_stats = [&](int t0) {
        if (tid < 2 * TILE) {
            int r = t0 + (tid & (TILE - 1));
            r = r < Tq ? r : Tq - 1;
            sreg = (tid < TILE ? lse_u : del_u)[r];
        }
    };
    sq.load(q_u, q_rs, 0, Tq, nq, tid);
    so.load(o_u, o_rs, 0, Tq, nq, tid);
    load_stats(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        sq.store(qs, tid);
        so.store(os, tid);
        if (tid < 2 * TILE) st[tid] = sreg;
        __syncthreads();
        if (t + 1 < nt) {
            sq.load(q_u, q_rs, (t + 1) * TILE, Tq, nq, tid);
            so.load(o_u, o_rs, (t + 1) * TILE, Tq, nq, tid);
            load_stats((t + 1) * TILE);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {        // 32 queries: one k-step of dV^T += dO^T P and dK^T += Q^T dS
            uint32_t pp[4], dsp[4];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int qb = 2 * s + sub;
                f32x4_t sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {     // first operand = query rows: the lane holds key ki, queries 4 g + r of the block
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(qs + (qb * 16 + ki) * LDR + c * 32 + g * 8), kf[c], sa, 0, 0, 0);
                    pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(os + (qb * 16 + ki) * LDR + c * 32 + g * 8), vf[c], pa, 0, 0, 0);
                }
                const f32x4_t ls = *(const f32x4_t*)(st + qb * 16 + 4 * g), de = *(const f32x4_t*)(st + TILE + qb * 16 + 4 * g);
                float pv[4], ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int query = t * TILE + qb * 16 + 4 * g + r;
                    float m = 1.f;
                    if (DROP) {
                        const uint32_t hb = hash_pair(seed, (drow0 + (uint32_t)query) * drop_pairs + kpair);
                        m = (khigh ? (hb >> 16) : (hb & 0xffffu)) >= thresh ? keep_scale : 0.f;
                    }
                    const bool ok = k_ok && query < nq;
                    const float p = __builtin_amdgcn_exp2f(sa[r] * scale_log2e - ls[r]);
                    pv[r] = ok ? p * m : 0.f;
                    ds[r] = ok ? p * (pa[r] * m - de[r]) * scale : 0.f;
                }
                pp[2 * sub] = pack2bf(pv[0], pv[1]);
                pp[2 * sub + 1] = pack2bf(pv[2], pv[3]);
                dsp[2 * sub] = pack2bf(ds[0], ds[1]);
                dsp[2 * sub + 1] = pack2bf(ds[2], ds[3]);
            }
            const bf16x8_t pf = frag_of(pp[0], pp[1], pp[2], pp[3]), dsf = frag_of(dsp[0], dsp[1], dsp[2], dsp[3]);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                av[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag<LDR>(os, s * 32, d * 16, lane), pf, av[d], 0, 0, 0);
                ak[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag<LDR>(qs, s * 32, d * 16, lane), dsf, ak[d], 0, 0, 0);
            }
        }
    }
    if (j < Tk) {       // lane: key ki, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            *(uint2*)(dk_u + (int64_t)j * dkv_rs + d * 16 + 4 * g) = make_uint2(pack2bf(ak[d][0], ak[d][1]), pack2bf(ak[d][2], ak[d][3]));
            *(uint2*)(dv_u + (int64_t)j * dkv_rs + d * 16 + 4 * g) = make_uint2(pack2bf(av[d][0], av[d][1]), pack2bf(av[d][2], av[d][3]));
        }
    }
}

template <int HD>
void launch_all(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* O, const bf16_t* dO, const int32_t* klens, int B, int H, int Tq, int Tk,
                int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs, bf16_t* dq, int64_t dq_bs, int64_t dq_rs, bf16_t* dk,
                bf16_t* dv, int64_t dkv_bs, int64_t dkv_rs, float scale, float drop_p, uint32_t seed, float* lse, float* delta, hipStream_t s) {
    const float sl2 = scale * 1.44269504088896341f;
    const uint32_t th = drop_thresh16(drop_p);
    const float ks = 1.0f / (1.0f - drop_p);
    const dim3 block(256), gq((unsigned)(B * H), (unsigned)((Tq + TILE - 1) / TILE)), gk((unsigned)(B * H), (unsigned)((Tk + TILE - 1) / TILE));
#define SC_HD_BWD_LAUNCH(DR)                                                                                                                              \
    do {                                                                                                                                                  \
        hipLaunchKernelGGL((attn_hd_bwd_stats_kernel<HD, DR>), gq, block, 0, s, q, k, v, O, dO, klens, H, Tq, Tk, q_bs, q_rs, kv_bs, kv_rs, o_bs, o_rs,  \
                           sl2, seed, th, ks, lse, delta);                                                                                                \
        hipLaunchKernelGGL((attn_hd_bwd_dkv_kernel<HD, DR>), gk, block, 0, s, q, k, v, dO, (const float*)lse, (const float*)delta, klens, H, Tq, Tk, q_bs, \
                           q_rs, kv_bs, kv_rs, o_bs, o_rs, scale, sl2, seed, th, ks, dk, dv, dkv_bs, dkv_rs);                                             \
        hipLaunchKernelGGL((attn_hd_bwd_dq_kernel<HD, DR>), gq, block, 0, s, q, k, v, dO, (const float*)lse, (const float*)delta, klens, H, Tq, Tk, q_bs,  \
                           q_rs, kv_bs, kv_rs, o_bs, o_rs, scale, sl2, seed, th, ks, dq, dq_bs, dq_rs);                                                   \
    } while (0)
    if (th) SC_HD_BWD_LAUNCH(true);
    else SC_HD_BWD_LAUNCH(false);
#undef SC_HD_BWD_LAUNCH
}

}  // namespace

extern "C" int64_t sc_attention_hd_bwd_workspace_bytes(int B, int H, int Tq) {
    return B > 0 && H > 0 && Tq > 0 ? 2 * (int64_t)B * H * Tq * (int64_t)sizeof(float) : 0;
}

extern "C" int sc_attention_hd_bwd(const void* q, const void* k, const void* v, const void* O, const void* dO, const int32_t* klens, int B, int H, int Tq,
                                   int Tk, int head_dim, int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs, void* dq,
                                   int64_t dq_bs, int64_t dq_rs, void* dk, void* dv, int64_t dkv_bs, int64_t dkv_rs, float scale, float drop_p, uint32_t seed,
                                   void* workspace, void* stream) {
    SC_CHECK_ARG(head_dim == 64 || head_dim == 96 || head_dim == 128, "sc_attention_hd_bwd: head_dim=%d unsupported (64, 96, 128)", head_dim);
    SC_CHECK_ARG(B >= 0 && H >= 1 && Tq >= 0 && Tk >= 0 && (int64_t)B * H < 0x7fffffffLL, "sc_attention_hd_bwd: bad sizes B=%d H=%d Tq=%d Tk=%d", B, H, Tq, Tk);
    SC_CHECK_ARG(Tq == Tk || Tq == 1, "sc_attention_hd_bwd: Tq=%d Tk=%d unsupported (Tq == Tk, or Tq == 1)", Tq, Tk);
    SC_CHECK_ARG(q_bs % 8 == 0 && q_rs % 8 == 0 && kv_bs % 8 == 0 && kv_rs % 8 == 0 && o_bs % 8 == 0 && o_rs % 8 == 0 && dq_bs % 8 == 0 && dq_rs % 8 == 0 &&
                     dkv_bs % 8 == 0 && dkv_rs % 8 == 0,
                 "sc_attention_hd_bwd: strides must be multiples of 8 elements (16-byte rows)");
    SC_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "sc_attention_hd_bwd: drop_p=%f must be in [0, 1)", (double)drop_p);
    SC_CHECK_ARG(drop_p == 0.f || (int64_t)B * H * Tk * ((Tk + 1) / 2) < 0xffffffffLL, "sc_attention_hd_bwd: B*H*Tk*Tk/2 must fit 32 bits (dropout pair index)");
    if (B == 0 || Tk == 0) return 0;
    SC_CHECK_ARG(q && k && v && O && dO && dq && dk && dv && workspace, "sc_attention_hd_bwd: null operand");
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)O | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)workspace) & 15) == 0,
                 "sc_attention_hd_bwd: misaligned pointers");
    SC_CHECK_ARG((Tk + TILE - 1) / TILE <= 65535, "sc_attention_hd_bwd: Tk=%d too long", Tk);
    float* lse = (float*)workspace;
    float* delta = lse + (int64_t)B * H * Tq;
#define SC_HD_BWD_ARGS                                                                                                                              \
    (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)O, (const bf16_t*)dO, klens, B, H, Tq, Tk, q_bs, q_rs, kv_bs, kv_rs, o_bs, o_rs, \
        (bf16_t*)dq, dq_bs, dq_rs, (bf16_t*)dk, (bf16_t*)dv, dkv_bs, dkv_rs, scale, drop_p, seed, lse, delta, (hipStream_t)stream
    if (head_dim == 64) launch_all<64>(SC_HD_BWD_ARGS);
    else if (head_dim == 96) launch_all<96>(SC_HD_BWD_ARGS);
    else launch_all<128>(SC_HD_BWD_ARGS);
#undef SC_HD_BWD_ARGS
    SC_CHECK_LAUNCH();
    return 0;
}
