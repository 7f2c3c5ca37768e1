// Fused attention backward, gfx950: ONE kernel set, templated on the head dim, behind two entries.
//   sc_attention_bwd_packed  head_dim 64, addressed as sc_attention_fwd_packed addresses its operands: bf16 rows, head h at column h*64, utterance b at
//                            rows row_off[b] .. (row_off == nullptr: b * Tmax), klens[b] valid keys (HuBERT fine-tuning)
//   sc_attention_hd_bwd      head_dim 64 / 96 / 128, addressed as sc_attention_hd_fwd addresses them (element (b, t, h, e) at b*bs + t*rs + h*head_dim + e),
//                            for the full-row layers of a parallel branch deeper than one layer (Tq == Tk) and the CLS query of its last layer (Tq == 1)
// Each entry checks its own arguments and fills one BwdArgs; where the two layouts differ -- how a block finds its (utterance, head) unit -- is stated once,
// in unit_of().  Three kernels:
//   attn_bwd_stats_kernel  per (b, h, query): lse = log2 sum_k exp2(s_k) (s in log2 units) and delta -> the fp32 workspace (delta = dO . O from the stored
//                          output, or the same number taken before O's rounding, sum_k P_dropped dP: see the kernel)
//   attn_bwd_dkv_kernel    key-tile-stationary sweep over the query tiles:  dV^T += dO^T P_dropped,  dK^T += Q^T dS
//   attn_bwd_dq_kernel     query-tile-stationary sweep over the key tiles:  dQ^T += K^T dS^T
// S = Q K^T and dP = dO V^T are recomputed on v_mfma_f32_16x16x32_bf16 in both sweeps (HD / 32 k-steps each); the softmax arithmetic is fp32 in registers;
// nothing of size Tq x Tk reaches memory.  Every output element is produced by exactly one wave in a fixed order (no atomics): bitwise reproducible.
// The streamed 64-row tiles are staged row-major in LDS and read twice: row-wise (ds_read_b128, the product that contracts along the head dim) and through
// ds_read_b64_tr_b16 (the product that contracts along the tile's ROW index: its 4 x 16 blocks deliver rows 4g .. 4g+3 to lane group g, the order in which
// the 16x16 accumulator of S / dP holds them, so P and dS go from the accumulators straight into the next MFMA's operand registers).
// LDS row pitch = HD + 16 elements = 8 * odd dwords for 64 / 96 / 128 (40, 56, 72): the 8 rows that one 32-lane half of a transposed read touches start
// 8 banks apart (each covers 8), and the 16 rows of one ds_read_b128 lane group -- rows r and r + 8 fall on the same even 16-byte slot, and exactly one of
// the two belongs to the lane group's g = 1 lanes, which read 16 bytes further on -- cover the 16 slots of the 256-byte bank row once each.
// Query rows >= klens[b] take no part (dq = 0, no contribution to dk / dv); key rows >= klens[b] get dk = dv = 0; every row of every utterance is written.
// Rows that take no part are zeroed ON THEIR WAY INTO LDS (keys >= klens[b] of the K / V tiles, queries >= klens[b] of the Q / dO tiles): a zero P / dS
// times whatever such a row holds must add exactly 0, so NEITHER entry has a finiteness precondition on them (the forward zeroes V the same way).
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

// What an entry hands to the three kernels (by value).  Strides in elements: bs from utterance to utterance (unused with row_off), rs from row to row.
struct BwdArgs {
    const bf16_t *q, *k, *v, *O, *dO;
    bf16_t *dq, *dk, *dv;
    const int32_t* klens;        // nullptr: every key is valid
    const int32_t* row_off;      // nullptr: uniform rows (utterance b at b * bs, Tq x Tk); else B + 1 row offsets, Tq = Tk = row_off[b + 1] - row_off[b]
    float *lse, *delta;          // the workspace halves
    int H, Tq, Tk;               // with row_off: Tq = Tk = Tmax, the longest utterance (the forward's mask pitch)
    int64_t q_bs, q_rs, kv_bs, kv_rs, o_bs, o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs;
    float scale, scale_log2e, keep_scale;
    uint32_t seed, thresh;
};

// One (utterance, head) unit: every kernel starts here, and nothing else in this file knows the two layouts apart.
struct Unit {
    int Tq, Tk;
    int klen, nq;                       // valid keys (clamped to Tk); queries that take part = min(klen, Tq)
    int64_t q0, kv0, o0, dq0, dkv0;     // element offset of (row 0, head h) in q | k, v | O, dO | dq | dk, dv
    int64_t st0;                        // offset of the unit's Tq statistics in lse / delta: (query rows before the utterance) * H + h * Tq
    uint32_t mask0, mask_step;          // the forward's dropout pair index of (query i, key j) is mask0 + i * mask_step + (j >> 1), mod 2^32
};
template <int HD>
__device__ __forceinline__ Unit unit_of(const BwdArgs& a, int b, int h) {
    Unit u;
    const uint32_t pairs = (uint32_t)((a.Tk + 1) >> 1);
    if (a.row_off) {       // mask row (row_off[b] + i) * H + h (attention.hip: drop_row), ceil(Tmax / 2) pairs each
        const int64_t r0 = a.row_off[b];
        u.Tq = u.Tk = a.row_off[b + 1] - (int)r0;
        u.q0 = r0 * a.q_rs, u.kv0 = r0 * a.kv_rs, u.o0 = r0 * a.o_rs, u.dq0 = r0 * a.dq_rs, u.dkv0 = r0 * a.dkv_rs;
        u.st0 = r0 * a.H + (int64_t)h * u.Tq;
        u.mask0 = ((uint32_t)r0 * (uint32_t)a.H + (uint32_t)h) * pairs;
        u.mask_step = (uint32_t)a.H * pairs;
    } else {               // mask row (b * H + h) * Tk + i (attention_hd.hip, and attention.hip's uniform layout), ceil(Tk / 2) pairs each
        u.Tq = a.Tq, u.Tk = a.Tk;
        u.q0 = b * a.q_bs, u.kv0 = b * a.kv_bs, u.o0 = b * a.o_bs, u.dq0 = b * a.dq_bs, u.dkv0 = b * a.dkv_bs;
        u.st0 = ((int64_t)b * a.H + h) * u.Tq;
        u.mask0 = (uint32_t)(b * a.H + h) * (uint32_t)u.Tk * pairs;
        u.mask_step = pairs;
    }
    const int hc = h * HD;
    u.q0 += hc, u.kv0 += hc, u.o0 += hc, u.dq0 += hc, u.dkv0 += hc;
    const int kl = a.klens ? a.klens[b] : u.Tk;
    u.klen = kl < 0 ? 0 : (kl > u.Tk ? u.Tk : kl);
    u.nq = u.klen < u.Tq ? u.klen : u.Tq;
    return u;
}

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
// sum / max over the four 16-lane groups of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) with the VALU lane swaps: every lane adds the same operands in the
// same order, and no LDS-crossbar shuffle feeds the arithmetic
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
// DELTA_PDP chooses where delta comes from.  false: delta = dO . O from the stored output.  With dropout the stored O = bf16(P_dropped V) no longer cancels
// against the recomputed sum_k P_dropped dP: with ONE kept key P_dropped = 1 / (1 - p), O = bf16(v / (1 - p)) is off v / (1 - p) by a bf16 ulp per element,
// and dS = P (m dP - delta), which is 0 analytically, keeps dO . (O - o) ~ sqrt(head_dim) 2^-9 |dO| |v|.  So the true form takes
// delta = sum_k P_dropped,k dP_k from the same MFMA products and the same mask the sweeps recompute (the online sum carried beside l), and the cancellation
// is exact in fp32.  sc_attention_hd_bwd launches the true form whenever it drops; sc_attention_bwd_packed always launches the false form.
template <int HD, bool DELTA_PDP>
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(const BwdArgs a) {
    constexpr int NC = BwdTile<HD>::NC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = blockIdx.x, b = z / a.H, h = z - b * a.H;
    const Unit u = unit_of<HD>(a, b, h);
    const int i0 = (blockIdx.y * 4 + wave) * 16;
    if (i0 >= u.Tq) return;
    const int qi = lane & 15, g = lane >> 4;
    const int i = i0 + qi, ic = i < u.Tq ? i : u.Tq - 1;
    const bf16_t* qr = a.q + u.q0 + (int64_t)ic * a.q_rs + g * 8;
    const bf16_t* orow = a.O + u.o0 + (int64_t)ic * a.o_rs + g * 8;
    const bf16_t* drow = a.dO + u.o0 + (int64_t)ic * a.o_rs + g * 8;
    bf16x8_t qf[NC], dof[NC];
    float dpart = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        qf[c] = *(const bf16x8_t*)(qr + c * 32);
        if (DELTA_PDP) {
            dof[c] = *(const bf16x8_t*)(drow + c * 32);
        } else {       // one expression of the chunk's eight products, then one add: scalar fp32 code (a per-element loop is SLP-vectorised into v_pk_add_f32)
            const u32x4_t du = *(const u32x4_t*)(drow + c * 32), ou = *(const u32x4_t*)(orow + c * 32);
            dpart += lo2f(du[0]) * lo2f(ou[0]) + hi2f(du[0]) * hi2f(ou[0]) + lo2f(du[1]) * lo2f(ou[1]) + hi2f(du[1]) * hi2f(ou[1])
                   + lo2f(du[2]) * lo2f(ou[2]) + hi2f(du[2]) * hi2f(ou[2]) + lo2f(du[3]) * lo2f(ou[3]) + hi2f(du[3]) * hi2f(ou[3]);
        }
    }
    const uint32_t mrow = u.mask0 + (uint32_t)ic * u.mask_step;
    // lane-local online max / sum over this lane's keys (4 g + r of every 16-key block); the four groups are combined once at the end
    float m = -INFINITY, l = 0.f, da = 0.f;
    const int nkb = (u.klen + 15) / 16;
    const bf16_t* kb_ = a.k + u.kv0 + g * 8;
    const bf16_t* vb_ = a.v + u.kv0 + g * 8;
    for (int kb = 0; kb < nkb; ++kb) {
        int key = kb * 16 + qi;
        key = key < u.Tk ? key : u.Tk - 1;
        const bf16_t* kr = kb_ + (int64_t)key * a.kv_rs;
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(kr + c * 32), qf[c], s, 0, 0, 0);
        float pm[4] = {0.f, 0.f, 0.f, 0.f};      // m dP of this lane's keys (0 for a dropped key and for keys >= klen, whatever V holds there)
        if (DELTA_PDP) {
            const bf16_t* vr = vb_ + (int64_t)key * a.kv_rs;
            f32x4_t pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(vr + c * 32), dof[c], pa, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const int kk = kb * 16 + 4 * g + r;      // even: registers r, r + 1 are one mask pair
                const uint32_t hb = hash_pair(a.seed, mrow + ((uint32_t)kk >> 1));
                pm[r] = kk < u.klen && (hb & 0xffffu) >= a.thresh ? pa[r] * a.keep_scale : 0.f;
                pm[r + 1] = kk + 1 < u.klen && (hb >> 16) >= a.thresh ? pa[r + 1] * a.keep_scale : 0.f;
            }
        }
        float bm = m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (kb * 16 + 4 * g + r) < u.klen ? s[r] * a.scale_log2e : -INFINITY;
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
    const float dd = DELTA_PDP ? groups_sum(m > -INFINITY ? da * __builtin_amdgcn_exp2f(m - mt) : 0.f) / lt : groups_sum(dpart);
    if (g == 0 && i < u.Tq) {
        const bool ok = i < u.klen && lt > 0.f;
        a.lse[u.st0 + i] = ok ? mt + __builtin_amdgcn_logf(lt) : 0.f;      // v_log_f32: log2
        a.delta[u.st0 + i] = ok ? dd : 0.f;
    }
}

// ---- dQ: a block owns 64 queries (16 per wave) of one (b, h) and walks the key tiles
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const BwdArgs a) {
    using TL = BwdTile<HD>;
    constexpr int LDR = TL::LDR, NC = TL::NC, ND = TL::ND;
    __shared__ __attribute__((aligned(16))) bf16_t ks[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t vs[TILE * LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / a.H, h = z - b * a.H;
    const Unit u = unit_of<HD>(a, b, h);
    const int q0 = blockIdx.y * TILE;
    if (q0 >= u.Tq) return;
    bf16_t* dq_u = a.dq + u.dq0;
    if (q0 >= u.nq) { zero_rows<HD>(dq_u, a.dq_rs, q0, u.Tq, tid); return; }
    const int qi = lane & 15, g = lane >> 4;
    const int i = q0 + wave * 16 + qi, ic = i < u.Tq ? i : u.Tq - 1;
    const bool q_ok = i < u.nq;
    const bf16_t* qr = a.q + u.q0 + (int64_t)ic * a.q_rs + g * 8;
    const bf16_t* drow = a.dO + u.o0 + (int64_t)ic * a.o_rs + g * 8;
    bf16x8_t qf[NC], dof[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        qf[c] = *(const bf16x8_t*)(qr + c * 32);
        dof[c] = *(const bf16x8_t*)(drow + c * 32);
    }
    const float lse_i = a.lse[u.st0 + ic], del_i = a.delta[u.st0 + ic];
    const uint32_t mrow = DROP ? u.mask0 + (uint32_t)ic * u.mask_step : 0u;
    const bf16_t* k_u = a.k + u.kv0;
    const bf16_t* v_u = a.v + u.kv0;
    f32x4_t acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int nt = (u.klen + TILE - 1) / TILE;
    Stage<HD> sk, sv;
    sk.load(k_u, a.kv_rs, 0, u.Tk, u.klen, tid);
    sv.load(v_u, a.kv_rs, 0, u.Tk, u.klen, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                     // every wave is done with the previous tile
        sk.store(ks, tid);
        sv.store(vs, tid);
        __syncthreads();
        if (t + 1 < nt) {
            sk.load(k_u, a.kv_rs, (t + 1) * TILE, u.Tk, u.klen, tid);
            sv.load(v_u, a.kv_rs, (t + 1) * TILE, u.Tk, u.klen, tid);
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
                        const uint32_t hb = hash_pair(a.seed, mrow + ((uint32_t)key >> 1));
                        m0 = (hb & 0xffffu) >= a.thresh ? a.keep_scale : 0.f;
                        m1 = (hb >> 16) >= a.thresh ? a.keep_scale : 0.f;
                    }
                    const bool ok0 = q_ok && key < u.klen, ok1 = q_ok && key + 1 < u.klen;
                    const float p0 = __builtin_amdgcn_exp2f(sa[r] * a.scale_log2e - lse_i), p1 = __builtin_amdgcn_exp2f(sa[r + 1] * a.scale_log2e - lse_i);
                    ds[r] = ok0 ? p0 * (pa[r] * m0 - del_i) * a.scale : 0.f;
                    ds[r + 1] = ok1 ? p1 * (pa[r + 1] * m1 - del_i) * a.scale : 0.f;
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
    if (i < u.Tq) {       // lane: query qi, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < ND; ++d)
            *(uint2*)(dq_u + (int64_t)i * a.dq_rs + d * 16 + 4 * g) = make_uint2(pack2bf(acc[d][0], acc[d][1]), pack2bf(acc[d][2], acc[d][3]));
    }
}

// ---- dK, dV: a block owns 64 keys (16 per wave) of one (b, h) and walks the query tiles
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const BwdArgs a) {
    using TL = BwdTile<HD>;
    constexpr int LDR = TL::LDR, NC = TL::NC, ND = TL::ND;
    __shared__ __attribute__((aligned(16))) bf16_t qs[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t os[TILE * LDR];
    __shared__ __attribute__((aligned(16))) float st[2 * TILE];      // lse | delta of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / a.H, h = z - b * a.H;
    const Unit u = unit_of<HD>(a, b, h);
    const int k0 = blockIdx.y * TILE;
    if (k0 >= u.Tk) return;
    bf16_t* dk_u = a.dk + u.dkv0;
    bf16_t* dv_u = a.dv + u.dkv0;
    if (k0 >= u.klen) { zero_rows<HD>(dk_u, a.dkv_rs, k0, u.Tk, tid); zero_rows<HD>(dv_u, a.dkv_rs, k0, u.Tk, tid); return; }
    const int ki = lane & 15, g = lane >> 4;
    const int j = k0 + wave * 16 + ki, jc = j < u.Tk ? j : u.Tk - 1;
    const bool k_ok = j < u.klen;
    const bf16_t* kr = a.k + u.kv0 + (int64_t)jc * a.kv_rs + g * 8;
    const bf16_t* vr = a.v + u.kv0 + (int64_t)jc * a.kv_rs + g * 8;
    bf16x8_t kf[NC], vf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        kf[c] = *(const bf16x8_t*)(kr + c * 32);
        vf[c] = *(const bf16x8_t*)(vr + c * 32);
    }
    const uint32_t mkey = u.mask0 + ((uint32_t)jc >> 1);      // this lane's key pair in the forward's mask row of query 0
    const bool khigh = (jc & 1) != 0;
    const bf16_t* q_u = a.q + u.q0;
    const bf16_t* o_u = a.dO + u.o0;
    const float* lse_u = a.lse + u.st0;
    const float* del_u = a.delta + u.st0;
    f32x4_t ak[ND], av[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { ak[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; av[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
    const int nt = (u.nq + TILE - 1) / TILE;      // queries >= nq take no part
    Stage<HD> sq, so;
    float sreg = 0.f;
    auto load_stats = [&](int t0) {
        if (tid < 2 * TILE) {
            int r = t0 + (tid & (TILE - 1));
            r = r < u.Tq ? r : u.Tq - 1;
            sreg = (tid < TILE ? lse_u : del_u)[r];
        }
    };
    sq.load(q_u, a.q_rs, 0, u.Tq, u.nq, tid);
    so.load(o_u, a.o_rs, 0, u.Tq, u.nq, tid);
    load_stats(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        sq.store(qs, tid);
        so.store(os, tid);
        if (tid < 2 * TILE) st[tid] = sreg;
        __syncthreads();
        if (t + 1 < nt) {
            sq.load(q_u, a.q_rs, (t + 1) * TILE, u.Tq, u.nq, tid);
            so.load(o_u, a.o_rs, (t + 1) * TILE, u.Tq, u.nq, tid);
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
                        const uint32_t hb = hash_pair(a.seed, (uint32_t)query * u.mask_step + mkey);
                        m = (khigh ? (hb >> 16) : (hb & 0xffffu)) >= a.thresh ? a.keep_scale : 0.f;
                    }
                    const bool ok = k_ok && query < u.nq;
                    const float p = __builtin_amdgcn_exp2f(sa[r] * a.scale_log2e - ls[r]);
                    pv[r] = ok ? p * m : 0.f;
                    ds[r] = ok ? p * (pa[r] * m - de[r]) * a.scale : 0.f;
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
    if (j < u.Tk) {       // lane: key ki, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            *(uint2*)(dk_u + (int64_t)j * a.dkv_rs + d * 16 + 4 * g) = make_uint2(pack2bf(ak[d][0], ak[d][1]), pack2bf(ak[d][2], ak[d][3]));
            *(uint2*)(dv_u + (int64_t)j * a.dkv_rs + d * 16 + 4 * g) = make_uint2(pack2bf(av[d][0], av[d][1]), pack2bf(av[d][2], av[d][3]));
        }
    }
}

// statistics, dK / dV sweep, dQ sweep over B utterances; a.Tq / a.Tk bound the grids (with row_off: the longest utterance)
template <int HD>
void launch(const BwdArgs& a, int B, bool delta_pdp, hipStream_t s) {
    const dim3 block(256), gq((unsigned)(B * a.H), (unsigned)((a.Tq + TILE - 1) / TILE)), gk((unsigned)(B * a.H), (unsigned)((a.Tk + TILE - 1) / TILE));
    if (delta_pdp) hipLaunchKernelGGL((attn_bwd_stats_kernel<HD, true>), gq, block, 0, s, a);
    else hipLaunchKernelGGL((attn_bwd_stats_kernel<HD, false>), gq, block, 0, s, a);
    if (a.thresh) {
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, true>), gk, block, 0, s, a);
        hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, true>), gq, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<HD, false>), gk, block, 0, s, a);
        hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, false>), gq, block, 0, s, a);
    }
}

// the fields every entry fills the same way
BwdArgs common_args(const void* q, const void* k, const void* v, const void* O, const void* dO, void* dq, void* dk, void* dv, const int32_t* klens, int H,
                    float scale, float drop_p, uint32_t seed, void* workspace, int64_t stat_rows) {
    BwdArgs a = {};
    a.q = (const bf16_t*)q, a.k = (const bf16_t*)k, a.v = (const bf16_t*)v, a.O = (const bf16_t*)O, a.dO = (const bf16_t*)dO;
    a.dq = (bf16_t*)dq, a.dk = (bf16_t*)dk, a.dv = (bf16_t*)dv;
    a.klens = klens;
    a.lse = (float*)workspace;
    a.delta = a.lse + stat_rows * H;
    a.H = H;
    a.scale = scale, a.scale_log2e = scale * 1.44269504088896341f, a.keep_scale = 1.0f / (1.0f - drop_p);
    a.seed = seed, a.thresh = drop_thresh16(drop_p);
    return a;
}

}  // namespace

extern "C" int64_t sc_attention_bwd_packed_workspace_bytes(int64_t total_rows, int H) {
    return total_rows > 0 && H > 0 ? 2 * total_rows * (int64_t)H * (int64_t)sizeof(float) : 0;
}

// Rows >= klens[b] of an utterance (K / V, and the Q / dO / O rows of such queries) take no part and may hold anything, NaN and Inf included: they are
// zeroed on their way into LDS, as in sc_attention_hd_bwd.  For finite inputs that changes no bit (a zero P / dS times a finite value already added 0).
extern "C" int sc_attention_bwd_packed(const void* q, const void* k, const void* v, int64_t ld_qkv, const void* O, const void* dO, int64_t ld_o,
                                       const int32_t* klens, const int32_t* row_off, int B, int H, int Tmax, int64_t total_rows, int head_dim, float scale,
                                       float drop_p, uint32_t seed, void* dq, void* dk, void* dv, int64_t ld_dqkv, void* workspace, void* stream) {
    SC_CHECK_ARG(head_dim == 64, "sc_attention_bwd_packed: head_dim=%d unsupported (64 only)", head_dim);
    SC_CHECK_ARG(q && k && v && O && dO && dq && dk && dv && workspace && klens, "sc_attention_bwd_packed: null operand");
    SC_CHECK_ARG(ld_qkv % 8 == 0 && ld_o % 8 == 0 && ld_dqkv % 8 == 0, "sc_attention_bwd_packed: row strides must be multiples of 8 (16-byte rows)");
    SC_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)O | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)workspace) & 15) == 0,
                 "sc_attention_bwd_packed: misaligned pointers");
    SC_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "sc_attention_bwd_packed: drop_p=%f must be in [0, 1)", (double)drop_p);
    SC_CHECK_ARG(B >= 0 && H > 0 && Tmax >= 0 && total_rows >= 0 && (int64_t)B * H < 0x7fffffffLL, "sc_attention_bwd_packed: bad sizes");
    SC_CHECK_ARG(row_off || total_rows == (int64_t)B * Tmax, "sc_attention_bwd_packed: the uniform layout has total_rows = B * Tmax");
    SC_CHECK_ARG(drop_p == 0.f || (row_off ? total_rows * H * ((Tmax + 1) / 2) : (int64_t)B * H * Tmax * Tmax) < 0xffffffffLL,
                 "sc_attention_bwd_packed: the mask element index must fit 32 bits");
    if (B <= 0 || Tmax <= 0 || total_rows <= 0) return 0;
    SC_CHECK_ARG((Tmax + TILE - 1) / TILE <= 65535, "sc_attention_bwd_packed: Tmax=%d too long", Tmax);
    BwdArgs a = common_args(q, k, v, O, dO, dq, dk, dv, klens, H, scale, drop_p, seed, workspace, total_rows);
    a.row_off = row_off;
    a.Tq = a.Tk = Tmax;
    a.q_rs = a.kv_rs = ld_qkv, a.o_rs = ld_o, a.dq_rs = a.dkv_rs = ld_dqkv;
    a.q_bs = a.kv_bs = Tmax * ld_qkv, a.o_bs = Tmax * ld_o, a.dq_bs = a.dkv_bs = Tmax * ld_dqkv;      // the uniform layout is the strided one
    launch<64>(a, B, false, (hipStream_t)stream);
    SC_CHECK_LAUNCH();
    return 0;
}

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
    BwdArgs a = common_args(q, k, v, O, dO, dq, dk, dv, klens, H, scale, drop_p, seed, workspace, (int64_t)B * Tq);
    a.Tq = Tq, a.Tk = Tk;
    a.q_bs = q_bs, a.q_rs = q_rs, a.kv_bs = kv_bs, a.kv_rs = kv_rs, a.o_bs = o_bs, a.o_rs = o_rs;
    a.dq_bs = dq_bs, a.dq_rs = dq_rs, a.dkv_bs = dkv_bs, a.dkv_rs = dkv_rs;
    const bool delta_pdp = a.thresh != 0;      // it drops: delta from the pre-pass's own P_dropped dP (attn_bwd_stats_kernel)
    if (head_dim == 64) launch<64>(a, B, delta_pdp, (hipStream_t)stream);
    else if (head_dim == 96) launch<96>(a, B, delta_pdp, (hipStream_t)stream);
    else launch<128>(a, B, delta_pdp, (hipStream_t)stream);
    SC_CHECK_LAUNCH();
    return 0;
}
