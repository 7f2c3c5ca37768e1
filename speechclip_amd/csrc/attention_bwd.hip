// Fused attention backward for head_dim 64 over packed (padding-free) or uniform rows, gfx950.
// Operands are addressed exactly as sc_attention_fwd_packed addresses them: bf16 rows, head h at column h*64, utterance b at rows row_off[b] ..
// (row_off == nullptr: b * Tmax), klens[b] valid keys.  Nothing of size L x L reaches memory: S = Q K^T and dP = dO V^T are recomputed on the matrix
// cores (v_mfma_f32_16x16x32_bf16) in both sweeps, the softmax arithmetic is fp32 in registers.  Three kernels:
//   attn_bwd_stats_kernel  per (row, head): lse = log2 sum_k exp2(s_k) (s in log2 units) and delta = dO . O -> the fp32 workspace
//   attn_bwd_dq_kernel     query-tile-stationary sweep over the key tiles:  dQ^T += K^T dS^T
//   attn_bwd_dkv_kernel    key-tile-stationary sweep over the query tiles:  dV^T += dO^T P_dropped,  dK^T += Q^T dS
// Every output element is produced by exactly one wave in a fixed order (no atomics): results are bitwise reproducible.
// The streamed tiles are staged row-major in LDS (rows padded to 144 bytes); the operands that contract over the tile's ROW index come out of the
// same image through ds_read_b64_tr_b16, whose 4 x 16 blocks deliver rows 4g .. 4g+3 to lane group g -- the order in which the 16x16 accumulator of the
// recomputed S / dP holds them, so P and dS go from the accumulators straight into the next MFMA's operand registers.
// Query rows >= klens[b] take no part (dq = 0, no contribution to dk / dv); key rows >= klens[b] get dk = dv = 0; every row of every utterance is written.
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

constexpr int LDR = 72;        // LDS row pitch in elements: 64 head dims + 8 (144 bytes: 16-byte aligned, rows spread over the banks)
constexpr int TILE = 64;       // streamed rows per tile

// rows k0 .. k0+3 (this lane group's) x 16 columns of a row-major LDS image, column (lane & 15) delivered to the lane
__device__ __forceinline__ s16x4_t lds_tr(const bf16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}
// MFMA operand with k-slots 0-3 = rows r0 + 4g .. + 3 and 4-7 = rows r0 + 16 + 4g .. + 3 of the image (column d0 + (lane & 15))
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

struct Geom {      // one (utterance, head) unit
    int T, klen;
    int64_t row_base;
    uint32_t drop_pairs;
};
__device__ __forceinline__ Geom unit_geom(const int32_t* klens, const int32_t* row_off, int b, int Tmax) {
    Geom u;
    u.T = row_off ? row_off[b + 1] - row_off[b] : Tmax;
    u.row_base = row_off ? (int64_t)row_off[b] : (int64_t)b * Tmax;
    const int kl = klens[b];
    u.klen = kl < 0 ? 0 : (kl > u.T ? u.T : kl);
    u.drop_pairs = (uint32_t)((Tmax + 1) >> 1);      // (uniform layout: T == Tmax)
    return u;
}
// the forward's mask row index (attention.hip: drop_row)
__device__ __forceinline__ uint32_t drop_row_of(const Geom& u, bool packed, int b, int h, int H, int query) {
    return packed ? (uint32_t)((u.row_base + query) * H + h) : (uint32_t)((b * H + h) * u.T + query);
}

// 64 rows x 128 bytes of zeros at rows r0 .. of one head's column block (rows < T only)
__device__ __forceinline__ void zero_rows(bf16_t* base, int64_t ld, int r0, int T, int tid) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int r = r0 + (tid >> 3) + 32 * it;
        if (r < T) *(uint4*)(base + (int64_t)r * ld + (tid & 7) * 8) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- statistics: one wave per 16 queries; K fragments are single 16-byte global loads (the product contracts along the head dimension)
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, int64_t ld_qkv,
                                                             const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, int64_t ld_o,
                                                             const int32_t* __restrict__ klens, const int32_t* __restrict__ row_off, int H, int Tmax,
                                                             float scale_log2e, float* __restrict__ lse, float* __restrict__ delta) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const Geom u = unit_geom(klens, row_off, b, Tmax);
    const int i0 = (blockIdx.y * 4 + wave) * 16;
    if (i0 >= u.T) return;
    const int qi = lane & 15, g = lane >> 4;
    const int i = i0 + qi, ic = i < u.T ? i : u.T - 1;
    const int64_t row = u.row_base + ic;
    bf16x8_t qf[2];
    float dpart = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        qf[c] = *(const bf16x8_t*)(q + row * ld_qkv + h * 64 + c * 32 + g * 8);
        const uint4 du = *(const uint4*)(dO + row * ld_o + h * 64 + c * 32 + g * 8);
        const uint4 ou = *(const uint4*)(O + row * ld_o + h * 64 + c * 32 + g * 8);
        dpart += lo2f(du.x) * lo2f(ou.x) + hi2f(du.x) * hi2f(ou.x) + lo2f(du.y) * lo2f(ou.y) + hi2f(du.y) * hi2f(ou.y)
               + lo2f(du.z) * lo2f(ou.z) + hi2f(du.z) * hi2f(ou.z) + lo2f(du.w) * lo2f(ou.w) + hi2f(du.w) * hi2f(ou.w);
    }
    const float dd = groups_sum(dpart);
    // lane-local online max / sum over this lane's keys (4 g + r of every 16-key block); the four groups are combined once at the end
    float m = -INFINITY, l = 0.f;
    const int nkb = (u.klen + 15) / 16;
    for (int kb = 0; kb < nkb; ++kb) {
        int key = kb * 16 + qi;
        key = key < u.T ? key : u.T - 1;
        const bf16_t* kr = k + (u.row_base + key) * ld_qkv + h * 64 + g * 8;
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 2; ++c) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(kr + c * 32), qf[c], s, 0, 0, 0);
        float bm = m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (kb * 16 + 4 * g + r) < u.klen ? s[r] * scale_log2e : -INFINITY;
            bm = fmaxf(bm, s[r]);
        }
        if (bm > -INFINITY) {
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) ps += __builtin_amdgcn_exp2f(s[r] - bm);
            l = l * __builtin_amdgcn_exp2f(m - bm) + ps;
            m = bm;
        }
    }
    const float mt = groups_max(m);
    const float lt = groups_sum(m > -INFINITY ? l * __builtin_amdgcn_exp2f(m - mt) : 0.f);
    if (g == 0 && i < u.T) {
        const bool ok = i < u.klen && lt > 0.f;
        lse[row * H + h] = ok ? mt + __builtin_amdgcn_logf(lt) : 0.f;      // v_log_f32: log2
        delta[row * H + h] = ok ? dd : 0.f;
    }
}

// 64 rows of a [rows][head] operand (row t0 + r, clamped to the utterance) -> registers -> the LDS image
struct Stage {
    uint4 v0, v1;      // rows (tid >> 3) and (tid >> 3) + 32, 16-byte chunk tid & 7
    __device__ __forceinline__ static uint4 row(const bf16_t* base, int64_t ld, int r, int T, int tid) {
        r = r < T ? r : T - 1;
        return *(const uint4*)(base + (int64_t)r * ld + (tid & 7) * 8);
    }
    __device__ __forceinline__ void load(const bf16_t* base, int64_t ld, int t0, int T, int tid) {
        v0 = row(base, ld, t0 + (tid >> 3), T, tid);
        v1 = row(base, ld, t0 + (tid >> 3) + 32, T, tid);
    }
    __device__ __forceinline__ void store(bf16_t* img, int tid) const {
        *(uint4*)(img + (tid >> 3) * LDR + (tid & 7) * 8) = v0;
        *(uint4*)(img + ((tid >> 3) + 32) * LDR + (tid & 7) * 8) = v1;
    }
};

// ---- dQ: a block owns 64 queries (16 per wave) of one (b, h) and walks the key tiles
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          int64_t ld_qkv, const bf16_t* __restrict__ dO, int64_t ld_o, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, const int32_t* __restrict__ klens,
                                                          const int32_t* __restrict__ row_off, int H, int Tmax, float scale, float scale_log2e,
                                                          uint32_t seed, uint32_t thresh, float keep_scale, bf16_t* __restrict__ dq, int64_t ld_d) {
    __shared__ __attribute__((aligned(16))) bf16_t ks[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t vs[TILE * LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const Geom u = unit_geom(klens, row_off, b, Tmax);
    const int q0 = blockIdx.y * TILE;
    if (q0 >= u.T) return;
    bf16_t* dq_u = dq + u.row_base * ld_d + h * 64;
    if (q0 >= u.klen) { zero_rows(dq_u, ld_d, q0, u.T, tid); return; }
    const int qi = lane & 15, g = lane >> 4;
    const int i = q0 + wave * 16 + qi, ic = i < u.T ? i : u.T - 1;
    const bool q_ok = i < u.klen;
    const int64_t row = u.row_base + ic;
    bf16x8_t qf[2], dof[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        qf[c] = *(const bf16x8_t*)(q + row * ld_qkv + h * 64 + c * 32 + g * 8);
        dof[c] = *(const bf16x8_t*)(dO + row * ld_o + h * 64 + c * 32 + g * 8);
    }
    const float lse_i = lse[row * H + h], del_i = delta[row * H + h];
    const uint32_t drow = DROP ? drop_row_of(u, row_off != nullptr, b, h, H, ic) * u.drop_pairs : 0u;
    const bf16_t* k_u = k + u.row_base * ld_qkv + h * 64;
    const bf16_t* v_u = v + u.row_base * ld_qkv + h * 64;
    f32x4_t acc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int nt = (u.klen + TILE - 1) / TILE;
    Stage sk, sv;
    sk.load(k_u, ld_qkv, 0, u.T, tid);
    sv.load(v_u, ld_qkv, 0, u.T, tid);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                     // every wave is done with the previous tile
        sk.store(ks, tid);
        sv.store(vs, tid);
        __syncthreads();
        if (t + 1 < nt) {
            sk.load(k_u, ld_qkv, (t + 1) * TILE, u.T, tid);
            sv.load(v_u, ld_qkv, (t + 1) * TILE, u.T, tid);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {        // 32 keys: one k-step of dQ^T += K^T dS^T
            uint32_t dsp[4];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int kb = 2 * s + sub;
                f32x4_t sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(ks + (kb * 16 + qi) * LDR + c * 32 + g * 8), qf[c], sa, 0, 0, 0);
                    pa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(vs + (kb * 16 + qi) * LDR + c * 32 + g * 8), dof[c], pa, 0, 0, 0);
                }
                float ds[4];
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const int key = t * TILE + kb * 16 + 4 * g + r;      // even: registers r, r + 1 are one mask pair
                    float m0 = 1.f, m1 = 1.f;
                    if (DROP) {
                        const uint32_t hb = hash_pair(seed, drow + ((uint32_t)key >> 1));
                        m0 = (hb & 0xffffu) >= thresh ? keep_scale : 0.f;
                        m1 = (hb >> 16) >= thresh ? keep_scale : 0.f;
                    }
                    const bool ok0 = q_ok && key < u.klen, ok1 = q_ok && key + 1 < u.klen;
                    const float p0 = __builtin_amdgcn_exp2f(sa[r] * scale_log2e - lse_i), p1 = __builtin_amdgcn_exp2f(sa[r + 1] * scale_log2e - lse_i);
                    ds[r] = ok0 ? p0 * (pa[r] * m0 - del_i) * scale : 0.f;
                    ds[r + 1] = ok1 ? p1 * (pa[r + 1] * m1 - del_i) * scale : 0.f;
                }
                dsp[2 * sub] = pack2bf(ds[0], ds[1]);
                dsp[2 * sub + 1] = pack2bf(ds[2], ds[3]);
            }
            const bf16x8_t dsf = frag_of(dsp[0], dsp[1], dsp[2], dsp[3]);
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag(ks, s * 32, d * 16, lane), dsf, acc[d], 0, 0, 0);
        }
    }
    if (i < u.T) {       // lane: query qi, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < 4; ++d)
            *(uint2*)(dq_u + (int64_t)i * ld_d + d * 16 + 4 * g) = make_uint2(pack2bf(acc[d][0], acc[d][1]), pack2bf(acc[d][2], acc[d][3]));
    }
}

// ---- dK, dV: a block owns 64 keys (16 per wave) of one (b, h) and walks the query tiles
template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                           int64_t ld_qkv, const bf16_t* __restrict__ dO, int64_t ld_o, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, const int32_t* __restrict__ klens,
                                                           const int32_t* __restrict__ row_off, int H, int Tmax, float scale, float scale_log2e,
                                                           uint32_t seed, uint32_t thresh, float keep_scale, bf16_t* __restrict__ dk,
                                                           bf16_t* __restrict__ dv, int64_t ld_d) {
    __shared__ __attribute__((aligned(16))) bf16_t qs[TILE * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t os[TILE * LDR];
    __shared__ __attribute__((aligned(16))) float st[2 * TILE];      // lse | delta of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x, b = z / H, h = z - b * H;
    const Geom u = unit_geom(klens, row_off, b, Tmax);
    const int k0 = blockIdx.y * TILE;
    if (k0 >= u.T) return;
    bf16_t* dk_u = dk + u.row_base * ld_d + h * 64;
    bf16_t* dv_u = dv + u.row_base * ld_d + h * 64;
    if (k0 >= u.klen) { zero_rows(dk_u, ld_d, k0, u.T, tid); zero_rows(dv_u, ld_d, k0, u.T, tid); return; }
    const int ki = lane & 15, g = lane >> 4;
    const int j = k0 + wave * 16 + ki, jc = j < u.T ? j : u.T - 1;
    const bool k_ok = j < u.klen;
    bf16x8_t kf[2], vf[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        kf[c] = *(const bf16x8_t*)(k + (u.row_base + jc) * ld_qkv + h * 64 + c * 32 + g * 8);
        vf[c] = *(const bf16x8_t*)(v + (u.row_base + jc) * ld_qkv + h * 64 + c * 32 + g * 8);
    }
    const bool packed = row_off != nullptr;
    const uint32_t kpair = (uint32_t)jc >> 1;
    const bool khigh = (jc & 1) != 0;
    const bf16_t* q_u = q + u.row_base * ld_qkv + h * 64;
    const bf16_t* o_u = dO + u.row_base * ld_o + h * 64;
    f32x4_t ak[4], av[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) { ak[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; av[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
    const int nt = (u.klen + TILE - 1) / TILE;      // queries >= klen take no part
    Stage sq, so;
    float sreg = 0.f;
    auto load_stats = [&](int t0) {
        if (tid < 2 * TILE) {
            int r = t0 + (tid & (TILE - 1));
            r = r < u.T ? r : u.T - 1;
            sreg = (tid < TILE ? lse : delta)[(u.row_base + r) * H + h];
        }
    };
    sq.load(q_u, ld_qkv, 0, u.T, tid);
    so.load(o_u, ld_o, 0, u.T, tid);
    load_stats(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        sq.store(qs, tid);
        so.store(os, tid);
        if (tid < 2 * TILE) st[tid] = sreg;
        __syncthreads();
        if (t + 1 < nt) {
            sq.load(q_u, ld_qkv, (t + 1) * TILE, u.T, tid);
            so.load(o_u, ld_o, (t + 1) * TILE, u.T, tid);
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
                for (int c = 0; c < 2; ++c) {     // first operand = query rows: the lane holds key ki, queries 4 g + r of the block
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
                        const uint32_t hb = hash_pair(seed, drop_row_of(u, packed, b, h, H, query) * u.drop_pairs + kpair);
                        m = (khigh ? (hb >> 16) : (hb & 0xffffu)) >= thresh ? keep_scale : 0.f;
                    }
                    const bool ok = k_ok && query < u.klen;
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
            for (int d = 0; d < 4; ++d) {
                av[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag(os, s * 32, d * 16, lane), pf, av[d], 0, 0, 0);
                ak[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr_frag(qs, s * 32, d * 16, lane), dsf, ak[d], 0, 0, 0);
            }
        }
    }
    if (j < u.T) {       // lane: key ki, head dims 16 d + 4 g .. + 3
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            *(uint2*)(dk_u + (int64_t)j * ld_d + d * 16 + 4 * g) = make_uint2(pack2bf(ak[d][0], ak[d][1]), pack2bf(ak[d][2], ak[d][3]));
            *(uint2*)(dv_u + (int64_t)j * ld_d + d * 16 + 4 * g) = make_uint2(pack2bf(av[d][0], av[d][1]), pack2bf(av[d][2], av[d][3]));
        }
    }
}

}  // namespace

extern "C" int64_t sc_attention_bwd_packed_workspace_bytes(int64_t total_rows, int H) {
    return total_rows > 0 && H > 0 ? 2 * total_rows * (int64_t)H * (int64_t)sizeof(float) : 0;
}

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
    const int nblk = (Tmax + TILE - 1) / TILE;
    SC_CHECK_ARG(nblk <= 65535, "sc_attention_bwd_packed: Tmax=%d too long", Tmax);
    hipStream_t s = (hipStream_t)stream;
    float* lse = (float*)workspace;
    float* delta = lse + total_rows * H;
    const float sl2 = scale * 1.44269504088896341f;
    const uint32_t th = drop_thresh16(drop_p);
    const float ks = 1.0f / (1.0f - drop_p);
    const dim3 grid((unsigned)(B * H), (unsigned)nblk), block(256);
    hipLaunchKernelGGL(attn_bwd_stats_kernel, grid, block, 0, s, (const bf16_t*)q, (const bf16_t*)k, ld_qkv, (const bf16_t*)O, (const bf16_t*)dO, ld_o, klens,
                       row_off, H, Tmax, sl2, lse, delta);
#define SC_BWD_LAUNCH(DR)                                                                                                                          \
    do {                                                                                                                                           \
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<DR>), grid, block, 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld_qkv,             \
                           (const bf16_t*)dO, ld_o, (const float*)lse, (const float*)delta, klens, row_off, H, Tmax, scale, sl2, seed, th, ks,      \
                           (bf16_t*)dk, (bf16_t*)dv, ld_dqkv);                                                                                      \
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DR>), grid, block, 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld_qkv,              \
                           (const bf16_t*)dO, ld_o, (const float*)lse, (const float*)delta, klens, row_off, H, Tmax, scale, sl2, seed, th, ks,      \
                           (bf16_t*)dq, ld_dqkv);                                                                                                   \
    } while (0)
    if (th) SC_BWD_LAUNCH(true);
    else SC_BWD_LAUNCH(false);
#undef SC_BWD_LAUNCH
    SC_CHECK_LAUNCH();
    return 0;
}
