// Backward pieces for fine-tuning the CLIP image tower (clip.image_encoder_trainable; reference avssl/module/clip_official.py `freeze_models` /
// `trainable_params`: model.visual trains with the speech side).  The ViT blocks are the pre-LN layer bodies of train_hubert.py (MFMA GEMMs, split-K
// wgrad, sc_layernorm_bwd_bf16, the fused head-dim-64 attention backward); this file holds the ViT-specific arithmetic:
//   sc_quickgelu_bwd_bf16    du = dh q'(u), q(u) = u sigmoid(1.702 u): the activation of CLIP's MLP (the pre-activation is recomputed by the caller)
//   sc_vit_embed_bwd         adjoint of sc_vit_embed (frontend.hip): x0 = LN_pre([cls | patch] + pos).  The row, its mean and its rstd are recomputed
//                            from the forward's inputs; outputs the gradient of the patch GEMM's output (bf16), of the positional embedding (row 0 =
//                            the class embedding's) and of ln_pre's gamma / beta.
// Reductions over the batch and over rows are two fixed stages (per-block partials in a workspace, a fixed-order finish): no atomics, bitwise
// reproducible.  Row statistics: one row per wave at a time, wave_sum butterflies (the form rowops.hip keeps to).
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

__device__ __forceinline__ float quickgelu_grad(float x) {
    // s + 1.702 u s (1 - s), s = sigmoid(1.702 u), on u = clamp(x, +-64): there s is 0 (e^{108.9} = inf, 1 / inf = 0) or 1 to the last bit, and no product of
    // the expression meets an infinity whatever x is.  1 - s is formed from s, not as e^{-1.702 u} s (inf * 0 in the left tail).
    const float u = __builtin_amdgcn_fmed3f(x, -64.0f, 64.0f);
    const float s = __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * u));
    return s * fmaf(1.702f * u, 1.0f - s, 1.0f);
}

// Elements [head, head + 8 nvec) go as 16-byte groups (u, dh, du share their address modulo 16: `head` elements reach the boundary), the others one by one.
__global__ __launch_bounds__(256) void quickgelu_bwd_bf16_kernel(const bf16_t* __restrict__ u, const bf16_t* __restrict__ dh, bf16_t* __restrict__ du, int64_t n,
                                                                 int64_t head, int64_t nvec) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < nvec) {
        const int64_t i = head + t * 8;
        const uint4 uu = *(const uint4*)(u + i), gg = *(const uint4*)(dh + i);
        uint4 o;
        o.x = pack2bf(lo2f(gg.x) * quickgelu_grad(lo2f(uu.x)), hi2f(gg.x) * quickgelu_grad(hi2f(uu.x)));
        o.y = pack2bf(lo2f(gg.y) * quickgelu_grad(lo2f(uu.y)), hi2f(gg.y) * quickgelu_grad(hi2f(uu.y)));
        o.z = pack2bf(lo2f(gg.z) * quickgelu_grad(lo2f(uu.z)), hi2f(gg.z) * quickgelu_grad(hi2f(uu.z)));
        o.w = pack2bf(lo2f(gg.w) * quickgelu_grad(lo2f(uu.w)), hi2f(gg.w) * quickgelu_grad(hi2f(uu.w)));
        *(uint4*)(du + i) = o;
        return;
    }
    int64_t j = t - nvec;                                  // the `head` elements in front of the groups, then the tail behind them
    if (j >= head) j += nvec * 8;
    if (j < n) du[j] = f2bf(bf2f(dh[j]) * quickgelu_grad(bf2f(u[j])));
}

// Block (tk, split): token tk of the batches [split * bchunk, (split + 1) * bchunk); wave w takes every fourth of them, one row at a time.  A lane owns
// elements c * 256 + lane * 4 .. + 3 (c < 4) of a row, as in vit_embed_kernel.  The block writes ONE partial row triple ws[split][tk][dpos | dgamma | dbeta][D].
__global__ __launch_bounds__(256) void vit_embed_bwd_kernel(const float* __restrict__ dx, const bf16_t* __restrict__ patch, const float* __restrict__ cls,
                                                            const float* __restrict__ pos, const float* __restrict__ gamma, bf16_t* __restrict__ dpatch,
                                                            float* __restrict__ ws, int B, int ntok, int D, float eps, int bchunk) {
    __shared__ float red[3][4][1024];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tk = blockIdx.x, split = blockIdx.y;
    const int b_end = min(B, (split + 1) * bchunk);
    float g[4][4], base[4][4], ap[4][4], ag[4][4], ab[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int e = c * 256 + lane * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ap[c][i] = ag[c][i] = ab[c][i] = 0.f;
            g[c][i] = e < D ? gamma[e + i] : 0.f;
            base[c][i] = e < D ? pos[(int64_t)tk * D + e + i] : 0.f;
        }
    }
    for (int b = split * bchunk + w; b < b_end; b += 4) {
        const int64_t row = (int64_t)b * ntok + tk;
        const int64_t prow = (int64_t)b * (ntok - 1) + tk - 1;           // used for tk > 0 only
        float v[4][4];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = c * 256 + lane * 4;
            v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.f;
            if (e < D) {
                if (tk == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[c][i] = cls[e + i] + base[c][i];
                } else {
                    const uint2 p = *(const uint2*)(patch + prow * D + e);
                    v[c][0] = lo2f(p.x) + base[c][0]; v[c][1] = hi2f(p.x) + base[c][1];
                    v[c][2] = lo2f(p.y) + base[c][2]; v[c][3] = hi2f(p.y) + base[c][3];
                }
                s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
            }
        }
        const float mean = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = c * 256 + lane * 4;
            if (e < D) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float d = v[c][i] - mean; q += d * d; }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
        float gv[4][4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = c * 256 + lane * 4;
            if (e < D) {
                const f32x4_t dy = *(const f32x4_t*)(dx + row * D + e);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float xh = (v[c][i] - mean) * rstd;
                    gv[c][i] = dy[i] * g[c][i];
                    s1 += gv[c][i]; s2 += gv[c][i] * xh;
                    ag[c][i] += dy[i] * xh; ab[c][i] += dy[i];
                    v[c][i] = xh;
                }
            }
        }
        s1 = wave_sum(s1) / (float)D; s2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = c * 256 + lane * 4;
            if (e < D) {
                float dv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { dv[i] = rstd * (gv[c][i] - s1 - v[c][i] * s2); ap[c][i] += dv[i]; }
                if (tk > 0) {
                    uint2 o; o.x = pack2bf(dv[0], dv[1]); o.y = pack2bf(dv[2], dv[3]);
                    *(uint2*)(dpatch + prow * D + e) = o;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int e = c * 256 + lane * 4;
        if (e < D) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { red[0][w][e + i] = ap[c][i]; red[1][w][e + i] = ag[c][i]; red[2][w][e + i] = ab[c][i]; }
        }
    }
    __syncthreads();
    float* out = ws + ((int64_t)split * ntok + tk) * 3 * D;
    for (int c = threadIdx.x; c < D; c += 256) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[(int64_t)j * D + c] = (red[j][0][c] + red[j][1][c]) + (red[j][2][c] + red[j][3][c]);
    }
}

// Fixed-order finish.  blockIdx.y < ntok: dpos[y] = sum over the splits of their dpos partial; y == ntok / ntok + 1: dgamma / dbeta = sum over every
// (split, token) partial row, four interleaved running sums combined as (a0 + a1) + (a2 + a3).
__global__ __launch_bounds__(256) void vit_embed_bwd_finish_kernel(const float* __restrict__ ws, float* __restrict__ dpos, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, int nsplit, int ntok, int D) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    const int y = blockIdx.y;
    if (y < ntok) {
        float a = 0.f;
        for (int s = 0; s < nsplit; ++s) a += ws[(((int64_t)s * ntok + y) * 3 + 0) * D + c];
        dpos[(int64_t)y * D + c] = a;
        return;
    }
    const int j = y - ntok + 1;                            // 1: dgamma, 2: dbeta
    const int nrows = nsplit * ntok;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < nrows; r += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (r + k < nrows) a[k] += ws[(((int64_t)(r + k)) * 3 + j) * D + c];
    }
    (j == 1 ? dgamma : dbeta)[c] = (a[0] + a[1]) + (a[2] + a[3]);
}

int vit_embed_bwd_splits(int B, int ntok) {                // ~512 blocks, at least 4 batch entries (one per wave) per block
    int s = 512 / ntok;
    if (s > (B + 3) / 4) s = (B + 3) / 4;
    return s < 1 ? 1 : s;
}

}  // namespace

extern "C" int sc_quickgelu_bwd_bf16(const void* u, const void* dh, void* du, int64_t n, void* stream) {
    if (n <= 0) return 0;
    SC_CHECK_ARG(u && dh && du, "sc_quickgelu_bwd_bf16: null operand");
    SC_CHECK_ARG((((uintptr_t)u | (uintptr_t)dh | (uintptr_t)du) & 1) == 0, "sc_quickgelu_bwd_bf16: operands must be 2-byte aligned");
    const uintptr_t mu = (uintptr_t)u & 15;
    int64_t head = n;                                      // no common 16-byte phase: every element goes one by one
    if (((uintptr_t)dh & 15) == mu && ((uintptr_t)du & 15) == mu) head = (int64_t)(((16 - mu) & 15) / 2);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 8, threads = nvec + (n - nvec * 8);
    SC_CHECK_ARG((threads + 255) / 256 <= 0x7fffffff, "sc_quickgelu_bwd_bf16: n=%lld too large", (long long)n);
    hipLaunchKernelGGL(quickgelu_bwd_bf16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)u,
                       (const bf16_t*)dh, (bf16_t*)du, n, head, nvec);
    SC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t sc_vit_embed_bwd_workspace_bytes(int B, int ntok, int D) {
    if (B <= 0 || ntok <= 0 || D <= 0) return 0;
    return (int64_t)vit_embed_bwd_splits(B, ntok) * ntok * 3 * D * 4;
}

extern "C" int sc_vit_embed_bwd(const float* dx, const void* patch, const float* cls, const float* pos, const float* gamma, void* dpatch, float* dpos,
                                float* dgamma, float* dbeta, float* workspace, int B, int ntok, int D, float eps, void* stream) {
    SC_CHECK_ARG(dx && patch && cls && pos && gamma && dpatch && dpos && dgamma && dbeta && workspace, "sc_vit_embed_bwd: null operand");
    SC_CHECK_ARG(B > 0 && ntok >= 2 && ntok <= 65535 && D > 0 && D <= 1024 && D % 4 == 0, "sc_vit_embed_bwd: bad sizes B=%d ntok=%d D=%d (D %% 4 == 0, <= 1024)", B,
                 ntok, D);
    // cls / pos / gamma are read element by element: parameters may be views at any 4-byte offset of an optimizer's flat buffer
    SC_CHECK_ARG(((uintptr_t)dx & 15) == 0 && (((uintptr_t)patch | (uintptr_t)dpatch) & 7) == 0,
                 "sc_vit_embed_bwd: dx must be 16-byte aligned, patch and dpatch 8-byte aligned");
    const int nsplit = vit_embed_bwd_splits(B, ntok);
    const int bchunk = (B + nsplit - 1) / nsplit;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vit_embed_bwd_kernel, dim3(ntok, nsplit), dim3(256), 0, s, dx, (const bf16_t*)patch, cls, pos, gamma, (bf16_t*)dpatch, workspace, B, ntok,
                       D, eps, bchunk);
    SC_CHECK_LAUNCH();
    hipLaunchKernelGGL(vit_embed_bwd_finish_kernel, dim3((D + 255) / 256, ntok + 2), dim3(256), 0, s, (const float*)workspace, dpos, dgamma, dbeta, nsplit, ntok, D);
    SC_CHECK_LAUNCH();
    return 0;
}
