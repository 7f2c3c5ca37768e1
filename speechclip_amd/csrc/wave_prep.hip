// Audio side of the data hand-over: raw PCM of a RAGGED batch (int16 or f32, mono or stereo, every utterance its own rate) -> f32 [B, Lout] at the model's
// rate in one launch: sample conversion, mono mix, rational-ratio polyphase resampling, the train-mode crop window, zero right-padding.
//
// ARITHMETIC CONTRACT (include/speechclip_hip.h; speechclip_amd/data/audio_transforms.py restates it and executes it in float64 for the tests).
//   mono f32 sample  int16: (float)(sum_c s_c) * (1.0f / (C * 32768)) -- exact in f32 for C in {1, 2};  f32: s, or (s_0 + s_1) * 0.5f
//   identity rate    y[n] = x[n]: no table, no LDS, the bits of the input
//   resampled        u = n * M, j0 = u div L, p = u mod L;  y[n] = sum_k taps[p][k] * x[first + k],  first = j0 - d_hi(p), k < count(p), x = 0 outside
//                    [0, frames); d_hi(p) = floor((W - p) / L), count(p) = d_hi(p) + floor((W + p) / L) + 1 with W = 320 max(L, M) / 17, all in integers;
//                    one thread sums one output in fp32 in ascending k.
// One block = (utterance, segment of seg_outputs(L, M) consecutive outputs): the segment's input span is decoded and mixed ONCE into LDS as f32 (consecutive
// lanes read consecutive frames: coalesced), then every thread produces outputs lane-consecutively (a wave stores 256 contiguous bytes; its LDS reads are
// M / L words apart, its table rows come through L2: a table is at most 256 KiB and shared by every block of its rate).  Only the crop window is computed;
// every output element is written exactly once; no atomics; no host synchronisation; one launch on the caller's stream.
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

constexpr int G = SC_WAVE_PREP_GEOM;          // int64 fields per utterance
enum { G_FRAMES = 0, G_C, G_FMT, G_L, G_M, G_K, G_TABLE, G_START, G_LEN };
constexpr int THREADS = 256;
constexpr int SPAN = 8192;                    // f32 input samples one block stages in LDS (32 KiB)
constexpr int SEG_MAX = 2048;                 // outputs per block at most (and at identity rate)
constexpr int64_t MAX_FRAMES = (int64_t)1 << 40, MAX_RATIO = (int64_t)1 << 20;          // frames * L and n * M stay far inside int64

// the support |t| <= W = 320 max(L, M) / 17 in integers: 17 |p + d L| <= 320 max(L, M)
__host__ __device__ __forceinline__ int64_t wnum(int64_t L, int64_t M) { return 320 * (L > M ? L : M); }
__host__ __device__ __forceinline__ int64_t d_hi(int64_t p, int64_t L, int64_t wn) { return (wn - 17 * p) / (17 * L); }          // inputs before j0
__host__ __device__ __forceinline__ int64_t d_fwd(int64_t p, int64_t L, int64_t wn) { return (wn + 17 * p) / (17 * L); }         // inputs after j0
// outputs per block: the largest multiple of 64 (at most SEG_MAX) whose input span, j0(last) - j0(first) + 1 + d_hi(0) + d_fwd(L - 1)
// <= floor((seg - 1) M / L) + 2 + d_hi(0) + d_fwd(L - 1), fits SPAN; 0 when even 64 outputs do not fit
__host__ __device__ __forceinline__ int seg_outputs(int64_t L, int64_t M) {
    const int64_t wn = wnum(L, M);
    const int64_t avail = SPAN - 2 - d_hi(0, L, wn) - d_fwd(L - 1, L, wn);
    if (avail < 0) return 0;
    int64_t seg = avail * L / M + 1;
    seg = seg > SEG_MAX ? SEG_MAX : seg;
    return (int)(seg / 64 * 64);
}

__device__ __forceinline__ float load_mono(const uint8_t* __restrict__ src, int64_t j, int C, int fmt) {
    if (fmt == SC_WAVE_PREP_I16) {
        const int16_t* s = (const int16_t*)src;
        if (C == 1) return (float)(int)s[j] * (1.0f / 32768.0f);
        return (float)((int)s[2 * j] + (int)s[2 * j + 1]) * (1.0f / 65536.0f);
    }
    const float* s = (const float*)src;
    if (C == 1) return s[j];
    return (s[2 * j] + s[2 * j + 1]) * 0.5f;
}

__global__ __launch_bounds__(THREADS) void wave_prep_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ geom, const float* __restrict__ tables, float* __restrict__ out,
                                                            int64_t ld, int64_t Lout) {
    __shared__ float xs[SPAN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t* g = geom + (int64_t)b * G;
    const int64_t frames = g[G_FRAMES], L = g[G_L], M = g[G_M], K = g[G_K], table = g[G_TABLE], start = g[G_START], len = g[G_LEN];
    const int C = (int)g[G_C], fmt = (int)g[G_FMT];
    const bool ident = table < 0;
    const int seg = ident ? SEG_MAX : seg_outputs(L, M);
    const int64_t jb = (int64_t)blockIdx.x * seg;
    if (jb >= Lout) return;
    const int64_t je = jb + seg < Lout ? jb + seg : Lout;          // this block writes out[b, jb .. je)
    const int64_t jv = je < len ? je : len;                        // ... of which [jb, jv) are samples and [jv, je) padding
    const uint8_t* src = packed + offsets[b];
    float* row = out + (int64_t)b * ld;
    if (ident) {
        for (int64_t j = jb + tid; j < je; j += THREADS) row[j] = j < jv ? load_mono(src, start + j, C, fmt) : 0.0f;
        return;
    }
    const int64_t wn = wnum(L, M);
    int64_t js = 0;
    if (jb < jv) {          // block-uniform: stage the inputs the outputs [jb, jv) read, zeros outside the utterance
        js = (start + jb) * M / L - d_hi(0, L, wn);
        const int64_t jlast = (start + jv - 1) * M / L + d_fwd(L - 1, L, wn);
        const int cnt = (int)(jlast - js + 1);                     // <= SPAN by seg_outputs
        for (int i = tid; i < cnt; i += THREADS) {
            const int64_t j = js + i;
            xs[i] = (j < 0 || j >= frames) ? 0.0f : load_mono(src, j, C, fmt);
        }
        __syncthreads();
    }
    for (int64_t j = jb + tid; j < je; j += THREADS) {
        float acc = 0.0f;
        if (j < jv) {
            const int64_t u = (start + j) * M, j0 = u / L, p = u - j0 * L;
            const int64_t dh = d_hi(p, L, wn);
            const int cnt = (int)(dh + d_fwd(p, L, wn) + 1);
            const float* x = xs + (j0 - dh - js);
            const float* t = tables + table + p * K;
            for (int k = 0; k < cnt; ++k) acc += t[k] * x[k];
        }
        row[j] = acc;
    }
}

int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t r = a % b; a = b; b = r; }
    return a;
}

}  // namespace

extern "C" int sc_wave_prep(const void* packed, int64_t packed_bytes, const int64_t* offsets_host, const int64_t* offsets, const int64_t* geom_host,
                            const int64_t* geom, const float* tables_host, const float* tables, int64_t tables_len, int B, float* out, int64_t ld,
                            int64_t Lout, void* stream) {
    SC_CHECK_ARG(B >= 0, "sc_wave_prep: B=%d is negative", B);
    SC_CHECK_ARG(Lout >= 0 && ld >= Lout, "sc_wave_prep: Lout=%lld, ld=%lld: need 0 <= Lout <= ld", (long long)Lout, (long long)ld);
    SC_CHECK_ARG(packed_bytes >= 0 && tables_len >= 0, "sc_wave_prep: packed_bytes=%lld or tables_len=%lld is negative", (long long)packed_bytes, (long long)tables_len);
    if (B == 0) return 0;
    SC_CHECK_ARG(offsets_host && offsets && geom_host && geom, "sc_wave_prep: offsets or geom is null");
    SC_CHECK_ARG((tables_host == nullptr) == (tables == nullptr), "sc_wave_prep: tables needs its host and its device copy, or neither");
    SC_CHECK_ARG(B <= 65535, "sc_wave_prep: B=%d exceeds 65535 utterances per call", B);
    int64_t blocks = 0, kL = 0, kM = 0, kK = 0;          // kK = tap count of the ratio kL / kM (computed once per run of equal ratios)
    for (int b = 0; b < B; ++b) {
        const int64_t* g = geom_host + (int64_t)b * G;
        const int64_t frames = g[G_FRAMES], C = g[G_C], fmt = g[G_FMT], L = g[G_L], M = g[G_M], K = g[G_K], table = g[G_TABLE], start = g[G_START], len = g[G_LEN];
        SC_CHECK_ARG(C == 1 || C == 2, "sc_wave_prep: utterance %d: C=%lld (1 = mono and 2 = stereo are supported)", b, (long long)C);
        SC_CHECK_ARG(fmt == SC_WAVE_PREP_I16 || fmt == SC_WAVE_PREP_F32, "sc_wave_prep: utterance %d: fmt=%lld (0 = int16 and 1 = f32 are supported)", b, (long long)fmt);
        SC_CHECK_ARG(frames >= 0 && frames <= MAX_FRAMES, "sc_wave_prep: utterance %d: frames=%lld outside [0, 2^40]", b, (long long)frames);
        SC_CHECK_ARG(L > 0 && M > 0 && L <= MAX_RATIO && M <= MAX_RATIO && gcd64(L, M) == 1,
                     "sc_wave_prep: utterance %d: ratio L/M = %lld/%lld must be positive, reduced (coprime) and below 2^20", b, (long long)L, (long long)M);
        const int64_t n_out = (frames * L + M - 1) / M;
        SC_CHECK_ARG(start >= 0 && len >= 0 && start <= n_out && len <= n_out - start, "sc_wave_prep: utterance %d: window [%lld, %lld + %lld) outside [0, n_out = %lld]", b,
                     (long long)start, (long long)start, (long long)len, (long long)n_out);
        SC_CHECK_ARG(len <= Lout, "sc_wave_prep: utterance %d: len=%lld exceeds Lout=%lld", b, (long long)len, (long long)Lout);
        const int64_t fb = C * (fmt == SC_WAVE_PREP_I16 ? 2 : 4), o = offsets_host[b];
        SC_CHECK_ARG(o >= 0 && o % fb == 0 && o <= packed_bytes && frames * fb <= packed_bytes - o,
                     "sc_wave_prep: utterance %d: offset %lld (frame size %lld) + %lld bytes outside packed[0, %lld) or misaligned", b, (long long)o, (long long)fb,
                     (long long)(frames * fb), (long long)packed_bytes);
        SC_CHECK_ARG(packed || frames == 0, "sc_wave_prep: packed is null");
        int seg = SEG_MAX;
        if (L == 1 && M == 1) {
            SC_CHECK_ARG(table == -1 && K == 0, "sc_wave_prep: utterance %d: identity rate takes table = -1 and K = 0, got table=%lld K=%lld", b, (long long)table, (long long)K);
        } else {
            SC_CHECK_ARG(tables_host, "sc_wave_prep: tables is null but utterance %d resamples by %lld/%lld", b, (long long)L, (long long)M);
            SC_CHECK_ARG(K > 0 && L * K <= SC_WAVE_PREP_MAX_TABLE, "sc_wave_prep: utterance %d: the tap table of ratio %lld/%lld has %lld x %lld entries, over the cap of %d",
                         b, (long long)L, (long long)M, (long long)L, (long long)K, SC_WAVE_PREP_MAX_TABLE);
            if (L != kL || M != kM) {
                const int64_t wn = wnum(L, M);
                kL = L; kM = M; kK = 0;
                for (int64_t p = 0; p < L; ++p) {
                    const int64_t c = d_hi(p, L, wn) + d_fwd(p, L, wn) + 1;
                    kK = c > kK ? c : kK;
                }
            }
            SC_CHECK_ARG(K == kK, "sc_wave_prep: utterance %d: K=%lld, but the support of ratio %lld/%lld has %lld taps", b, (long long)K, (long long)L, (long long)M, (long long)kK);
            SC_CHECK_ARG(table >= 0 && table <= tables_len && L * K <= tables_len - table, "sc_wave_prep: utterance %d: table index %lld + %lld x %lld entries outside tables[0, %lld)",
                         b, (long long)table, (long long)L, (long long)K, (long long)tables_len);
            seg = seg_outputs(L, M);
            SC_CHECK_ARG(seg >= 64, "sc_wave_prep: utterance %d: ratio %lld/%lld decimates too steeply for one block's input span (%d samples)", b, (long long)L, (long long)M, SPAN);
        }
        const int64_t nb = (Lout + seg - 1) / seg;
        blocks = nb > blocks ? nb : blocks;
    }
    if (Lout == 0) return 0;
    SC_CHECK_ARG(out, "sc_wave_prep: out is null");
    SC_CHECK_ARG(blocks <= 0x7fffffff, "sc_wave_prep: Lout=%lld is too large for one launch", (long long)Lout);
    hipLaunchKernelGGL(wave_prep_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, (const uint8_t*)packed, offsets, geom, tables, out,
                       ld, Lout);
    SC_CHECK_LAUNCH();
    return 0;
}
