// Image side of the data hand-over, geometry included: CLIP's `_transform` = Resize(n_px, BICUBIC) -> CenterCrop(n_px) -> convert("RGB") -> ToTensor ->
// Normalize for a RAGGED batch of decoded 8-bit images (RGB or L, every image its own size), so that a batch crosses PCIe as the decoded bytes and nothing
// but the decode stays on the host.
//
// BYTE-EXACTNESS CONTRACT.  Pillow's 8-bit resampler is an integer algorithm once the per-axis coefficient tables exist: int32 weights with 22 fractional
// bits, acc = 2^21 + sum_k pix[xmin + k] * coef[k] in int32, out = clamp(acc >> 22, 0, 255) (arithmetic shift), horizontal pass first, vertical pass on the
// uint8 result of the horizontal one.  The tables come from the host (speechclip_amd/data/image_transforms.py: resample_coeffs / clip_window_plan, checked
// byte for byte against the installed Pillow); the kernels below execute them with integer arithmetic only, so the uint8 crop equals PIL's on every byte and
// is bitwise reproducible.  Only BICUBIC on 8-bit RGB / L images is restated: every other PIL mode is resized on the host and arrives here as an
// n_px x n_px RGB image (no pass runs).  The f32 output applies image_normalize_kernel's expression (frontend.hip) to those bytes, so it equals
// sc_image_normalize_u8 of the crop bit for bit.
//
// Only the crop window is computed: the horizontal pass produces the window's columns of the input rows [row0, row1] the window's rows need (uint8, caller's
// workspace), the vertical pass + normalise reads them.  An image without a horizontal pass has no workspace share: its second kernel reads the packed input.
// Every output element is written exactly once; no atomics; no host synchronisation; both launches go to the caller's stream.
#include "common.h"
#include "../../include/speechclip_hip.h"

namespace {

constexpr int G = SC_IMAGE_PREP_GEOM;          // int32 fields per image
enum { G_W = 0, G_H, G_C, G_LEFT, G_TOP, G_ROW0, G_ROW1, G_PASSES, G_HTAB, G_VTAB };
constexpr int PREC = 22;                       // fractional bits of a coefficient

// a table at int32 index t of `tables`: in_size, out_size, ksize, bounds[out][2] = (first input pixel, taps), coef[out][ksize]
struct Table {
    const int32_t* bounds;
    const int32_t* coef;
    int ksize;
};
__host__ __device__ __forceinline__ Table table_at(const int32_t* tables, int t) {
    const int32_t* p = tables + t;
    return Table{p + 3, p + 3 + 2 * (int64_t)p[1], p[2]};
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PREC, 0), 255); }

// one thread = one pixel (all C channels) of the horizontal pass: row r in [row0, row1], window column x
__global__ __launch_bounds__(256) void image_prep_h_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ in_off,
                                                           const int64_t* __restrict__ ws_off, const int32_t* __restrict__ geom,
                                                           const int32_t* __restrict__ tables, uint8_t* __restrict__ ws, int n) {
    const int b = blockIdx.y;
    const int32_t* g = geom + (int64_t)b * G;
    if (!(g[G_PASSES] & SC_IMAGE_PREP_HPASS)) return;
    const int rows = g[G_ROW1] - g[G_ROW0] + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * n) return;
    const int r = (int)(idx / n), x = (int)(idx - (int64_t)r * n);
    const int w = g[G_W], C = g[G_C];
    const Table t = table_at(tables, g[G_HTAB]);
    const int xx = g[G_LEFT] + x;
    const int xmin = t.bounds[2 * xx], cnt = t.bounds[2 * xx + 1];
    const int32_t* k = t.coef + (int64_t)xx * t.ksize;
    const uint8_t* src = packed + in_off[b] + ((int64_t)(g[G_ROW0] + r) * w + xmin) * C;
    uint8_t* dst = ws + ws_off[b] + idx * C;
    if (C == 3) {
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < cnt; ++i) {
            const int kv = k[i];
            a0 += (int)src[3 * i] * kv;
            a1 += (int)src[3 * i + 1] * kv;
            a2 += (int)src[3 * i + 2] * kv;
        }
        dst[0] = (uint8_t)clip8(a0);
        dst[1] = (uint8_t)clip8(a1);
        dst[2] = (uint8_t)clip8(a2);
    } else {
        int a0 = 1 << (PREC - 1);
        for (int i = 0; i < cnt; ++i) a0 += (int)src[i] * k[i];
        dst[0] = (uint8_t)clip8(a0);
    }
}

// one thread = one output pixel (y, x) of the window: vertical pass (or a plain read) on the first stage's bytes, then ToTensor + Normalize
__global__ __launch_bounds__(256) void image_prep_v_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ in_off,
                                                           const int64_t* __restrict__ ws_off, const int32_t* __restrict__ geom,
                                                           const int32_t* __restrict__ tables, const uint8_t* __restrict__ ws, int n, float m0, float m1,
                                                           float m2, float is0, float is1, float is2, float* __restrict__ out,
                                                           uint8_t* __restrict__ out_u8) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int y = idx / n, x = idx - y * n;
    const int32_t* g = geom + (int64_t)b * G;
    const int C = g[G_C], passes = g[G_PASSES];
    // the first stage's image: the workspace rows [row0, row1] x window columns, or the packed input itself
    const uint8_t* base;
    int64_t ld;          // bytes per row
    int rbase, col;
    if (passes & SC_IMAGE_PREP_HPASS) {
        base = ws + ws_off[b]; ld = (int64_t)n * C; rbase = g[G_ROW0]; col = x;
    } else {
        base = packed + in_off[b]; ld = (int64_t)g[G_W] * C; rbase = 0; col = g[G_LEFT] + x;
    }
    const int yy = g[G_TOP] + y;
    int p0, p1, p2;
    if (passes & SC_IMAGE_PREP_VPASS) {
        const Table t = table_at(tables, g[G_VTAB]);
        const int ymin = t.bounds[2 * yy], cnt = t.bounds[2 * yy + 1];
        const int32_t* k = t.coef + (int64_t)yy * t.ksize;
        const uint8_t* src = base + (int64_t)(ymin - rbase) * ld + (int64_t)col * C;
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        if (C == 3) {
            for (int i = 0; i < cnt; ++i) {
                const int kv = k[i];
                const uint8_t* s = src + i * ld;
                a0 += (int)s[0] * kv;
                a1 += (int)s[1] * kv;
                a2 += (int)s[2] * kv;
            }
            p0 = clip8(a0); p1 = clip8(a1); p2 = clip8(a2);
        } else {
            for (int i = 0; i < cnt; ++i) a0 += (int)src[i * ld] * k[i];
            p0 = p1 = p2 = clip8(a0);
        }
    } else {
        const uint8_t* s = base + (int64_t)(yy - rbase) * ld + (int64_t)col * C;
        p0 = s[0];
        p1 = C == 3 ? s[1] : p0;
        p2 = C == 3 ? s[2] : p0;
    }
    const int64_t npix = (int64_t)n * n;
    if (out_u8) {
        uint8_t* o8 = out_u8 + ((int64_t)b * npix + idx) * 3;
        o8[0] = (uint8_t)p0; o8[1] = (uint8_t)p1; o8[2] = (uint8_t)p2;
    }
    float* o = out + (int64_t)b * 3 * npix + idx;
    o[0] = ((float)p0 / 255.0f - m0) * is0;          // image_normalize_kernel's expression: same bytes, same bits
    o[npix] = ((float)p1 / 255.0f - m1) * is1;
    o[2 * npix] = ((float)p2 / 255.0f - m2) * is2;
}

inline int64_t ws_share(const int32_t* g, int n) {
    return (g[G_PASSES] & SC_IMAGE_PREP_HPASS) ? ((int64_t)g[G_ROW1] - g[G_ROW0] + 1) * n * g[G_C] : 0;
}

// every table entry a kernel will read for outputs [first, first + n) of a pass in_size -> (table's out_size): inside the table buffer, inside the image
int check_table(const int32_t* tables, int64_t tables_len, int t, int in_size, int first, int n, int lo, int hi, const char* axis, int b) {
    SC_CHECK_ARG(tables, "sc_image_prep_u8: tables is null but image %d runs the %s pass", b, axis);
    SC_CHECK_ARG(t >= 0 && (int64_t)t + 3 <= tables_len, "sc_image_prep_u8: image %d: %s table index %d outside tables[0, %lld)", b, axis, t, (long long)tables_len);
    const int32_t* p = tables + t;
    const int64_t out = p[1], ks = p[2];
    SC_CHECK_ARG(p[0] == in_size && out > 0 && ks > 0 && (int64_t)t + 3 + out * (2 + ks) <= tables_len,
                 "sc_image_prep_u8: image %d: %s table at %d (in %d, out %lld, ksize %lld) does not fit the image (%d) or tables[0, %lld)", b, axis, t, p[0],
                 (long long)out, (long long)ks, in_size, (long long)tables_len);
    SC_CHECK_ARG(first >= 0 && (int64_t)first + n <= out, "sc_image_prep_u8: image %d: window [%d, %d) does not lie inside the resized image (%s size %lld)", b,
                 first, first + n, axis, (long long)out);
    const Table tb = table_at(tables, t);
    for (int i = first; i < first + n; ++i) {
        const int64_t mn = tb.bounds[2 * i], cnt = tb.bounds[2 * i + 1];
        SC_CHECK_ARG(cnt >= 0 && cnt <= ks && mn >= lo && mn + cnt - 1 <= hi,
                     "sc_image_prep_u8: image %d: %s bounds of output %d = (%lld, %lld) leave [%d, %d] or exceed ksize %lld", b, axis, i, (long long)mn,
                     (long long)cnt, lo, hi, (long long)ks);
    }
    return 0;
}

}  // namespace

extern "C" int64_t sc_image_prep_workspace_bytes(const int32_t* geom, int B, int n_px) {
    if (B == 0) return 0;
    if (!geom || B < 0 || n_px <= 0) return -1;
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + (int64_t)b * G;
        if (g[G_ROW1] < g[G_ROW0] || (g[G_C] != 1 && g[G_C] != 3)) return -1;
        total += ws_share(g, n_px);
    }
    return total;
}

extern "C" int sc_image_prep_u8(const void* packed, int64_t packed_bytes, const int64_t* offsets_host, const int64_t* offsets, const int32_t* geom_host,
                                const int32_t* geom, const int32_t* tables_host, const int32_t* tables, int64_t tables_len, int B, int n_px,
                                const float* mean3, const float* std3, void* workspace, int64_t workspace_bytes, float* out_chw, void* out_u8, void* stream) {
    SC_CHECK_ARG(B >= 0, "sc_image_prep_u8: B=%d is negative", B);
    SC_CHECK_ARG(n_px > 0 && n_px <= 16384, "sc_image_prep_u8: n_px=%d must be in [1, 16384]", n_px);
    SC_CHECK_ARG(mean3 && std3 && std3[0] > 0.f && std3[1] > 0.f && std3[2] > 0.f, "sc_image_prep_u8: mean3 / std3 are null or std is not positive");
    if (B == 0) return 0;
    SC_CHECK_ARG(packed && offsets_host && offsets && geom_host && geom && out_chw, "sc_image_prep_u8: packed, offsets, geom or out_chw is null");
    SC_CHECK_ARG((tables_host == nullptr) == (tables == nullptr), "sc_image_prep_u8: tables needs its host and its device copy, or neither");
    const int n = n_px;
    int64_t ws_need = 0, max_rows = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom_host + (int64_t)b * G;
        const int w = g[G_W], h = g[G_H], C = g[G_C], left = g[G_LEFT], top = g[G_TOP], row0 = g[G_ROW0], row1 = g[G_ROW1], passes = g[G_PASSES];
        SC_CHECK_ARG(C == 1 || C == 3, "sc_image_prep_u8: image %d: C=%d (1 = L and 3 = RGB are supported)", b, C);
        SC_CHECK_ARG(w > 0 && h > 0, "sc_image_prep_u8: image %d: w=%d h=%d", b, w, h);
        SC_CHECK_ARG((passes & ~(SC_IMAGE_PREP_HPASS | SC_IMAGE_PREP_VPASS)) == 0, "sc_image_prep_u8: image %d: unknown passes bits 0x%x", b, passes);
        const int64_t in0 = offsets_host[b], in_bytes = (int64_t)w * h * C;
        SC_CHECK_ARG(in0 >= 0 && in0 + in_bytes <= packed_bytes, "sc_image_prep_u8: image %d: offsets %lld + %lld bytes outside packed[0, %lld)", b, (long long)in0,
                     (long long)in_bytes, (long long)packed_bytes);
        SC_CHECK_ARG(row0 >= 0 && row0 <= row1 && row1 < h, "sc_image_prep_u8: image %d: needed rows [%d, %d] outside [0, %d)", b, row0, row1, h);
        if (passes & SC_IMAGE_PREP_HPASS) {
            if (int rc = check_table(tables_host, tables_len, g[G_HTAB], w, left, n, 0, w - 1, "horizontal", b)) return rc;
        } else {
            SC_CHECK_ARG(left >= 0 && (int64_t)left + n <= w, "sc_image_prep_u8: image %d: window [%d, %d) does not lie inside the resized image (width %d)", b, left,
                         left + n, w);
        }
        if (passes & SC_IMAGE_PREP_VPASS) {
            if (int rc = check_table(tables_host, tables_len, g[G_VTAB], h, top, n, row0, row1, "vertical", b)) return rc;
        } else {
            SC_CHECK_ARG(top >= 0 && (int64_t)top + n <= h, "sc_image_prep_u8: image %d: window [%d, %d) does not lie inside the resized image (height %d)", b, top,
                         top + n, h);
            SC_CHECK_ARG(row0 <= top && top + n - 1 <= row1, "sc_image_prep_u8: image %d: needed rows [%d, %d] do not cover the window's rows [%d, %d]", b, row0,
                         row1, top, top + n - 1);
        }
        // the workspace shares lie back to back in batch order
        SC_CHECK_ARG(offsets_host[B + b] == ws_need, "sc_image_prep_u8: image %d: workspace offset %lld, expected %lld (shares are packed in batch order)", b,
                     (long long)offsets_host[B + b], (long long)ws_need);
        const int64_t share = ws_share(g, n);
        ws_need += share;
        if (share) max_rows = max_rows > (int64_t)row1 - row0 + 1 ? max_rows : (int64_t)row1 - row0 + 1;
    }
    SC_CHECK_ARG(workspace_bytes >= ws_need && (ws_need == 0 || workspace), "sc_image_prep_u8: workspace of %lld bytes (%s), sc_image_prep_workspace_bytes = %lld",
                 (long long)workspace_bytes, workspace ? "non-null" : "null", (long long)ws_need);
    SC_CHECK_ARG(B <= 65535, "sc_image_prep_u8: B=%d exceeds 65535 images per call", B);
    const int64_t hblocks = (max_rows * n + 255) / 256;
    SC_CHECK_ARG(hblocks <= 0x7fffffff, "sc_image_prep_u8: %lld needed rows x n_px=%d is too large for one launch", (long long)max_rows, n);
    const uint8_t* pk = (const uint8_t*)packed;
    if (hblocks > 0) {
        hipLaunchKernelGGL(image_prep_h_kernel, dim3((unsigned)hblocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, pk, offsets, offsets + B, geom, tables,
                           (uint8_t*)workspace, n);
        SC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(image_prep_v_kernel, dim3((unsigned)(((int64_t)n * n + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, pk, offsets,
                       offsets + B, geom, tables, (const uint8_t*)workspace, n, mean3[0], mean3[1], mean3[2], 1.0f / std3[0], 1.0f / std3[1], 1.0f / std3[2], out_chw,
                       (uint8_t*)out_u8);
    SC_CHECK_LAUNCH();
    return 0;
}
