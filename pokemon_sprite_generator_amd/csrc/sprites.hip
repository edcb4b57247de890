// Sprite batches from the device-resident dataset: gather + augmentation + normalisation in one pass
// (psg_sprite_contrast_mean, psg_sprite_augment; the parameter row is described in include/psg_hip.h), and the batch's
// text inputs gathered from the resident token table (psg_token_batch).
//
// Every float expression below is written once, in the order tests/sprite_ref.py restates it, and the build has
// contraction off: the fp32 evaluation of that restatement and these kernels then differ only where a sum is ordered
// differently (the contrast mean).
#include "psg_common.h"

namespace {

using namespace psg;

constexpr int NP = PSG_SPRITE_PARAMS;
constexpr int AUG_THREADS = 256;     // one output pixel per lane, consecutive lanes consecutive pixels of a row: the three plane stores coalesce
constexpr int MEAN_THREADS = 1024;   // one block per image: 46225 pixels at S = 215, 45-46 per lane
constexpr int TOK_THREADS = 256;     // one token per lane, consecutive lanes consecutive positions: both int64 stores coalesce

// the 24 orders of (0 brightness, 1 contrast, 2 saturation, 3 hue), lexicographic; entry k of an order in bits 2k..2k+1
__device__ const unsigned char kOrders[24] = {
    0xE4, 0xB4, 0xD8, 0x78, 0x9C, 0x6C, 0xE1, 0xB1, 0xC9, 0x39, 0x8D, 0x2D,
    0xD2, 0x72, 0xC6, 0x36, 0x4E, 0x1E, 0x93, 0x63, 0x87, 0x27, 0x4B, 0x1B};

struct Row {
    float a, b, c, d, e, f;      // inverse rotation
    float fb, fc, fs, fh;        // brightness, contrast, saturation, hue
    int flip, order;
    int ci, cj, ch, cw;          // crop box
};

__device__ __forceinline__ Row load_row(const float* p) {
    Row r;
    r.flip = p[0] != 0.f;
    r.a = p[1]; r.b = p[2]; r.c = p[3]; r.d = p[4]; r.e = p[5]; r.f = p[6];
    const int code = (int)p[7];
    r.order = kOrders[code < 0 ? 0 : (code > 23 ? 23 : code)];
    r.fb = p[8]; r.fc = p[9]; r.fs = p[10]; r.fh = p[11];
    r.ci = (int)p[12]; r.cj = (int)p[13]; r.ch = (int)p[14]; r.cw = (int)p[15];
    return r;
}

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }
__device__ __forceinline__ float luma(float r, float g, float b) { return (19595.f * r + 38470.f * g + 7471.f * b) / 65536.f; }

// hexcone RGB -> HSV, h <- frac(h + shift), HSV -> RGB; values stay on the 0..255 scale
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float shift) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    if (maxc == minc) return;                      // grey: s = 0, the round trip is the identity
    const float delta = maxc - minc, s = delta / maxc;
    const float rc = (maxc - r) / delta, gc = (maxc - g) / delta, bc = (maxc - b) / delta;
    float h = r == maxc ? bc - gc : (g == maxc ? 2.f + rc - bc : 4.f + gc - rc);
    h = h / 6.f;
    h = h - floorf(h);
    h = h + shift;
    h = h - floorf(h);
    const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
    const int i = (int)fi % 6;                     // (h rounds to 1.0 from just below 0: sector 6 is sector 0)
    const float p = maxc * (1.f - s), q = maxc * (1.f - s * f), t = maxc * (1.f - s * (1.f - f));
    switch (i) {
        case 0: r = maxc; g = t; b = p; break;
        case 1: r = q; g = maxc; b = p; break;
        case 2: r = p; g = maxc; b = t; break;
        case 3: r = p; g = q; b = maxc; break;
        case 4: r = t; g = p; b = maxc; break;
        default: r = maxc; g = p; b = q; break;
    }
}

// The colour ops in this sample's order.  TO_CONTRAST: stop in front of the contrast op (the image its mean is taken of).
template <bool TO_CONTRAST>
__device__ __forceinline__ void colour_ops(const Row& w, float mean, float& r, float& g, float& b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = (w.order >> (2 * k)) & 3;
        if (op == 0) {
            if (w.fb != 1.f) { r = clip255(w.fb * r); g = clip255(w.fb * g); b = clip255(w.fb * b); }
        } else if (op == 1) {
            if (TO_CONTRAST) return;
            if (w.fc != 1.f) {
                r = clip255(mean + w.fc * (r - mean)); g = clip255(mean + w.fc * (g - mean)); b = clip255(mean + w.fc * (b - mean));
            }
        } else if (op == 2) {
            if (w.fs != 1.f) {
                const float l = luma(r, g, b);
                r = clip255(l + w.fs * (r - l)); g = clip255(l + w.fs * (g - l)); b = clip255(l + w.fs * (b - l));
            }
        } else if (w.fh != 0.f) {
            hue_shift(r, g, b, w.fh);
        }
    }
}

// pixel (u, v) of the flipped and rotated image (0 <= u, v < S)
__device__ __forceinline__ void fetch(const uint32_t* img, int S, const Row& w, int u, int v, float& r, float& g, float& b) {
    const float uc = (float)u + 0.5f, vc = (float)v + 0.5f;
    const float xin = w.a * uc + w.b * vc + w.c, yin = w.d * uc + w.e * vc + w.f;
    const float fx = floorf(xin), fy = floorf(yin);
    r = g = b = 0.f;
    if (fx >= 0.f && fx < (float)S && fy >= 0.f && fy < (float)S) {      // (false for NaN coefficients too)
        int sx = (int)fx;
        const int sy = (int)fy;
        if (w.flip) sx = S - 1 - sx;
        const uint32_t px = img[sy * S + sx];
        r = (float)(px & 255u); g = (float)((px >> 8) & 255u); b = (float)((px >> 16) & 255u);
    }
}

__global__ __launch_bounds__(MEAN_THREADS) void sprite_contrast_mean_kernel(const uint32_t* __restrict__ src, int64_t N,
                                                                            const int64_t* __restrict__ idx,
                                                                            const float* __restrict__ params,
                                                                            float* __restrict__ mean, int S) {
    __shared__ float red[16];
    const int bi = blockIdx.x;
    const Row w = load_row(params + (size_t)bi * NP);
    const int64_t n = idx[bi];
    if (w.fc == 1.f || n < 0 || n >= N) {            // block-uniform
        if (threadIdx.x == 0) mean[bi] = w.fc == 1.f ? 0.f : __builtin_nanf("");
        return;
    }
    const uint32_t* img = src + (size_t)n * S * S;
    float acc = 0.f;
    for (int p = threadIdx.x; p < S * S; p += MEAN_THREADS) {
        const int v = p / S, u = p - v * S;
        float r, g, b;
        fetch(img, S, w, u, v, r, g, b);
        colour_ops<true>(w, 0.f, r, g, b);
        acc += luma(r, g, b);
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) mean[bi] = total / (float)(S * S);
}

__global__ __launch_bounds__(AUG_THREADS) void sprite_augment_kernel(const uint32_t* __restrict__ src, int64_t N,
                                                                     const int64_t* __restrict__ idx,
                                                                     const float* __restrict__ params,
                                                                     const float* __restrict__ mean,
                                                                     float* __restrict__ out, int S) {
    const int p = blockIdx.x * AUG_THREADS + threadIdx.x, bi = blockIdx.y;
    if (p >= S * S) return;
    float* o = out + (size_t)bi * 3 * S * S + p;
    const int64_t n = idx[bi];
    if (n < 0 || n >= N) {
        o[0] = o[(size_t)S * S] = o[(size_t)2 * S * S] = __builtin_nanf("");
        return;
    }
    const uint32_t* img = src + (size_t)n * S * S;
    const Row w = load_row(params + (size_t)bi * NP);
    const float m = mean[bi];
    const int y = p / S, x = p - y * S;
    // PIL's BILINEAR up-scale of the crop box: two taps either side of the output pixel's centre, clamped to the box
    const float cx = ((float)x + 0.5f) * (float)w.cw / (float)S - 0.5f, cy = ((float)y + 0.5f) * (float)w.ch / (float)S - 0.5f;
    const float x0f = floorf(cx), y0f = floorf(cy), wx = cx - x0f, wy = cy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    // (clamped to the image as well: a crop box that breaks the contract reads the wrong pixel, never outside the array)
    const int xs[2] = {min(max(min(max(x0, 0), w.cw - 1) + w.cj, 0), S - 1), min(max(min(max(x0 + 1, 0), w.cw - 1) + w.cj, 0), S - 1)};
    const int ys[2] = {min(max(min(max(y0, 0), w.ch - 1) + w.ci, 0), S - 1), min(max(min(max(y0 + 1, 0), w.ch - 1) + w.ci, 0), S - 1)};
    float t[2][2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fetch(img, S, w, xs[i], ys[j], t[j][i][0], t[j][i][1], t[j][i][2]);
            colour_ops<false>(w, m, t[j][i][0], t[j][i][1], t[j][i][2]);
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.f - wx) * t[0][0][c] + wx * t[0][1][c], bot = (1.f - wx) * t[1][0][c] + wx * t[1][1][c];
        const float v = (1.f - wy) * top + wy * bot;
        o[(size_t)c * S * S] = (v / 255.f - 0.5f) / 0.5f;
    }
}

// grid (ceil(S / TOK_THREADS), B): lane s of row b.  A row index outside [0, N) reads nothing and yields an empty row.
__global__ __launch_bounds__(TOK_THREADS) void token_batch_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ lens,
                                                                  int64_t N, int L, const int64_t* __restrict__ idx, int S,
                                                                  int32_t pad_id, int64_t* __restrict__ ids,
                                                                  int64_t* __restrict__ mask, int32_t* __restrict__ kv_len) {
    const int s = blockIdx.x * TOK_THREADS + threadIdx.x, b = blockIdx.y;
    if (s >= S) return;
    const int64_t row = idx[b];
    int n = 0;
    if (row >= 0 && row < N) n = min(max(lens[row], 0), S);       // (S <= L: a length past the table's width never reads past the row)
    const bool real = s < n;
    const size_t o = (size_t)b * S + s;
    ids[o] = real ? (int64_t)table[(size_t)row * L + s] : (int64_t)pad_id;
    mask[o] = real ? 1 : 0;
    if (s == 0) kv_len[b] = n;
}

int check_args(const void* src, int64_t N, const void* idx, const void* params, const void* mean, const void* out, int B, int S,
               const char* what) {
    PSG_REQUIRE(src && idx && params && mean && out, PSG_ERR_ARG, "%s: null pointer", what);
    PSG_REQUIRE(N > 0 && B > 0 && S > 0, PSG_ERR_SHAPE, "%s: N=%lld B=%d S=%d must be positive", what, (long long)N, B, S);
    PSG_REQUIRE(S <= 4096 && B <= 65535, PSG_ERR_SHAPE, "%s: S=%d (max 4096) or B=%d (max 65535) too large", what, S, B);
    PSG_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0, PSG_ERR_ALIGN, "%s: src must be 4-byte aligned", what);
    return PSG_OK;
}

}  // namespace

extern "C" {

int psg_sprite_contrast_mean(const uint8_t* src, int64_t N, const int64_t* idx, const float* params, float* mean, int B, int S,
                             psg_stream_t stream) {
    if (int rc = check_args(src, N, idx, params, mean, mean, B, S, "psg_sprite_contrast_mean")) return rc;
    hipLaunchKernelGGL(sprite_contrast_mean_kernel, dim3(B), dim3(MEAN_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(src), N, idx, params, mean, S);
    PSG_LAUNCH_CHECK("sprite_contrast_mean_kernel");
    return PSG_OK;
}

int psg_sprite_augment(const uint8_t* src, int64_t N, const int64_t* idx, const float* params, const float* mean, float* out, int B,
                       int S, psg_stream_t stream) {
    if (int rc = check_args(src, N, idx, params, mean, out, B, S, "psg_sprite_augment")) return rc;
    hipLaunchKernelGGL(sprite_augment_kernel, dim3((S * S + AUG_THREADS - 1) / AUG_THREADS, B), dim3(AUG_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint32_t*>(src), N, idx, params, mean, out, S);
    PSG_LAUNCH_CHECK("sprite_augment_kernel");
    return PSG_OK;
}

int psg_token_batch(const int32_t* table, const int32_t* lens, int64_t N, int L, const int64_t* idx, int B, int S, int32_t pad_id,
                    int64_t* ids, int64_t* mask, int32_t* kv_len, psg_stream_t stream) {
    PSG_REQUIRE(table && lens && idx && ids && mask && kv_len, PSG_ERR_ARG, "psg_token_batch: null pointer");
    PSG_REQUIRE(N > 0 && L > 0 && B > 0 && S > 0, PSG_ERR_SHAPE, "psg_token_batch: N=%lld L=%d B=%d S=%d must be positive", (long long)N,
                L, B, S);
    PSG_REQUIRE(S <= L && B <= 65535, PSG_ERR_SHAPE, "psg_token_batch: S=%d above L=%d, or B=%d above 65535", S, L, B);
    hipLaunchKernelGGL(token_batch_kernel, dim3((S + TOK_THREADS - 1) / TOK_THREADS, B), dim3(TOK_THREADS), 0, (hipStream_t)stream, table,
                       lens, N, L, idx, S, pad_id, ids, mask, kv_len);
    PSG_LAUNCH_CHECK("token_batch_kernel");
    return PSG_OK;
}

}  // extern "C"
