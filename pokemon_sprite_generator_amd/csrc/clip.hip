// The parts of CLIP (reference: src/models/clip_loss.py - transformers' CLIPModel + CLIPProcessor, openai/clip-vit-base-patch32)
// that BERT and the U-Net do not have: the image processor as one pass that writes patch rows (and its backward as a gather),
// the text tower's causal attention, and the cosine loss with its gradient.  Everything else of the two towers is psg_conv_fwd
// Linears, psg_layernorm and psg_attn_fwd / psg_attn_bwd.  No atomics; every reduction runs in a fixed order.
//
// The resize SPECIFICATION is the float path of the image processor (its torchvision backend):
// F.interpolate(mode='bicubic', align_corners=False, antialias=True), which neither clamps nor quantises and is differentiable.
// The PIL backend (through uint8, overshoot clipped) differs from it by up to 0.41 in normalised units on noise and cannot
// take a training batch; reproducing it is a non-goal.
#include "psg_common.h"

namespace {

using namespace psg;

template <typename F>
int launch_dtype(int dtype, const char* name, F&& launch) {
    if (!with_dtype(dtype, launch)) return set_error(PSG_ERR_DTYPE, "%s: unsupported dtype %d", name, dtype);
    PSG_LAUNCH_CHECK(name);
    return PSG_OK;
}

inline int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------
// image processor: fp32 NCHW [B,3,Hi,Hi] -> patch rows [B (S/P)^2, 3 P P]
// ---------------------------------------------------------------------------------------------------------------
// CLIP's statistics (CLIPImageProcessor's image_mean / image_std) as fp32 constants; the kernel multiplies by fp32(1 / std)
__device__ __forceinline__ float clip_mean(int c) { return c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f); }
__device__ __forceinline__ float clip_inv_std(int c) {
    return c == 0 ? 1.0f / 0.26862954f : (c == 1 ? 1.0f / 0.26130258f : 1.0f / 0.27577711f);
}

// Keys cubic, a = -0.5 (ATen's antialias bicubic filter; the non-antialiased 'bicubic' uses a = -0.75)
__device__ __forceinline__ double keys_cubic(double x) {
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// The taps of output index o when `in` source samples are resized to `out` >= in (ATen, _compute_indices_min_size_weights_aa
// with align_corners=False and scale = in / out <= 1, so the support is the filter's own 2 samples): centre = scale (o + 0.5),
// the window [trunc(centre - 1.5), trunc(centre + 2.5)) clipped to [0, in) - at most 4 samples - and the filter at
// (sample + 0.5 - centre), renormalised to sum 1 over the clipped window.  All in fp64 (as psg_image_prep_fwd takes its source
// index: in fp32 the index alone would cost more than every other rounding of the pass).
__device__ __forceinline__ void clip_taps(int o, int in, int out, int& x0, int& n, double w[4]) {
    const double scale = (double)in / (double)out;
    const double center = scale * ((double)o + 0.5);
    int lo = (int)(center - 1.5), hi = (int)(center + 2.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    x0 = lo;
    n = hi - lo;
    if (n > 4) n = 4;
    if (n < 0) n = 0;
    double total = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w[j] = j < n ? keys_cubic((double)(lo + j) + 0.5 - center) : 0.0;
        total += w[j];
    }
    if (total != 0.0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] /= total;
    }
}

// The outputs o whose window can hold source index i: trunc(centre - 1.5) <= i < trunc(centre + 2.5), that is centre(o) in
// [i - 1.5, i + 2.5) - about 4 out / in of them.  floor / ceil leave up to one index of slack either side; every candidate
// is then tested against its own window (clip_tap_weight), so the slack costs time only.
__device__ __forceinline__ void clip_window(int i, int in, int out, int& lo, int& hi) {
    const double inv = (double)out / (double)in;
    lo = (int)floor(((double)i - 1.5) * inv - 0.5);
    hi = (int)ceil(((double)i + 2.5) * inv - 0.5);
    if (lo < 0) lo = 0;
    if (hi > out - 1) hi = out - 1;
}
// the weight source index i has in output o (0 when o's window does not hold it)
__device__ __forceinline__ double clip_tap_weight(int o, int i, int in, int out) {
    int x0, n;
    double w[4];
    clip_taps(o, in, out, x0, n, w);
    const int j = i - x0;
    if (j < 0 || j >= n) return 0.0;
    return j == 0 ? w[0] : (j == 1 ? w[1] : (j == 2 ? w[2] : w[3]));
}

// where pixel (oy, ox), channel c of sample bb lives in the patch rows: row = patch, column c P^2 + ky P + kx - the
// flattening of the patch embedding's Conv2d(3, width, P, stride P) weight
__device__ __forceinline__ int64_t patch_at(int64_t bb, int oy, int ox, int c, int S, int P, int64_t ld) {
    const int G = S / P;
    const int64_t row = (bb * G + oy / P) * G + ox / P;
    return row * ld + (int64_t)c * P * P + (oy % P) * P + (ox % P);
}

// one output pixel per lane (its three channels): consecutive lanes write P consecutive elements of a patch row
template <typename T, bool RESIZE>
__global__ __launch_bounds__(256) void clip_prep_fwd_kernel(const float* __restrict__ img, T* __restrict__ y, int64_t ldy, int B, int Hi, int S,
                                                            int P, float a, float b) {
    const int64_t n = (int64_t)B * S * S;
    const int64_t plane = (int64_t)Hi * Hi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % S);
        const int64_t bh = i / S;
        const int oy = (int)(bh % S);
        const int64_t bb = bh / S;
        const float* src = img + bb * 3 * plane;
        float v[3];
        if (RESIZE) {
            int y0, ny, x0, nx;
            double wy64[4], wx64[4];
            clip_taps(oy, Hi, S, y0, ny, wy64);
            clip_taps(ox, Hi, S, x0, nx, wx64);
            float wy[4], wx[4];                            // each weight rounded once
#pragma unroll
            for (int j = 0; j < 4; ++j) { wy[j] = (float)wy64[j]; wx[j] = (float)wx64[j]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* p = src + c * plane;
                float acc = 0.f;
#pragma unroll
                for (int jy = 0; jy < 4; ++jy) {
                    if (jy >= ny) break;
                    const float* r = p + (int64_t)(y0 + jy) * Hi + x0;
                    float row = 0.f;
#pragma unroll
                    for (int jx = 0; jx < 4; ++jx) {
                        if (jx >= nx) break;
                        row += wx[jx] * (a * r[jx] + b);
                    }
                    acc += wy[jy] * row;
                }
                v[c] = acc;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = a * src[c * plane + (int64_t)oy * Hi + ox] + b;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) Elem<T>::st(y + patch_at(bb, oy, ox, c, S, P, ldy), (v[c] - clip_mean(c)) * clip_inv_std(c));
    }
}

// Backward as a gather, one source pixel per lane, every element of dimg written once:
//   dimg[b,c,iy,ix] = (sum over the outputs (oy, ox) whose windows hold (iy, ix) of wy * wx * dy[patch(oy, ox), c]) * inv_std[c] * a
// The candidate columns go in chunks of BWD_XC: a chunk's x weights are evaluated once and kept in registers while the candidate
// rows are walked (one y weight per row), so a pixel costs about (columns + rows) tap evaluations, not their product; at
// 215 -> 224 one chunk holds every column.  The order - chunk, row, column - is fixed; weights, products and the sum are fp64,
// rounded once with the two factors (as psg_image_prep_bwd).  Nothing is clamped in the forward, so there is no mask.
constexpr int BWD_XC = 8;
template <typename T, bool RESIZE>
__global__ __launch_bounds__(256) void clip_prep_bwd_kernel(const T* __restrict__ dy, int64_t lddy, float* __restrict__ dimg, int B, int Hi,
                                                            int S, int P, float a) {
    const int64_t plane = (int64_t)Hi * Hi;
    const int64_t n = (int64_t)B * plane;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bb = i / plane, p = i % plane;
        const int iy = (int)(p / Hi), ix = (int)(p % Hi);
        float g[3];
        if (RESIZE) {
            int oy_lo, oy_hi, ox_lo, ox_hi;
            clip_window(iy, Hi, S, oy_lo, oy_hi);
            clip_window(ix, Hi, S, ox_lo, ox_hi);
            double acc[3] = {0.0, 0.0, 0.0};
            for (int xb = ox_lo; xb <= ox_hi; xb += BWD_XC) {
                double wx[BWD_XC];                         // 0 past ox_hi and outside a window: such a column is never read
#pragma unroll
                for (int k = 0; k < BWD_XC; ++k) wx[k] = xb + k <= ox_hi ? clip_tap_weight(xb + k, ix, Hi, S) : 0.0;
                for (int oy = oy_lo; oy <= oy_hi; ++oy) {
                    const double wh = clip_tap_weight(oy, iy, Hi, S);
                    if (wh == 0.0) continue;
#pragma unroll
                    for (int k = 0; k < BWD_XC; ++k) {
                        if (wx[k] == 0.0) continue;
                        const double w = wh * wx[k];
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += w * (double)Elem<T>::ld(dy + patch_at(bb, oy, xb + k, c, S, P, lddy));
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = (float)(acc[c] * (double)clip_inv_std(c) * (double)a);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = Elem<T>::ld(dy + patch_at(bb, iy, ix, c, S, P, lddy)) * clip_inv_std(c) * a;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dimg[(bb * 3 + c) * plane + p] = g[c];
    }
}

int clip_prep_check(const char* who, int64_t ld, int B, int Hi, int Wi, int S, int P, int dtype) {
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "%s: unsupported dtype %d", who, dtype);
    PSG_REQUIRE(B > 0 && Hi > 0 && S > 0 && P > 0, PSG_ERR_SHAPE, "%s: bad shape B=%d %dx%d -> %d, patch %d", who, B, Hi, Wi, S, P);
    PSG_REQUIRE(Hi == Wi && Hi <= S, PSG_ERR_SHAPE,
                "%s: image %dx%d for size %d - only square images no larger than the target are supported (no centre crop, no widened antialias window)",
                who, Hi, Wi, S);
    PSG_REQUIRE(S % P == 0, PSG_ERR_SHAPE, "%s: size %d is not a multiple of the patch %d", who, S, P);
    PSG_REQUIRE(ld >= (int64_t)3 * P * P, PSG_ERR_SHAPE, "%s: row stride %ld below 3 * %d^2", who, (long)ld, P);
    return PSG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// causal self-attention of the text tower (77 tokens x 64): one workgroup per (sample, head), one query row per lane
// ---------------------------------------------------------------------------------------------------------------
// K and V of the head are staged once in LDS as fp32; lane l keeps its query and its output row in registers and walks the
// keys s = 0..l with a running maximum (the lanes of a wave read the same K / V address: a broadcast, no bank conflict).
// Key 0 alone gives p = exp(0) = 1 and a sum of 1: row 0 of the result is v[0] itself.
template <typename T, int D>
__global__ __launch_bounds__(128) void attn_causal_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                          const T* __restrict__ v, int64_t ldv, T* __restrict__ o, int64_t ldo,
                                                          float* __restrict__ lse, int heads, int L, float scale) {
    extern __shared__ __attribute__((aligned(16))) float kv_lds[];
    float* ks = kv_lds;
    float* vs = kv_lds + (size_t)L * D;
    const int h = blockIdx.x, bb = blockIdx.y;
    const int64_t row0 = (int64_t)bb * L;
    for (int i = threadIdx.x; i < L * (D / 4); i += blockDim.x) {
        const int s = i / (D / 4), j = (i % (D / 4)) * 4;
        *reinterpret_cast<f32x4*>(ks + s * D + j) = load4<T>(k + (row0 + s) * ldk + h * D + j);
        *reinterpret_cast<f32x4*>(vs + s * D + j) = load4<T>(v + (row0 + s) * ldv + h * D + j);
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (l >= L) return;
    f32x4 qr[D / 4], acc[D / 4];
#pragma unroll
    for (int j = 0; j < D / 4; ++j) {
        qr[j] = load4<T>(q + (row0 + l) * ldq + h * D + j * 4);
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, sum = 0.f;
    for (int s = 0; s <= l; ++s) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < D / 4; ++j) {
            const f32x4 kk = *reinterpret_cast<const f32x4*>(ks + s * D + j * 4);
            dot += qr[j][0] * kk[0] + qr[j][1] * kk[1] + qr[j][2] * kk[2] + qr[j][3] * kk[3];
        }
        const float sc = dot * scale;
        const float mn = fmaxf(m, sc);
        const float corr = expf(m - mn);                  // 0 on the first key (m = -inf)
        const float p = expf(sc - mn);
        sum = sum * corr + p;
#pragma unroll
        for (int j = 0; j < D / 4; ++j) acc[j] = acc[j] * corr + *reinterpret_cast<const f32x4*>(vs + s * D + j * 4) * p;
        m = mn;
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < D / 4; ++j) store4<T>(o + (row0 + l) * ldo + h * D + j * 4, acc[j] * inv);
    if (lse) lse[((int64_t)bb * heads + h) * L + l] = m + logf(sum);
}

constexpr int CAUSAL_MAX_L = 128;
using CausalDims = std::integer_sequence<int, 16, 32, 64>;

template <typename T>
int causal_init_attrs() {
    return set_max_lds(2 * CAUSAL_MAX_L * 64 * (int)sizeof(float), attn_causal_kernel<T, 16>, attn_causal_kernel<T, 32>, attn_causal_kernel<T, 64>);
}

// ---------------------------------------------------------------------------------------------------------------
// cosine loss
// ---------------------------------------------------------------------------------------------------------------
// One workgroup; wave w takes the rows w, w + 4, ...: three fp32 dot products per row (lane-strided, then the wave's butterfly),
// the row's gradient, and the wave's running sum of cosines in ascending row order; the four sums are added in wave order.
template <typename T>
__global__ __launch_bounds__(256) void cosine_loss_kernel(const T* __restrict__ u, int64_t ldu, const T* __restrict__ v, int64_t ldv,
                                                          T* __restrict__ du, int64_t lddu, float* __restrict__ out, int B, int D) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float eps = 1e-12f, inv_b = 1.0f / (float)B;
    float cos_sum = 0.f;
    for (int r = wid; r < B; r += 4) {
        const T* ur = u + (int64_t)r * ldu;
        const T* vr = v + (int64_t)r * ldv;
        float uu = 0.f, vv = 0.f, uv = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 a = load4<T>(ur + c), b = load4<T>(vr + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) { uu += a[e] * a[e]; vv += b[e] * b[e]; uv += a[e] * b[e]; }
        }
        uu = wave_sum(uu); vv = wave_sum(vv); uv = wave_sum(uv);
        const float nu = sqrtf(uu), nv = sqrtf(vv);
        const float du_n = fmaxf(nu, eps), dv_n = fmaxf(nv, eps);        // F.normalize: x / max(||x||, eps)
        const float cs = uv / (du_n * dv_n);
        cos_sum += cs;
        if (du) {
            // d cos / du = v^ / max(||u||, eps) - [||u|| > eps] cos u / ||u||^2   (the clamp passes no gradient below eps)
            const float kv = -inv_b / (du_n * dv_n);
            const float ku = nu > eps ? inv_b * cs / uu : 0.f;
            for (int c = lane * 4; c < D; c += 256) {
                const f32x4 a = load4<T>(ur + c), b = load4<T>(vr + c);
                store4<T>(du + (int64_t)r * lddu + c, b * kv + a * ku);
            }
        }
    }
    if (lane == 0) part[wid] = cos_sum;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = -(((part[0] + part[1]) + part[2]) + part[3]) * inv_b;
}

}  // namespace

extern "C" {

// psg_init: the causal kernel may take K and V of 128 keys x 64 as fp32 (64 KiB)
int psg_clip_init_attrs(void) {
    const int rc = causal_init_attrs<float>();
    return rc != PSG_OK ? rc : causal_init_attrs<bf16_t>();
}

int psg_clip_prep_fwd(const float* img, void* y, int64_t ldy, int B, int Hi, int Wi, int S, int P, float a, float b, int dtype,
                      psg_stream_t stream) {
    PSG_REQUIRE(img && y, PSG_ERR_ARG, "clip_prep_fwd: null pointer");
    int rc;
    if ((rc = clip_prep_check("clip_prep_fwd", ldy, B, Hi, Wi, S, P, dtype)) != PSG_OK) return rc;
    const int g = grid_for((int64_t)B * S * S, 256, 65536);
    return launch_dtype(dtype, "clip_prep_fwd", [&](auto elem) {
        using T = decltype(elem);
        if (Hi != S)
            hipLaunchKernelGGL((clip_prep_fwd_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (T*)y, ldy, B, Hi, S, P, a, b);
        else
            hipLaunchKernelGGL((clip_prep_fwd_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (T*)y, ldy, B, Hi, S, P, a, b);
    });
}

int psg_clip_prep_bwd(const void* dy, int64_t lddy, float* dimg, int B, int Hi, int Wi, int S, int P, float a, int dtype,
                      psg_stream_t stream) {
    PSG_REQUIRE(dy && dimg, PSG_ERR_ARG, "clip_prep_bwd: null pointer");
    int rc;
    if ((rc = clip_prep_check("clip_prep_bwd", lddy, B, Hi, Wi, S, P, dtype)) != PSG_OK) return rc;
    const int g = grid_for((int64_t)B * Hi * Hi, 256, 65536);
    return launch_dtype(dtype, "clip_prep_bwd", [&](auto elem) {
        using T = decltype(elem);
        if (Hi != S)
            hipLaunchKernelGGL((clip_prep_bwd_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, lddy, dimg, B, Hi, S, P, a);
        else
            hipLaunchKernelGGL((clip_prep_bwd_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, lddy, dimg, B, Hi, S, P, a);
    });
}

int psg_attn_fwd_causal(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                        float* lse, int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed, int dtype,
                        psg_stream_t stream) {
    (void)seed;
    PSG_REQUIRE(q && k && v && o, PSG_ERR_ARG, "attn_fwd_causal: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "attn_fwd_causal: unsupported dtype %d", dtype);
    PSG_REQUIRE(drop_p == 0.f, PSG_ERR_ARG, "attn_fwd_causal: forward only, drop_p must be 0");
    PSG_REQUIRE(B > 0 && B <= 65535 && heads > 0 && L > 0 && L == S && L <= CAUSAL_MAX_L, PSG_ERR_SHAPE,
                "attn_fwd_causal: bad shape B=%d heads=%d L=%d S=%d (L == S <= %d)", B, heads, L, S, CAUSAL_MAX_L);
    PSG_REQUIRE(d == 16 || d == 32 || d == 64, PSG_ERR_SHAPE, "attn_fwd_causal: head_dim %d (16, 32 or 64)", d);
    const int64_t E = (int64_t)heads * d;
    PSG_REQUIRE(ldq >= E && ldk >= E && ldv >= E && ldo >= E && ((ldq | ldk | ldv | ldo) & 3) == 0, PSG_ERR_SHAPE,
                "attn_fwd_causal: row strides must be multiples of 4 and >= heads * d = %ld", (long)E);
    const uintptr_t al = dtype == PSG_BF16 ? 7 : 15;                 // 4 elements
    PSG_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                  reinterpret_cast<uintptr_t>(o)) & al) == 0, PSG_ERR_ALIGN, "attn_fwd_causal: q, k, v, o must start on a 4-element boundary");
    const int threads = L <= 64 ? 64 : 128;
    const size_t lds = (size_t)2 * L * d * sizeof(float);
    bool found = false;
    const int rc = launch_dtype(dtype, "attn_fwd_causal", [&](auto elem) {
        using T = decltype(elem);
        found = with_const(CausalDims{}, d, [&](auto dc) {
            hipLaunchKernelGGL((attn_causal_kernel<T, decltype(dc)::value>), dim3(heads, B), dim3(threads), lds, (hipStream_t)stream,
                               (const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (T*)o, ldo, lse, heads, L, scale);
        });
    });
    if (rc == PSG_OK && !found) return set_error(PSG_ERR_SHAPE, "attn_fwd_causal: head_dim %d", d);
    return rc;
}

int psg_cosine_loss(const void* u, int64_t ldu, const void* v, int64_t ldv, void* du, int64_t lddu, float* out, int B, int D, int dtype,
                    psg_stream_t stream) {
    PSG_REQUIRE(u && v && out, PSG_ERR_ARG, "cosine_loss: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "cosine_loss: unsupported dtype %d", dtype);
    PSG_REQUIRE(B > 0 && D > 0 && (D & 3) == 0, PSG_ERR_SHAPE, "cosine_loss: bad shape B=%d D=%d (D a multiple of 4)", B, D);
    PSG_REQUIRE(ldu >= D && ldv >= D && ((ldu | ldv) & 3) == 0 && (!du || (lddu >= D && (lddu & 3) == 0)), PSG_ERR_SHAPE,
                "cosine_loss: row strides must be multiples of 4 and >= D = %d", D);
    const uintptr_t al = dtype == PSG_BF16 ? 7 : 15;
    PSG_REQUIRE(((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(du)) & al) == 0, PSG_ERR_ALIGN,
                "cosine_loss: u, v, du must start on a 4-element boundary");
    return launch_dtype(dtype, "cosine_loss", [&](auto elem) {
        using T = decltype(elem);
        hipLaunchKernelGGL(cosine_loss_kernel<T>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const T*)u, ldu, (const T*)v, ldv, (T*)du, lddu, out, B, D);
    });
}

}  // extern "C"
