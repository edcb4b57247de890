// The stage-1 loss around the VGG16 convolutions (reference: src/models/losses.py): 2x2 max-pool forward / backward, the image
// preprocessing (clamp, optional bilinear resize, ImageNet normalisation) forward / backward, the feature-map L1 with its
// gradient, and the KL term with its gradients.  All of them are bandwidth kernels: one 16-byte chunk of channels per lane
// (4 fp32 / 8 bf16), every output element written exactly once (the backward passes are gathers: no zero-fill, no scatter,
// no atomics), reductions in the fixed two-stage order of recon_loss_kernel / recon_finish_kernel (elementwise.hip).
#include "psg_common.h"

namespace {

using namespace psg;

constexpr int RED_BLOCKS = 1024;     // partials of a two-stage reduction (as elementwise.hip)
constexpr int RED_THREADS = 256;

inline int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

template <typename F>
int launch_dtype(int dtype, const char* name, F&& launch) {
    if (!with_dtype(dtype, launch)) return set_error(PSG_ERR_DTYPE, "%s: unsupported dtype %d", name, dtype);
    PSG_LAUNCH_CHECK(name);
    return PSG_OK;
}

// one 16-byte chunk of channels, moved with one dwordx4 access
template <typename T> struct alignas(16) Chunk { T v[Elem<T>::CH]; };
template <typename T> __device__ __forceinline__ Chunk<T> ld_chunk(const T* p) { return *reinterpret_cast<const Chunk<T>*>(p); }
template <typename T> __device__ __forceinline__ void st_chunk(T* p, const Chunk<T>& c) { *reinterpret_cast<Chunk<T>*>(p) = c; }
// the CH tap bytes of a chunk: one 4- or 8-byte access
template <int CH> struct alignas(CH) Taps { uint8_t v[CH]; };

// ---------------------------------------------------------------------------------------------------------------
// 2x2 max-pool, stride 2, floor (nn.MaxPool2d(2, 2) of torchvision's vgg16().features)
// ---------------------------------------------------------------------------------------------------------------
// A later tap replaces the maximum only if it is strictly greater (torch.max_pool2d on the CPU): on ties the first tap in
// row-major order wins.  The values are moved, never recomputed: y holds the bits of the winning input.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy,
                                                          uint8_t* __restrict__ tap, int B, int Hi, int Wi, int Ho, int Wo, int C) {
    constexpr int CH = Elem<T>::CH;
    const int cn = C / CH;
    const int64_t n = (int64_t)B * Ho * Wo * cn;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cn) * CH;
        int64_t r = i / cn;                                   // output pixel (b * Ho + ho) * Wo + wo
        const int wo = (int)(r % Wo);
        const int64_t bh = r / Wo;
        const int ho = (int)(bh % Ho);
        const int64_t b = bh / Ho;
        const T* p = x + ((b * Hi + 2 * ho) * Wi + 2 * wo) * ldx + c;
        const Chunk<T> t0 = ld_chunk(p), t1 = ld_chunk(p + ldx), t2 = ld_chunk(p + (int64_t)Wi * ldx), t3 = ld_chunk(p + ((int64_t)Wi + 1) * ldx);
        Chunk<T> o;
        Taps<CH> w;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            T best = t0.v[j];
            int k = 0;
            if ((float)t1.v[j] > (float)best) { best = t1.v[j]; k = 1; }
            if ((float)t2.v[j] > (float)best) { best = t2.v[j]; k = 2; }
            if ((float)t3.v[j] > (float)best) { best = t3.v[j]; k = 3; }
            o.v[j] = best;
            w.v[j] = (uint8_t)k;
        }
        st_chunk(y + r * ldy + c, o);
        if (tap) *reinterpret_cast<Taps<CH>*>(tap + r * C + c) = w;
    }
}

// Gather: the input element (hi, wi) belongs to the cell (hi / 2, wi / 2) as tap (hi & 1) * 2 + (wi & 1); it gets the cell's
// dy if that is the recorded tap, else 0, and 0 in the last row / column an odd Hi / Wi drops.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const uint8_t* __restrict__ tap,
                                                          T* __restrict__ dx, int64_t lddx, int B, int Hi, int Wi, int Ho, int Wo, int C) {
    constexpr int CH = Elem<T>::CH;
    const int cn = C / CH;
    const int64_t n = (int64_t)B * Hi * Wi * cn;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cn) * CH;
        const int64_t r = i / cn;                             // input pixel (b * Hi + hi) * Wi + wi
        const int wi = (int)(r % Wi);
        const int64_t bh = r / Wi;
        const int hi = (int)(bh % Hi);
        const int64_t b = bh / Hi;
        const int ho = hi >> 1, wo = wi >> 1;
        Chunk<T> o;
        if (ho < Ho && wo < Wo) {
            const int64_t q = (b * Ho + ho) * Wo + wo;
            const Chunk<T> g = ld_chunk(dy + q * lddy + c);
            const Taps<CH> w = *reinterpret_cast<const Taps<CH>*>(tap + q * C + c);
            const int mine = (hi & 1) * 2 + (wi & 1);
#pragma unroll
            for (int j = 0; j < CH; ++j) o.v[j] = (w.v[j] == mine) ? g.v[j] : (T)0.f;
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j) o.v[j] = (T)0.f;
        }
        st_chunk(dx + r * lddx + c, o);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// image preprocessing: fp32 NCHW [B,3,Hi,Wi] -> channels-last [B,Ho,Wo,8] (channels 3..7 zero)
// ---------------------------------------------------------------------------------------------------------------
// losses.py:51-53 (ImageNet statistics, as fp32 constants); the kernel multiplies by the fp32 reciprocal of std
__device__ __forceinline__ float prep_mean(int c) { return c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f); }
__device__ __forceinline__ float prep_inv_std(int c) { return c == 0 ? 1.0f / 0.229f : (c == 1 ? 1.0f / 0.224f : 1.0f / 0.225f); }
__device__ __forceinline__ float prep_clamp(float x, float a, float b) { return fminf(fmaxf(a * x + b, 0.f), 1.f); }

// F.interpolate(mode='bilinear', align_corners=False): src = (in / out) * (dst + 0.5) - 0.5, clamped at 0; i0 = floor(src),
// i1 = min(i0 + 1, in - 1), weights (1 - f, f) with f = src - i0.  The formula is PyTorch's; its evaluation is not: torch takes the
// source index in fp32 for an fp32 image, here it is taken in fp64 (in fp32 the index alone is off by up to ~3 * 2^-24 * in, more
// than every other rounding of the pass), so an fp32 launch is closer to the exact resize than torch's fp32 interpolate and NOT
// bit-comparable with it.
__device__ __forceinline__ void prep_coord64(int o, int in, int out, int& i0, int& i1, double& f) {
    double s = ((double)in / (double)out) * ((double)o + 0.5) - 0.5;
    if (s < 0.0) s = 0.0;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    f = s - (double)i0;
}
// the forward's fp32 weights: each rounded once from fp64 (1 - f taken in fp32 would lose the small weights' relative precision)
__device__ __forceinline__ void prep_coord(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
    double f;
    prep_coord64(o, in, out, i0, i1, f);
    l0 = (float)(1.0 - f);
    l1 = (float)f;
}
// the output indices o whose two taps can include input index i: src(o) in (i - 1, i + 1), one index of slack either side;
// i = 0 also collects the outputs whose source index was clamped to 0
__device__ __forceinline__ void prep_window(int i, int in, int out, int& lo, int& hi) {
    const double inv = (double)out / (double)in;
    lo = (int)floor(((double)i - 0.5) * inv - 0.5) - 1;
    hi = (int)ceil(((double)i + 1.5) * inv - 0.5) + 1;
    if (lo < 0 || i == 0) lo = 0;
    if (hi > out - 1) hi = out - 1;
}

// one output pixel per lane: consecutive lanes read consecutive floats of the three planes and write consecutive chunks
template <typename T, bool RESIZE>
__global__ __launch_bounds__(256) void image_prep_fwd_kernel(const float* __restrict__ img, T* __restrict__ y, int64_t ldy, int B, int Hi,
                                                             int Wi, int Ho, int Wo, float a, float b) {
    const int64_t n = (int64_t)B * Ho * Wo;
    const int64_t plane = (int64_t)Hi * Wi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int wo = (int)(i % Wo);
        const int64_t bh = i / Wo;
        const int ho = (int)(bh % Ho);
        const int64_t bb = bh / Ho;
        const float* src = img + bb * 3 * plane;
        float v[3];
        if (RESIZE) {
            int h0, h1, w0, w1; float kh, lh, kw, lw;
            prep_coord(ho, Hi, Ho, h0, h1, kh, lh);
            prep_coord(wo, Wi, Wo, w0, w1, kw, lw);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* p = src + c * plane;
                const float v00 = prep_clamp(p[(int64_t)h0 * Wi + w0], a, b), v01 = prep_clamp(p[(int64_t)h0 * Wi + w1], a, b);
                const float v10 = prep_clamp(p[(int64_t)h1 * Wi + w0], a, b), v11 = prep_clamp(p[(int64_t)h1 * Wi + w1], a, b);
                v[c] = kh * (kw * v00 + lw * v01) + lh * (kw * v10 + lw * v11);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = prep_clamp(src[c * plane + (int64_t)ho * Wi + wo], a, b);
        }
        T* o = y + i * ldy;
        const f32x4 lo = {(v[0] - prep_mean(0)) * prep_inv_std(0), (v[1] - prep_mean(1)) * prep_inv_std(1),
                          (v[2] - prep_mean(2)) * prep_inv_std(2), 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if constexpr (Elem<T>::CH == 8) {
            Chunk<T> ch;
#pragma unroll
            for (int j = 0; j < 8; ++j) ch.v[j] = (T)(j < 4 ? lo[j] : 0.f);
            st_chunk(o, ch);
        } else {
            store4<T>(o, lo);
            store4<T>(o + 4, zero);
        }
    }
}

// backward as a gather, one input pixel per lane, every element of the fp32 NCHW gradient written once:
//   dimg[b,c,h,w] = (sum over the output pixels whose stencil holds (h, w) of weight * dy[b,ho,wo,c]) * inv_std[c] * a * mask,
// mask = [0 <= a x + b <= 1] recomputed from the image; without a resize the sum is the one dy[b,h,w,c].  The resize sum (its
// weights, products and the accumulation in ascending (ho, wo), a fixed order) is taken in fp64 and rounded once with the two
// factors: this leg is never the sprites' path, and a handful of fp32 roundings per term is what the per-element bound against
// fp64 (4 * 2^-24 of the terms' magnitudes) does not leave room for.
template <typename T, bool RESIZE>
__global__ __launch_bounds__(256) void image_prep_bwd_kernel(const float* __restrict__ img, const T* __restrict__ dy, int64_t lddy,
                                                             float* __restrict__ dimg, int B, int Hi, int Wi, int Ho, int Wo, float a,
                                                             float b) {
    const int64_t plane = (int64_t)Hi * Wi;
    const int64_t n = (int64_t)B * plane;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bb = i / plane, p = i % plane;
        float g[3];
        if (RESIZE) {
            const int hi = (int)(p / Wi), wi = (int)(p % Wi);
            int ho_lo, ho_hi, wo_lo, wo_hi;
            prep_window(hi, Hi, Ho, ho_lo, ho_hi);
            prep_window(wi, Wi, Wo, wo_lo, wo_hi);
            double acc[3] = {0.0, 0.0, 0.0};
            for (int ho = ho_lo; ho <= ho_hi; ++ho) {
                int h0, h1; double fh;
                prep_coord64(ho, Hi, Ho, h0, h1, fh);
                double wh = 0.0;
                if (h0 == hi) wh += 1.0 - fh;
                if (h1 == hi) wh += fh;
                if (wh == 0.0) continue;
                for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                    int w0, w1; double fw;
                    prep_coord64(wo, Wi, Wo, w0, w1, fw);
                    double ww = 0.0;
                    if (w0 == wi) ww += 1.0 - fw;
                    if (w1 == wi) ww += fw;
                    if (ww == 0.0) continue;
                    const f32x4 d = load4<T>(dy + ((bb * Ho + ho) * Wo + wo) * lddy);
                    const double w = wh * ww;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += w * (double)d[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = (float)(acc[c] * (double)prep_inv_std(c) * (double)a);
        } else {
            const f32x4 d = load4<T>(dy + i * lddy);
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = d[c] * prep_inv_std(c) * a;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t at = (bb * 3 + c) * plane + p;
            const float u = a * img[at] + b;
            dimg[at] = (u >= 0.f && u <= 1.f) ? g[c] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// feature-map L1 and its gradient
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void feat_l1_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                                              T* __restrict__ grad, int64_t ldg, float* __restrict__ partial,
                                                              int64_t rows, int cols, float gval) {
    __shared__ float red[16];
    constexpr int CH = Elem<T>::CH;
    const int cn = cols / CH;
    const int64_t n = rows * cn;
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cn) * CH;
        const int64_t r = i / cn;
        const Chunk<T> va = ld_chunk(a + r * lda + c), vb = ld_chunk(b + r * ldb + c);
        Chunk<T> g;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const float d = (float)va.v[j] - (float)vb.v[j];
            acc += fabsf(d);
            g.v[j] = (T)(d > 0.f ? gval : (d < 0.f ? -gval : 0.f));
        }
        if (grad) st_chunk(grad + r * ldg + c, g);
    }
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one block sums the partials in a fixed order: out2 = {mean, scale * mean}
__global__ void feat_l1_finish_kernel(const float* __restrict__ partial, int count, float* __restrict__ out2, float inv_n, float scale) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) acc += partial[i];
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) { const float m = s * inv_n; out2[0] = m; out2[1] = scale * m; }
}

// ---------------------------------------------------------------------------------------------------------------
// KL(N(mu, exp(logvar)) || N(0, 1)) averaged over all n elements, and its gradients
// ---------------------------------------------------------------------------------------------------------------
// -0.5 (1 + lv - mu^2 - e^lv) = 0.5 (mu^2 + (e^lv - 1 - lv)): both summands are >= 0, so the sum has no cancellation; the one
// inside the second (e^lv - 1 - lv ~ lv^2 / 2 for small lv) is taken in fp64.  n is the latent's size (thousands): the
// fp64 arithmetic is not what this launch costs.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < nw; ++i) r += red[i];
    return r;
}

__global__ __launch_bounds__(RED_THREADS) void kl_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                         float* __restrict__ dmu, float* __restrict__ dlogvar,
                                                         double* __restrict__ partial, int64_t n, float inv_n) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mu[i], lv = logvar[i];
        const double md = (double)m, ld = (double)lv;
        acc += md * md + (expm1(ld) - ld);
        if (dmu) dmu[i] = m * inv_n;
        if (dlogvar) dlogvar[i] = 0.5f * expm1f(lv) * inv_n;
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void kl_finish_kernel(const double* __restrict__ partial, int count, float* __restrict__ out, double half_inv_n) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += blockDim.x) acc += partial[i];
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) out[0] = (float)(s * half_inv_n);
}

// rows of a channels-last operand: C a whole number of 16-byte chunks, ld a multiple of the chunk, base 16-byte aligned
int rows_ok(const char* who, const char* what, const void* p, int64_t ld, int C, int dtype) {
    const int ch = dtype == PSG_BF16 ? 8 : 4;
    PSG_REQUIRE(ld >= C && (ld % ch) == 0, PSG_ERR_SHAPE, "%s: ld of %s = %ld must be a multiple of %d and >= C = %d", who, what, (long)ld, ch, C);
    PSG_REQUIRE(aligned16(p), PSG_ERR_ALIGN, "%s: %s must be 16-byte aligned", who, what);
    return PSG_OK;
}

}  // namespace

extern "C" {

int psg_maxpool2x2_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, uint8_t* tap, int B, int Hi, int Wi, int C, int dtype,
                       psg_stream_t stream) {
    PSG_REQUIRE(x && y, PSG_ERR_ARG, "maxpool2x2_fwd: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "maxpool2x2_fwd: unsupported dtype %d", dtype);
    const int ch = dtype == PSG_BF16 ? 8 : 4;
    PSG_REQUIRE(B > 0 && Hi >= 2 && Wi >= 2 && C > 0 && (C % ch) == 0, PSG_ERR_SHAPE,
                "maxpool2x2_fwd: bad shape B=%d Hi=%d Wi=%d C=%d (Hi, Wi >= 2, C a multiple of %d)", B, Hi, Wi, C, ch);
    int rc;
    if ((rc = rows_ok("maxpool2x2_fwd", "x", x, ldx, C, dtype)) != PSG_OK) return rc;
    if ((rc = rows_ok("maxpool2x2_fwd", "y", y, ldy, C, dtype)) != PSG_OK) return rc;
    PSG_REQUIRE(!tap || aligned8(tap), PSG_ERR_ALIGN, "maxpool2x2_fwd: tap must be 8-byte aligned");
    const int Ho = Hi / 2, Wo = Wi / 2;
    const int g = grid_for((int64_t)B * Ho * Wo * (C / ch), 256, 65536);
    return launch_dtype(dtype, "maxpool2x2_fwd", [&](auto elem) {
        using T = decltype(elem);
        hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (T*)y, ldy, tap, B, Hi, Wi,
                           Ho, Wo, C);
    });
}

int psg_maxpool2x2_bwd(const void* dy, int64_t lddy, const uint8_t* tap, void* dx, int64_t lddx, int B, int Hi, int Wi, int C,
                       int dtype, psg_stream_t stream) {
    PSG_REQUIRE(dy && tap && dx, PSG_ERR_ARG, "maxpool2x2_bwd: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "maxpool2x2_bwd: unsupported dtype %d", dtype);
    const int ch = dtype == PSG_BF16 ? 8 : 4;
    PSG_REQUIRE(B > 0 && Hi >= 2 && Wi >= 2 && C > 0 && (C % ch) == 0, PSG_ERR_SHAPE,
                "maxpool2x2_bwd: bad shape B=%d Hi=%d Wi=%d C=%d (Hi, Wi >= 2, C a multiple of %d)", B, Hi, Wi, C, ch);
    int rc;
    if ((rc = rows_ok("maxpool2x2_bwd", "dy", dy, lddy, C, dtype)) != PSG_OK) return rc;
    if ((rc = rows_ok("maxpool2x2_bwd", "dx", dx, lddx, C, dtype)) != PSG_OK) return rc;
    PSG_REQUIRE(aligned8(tap), PSG_ERR_ALIGN, "maxpool2x2_bwd: tap must be 8-byte aligned");
    const int Ho = Hi / 2, Wo = Wi / 2;
    const int g = grid_for((int64_t)B * Hi * Wi * (C / ch), 256, 65536);
    return launch_dtype(dtype, "maxpool2x2_bwd", [&](auto elem) {
        using T = decltype(elem);
        hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, lddy, tap, (T*)dx, lddx, B, Hi,
                           Wi, Ho, Wo, C);
    });
}

int psg_image_prep_fwd(const float* img, void* y, int64_t ldy, int B, int Hi, int Wi, int Ho, int Wo, float a, float b, int dtype,
                       psg_stream_t stream) {
    PSG_REQUIRE(img && y, PSG_ERR_ARG, "image_prep_fwd: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "image_prep_fwd: unsupported dtype %d", dtype);
    PSG_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, PSG_ERR_SHAPE, "image_prep_fwd: bad shape B=%d %dx%d -> %dx%d", B, Hi, Wi, Ho, Wo);
    int rc;
    if ((rc = rows_ok("image_prep_fwd", "y", y, ldy, 8, dtype)) != PSG_OK) return rc;
    const bool resize = Ho != Hi || Wo != Wi;
    const int g = grid_for((int64_t)B * Ho * Wo, 256, 65536);
    return launch_dtype(dtype, "image_prep_fwd", [&](auto elem) {
        using T = decltype(elem);
        if (resize)
            hipLaunchKernelGGL((image_prep_fwd_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (T*)y, ldy, B, Hi, Wi, Ho, Wo, a, b);
        else
            hipLaunchKernelGGL((image_prep_fwd_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (T*)y, ldy, B, Hi, Wi, Ho, Wo, a, b);
    });
}

int psg_image_prep_bwd(const float* img, const void* dy, int64_t lddy, float* dimg, int B, int Hi, int Wi, int Ho, int Wo, float a,
                       float b, int dtype, psg_stream_t stream) {
    PSG_REQUIRE(img && dy && dimg, PSG_ERR_ARG, "image_prep_bwd: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "image_prep_bwd: unsupported dtype %d", dtype);
    PSG_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, PSG_ERR_SHAPE, "image_prep_bwd: bad shape B=%d %dx%d -> %dx%d", B, Hi, Wi, Ho, Wo);
    int rc;
    if ((rc = rows_ok("image_prep_bwd", "dy", dy, lddy, 8, dtype)) != PSG_OK) return rc;
    const bool resize = Ho != Hi || Wo != Wi;
    const int g = grid_for((int64_t)B * Hi * Wi, 256, 65536);
    return launch_dtype(dtype, "image_prep_bwd", [&](auto elem) {
        using T = decltype(elem);
        if (resize)
            hipLaunchKernelGGL((image_prep_bwd_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (const T*)dy, lddy, dimg, B, Hi,
                               Wi, Ho, Wo, a, b);
        else
            hipLaunchKernelGGL((image_prep_bwd_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, (const T*)dy, lddy, dimg, B, Hi,
                               Wi, Ho, Wo, a, b);
    });
}

int64_t psg_feat_l1_workspace_bytes(void) { return (int64_t)RED_BLOCKS * sizeof(float); }

int psg_feat_l1(const void* a, int64_t lda, const void* b, int64_t ldb, void* grad, int64_t ldg, float* out2, int64_t rows, int cols,
                float scale, int dtype, void* ws, int64_t ws_bytes, psg_stream_t stream) {
    PSG_REQUIRE(a && b && out2 && ws, PSG_ERR_ARG, "feat_l1: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "feat_l1: unsupported dtype %d", dtype);
    const int ch = dtype == PSG_BF16 ? 8 : 4;
    PSG_REQUIRE(rows > 0 && cols > 0 && (cols % ch) == 0, PSG_ERR_SHAPE, "feat_l1: bad shape rows=%ld cols=%d (cols a multiple of %d)",
                (long)rows, cols, ch);
    int rc;
    if ((rc = rows_ok("feat_l1", "a", a, lda, cols, dtype)) != PSG_OK) return rc;
    if ((rc = rows_ok("feat_l1", "b", b, ldb, cols, dtype)) != PSG_OK) return rc;
    if (grad && (rc = rows_ok("feat_l1", "grad", grad, ldg, cols, dtype)) != PSG_OK) return rc;
    PSG_REQUIRE(ws_bytes >= psg_feat_l1_workspace_bytes(), PSG_ERR_WORKSPACE, "feat_l1: workspace of %ld bytes, need %ld", (long)ws_bytes,
                (long)psg_feat_l1_workspace_bytes());
    const double nel = (double)rows * (double)cols;
    const float gval = scale / (float)nel;
    const int g = grid_for(rows * (cols / ch), RED_THREADS, RED_BLOCKS);
    rc = launch_dtype(dtype, "feat_l1", [&](auto elem) {
        using T = decltype(elem);
        hipLaunchKernelGGL(feat_l1_kernel<T>, dim3(g), dim3(RED_THREADS), 0, (hipStream_t)stream, (const T*)a, lda, (const T*)b, ldb, (T*)grad,
                           ldg, (float*)ws, rows, cols, gval);
    });
    if (rc != PSG_OK) return rc;
    hipLaunchKernelGGL(feat_l1_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, g, out2, 1.0f / (float)nel, scale);
    PSG_LAUNCH_CHECK("feat_l1_finish");
    return PSG_OK;
}

int64_t psg_kl_workspace_bytes(void) { return (int64_t)RED_BLOCKS * sizeof(double); }

int psg_kl_f32(const float* mu, const float* logvar, float* dmu, float* dlogvar, float* out, int64_t n, void* ws, int64_t ws_bytes,
               psg_stream_t stream) {
    PSG_REQUIRE(mu && logvar && out && ws, PSG_ERR_ARG, "kl: null pointer");
    PSG_REQUIRE(n > 0, PSG_ERR_SHAPE, "kl: n=%ld", (long)n);
    PSG_REQUIRE(aligned8(ws), PSG_ERR_ALIGN, "kl: ws must be 8-byte aligned");
    PSG_REQUIRE(ws_bytes >= psg_kl_workspace_bytes(), PSG_ERR_WORKSPACE, "kl: workspace of %ld bytes, need %ld", (long)ws_bytes,
                (long)psg_kl_workspace_bytes());
    const int g = grid_for(n, RED_THREADS, RED_BLOCKS);
    hipLaunchKernelGGL(kl_kernel, dim3(g), dim3(RED_THREADS), 0, (hipStream_t)stream, mu, logvar, dmu, dlogvar, (double*)ws, n, 1.0f / (float)n);
    PSG_LAUNCH_CHECK("kl");
    hipLaunchKernelGGL(kl_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, g, out, 0.5 / (double)n);
    PSG_LAUNCH_CHECK("kl_finish");
    return PSG_OK;
}

}  // extern "C"
