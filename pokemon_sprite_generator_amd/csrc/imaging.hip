// The two ends of the demo's generation path (psg_resample_u8, psg_image_to_u8, psg_latent_mix_f32; specified in
// include/psg_hip.h): PIL's 8-bit separable resample with ToTensor + normalise fused into its last pass, the decoder's
// fp32 image to uint8 HWC, and the latent / noise blend.
//
// The resample is integer arithmetic end to end (PIL's Resample.c: 22-bit fixed-point coefficients, an int32 accumulator
// that starts at 1 << 21, `>> 22`, clamp to 0..255, uint8 between the passes), so the result is bit-exact by construction.
// Every pixel access is a single-byte load or store: rows of an interleaved C = 3 image start at any byte address.
#include "psg_common.h"

namespace {

using namespace psg;

constexpr int PRECISION_BITS = 32 - 8 - 2;     // PIL's
constexpr int RS_LANES = 64;                   // lanes along x * C: consecutive lanes, consecutive bytes of a row
constexpr int RS_WAVES = 4;                    // waves of a workgroup, each on its own row(s)
constexpr int H_ROWS = 4;                      // horizontal pass: rows per lane - one coefficient load serves all of them
constexpr int MAX_DIM = 1 << 17;               // any image side: e = x * C + c stays far inside 32 bits, gridDim.y inside 65535
constexpr int MAX_BATCH = 65535;               // gridDim.z
constexpr int PW_THREADS = 256;

struct Emit {
    uint8_t* u8;          // [B, H, W, C] or NULL
    float* f32;           // [B, 3, H, W] or NULL: lut[value] of the first three channels
    const float* lut;
};

__device__ __forceinline__ uint8_t clip8(int32_t acc) {
    const int32_t v = acc >> PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// byte e = x * C + c of row y of image b, of a pass's final result
__device__ __forceinline__ void emit(const Emit& o, int b, int y, int e, int H, int W, int C, uint8_t v) {
    if (o.u8) o.u8[((size_t)b * H + y) * ((size_t)W * C) + e] = v;
    if (o.f32) {
        const int x = e / C, c = e - x * C;
        if (c < 3) o.f32[(((size_t)b * 3 + c) * H + y) * (size_t)W + x] = o.lut[v];
    }
}

// (first, count) of a bounds row, cut to the table width and to the input: whatever the table holds, no tap is read outside
__device__ __forceinline__ void taps_of(const int32_t* bounds, int i, int kmax, int in_size, int& first, int& count) {
    first = max(bounds[2 * i], 0);
    count = min(min(bounds[2 * i + 1], kmax), in_size - first);
}

// Horizontal pass: src [B, H, Win, C] -> [B, H, Wout, C].  A lane owns one output byte column e = x * C + c and H_ROWS rows:
// the lanes of a column block walk the same coefficient rows whatever their image row, so each coefficient is loaded once
// per lane and used H_ROWS times, and the H_ROWS byte loads of a tap are independent.
template <bool FINAL>
__global__ __launch_bounds__(RS_LANES * RS_WAVES) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                         Emit o, const int32_t* __restrict__ bounds,
                                                                         const int32_t* __restrict__ coef, int kmax, int H,
                                                                         int Win, int Wout, int C) {
    const int e = blockIdx.x * RS_LANES + threadIdx.x, b = blockIdx.z;
    const int y0 = (blockIdx.y * RS_WAVES + threadIdx.y) * H_ROWS;
    if (e >= Wout * C || y0 >= H) return;
    const int x = e / C, c = e - x * C;
    int first, count;
    taps_of(bounds, x, kmax, Win, first, count);
    const int32_t* k = coef + (size_t)x * kmax;
    const size_t in_row = (size_t)Win * C;
    const uint8_t* p = src + ((size_t)b * H + y0) * in_row + (size_t)first * C + c;
    const int rows = min(H_ROWS, H - y0);
    int32_t acc[H_ROWS];
#pragma unroll
    for (int r = 0; r < H_ROWS; ++r) acc[r] = 1 << (PRECISION_BITS - 1);
    if (rows == H_ROWS) {
        for (int t = 0; t < count; ++t) {
            const int32_t w = k[t];
#pragma unroll
            for (int r = 0; r < H_ROWS; ++r) acc[r] += (int32_t)p[r * in_row + (size_t)t * C] * w;
        }
    } else {
        for (int t = 0; t < count; ++t) {
            const int32_t w = k[t];
#pragma unroll
            for (int r = 0; r < H_ROWS; ++r)
                if (r < rows) acc[r] += (int32_t)p[r * in_row + (size_t)t * C] * w;
        }
    }
#pragma unroll
    for (int r = 0; r < H_ROWS; ++r) {
        if (r >= rows) break;
        const uint8_t v = clip8(acc[r]);
        if (FINAL) emit(o, b, y0 + r, e, H, Wout, C, v);
        else dst[((size_t)b * H + y0 + r) * ((size_t)Wout * C) + e] = v;
    }
}

// Vertical pass: src [B, Hin, W, C] -> the final [B, Hout, W, C].  A wave owns 64 consecutive bytes of one output row: every
// tap is one coalesced row segment, and the bounds and coefficient rows are the same for the whole wave.
__global__ __launch_bounds__(RS_LANES * RS_WAVES) void resample_v_kernel(const uint8_t* __restrict__ src, Emit o,
                                                                         const int32_t* __restrict__ bounds,
                                                                         const int32_t* __restrict__ coef, int kmax, int Hin,
                                                                         int Hout, int W, int C) {
    const int e = blockIdx.x * RS_LANES + threadIdx.x, b = blockIdx.z;
    const int y = blockIdx.y * RS_WAVES + threadIdx.y;
    if (e >= W * C || y >= Hout) return;
    int first, count;
    taps_of(bounds, y, kmax, Hin, first, count);
    const int32_t* k = coef + (size_t)y * kmax;
    const size_t row = (size_t)W * C;
    const uint8_t* p = src + ((size_t)b * Hin + first) * row + e;
    int32_t acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < count; ++t) acc += (int32_t)p[(size_t)t * row] * k[t];
    emit(o, b, y, e, Hout, W, C, clip8(acc));
}

// Both passes skipped (the sizes are equal): the copy, through the same emit
__global__ __launch_bounds__(RS_LANES * RS_WAVES) void resample_copy_kernel(const uint8_t* __restrict__ src, Emit o, int H, int W, int C) {
    const int e = blockIdx.x * RS_LANES + threadIdx.x, b = blockIdx.z;
    const int y = blockIdx.y * RS_WAVES + threadIdx.y;
    if (e >= W * C || y >= H) return;
    emit(o, b, y, e, H, W, C, src[((size_t)b * H + y) * ((size_t)W * C) + e]);
}

// One lane per pixel: three strided fp32 loads (coalesced along x for NCHW planes and for channels_last alike), three byte stores
__global__ __launch_bounds__(PW_THREADS) void image_to_u8_kernel(const float* __restrict__ img, int64_t sb, int64_t sc, int64_t sh,
                                                                 int64_t sw, uint8_t* __restrict__ out, int H, int W) {
    const int x = blockIdx.x * PW_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float* p = img + b * sb + y * sh + x * sw;
    uint8_t* q = out + (((size_t)b * H + y) * W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = (p[c * sc] + 1.0f) / 2.0f;
        t = fminf(fmaxf(t, 0.f), 1.f);             // (NaN -> 0: fmaxf returns its other operand)
        t = t * 255.f;
        q[c] = (uint8_t)(int)t;
    }
}

template <bool VEC>
__global__ __launch_bounds__(PW_THREADS) void latent_mix_kernel(const float* __restrict__ a, const float* __restrict__ b, float c0,
                                                                float c1, float* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * PW_THREADS + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= n) return;
    if (VEC && i + 4 <= n) {
        const f32x4 va = load4(a + i), vb = load4(b + i);
        store4(out + i, va * c0 + vb * c1);
    } else {
        for (int64_t j = i; j < n && j < i + (VEC ? 4 : 1); ++j) out[j] = a[j] * c0 + b[j] * c1;
    }
}

// One axis of psg_resample_u8: k == 0 is the skipped pass (equal sizes, no tables); else the HOST copy of the bounds is checked
int check_axis(const char* axis, int in_size, int out_size, const int32_t* bounds_host, const int32_t* bounds, const int32_t* coef,
               int k) {
    PSG_REQUIRE(k >= 0, PSG_ERR_SHAPE, "psg_resample_u8: %s tap width %d is negative", axis, k);
    if (k == 0) {
        PSG_REQUIRE(in_size == out_size, PSG_ERR_SHAPE, "psg_resample_u8: %s pass skipped (tap width 0) but the sizes differ: %d -> %d",
                    axis, in_size, out_size);
        return PSG_OK;
    }
    PSG_REQUIRE(bounds_host && bounds && coef, PSG_ERR_ARG, "psg_resample_u8: null %s table", axis);
    for (int i = 0; i < out_size; ++i) {
        const int64_t first = bounds_host[2 * i], count = bounds_host[2 * i + 1];
        PSG_REQUIRE(first >= 0 && count >= 0 && count <= k && first + count <= in_size, PSG_ERR_SHAPE,
                    "psg_resample_u8: %s bounds row %d (first %lld, taps %lld) reaches outside the input of %d or the table width %d",
                    axis, i, (long long)first, (long long)count, in_size, k);
    }
    return PSG_OK;
}

}  // namespace

extern "C" {

int psg_resample_u8(const uint8_t* src, uint8_t* out_u8, float* out_f32, const float* lut, int B, int Hin, int Win, int C, int Hout,
                    int Wout, const int32_t* xbounds_host, const int32_t* xbounds, const int32_t* xcoef, int kx,
                    const int32_t* ybounds_host, const int32_t* ybounds, const int32_t* ycoef, int ky, void* ws, int64_t ws_bytes,
                    psg_stream_t stream) {
    PSG_REQUIRE(src && (out_u8 || out_f32), PSG_ERR_ARG, "psg_resample_u8: null pointer (src, or both outputs)");
    PSG_REQUIRE(B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, PSG_ERR_SHAPE,
                "psg_resample_u8: B=%d Hin=%d Win=%d Hout=%d Wout=%d must be positive", B, Hin, Win, Hout, Wout);
    PSG_REQUIRE(C >= 1 && C <= 4, PSG_ERR_SHAPE, "psg_resample_u8: C=%d outside 1..4", C);
    PSG_REQUIRE(B <= MAX_BATCH && Hin <= MAX_DIM && Win <= MAX_DIM && Hout <= MAX_DIM && Wout <= MAX_DIM, PSG_ERR_SHAPE,
                "psg_resample_u8: B=%d (max %d) or a side (max %d) too large", B, MAX_BATCH, MAX_DIM);
    PSG_REQUIRE(!out_f32 || (C >= 3 && lut), PSG_ERR_ARG, "psg_resample_u8: the fp32 output needs C >= 3 (C=%d) and the 256-entry table", C);
    if (int rc = check_axis("horizontal", Win, Wout, xbounds_host, xbounds, xcoef, kx)) return rc;
    if (int rc = check_axis("vertical", Hin, Hout, ybounds_host, ybounds, ycoef, ky)) return rc;
    const int64_t need = kx && ky ? (int64_t)B * Hin * Wout * C : 0;
    PSG_REQUIRE(need == 0 || (ws && ws_bytes >= need), PSG_ERR_WORKSPACE, "psg_resample_u8: workspace of %lld bytes, %lld needed",
                (long long)(ws ? ws_bytes : 0), (long long)need);

    const hipStream_t s = (hipStream_t)stream;
    const Emit o = {out_u8, out_f32, lut};
    const dim3 block(RS_LANES, RS_WAVES);
    const int cols = (Wout * C + RS_LANES - 1) / RS_LANES;
    const dim3 hgrid(cols, (Hin + RS_WAVES * H_ROWS - 1) / (RS_WAVES * H_ROWS), B), vgrid(cols, (Hout + RS_WAVES - 1) / RS_WAVES, B);
    uint8_t* mid = static_cast<uint8_t*>(ws);
    if (kx && ky) {
        hipLaunchKernelGGL(resample_h_kernel<false>, hgrid, block, 0, s, src, mid, o, xbounds, xcoef, kx, Hin, Win, Wout, C);
        PSG_LAUNCH_CHECK("resample_h_kernel");
        hipLaunchKernelGGL(resample_v_kernel, vgrid, block, 0, s, mid, o, ybounds, ycoef, ky, Hin, Hout, Wout, C);
        PSG_LAUNCH_CHECK("resample_v_kernel");
    } else if (kx) {
        hipLaunchKernelGGL(resample_h_kernel<true>, hgrid, block, 0, s, src, mid, o, xbounds, xcoef, kx, Hin, Win, Wout, C);
        PSG_LAUNCH_CHECK("resample_h_kernel");
    } else if (ky) {
        hipLaunchKernelGGL(resample_v_kernel, vgrid, block, 0, s, src, o, ybounds, ycoef, ky, Hin, Hout, Wout, C);
        PSG_LAUNCH_CHECK("resample_v_kernel");
    } else {
        hipLaunchKernelGGL(resample_copy_kernel, vgrid, block, 0, s, src, o, Hout, Wout, C);
        PSG_LAUNCH_CHECK("resample_copy_kernel");
    }
    return PSG_OK;
}

int psg_image_to_u8(const float* img, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, uint8_t* out, int B,
                    int H, int W, psg_stream_t stream) {
    PSG_REQUIRE(img && out, PSG_ERR_ARG, "psg_image_to_u8: null pointer");
    PSG_REQUIRE(B > 0 && H > 0 && W > 0, PSG_ERR_SHAPE, "psg_image_to_u8: B=%d H=%d W=%d must be positive", B, H, W);
    PSG_REQUIRE(B <= MAX_BATCH && H <= MAX_BATCH && W <= MAX_DIM, PSG_ERR_SHAPE, "psg_image_to_u8: B=%d, H=%d (max %d) or W=%d (max %d) too large",
                B, H, MAX_BATCH, W, MAX_DIM);
    PSG_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, PSG_ERR_SHAPE,
                "psg_image_to_u8: negative stride (%lld, %lld, %lld, %lld)", (long long)stride_b, (long long)stride_c,
                (long long)stride_h, (long long)stride_w);
    hipLaunchKernelGGL(image_to_u8_kernel, dim3((W + PW_THREADS - 1) / PW_THREADS, H, B), dim3(PW_THREADS), 0, (hipStream_t)stream, img,
                       stride_b, stride_c, stride_h, stride_w, out, H, W);
    PSG_LAUNCH_CHECK("image_to_u8_kernel");
    return PSG_OK;
}

int psg_latent_mix_f32(const float* a, const float* b, float c0, float c1, float* out, int64_t n, psg_stream_t stream) {
    PSG_REQUIRE(a && b && out, PSG_ERR_ARG, "psg_latent_mix_f32: null pointer");
    PSG_REQUIRE(n > 0 && n <= ((int64_t)1 << 31), PSG_ERR_SHAPE, "psg_latent_mix_f32: n=%lld must be positive (max 2^31)", (long long)n);
    const bool vec = aligned16(a) && aligned16(b) && aligned16(out);
    const int64_t lanes = vec ? (n + 3) / 4 : n;
    const dim3 grid((unsigned)((lanes + PW_THREADS - 1) / PW_THREADS));
    if (vec) hipLaunchKernelGGL(latent_mix_kernel<true>, grid, dim3(PW_THREADS), 0, (hipStream_t)stream, a, b, c0, c1, out, n);
    else hipLaunchKernelGGL(latent_mix_kernel<false>, grid, dim3(PW_THREADS), 0, (hipStream_t)stream, a, b, c0, c1, out, n);
    PSG_LAUNCH_CHECK("latent_mix_kernel");
    return PSG_OK;
}

}  // extern "C"
