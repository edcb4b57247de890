// The training objective beyond uniform eps regression (opt-in; gfx950): v-prediction and per-timestep loss weights
// (Min-SNR) in ONE loss launch that builds its target in registers, and the sampler side of v-prediction.
// All three are single streaming passes; roofline = HBM bandwidth.
#include "psg_common.h"
#include "guided_step.h"

namespace psg {

static inline int obj_grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g > max_blocks) g = max_blocks;
    if (g < 1) g = 1;
    return (int)g;
}

// psg_noise_add_f32's clamp: torch.clamp(x, -3, 3) with NaN kept
__device__ __forceinline__ float obj_clamp3(float x) { return x != x ? x : fminf(fmaxf(x, -3.0f), 3.0f); }

// ---------------------------------------------------------------------------
// weighted SmoothL1 against a target built from (x0, noise, t): deterministic two-stage reduction, the grid and the
// workspace of psg_smooth_l1_f32 (OBJ_BLOCKS partials = psg_reduce_workspace_bytes())
// ---------------------------------------------------------------------------
constexpr int OBJ_BLOCKS = 1024;
constexpr int OBJ_THREADS = 256;

struct LossElem { float term, g; };
__device__ __forceinline__ LossElem loss_elem(float p, float target, float beta) {
    const float d = p - target;
    const float ad = fabsf(d);
    LossElem r;
    if (ad < beta) { r.term = 0.5f * d * d / beta; r.g = d / beta; }
    else { r.term = ad - 0.5f * beta; r.g = d > 0.f ? 1.f : -1.f; }
    return r;
}

// v = A noise - B clamp?(x0): two rounded products and one rounded subtraction
__device__ __forceinline__ float v_target(float a, float c, float x, float nz, int do_clamp) {
    if (do_clamp) x = obj_clamp3(x);
    return __fsub_rn(__fmul_rn(a, nz), __fmul_rn(c, x));
}

// `rows` samples of `per_row` items each; an item is one float (VEC false) or one float4 (VEC true: chw % 4 == 0, so no
// float4 straddles two samples).  The sample index is one division per item, in 32 bits while the item count allows it.
template <bool VEC, int PRED>
__global__ __launch_bounds__(OBJ_THREADS) void diffusion_loss_kernel(
        const float* __restrict__ pred, const float* __restrict__ x0, const float* __restrict__ noise, const int64_t* __restrict__ t,
        const float* __restrict__ tabA, const float* __restrict__ tabB, const float* __restrict__ wtab, float* __restrict__ grad,
        float* __restrict__ target_out, float* __restrict__ partial, int32_t* nan_flag, float beta, float grad_scale, int64_t rows,
        int64_t per_row, int num_t, int do_clamp) {
    __shared__ float red[16];
    constexpr int W = VEC ? 4 : 1;
    const int64_t items = rows * per_row;
    const float inv_n = 1.0f / (float)(items * W);
    const bool narrow = items <= 0x7fffffffll;
    float acc = 0.f;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = narrow ? (int64_t)((uint32_t)i / (uint32_t)per_row) : i / per_row;
        int64_t tb = t[b];
        if (tb < 0 || tb >= num_t) { bad |= PSG_FLAG_T_RANGE; tb = tb < 0 ? 0 : num_t - 1; }
        float a = 0.f, c = 0.f;
        if (PRED == PSG_PRED_V) { a = tabA[tb]; c = tabB[tb]; }
        const float w = wtab ? wtab[tb] : 1.0f;
        const float gw = w * inv_n * grad_scale;
        if (VEC) {
            const f32x4 p = load4<float>(pred + 4 * i), nz = load4<float>(noise + 4 * i);
            f32x4 tg = nz, g;
            if (PRED == PSG_PRED_V) {
                const f32x4 xv = load4<float>(x0 + 4 * i);
#pragma unroll
                for (int e = 0; e < 4; ++e) tg[e] = v_target(a, c, xv[e], nz[e], do_clamp);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const LossElem le = loss_elem(p[e], tg[e], beta);
                acc += w * le.term;
                g[e] = le.g * gw;
                if (isnan(p[e]) || isinf(p[e])) bad |= PSG_FLAG_PRED_BAD;
            }
            if (grad) store4<float>(grad + 4 * i, g);
            if (target_out) store4<float>(target_out + 4 * i, tg);
        } else {
            const float p = pred[i], nz = noise[i];
            const float tg = PRED == PSG_PRED_V ? v_target(a, c, x0[i], nz, do_clamp) : nz;
            const LossElem le = loss_elem(p, tg, beta);
            acc += w * le.term;
            if (isnan(p) || isinf(p)) bad |= PSG_FLAG_PRED_BAD;
            if (grad) grad[i] = le.g * gw;
            if (target_out) target_out[i] = tg;
        }
    }
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
    if (bad && nan_flag) atomicOr(nan_flag, bad);
}

// final stage: one block sums `count` partials in a fixed order
__global__ __launch_bounds__(256) void diffusion_loss_finish_kernel(const float* __restrict__ partial, int count, float* out, float scale,
                                                                    int32_t* nan_flag) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) acc += partial[i];
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float r = s * scale;
        *out = r;
        if (nan_flag && (isnan(r) || isinf(r))) atomicOr(nan_flag, PSG_FLAG_LOSS_BAD);
    }
}

// ---------------------------------------------------------------------------
// sampler side: the DDIM step on a v-predicting network, and v -> eps for the chains that keep their own update
// ---------------------------------------------------------------------------
// n counts float4s when VEC.  psg_guided_update_f32's kernel with the parameterisation as a template argument.
template <bool VEC, int PRED>
__global__ __launch_bounds__(256) void guided_update_pred_kernel(float* x, float* x_copy, const float* __restrict__ pred_c,
                                                                 const float* __restrict__ pred_u, const float* __restrict__ z,
                                                                 const float* __restrict__ tab, int k, const int32_t* __restrict__ step_dev,
                                                                 float w, float clip, int64_t n) {
    int j = *step_dev;
    j = j < 0 ? 0 : (j >= k ? k - 1 : j);
    const GuidedCoef co = {tab[j], tab[k + j], tab[2 * k + j], tab[3 * k + j], tab[4 * k + j]};
    const bool has_u = pred_u != nullptr, has_z = z != nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC) {
            const f32x4 xv = load4<float>(x + 4 * i), pc = load4<float>(pred_c + 4 * i);
            f32x4 pu = {0.f, 0.f, 0.f, 0.f}, zv = {0.f, 0.f, 0.f, 0.f}, r;
            if (has_u) pu = load4<float>(pred_u + 4 * i);
            if (has_z) zv = load4<float>(z + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = guided_elem_pred<PRED>(xv[e], pc[e], pu[e], has_u, w, co, clip, zv[e], has_z);
            store4<float>(x + 4 * i, r);
            if (x_copy) store4<float>(x_copy + 4 * i, r);
        } else {
            const float r = guided_elem_pred<PRED>(x[i], pred_c[i], has_u ? pred_u[i] : 0.f, has_u, w, co, clip, has_z ? z[i] : 0.f, has_z);
            x[i] = r;
            if (x_copy) x_copy[i] = r;
        }
    }
}

// out = eps of the (guided) prediction; out may be pred_c (each element is read before it is written, by the same lane).
// x is read only for PSG_PRED_V.
template <bool VEC, int PRED>
__global__ __launch_bounds__(256) void pred_to_eps_kernel(const float* __restrict__ x, const float* pred_c, const float* __restrict__ pred_u,
                                                          float w, const float* __restrict__ tabA, const float* __restrict__ tabB, int num_t,
                                                          const int32_t* __restrict__ t_dev, float* out, int64_t n) {
    float a = 0.f, c = 0.f;
    if (PRED == PSG_PRED_V) {
        int t = *t_dev;
        t = t < 0 ? 0 : (t >= num_t ? num_t - 1 : t);
        a = tabA[t]; c = tabB[t];
    }
    const bool has_u = pred_u != nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC) {
            const f32x4 pc = load4<float>(pred_c + 4 * i);
            f32x4 pu = {0.f, 0.f, 0.f, 0.f}, xv = {0.f, 0.f, 0.f, 0.f}, r;
            if (has_u) pu = load4<float>(pred_u + 4 * i);
            if (PRED == PSG_PRED_V) xv = load4<float>(x + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = guided_combine(pc[e], pu[e], has_u, w);
                r[e] = PRED == PSG_PRED_V ? __fadd_rn(__fmul_rn(c, xv[e]), __fmul_rn(a, p)) : p;
            }
            store4<float>(out + 4 * i, r);
        } else {
            const float p = guided_combine(pred_c[i], has_u ? pred_u[i] : 0.f, has_u, w);
            out[i] = PRED == PSG_PRED_V ? __fadd_rn(__fmul_rn(c, x[i]), __fmul_rn(a, p)) : p;
        }
    }
}

using Preds = std::integer_sequence<int, PSG_PRED_EPS, PSG_PRED_V>;

}  // namespace psg

using namespace psg;

extern "C" {

int psg_diffusion_loss_f32(const float* pred, const float* x0, const float* noise, const int64_t* t, const float* tabA,
                           const float* tabB, const float* wtab, int prediction, float* grad, float* target_out, float* loss_out,
                           int32_t* nan_flag, float beta, float grad_scale, int64_t B, int64_t chw, int num_t, int do_clamp, void* ws,
                           psg_stream_t stream) {
    PSG_REQUIRE(prediction == PSG_PRED_EPS || prediction == PSG_PRED_V, PSG_ERR_ARG, "diffusion_loss: prediction %d", prediction);
    PSG_REQUIRE(pred && noise && t && loss_out && ws, PSG_ERR_ARG, "diffusion_loss: null pointer");
    PSG_REQUIRE(prediction == PSG_PRED_EPS || (x0 && tabA && tabB), PSG_ERR_ARG, "diffusion_loss: v-prediction needs x0, tabA and tabB");
    PSG_REQUIRE(B >= 0 && chw > 0 && num_t > 0 && beta > 0.f, PSG_ERR_SHAPE, "diffusion_loss: bad shape B=%ld chw=%ld num_t=%d beta=%f",
                (long)B, (long)chw, num_t, (double)beta);
    if (B == 0) return PSG_OK;
    const bool vec = (chw & 3) == 0 && aligned16(pred) && aligned16(noise) && aligned16(grad) && aligned16(target_out) &&
                     (prediction == PSG_PRED_EPS || aligned16(x0));
    const int64_t per_row = vec ? chw / 4 : chw;
    const int g = obj_grid_for(B * per_row, OBJ_THREADS, OBJ_BLOCKS);
    with_const(Bools{}, vec, [&](auto V) {
        with_const(Preds{}, prediction, [&](auto P) {
            hipLaunchKernelGGL((diffusion_loss_kernel<decltype(V)::value, decltype(P)::value>), dim3(g), dim3(OBJ_THREADS), 0, (hipStream_t)stream, pred, x0, noise, t,
                               tabA, tabB, wtab, grad, target_out, (float*)ws, nan_flag, beta, grad_scale, B, per_row, num_t, do_clamp);
        });
    });
    PSG_LAUNCH_CHECK("diffusion_loss");
    hipLaunchKernelGGL(diffusion_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, g, loss_out,
                       1.0f / (float)(B * chw), nan_flag);
    PSG_LAUNCH_CHECK("diffusion_loss_finish");
    return PSG_OK;
}

int psg_guided_update_pred_f32(float* x, float* x_copy, const float* pred_c, const float* pred_u, const float* z, const float* tab, int k,
                               const int32_t* step_dev, float w, float clip, int64_t n, int prediction, psg_stream_t stream) {
    PSG_REQUIRE(x && pred_c && tab && step_dev, PSG_ERR_ARG, "guided_update_pred: null pointer");
    PSG_REQUIRE(clip >= 0.f && k >= 1, PSG_ERR_ARG, "guided_update_pred: clip=%g k=%d", (double)clip, k);
    PSG_REQUIRE(prediction == PSG_PRED_EPS || prediction == PSG_PRED_V, PSG_ERR_ARG, "guided_update_pred: prediction %d", prediction);
    if (n <= 0) return PSG_OK;
    // x_copy = x + n with n % 4 != 0 is off the 16-byte boundary: every pointer is looked at, not only x
    const bool vec = (n & 3) == 0 && aligned16(x) && aligned16(x_copy) && aligned16(pred_c) && aligned16(pred_u) && aligned16(z);
    const int64_t items = vec ? n / 4 : n;
    with_const(Bools{}, vec, [&](auto V) {
        with_const(Preds{}, prediction, [&](auto P) {
            hipLaunchKernelGGL((guided_update_pred_kernel<decltype(V)::value, decltype(P)::value>), dim3(obj_grid_for(items, 256, 2048)), dim3(256), 0,
                               (hipStream_t)stream, x, x_copy, pred_c, pred_u, z, tab, k, step_dev, w, clip, items);
        });
    });
    PSG_LAUNCH_CHECK("guided_update_pred");
    return PSG_OK;
}

int psg_pred_to_eps_f32(const float* x, const float* pred_c, const float* pred_u, float w, const float* tabA, const float* tabB, int num_t,
                        const int32_t* t_dev, int prediction, float* out, int64_t n, psg_stream_t stream) {
    PSG_REQUIRE(prediction == PSG_PRED_EPS || prediction == PSG_PRED_V, PSG_ERR_ARG, "pred_to_eps: prediction %d", prediction);
    PSG_REQUIRE(pred_c && out && t_dev, PSG_ERR_ARG, "pred_to_eps: null pointer");
    PSG_REQUIRE(prediction == PSG_PRED_EPS || (x && tabA && tabB), PSG_ERR_ARG, "pred_to_eps: v-prediction needs x, tabA and tabB");
    PSG_REQUIRE(num_t > 0, PSG_ERR_SHAPE, "pred_to_eps: num_t=%d", num_t);
    if (n <= 0) return PSG_OK;
    if (prediction == PSG_PRED_EPS && !pred_u && out == pred_c) return PSG_OK;      // eps already, in place: nothing to do
    const bool vec = (n & 3) == 0 && aligned16(pred_c) && aligned16(pred_u) && aligned16(out) && (prediction == PSG_PRED_EPS || aligned16(x));
    const int64_t items = vec ? n / 4 : n;
    with_const(Bools{}, vec, [&](auto V) {
        with_const(Preds{}, prediction, [&](auto P) {
            hipLaunchKernelGGL((pred_to_eps_kernel<decltype(V)::value, decltype(P)::value>), dim3(obj_grid_for(items, 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                               x, pred_c, pred_u, w, tabA, tabB, num_t, t_dev, out, items);
        });
    });
    PSG_LAUNCH_CHECK("pred_to_eps");
    return PSG_OK;
}

}  // extern "C"
