// Attention backward for FEW keys and VERY MANY queries: the text cross-attention of the VAE decoder
// (src/models/vae_decoder.py:49-65; S = 32 text tokens, L = 27^2 ... 215^2 pixels, head_dim 64 ... 4), differentiated by
// stage 3 (final_trainer.py:215-236 back-propagates the image loss through the frozen decoder into text_emb).
//
// psg_attn_bwd's dK/dV kernel gives one workgroup a 16-key tile and walks all L queries serially: ceil(S/16) * B * heads
// workgroups, 64 at the stage-3 batch.  Here the grid is over QUERY SLABS x (b, head):
//   * a workgroup stages the K / V rows of its head once (32-key tiles; one tile when S <= 32) and walks the 64-query tiles
//     of its slab: Q (pre-scaled), dO and delta = rowsum(dO * O) are staged per tile, P is recomputed from lse, dS = P (dP - delta);
//   * dq rows are written directly;
//   * dS^T Q and P^T dO are accumulated in registers over the slab (thread = one key x a 4-wide column chunk; for
//     head_dim < 32 the spare threads split the tile's queries and are summed through LDS in a fixed order) and stored as one
//     fp32 partial [2][S][d] per slab in the workspace;
//   * attn_longq_reduce_kernel sums the slab partials in slab order and writes dk / dv in the element type.
// No atomics anywhere: the same inputs give the same bits.  fp32 accumulation, fused multiply-adds.
#include "attention.h"
#include <type_traits>

namespace psg {

constexpr int LQ_TQ = 64;         // queries per tile
constexpr int LQ_KT = 32;         // keys per tile
constexpr int LQ_PS = LQ_KT + 1;  // row stride of the P / dS tiles
constexpr int LQ_MAX_TPS = 16;    // query tiles per slab, at most
constexpr int LQ_MAX_S = 256;

// row stride of the Q / dO tiles: rows start 16-byte aligned and 16 lanes reading 16 bytes of 16 different rows touch all 64
// banks once (stride = 4 mod 8 words)
template <int D> struct LqGeom {
    static constexpr int D4 = D / 4;
    static constexpr int QS = D == 4 ? 4 : D + 4;
    static constexpr int NCQ = D4 >= 4 ? D4 / 4 : 1;      // dq: column chunks per thread (thread = query x chunk part)
    static constexpr int NCK = D4 >= 8 ? D4 / 8 : 1;      // dk/dv: column chunks per thread (thread = key x chunk part)
    static constexpr int NG = D4 >= 8 ? 1 : 8 / D4;       // dk/dv: query groups sharing a (key, chunk)
    static constexpr size_t lds_floats = (size_t)2 * LQ_TQ * QS + 2 * LQ_TQ * LQ_PS + 2 * LQ_KT * D + 2 * LQ_TQ + (NG > 1 ? 256 * 8 : 0);
};

__device__ __forceinline__ f32x4 fma4(float a, f32x4 b, f32x4 c) {
    f32x4 r = {__builtin_fmaf(a, b[0], c[0]), __builtin_fmaf(a, b[1], c[1]), __builtin_fmaf(a, b[2], c[2]), __builtin_fmaf(a, b[3], c[3])};
    return r;
}
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float c) {
    return __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], __builtin_fmaf(a[0], b[0], c))));
}

// ws: [B*heads][nslab][2][S][D] fp32
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_longq_kernel(const AttnArgs<T> p, float* __restrict__ ws, int tps, int nslab) {
    using G = LqGeom<D>;
    constexpr int D4 = G::D4, QS = G::QS, NCQ = G::NCQ, NCK = G::NCK, NG = G::NG;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm;                          // [TQ][QS] scaled queries
    float* Gs = Qs + LQ_TQ * QS;             // [TQ][QS] dO
    float* Ps = Gs + LQ_TQ * QS;             // [TQ][PS] P
    float* Ds = Ps + LQ_TQ * LQ_PS;          // [TQ][PS] dS
    float* Ks = Ds + LQ_TQ * LQ_PS;          // [KT][D]
    float* Vs = Ks + LQ_KT * D;              // [KT][D]
    float* lses = Vs + LQ_KT * D;            // [TQ]
    float* dels = lses + LQ_TQ;              // [TQ]
    float* red = dels + LQ_TQ;               // [256][8] (NG > 1)

    const int tid = threadIdx.x;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int slab = blockIdx.x;
    const int ntiles = (p.L + LQ_TQ - 1) / LQ_TQ;
    const int t0 = slab * tps, t1 = min(ntiles, t0 + tps);
    const int nkt = (p.S + LQ_KT - 1) / LQ_KT;
    const T* qg = p.q + (int64_t)b * p.L * p.ldq + h * D;
    const T* kg = p.k + (int64_t)b * p.S * p.ldk + h * D;
    const T* vg = p.v + (int64_t)b * p.S * p.ldv + h * D;
    const T* og = p.o + (int64_t)b * p.L * p.ldo + h * D;
    const T* gg = p.dout + (int64_t)b * p.L * p.lddo + h * D;
    T* dqg = p.dq + (int64_t)b * p.L * p.lddq + h * D;
    const float* lse = p.lse + (int64_t)bh * p.L;
    float* delta = p.delta + (int64_t)bh * p.L;
    float* part = ws + ((int64_t)bh * nslab + slab) * 2 * p.S * D;

    // phase A: queries qp, qp + 32 x keys 4 ka .. 4 ka + 3
    const int qp = tid & 31, ka = tid >> 5;
    // dq: query qr x column chunks qc + 4 i
    const int qr = tid & 63, qc = tid >> 6;
    // dk / dv: key ks x column chunks kc + 8 i, queries kgp + NG j
    const int ks = tid & 31, krest = tid >> 5;
    const int kc = NG > 1 ? krest % D4 : krest, kgp = NG > 1 ? krest / D4 : 0;

    f32x4 accK[NCK], accV[NCK];
#pragma unroll
    for (int i = 0; i < NCK; ++i) { accK[i] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    // the slab's dS^T Q / P^T dO of key tile kt -> the workspace partial (first: store; later visits of a key tile: add, by
    // the thread that stored it)
    auto flush = [&](int kt, bool first) {
        if (NG > 1) {
            *reinterpret_cast<f32x4*>(red + tid * 8) = accK[0];
            *reinterpret_cast<f32x4*>(red + tid * 8 + 4) = accV[0];
            __syncthreads();
            if (kgp == 0) {
#pragma unroll
                for (int g = 1; g < NG; ++g) {
                    const int t = ks + 32 * (g * D4 + kc);
                    const f32x4 a = *reinterpret_cast<const f32x4*>(red + t * 8), c = *reinterpret_cast<const f32x4*>(red + t * 8 + 4);
                    accK[0] += a; accV[0] += c;
                }
            }
        }
        const int s = kt * LQ_KT + ks;
        if (kgp == 0 && s < p.S) {
#pragma unroll
            for (int i = 0; i < NCK; ++i) {
                float* pk = part + (int64_t)s * D + (kc + 8 * i) * 4;
                float* pv = pk + (int64_t)p.S * D;
                f32x4 a = accK[i], c = accV[i];
                if (!first) { a += *reinterpret_cast<const f32x4*>(pk); c += *reinterpret_cast<const f32x4*>(pv); }
                *reinterpret_cast<f32x4*>(pk) = a;
                *reinterpret_cast<f32x4*>(pv) = c;
            }
        }
    };

    for (int t = t0; t < t1; ++t) {
        const int l0 = t * LQ_TQ;
        __syncthreads();                                   // the previous tile's readers are done
        for (int e = tid; e < LQ_TQ * D4; e += 256) {      // (whole waves: LQ_TQ * D4 is a multiple of 64)
            const int r = e / D4, c = e - r * D4, l = l0 + r;
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f}, g4 = q4;
            float dl = 0.f;
            if (l < p.L) {
                q4 = load4<T>(qg + (int64_t)l * p.ldq + c * 4) * p.scale;
                g4 = load4<T>(gg + (int64_t)l * p.lddo + c * 4);
                dl = dot4(g4, load4<T>(og + (int64_t)l * p.ldo + c * 4), 0.f);
            }
#pragma unroll
            for (int o = D4 >> 1; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);      // the D4 adjacent lanes of a row
            *reinterpret_cast<f32x4*>(Qs + r * QS + c * 4) = q4;
            *reinterpret_cast<f32x4*>(Gs + r * QS + c * 4) = g4;
            if (c == 0) {
                dels[r] = dl;
                lses[r] = l < p.L ? lse[l] : 0.f;
                if (l < p.L) delta[l] = dl;
            }
        }
        f32x4 accQ[NCQ];
#pragma unroll
        for (int i = 0; i < NCQ; ++i) accQ[i] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int kt = 0; kt < nkt; ++kt) {
            if (nkt > 1 || t == t0) {
                for (int e = tid; e < LQ_KT * D4; e += 256) {
                    const int r = e / D4, c = e - r * D4, s = kt * LQ_KT + r;
                    f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = k4;
                    if (s < p.S) { k4 = load4<T>(kg + (int64_t)s * p.ldk + c * 4); v4 = load4<T>(vg + (int64_t)s * p.ldv + c * 4); }
                    *reinterpret_cast<f32x4*>(Ks + r * D + c * 4) = k4;
                    *reinterpret_cast<f32x4*>(Vs + r * D + c * 4) = v4;
                }
            }
            __syncthreads();
            {   // P, dS of (queries qp, qp + 32) x (keys 4 ka .. 4 ka + 3)
                float sc[2][4], dp[2][4];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { sc[i][j] = 0.f; dp[i][j] = 0.f; }
#pragma unroll 2
                for (int c = 0; c < D4; ++c) {      // (not unrolled further: the loads of every chunk hoisted at once spill)
                    const f32x4 qa = *reinterpret_cast<const f32x4*>(Qs + qp * QS + c * 4), qb = *reinterpret_cast<const f32x4*>(Qs + (qp + 32) * QS + c * 4);
                    const f32x4 ga = *reinterpret_cast<const f32x4*>(Gs + qp * QS + c * 4), gb = *reinterpret_cast<const f32x4*>(Gs + (qp + 32) * QS + c * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 k4 = *reinterpret_cast<const f32x4*>(Ks + (ka * 4 + j) * D + c * 4);
                        const f32x4 v4 = *reinterpret_cast<const f32x4*>(Vs + (ka * 4 + j) * D + c * 4);
                        sc[0][j] = dot4(qa, k4, sc[0][j]); sc[1][j] = dot4(qb, k4, sc[1][j]);
                        dp[0][j] = dot4(ga, v4, dp[0][j]); dp[1][j] = dot4(gb, v4, dp[1][j]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int r = qp + 32 * i;
                    const float ls = lses[r], dl = dels[r];
                    const bool row_ok = l0 + r < p.L;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = row_ok && kt * LQ_KT + ka * 4 + j < p.S;
                        const float pr = ok ? __expf(sc[i][j] - ls) : 0.f;
                        Ps[r * LQ_PS + ka * 4 + j] = pr;
                        Ds[r * LQ_PS + ka * 4 + j] = pr * (dp[i][j] - dl);
                    }
                }
            }
            __syncthreads();
            if (qc < D4) {       // dq += dS K
#pragma unroll 4
                for (int s = 0; s < LQ_KT; ++s) {
                    const float ds = Ds[qr * LQ_PS + s];
#pragma unroll
                    for (int i = 0; i < NCQ; ++i) accQ[i] = fma4(ds, *reinterpret_cast<const f32x4*>(Ks + s * D + (qc + 4 * i) * 4), accQ[i]);
                }
            }
            // dk += dS^T Q (Q carries `scale`), dv += P^T dO
#pragma unroll 4
            for (int r = kgp; r < LQ_TQ; r += NG) {
                const float pr = Ps[r * LQ_PS + ks], ds = Ds[r * LQ_PS + ks];
#pragma unroll
                for (int i = 0; i < NCK; ++i) {
                    accK[i] = fma4(ds, *reinterpret_cast<const f32x4*>(Qs + r * QS + (kc + 8 * i) * 4), accK[i]);
                    accV[i] = fma4(pr, *reinterpret_cast<const f32x4*>(Gs + r * QS + (kc + 8 * i) * 4), accV[i]);
                }
            }
            if (nkt > 1) {       // (workgroup-uniform) more key tiles than the registers hold: one partial visit per (tile, key tile)
                flush(kt, t == t0);
#pragma unroll
                for (int i = 0; i < NCK; ++i) { accK[i] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                __syncthreads();
            }
        }
        const int l = l0 + qr;
        if (qc < D4 && l < p.L) {
#pragma unroll
            for (int i = 0; i < NCQ; ++i) store4<T>(dqg + (int64_t)l * p.lddq + (qc + 4 * i) * 4, accQ[i] * p.scale);
        }
    }
    if (nkt == 1) flush(0, true);
}

// dk, dv = the slab partials summed in slab order
template <typename T>
__global__ __launch_bounds__(256) void attn_longq_reduce_kernel(const AttnArgs<T> p, const float* __restrict__ ws, int nslab) {
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int which = blockIdx.z;
    const int n = p.S * p.d;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float* src = ws + (int64_t)bh * nslab * 2 * n + (int64_t)which * n + e;
    float acc = 0.f;
    for (int i = 0; i < nslab; ++i) acc += src[(int64_t)i * 2 * n];
    const int s = e / p.d, c = e - s * p.d;
    T* dst = which ? p.dv + ((int64_t)b * p.S + s) * p.lddv : p.dk + ((int64_t)b * p.S + s) * p.lddk;
    Elem<T>::st(dst + h * p.d + c, acc);
}

using LqDims = std::integer_sequence<int, 4, 8, 16, 32, 64>;

// query tiles per slab: enough workgroups for four rounds of the chip where the problem has them, at most LQ_MAX_TPS tiles a slab
static int lq_tps(int B, int heads, int L) {
    const int64_t ntiles = (L + LQ_TQ - 1) / LQ_TQ;
    const int64_t t = ntiles * B * heads / 1024;
    return (int)(t < 1 ? 1 : (t > LQ_MAX_TPS ? LQ_MAX_TPS : t));
}
static int lq_nslab(int B, int heads, int L) {
    const int ntiles = (L + LQ_TQ - 1) / LQ_TQ, tps = lq_tps(B, heads, L);
    return (ntiles + tps - 1) / tps;
}

template <typename T>
static int longq_init_attrs_t() {
    int rc = PSG_OK;
    for_each_nd(LqDims{}, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        rc = set_max_lds((int)(LqGeom<D>::lds_floats * sizeof(float)), attn_longq_kernel<T, D>);
        return rc;
    });
    return rc;
}

int attn_longq_init_attrs() {
    { int rc = longq_init_attrs_t<float>(); if (rc) return rc; }
    return longq_init_attrs_t<bf16_t>();
}

}  // namespace psg
using namespace psg;

extern "C" {

int64_t psg_attn_bwd_longq_workspace_bytes(int B, int heads, int L, int S, int d) {
    if (B <= 0 || heads <= 0 || L <= 0 || S <= 0 || d <= 0) return set_error(PSG_ERR_SHAPE, "attn_bwd_longq_workspace_bytes: non-positive dimension");
    return (int64_t)B * heads * lq_nslab(B, heads, L) * 2 * S * d * (int64_t)sizeof(float);
}

int psg_attn_bwd_longq(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                       int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta, void* dq, int64_t lddq,
                       void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int heads, int L, int S, int d, float scale,
                       float drop_p, uint64_t seed, int dtype, void* ws, int64_t ws_bytes, psg_stream_t stream) {
    const char* who = "attn_bwd_longq";
    PSG_REQUIRE(q && k && v && o && dout && lse && delta && dq && dk && dv, PSG_ERR_ARG, "%s: null pointer", who);
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "%s: dtype %d", who, dtype);
    PSG_REQUIRE(drop_p == 0.f, PSG_ERR_ARG, "%s: no dropout on this path, drop_p must be 0 (got %g)", who, (double)drop_p);
    PSG_REQUIRE(B > 0 && heads > 0 && L > 0 && S > 0, PSG_ERR_SHAPE, "%s: non-positive dimension", who);
    PSG_REQUIRE(d == 4 || d == 8 || d == 16 || d == 32 || d == 64, PSG_ERR_SHAPE, "%s: head_dim %d is not one of 4, 8, 16, 32, 64", who, d);
    PSG_REQUIRE(S <= LQ_MAX_S, PSG_ERR_SHAPE, "%s: S=%d exceeds %d keys", who, S, LQ_MAX_S);
    const int64_t hd = (int64_t)heads * d;
    PSG_REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd && lddo >= hd && lddq >= hd && lddk >= hd && lddv >= hd, PSG_ERR_SHAPE,
                "%s: row stride < heads*d", who);
    PSG_REQUIRE(((ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv) & 3) == 0, PSG_ERR_ALIGN, "%s: row strides must be multiples of 4", who);
    PSG_REQUIRE((int64_t)B * heads <= 65535, PSG_ERR_SHAPE, "%s: B*heads=%ld exceeds grid.y", who, (long)B * heads);
    const bool al = dtype == PSG_BF16 ? aligned8(q) && aligned8(k) && aligned8(v) && aligned8(o) && aligned8(dout) && aligned8(dq)
                                      : aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && aligned16(dout) && aligned16(dq);
    PSG_REQUIRE(al, PSG_ERR_ALIGN, "%s: q, k, v, o, dout and dq must start on a 4-element boundary", who);
    const int64_t need = psg_attn_bwd_longq_workspace_bytes(B, heads, L, S, d);
    PSG_REQUIRE(ws && ws_bytes >= need && aligned16(ws), PSG_ERR_WORKSPACE, "%s: workspace of %ld bytes, %ld needed (16-byte aligned)", who,
                (long)ws_bytes, (long)need);
    hipStream_t s = (hipStream_t)stream;
    const int tps = lq_tps(B, heads, L), nslab = lq_nslab(B, heads, L);
    int rc = PSG_OK;
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        AttnArgs<T> p = {};
        p.q = (const T*)q; p.k = (const T*)k; p.v = (const T*)v; p.o = (const T*)o; p.dout = (const T*)dout; p.lse = const_cast<float*>(lse); p.delta = delta;
        p.dq = (T*)dq; p.dk = (T*)dk; p.dv = (T*)dv;
        p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
        p.B = B; p.H = heads; p.L = L; p.S = S; p.d = d; p.scale = scale; p.drop_scale = 1.0f; p.seed = seed;
        ProfScope prof(PROF_ATTN, 10.0 * (double)B * heads * L * S * d, s, (double)B * heads * d * (4.0 * L + 4.0 * S) * (double)sizeof(T));
        with_const(LqDims{}, d, [&](auto dc) {
            constexpr int D = decltype(dc)::value;
            hipLaunchKernelGGL((attn_longq_kernel<T, D>), dim3(nslab, B * heads), dim3(256), LqGeom<D>::lds_floats * sizeof(float), s, p, (float*)ws, tps,
                               nslab);
        });
        hipLaunchKernelGGL(attn_longq_reduce_kernel<T>, dim3((S * d + 255) / 256, B * heads, 2), dim3(256), 0, s, p, (const float*)ws, nslab);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, who);
    });
    return rc;
}

}  // extern "C"
