// Multi-head attention core: softmax((q*scale) k^T) v and its backward.
// Shape-general fp32-accumulate kernels (any L, S, head_dim % 4 == 0 up to 320, fp32 or bf16 I/O):
// K/V chunks of 32 keys are staged through LDS (row stride d+1: conflict-free), the [16 x S]
// score slab of a 16-query tile lives in LDS, row softmax is a wave-shuffle reduction, and the
// probabilities never touch HBM.  lse (log-sum-exp) is saved for backward, which recomputes P.
// Problems are tiny and independent (B*heads of them per call): latency/LDS-bound, not MFMA-bound.
#include "attention.h"
#include <type_traits>

namespace psg {

constexpr int AT_Q = 16;      // query rows per workgroup (fwd, dq)
constexpr int AT_KC = 32;     // keys per staged chunk
constexpr int AT_MAXC = 20;   // head_dim <= 16 * AT_MAXC = 320

// dropout element index of P[bh][l][s]: each query row owns ceil(S/2) hash PAIRS (keys 2k, 2k+1 share one 32-bit hash),
// exactly as attention_mfma.hip lays them out - so the VALU and the MFMA kernels draw the SAME mask for every S (odd S
// too: 7x7 self-attention has S = 49) and a forward on one path can be differentiated on the other
template <typename T>
__device__ __forceinline__ uint64_t attn_idx(const AttnArgs<T>& p, int bh, int l, int s) {
    return ((uint64_t)bh * p.L + l) * (uint64_t)(2 * ((p.S + 1) >> 1)) + s;
}

// stage `rows` rows of d elements (global row r at base + r*ld) into LDS with row stride d+1, scaled
template <typename T>
__device__ __forceinline__ void stage_rows(float* dst, const T* base, int64_t ld, int r0, int rows, int rmax, int d, float scl) {
    const int d4 = d >> 2;
    for (int e = threadIdx.x; e < rows * d4; e += blockDim.x) {
        const int r = e / d4, c = (e - r * d4) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < rmax) v = load4<T>(base + (int64_t)(r0 + r) * ld + c);
        float* o = dst + r * (d + 1) + c;
        o[0] = v[0] * scl; o[1] = v[1] * scl; o[2] = v[2] * scl; o[3] = v[3] * scl;
    }
}

// per-sample key bound of the forward kernels: S, or (VARLEN) kv_len[b] clamped to [1, S]
template <bool VARLEN>
__device__ __forceinline__ int key_end(const int32_t* kv_len, int b, int S) {
    if (!VARLEN) return S;
    const int n = kv_len[b];
    return n < 1 ? 1 : (n > S ? S : n);
}

template <typename T, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs<T> p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int d = p.d, dp = d + 1;
    const int Sp = (p.S + 3) & ~3;
    float* Qs = sm;                       // [AT_Q][dp]
    float* Ss = Qs + AT_Q * dp;           // [AT_Q][Sp]
    float* KV = Ss + AT_Q * Sp;           // [AT_KC][dp]
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int l0 = blockIdx.x * AT_Q;
    const T* qg = p.q + (int64_t)b * p.L * p.ldq + h * d;
    const T* kg = p.k + (int64_t)b * p.S * p.ldk + h * d;
    const T* vg = p.v + (int64_t)b * p.S * p.ldv + h * d;
    T* og = p.out + (int64_t)b * p.L * p.ldo + h * d;
    const int tid = threadIdx.x;
    const int Se = key_end<VARLEN>(p.kv_len, b, p.S);

    stage_rows<T>(Qs, qg, p.ldq, l0, AT_Q, p.L, d, p.scale);
    // scores
    for (int s0 = 0; s0 < Se; s0 += AT_KC) {
        __syncthreads();
        stage_rows<T>(KV, kg, p.ldk, s0, AT_KC, Se, d, 1.0f);
        __syncthreads();
        const int kj = tid & 31, qa = tid >> 5, qb = qa + 8;
        const float* kr = KV + kj * dp;
        const float* q0 = Qs + qa * dp;
        const float* q1 = Qs + qb * dp;
        float a0 = 0.f, a1 = 0.f;
        for (int e = 0; e < d; ++e) { const float kv = kr[e]; a0 += q0[e] * kv; a1 += q1[e] * kv; }
        if (s0 + kj < Se) { Ss[qa * Sp + s0 + kj] = a0; Ss[qb * Sp + s0 + kj] = a1; }
    }
    __syncthreads();
    // row softmax: wave w handles rows 4w..4w+3
    {
        const int lane = tid & 63, wv = tid >> 6;
        for (int r = wv * 4; r < wv * 4 + 4; ++r) {
            const int l = l0 + r;
            float* row = Ss + r * Sp;
            float mx = -INFINITY;
            for (int s = lane; s < Se; s += 64) mx = fmaxf(mx, row[s]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int s = lane; s < Se; s += 64) { const float e = __expf(row[s] - mx); row[s] = e; sum += e; }
            sum = wave_sum(sum);
            const float inv = 1.0f / sum;
            for (int s = lane; s < Se; s += 64) {
                float pv = row[s] * inv;
                if (p.drop_thresh && l < p.L) pv = drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, l, s), p.drop_thresh) ? pv * p.drop_scale : 0.f;
                row[s] = pv;
            }
            if (lane == 0 && l < p.L && (!VARLEN || p.lse)) p.lse[(int64_t)bh * p.L + l] = mx + __logf(sum);
        }
    }
    // O = P V
    const int qi = tid >> 4, dd0 = tid & 15;
    const int nc = (d + 15) >> 4;
    float acc[AT_MAXC];
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) acc[c] = 0.f;
    for (int s0 = 0; s0 < Se; s0 += AT_KC) {
        __syncthreads();
        stage_rows<T>(KV, vg, p.ldv, s0, AT_KC, Se, d, 1.0f);
        __syncthreads();
        const int jn = min(AT_KC, Se - s0);
        for (int j = 0; j < jn; ++j) {
            const float pv = Ss[qi * Sp + s0 + j];
            const float* vr = KV + j * dp + dd0;
#pragma unroll
            for (int c = 0; c < AT_MAXC; ++c)
                if (c < nc && dd0 + 16 * c < d) acc[c] += pv * vr[16 * c];
        }
    }
    if (l0 + qi < p.L) {
#pragma unroll
        for (int c = 0; c < AT_MAXC; ++c)
            if (c < nc && dd0 + 16 * c < d) Elem<T>::st(og + (int64_t)(l0 + qi) * p.ldo + dd0 + 16 * c, acc[c]);
    }
}

// delta[bh, l] = sum_d dO * O
template <typename T>
__global__ void attn_delta_kernel(const AttnArgs<T> p) {
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // (b*L + l)*H + h order? use bh-major
    const int lane = threadIdx.x & 63;
    const int64_t total = (int64_t)p.B * p.H * p.L;
    if (row >= total) return;
    const int bh = (int)(row / p.L), l = (int)(row - (int64_t)bh * p.L);
    const int b = bh / p.H, h = bh - b * p.H;
    const T* o = p.o + ((int64_t)b * p.L + l) * p.ldo + h * p.d;
    const T* g = p.dout + ((int64_t)b * p.L + l) * p.lddo + h * p.d;
    float a = 0.f;
    for (int e = lane; e < p.d; e += 64) a += Elem<T>::ld(o + e) * Elem<T>::ld(g + e);
    a = wave_sum(a);
    if (lane == 0) p.delta[row] = a;
}

// dQ for a 16-query tile (VARLEN: over the keys below kv_len[b] only)
template <typename T, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_dq_kernel(const AttnArgs<T> p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int d = p.d, dp = d + 1;
    const int Sp = (p.S + 3) & ~3;
    float* Qs = sm;                       // [AT_Q][dp]  (scaled)
    float* Gs = Qs + AT_Q * dp;           // [AT_Q][dp]  dO
    float* Ss = Gs + AT_Q * dp;           // [AT_Q][Sp]  dS
    float* Ks = Ss + AT_Q * Sp;           // [AT_KC][dp]
    float* Vs = Ks + AT_KC * dp;          // [AT_KC][dp]
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int l0 = blockIdx.x * AT_Q;
    const T* qg = p.q + (int64_t)b * p.L * p.ldq + h * d;
    const T* kg = p.k + (int64_t)b * p.S * p.ldk + h * d;
    const T* vg = p.v + (int64_t)b * p.S * p.ldv + h * d;
    const T* gg = p.dout + (int64_t)b * p.L * p.lddo + h * d;
    T* dqg = p.dq + (int64_t)b * p.L * p.lddq + h * d;
    const int tid = threadIdx.x;
    const int Se = key_end<VARLEN>(p.kv_len, b, p.S);

    stage_rows<T>(Qs, qg, p.ldq, l0, AT_Q, p.L, d, p.scale);
    stage_rows<T>(Gs, gg, p.lddo, l0, AT_Q, p.L, d, 1.0f);
    const int kj = tid & 31, qa = tid >> 5, qb = qa + 8;
    const int la = l0 + qa, lb = l0 + qb;
    const float lse_a = la < p.L ? p.lse[(int64_t)bh * p.L + la] : 0.f;
    const float lse_b = lb < p.L ? p.lse[(int64_t)bh * p.L + lb] : 0.f;
    float del_a = la < p.L ? p.delta[(int64_t)bh * p.L + la] : 0.f;
    float del_b = lb < p.L ? p.delta[(int64_t)bh * p.L + lb] : 0.f;
    if (VARLEN && Se < p.S) {                      // (workgroup-uniform) a sample with masked keys: delta = sum_s drop(P) dP
        // in fp32 from the recomputed probabilities instead of rowsum(dO O).  Few live keys concentrate P; dS = P (dP' - delta)
        // then cancels (exactly, at kv_len = 1) and the rounding of O to the I/O dtype inside delta would be all that is left
        // of dk.  Samples at full length keep psg_attn_bwd's delta (and its bits).  The dK/dV kernel reads what is stored here.
        float part_a = 0.f, part_b = 0.f;
        for (int s0 = 0; s0 < Se; s0 += AT_KC) {
            __syncthreads();
            stage_rows<T>(Ks, kg, p.ldk, s0, AT_KC, Se, d, 1.0f);
            stage_rows<T>(Vs, vg, p.ldv, s0, AT_KC, Se, d, 1.0f);
            __syncthreads();
            const float* kr = Ks + kj * dp; const float* vr = Vs + kj * dp;
            const float* q0 = Qs + qa * dp; const float* q1 = Qs + qb * dp;
            const float* g0 = Gs + qa * dp; const float* g1 = Gs + qb * dp;
            float s_a = 0.f, s_b = 0.f, dp_a = 0.f, dp_b = 0.f;
            for (int e = 0; e < d; ++e) {
                const float kv = kr[e], vv = vr[e];
                s_a += q0[e] * kv; s_b += q1[e] * kv;
                dp_a += g0[e] * vv; dp_b += g1[e] * vv;
            }
            const int s = s0 + kj;
            if (s < Se) {
                if (p.drop_thresh) {
                    dp_a = (la < p.L && drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, la, s), p.drop_thresh)) ? dp_a * p.drop_scale : 0.f;
                    dp_b = (lb < p.L && drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, lb, s), p.drop_thresh)) ? dp_b * p.drop_scale : 0.f;
                }
                part_a += __expf(s_a - lse_a) * dp_a;
                part_b += __expf(s_b - lse_b) * dp_b;
            }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { part_a += __shfl_xor(part_a, o, 64); part_b += __shfl_xor(part_b, o, 64); }   // the 32 key lanes of a query
        del_a = la < p.L ? part_a : 0.f;
        del_b = lb < p.L ? part_b : 0.f;
        if (kj == 0) {
            if (la < p.L) p.delta[(int64_t)bh * p.L + la] = del_a;
            if (lb < p.L) p.delta[(int64_t)bh * p.L + lb] = del_b;
        }
    }
    for (int s0 = 0; s0 < Se; s0 += AT_KC) {
        __syncthreads();
        stage_rows<T>(Ks, kg, p.ldk, s0, AT_KC, Se, d, 1.0f);
        stage_rows<T>(Vs, vg, p.ldv, s0, AT_KC, Se, d, 1.0f);
        __syncthreads();
        const float* kr = Ks + kj * dp; const float* vr = Vs + kj * dp;
        const float* q0 = Qs + qa * dp; const float* q1 = Qs + qb * dp;
        const float* g0 = Gs + qa * dp; const float* g1 = Gs + qb * dp;
        float s_a = 0.f, s_b = 0.f, dp_a = 0.f, dp_b = 0.f;
        for (int e = 0; e < d; ++e) {
            const float kv = kr[e], vv = vr[e];
            s_a += q0[e] * kv; s_b += q1[e] * kv;
            dp_a += g0[e] * vv; dp_b += g1[e] * vv;
        }
        const int s = s0 + kj;
        if (s < Se) {
            float pa = __expf(s_a - lse_a), pb = __expf(s_b - lse_b);
            if (p.drop_thresh) {
                dp_a = (la < p.L && drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, la, s), p.drop_thresh)) ? dp_a * p.drop_scale : 0.f;
                dp_b = (lb < p.L && drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, lb, s), p.drop_thresh)) ? dp_b * p.drop_scale : 0.f;
            }
            Ss[qa * Sp + s] = la < p.L ? pa * (dp_a - del_a) : 0.f;
            Ss[qb * Sp + s] = lb < p.L ? pb * (dp_b - del_b) : 0.f;
        }
    }
    // dQ = scale * dS K
    const int qi = tid >> 4, dd0 = tid & 15;
    const int nc = (d + 15) >> 4;
    float acc[AT_MAXC];
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) acc[c] = 0.f;
    for (int s0 = 0; s0 < Se; s0 += AT_KC) {
        __syncthreads();
        stage_rows<T>(Ks, kg, p.ldk, s0, AT_KC, Se, d, 1.0f);
        __syncthreads();
        const int jn = min(AT_KC, Se - s0);
        for (int j = 0; j < jn; ++j) {
            const float ds = Ss[qi * Sp + s0 + j];
            const float* kr = Ks + j * dp + dd0;
#pragma unroll
            for (int c = 0; c < AT_MAXC; ++c)
                if (c < nc && dd0 + 16 * c < d) acc[c] += ds * kr[16 * c];
        }
    }
    if (l0 + qi < p.L) {
#pragma unroll
        for (int c = 0; c < AT_MAXC; ++c)
            if (c < nc && dd0 + 16 * c < d) Elem<T>::st(dqg + (int64_t)(l0 + qi) * p.lddq + dd0 + 16 * c, acc[c] * p.scale);
    }
}

// dK, dV for a 16-key tile: loops over all queries in chunks of 32 (VARLEN: rows s >= kv_len[b] are written as zeros, and
// K / V rows past the bound are never read)
template <typename T, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_dkv_kernel(const AttnArgs<T> p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int d = p.d, dp = d + 1;
    float* Ks = sm;                        // [16][dp]
    float* Vs = Ks + AT_Q * dp;            // [16][dp]
    float* Qs = Vs + AT_Q * dp;            // [32][dp] scaled
    float* Gs = Qs + AT_KC * dp;           // [32][dp]
    float* Pt = Gs + AT_KC * dp;           // [16][33] P_dropped^T
    float* Dt = Pt + AT_Q * 33;            // [16][33] dS^T
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int s0 = blockIdx.x * AT_Q;
    const T* qg = p.q + (int64_t)b * p.L * p.ldq + h * d;
    const T* kg = p.k + (int64_t)b * p.S * p.ldk + h * d;
    const T* vg = p.v + (int64_t)b * p.S * p.ldv + h * d;
    const T* gg = p.dout + (int64_t)b * p.L * p.lddo + h * d;
    T* dkg = p.dk + (int64_t)b * p.S * p.lddk + h * d;
    T* dvg = p.dv + (int64_t)b * p.S * p.lddv + h * d;
    const int tid = threadIdx.x;
    const int Se = key_end<VARLEN>(p.kv_len, b, p.S);
    const int kj = tid >> 4, dd0 = tid & 15;       // accumulate phase mapping
    const int nc = (d + 15) >> 4;
    if (VARLEN && s0 >= Se) {                      // (workgroup-uniform) a tile of padded keys
        if (s0 + kj < p.S) {
#pragma unroll
            for (int c = 0; c < AT_MAXC; ++c)
                if (c < nc && dd0 + 16 * c < d) {
                    Elem<T>::st(dkg + (int64_t)(s0 + kj) * p.lddk + dd0 + 16 * c, 0.f);
                    Elem<T>::st(dvg + (int64_t)(s0 + kj) * p.lddv + dd0 + 16 * c, 0.f);
                }
        }
        return;
    }
    stage_rows<T>(Ks, kg, p.ldk, s0, AT_Q, Se, d, 1.0f);
    stage_rows<T>(Vs, vg, p.ldv, s0, AT_Q, Se, d, 1.0f);

    float accK[AT_MAXC], accV[AT_MAXC];
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) { accK[c] = 0.f; accV[c] = 0.f; }

    for (int l0 = 0; l0 < p.L; l0 += AT_KC) {
        __syncthreads();
        stage_rows<T>(Qs, qg, p.ldq, l0, AT_KC, p.L, d, p.scale);
        stage_rows<T>(Gs, gg, p.lddo, l0, AT_KC, p.L, d, 1.0f);
        __syncthreads();
        {   // scores for (query qi = tid&31, keys ka = tid>>5, kb = ka+8)
            const int qi = tid & 31, ka = tid >> 5, kb = ka + 8;
            const float* qr = Qs + qi * dp; const float* gr = Gs + qi * dp;
            const float* k0 = Ks + ka * dp; const float* k1 = Ks + kb * dp;
            const float* v0 = Vs + ka * dp; const float* v1 = Vs + kb * dp;
            float s_a = 0.f, s_b = 0.f, dp_a = 0.f, dp_b = 0.f;
            for (int e = 0; e < d; ++e) {
                const float qv = qr[e], gv = gr[e];
                s_a += qv * k0[e]; s_b += qv * k1[e];
                dp_a += gv * v0[e]; dp_b += gv * v1[e];
            }
            const int l = l0 + qi;
            float pa = 0.f, pb = 0.f, da = 0.f, db = 0.f;
            if (l < p.L) {
                const float lse = p.lse[(int64_t)bh * p.L + l], del = p.delta[(int64_t)bh * p.L + l];
                const int sa = s0 + ka, sb = s0 + kb;
                if (sa < Se) {
                    float pr = __expf(s_a - lse), pd = pr;
                    if (p.drop_thresh) {
                        const bool keep = drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, l, sa), p.drop_thresh);
                        pd = keep ? pr * p.drop_scale : 0.f; dp_a = keep ? dp_a * p.drop_scale : 0.f;
                    }
                    pa = pd; da = pr * (dp_a - del);
                }
                if (sb < Se) {
                    float pr = __expf(s_b - lse), pd = pr;
                    if (p.drop_thresh) {
                        const bool keep = drop_keep(eff_seed(p.seed, p.seed_dev), attn_idx(p, bh, l, sb), p.drop_thresh);
                        pd = keep ? pr * p.drop_scale : 0.f; dp_b = keep ? dp_b * p.drop_scale : 0.f;
                    }
                    pb = pd; db = pr * (dp_b - del);
                }
            }
            Pt[ka * 33 + qi] = pa; Pt[kb * 33 + qi] = pb;
            Dt[ka * 33 + qi] = da; Dt[kb * 33 + qi] = db;
        }
        __syncthreads();
        const int jn = min(AT_KC, p.L - l0);
        for (int j = 0; j < jn; ++j) {
            const float pv = Pt[kj * 33 + j], ds = Dt[kj * 33 + j];
            const float* gr = Gs + j * dp + dd0;
            const float* qr = Qs + j * dp + dd0;
#pragma unroll
            for (int c = 0; c < AT_MAXC; ++c)
                if (c < nc && dd0 + 16 * c < d) { accV[c] += pv * gr[16 * c]; accK[c] += ds * qr[16 * c]; }
        }
    }
    if (s0 + kj < p.S) {
        const bool pad = VARLEN && s0 + kj >= Se;
#pragma unroll
        for (int c = 0; c < AT_MAXC; ++c)
            if (c < nc && dd0 + 16 * c < d) {
                Elem<T>::st(dkg + (int64_t)(s0 + kj) * p.lddk + dd0 + 16 * c, pad ? 0.f : accK[c]);   // Qs already carries `scale`
                Elem<T>::st(dvg + (int64_t)(s0 + kj) * p.lddv + dd0 + 16 * c, pad ? 0.f : accV[c]);
            }
    }
}

static size_t fwd_lds(int S, int d) { return sizeof(float) * ((size_t)AT_Q * (d + 1) + (size_t)AT_Q * ((S + 3) & ~3) + (size_t)AT_KC * (d + 1)); }
static size_t dq_lds(int S, int d) { return sizeof(float) * ((size_t)2 * AT_Q * (d + 1) + (size_t)AT_Q * ((S + 3) & ~3) + (size_t)2 * AT_KC * (d + 1)); }
static size_t dkv_lds(int d) { return sizeof(float) * ((size_t)2 * AT_Q * (d + 1) + (size_t)2 * AT_KC * (d + 1) + 2 * AT_Q * 33); }

static int attn_check(const char* who, int B, int heads, int L, int S, int d, int dtype, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo) {
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "%s: dtype %d", who, dtype);
    PSG_REQUIRE(B > 0 && heads > 0 && L > 0 && S > 0 && d > 0, PSG_ERR_SHAPE, "%s: non-positive dimension", who);
    PSG_REQUIRE(d % 4 == 0 && d <= 16 * AT_MAXC, PSG_ERR_SHAPE, "%s: head_dim %d must be a multiple of 4 and <= %d", who, d, 16 * AT_MAXC);
    PSG_REQUIRE(ldq >= heads * d && ldk >= heads * d && ldv >= heads * d && ldo >= heads * d, PSG_ERR_SHAPE, "%s: row stride < heads*d", who);
    PSG_REQUIRE(((ldq | ldk | ldv | ldo) & 3) == 0, PSG_ERR_ALIGN, "%s: row strides must be multiples of 4", who);
    PSG_REQUIRE(S <= 4096, PSG_ERR_SHAPE, "%s: S=%d too long for the LDS score slab", who, S);
    PSG_REQUIRE((int64_t)B * heads <= 65535, PSG_ERR_SHAPE, "%s: B*heads=%ld exceeds grid.y", who, (long)B * heads);
    return PSG_OK;
}

// the VALU kernels of element type T (attention_mfma.hip / attention_f32.hip raise their own)
template <typename T>
static int valu_init_attrs() {
    return set_max_lds(150 * 1024, attn_fwd_kernel<T, false>, attn_fwd_kernel<T, true>, attn_dq_kernel<T, false>, attn_dq_kernel<T, true>,
                       attn_dkv_kernel<T, false>, attn_dkv_kernel<T, true>);
}

static int64_t g_attn_paths[3] = {0, 0, 0};         // launches taken by the bf16 MFMA / the VALU / the fp32 MFMA kernels
static int f32_mfma_on() {
    static int on = -1;                              // PSG_ATTN_F32_MFMA=0: the strict path runs the VALU kernels (A/B)
    if (on < 0) { const char* e = getenv("PSG_ATTN_F32_MFMA"); on = (e && atoi(e) == 0) ? 0 : 1; }
    return on;
}
static int g_attn_allow = 3;                         // psg_attn_set_paths: bit 0 bf16 MFMA, bit 1 exact-fp32 MFMA

enum AttnPass { ATTN_FWD, ATTN_FWD_VARLEN, ATTN_BWD, ATTN_FWD_VARLEN_TRAIN, ATTN_BWD_VARLEN, ATTN_PASSES };
enum AttnFamily { ATTN_MFMA_BF16 = 0, ATTN_VALU = 1, ATTN_MFMA_F32 = 2 };      // (the index in g_attn_paths)
static inline bool pass_bwd(int pass) { return pass == ATTN_BWD || pass == ATTN_BWD_VARLEN; }
static inline bool pass_varlen(int pass) { return pass != ATTN_FWD && pass != ATTN_BWD; }

// the shape checks of a pass's entry point after attn_check: the LDS need of the VALU kernels (every call must be able to
// run on them)
static int attn_check_lds(const char* who, int pass, int S, int d) {
    if (pass_bwd(pass)) {
        const size_t l1 = dq_lds(S, d), l2 = dkv_lds(d);
        PSG_REQUIRE(l1 <= 150 * 1024 && l2 <= 150 * 1024, PSG_ERR_SHAPE, "%s: LDS need too large", who);
    } else {
        const size_t lds = fwd_lds(S, d);
        PSG_REQUIRE(lds <= 150 * 1024, PSG_ERR_SHAPE, "%s: LDS need %zu too large", who, lds);
    }
    return PSG_OK;
}

// The kernel family of one call - the bf16 MFMA kernels, the exact-fp32 MFMA kernels or the VALU kernels.  A forward that a
// backward may follow (plain or varlen_train) and a backward take an MFMA family where both its forward and its backward
// kernels fit LDS, so a training pair stays on one family; the forward-only varlen entry where its forward kernel does.
// ldg: the OR of the gradient row strides (0 for a forward); ptrs_ok: every pointer of the call is aligned as the family's
// vector loads and stores need (attn_route), or what psg_attn_route was told.
static AttnFamily attn_family(int pass, int dtype, int L, int S, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t ldg,
                              bool ptrs_ok) {
    const bool bwd = pass_bwd(pass), fwd_only = pass == ATTN_FWD_VARLEN;
    if (dtype == PSG_BF16) {
        if ((g_attn_allow & 1) && attn_mfma_applicable(L, S, d, ldq, ldk, ldv, ldo, fwd_only) && (!bwd || (ldg & 7) == 0) && ptrs_ok)
            return ATTN_MFMA_BF16;
    } else if ((g_attn_allow & 2) && f32_mfma_on() && attn_f32_applicable(L, S, d, ldq, ldk, ldv, ldo, fwd_only) && (!bwd || (ldg & 3) == 0) && ptrs_ok) {
        return ATTN_MFMA_F32;
    }
    return ATTN_VALU;
}

// the VALU kernels' launches: workgroups of 256 threads, one per 16-query tile (forward, dQ) or 16-key tile (dK/dV) and (b, head)
static AttnPlan valu_plan(int B, int H, int L, int S, int d) {
    AttnPlan pl = {};
    pl.nd = (d + 15) >> 4; pl.waves = pl.dkv_waves = 4;
    pl.nh = 1;
    pl.lds_fwd = fwd_lds(S, d); pl.lds_dq = dq_lds(S, d); pl.lds_dkv = dkv_lds(d);
    pl.grid_q[0] = (L + AT_Q - 1) / AT_Q; pl.grid_kv[0] = (S + AT_Q - 1) / AT_Q; pl.grid_q[1] = pl.grid_kv[1] = B * H;
    return pl;
}

// Launches the call on its family (attn_family), counted in g_attn_paths.
template <typename T>
static int attn_route(AttnPass pass, const AttnArgs<T>& p, hipStream_t s) {
    const bool bwd = pass_bwd(pass), varlen = pass_varlen(pass);
    // (varlen: the FLOP count is the padded problem's, the key lengths live on the device)
    ProfScope prof(PROF_ATTN, (bwd ? 10.0 : 4.0) * (double)p.B * p.H * p.L * p.S * p.d, s,
                   (double)p.B * p.H * p.d * (bwd ? 4.0 * p.L + 4.0 * p.S : 2.0 * p.L + 2.0 * p.S) * (double)sizeof(T));
    constexpr bool BF = std::is_same<T, bf16_t>::value;
    const bool in16 = aligned16(p.q) && aligned16(p.k) && aligned16(p.v);
    const int64_t ldg = p.lddo | p.lddq | p.lddk | p.lddv;
    bool out_ok;
    if constexpr (BF) out_ok = bwd ? aligned16(p.o) && aligned16(p.dout) && aligned8(p.dq) && aligned8(p.dk) && aligned8(p.dv) : aligned8(p.out);
    else out_ok = bwd ? aligned16(p.o) && aligned16(p.dout) && aligned16(p.dq) && aligned16(p.dk) && aligned16(p.dv) : aligned16(p.out);
    const AttnFamily fam = attn_family(pass, BF ? PSG_BF16 : PSG_F32, p.L, p.S, p.d, p.ldq, p.ldk, p.ldv, p.ldo, ldg, in16 && out_ok);
    ++g_attn_paths[fam];
    if constexpr (BF) {
        if (fam == ATTN_MFMA_BF16)
            return bwd ? (varlen ? attn_mfma_bwd<true>(p, s) : attn_mfma_bwd<false>(p, s)) : varlen ? attn_mfma_fwd<true>(p, s) : attn_mfma_fwd<false>(p, s);
    } else {
        if (fam == ATTN_MFMA_F32)
            return bwd ? (varlen ? attn_f32_bwd<true>(p, s) : attn_f32_bwd<false>(p, s)) : varlen ? attn_f32_fwd<true>(p, s) : attn_f32_fwd<false>(p, s);
    }
    const AttnPlan pl = valu_plan(p.B, p.H, p.L, p.S, p.d);
    const dim3 grid(pl.grid_q[0], pl.grid_q[1]), block(64 * pl.waves);
    if (bwd) {
        const int64_t rows = (int64_t)p.B * p.H * p.L;
        hipLaunchKernelGGL(attn_delta_kernel<T>, dim3((int)((rows + 3) / 4)), dim3(256), 0, s, p);
        const dim3 kgrid(pl.grid_kv[0], pl.grid_kv[1]), kblock(64 * pl.dkv_waves);
        if (varlen) {
            hipLaunchKernelGGL((attn_dq_kernel<T, true>), grid, block, pl.lds_dq, s, p);
            hipLaunchKernelGGL((attn_dkv_kernel<T, true>), kgrid, kblock, pl.lds_dkv, s, p);
        } else {
            hipLaunchKernelGGL((attn_dq_kernel<T, false>), grid, block, pl.lds_dq, s, p);
            hipLaunchKernelGGL((attn_dkv_kernel<T, false>), kgrid, kblock, pl.lds_dkv, s, p);
        }
        PSG_LAUNCH_CHECK("attn_bwd");
    } else if (varlen) {
        hipLaunchKernelGGL((attn_fwd_kernel<T, true>), grid, block, pl.lds_fwd, s, p);
        PSG_LAUNCH_CHECK("attn_fwd_varlen");
    } else {
        hipLaunchKernelGGL((attn_fwd_kernel<T, false>), grid, block, pl.lds_fwd, s, p);
        PSG_LAUNCH_CHECK("attn_fwd");
    }
    return PSG_OK;
}

// f((T*)nullptr) for the element type T of dtype (PSG_F32 or PSG_BF16: attn_check has accepted it)
template <typename F>
static int with_elem(int dtype, F&& f) { return dtype == PSG_BF16 ? f((bf16_t*)nullptr) : f((float*)nullptr); }

static int attn_bwd_entry(const char* who, const int32_t* kv_len, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                 int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta, void* dq, int64_t lddq,
                 void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int heads, int L, int S, int d, float scale,
                 float drop_p, uint64_t seed, int dtype, psg_stream_t stream) {
    PSG_REQUIRE(q && k && v && o && dout && lse && delta && dq && dk && dv, PSG_ERR_ARG, "%s: null pointer", who);
    int rc = attn_check(who, B, heads, L, S, d, dtype, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    PSG_REQUIRE(lddo >= heads * d && lddq >= heads * d && lddk >= heads * d && lddv >= heads * d && ((lddo | lddq | lddk | lddv) & 3) == 0,
                PSG_ERR_SHAPE, "%s: gradient row strides", who);        // (psg_attn_route: the same on their OR)
    PSG_REQUIRE(drop_p >= 0.f && drop_p < 1.f, PSG_ERR_ARG, "%s: drop_p", who);
    rc = attn_check_lds(who, ATTN_BWD, S, d);
    if (rc) return rc;
    return with_elem(dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        AttnArgs<T> p = {};
        p.q = (const T*)q; p.k = (const T*)k; p.v = (const T*)v; p.o = (const T*)o; p.dout = (const T*)dout; p.lse = const_cast<float*>(lse); p.delta = delta;
        p.dq = (T*)dq; p.dk = (T*)dk; p.dv = (T*)dv;
        p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
        p.B = B; p.H = heads; p.L = L; p.S = S; p.d = d; p.scale = scale;
        p.drop_thresh = drop_p > 0.f ? drop_thresh(drop_p) : 0u; p.drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f; p.seed = seed; p.seed_dev = seed_source(); p.kv_len = kv_len;
        return attn_route(kv_len ? ATTN_BWD_VARLEN : ATTN_BWD, p, (hipStream_t)stream);
    });
}

}  // namespace psg
using namespace psg;

extern "C" {

int psg_attn_init_attrs(void) {
    { int rc = attn_mfma_init_attrs(); if (rc) return rc; }
    { int rc = attn_f32_init_attrs(); if (rc) return rc; }
    { int rc = attn_longq_init_attrs(); if (rc) return rc; }
    { int rc = valu_init_attrs<float>(); if (rc) return rc; }
    return valu_init_attrs<bf16_t>();
}

int psg_attn_set_paths(int allow_mask) { g_attn_allow = allow_mask & 3; return PSG_OK; }
int psg_attn_path_counts(int64_t* mfma, int64_t* valu, int64_t* mfma_f32) {
    if (mfma) *mfma = g_attn_paths[0];
    if (valu) *valu = g_attn_paths[1];
    if (mfma_f32) *mfma_f32 = g_attn_paths[2];
    return PSG_OK;
}

int psg_attn_route(int pass, int dtype, int B, int heads, int L, int S, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                   int64_t ld_grads, int ptrs_aligned16, int32_t* out) {
    PSG_REQUIRE(out, PSG_ERR_ARG, "attn_route: null pointer");
    PSG_REQUIRE(pass >= 0 && pass < ATTN_PASSES, PSG_ERR_ARG, "attn_route: pass %d", pass);
    int rc = attn_check("attn_route", B, heads, L, S, d, dtype, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    const bool bwd = pass_bwd(pass);
    if (bwd) PSG_REQUIRE(ld_grads >= heads * d && (ld_grads & 3) == 0, PSG_ERR_SHAPE, "attn_route: gradient row strides");
    rc = attn_check_lds("attn_route", pass, S, d);
    if (rc) return rc;
    const AttnFamily fam = attn_family(pass, dtype, L, S, d, ldq, ldk, ldv, ldo, bwd ? ld_grads : 0, ptrs_aligned16 != 0);
    const AttnPlan pl = fam == ATTN_MFMA_BF16 ? attn_mfma_plan(B, heads, L, S, d) : fam == ATTN_MFMA_F32 ? attn_f32_plan(B, heads, L, S, d)
                                                                                  : valu_plan(B, heads, L, S, d);
    // a forward launches no dQ / dK/dV kernel and a backward no forward kernel: their fields are 0
    const int32_t v[PSG_ATTN_ROUTE_FIELDS] = {
        fam, pl.nd, pl.waves, bwd ? pl.kw : 0, bwd ? pl.qw : 0, bwd ? pl.dkv_waves : 0, bwd ? pl.qw_cut : 0, bwd ? pl.w_cut : 0,
        bwd ? pl.nh : 0, bwd ? pl.kv_reg : 0, bwd ? 0 : (int32_t)pl.lds_fwd, bwd ? (int32_t)pl.lds_dq : 0, bwd ? (int32_t)pl.lds_dkv : 0,
        bwd ? 0 : pl.grid_q[0], bwd ? 0 : pl.grid_q[1], bwd ? pl.grid_q[0] : 0, bwd ? pl.grid_q[1] : 0, bwd ? pl.grid_kv[0] : 0,
        bwd ? pl.grid_kv[1] : 0, pass_varlen(pass) ? 1 : 0};
    for (int i = 0; i < PSG_ATTN_ROUTE_FIELDS; ++i) out[i] = v[i];
    return PSG_OK;
}

int psg_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                 float* lse, int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed, int dtype,
                 psg_stream_t stream) {
    PSG_REQUIRE(q && k && v && o && lse, PSG_ERR_ARG, "attn_fwd: null pointer");
    int rc = attn_check("attn_fwd", B, heads, L, S, d, dtype, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    PSG_REQUIRE(drop_p >= 0.f && drop_p < 1.f, PSG_ERR_ARG, "attn_fwd: drop_p");
    rc = attn_check_lds("attn_fwd", ATTN_FWD, S, d);
    if (rc) return rc;
    return with_elem(dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        AttnArgs<T> p = {};
        p.q = (const T*)q; p.k = (const T*)k; p.v = (const T*)v; p.out = (T*)o; p.lse = lse; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
        p.B = B; p.H = heads; p.L = L; p.S = S; p.d = d; p.scale = scale;
        p.drop_thresh = drop_p > 0.f ? drop_thresh(drop_p) : 0u; p.drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f; p.seed = seed; p.seed_dev = seed_source();
        return attn_route(ATTN_FWD, p, (hipStream_t)stream);
    });
}

int psg_attn_fwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                        int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed,
                        int dtype, const int32_t* kv_len, psg_stream_t stream) {
    PSG_REQUIRE(q && k && v && o && kv_len, PSG_ERR_ARG, "attn_fwd_varlen: null pointer");
    int rc = attn_check("attn_fwd_varlen", B, heads, L, S, d, dtype, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    PSG_REQUIRE(drop_p == 0.f, PSG_ERR_ARG, "attn_fwd_varlen: forward-only entry, drop_p must be 0 (got %g)", (double)drop_p);
    rc = attn_check_lds("attn_fwd_varlen", ATTN_FWD_VARLEN, S, d);
    if (rc) return rc;
    return with_elem(dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        AttnArgs<T> p = {};
        p.q = (const T*)q; p.k = (const T*)k; p.v = (const T*)v; p.out = (T*)o; p.lse = lse; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
        p.B = B; p.H = heads; p.L = L; p.S = S; p.d = d; p.scale = scale;
        p.drop_scale = 1.0f; p.seed = seed; p.kv_len = kv_len;
        return attn_route(ATTN_FWD_VARLEN, p, (hipStream_t)stream);
    });
}

int psg_attn_fwd_varlen_train(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                              int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed,
                              int dtype, const int32_t* kv_len, psg_stream_t stream) {
    PSG_REQUIRE(q && k && v && o && lse && kv_len, PSG_ERR_ARG, "attn_fwd_varlen_train: null pointer");
    int rc = attn_check("attn_fwd_varlen_train", B, heads, L, S, d, dtype, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    PSG_REQUIRE(drop_p >= 0.f && drop_p < 1.f, PSG_ERR_ARG, "attn_fwd_varlen_train: drop_p");
    rc = attn_check_lds("attn_fwd_varlen_train", ATTN_FWD_VARLEN_TRAIN, S, d);
    if (rc) return rc;
    return with_elem(dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        AttnArgs<T> p = {};
        p.q = (const T*)q; p.k = (const T*)k; p.v = (const T*)v; p.out = (T*)o; p.lse = lse; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
        p.B = B; p.H = heads; p.L = L; p.S = S; p.d = d; p.scale = scale;
        p.drop_thresh = drop_p > 0.f ? drop_thresh(drop_p) : 0u; p.drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f; p.seed = seed; p.seed_dev = seed_source();
        p.kv_len = kv_len;
        return attn_route(ATTN_FWD_VARLEN_TRAIN, p, (hipStream_t)stream);
    });
}

int psg_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                 int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta, void* dq, int64_t lddq,
                 void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int heads, int L, int S, int d, float scale,
                 float drop_p, uint64_t seed, int dtype, psg_stream_t stream) {
    return attn_bwd_entry("attn_bwd", nullptr, q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, delta, dq, lddq, dk, lddk, dv, lddv, B, heads, L, S, d,
                          scale, drop_p, seed, dtype, stream);
}

int psg_attn_bwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                        int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta, void* dq, int64_t lddq,
                        void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int heads, int L, int S, int d, float scale,
                        float drop_p, uint64_t seed, int dtype, const int32_t* kv_len, psg_stream_t stream) {
    PSG_REQUIRE(kv_len, PSG_ERR_ARG, "attn_bwd_varlen: null pointer");
    return attn_bwd_entry("attn_bwd_varlen", kv_len, q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, delta, dq, lddq, dk, lddk, dv, lddv, B, heads, L, S,
                          d, scale, drop_p, seed, dtype, stream);
}

}  // extern "C"
