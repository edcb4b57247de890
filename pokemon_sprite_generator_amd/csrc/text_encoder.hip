// Row kernels of the BERT text encoder (reference: src/models/text_encoder.py, a transformers BertModel):
//   psg_layernorm      y = LN(x [+ r]) * gamma + beta over rows of width N (BERT's two post-LNs per layer, the final
//                      nn.LayerNorm of the TextEncoder);
//   psg_layernorm_bwd  its backward (fine-tuning): dz, dgamma, dbeta from the forward's operands and dy;
//   psg_bert_embed_ln  BertEmbeddings: LN(word_emb[id] + type_emb[type] + pos_emb[s]);
//   psg_bert_embed_ln_bwd, psg_embed_scatter  its backward (finetune_strategy 'full'): dz in fp32 + dgamma / dbeta, and the
//                      atomic-free sum of dz rows into the word / position / token-type table gradients.
// One wave per row (N = 768: 64 lanes x 12 values), four rows per workgroup and many workgroups per CU in flight.  A lane
// holds its chunks of 8 consecutive values in registers from the load to the store: one pass over HBM each way.
// Statistics are fp32 and reduced in a fixed order (per-lane chunk order, then the xor butterfly, which leaves every lane
// with the same bits): the result does not depend on the launch geometry.  Mean first, then the centred second moment
// (two passes over registers, biased variance, eps inside the square root, as torch's layer_norm).
#include "psg_common.h"

namespace psg {

constexpr int LN_ROWS = 4;          // rows (waves) per workgroup
constexpr int LN_MAXN = 4096;       // 64 lanes x 8 chunks x 8 values

template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float (&v)[8]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
}
template <typename T> __device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
    const f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
}
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float (&v)[8]) {
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (bf16_t)v[j];
    *reinterpret_cast<bf16x8*>(p) = a;
}

// mean and 1/sqrt(var + eps) of the row a wave holds (chunk i of the lane = columns 8*(lane + 64*i) .. +7, valid while
// < nch): the one statement of the statistics - the backward recomputes them with this code, so its x_hat has the forward's bits
template <int CPL>
__device__ __forceinline__ void ln_stats(const float (&v)[CPL][8], int lane, int nch, int N, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        if (lane + 64 * i < nch)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
    mean = wave_sum(s) / (float)N;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        if (lane + 64 * i < nch)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float c = v[i][j] - mean; q += c * c; }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + eps);
}

// normalise the row a wave holds and store it
template <int CPL, typename TO>
__device__ __forceinline__ void ln_store(float (&v)[CPL][8], int lane, int nch, int N, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, float eps, TO* yrow) {
    float mean, rstd;
    ln_stats<CPL>(v, lane, nch, N, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            float g[8], bb[8], o[8];
            ld8<float>(gamma + 8 * c, g);
            ld8<float>(beta + 8 * c, bb);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + bb[j];
            st8<TO>(yrow + 8 * c, o);
        }
    }
}

template <typename TI, typename TO, int CPL, bool RES>
__global__ __launch_bounds__(64 * LN_ROWS) void layernorm_kernel(const TI* __restrict__ x, int64_t ldx, const TI* __restrict__ r,
                                                                  int64_t ldr, TO* __restrict__ y, int64_t ldy,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  int64_t rows, int N, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = N >> 3;
    float v[CPL][8];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            ld8<TI>(x + row * ldx + 8 * c, v[i]);
            if (RES) {
                float t[8];
                ld8<TI>(r + row * ldr + 8 * c, t);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] += t[j];
            }
        }
    }
    ln_store<CPL, TO>(v, lane, nch, N, gamma, beta, eps, y + row * ldy);
}

// BertEmbeddings (eval): inputs_embeds + token_type_embeddings, then + position_embeddings (transformers' order), LayerNorm.
// Row t = b*S + s has position s.  An id outside [0, vocab) or a type id outside [0, type_vocab) reads nothing and yields a
// NaN row: the caller's NaN check then drops the batch.
template <typename TO, int CPL>
__global__ __launch_bounds__(64 * LN_ROWS) void embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ type_ids,
                                                                 const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                                 const float* __restrict__ temb, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, TO* __restrict__ y, int64_t ldy,
                                                                 int64_t rows, int S, int N, int vocab, int type_vocab, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = N >> 3;
    const int s = (int)(row % S);
    const int64_t id = ids[row];
    const int64_t tt = type_ids ? type_ids[row] : 0;
    TO* yrow = y + row * ldy;
    if (id < 0 || id >= vocab || tt < 0 || tt >= type_vocab) {      // (wave-uniform)
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = __builtin_nanf("");
        for (int c = lane; c < nch; c += 64) st8<TO>(yrow + 8 * c, o);
        return;
    }
    const float* wr = wemb + id * N;
    const float* tr = temb + tt * N;
    const float* pr = pemb + (int64_t)s * N;
    float v[CPL][8];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            float a[8], t[8], p[8];
            ld8<float>(wr + 8 * c, a);
            ld8<float>(tr + 8 * c, t);
            ld8<float>(pr + 8 * c, p);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = (a[j] + t[j]) + p[j];
        }
    }
    ln_store<CPL, TO>(v, lane, nch, N, gamma, beta, eps, yrow);
}

// ------------------------------------------------------------------------------------------------ LayerNorm backward
// z = x (+ r), x_hat = (z - mean) rstd (statistics recomputed by ln_stats: nothing but the inputs is saved), g = dy gamma:
//   dz     = rstd (g - mean_N(g) - x_hat mean_N(g x_hat))        one wave per row, chunks in registers from load to store
//   dgamma = sum_rows dy x_hat,  dbeta = sum_rows dy             (PG) a wave walks LNB_RPW consecutive rows and keeps its columns'
// sums in registers; the four waves of a workgroup meet in LDS in wave order, and the workgroup's partial row goes to the
// workspace [2][workgroups][N] (ln_param_sum_kernel adds the workgroups in a fixed order).  No atomics; the grid depends on
// (rows, N) alone, so the bits do not depend on the device.
constexpr int LNB_RPW = 16;                         // rows per wave
constexpr int LNB_WG_ROWS = LN_ROWS * LNB_RPW;      // rows per workgroup

template <typename TI, typename TDY, int CPL, bool PG>
__global__ __launch_bounds__(64 * LN_ROWS) void layernorm_bwd_kernel(const TI* __restrict__ x, int64_t ldx, const TI* __restrict__ r,
                                                                      int64_t ldr, const TDY* __restrict__ dy, int64_t lddy,
                                                                      const float* __restrict__ gamma, TI* __restrict__ dz, int64_t lddz,
                                                                      float* __restrict__ part, int64_t rows, int N, float eps) {
    __shared__ float red[LN_ROWS - 1][2][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = N >> 3;
    const float invN = 1.0f / (float)N;
    float ag[PG ? CPL : 1][8], ab[PG ? CPL : 1][8];
    if (PG) {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { ag[i][j] = 0.f; ab[i][j] = 0.f; }
    }
    const int64_t row0 = ((int64_t)blockIdx.x * LN_ROWS + wave) * LNB_RPW;
    for (int it = 0; it < LNB_RPW; ++it) {
        const int64_t row = row0 + it;
        if (row >= rows) break;                                   // (wave-uniform)
        float v[CPL][8], g[CPL][8];
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                ld8<TI>(x + row * ldx + 8 * c, v[i]);
                if (r) {                                          // (uniform)
                    float t[8];
                    ld8<TI>(r + row * ldr + 8 * c, t);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[i][j] += t[j];
                }
                ld8<TDY>(dy + row * lddy + 8 * c, g[i]);
            }
        }
        float mean, rstd;
        ln_stats<CPL>(v, lane, nch, N, eps, mean, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float gm[8];
                ld8<float>(gamma + 8 * c, gm);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = (v[i][j] - mean) * rstd;
                    if (PG) { ag[i][j] += g[i][j] * xh; ab[i][j] += g[i][j]; }
                    v[i][j] = xh;
                    g[i][j] *= gm[j];
                    s1 += g[i][j];
                    s2 += g[i][j] * xh;
                }
            }
        }
        s1 = wave_sum(s1) * invN;
        s2 = wave_sum(s2) * invN;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = rstd * ((g[i][j] - s1) - v[i][j] * s2);
                st8<TI>(dz + row * lddz + 8 * c, o);
            }
        }
    }
    if (PG) {
        float* pg = part + (int64_t)blockIdx.x * N;
        float* pb = part + ((int64_t)gridDim.x + blockIdx.x) * N;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { red[wave - 1][0][j][lane] = ag[i][j]; red[wave - 1][1][j][lane] = ab[i][j]; }
            }
            __syncthreads();
            if (wave == 0 && c < nch) {
#pragma unroll
                for (int w = 0; w < LN_ROWS - 1; ++w)
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ag[i][j] += red[w][0][j][lane]; ab[i][j] += red[w][1][j][lane]; }
                st8<float>(pg + 8 * c, ag[i]);
                st8<float>(pb + 8 * c, ab[i]);
            }
        }
    }
}

// out[c] (+)= sum over the nwg workgroup partials of column c, for dgamma (blockIdx.y = 0) and dbeta (1): 64 columns x 4
// partial lanes per workgroup, each lane in ascending order, the four lanes in LDS order
__global__ __launch_bounds__(256) void ln_param_sum_kernel(const float* __restrict__ part, int nwg, int N, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int accumulate) {
    __shared__ float red[4][64];
    float* out = blockIdx.y ? dbeta : dgamma;
    if (!out) return;                                             // (workgroup-uniform)
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float a = 0.f;
    if (c < N) {
        const float* base = part + (int64_t)blockIdx.y * nwg * N + c;
        for (int w = rl; w < nwg; w += 4) a += base[(int64_t)w * N];
    }
    red[rl][cl] = a;
    __syncthreads();
    if (rl == 0 && c < N) {
        float v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        if (accumulate) v += out[c];
        out[c] = v;
    }
}

// ------------------------------------------------------------------------------------------- BertEmbeddings backward
// layernorm_bwd_kernel with z = (word[id] + type[tt]) + pos[s] rebuilt from the fp32 tables in embed_ln_kernel's association
// (x_hat has the forward's bits; the forward saves nothing).  dz is fp32 whatever dy's dtype: it is what the table scatters
// sum.  A row whose id or type id is outside its table (a NaN row of the forward) reads no table, gets a zero dz row and
// adds nothing to dgamma / dbeta.
template <typename TDY, int CPL, bool PG>
__global__ __launch_bounds__(64 * LN_ROWS) void embed_ln_bwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ type_ids,
                                                                     const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                                     const float* __restrict__ temb, const float* __restrict__ gamma,
                                                                     const TDY* __restrict__ dy, int64_t lddy, float* __restrict__ dz,
                                                                     float* __restrict__ part, int64_t rows, int S, int N, int vocab,
                                                                     int type_vocab, float eps) {
    __shared__ float red[LN_ROWS - 1][2][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = N >> 3;
    const float invN = 1.0f / (float)N;
    float ag[PG ? CPL : 1][8], ab[PG ? CPL : 1][8];
    if (PG) {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { ag[i][j] = 0.f; ab[i][j] = 0.f; }
    }
    const int64_t row0 = ((int64_t)blockIdx.x * LN_ROWS + wave) * LNB_RPW;
    for (int it = 0; it < LNB_RPW; ++it) {
        const int64_t row = row0 + it;
        if (row >= rows) break;                                   // (wave-uniform)
        const int64_t id = ids[row];
        const int64_t tt = type_ids ? type_ids[row] : 0;
        float* dzrow = dz + row * N;
        if (id < 0 || id >= vocab || tt < 0 || tt >= type_vocab) {      // (wave-uniform)
            const float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int c = lane; c < nch; c += 64) st8<float>(dzrow + 8 * c, o);
            continue;
        }
        const float* wr = wemb + id * N;
        const float* tr = temb + tt * N;
        const float* pr = pemb + (row % S) * N;
        float v[CPL][8], g[CPL][8];
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float a[8], t[8], p[8];
                ld8<float>(wr + 8 * c, a);
                ld8<float>(tr + 8 * c, t);
                ld8<float>(pr + 8 * c, p);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = (a[j] + t[j]) + p[j];
                ld8<TDY>(dy + row * lddy + 8 * c, g[i]);
            }
        }
        float mean, rstd;
        ln_stats<CPL>(v, lane, nch, N, eps, mean, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float gm[8];
                ld8<float>(gamma + 8 * c, gm);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = (v[i][j] - mean) * rstd;
                    if (PG) { ag[i][j] += g[i][j] * xh; ab[i][j] += g[i][j]; }
                    v[i][j] = xh;
                    g[i][j] *= gm[j];
                    s1 += g[i][j];
                    s2 += g[i][j] * xh;
                }
            }
        }
        s1 = wave_sum(s1) * invN;
        s2 = wave_sum(s2) * invN;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = rstd * ((g[i][j] - s1) - v[i][j] * s2);
                st8<float>(dzrow + 8 * c, o);
            }
        }
    }
    if (PG) {                                                     // the workgroup's partial rows, as layernorm_bwd_kernel
        float* pg = part + (int64_t)blockIdx.x * N;
        float* pb = part + ((int64_t)gridDim.x + blockIdx.x) * N;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane + 64 * i;
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { red[wave - 1][0][j][lane] = ag[i][j]; red[wave - 1][1][j][lane] = ab[i][j]; }
            }
            __syncthreads();
            if (wave == 0 && c < nch) {
#pragma unroll
                for (int w = 0; w < LN_ROWS - 1; ++w)
#pragma unroll
                    for (int j = 0; j < 8; ++j) { ag[i][j] += red[w][0][j][lane]; ab[i][j] += red[w][1][j][lane]; }
                st8<float>(pg + 8 * c, ag[i]);
                st8<float>(pb + 8 * c, ab[i]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- embedding-table scatter-add
// table_grad[k] (+)= sum of dz[perm[j]] over the run of sorted positions j with key[j] == k: the inverted-index form, no float
// atomics.  The sorted positions are cut at every multiple of ES_CHUNK, so no run is summed by one wave however long it is:
//   embed_scatter_chunk_kernel  one wave per (chunk, slab of 256 columns) walks its positions in ascending j with the column
//                               sums in registers and, wherever the key changes (and at the chunk's end), stores the sum of
//                               the segment to part[first position of the segment];
//   embed_scatter_sum_kernel    the wave of a run's first position adds the run's segments in chunk order - part[j], then
//                               part[c] for every chunk start c the run reaches - and writes old + sum (the add last) or sum.
// Every sum's order is fixed by (key, perm) alone.  Keys outside [0, V) and key == skip_key contribute nothing and write nothing.
constexpr int ES_CHUNK = 32;        // sorted positions per chunk (psg_embed_scatter_chunk_rows)
constexpr int ES_COLS = 256;        // columns per wave: one f32x4 per lane

__global__ __launch_bounds__(64) void embed_scatter_chunk_kernel(const float* __restrict__ dz, int64_t lddz, const int64_t* __restrict__ key,
                                                                  const int64_t* __restrict__ perm, float* __restrict__ part,
                                                                  int64_t rows, int N, int64_t V, int64_t skip_key) {
    const int col = 4 * ((int)blockIdx.y * 64 + (int)threadIdx.x);
    if (col >= N) return;
    const int64_t j0 = (int64_t)blockIdx.x * ES_CHUNK;
    const int64_t j1 = j0 + ES_CHUNK < rows ? j0 + ES_CHUNK : rows;
    int64_t kcur = key[j0], seg = j0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t jb = j0; jb < j1; jb += 4) {
        int64_t k[4];
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                             // the four rows' loads in flight together
            const int64_t j = jb + u;
            k[u] = j < j1 ? key[j] : -1;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < j1 && k[u] >= 0 && k[u] < V && k[u] != skip_key) v[u] = *reinterpret_cast<const f32x4*>(dz + perm[j] * lddz + col);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = jb + u;
            if (j < j1) {
                if (k[u] != kcur) {                               // (wave-uniform)
                    *reinterpret_cast<f32x4*>(part + seg * N + col) = acc;
                    acc = f32x4{0.f, 0.f, 0.f, 0.f};
                    kcur = k[u];
                    seg = j;
                }
                acc += v[u];
            }
        }
    }
    *reinterpret_cast<f32x4*>(part + seg * N + col) = acc;
}

__global__ __launch_bounds__(256) void embed_scatter_sum_kernel(const float* __restrict__ part, const int64_t* __restrict__ key,
                                                                 float* __restrict__ out, int64_t rows, int N, int64_t V, int64_t skip_key,
                                                                 int accumulate) {
    const int col = 4 * ((int)blockIdx.y * 64 + (int)(threadIdx.x & 63));
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows || col >= N) return;
    const int64_t k = key[j];
    if (k < 0 || k >= V || k == skip_key) return;                 // (wave-uniform, as every branch below)
    if (j > 0 && key[j - 1] == k) return;                         // not the first position of its run
    f32x4 acc = *reinterpret_cast<const f32x4*>(part + j * N + col);
    int64_t c = (j / ES_CHUNK + 1) * ES_CHUNK;
    while (c < rows && key[c] == k) {
        f32x4 v[4] = {};
        int n = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {                             // up to four segments' loads in flight; added in chunk order
            if (c < rows && key[c] == k) {
                v[u] = *reinterpret_cast<const f32x4*>(part + c * N + col);
                c += ES_CHUNK;
                n = u + 1;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < n) acc += v[u];
    }
    float* o = out + k * N + col;
    if (accumulate) acc = *reinterpret_cast<const f32x4*>(o) + acc;
    *reinterpret_cast<f32x4*>(o) = acc;
}

__global__ __launch_bounds__(256) void zero_f32x4_kernel(float* __restrict__ p, int64_t n4) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) reinterpret_cast<f32x4*>(p)[i] = z;
}

using LnCpls = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;      // 16-byte chunks per lane: every N row_width_check admits

static int row_width_check(const char* who, int N) {
    PSG_REQUIRE(N >= 8 && N <= LN_MAXN && N % 8 == 0, PSG_ERR_SHAPE, "%s: row width N=%d must be a multiple of 8 in [8, %d]", who, N, LN_MAXN);
    return PSG_OK;
}

}  // namespace psg
using namespace psg;

extern "C" {

int psg_layernorm(const void* x, int64_t ldx, const void* r, int64_t ldr, void* y, int64_t ldy, const float* gamma,
                  const float* beta, int64_t rows, int N, float eps, int x_dtype, int y_dtype, psg_stream_t stream) {
    PSG_REQUIRE(x && y && gamma && beta, PSG_ERR_ARG, "layernorm: null pointer");
    PSG_REQUIRE((x_dtype == PSG_F32 || x_dtype == PSG_BF16) && (y_dtype == PSG_F32 || y_dtype == PSG_BF16), PSG_ERR_DTYPE,
                "layernorm: dtypes %d -> %d", x_dtype, y_dtype);
    { const int rc = row_width_check("layernorm", N); if (rc) return rc; }
    PSG_REQUIRE(rows > 0 && rows <= (int64_t)LN_ROWS * 0x7FFFFFFF, PSG_ERR_SHAPE, "layernorm: rows=%ld", (long)rows);
    PSG_REQUIRE(eps >= 0.f, PSG_ERR_ARG, "layernorm: eps %g", (double)eps);
    PSG_REQUIRE(ldx >= N && ldy >= N && (!r || ldr >= N), PSG_ERR_SHAPE, "layernorm: row stride < N");
    PSG_REQUIRE(((ldx | ldy | (r ? ldr : 0)) & 7) == 0 && aligned16(x) && aligned16(y) && (!r || aligned16(r)) && aligned16(gamma) &&
                aligned16(beta), PSG_ERR_ALIGN, "layernorm: rows must start on 16-byte boundaries (strides multiples of 8)");
    const int cpl = (N / 8 + 63) / 64;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + LN_ROWS - 1) / LN_ROWS)), block(64 * LN_ROWS);
    with_dtype(x_dtype, [&](auto ti) { with_dtype(y_dtype, [&](auto to) {
    with_const(LnCpls{}, cpl, [&](auto c) { with_const(Bools{}, r != nullptr, [&](auto res) {
        using TI = decltype(ti); using TO = decltype(to);
        hipLaunchKernelGGL((layernorm_kernel<TI, TO, decltype(c)::value, decltype(res)::value>), grid, block, 0, s, (const TI*)x, ldx,
                           (const TI*)r, r ? ldr : (int64_t)0, (TO*)y, ldy, gamma, beta, rows, N, eps);
    }); }); }); });
    PSG_LAUNCH_CHECK("layernorm");
    return PSG_OK;
}

int64_t psg_layernorm_bwd_workspace_bytes(int64_t rows, int N) {
    if (rows <= 0 || N <= 0) return 0;
    return 2 * ((rows + LNB_WG_ROWS - 1) / LNB_WG_ROWS) * (int64_t)N * (int64_t)sizeof(float);
}

int psg_layernorm_bwd(const void* x, int64_t ldx, const void* r, int64_t ldr, const void* dy, int64_t lddy, const float* gamma,
                      void* dz, int64_t lddz, float* dgamma, float* dbeta, int accumulate, int64_t rows, int N, float eps,
                      int x_dtype, int dy_dtype, void* ws, int64_t ws_bytes, psg_stream_t stream) {
    PSG_REQUIRE(x && dy && gamma && dz, PSG_ERR_ARG, "layernorm_bwd: null pointer");
    PSG_REQUIRE((x_dtype == PSG_F32 || x_dtype == PSG_BF16) && (dy_dtype == PSG_F32 || dy_dtype == PSG_BF16), PSG_ERR_DTYPE,
                "layernorm_bwd: dtypes x %d, dy %d", x_dtype, dy_dtype);
    { const int rc = row_width_check("layernorm_bwd", N); if (rc) return rc; }
    PSG_REQUIRE(rows > 0 && rows <= (int64_t)LNB_WG_ROWS * 0x7FFFFFFF, PSG_ERR_SHAPE, "layernorm_bwd: rows=%ld", (long)rows);
    PSG_REQUIRE(eps >= 0.f, PSG_ERR_ARG, "layernorm_bwd: eps %g", (double)eps);
    PSG_REQUIRE(ldx >= N && lddy >= N && lddz >= N && (!r || ldr >= N), PSG_ERR_SHAPE, "layernorm_bwd: row stride < N");
    PSG_REQUIRE(((ldx | lddy | lddz | (r ? ldr : 0)) & 7) == 0 && aligned16(x) && aligned16(dy) && aligned16(dz) && (!r || aligned16(r)) &&
                aligned16(gamma), PSG_ERR_ALIGN, "layernorm_bwd: rows must start on 16-byte boundaries (strides multiples of 8)");
    const bool pg = dgamma || dbeta;
    PSG_REQUIRE(!pg || ws, PSG_ERR_ARG, "layernorm_bwd: dgamma / dbeta need a workspace");
    PSG_REQUIRE(!pg || aligned16(ws), PSG_ERR_ALIGN, "layernorm_bwd: workspace must start on a 16-byte boundary");
    PSG_REQUIRE(!pg || ws_bytes >= psg_layernorm_bwd_workspace_bytes(rows, N), PSG_ERR_WORKSPACE, "layernorm_bwd: workspace of %ld bytes, need %ld",
                (long)ws_bytes, (long)psg_layernorm_bwd_workspace_bytes(rows, N));
    const int cpl = (N / 8 + 63) / 64;
    const int nwg = (int)((rows + LNB_WG_ROWS - 1) / LNB_WG_ROWS);
    hipStream_t s = (hipStream_t)stream;
    with_dtype(x_dtype, [&](auto ti) { with_dtype(dy_dtype, [&](auto tdy) {
    with_const(LnCpls{}, cpl, [&](auto c) { with_const(Bools{}, pg, [&](auto p) {
        using TI = decltype(ti); using TDY = decltype(tdy);
        hipLaunchKernelGGL((layernorm_bwd_kernel<TI, TDY, decltype(c)::value, decltype(p)::value>), dim3((unsigned)nwg), dim3(64 * LN_ROWS), 0, s,
                           (const TI*)x, ldx, (const TI*)r, r ? ldr : (int64_t)0, (const TDY*)dy, lddy, gamma, (TI*)dz, lddz, (float*)ws, rows, N, eps);
    }); }); }); });
    PSG_LAUNCH_CHECK("layernorm_bwd");
    if (pg) {
        hipLaunchKernelGGL(ln_param_sum_kernel, dim3((unsigned)((N + 63) / 64), 2), dim3(256), 0, s, (const float*)ws, nwg, N, dgamma, dbeta, accumulate);
        PSG_LAUNCH_CHECK("layernorm_bwd_param_sum");
    }
    return PSG_OK;
}

int psg_bert_embed_ln(const int64_t* ids, const int64_t* type_ids, const float* word_emb, const float* pos_emb,
                      const float* type_emb, const float* gamma, const float* beta, void* y, int64_t ldy, int B, int S, int N,
                      int vocab, int max_pos, int type_vocab, float eps, int dtype, psg_stream_t stream) {
    PSG_REQUIRE(ids && word_emb && pos_emb && type_emb && gamma && beta && y, PSG_ERR_ARG, "bert_embed_ln: null pointer");
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "bert_embed_ln: dtype %d", dtype);
    { const int rc = row_width_check("bert_embed_ln", N); if (rc) return rc; }
    PSG_REQUIRE(B > 0 && S > 0 && vocab > 0 && type_vocab > 0 && max_pos > 0, PSG_ERR_SHAPE, "bert_embed_ln: non-positive dimension");
    PSG_REQUIRE(S <= max_pos, PSG_ERR_SHAPE, "bert_embed_ln: S=%d exceeds the %d position embeddings", S, max_pos);
    PSG_REQUIRE(eps >= 0.f, PSG_ERR_ARG, "bert_embed_ln: eps %g", (double)eps);
    PSG_REQUIRE(ldy >= N, PSG_ERR_SHAPE, "bert_embed_ln: row stride < N");
    PSG_REQUIRE((ldy & 7) == 0 && aligned16(y) && aligned16(word_emb) && aligned16(pos_emb) && aligned16(type_emb) && aligned16(gamma) &&
                aligned16(beta), PSG_ERR_ALIGN, "bert_embed_ln: tables and rows must start on 16-byte boundaries");
    const int cpl = (N / 8 + 63) / 64;
    const int64_t rows = (int64_t)B * S;
    hipStream_t s = (hipStream_t)stream;
    with_dtype(dtype, [&](auto to) { with_const(LnCpls{}, cpl, [&](auto c) {
        using TO = decltype(to);
        hipLaunchKernelGGL((embed_ln_kernel<TO, decltype(c)::value>), dim3((unsigned)((rows + LN_ROWS - 1) / LN_ROWS)), dim3(64 * LN_ROWS), 0, s, ids,
                           type_ids, word_emb, pos_emb, type_emb, gamma, beta, (TO*)y, ldy, rows, S, N, vocab, type_vocab, eps);
    }); });
    PSG_LAUNCH_CHECK("bert_embed_ln");
    return PSG_OK;
}

int64_t psg_bert_embed_ln_bwd_workspace_bytes(int64_t rows, int N) { return psg_layernorm_bwd_workspace_bytes(rows, N); }

int psg_bert_embed_ln_bwd(const int64_t* ids, const int64_t* type_ids, const float* word_emb, const float* pos_emb,
                          const float* type_emb, const float* gamma, const void* dy, int64_t lddy, float* dz, float* dgamma,
                          float* dbeta, int accumulate, int B, int S, int N, int vocab, int max_pos, int type_vocab, float eps,
                          int dy_dtype, void* ws, int64_t ws_bytes, psg_stream_t stream) {
    PSG_REQUIRE(ids && word_emb && pos_emb && type_emb && gamma && dy && dz, PSG_ERR_ARG, "bert_embed_ln_bwd: null pointer");
    PSG_REQUIRE(dy_dtype == PSG_F32 || dy_dtype == PSG_BF16, PSG_ERR_DTYPE, "bert_embed_ln_bwd: dtype %d", dy_dtype);
    { const int rc = row_width_check("bert_embed_ln_bwd", N); if (rc) return rc; }
    PSG_REQUIRE(B > 0 && S > 0 && vocab > 0 && type_vocab > 0 && max_pos > 0, PSG_ERR_SHAPE, "bert_embed_ln_bwd: non-positive dimension");
    PSG_REQUIRE(S <= max_pos, PSG_ERR_SHAPE, "bert_embed_ln_bwd: S=%d exceeds the %d position embeddings", S, max_pos);
    PSG_REQUIRE(eps >= 0.f, PSG_ERR_ARG, "bert_embed_ln_bwd: eps %g", (double)eps);
    PSG_REQUIRE(lddy >= N, PSG_ERR_SHAPE, "bert_embed_ln_bwd: row stride < N");
    PSG_REQUIRE((lddy & 7) == 0 && aligned16(dy) && aligned16(dz) && aligned16(word_emb) && aligned16(pos_emb) && aligned16(type_emb) &&
                aligned16(gamma), PSG_ERR_ALIGN, "bert_embed_ln_bwd: tables and rows must start on 16-byte boundaries");
    const int64_t rows = (int64_t)B * S;
    const bool pg = dgamma || dbeta;
    PSG_REQUIRE(!pg || ws, PSG_ERR_ARG, "bert_embed_ln_bwd: dgamma / dbeta need a workspace");
    PSG_REQUIRE(!pg || aligned16(ws), PSG_ERR_ALIGN, "bert_embed_ln_bwd: workspace must start on a 16-byte boundary");
    PSG_REQUIRE(!pg || ws_bytes >= psg_bert_embed_ln_bwd_workspace_bytes(rows, N), PSG_ERR_WORKSPACE,
                "bert_embed_ln_bwd: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)psg_bert_embed_ln_bwd_workspace_bytes(rows, N));
    const int cpl = (N / 8 + 63) / 64;
    const int nwg = (int)((rows + LNB_WG_ROWS - 1) / LNB_WG_ROWS);
    hipStream_t s = (hipStream_t)stream;
    with_dtype(dy_dtype, [&](auto tdy) { with_const(LnCpls{}, cpl, [&](auto c) { with_const(Bools{}, pg, [&](auto p) {
        using TDY = decltype(tdy);
        hipLaunchKernelGGL((embed_ln_bwd_kernel<TDY, decltype(c)::value, decltype(p)::value>), dim3((unsigned)nwg), dim3(64 * LN_ROWS), 0, s, ids,
                           type_ids, word_emb, pos_emb, type_emb, gamma, (const TDY*)dy, lddy, dz, (float*)ws, rows, S, N, vocab, type_vocab, eps);
    }); }); });
    PSG_LAUNCH_CHECK("bert_embed_ln_bwd");
    if (pg) {
        hipLaunchKernelGGL(ln_param_sum_kernel, dim3((unsigned)((N + 63) / 64), 2), dim3(256), 0, s, (const float*)ws, nwg, N, dgamma, dbeta, accumulate);
        PSG_LAUNCH_CHECK("bert_embed_ln_bwd_param_sum");
    }
    return PSG_OK;
}

int psg_embed_scatter_chunk_rows(void) { return ES_CHUNK; }

int64_t psg_embed_scatter_workspace_bytes(int64_t rows, int N) {
    if (rows <= 0 || N <= 0) return 0;
    return rows * (int64_t)N * (int64_t)sizeof(float);
}

int psg_embed_scatter(const float* dz, int64_t lddz, const int64_t* key, const int64_t* perm, float* table_grad, int64_t rows,
                      int N, int64_t V, int64_t skip_key, int accumulate, void* ws, int64_t ws_bytes, psg_stream_t stream) {
    PSG_REQUIRE(dz && key && perm && table_grad && ws, PSG_ERR_ARG, "embed_scatter: null pointer");
    { const int rc = row_width_check("embed_scatter", N); if (rc) return rc; }
    PSG_REQUIRE(rows > 0 && rows <= (int64_t)0x7FFFFFFF && V > 0 && V <= (int64_t)0x7FFFFFFF, PSG_ERR_SHAPE,
                "embed_scatter: rows=%ld, V=%ld", (long)rows, (long)V);
    PSG_REQUIRE(lddz >= N, PSG_ERR_SHAPE, "embed_scatter: row stride < N");
    PSG_REQUIRE((lddz & 3) == 0 && aligned16(dz) && aligned16(table_grad) && aligned16(ws), PSG_ERR_ALIGN,
                "embed_scatter: rows, table and workspace must start on 16-byte boundaries");
    PSG_REQUIRE(ws_bytes >= psg_embed_scatter_workspace_bytes(rows, N), PSG_ERR_WORKSPACE, "embed_scatter: workspace of %ld bytes, need %ld",
                (long)ws_bytes, (long)psg_embed_scatter_workspace_bytes(rows, N));
    hipStream_t s = (hipStream_t)stream;
    const unsigned slabs = (unsigned)((N + ES_COLS - 1) / ES_COLS);
    if (!accumulate) {
        const int64_t n4 = V * (int64_t)N / 4;
        const int64_t wgs = (n4 + 255) / 256;
        hipLaunchKernelGGL(zero_f32x4_kernel, dim3((unsigned)(wgs < 4096 ? wgs : 4096)), dim3(256), 0, s, table_grad, n4);
        PSG_LAUNCH_CHECK("embed_scatter_zero");
    }
    hipLaunchKernelGGL(embed_scatter_chunk_kernel, dim3((unsigned)((rows + ES_CHUNK - 1) / ES_CHUNK), slabs), dim3(64), 0, s, dz, lddz, key, perm,
                       (float*)ws, rows, N, V, skip_key);
    PSG_LAUNCH_CHECK("embed_scatter_chunk");
    hipLaunchKernelGGL(embed_scatter_sum_kernel, dim3((unsigned)((rows + 3) / 4), slabs), dim3(256), 0, s, (const float*)ws, key, table_grad, rows, N,
                       V, skip_key, accumulate);
    PSG_LAUNCH_CHECK("embed_scatter_sum");
    return PSG_OK;
}

}  // extern "C"
