// Weight gradient of the VAE decoder's high-resolution convolutions (src/models/vae_decoder.py:163-175: blocks 4 and 5 at
// 108 x 108 / 215 x 215 with 64 / 32 channels, and the 32 -> 3 image convolution) for stage 1 (src/training/vae_trainer.py):
// few output channels (Cout <= 64), few input channels (Cin <= 128), very many pixels.  bf16 operands, fp32 accumulation.
//
//   dW[co][tap][ci] = sum_m dY[m][co] * X[pix(m) + tap][ci]           3x3 pad 1 or 1x1, stride 1, same-size output
//
// One 256-thread workgroup owns ALL Cout rows, one 32-channel chunk of Cin with all its taps (the column block), and a slab of
// 8 x 16-pixel image tiles.  Per tile it stages dY [128 px][Cout] and the input tile WITH ITS HALO [10 x 18 px][32 ch] in LDS
// exactly as they lie in memory (zeros outside the image), so the nine taps read one image of the input and dY is read once
// per column block; the next tile's global loads are in flight while the current one is multiplied.  The 16x16x32 bf16 MFMA
// wants 8 consecutive reduction indices (pixels) per lane: both operands get them from the transposing LDS read
// ds_read_b64_tr_b16 (4 pixel rows x 16 channels per 16-lane group), dY^T needs no transpose pass.  Rows beyond Cout are only
// the padding to the next multiple of 16.  The four waves split the column tiles (tap, 16 channels).  Each workgroup writes
// its fp32 partial [Cout][Q] (and the column sums of dY: the bias gradient, one extra MFMA against a ones operand) to the
// workspace; a second kernel adds the slabs in a fixed order and scatters into the master layout: no atomics, bitwise
// reproducible.
#include "psg_common.h"

namespace psg {
namespace {

constexpr int TH = 8, TW = 16, TPIX = TH * TW;          // output tile: 128 pixels = 4 K steps of 32
constexpr int CW = 32;                                  // input channels per column block
constexpr int XROWB = CW * 2 + 16;                      // LDS bytes per staged input pixel (16 bytes of padding)
constexpr int FIN_PARTS = 8, FIN_OUT = 32;              // finish kernel: 8 interleaved partial sums of 32 outputs per block

struct SlimP {
    const char* x; const char* dy; float* slab; float* bslab;
    int64_t ldxB, lddyB;                                // row strides in bytes
    int B, H, W, Cin, Cout, Q;
    int tiles_h, tiles_w, ntiles, tiles_per_slab;
};

typedef __attribute__((ext_vector_type(8))) short s16x8_t;
__device__ __forceinline__ s16x4 tr_read(const char* a) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a)); }
__device__ __forceinline__ bf16x8 tr_frag(const char* lo, const char* hi) {
    const s16x4 a = tr_read(lo), c = tr_read(hi);
    s16x8_t v = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
    return *reinterpret_cast<bf16x8*>(&v);
}

// KS: 1 or 3.  NR: 16-row tiles of Cout (1, 2, 4).
template <int KS, int NR>
__global__ __launch_bounds__(256) void wgrad_slim_kernel(const SlimP p) {
    constexpr int HALO = KS / 2, XH = TH + 2 * HALO, XW = TW + 2 * HALO, XPIX = XH * XW;
    constexpr int NC = KS * KS * (CW / 16);             // column tiles of 16: (tap, half of the channel chunk)
    constexpr int NCW = (NC + 3) / 4;                   // ... per wave
    constexpr int YCH = 2 * NR;                         // 16-byte chunks per staged dY pixel
    constexpr int YROWB = NR * 32 + 16;
    constexpr int YN = TPIX * YCH / 256;                // 16-byte loads per thread and tile: dY
    constexpr int XN = (XPIX * 4 + 255) / 256;          // ... input
    __shared__ __attribute__((aligned(16))) char xlds[XPIX * XROWB];
    __shared__ __attribute__((aligned(16))) char ylds[TPIX * YROWB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, sl = blockIdx.y;
    const int c0 = chunk * CW;
    const int t0 = sl * p.tiles_per_slab;
    const int t1 = min(t0 + p.tiles_per_slab, p.ntiles);
    const int tiles_img = p.tiles_h * p.tiles_w;

    u32x4 ry[YN], rx[XN];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto load_tile = [&](int t) {
        const int b = t / tiles_img, r = t - b * tiles_img;
        const int h0 = (r / p.tiles_w) * TH, w0 = (r % p.tiles_w) * TW;
#pragma unroll
        for (int i = 0; i < YN; ++i) {
            const int e = tid + i * 256;
            const int pix = e / YCH, ch = e - pix * YCH;
            const int h = h0 + (pix >> 4), w = w0 + (pix & 15);
            const bool ok = h < p.H && w < p.W && ch * 8 < p.Cout;
            const int64_t off = ((int64_t)(b * p.H + h) * p.W + w) * p.lddyB + ch * 16;
            ry[i] = ok ? *reinterpret_cast<const u32x4*>(p.dy + off) : zero4;
        }
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = tid + i * 256;
            const int pix = e >> 2, ch = e & 3;
            const int h = h0 + pix / XW - HALO, w = w0 + pix % XW - HALO;
            const bool ok = e < XPIX * 4 && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W && c0 + ch * 8 < p.Cin;
            const int64_t off = ((int64_t)(b * p.H + h) * p.W + w) * p.ldxB + (c0 + ch * 8) * 2;
            rx[i] = ok ? *reinterpret_cast<const u32x4*>(p.x + off) : zero4;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < YN; ++i) {
            const int e = tid + i * 256;
            const int pix = e / YCH, ch = e - pix * YCH;
            *reinterpret_cast<u32x4*>(ylds + pix * YROWB + ch * 16) = ry[i];
        }
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = tid + i * 256;
            if (e < XPIX * 4) *reinterpret_cast<u32x4*>(xlds + (e >> 2) * XROWB + (e & 3) * 16) = rx[i];
        }
    };

    f32x4 acc[NR][NCW], accb[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NCW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.bslab != nullptr && chunk == 0 && wave == 0;       // wave-uniform
    const bf16_t one = (bf16_t)1.0f;
    const bf16x8 ones = {one, one, one, one, one, one, one, one};

    // transposed fragment reads: lane -> (16-lane group g, row q4 of the 4 x 16 block, 4-column piece p4); group g of K step s
    // covers the 8 pixels (tile row 2 s + (g >> 1), columns 8 (g & 1) .. + 7), element e <-> pixel + e
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
    const int trow = g >> 1, tcol = 8 * (g & 1);

    load_tile(t0);                                      // every slab has at least one tile
    for (int t = t0; t < t1; ++t) {
        store_tile();
        __syncthreads();
        if (t + 1 < t1) load_tile(t + 1);               // in flight during the products below
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int pr = 2 * s + trow;
            bf16x8 af[NR];
            const char* ya = ylds + (pr * TW + tcol + q4) * YROWB + p4 * 8;
#pragma unroll
            for (int i = 0; i < NR; ++i) af[i] = tr_frag(ya + i * 32, ya + 4 * YROWB + i * 32);
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < NR; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, accb[i], 0, 0, 0);
            }
#pragma unroll
            for (int jj = 0; jj < NCW; ++jj) {
                const int j = wave + 4 * jj;            // wave-uniform
                if (j < NC) {
                    const int tap = j / (CW / 16), half = j % (CW / 16);
                    const int kh = tap / KS, kw = tap % KS;
                    const char* xb = xlds + ((pr + kh) * XW + tcol + kw + q4) * XROWB + half * 32 + p4 * 8;
                    const bf16x8 bf = tr_frag(xb, xb + 4 * XROWB);
#pragma unroll
                    for (int i = 0; i < NR; ++i) acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf, acc[i][jj], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                // the tile has been read: the next one may overwrite it
    }

    // C/D: column = lane & 15, row = 4 (lane >> 4) + r
    float* out = p.slab + (int64_t)sl * p.Cout * p.Q;
#pragma unroll
    for (int jj = 0; jj < NCW; ++jj) {
        const int j = wave + 4 * jj;
        if (j >= NC) continue;
        const int tap = j / (CW / 16), ci = c0 + (j % (CW / 16)) * 16 + i16;
        if (ci >= p.Cin) continue;
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = i * 16 + 4 * g + r;
                if (co < p.Cout) out[(int64_t)co * p.Q + tap * p.Cin + ci] = acc[i][jj][r];
            }
    }
    if (do_bias && i16 == 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = i * 16 + 4 * g + r;
                if (co < p.Cout) p.bslab[(int64_t)sl * p.Cout + co] = accb[i][r];
            }
    }
}

// slabs -> dw (and dbias).  A block sums FIN_OUT outputs: FIN_PARTS interleaved partial sums (slabs part, part + 8, ...) each in
// slab order, then the partials in part order - a fixed tree, the same bits every run.
__global__ __launch_bounds__(FIN_PARTS * FIN_OUT) void wgrad_slim_finish_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                                                               float* __restrict__ dw, float* __restrict__ dbias, int Cout,
                                                                               int Cin, int taps, int ohwi, int slabs, float scale,
                                                                               int accumulate, int accumulate_bias) {
    __shared__ float red[FIN_PARTS][FIN_OUT];
    const int Q = taps * Cin, nw = Cout * Q;
    const int o = threadIdx.x % FIN_OUT, part = threadIdx.x / FIN_OUT;
    const int idx = blockIdx.x * FIN_OUT + o;            // [co][q] of the slabs, then the Cout bias sums
    float v = 0.f;
    if (idx < nw) {
        for (int s = part; s < slabs; s += FIN_PARTS) v += slab[(int64_t)s * nw + idx];
    } else if (bslab && idx < nw + Cout) {
        for (int s = part; s < slabs; s += FIN_PARTS) v += bslab[(int64_t)s * Cout + (idx - nw)];
    }
    red[part][o] = v;
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int k = 1; k < FIN_PARTS; ++k) v += red[k][o];
    v *= scale;
    if (idx < nw) {
        int dst = idx;                                   // OHWI is the slab's own order
        if (!ohwi) {
            const int co = idx / Q, q = idx - co * Q, tap = q / Cin, ci = q - tap * Cin;
            dst = (co * Cin + ci) * taps + tap;
        }
        dw[dst] = accumulate ? dw[dst] + v : v;
    } else if (bslab && idx < nw + Cout) {
        dbias[idx - nw] = accumulate_bias ? dbias[idx - nw] + v : v;
    }
}

int g_slim_split_pin = 0;

struct SlimPlan { int tiles_h, tiles_w, ntiles, tiles_per_slab, slabs; };
// The slab count follows the pixel count and the CUs: two workgroup rows per CU (not capped: a slab is at least one tile); a
// pin is taken as asked, up to one tile per slab.
SlimPlan slim_plan(const psg_wgrad_desc* d) {
    SlimPlan s;
    s.tiles_h = (d->Hi + TH - 1) / TH;
    s.tiles_w = (d->Wi + TW - 1) / TW;
    s.ntiles = d->B * s.tiles_h * s.tiles_w;
    int64_t want = g_slim_split_pin > 0 ? g_slim_split_pin : 2 * (int64_t)avail_cus();
    if (want > s.ntiles) want = s.ntiles;
    if (want < 1) want = 1;
    s.tiles_per_slab = (int)((s.ntiles + want - 1) / want);
    s.slabs = (s.ntiles + s.tiles_per_slab - 1) / s.tiles_per_slab;
    return s;
}

// everything of the contract that needs no pointer
int slim_check_shape(const char* what, const psg_wgrad_desc* d) {
    PSG_REQUIRE(d, PSG_ERR_ARG, "%s: null descriptor", what);
    PSG_REQUIRE(d->dtype == PSG_BF16, PSG_ERR_DTYPE, "%s: dtype %d (bf16 only; fp32 goes to psg_conv_wgrad)", what, d->dtype);
    PSG_REQUIRE(d->B > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0 && d->Cout > 0, PSG_ERR_SHAPE, "%s: non-positive dimension", what);
    PSG_REQUIRE((d->ksize == 1 && d->pad == 0) || (d->ksize == 3 && d->pad == 1), PSG_ERR_SHAPE, "%s: ksize %d pad %d", what, d->ksize, d->pad);
    PSG_REQUIRE(d->stride == 1 && d->Ho == d->Hi && d->Wo == d->Wi, PSG_ERR_SHAPE, "%s: stride %d, output %dx%d of input %dx%d (stride 1, same size only)",
                what, d->stride, d->Ho, d->Wo, d->Hi, d->Wi);
    PSG_REQUIRE(d->Cout == 8 || d->Cout == 16 || d->Cout == 32 || d->Cout == 64, PSG_ERR_SHAPE, "%s: Cout=%d is not 8, 16, 32 or 64", what, d->Cout);
    PSG_REQUIRE(d->Cin % 8 == 0 && d->Cin <= 128, PSG_ERR_SHAPE, "%s: Cin=%d must be a multiple of 8, at most 128", what, d->Cin);
    PSG_REQUIRE(d->ldx >= d->Cin && d->ldx % 8 == 0 && d->lddy >= d->Cout && d->lddy % 8 == 0, PSG_ERR_SHAPE, "%s: row strides ldx=%ld lddy=%ld", what,
                (long)d->ldx, (long)d->lddy);
    PSG_REQUIRE((int64_t)d->B * (d->Hi + TH) * (d->Wi + TW) < (1ll << 31), PSG_ERR_SHAPE, "%s: too many pixels", what);
    PSG_REQUIRE(d->dw_layout == PSG_W_OIHW || d->dw_layout == PSG_W_OHWI, PSG_ERR_ARG, "%s: dw_layout %d", what, d->dw_layout);
    return PSG_OK;
}

int64_t slim_ws_bytes(const psg_wgrad_desc* d, const SlimPlan& s) {
    const int64_t Q = (int64_t)d->ksize * d->ksize * d->Cin;
    return (int64_t)s.slabs * ((int64_t)d->Cout * Q + d->Cout) * (int64_t)sizeof(float);
}

template <int KS, int NR>
void slim_launch(const SlimP& p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((wgrad_slim_kernel<KS, NR>), grid, dim3(256), 0, stream, p);
}

}  // namespace
}  // namespace psg

using namespace psg;

extern "C" {

int psg_conv_wgrad_slim_set_splits(int n) {
    g_slim_split_pin = n > 0 ? n : 0;
    return PSG_OK;
}

int64_t psg_conv_wgrad_slim_workspace_bytes(const psg_wgrad_desc* d) {
    if (slim_check_shape("conv_wgrad_slim_workspace_bytes", d) != PSG_OK) return -1;
    return slim_ws_bytes(d, slim_plan(d));
}

int psg_conv_wgrad_slim(const psg_wgrad_desc* d, psg_stream_t stream) {
    const int rc = slim_check_shape("conv_wgrad_slim", d);
    if (rc != PSG_OK) return rc;
    PSG_REQUIRE(d->x && d->dy && d->dw, PSG_ERR_ARG, "conv_wgrad_slim: null pointer");
    PSG_REQUIRE(aligned16(d->x) && aligned16(d->dy), PSG_ERR_ALIGN, "conv_wgrad_slim: x and dy must be 16-byte aligned");
    const SlimPlan s = slim_plan(d);
    const int64_t need = slim_ws_bytes(d, s);
    PSG_REQUIRE(d->ws && d->ws_bytes >= need, PSG_ERR_WORKSPACE, "conv_wgrad_slim: workspace of %ld bytes, %ld needed", (long)(d->ws ? d->ws_bytes : 0),
                (long)need);
    PSG_REQUIRE(aligned16(d->ws), PSG_ERR_ALIGN, "conv_wgrad_slim: workspace must be 16-byte aligned");
    const int taps = d->ksize * d->ksize;
    SlimP p;
    p.x = (const char*)d->x; p.dy = (const char*)d->dy;
    p.slab = (float*)d->ws;
    p.bslab = d->dbias ? p.slab + (int64_t)s.slabs * d->Cout * taps * d->Cin : nullptr;
    p.ldxB = d->ldx * 2; p.lddyB = d->lddy * 2;
    p.B = d->B; p.H = d->Hi; p.W = d->Wi; p.Cin = d->Cin; p.Cout = d->Cout; p.Q = taps * d->Cin;
    p.tiles_h = s.tiles_h; p.tiles_w = s.tiles_w; p.ntiles = s.ntiles; p.tiles_per_slab = s.tiles_per_slab;
    const dim3 grid((d->Cin + CW - 1) / CW, s.slabs);
    const hipStream_t st = (hipStream_t)stream;
    const int nr = d->Cout <= 16 ? 1 : d->Cout / 16;
    {
        ProfScope prof(PROF_WGRAD, 2.0 * d->B * d->Hi * d->Wi * (double)d->Cout * p.Q, st);
        if (d->ksize == 3) {
            if (nr == 1) slim_launch<3, 1>(p, grid, st); else if (nr == 2) slim_launch<3, 2>(p, grid, st); else slim_launch<3, 4>(p, grid, st);
        } else {
            if (nr == 1) slim_launch<1, 1>(p, grid, st); else if (nr == 2) slim_launch<1, 2>(p, grid, st); else slim_launch<1, 4>(p, grid, st);
        }
        PSG_LAUNCH_CHECK("conv_wgrad_slim");
        const int n = d->Cout * p.Q + (d->dbias ? d->Cout : 0);
        hipLaunchKernelGGL(wgrad_slim_finish_kernel, dim3((n + FIN_OUT - 1) / FIN_OUT), dim3(FIN_PARTS * FIN_OUT), 0, st, p.slab, p.bslab, d->dw, d->dbias,
                           d->Cout, d->Cin, taps, d->dw_layout == PSG_W_OHWI ? 1 : 0, s.slabs, d->scale == 0.f ? 1.f : d->scale, d->accumulate,
                           d->accumulate_bias);
        PSG_LAUNCH_CHECK("conv_wgrad_slim_finish");
    }
    return PSG_OK;
}

}  // extern "C"
