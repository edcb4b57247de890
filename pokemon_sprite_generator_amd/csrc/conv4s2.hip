// Gradients of nn.Conv2d(k=4, s=2, p in {1,2}) - the VAE encoder's three downsampling convolutions
// (reference src/models/vae_decoder.py:78-89).  Channels-last operands with row strides, fp32 accumulation.
//
// Data gradient.  An input pixel (h, w) is read by the taps kh = (h + pad) & 1 (+ 2), kw = (w + pad) & 1 (+ 2) and by no
// other: per parity class ((h+pad)&1, (w+pad)&1) the data gradient is a dense GEMM of K = 4 * Cout over a fixed quarter of
// the weight.  One wave owns 16 pixels of one class; both MFMA operands are 16-byte chunks read straight from global
// memory (a chunk of 8 bf16 / 4 fp32 output channels lies inside one tap because Cout % 8 == 0), so there is no LDS and
// no barrier.  bf16: v_mfma_f32_16x16x32_bf16.  fp32: v_mfma_f32_16x16x4_f32 on fp32 operands - element i of every lane's
// chunk is one instruction's k slice, a permutation of k that both operands share.
//
// Weight gradient.  dw is tiny (Cout x 16 Cin) and the reduction over M = B Ho Wo is long: M is split into slabs, every
// workgroup writes its fp32 partial tile into the workspace and a second kernel adds the slabs in a fixed order, scatters
// into the master's layout (OIHW / OHWI, the first cin_real input channels), and adds into dw / dbias when asked.  No
// atomics anywhere.  The products run on v_mfma_f32_16x16x4_f32 for both dtypes (bf16 operands convert exactly): its A and
// B fragments are ONE element per lane with 16 lanes along the contiguous channel axis, so dY^T needs no transpose and
// the gather of x - for one output pixel and one kh a contiguous run of 4 Cin elements - needs no staging.
#include "psg_common.h"

using namespace psg;

namespace {

template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
    typedef bf16x8 chunk;
    static __device__ __forceinline__ f32x4 mma(chunk a, chunk b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Frag<float> {
    typedef f32x4 chunk;
    static __device__ __forceinline__ f32x4 mma(chunk a, chunk b, f32x4 c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], c, 0, 0, 0);
        return c;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// data gradient: grid (pixel tiles of the largest class, 4 classes), 4 waves x 16 pixels per workgroup
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv4s2_dgrad_kernel(const T* __restrict__ g, int64_t ldg, const T* __restrict__ wd, int64_t ldw,
                                                            T* __restrict__ dx, int64_t lddx, int B, int Hi, int Wi, int Cin, int Ho,
                                                            int Wo, int Cout, int pad) {
    typedef typename Frag<T>::chunk chunk;
    constexpr int CH = Elem<T>::CH;
    const int ph = blockIdx.y >> 1, pw = blockIdx.y & 1;
    const int h0 = (ph + pad) & 1, w0 = (pw + pad) & 1;               // first row / column of the class
    const int nh = (Hi - h0 + 1) >> 1, nw = (Wi - w0 + 1) >> 1;       // rows / columns of the class (may be 0)
    const int npix = B * nh * nw;                                     // (B Hi Wi < 2^31 is checked on the host: 32-bit pixel decode)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    const int p0 = (blockIdx.x * 4 + wave) * 16;
    if (p0 >= npix) return;                                           // wave-uniform; the kernel has no barrier

    // the pixel of this lane's A row
    const int p = p0 + r;
    const bool pv = p < npix;
    int ab = 0, hb = 0, wb = 0;
    if (pv) {
        const int wi = (int)((unsigned)p % (unsigned)nw);
        const unsigned t = (unsigned)p / (unsigned)nw;
        const int hi = (int)(t % (unsigned)nh);
        ab = (int)(t / (unsigned)nh);
        hb = (h0 + 2 * hi + pad - ph) >> 1;                           // oh of tap kh = ph; tap kh = ph + 2 reads oh - 1
        wb = (w0 + 2 * wi + pad - pw) >> 1;
    }
    const int cpt = Cout / CH, nch = 4 * cpt;                         // chunks per tap, chunks of the class's K
    const int steps = (nch + 3) >> 2;

    for (int cib = 0; cib < Cin; cib += 64) {
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < steps; ++s) {
            const int c = 4 * s + q;
            const bool cv = c < nch;
            const int tap = cv ? c / cpt : 0;
            const int co = cv ? (c - tap * cpt) * CH : 0;
            const int th = tap >> 1, tw = tap & 1;
            const int oh = hb - th, ow = wb - tw;
            chunk a = {};
            if (cv && pv && oh >= 0 && oh < Ho && ow >= 0 && ow < Wo)
                a = *reinterpret_cast<const chunk*>(g + (((int64_t)ab * Ho + oh) * Wo + ow) * ldg + co);
            const int64_t koff = (int64_t)((ph + 2 * th) * 4 + pw + 2 * tw) * Cout + co;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (cib + n * 16 < Cin) {                             // wave-uniform
                    const int ci = cib + n * 16 + r;
                    chunk b = {};
                    if (cv && ci < Cin) b = *reinterpret_cast<const chunk*>(wd + (int64_t)ci * ldw + koff);
                    acc[n] = Frag<T>::mma(a, b, acc[n]);
                }
            }
        }
        // C/D: column (ci) = lane & 15, row (pixel) = 4 * (lane >> 4) + j
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int po = p0 + q * 4 + j;
            if (po < npix) {
                const int wi = (int)((unsigned)po % (unsigned)nw);
                const unsigned t = (unsigned)po / (unsigned)nw;
                const int hi = (int)(t % (unsigned)nh);
                const int ob = (int)(t / (unsigned)nh);
                T* row = dx + (((int64_t)ob * Hi + h0 + 2 * hi) * Wi + w0 + 2 * wi) * lddx;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int ci = cib + n * 16 + r;
                    if (ci < Cin) Elem<T>::st(row + ci, acc[n][j]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient: grid (K / 64, ceil(Cout / 32), splits); a workgroup owns a 32 (co) x 64 (k) tile of one M slab, its four
// waves take every fourth group of 4 rows and are added in wave order through LDS
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WG_CO = 32, WG_K = 64, WG_ROWS = 16;                     // tile; rows per step of the workgroup
constexpr int WG_UNROLL = 2;                                          // steps whose loads are issued together

template <typename T>
__global__ __launch_bounds__(256) void conv4s2_wgrad_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ g, int64_t ldg,
                                                            float* __restrict__ slab, float* __restrict__ bslab, int B, int Hi, int Wi,
                                                            int Cin, int Ho, int Wo, int Cout, int pad, int64_t M, int64_t rps) {
    __shared__ f32x4 red[4][8][64];
    __shared__ float bred[4][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    const int k0 = blockIdx.x * WG_K, co0 = blockIdx.y * WG_CO, sp = blockIdx.z;
    const int Kp = 16 * Cin;
    const int64_t r0 = (int64_t)sp * rps;
    const int64_t r1 = r0 + rps < M ? r0 + rps : M;

    // this lane's four k columns: k = (kh, kw, ci)
    int kh[4], kw[4];
    int64_t koff[4];                                                   // offset of the tap's element from the window's first pixel
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int k = k0 + n * 16 + r;
        kh[n] = k / (4 * Cin);
        const int rem = k - kh[n] * 4 * Cin;
        kw[n] = rem / Cin;
        koff[n] = ((int64_t)kh[n] * Wi + kw[n]) * ldx + (rem - kw[n] * Cin);
    }
    const int coA[2] = {co0 + r, co0 + 16 + r};

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs[2] = {0.f, 0.f};

    // WG_UNROLL row groups are loaded together, every load unconditional at a valid address (a row past the slab reads the
    // slab's last row, a tap outside the image reads the tensor's first element) and zeroed afterwards, so that the
    // 6 * WG_UNROLL loads of an iteration are in flight at once.  M < 2^31 (host check): 32-bit row decode.
    const bool cov[2] = {coA[0] < Cout, coA[1] < Cout};
    const int coC[2] = {cov[0] ? coA[0] : 0, cov[1] ? coA[1] : 0};
    const int rlast = (int)r1 - 1;                                      // r0 <= rlast: every slab has at least one row
    for (int base = (int)r0 + wave * 4; base < (int)r1; base += WG_ROWS * WG_UNROLL) {   // wave-uniform trip count
        float a[WG_UNROLL][2], b[WG_UNROLL][4];
#pragma unroll
        for (int u = 0; u < WG_UNROLL; ++u) {
            const int m = base + u * WG_ROWS + q;
            const bool mv = m <= rlast;
            const int mc = mv ? m : rlast;
            const unsigned t = (unsigned)mc / (unsigned)Wo;
            const int ow = mc - (int)t * Wo;
            const int nb = (int)(t / (unsigned)Ho);
            const int oh = (int)t - nb * Ho;
            const T* grow = g + (int64_t)mc * ldg;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float v = Elem<T>::ld(grow + coC[i]);
                a[u][i] = (mv && cov[i]) ? v : 0.f;
            }
            // the window's first pixel (2 oh - pad, 2 ow - pad), possibly outside the image: one 64-bit product per row, the
            // tap's own offset (koff, constant per lane) is added to it
            const int ih0 = 2 * oh - pad, iw0 = 2 * ow - pad;
            const int64_t rowoff = (int64_t)((nb * Hi + ih0) * Wi + iw0) * ldx;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const bool ok = mv && (unsigned)(ih0 + kh[n]) < (unsigned)Hi && (unsigned)(iw0 + kw[n]) < (unsigned)Wi;
                const float v = Elem<T>::ld(x + (ok ? rowoff + koff[n] : 0));
                b[u][n] = ok ? v : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < WG_UNROLL; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bs[i] += a[u][i];
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], b[u][n], acc[i][n], 0, 0, 0);
            }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        bred[wave][i][lane] = bs[i];
#pragma unroll
        for (int n = 0; n < 4; ++n) red[wave][i * 4 + n][lane] = acc[i][n];
    }
    __syncthreads();
    // C/D: column (k) = lane & 15, row (co) = 4 * (lane >> 4) + j
    for (int e = threadIdx.x; e < 8 * 64; e += 256) {
        const int t = e >> 6, l = e & 63;
        f32x4 v = red[0][t][l];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += red[w][t][l];
        const int col = k0 + (t & 3) * 16 + (l & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + (t >> 2) * 16 + (l >> 4) * 4 + j;
            if (co < Cout) slab[((int64_t)sp * Cout + co) * Kp + col] = v[j];
        }
    }
    if (bslab && blockIdx.x == 0 && threadIdx.x < 32) {
        const int i = threadIdx.x >> 4, c = threadIdx.x & 15;
        float v = 0.f;
        for (int w = 0; w < 4; ++w)
            for (int qq = 0; qq < 4; ++qq) v += bred[w][i][qq * 16 + c];
        const int co = co0 + i * 16 + c;
        if (co < Cout) bslab[(int64_t)sp * Cout + co] = v;
    }
}

// slabs -> dw (and dbias): one thread per output element, the slabs added in split order
__global__ void conv4s2_finish_kernel(const float* __restrict__ slab, const float* __restrict__ bslab, float* __restrict__ dw,
                                      float* __restrict__ dbias, int Cout, int Cin, int cin_real, int ohwi, int splits, int accumulate,
                                      int accumulate_bias) {
    const int nw = Cout * cin_real * 16;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int Kp = 16 * Cin;
    if (idx < nw) {
        int co, c, tap;
        if (ohwi) {
            c = idx % cin_real;
            const int t = idx / cin_real;
            tap = t & 15;
            co = t >> 4;
        } else {
            tap = idx & 15;
            const int t = idx >> 4;
            c = t % cin_real;
            co = t / cin_real;
        }
        const float* p = slab + (int64_t)co * Kp + tap * Cin + c;
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += p[(int64_t)s * Cout * Kp];
        dw[idx] = accumulate ? dw[idx] + v : v;
    } else if (dbias && idx < nw + Cout) {
        const int co = idx - nw;
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += bslab[(int64_t)s * Cout + co];
        dbias[co] = accumulate_bias ? dbias[co] + v : v;
    }
}

int g_split_pin = 0;

struct WPlan { int splits; int64_t rps; };
// The split plan: about four workgroups per CU, at least 64 rows per slab, at most 256 slabs; a pin is taken as asked
// (down to one 16-row step per slab).  Slabs are whole 16-row steps; the launch gets ceil(M / rows per slab) of them.
WPlan wgrad_plan(int64_t M, int Cin, int Cout) {
    const int64_t tiles = (int64_t)(16 * Cin / WG_K) * ((Cout + WG_CO - 1) / WG_CO);
    int64_t want;
    if (g_split_pin > 0) {
        want = g_split_pin;
    } else {
        want = 1024 / tiles;
        const int64_t maxs = (M + 63) / 64;
        if (want > maxs) want = maxs;
        if (want > 256) want = 256;
    }
    if (want < 1) want = 1;
    int64_t rps = (M + want - 1) / want;
    rps = (rps + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
    WPlan p;
    p.rps = rps;
    p.splits = (int)((M + rps - 1) / rps);
    return p;
}

int check_geom(const char* what, int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int pad, int dtype) {
    PSG_REQUIRE(dtype == PSG_F32 || dtype == PSG_BF16, PSG_ERR_DTYPE, "%s: dtype %d", what, dtype);
    PSG_REQUIRE(pad == 1 || pad == 2, PSG_ERR_ARG, "%s: pad %d (the 4x4 stride-2 convolutions have pad 1 or 2)", what, pad);
    PSG_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && Cin > 0 && Cout > 0, PSG_ERR_SHAPE,
                "%s: B=%d Hi=%d Wi=%d Cin=%d Ho=%d Wo=%d Cout=%d", what, B, Hi, Wi, Cin, Ho, Wo, Cout);
    PSG_REQUIRE(Hi + 2 * pad >= 4 && Wi + 2 * pad >= 4 && Ho == (Hi + 2 * pad - 4) / 2 + 1 && Wo == (Wi + 2 * pad - 4) / 2 + 1, PSG_ERR_SHAPE,
                "%s: output %dx%d is not (H+2p-4)/2+1 of input %dx%d with pad %d", what, Ho, Wo, Hi, Wi, pad);
    PSG_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, PSG_ERR_SHAPE, "%s: Cin=%d and Cout=%d must be multiples of 8", what, Cin, Cout);
    PSG_REQUIRE((int64_t)B * Hi * Wi < (1ll << 31) && (int64_t)Cout * Cin * 16 < (1ll << 28), PSG_ERR_SHAPE, "%s: problem too large", what);
    return PSG_OK;
}

int check_rows(const char* what, const char* name, const void* p, int64_t ld, int C, int dtype) {
    const int64_t esz = dtype == PSG_BF16 ? 2 : 4;
    PSG_REQUIRE(ld >= C, PSG_ERR_SHAPE, "%s: leading dimension of %s (%ld) is smaller than its %d channels", what, name, (long)ld, C);
    PSG_REQUIRE(aligned16(p) && (ld * esz) % 16 == 0, PSG_ERR_ALIGN, "%s: %s and its rows must be 16-byte aligned (ld=%ld)", what, name, (long)ld);
    return PSG_OK;
}

}  // namespace

extern "C" {

int psg_conv4s2_dgrad(const void* g, int64_t ldg, const void* wd, void* dx, int64_t lddx, int B, int Hi, int Wi, int Cin, int Ho, int Wo,
                      int Cout, int pad, int dtype, psg_stream_t stream) {
    PSG_REQUIRE(g && wd && dx, PSG_ERR_ARG, "conv4s2_dgrad: null pointer");
    int rc = check_geom("conv4s2_dgrad", B, Hi, Wi, Cin, Ho, Wo, Cout, pad, dtype);
    if (rc != PSG_OK) return rc;
    if ((rc = check_rows("conv4s2_dgrad", "g", g, ldg, Cout, dtype)) != PSG_OK) return rc;
    if ((rc = check_rows("conv4s2_dgrad", "dx", dx, lddx, Cin, dtype)) != PSG_OK) return rc;
    PSG_REQUIRE(aligned16(wd), PSG_ERR_ALIGN, "conv4s2_dgrad: wd must be 16-byte aligned");
    const int64_t ldw = psg_kpad((int64_t)16 * Cout, dtype);
    const int64_t maxpix = (int64_t)B * ((Hi + 1) / 2) * ((Wi + 1) / 2);
    const dim3 grid((unsigned)((maxpix + 63) / 64), 4);
    if (!with_dtype(dtype, [&](auto elem) {
            using T = decltype(elem);
            hipLaunchKernelGGL(conv4s2_dgrad_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)g, ldg, (const T*)wd, ldw, (T*)dx,
                               lddx, B, Hi, Wi, Cin, Ho, Wo, Cout, pad);
        }))
        return set_error(PSG_ERR_DTYPE, "conv4s2_dgrad: dtype %d", dtype);
    PSG_LAUNCH_CHECK("conv4s2_dgrad");
    return PSG_OK;
}

int psg_conv4s2_wgrad_set_splits(int n) {
    g_split_pin = n > 0 ? n : 0;
    return PSG_OK;
}

int64_t psg_conv4s2_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int dtype) {
    if (!(dtype == PSG_F32 || dtype == PSG_BF16)) { set_error(PSG_ERR_DTYPE, "conv4s2_wgrad_workspace_bytes: dtype %d", dtype); return -1; }
    if (!(B > 0 && Ho > 0 && Wo > 0 && Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0 && (int64_t)Cout * Cin * 16 < (1ll << 28))) {
        set_error(PSG_ERR_SHAPE, "conv4s2_wgrad_workspace_bytes: B=%d Ho=%d Wo=%d Cin=%d Cout=%d (channels must be multiples of 8)", B, Ho, Wo, Cin, Cout);
        return -1;
    }
    const WPlan p = wgrad_plan((int64_t)B * Ho * Wo, Cin, Cout);
    return (int64_t)p.splits * ((int64_t)Cout * 16 * Cin + Cout) * (int64_t)sizeof(float);
}

int psg_conv4s2_wgrad(const void* x, int64_t ldx, const void* g, int64_t ldg, float* dw, int dw_layout, int cin_real, float* dbias, int B,
                      int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int pad, int accumulate, int accumulate_bias, int dtype, void* ws,
                      int64_t ws_bytes, psg_stream_t stream) {
    PSG_REQUIRE(x && g && dw, PSG_ERR_ARG, "conv4s2_wgrad: null pointer");
    int rc = check_geom("conv4s2_wgrad", B, Hi, Wi, Cin, Ho, Wo, Cout, pad, dtype);
    if (rc != PSG_OK) return rc;
    PSG_REQUIRE(dw_layout == PSG_W_OIHW || dw_layout == PSG_W_OHWI, PSG_ERR_ARG, "conv4s2_wgrad: dw_layout %d", dw_layout);
    PSG_REQUIRE(cin_real >= 1 && cin_real <= Cin, PSG_ERR_ARG, "conv4s2_wgrad: cin_real %d is not in [1, Cin=%d]", cin_real, Cin);
    if ((rc = check_rows("conv4s2_wgrad", "x", x, ldx, Cin, dtype)) != PSG_OK) return rc;
    if ((rc = check_rows("conv4s2_wgrad", "g", g, ldg, Cout, dtype)) != PSG_OK) return rc;
    const int64_t M = (int64_t)B * Ho * Wo;
    const WPlan p = wgrad_plan(M, Cin, Cout);
    const int64_t slab_elems = (int64_t)p.splits * Cout * 16 * Cin;
    const int64_t need = (slab_elems + (int64_t)p.splits * Cout) * (int64_t)sizeof(float);
    PSG_REQUIRE(ws && ws_bytes >= need, PSG_ERR_WORKSPACE, "conv4s2_wgrad: workspace of %ld bytes, %ld needed", (long)(ws ? ws_bytes : 0), (long)need);
    PSG_REQUIRE(aligned16(ws), PSG_ERR_ALIGN, "conv4s2_wgrad: workspace must be 16-byte aligned");
    float* slab = (float*)ws;
    float* bslab = dbias ? slab + slab_elems : nullptr;
    const dim3 grid(16 * Cin / WG_K, (Cout + WG_CO - 1) / WG_CO, p.splits);
    if (!with_dtype(dtype, [&](auto elem) {
            using T = decltype(elem);
            hipLaunchKernelGGL(conv4s2_wgrad_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)g, ldg, slab, bslab,
                               B, Hi, Wi, Cin, Ho, Wo, Cout, pad, M, p.rps);
        }))
        return set_error(PSG_ERR_DTYPE, "conv4s2_wgrad: dtype %d", dtype);
    PSG_LAUNCH_CHECK("conv4s2_wgrad");
    const int n = Cout * cin_real * 16 + (dbias ? Cout : 0);
    hipLaunchKernelGGL(conv4s2_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, slab, bslab, dw, dbias, Cout, Cin,
                       cin_real, dw_layout == PSG_W_OHWI ? 1 : 0, p.splits, accumulate, accumulate_bias);
    PSG_LAUNCH_CHECK("conv4s2_finish");
    return PSG_OK;
}

}  // extern "C"
