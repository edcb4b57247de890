// Implicit-GEMM convolution / linear: C ABI, descriptor checks and tile choice.  The kernel template lives in
// conv_gemm_kernel.h; each (dtype, tile) instantiation is its own translation unit (conv_tile.hip compiled once per tile,
// see the Makefile) so that the eight of them build in parallel - one file with all of them took five minutes.
#include "conv_gemm_kernel.h"
#include <cstring>
#include <mutex>
#include <queue>
#include <vector>

namespace psg {

// One row per (dtype, BM, BN) tile of conv_gemm_kernel; each is instantiated in its own conv_tile_<dtype>_<BM>_<BN>.o, which
// exports the tile's kernels (conv_kernels: null where a (mode, split, class) combination is not built).  The plan's scoring
// and split-K estimate, psg_conv_init_attrs, the range of the tile pin and the launch read these rows and nothing else: fp32
// and parity-class launches have no 160-wide tile because there is no such row / kernel.  (The Makefile's TILES is the
// build's list of the same tiles: a row without its object is an undefined symbol when the library is loaded.)
struct ConvTile {
    int dtype, BM, BN;
    int cand;                      // the candidate number PSG_CONV_TILE / psg_conv_set_tile pins
    double eff;                    // measured relative MFMA efficiency of the tile shape
    // (a K <= 640 boost for 128x64 - three resident workgroups hiding the short loop ends - paid before the epilogue was
    //  specialised per kind; since then 128x128 wins those layers by 10 %: gemm_direct.py)
    const ConvKernels& (*kernels)();
};
#define PSG_TILE(D, T, BM, BN, CAND, EFF) {D, BM, BN, CAND, EFF, conv_kernels<T, BM, BN>}
static const ConvTile CONV_TILES[] = {
    PSG_TILE(PSG_BF16, bf16_t, 128, 128, 0, 1.0), PSG_TILE(PSG_BF16, bf16_t, 128, 64, 1, 0.78), PSG_TILE(PSG_BF16, bf16_t, 64, 64, 2, 0.55),
    PSG_TILE(PSG_BF16, bf16_t, 128, 160, 3, 1.0), PSG_TILE(PSG_BF16, bf16_t, 64, 160, 4, 0.70),  // 160 = 2 x 5 x 16: only the 16x16x32 bf16 tiles divide it
    PSG_TILE(PSG_F32, float, 128, 128, 0, 1.0),   PSG_TILE(PSG_F32, float, 128, 64, 1, 0.78),   PSG_TILE(PSG_F32, float, 64, 64, 2, 0.55),
};
#undef PSG_TILE

// Settings: the environment, read once (PSG_CONV_TILE = candidate pins the tile; PSG_CONV_SPLITK / PSG_CONV_PW / PSG_EPI_LDS /
// PSG_EPI_KINDS = 0 turn split-K, the persistent pointwise kernel, the LDS-staged stores and the per-kind epilogues off;
// PSG_CONV_TAPCLASS = 0 / 1 / 2), and the pins of psg_conv_set_tile / _set_tapclass / _set_pw (kernel A/B runs, tests).
struct ConvSettings {
    int tile;                      // pinned candidate, -1: the plan's choice.  A pinned launch is never split
    bool splitk;
    int tapcls;                    // border-class form: 0 off, 1 where tapcls_pays says so, 2 on every launch it applies to
    bool pw, epi_lds, epi_kinds;
};
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int tile_pin(int c) { for (const ConvTile& t : CONV_TILES) if (t.cand == c) return c; return -1; }
static int tapcls_pin(int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }
static ConvSettings& conv_settings() {
    static ConvSettings s = {tile_pin(env_int("PSG_CONV_TILE", -1)), env_int("PSG_CONV_SPLITK", 1) != 0, tapcls_pin(env_int("PSG_CONV_TAPCLASS", 1)),
                             env_int("PSG_CONV_PW", 1) != 0, env_int("PSG_EPI_LDS", 1) != 0, env_int("PSG_EPI_KINDS", 1) != 0};
    return s;
}
static int64_t g_tapcls_launches = 0, g_pw_launches = 0;

// gather mode of a launch (MODE of conv_gemm_kernel)
static int conv_mode(const ConvP& p) { return p.ntap > 0 ? 3 : (!p.fast ? 2 : (!p.transposed ? 0 : (p.stride == 1 ? 1 : 2))); }
static int64_t conv_ws_bytes(const ConvP& p, int splits) { return splits > 1 ? (int64_t)splits * p.M * p.N * 4 : 0; }
static double conv_tile_count(const ConvP& p, const ConvTile& t) { return (double)(((int64_t)p.M + t.BM - 1) / t.BM) * (double)((p.N + t.BN - 1) / t.BN); }

// tile choice: maximise (useful fraction of the tile grid) x (chip fill of the last wave) x (tile efficiency); then, for
// grids that leave most of the chip idle (small M: sampling, small batches), split-K on top
struct ConvPlan { const ConvTile* tile; int splits, kt_per_split; };
static ConvPlan conv_plan(const ConvP& p, int dtype, bool may_split) {
    const ConvSettings& st = conv_settings();
    const int64_t M = p.M;
    const int mode = conv_mode(p);
    ConvPlan pl = {nullptr, 1, p.KT};
    if (st.tile >= 0) {                                    // pinned: that row (none: no such tile for the dtype), unsplit
        for (const ConvTile& t : CONV_TILES) if (t.dtype == dtype && t.cand == st.tile) pl.tile = &t;
        return pl;
    }
    // resident workgroups on the chip (2 per CU; psg_set_available_cus / psg_set_reserve_rounds)
    const double slots = 2.0 * avail_cus_for((double)((M + 127) / 128) * (double)((p.N + 127) / 128) / 512.0);
    double best = -1.0;
    for (const ConvTile& t : CONV_TILES) {
        if (t.dtype != dtype || !t.kernels().gemm[mode][0][0]) continue;
        const double tiles = conv_tile_count(p, t);
        const double useful = (double)M * p.N / (tiles * t.BM * t.BN);
        const double waves = ceil(tiles / slots);
        const double score = useful * (tiles / (waves * slots)) * t.eff;
        if (score > best) { best = score; pl.tile = &t; }
    }
    // Split-K: when the unsplit grid fills less than ~60 % of the chip and the K loop is long enough to share.  Estimated time
    // of (tile t, s splits) in K steps of a 128 x 128 tile: rounds x (steps per split + 6 of prologue / epilogue) x
    // (tile area / efficiency) + the partial tiles' trip through memory ((s + 1) x M x N x 4 bytes at ~3 TB/s, 0.9 us per step).
    if (may_split && st.splitk && pl.tile && p.KT >= 16 && (conv_tile_count(p, *pl.tile) < 0.6 * slots || best < 0.6)) {
        auto est = [&](const ConvTile& t, int s) {
            const int per = (p.KT + s - 1) / s;
            const double rounds = ceil(conv_tile_count(p, t) * s / slots);
            const double step = (double)t.BM * t.BN / (128.0 * 128.0) / t.eff;
            const double fin = s > 1 ? ((s + 1.0) * (double)M * p.N * 4.0 / 3.0e6 + 4.0) / 0.9 : 0.0;
            return rounds * (per + 6.0) * step + fin;
        };
        double tbest = est(*pl.tile, 1);
        const int svals[9] = {2, 3, 4, 5, 6, 8, 10, 12, 16};
        for (const ConvTile& t : CONV_TILES) {
            if (t.dtype != dtype || !t.kernels().gemm[mode][1][0]) continue;
            for (int si = 0; si < 9; ++si) {
                const int s = svals[si];
                if (p.KT / s < 8) break;                       // at least 8 K steps per split
                if ((double)s * M * p.N * 4.0 > 256.0e6) break;   // partial tiles: <= 256 MB
                const double e = est(t, s);
                if (e < tbest * 0.9) { tbest = e; pl.tile = &t; pl.splits = s; }
            }
        }
        if (pl.splits > 1) { pl.kt_per_split = (p.KT + pl.splits - 1) / pl.splits; pl.splits = (p.KT + pl.kt_per_split - 1) / pl.kt_per_split; }
    }
    return pl;
}

// Border-class form (TapCls in conv_gemm_kernel.h; ConvSettings::tapcls).  It applies to: a tile with the kernel (bf16), the
// taps-innermost fast path, stride-1 3x3 pad 1 (forward or data gradient), at least 3 x 3 positions, unsplit
static bool tapcls_applicable(const ConvP& p, const ConvKernels& k) {
    return k.gemm[conv_mode(p)][0][1] && p.fast && p.ks == 3 && p.stride == 1 && p.pad == 1 && p.Ho >= 3 && p.Wo >= 3 &&
           p.splits == 1 && (int64_t)p.M + 9 * 128 < (1 << 24);
}
static int tapcls_mtiles(const ConvP& p, int BM) {
    const TapCls c = tapcls_of(p, BM, 1 << 30, p.transposed != 0);
    return c.r0 / BM + (c.nrow + BM - 1) / BM;
}

// Makespan estimate of the plain and the border-class grid of a BM x BN plan.  The two resident workgroups of a CU share its
// matrix pipe, so a CU is one machine that works off the K steps of its tiles; each tile goes, in dispatch order (the class
// order is heaviest first), to the CU with the least work so far, at K steps + TAPCLS_OV of prologue / epilogue (+ TAPCLS_EPI
// for the class form's per-row stores).  The class form is used when it shortens the estimate by TAPCLS_GAIN, and only on
// grids of more than one round of resident workgroups: in a single round the 9-tap tiles set the time whatever the others do,
// and the light tiles do not land beside them (4x4 layers, 64x160 tiles: 10-13 % slower in class order).  Per-layer
// measurement (tools/tapcls_bench.py): 27x27 +1..4 %, 14x14 +2..4 %, 7x7 +3.5..4 %.
static constexpr double TAPCLS_OV = 6.0, TAPCLS_EPI = 1.0, TAPCLS_GAIN = 0.02;
static bool tapcls_pays(const ConvP& p, int BM, int BN) {
    const int ntiles = (p.N + BN - 1) / BN;
    const int mtiles = (p.M + BM - 1) / BM;
    const int cus = avail_cus_for((double)mtiles * ntiles / 512.0);
    if ((int64_t)mtiles * ntiles <= 2 * cus) return false;
    struct Key { int B, Ho, Wo, N, tpt, dg, BM, BN, cus; bool operator==(const Key& o) const { return !memcmp(this, &o, sizeof(Key)); } };
    static std::mutex mu;
    static std::vector<std::pair<Key, bool>> memo;
    const Key key = {p.B, p.Ho, p.Wo, p.N, p.tpt, p.transposed, BM, BN, cus};
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : memo) if (e.first == key) return e.second;
    auto span = [&](bool cls) {
        std::priority_queue<double, std::vector<double>, std::greater<double>> q;
        for (int i = 0; i < cus; ++i) q.push(0.0);
        double sp = 0.0;
        const int total = cls ? tapcls_mtiles(p, BM) : mtiles;
        for (int mt = 0; mt < total; ) {
            const TapCls c = tapcls_of(p, BM, mt, p.transposed != 0);
            const int n = cls ? c.r0 / BM + (c.nrow + BM - 1) / BM - mt : total;
            const double d = cls ? (double)p.tpt * (c.kh1 - c.kh0 + 1) * (c.kw1 - c.kw0 + 1) + TAPCLS_OV + TAPCLS_EPI : 9.0 * p.tpt + TAPCLS_OV;
            for (int t = 0; t < n * ntiles; ++t) { const double f = q.top() + d; q.pop(); q.push(f); sp = f > sp ? f : sp; }
            mt += n;
        }
        return sp;
    };
    const bool pays = span(true) < (1.0 - TAPCLS_GAIN) * span(false);
    memo.push_back({key, pays});
    return pays;
}

// The plan of one launch: the tile, the K split, the border-class order, persistent pointwise or per-tile kernel, the grid,
// the LDS and workspace bytes and the profile's work figures (ConvLaunch).  "No kernel for this (dtype, tile, mode, split,
// class)" is decided here, from the tile table, for psg_conv_route and psg_conv_fwd alike.  size_only: stop once the split
// (ws_bytes) is known - psg_conv_fwd_workspace_bytes, which must not pay for tapcls_pays.
static int conv_plan_launch(const ConvP& p0, int dtype, bool size_only, ConvLaunch& L) {
    const ConvSettings& st = conv_settings();
    ConvP& p = L.p;
    p = p0;
    ConvPlan pl = conv_plan(p, dtype, p.ws != nullptr);
    if (conv_ws_bytes(p, pl.splits) > p.ws_bytes) pl = conv_plan(p, dtype, false);   // workspace too small: the best UNSPLIT tile, not the split plan's tile
    PSG_REQUIRE(pl.tile, PSG_ERR_ARG, "conv_gemm: no %s tile for candidate %d", dtype == PSG_BF16 ? "bf16" : "fp32", st.tile);
    const int BM = pl.tile->BM, BN = pl.tile->BN;
    const ConvKernels& k = pl.tile->kernels();
    p.splits = pl.splits; p.kt_per_split = pl.kt_per_split;
    L.ws_bytes = conv_ws_bytes(p, p.splits);
    if (size_only) return PSG_OK;
    p.tapcls = (st.tapcls && tapcls_applicable(p, k) && (st.tapcls == 2 || tapcls_pays(p, BM, BN))) ? 1 : 0;
    L.BM = BM; L.BN = BN; L.mode = conv_mode(p);
    L.kernel = k.gemm[L.mode][p.splits > 1][p.tapcls]; L.finish = k.finish;
    // (only a pinned tile gets here without a kernel - 160 wide, parity class: the plan skips the null entries)
    PSG_REQUIRE(L.kernel, PSG_ERR_ARG, "conv_gemm: no %s %dx%d kernel for mode %d", dtype == PSG_BF16 ? "bf16" : "fp32", BM, BN, L.mode);
    L.pw = (st.pw && BM == 128 && BN == 128 && conv_pw_plan(dtype, L)) ? 1 : 0;
    if (!L.pw) {
        L.mtiles = p.tapcls ? tapcls_mtiles(p, BM) : (p.M + BM - 1) / BM; L.ntiles = (p.N + BN - 1) / BN;
        L.grid = L.mtiles * L.ntiles * p.splits;
        L.lds = conv_lds(BM, BN, p.tapcls);
    }
    p.mtiles = L.mtiles; p.ntiles = L.ntiles;
    L.epi_lds = (p.epi_lds && p.splits == 1) ? 1 : 0;
    // useful FLOPs; algorithmic bytes: every input pixel, weight and output element once (+ the epilogue's residual / saved tensors)
    L.flops = 2.0 * (double)p.M * (double)p.N * (double)p.taps * (double)p.Cin;
    L.abytes = ((double)p.B * p.Hi * p.Wi * p.Cin + (double)p.N * p.taps * p.Cin + (double)p.M * p.N * (1.0 + (p.residual || p.dact_u ? 1.0 : 0.0) + (p.preact ? 1.0 : 0.0))) *
               (dtype == PSG_BF16 ? 2.0 : 4.0);
    return PSG_OK;
}

// The launches of a descriptor that conv_setup accepted: one, or up to four for the data gradient of a stride-2 3x3 conv
static int conv_plan_all(const ConvP& p, int dtype, bool size_only, ConvLaunch (&L)[4], int& n) {
    n = 0;
    if (p.transposed && p.stride == 2 && p.fast && p.ks == 3) {
        // Data gradient of a stride-2 conv: a result pixel (ho, wo) is reached only by the taps with
        // kh = (ho + pad) mod 2 (mod 2), same for kw - 1, 2, 2 or 4 of the 9.  One launch per parity class, each a
        // dense stride-1-like gather on the class's own grid: 2.25 taps per pixel on average instead of 9.
        for (int ah = 0; ah < 2; ++ah)
            for (int aw = 0; aw < 2; ++aw) {
                ConvP q = p;
                q.sub_h0 = (ah - p.pad) & 1; q.sub_w0 = (aw - p.pad) & 1;
                q.sub_nH = (p.Ho - q.sub_h0 + 1) >> 1; q.sub_nW = (p.Wo - q.sub_w0 + 1) >> 1;
                if (q.sub_nH <= 0 || q.sub_nW <= 0) continue;
                q.ntap = 0;
                for (int kh = ah; kh < 3; kh += 2)
                    for (int kw = aw; kw < 3; kw += 2) {
                        q.tap_dh[q.ntap] = (q.sub_h0 + p.pad - kh) / 2;
                        q.tap_dw[q.ntap] = (q.sub_w0 + p.pad - kw) / 2;
                        q.tap_wi[q.ntap] = kh * 3 + kw;
                        ++q.ntap;
                    }
                q.M = p.B * q.sub_nH * q.sub_nW;
                q.taps = q.ntap;                           // (profiling: useful FLOPs of this class)
                q.KT = q.ntap * p.tpt;
                const int rc = conv_plan_launch(q, dtype, size_only, L[n]);
                if (rc) return rc;
                ++n;
            }
        return PSG_OK;
    }
    const int rc = conv_plan_launch(p, dtype, size_only, L[0]);
    if (rc) return rc;
    n = 1;
    return PSG_OK;
}

static int launch_planned(const ConvLaunch& L, hipStream_t s) {
    ConvP p = L.p;
#ifdef PSG_ABL
    if (PSG_ABL & 8) { const char* e = getenv("PSG_DBG_PTR"); p.ws = (e && p.splits <= 1) ? reinterpret_cast<float*>(strtoull(e, nullptr, 0)) : (p.splits <= 1 ? nullptr : p.ws); }
#endif
    ProfScope prof(p.transposed ? PROF_CONV_DGRAD : PROF_CONV_FWD, L.flops, s, L.abytes);
    const ConvP fin = p;                               // (the finishing kernel runs the epilogue: it keeps the operands)
    if (p.splits > 1) { p.bias = nullptr; p.rowadd = nullptr; p.residual = nullptr; p.preact = nullptr; p.dact_u = nullptr; }
    if (L.pw) hipLaunchKernelGGL(L.pw_kernel, dim3(L.grid), dim3(256), L.lds, s, p, L.mtiles * L.ntiles, L.aux_bytes);
    else hipLaunchKernelGGL(L.kernel, dim3(L.grid), dim3(256), L.lds, s, p);
    g_pw_launches += L.pw; g_tapcls_launches += p.tapcls;
    PSG_LAUNCH_CHECK(L.pw ? "conv_pw launch" : "conv_gemm launch");
    if (p.splits > 1) {
        const int64_t n = (int64_t)p.M * (p.N >> 2);
        hipLaunchKernelGGL(L.finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fin);
        PSG_LAUNCH_CHECK("conv_splitk_finish launch");
    }
    return PSG_OK;
}

}  // namespace psg
using namespace psg;

extern "C" {

int psg_conv_init_attrs(void) {
    for (const ConvTile& t : CONV_TILES)
        for (const auto& mode : t.kernels().gemm)
            for (const auto& split : mode)
                for (int cls = 0; cls < 2; ++cls)
                    if (split[cls]) if (int rc = set_max_lds(conv_lds(t.BM, t.BN, cls), split[cls])) return rc;
    return conv_pw_set_attrs();
}

static int conv_setup(const psg_conv_desc* d, ConvP& p) {
    PSG_REQUIRE(d && d->x && d->w && d->y, PSG_ERR_ARG, "conv_fwd: null pointer");
    PSG_REQUIRE(d->dtype == PSG_F32 || d->dtype == PSG_BF16, PSG_ERR_DTYPE, "conv_fwd: dtype %d", d->dtype);
    const int CH = d->dtype == PSG_BF16 ? 8 : 4;
    PSG_REQUIRE(d->B > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0 && d->Ho > 0 && d->Wo > 0 && d->Cout > 0, PSG_ERR_SHAPE,
                "conv_fwd: non-positive dimension");
    PSG_REQUIRE((d->ksize == 1 && d->pad == 0) || (d->ksize == 3 && d->pad == 1) ||
                (d->ksize == 4 && (d->pad == 1 || d->pad == 2) && d->stride == 2 && !d->transposed),
                PSG_ERR_SHAPE, "conv_fwd: ksize/pad/stride %d/%d/%d", d->ksize, d->pad, d->stride);
    PSG_REQUIRE(d->stride == 1 || d->stride == 2, PSG_ERR_SHAPE, "conv_fwd: stride %d", d->stride);
    PSG_REQUIRE(d->Cin % CH == 0, PSG_ERR_SHAPE, "conv_fwd: Cin=%d must be a multiple of %d", d->Cin, CH);
    PSG_REQUIRE(d->Cout % 4 == 0, PSG_ERR_SHAPE, "conv_fwd: Cout=%d must be a multiple of 4", d->Cout);
    PSG_REQUIRE(d->ldx >= d->Cin && d->ldx % CH == 0, PSG_ERR_SHAPE, "conv_fwd: ldx=%ld (Cin=%d)", (long)d->ldx, d->Cin);
    PSG_REQUIRE(d->ldy >= d->Cout && d->ldy % 4 == 0, PSG_ERR_SHAPE, "conv_fwd: ldy=%ld", (long)d->ldy);
    PSG_REQUIRE(aligned16(d->x) && aligned16(d->w) && aligned16(d->y), PSG_ERR_ALIGN, "conv_fwd: x/w/y must be 16-byte aligned");
    PSG_REQUIRE(!d->bias || aligned16(d->bias), PSG_ERR_ALIGN, "conv_fwd: bias alignment");
    PSG_REQUIRE(!d->rowadd || (aligned16(d->rowadd) && d->ld_rowadd % 4 == 0), PSG_ERR_ALIGN, "conv_fwd: rowadd alignment");
    PSG_REQUIRE(!d->residual || (aligned16(d->residual) && d->ld_residual % 4 == 0), PSG_ERR_ALIGN, "conv_fwd: residual alignment");
    PSG_REQUIRE(!d->preact || (aligned16(d->preact) && d->ld_preact % 4 == 0), PSG_ERR_ALIGN, "conv_fwd: preact alignment");
    PSG_REQUIRE(!d->dact_u || (aligned16(d->dact_u) && d->ld_dact % 4 == 0), PSG_ERR_ALIGN, "conv_fwd: dact_u alignment");
    PSG_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, PSG_ERR_ARG, "conv_fwd: drop_p %f", d->drop_p);
    PSG_REQUIRE(d->act >= PSG_ACT_NONE && d->act <= PSG_ACT_QUICK_GELU, PSG_ERR_ARG, "conv_fwd: unknown act %d", d->act);
    PSG_REQUIRE(!(d->residual && d->dact_u), PSG_ERR_ARG, "conv_fwd: residual and dact_u are mutually exclusive");
    PSG_REQUIRE((d->flags & ~(PSG_CONV_SAVE_DACT | PSG_CONV_DACT_MUL | PSG_CONV_GENERIC_EPILOGUE)) == 0, PSG_ERR_ARG, "conv_fwd: unknown flags 0x%x", d->flags);
    PSG_REQUIRE(!(d->flags & PSG_CONV_SAVE_DACT) || (d->preact && !d->dact_u), PSG_ERR_ARG, "conv_fwd: SAVE_DACT needs preact (forward form)");
    PSG_REQUIRE(!(d->flags & PSG_CONV_DACT_MUL) || (d->dact_u && d->drop_p == 0.f), PSG_ERR_ARG,
                "conv_fwd: DACT_MUL needs dact_u and drop_p = 0 (the saved derivative already carries the mask)");
    // geometry consistency
    if (!d->transposed) {
        PSG_REQUIRE(d->Ho == (d->Hi + 2 * d->pad - d->ksize) / d->stride + 1 && d->Wo == (d->Wi + 2 * d->pad - d->ksize) / d->stride + 1,
                    PSG_ERR_SHAPE, "conv_fwd: output %dx%d inconsistent with input %dx%d k%d s%d p%d", d->Ho, d->Wo, d->Hi, d->Wi, d->ksize, d->stride, d->pad);
    } else {
        PSG_REQUIRE(d->Hi == (d->Ho + 2 * d->pad - d->ksize) / d->stride + 1 && d->Wi == (d->Wo + 2 * d->pad - d->ksize) / d->stride + 1,
                    PSG_ERR_SHAPE, "conv_fwd(transposed): grad grid %dx%d inconsistent with input grid %dx%d", d->Hi, d->Wi, d->Ho, d->Wo);
    }
    const int64_t M = (int64_t)d->B * d->Ho * d->Wo;
    PSG_REQUIRE(M < (1ll << 30) && (int64_t)d->B * d->Hi * d->Wi < (1ll << 30), PSG_ERR_SHAPE, "conv_fwd: too many pixels");
    const int taps = d->ksize * d->ksize;
    const int64_t Kpad = psg_kpad((int64_t)taps * d->Cin, d->dtype);
    PSG_REQUIRE(d->ldw == 0 || (d->ldw >= Kpad && d->ldw % CH == 0), PSG_ERR_SHAPE, "conv_fwd: ldw=%ld < Kpad=%ld", (long)d->ldw, (long)Kpad);

    p.x = d->x; p.w = d->w; p.y = d->y; p.bias = d->bias; p.rowadd = d->rowadd; p.residual = d->residual;
    p.preact = d->preact; p.dact_u = d->dact_u;
    p.ldw = d->ldw > 0 ? d->ldw : Kpad;
    p.ldx = d->ldx; p.ldy = d->ldy; p.ldra = d->ld_rowadd; p.ldres = d->ld_residual; p.ldpre = d->ld_preact; p.lddact = d->ld_dact;
    p.B = d->B; p.Hi = d->Hi; p.Wi = d->Wi; p.Cin = d->Cin; p.Ho = d->Ho; p.Wo = d->Wo; p.N = d->Cout;
    p.ks = d->ksize; p.stride = d->stride; p.pad = d->pad; p.transposed = d->transposed;
    p.M = (int)M; p.taps = taps; p.cpt = d->Cin / CH; p.Kpad = (int)Kpad; p.KT = (int)(Kpad / (8 * CH));
    p.fast = (p.cpt % 8 == 0) ? 1 : 0; p.tpt = p.fast ? p.cpt / 8 : 1;
    p.act = d->act; p.alpha = d->alpha; p.flags = d->flags;
    // coalesced (LDS-staged) stores need 16-byte row chunks: bf16, channel counts and row strides multiples of 8
    p.epi_lds = (conv_settings().epi_lds && d->dtype == PSG_BF16 && d->Cout % 8 == 0 && d->ldy % 8 == 0 && (!d->preact || d->ld_preact % 8 == 0) &&
                 (!d->residual || d->ld_residual % 8 == 0) && (!d->dact_u || d->ld_dact % 8 == 0)) ? 1 : 0;
    p.epi_generic = (!conv_settings().epi_kinds || (d->flags & PSG_CONV_GENERIC_EPILOGUE)) ? 1 : 0;
    p.drop_thresh = d->drop_p > 0.f ? drop_thresh(d->drop_p) : 0u;
    p.drop_scale = d->drop_p > 0.f ? 1.0f / (1.0f - d->drop_p) : 1.0f;
    p.drop_seed = d->drop_seed;
    p.seed_dev = seed_source();
    p.mtiles = p.ntiles = 0;
    {
        const int64_t esz = d->dtype == PSG_BF16 ? 2 : 4;
        const int64_t xb = (((int64_t)d->B * d->Hi * d->Wi - 1) * d->ldx + d->Cin) * esz;
        const int64_t wb = (((int64_t)d->Cout - 1) * p.ldw + Kpad) * esz;
        PSG_REQUIRE(xb < 0x7FFFFFF0ll && wb < 0x7FFFFFF0ll, PSG_ERR_SHAPE, "conv_fwd: operand extent >= 2 GiB (x %ld B, w %ld B)", (long)xb, (long)wb);
        p.x_bytes = (uint32_t)xb; p.w_bytes = (uint32_t)wb;
    }
    p.ws = (d->ws && aligned16(d->ws)) ? reinterpret_cast<float*>(d->ws) : nullptr;
    p.ws_bytes = p.ws ? d->ws_bytes : 0;
    p.splits = 1; p.kt_per_split = p.KT;
    p.ntap = 0; p.sub_h0 = p.sub_w0 = p.sub_nH = p.sub_nW = 0;
    p.tapcls = 0;
    return PSG_OK;
}

// Bytes of workspace with which psg_conv_fwd would split the K axis of this launch over several workgroups (0: it would not -
// large grids, stride-2 data gradients, short K).  The workspace is optional: without it (ws NULL / too small) the launch
// runs unsplit.  Meant for small-M launches (sampling, small batches); the call costs a plan evaluation on the host.
int64_t psg_conv_fwd_workspace_bytes(const psg_conv_desc* d) {
    ConvP p;
    if (conv_setup(d, p) != PSG_OK) return -1;
    static float any_ws;                               // plan as psg_conv_fwd would with an unlimited workspace
    p.ws = &any_ws; p.ws_bytes = INT64_MAX;
    ConvLaunch L[4];
    int n = 0;
    if (conv_plan_all(p, d->dtype, true, L, n)) return 0;    // (a pinned tile the dtype has no row for: pinned launches are never split)
    return L[0].ws_bytes;                              // (parity-class launches - the only plans of more than one - are never split)
}

int psg_conv_fwd(const psg_conv_desc* d, psg_stream_t stream) {
    ConvP p;
    int rc = conv_setup(d, p);
    if (rc) return rc;
    ConvLaunch L[4];
    int n = 0;
    if ((rc = conv_plan_all(p, d->dtype, false, L, n))) return rc;
    for (int i = 0; i < n; ++i)
        if ((rc = launch_planned(L[i], (hipStream_t)stream))) return rc;
    return PSG_OK;
}

int psg_conv_route(const psg_conv_desc* d, int32_t* out) {
    PSG_REQUIRE(out, PSG_ERR_ARG, "conv_route: null pointer");
    ConvP p;
    int rc = conv_setup(d, p);
    if (rc) return rc;
    ConvLaunch L[4];
    int n = 0;
    if ((rc = conv_plan_all(p, d->dtype, false, L, n))) return rc;
    for (int i = 0; i < 1 + 4 * PSG_CONV_ROUTE_FIELDS; ++i) out[i] = 0;
    out[0] = n;
    for (int i = 0; i < n; ++i) {
        const ConvP& q = L[i].p;
        const int32_t v[PSG_CONV_ROUTE_FIELDS] = {L[i].BM, L[i].BN, L[i].mode, q.splits, q.kt_per_split, q.tapcls, L[i].pw, L[i].epi_lds,
                                                  L[i].mtiles, L[i].ntiles, L[i].grid, q.M, q.KT, q.sub_h0, q.sub_w0, q.sub_nH, q.sub_nW, q.ntap};
        for (int f = 0; f < PSG_CONV_ROUTE_FIELDS; ++f) out[1 + i * PSG_CONV_ROUTE_FIELDS + f] = v[f];
    }
    return PSG_OK;
}

int psg_conv_set_tile(int c) { conv_settings().tile = tile_pin(c); return PSG_OK; }
int psg_conv_set_tapclass(int on) { conv_settings().tapcls = tapcls_pin(on); return PSG_OK; }
int psg_conv_set_pw(int on) { conv_settings().pw = on != 0; return PSG_OK; }
int64_t psg_conv_tapclass_launches(void) { return g_tapcls_launches; }
int64_t psg_conv_pw_launches(void) { return g_pw_launches; }

}  // extern "C"
