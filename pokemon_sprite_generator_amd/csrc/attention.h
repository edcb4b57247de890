// Attention: the kernel argument block shared by the three kernel families (attention.hip: VALU, attention_mfma.hip: bf16
// matrix cores, attention_f32.hip: exact-fp32 matrix cores) and the MFMA families' host entry points.
#pragma once
#include "psg_common.h"

namespace psg {

// T: element type of q, k, v, o, dout and of every output
template <typename T>
struct AttnArgs {
    const T *q, *k, *v, *o, *dout;
    T *out, *dq, *dk, *dv;
    float* lse; float* delta;                      // delta = rowsum(dO * O): written by the dQ (VALU: delta) kernel, read by dK/dV
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, L, S, d;
    float scale;
    uint32_t drop_thresh; float drop_scale; uint64_t seed;
    const uint64_t* seed_dev;
    const int32_t* kv_len;     // the varlen entries: keys s >= kv_len[b] of sample b are left out (NULL otherwise)
};

// Head-dim list of an MFMA family: the kernels are instantiated for head_dim = 16 * ND, ND in NDs.  Calls
// f(std::integral_constant<int, ND>) for the ND of head_dim d; false when d is not in the list.
template <typename NDs, typename F>
inline bool with_nd(NDs nds, int d, F&& f) { return d % 16 == 0 && with_const(nds, d / 16, f); }
// f(std::integral_constant<int, ND>) for every ND of the list, in order, until one returns non-zero (which is returned)
template <int... NDs, typename F>
inline int for_each_nd(std::integer_sequence<int, NDs...>, F&& f) {
    int rc = PSG_OK;
    ((rc = rc ? rc : f(std::integral_constant<int, NDs>{})), ...);
    return rc;
}

// What the host decides about the launches of one call, written by the family that serves it (attn_mfma_plan, attn_f32_plan,
// attention.hip's valu_plan).  The launches take their grids, workgroup sizes and dynamic LDS from it and psg_attn_route
// reports it: no number here is computed a second time elsewhere.
struct AttnPlan {
    int nd;                      // 16-column slices of head_dim: the ND of an MFMA instantiation, the VALU kernels' ceil(d / 16)
    int waves;                   // waves per workgroup of the forward and of the dQ kernel
    int kw, qw, dkv_waves;       // dK/dV kernel: key-tile waves x query-group waves as the kernel derives them, and the waves launched
    int qw_cut, w_cut;           // qw was reduced until the partial sums fit / the wave count until the private K/V tiles fit
    int nh, kv_reg;              // dK/dV kernel: passes over the head dimension; K/V operands in registers (else private LDS tiles)
    size_t lds_fwd, lds_dq, lds_dkv;
    int grid_q[2], grid_kv[2];   // grid (x, y) of the forward / dQ launch and of the dK/dV launch
};

// whether the family's kernels take this problem: its head_dim and row strides, and the LDS fit of its forward kernel and,
// unless forward_only (psg_attn_fwd_varlen; the training pair psg_attn_fwd_varlen_train / psg_attn_bwd_varlen is not), of its
// backward kernels
bool attn_mfma_applicable(int L, int S, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, bool forward_only);
AttnPlan attn_mfma_plan(int B, int H, int L, int S, int d);
int attn_mfma_init_attrs();
template <bool VARLEN> int attn_mfma_fwd(const AttnArgs<bf16_t>& p, hipStream_t s);
template <bool VARLEN> int attn_mfma_bwd(const AttnArgs<bf16_t>& p, hipStream_t s);

bool attn_f32_applicable(int L, int S, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, bool forward_only);
AttnPlan attn_f32_plan(int B, int H, int L, int S, int d);
int attn_f32_init_attrs();
template <bool VARLEN> int attn_f32_fwd(const AttnArgs<float>& p, hipStream_t s);
template <bool VARLEN> int attn_f32_bwd(const AttnArgs<float>& p, hipStream_t s);

// attention_longq.hip (psg_attn_bwd_longq: few keys, very many queries); its own entry point, never chosen by the routing above
int attn_longq_init_attrs();

}  // namespace psg
