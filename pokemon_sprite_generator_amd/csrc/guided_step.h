// One DDIM step of one element, shared by psg_guided_update_f32 (elementwise.hip) and psg_guided_update_pred_f32
// (objective.hip).  Every operation is its own rounding (__f*_rn), so tests/guided_ref.py and tests/objective_ref.py give
// the same bits in numpy float32.
#pragma once
#include "psg_common.h"

namespace psg {

struct GuidedCoef { float s0, s1, p0, p1, sg; };

// classifier-free guidance on the network's output, whatever it predicts: u + w (c - u); c alone without an unconditional half
__device__ __forceinline__ float guided_combine(float pc, float pu, bool has_u, float w) {
    return has_u ? __fadd_rn(pu, __fmul_rn(w, __fsub_rn(pc, pu))) : pc;
}

// From (x0, e) on: the clamp lets NaN through (both comparisons are false), as numpy.clip; `c != x0` is then true and e
// becomes NaN with it.
__device__ __forceinline__ float guided_finish(float x, float x0, float e, const GuidedCoef& k, float clip, float z, bool has_z) {
    if (clip > 0.f) {
        const float c = x0 < -clip ? -clip : (x0 > clip ? clip : x0);
        if (c != x0) e = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.s0, c)), k.s1);
        x0 = c;
    }
    float r = __fadd_rn(__fmul_rn(k.p0, x0), __fmul_rn(k.p1, e));
    if (has_z) r = __fadd_rn(r, __fmul_rn(k.sg, z));
    return r;
}

// The formula of psg_guided_update_pred_f32 in psg_hip.h.  PSG_PRED_EPS: x0 = (x - S1 e) / S0, psg_guided_update_f32's own
// line; PSG_PRED_V: x0 = S0 x - S1 v and e = S1 x + S0 v, no division.
template <int PRED>
__device__ __forceinline__ float guided_elem_pred(float x, float pc, float pu, bool has_u, float w, const GuidedCoef& k, float clip,
                                                  float z, bool has_z) {
    const float p = guided_combine(pc, pu, has_u, w);
    float x0, e;
    if (PRED == PSG_PRED_V) {
        x0 = __fsub_rn(__fmul_rn(k.s0, x), __fmul_rn(k.s1, p));
        e = __fadd_rn(__fmul_rn(k.s1, x), __fmul_rn(k.s0, p));
    } else {
        e = p;
        x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.s1, e)), k.s0);
    }
    return guided_finish(x, x0, e, k, clip, z, has_z);
}

__device__ __forceinline__ float guided_elem(float x, float ec, float eu, bool has_u, float w, const GuidedCoef& k, float clip,
                                             float z, bool has_z) {
    return guided_elem_pred<PSG_PRED_EPS>(x, ec, eu, has_u, w, k, clip, z, has_z);
}

}  // namespace psg
