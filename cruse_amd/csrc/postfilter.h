// The perceptual post-filter of a mask value (the reference's utils/utils.py:345-362), shared by the streaming decode kernels
// (stream.hip, the PF instances) and the offline pointwise kernel (postfilter.hip).
//
// g: the mask value in [0, 1], s = sin(pi g / 2), tau >= 0.
//   kind 1 ("iam", postfiltering :345-349):                 pf = g (1 + tau) s^2 / (s^2 + tau)
//   kind 2 ("envelope", envelope_postfiltering :352-362):   pf = g s sqrt((1 + tau) s / (s^2 + tau))
// Both are the reference's expressions in closed form, with two repairs: at g = 0 the reference's "iam" form is 0 / 0,
// the closed form gives the limit 0; the "envelope" form's eps term, the only way the unprocessed magnitude enters, is dropped.
// tau == 0 is an explicit bypass (g to the bit), not the formula at tau = 0.
#pragma once
#include "common.h"

namespace cruse_pf {

enum { KIND_IAM = 1, KIND_ENVELOPE = 2 };

__device__ __forceinline__ float post_filter(float g, float tau, int kind) {
    if (tau == 0.0f) return g;
    const float s = sinf(1.57079632679489662f * g);
    const float s2 = s * s;
    const float den = s2 + tau;                           // > 0: tau > 0
    if (kind == KIND_IAM) return g * (((1.0f + tau) * s2) / den);
    return g * s * sqrtf(((1.0f + tau) * s) / den);
}

inline int kind_args(const char* who, int kind) {
    CRUSE_REQUIRE(kind == KIND_IAM || kind == KIND_ENVELOPE, CRUSE_E_SHAPE, "%s: post-filter kind %d (1: iam, 2: envelope)", who, kind);
    return CRUSE_OK;
}

}  // namespace cruse_pf
