// cruse_mask_postfilter: the reference's perceptual post-filters (utils/utils.py:345-362) on a whole mask tensor, one pointwise launch.
// The function itself is postfilter.h's, the one the streaming decode kernels apply in their gain line.
#include "postfilter.h"

namespace {

using cruse_pf::post_filter;

// mask / out: n = rows * F floats; element i reads tau[i / span] (span = rows_per_tau * F), tau[0] where span == 0.  VEC: both pointers
// are 16-byte aligned: float4 accesses over the first n / 4 * 4 elements, scalar over the rest.  out may be mask (every element is read
// by the thread that writes it).
template <bool VEC>
__global__ __launch_bounds__(256) void mask_postfilter_kernel(int kind, const float* mask, long long n, long long span, const float* tau,
                                                              float* out) {
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    long long done = 0;
    if constexpr (VEC) {
        const long long n4 = n >> 2;
        for (long long v = t0; v < n4; v += stride) {
            const long long i = v << 2;
            const float4 g = reinterpret_cast<const float4*>(mask)[v];
            const long long a = span ? i / span : 0, b = span ? (i + 3) / span : 0;
            const float ta = tau[a], tb = tau[b];
            float4 r;
            if (a == b) {
                r.x = post_filter(g.x, ta, kind); r.y = post_filter(g.y, ta, kind);
                r.z = post_filter(g.z, ta, kind); r.w = post_filter(g.w, ta, kind);
            } else {                                       // the vector straddles tau groups (span may be as small as 1)
                r.x = post_filter(g.x, ta, kind);
                r.y = post_filter(g.y, tau[(i + 1) / span], kind);
                r.z = post_filter(g.z, tau[(i + 2) / span], kind);
                r.w = post_filter(g.w, tb, kind);
            }
            reinterpret_cast<float4*>(out)[v] = r;
        }
        done = n4 << 2;
    }
    for (long long i = done + t0; i < n; i += stride) out[i] = post_filter(mask[i], tau[span ? i / span : 0], kind);
}

}  // namespace

extern "C" int cruse_mask_postfilter(int kind, const float* mask, long long rows, long long F, const float* tau, long long rows_per_tau,
                                     float* out, void* stream) {
    const int rc = cruse_pf::kind_args("mask_postfilter", kind);
    if (rc) return rc;
    CRUSE_REQUIRE(rows >= 1 && F >= 1 && rows <= 0x7fffffffffffffffLL / F / 4, CRUSE_E_SHAPE, "mask_postfilter: rows = %lld, F = %lld", rows, F);
    CRUSE_REQUIRE(rows_per_tau >= 0 && rows_per_tau <= rows, CRUSE_E_SHAPE, "mask_postfilter: rows_per_tau = %lld outside [0, rows = %lld]",
                  rows_per_tau, rows);
    CRUSE_REQUIRE(mask && tau && out, CRUSE_E_SHAPE, "mask_postfilter: null mask, tau or out");
    const long long n = rows * F, span = rows_per_tau * F;
    const bool vec = n >= 4 && (((uintptr_t)mask | (uintptr_t)out) & 15) == 0;
    long long g = ((vec ? n / 4 + 3 : n) + 255) / 256;
    if (g > 4096) g = 4096;
    if (vec)
        hipLaunchKernelGGL(mask_postfilter_kernel<true>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, kind, mask, n, span, tau, out);
    else
        hipLaunchKernelGGL(mask_postfilter_kernel<false>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, kind, mask, n, span, tau, out);
    CRUSE_LAUNCH_CHECK("mask_postfilter");
    return CRUSE_OK;
}
