// Causal convolution of a batch of clips with a bank of filters by uniformly partitioned overlap-save FFT convolution
// (cruse_fftconv_*): scipy.signal.fftconvolve(x, h)[:L] of SynDataset.snr_mix / add_reverb (dataset/dataset.py:215-247) at training
// rate, DESIGN section 15.  f32 throughout.  No atomics, one fixed summation order: a result is bit-identical from run to run and a
// clip convolves the same alone and inside a batch.
//
// P = CRUSE_FFTCONV_PART samples per partition, transforms of 2 P real samples done as complex transforms of P points in LDS
// (fftconv_core.h).  A spectrum is P complex values: bins 1 .. P-1, and (X[0], X[P]) -- both real -- in bin 0.
//   prepare  one workgroup per (filter, partition, full | early): spec <- spectrum of h[jP : (j+1)P) followed by P zeros; the early
//            copy takes the taps below clamp(early_len, 0, R) only
//   apply 1  one workgroup per (clip, block i): ws <- spectrum of x[(i-1)P : (i+1)P), zeros outside the clip
//   apply 2  one workgroup per (clip, block i): Y = sum_j X[i-j] H[j], j = 0 .. min(npart, i+1) - 1 ascending, a second accumulator on
//            the early spectra; merge, inverse transform, and the second half of the 2 P samples is y[iP : (i+1)P), cut at L
// A clip whose filter index is negative or >= NR is not transformed: apply 2 copies x to y (and y_early).
#include "common.h"
#include "fftconv_core.h"

namespace {

constexpr int P = FC_N;
constexpr int MAX_L = 1 << 30;
constexpr size_t SPEC_ONE = (size_t)P * sizeof(cf);                    // bytes of one spectrum

// v (point tid + 256 t) -> v (bin tid + 256 m); ends without a barrier, s is still being read
__device__ __forceinline__ void fft_regs(int tid, cf* v, cf* s) {
    fc_step_first(tid, v, s);
    __syncthreads();
    fc_step_load<8>(tid, v, s);
    __syncthreads();
    fc_step_store<8>(tid, v, s);
    __syncthreads();
    fc_step_load<64>(tid, v, s);
    __syncthreads();
    fc_step_store<64>(tid, v, s);
    __syncthreads();
    fc_step_last(tid, v, s);
}

// the spectrum of the 2 P real samples packed in v -> out[P]
__device__ __forceinline__ void spectrum_out(int tid, cf* v, cf* s, cf* __restrict__ out) {
    fft_regs(tid, v, s);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) s[fc_pad(tid + FC_T * m)] = v[m];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = tid + FC_T * m;
        out[k] = fc_split(k, v[m], s[fc_pad((P - k) & (P - 1))]);
    }
}

// f(b): the filter of clip b, or -1 for a clip that passes through
__device__ __forceinline__ int filter_of(const int* __restrict__ h_index, int b, int NR) {
    const int f = h_index ? h_index[b] : (NR == 1 ? 0 : b);
    return (f < 0 || f >= NR) ? -1 : f;
}

// grid (npart, NR, 1 | 2)
__global__ void __launch_bounds__(FC_T) fftconv_prepare_kernel(const float* __restrict__ h, int NR, int R, int npart, const int* __restrict__ early_len,
                                                               cf* __restrict__ spec) {
    __shared__ cf s[FC_LDS];
    const int tid = threadIdx.x, j = blockIdx.x, r = blockIdx.y, early = blockIdx.z;
    int lim = R;
    if (early) lim = min(max(early_len[r], 0), R);
    const float* hr = h + (size_t)r * R;
    cf v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int n = 2 * (tid + FC_T * t);                            // sample of the 2 P window; the second half is zero
        const int g = j * P + n;                                       // < R + P: an int
        v[t].x = (n < P && g < lim) ? hr[g] : 0.0f;
        v[t].y = (n < P && g + 1 < lim) ? hr[g + 1] : 0.0f;
    }
    spectrum_out(tid, v, s, spec + ((size_t)(early * NR + r) * npart + j) * P);
}

// grid (B * nblk)
__global__ void __launch_bounds__(FC_T) fftconv_forward_kernel(const float* __restrict__ x, int L, int nblk, int NR, const int* __restrict__ h_index,
                                                               cf* __restrict__ ws) {
    __shared__ cf s[FC_LDS];
    const int tid = threadIdx.x, b = blockIdx.x / nblk, i = blockIdx.x - b * nblk;
    if (filter_of(h_index, b, NR) < 0) return;                         // workgroup-uniform
    const float* xb = x + (size_t)b * L;
    cf v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int g = (i - 1) * P + 2 * (tid + FC_T * t);              // in [-P, L + P): an int for L <= 2^30
        v[t].x = (g >= 0 && g < L) ? xb[g] : 0.0f;
        v[t].y = (g + 1 >= 0 && g + 1 < L) ? xb[g + 1] : 0.0f;
    }
    spectrum_out(tid, v, s, ws + (size_t)blockIdx.x * P);
}

// accumulated spectrum a (bin tid + 256 m) -> samples iP .. of yb, cut at L
__device__ __forceinline__ void block_out(int tid, cf* a, cf* s, float* __restrict__ yb, int i, int L) {
#pragma unroll
    for (int m = 0; m < 8; ++m) s[fc_pad(tid + FC_T * m)] = a[m];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = tid + FC_T * m;
        a[m] = fc_merge(k, a[m], s[fc_pad((P - k) & (P - 1))]);
    }
    __syncthreads();
    fft_regs(tid, a, s);
    // z[n] = conj(a) at n = tid + 256 m; the samples 2n, 2n + 1 of the window; its second half (m >= 4) is the block
#pragma unroll
    for (int m = 4; m < 8; ++m) {
        const int g = i * P + 2 * (tid + FC_T * (m - 4));              // < L + P
        if (g < L) yb[g] = a[m].x;
        if (g + 1 < L) yb[g + 1] = -a[m].y;
    }
}

// grid (B * nblk)
template <bool EARLY>
__global__ void __launch_bounds__(FC_T) fftconv_output_kernel(const float* __restrict__ x, int L, int nblk, int NR, int npart,
                                                              const int* __restrict__ h_index, const cf* __restrict__ spec, const cf* __restrict__ ws,
                                                              float* __restrict__ y, float* __restrict__ y_early) {
    __shared__ cf s[FC_LDS];
    const int tid = threadIdx.x, b = blockIdx.x / nblk, i = blockIdx.x - b * nblk;
    const int f = filter_of(h_index, b, NR);
    const size_t row = (size_t)b * L;
    if (f < 0) {                                                       // pass-through: the samples themselves
        for (int n = tid; n < P; n += FC_T) {
            const int g = i * P + n;
            if (g < L) {
                const float val = x[row + g];
                y[row + g] = val;
                if (EARLY) y_early[row + g] = val;
            }
        }
        return;
    }
    cf acc[8], acce[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) { acc[m] = {0.0f, 0.0f}; acce[m] = {0.0f, 0.0f}; }
    const int np = min(npart, i + 1);
    const cf* hp = spec + (size_t)f * npart * P;
    const cf* he = hp + (size_t)NR * npart * P;
    const cf* xp = ws + (size_t)blockIdx.x * P;                        // block i of clip b; block i - j lies j spectra below
    for (int j = 0; j < np; ++j) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int k = tid + FC_T * m;
            const cf xv = xp[k];
            fc_mac_bin(k, acc[m], xv, hp[k]);
            if (EARLY) fc_mac_bin(k, acce[m], xv, he[k]);
        }
        xp -= P; hp += P; he += P;
    }
    block_out(tid, acc, s, y + row, i, L);
    if (EARLY) {
        __syncthreads();
        block_out(tid, acce, s, y_early + row, i, L);
    }
}

// y[b] = x[b] / (max |ref[b]| + eps): one workgroup per clip, the maximum first (exact, order-free), then the scale snr_mix applies
__global__ void __launch_bounds__(256) peak_scale_kernel(const float* __restrict__ x, const float* __restrict__ ref, int L, float eps, float* __restrict__ y) {
    __shared__ float wmax[4];
    const size_t row = (size_t)blockIdx.x * L;
    float m = 0.0f;
    for (int n = threadIdx.x; n < L; n += 256) m = fmaxf(m, fabsf(ref[row + n]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    const float inv = 1.f / (fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])) + eps);
    for (int n = threadIdx.x; n < L; n += 256) y[row + n] = x[row + n] * inv;
}

int nparts(int n) { return (int)(((long long)n + P - 1) / P); }

}  // namespace

extern "C" size_t cruse_fftconv_spec_bytes(int NR, int R, int early) {
    if (NR < 1 || R < 1) return 0;
    return (size_t)(early ? 2 : 1) * (size_t)NR * (size_t)nparts(R) * SPEC_ONE;
}

extern "C" size_t cruse_fftconv_ws_bytes(int B, int L) {
    if (B < 1 || L < 1) return 0;
    return (size_t)B * (size_t)nparts(L) * SPEC_ONE;
}

extern "C" int cruse_fftconv_prepare(const float* h, int NR, int R, const int* early_len, void* spec, size_t spec_bytes, void* stream) {
    CRUSE_REQUIRE(h, CRUSE_E_SHAPE, "fftconv_prepare: h is null");
    CRUSE_REQUIRE(spec, CRUSE_E_SHAPE, "fftconv_prepare: spec is null");
    CRUSE_REQUIRE(NR >= 1 && R >= 1, CRUSE_E_SHAPE, "fftconv_prepare: NR = %d, R = %d", NR, R);
    CRUSE_REQUIRE(R <= MAX_L, CRUSE_E_SHAPE, "fftconv_prepare: R = %d > %d", R, MAX_L);
    const int npart = nparts(R);
    CRUSE_REQUIRE(NR <= 65535, CRUSE_E_SHAPE, "fftconv_prepare: NR = %d filters, at most 65535", NR);
    const size_t need = cruse_fftconv_spec_bytes(NR, R, early_len != nullptr);
    CRUSE_REQUIRE(spec_bytes >= need, CRUSE_E_SHAPE, "fftconv_prepare: spec_bytes = %zu, %zu needed", spec_bytes, need);
    CRUSE_REQUIRE(((uintptr_t)spec & 7) == 0, CRUSE_E_ALIGN, "fftconv_prepare: spec not 8-byte aligned");
    hipLaunchKernelGGL(fftconv_prepare_kernel, dim3(npart, NR, early_len ? 2 : 1), dim3(FC_T), 0, (hipStream_t)stream, h, NR, R, npart, early_len,
                       (cf*)spec);
    CRUSE_LAUNCH_CHECK("cruse_fftconv_prepare");
    return CRUSE_OK;
}

extern "C" int cruse_fftconv_apply(const float* x, int B, int L, const void* spec, size_t spec_bytes, int NR, int R, const int* h_index, void* ws,
                                   size_t ws_bytes, float* y, float* y_early, void* stream) {
    CRUSE_REQUIRE(x, CRUSE_E_SHAPE, "fftconv_apply: x is null");
    CRUSE_REQUIRE(spec, CRUSE_E_SHAPE, "fftconv_apply: spec is null");
    CRUSE_REQUIRE(ws, CRUSE_E_SHAPE, "fftconv_apply: ws is null");
    CRUSE_REQUIRE(y, CRUSE_E_SHAPE, "fftconv_apply: y is null");
    CRUSE_REQUIRE(B >= 1 && L >= 1 && NR >= 1 && R >= 1, CRUSE_E_SHAPE, "fftconv_apply: B = %d, L = %d, NR = %d, R = %d", B, L, NR, R);
    CRUSE_REQUIRE(L <= MAX_L && R <= MAX_L, CRUSE_E_SHAPE, "fftconv_apply: L = %d, R = %d, at most %d", L, R, MAX_L);
    CRUSE_REQUIRE(h_index || NR == 1 || NR == B, CRUSE_E_SHAPE, "fftconv_apply: NR = %d filters for B = %d clips need an h_index (NR = 1 or B without)", NR, B);
    const int nblk = nparts(L), npart = nparts(R);
    CRUSE_REQUIRE((long long)B * nblk <= 0x7fffffffLL, CRUSE_E_SHAPE, "fftconv_apply: B * blocks = %lld workgroups, at most 2^31 - 1", (long long)B * nblk);
    const size_t need_spec = cruse_fftconv_spec_bytes(NR, R, y_early != nullptr), need_ws = cruse_fftconv_ws_bytes(B, L);
    CRUSE_REQUIRE(spec_bytes >= need_spec, CRUSE_E_SHAPE, "fftconv_apply: spec_bytes = %zu, %zu needed%s", spec_bytes, need_spec,
                  y_early ? " (with the early spectra)" : "");
    CRUSE_REQUIRE(ws_bytes >= need_ws, CRUSE_E_SHAPE, "fftconv_apply: ws_bytes = %zu, %zu needed", ws_bytes, need_ws);
    CRUSE_REQUIRE((((uintptr_t)spec | (uintptr_t)ws) & 7) == 0, CRUSE_E_ALIGN, "fftconv_apply: spec / ws not 8-byte aligned");
    const dim3 grid((unsigned)((long long)B * nblk));
    hipLaunchKernelGGL(fftconv_forward_kernel, grid, dim3(FC_T), 0, (hipStream_t)stream, x, L, nblk, NR, h_index, (cf*)ws);
    CRUSE_LAUNCH_CHECK("cruse_fftconv_apply (forward)");
    if (y_early)
        hipLaunchKernelGGL(fftconv_output_kernel<true>, grid, dim3(FC_T), 0, (hipStream_t)stream, x, L, nblk, NR, npart, h_index, (const cf*)spec,
                           (const cf*)ws, y, y_early);
    else
        hipLaunchKernelGGL(fftconv_output_kernel<false>, grid, dim3(FC_T), 0, (hipStream_t)stream, x, L, nblk, NR, npart, h_index, (const cf*)spec,
                           (const cf*)ws, y, y_early);
    CRUSE_LAUNCH_CHECK("cruse_fftconv_apply (output)");
    return CRUSE_OK;
}

extern "C" int cruse_peak_scale(const float* x, const float* ref, int B, int L, float eps, float* y, void* stream) {
    CRUSE_REQUIRE(x && ref && y, CRUSE_E_SHAPE, "peak_scale: null buffer");
    CRUSE_REQUIRE(B >= 1 && L >= 1, CRUSE_E_SHAPE, "peak_scale: B = %d, L = %d", B, L);
    hipLaunchKernelGGL(peak_scale_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, ref, L, eps, y);
    CRUSE_LAUNCH_CHECK("cruse_peak_scale");
    return CRUSE_OK;
}
