// The FFT under cruse_fftconv_* (fftconv.hip) as per-lane steps: a complex transform of FC_N = CRUSE_FFTCONV_PART
// points held 8 per lane by a workgroup of 256 lanes, radix 8 * 8 * 8 * 4 (Stockham autosort: every pass reads stride FC_N / radix,
// writes its butterflies side by side, and the last pass leaves natural order), and the split / merge passes that make it the
// transform of 2 FC_N real samples.  f32 throughout; twiddles come from sincospif of an exact rational argument.  Every sum of
// products is written with fmaf, so no contraction is left to the compiler and two instantiations round alike.
// The steps take the lane index as an argument and touch LDS only through `s`, so a host program can run them lane by lane,
// step by step (a barrier = finishing the loop over lanes); the kernels call them with __syncthreads() between.
#pragma once
#include <math.h>
#include "../../include/cruse_hip.h"

#ifdef __HIPCC__
#define FC_HD __host__ __device__ __forceinline__
#else
#define FC_HD inline
#endif

struct cf { float x, y; };

constexpr int FC_N = CRUSE_FFTCONV_PART;   // complex points of one transform = real samples of one partition
constexpr int FC_T = 256;                  // lanes of a workgroup, 8 points each
constexpr int FC_LDS = FC_N + FC_N / 32;   // cf elements of the padded image
static_assert(FC_N == 2048, "the radix plan 8 * 8 * 8 * 4 and 8 points per lane are written for 2048 points");

// image index of point i: one cf of padding after every 32, so that a pass that writes its 8 results 8 * NS apart (NS = 1: lanes 8
// points apart) spreads a 32-lane group of 8-byte accesses over all 64 banks
FC_HD int fc_pad(int i) { return i + (i >> 5); }

FC_HD cf fc_mul(cf a, cf b) { return {fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)}; }
// a += x * h
FC_HD void fc_mac(cf& a, cf x, cf h) {
    a.x = fmaf(x.x, h.x, fmaf(-x.y, h.y, a.x));
    a.y = fmaf(x.x, h.y, fmaf(x.y, h.x, a.y));
}

// exp(-2 pi i num / den), den a power of two: the argument of sincospif is exact
FC_HD cf fc_twid(int num, int den) {
    const float a = (float)(-2 * num) / (float)den;
#ifdef __HIP_DEVICE_COMPILE__
    float s, c;
    sincospif(a, &s, &c);
    return {c, s};
#else
    return {(float)cos(M_PI * (double)a), (float)sin(M_PI * (double)a)};
#endif
}

FC_HD void fc_fft2(cf& a, cf& b) {
    const cf t = a;
    a = {t.x + b.x, t.y + b.y};
    b = {t.x - b.x, t.y - b.y};
}
// X[k] of the 4 points ends in a[{0, 2, 1, 3}[k]]
FC_HD void fc_fft4(cf& a0, cf& a1, cf& a2, cf& a3) {
    fc_fft2(a0, a2);
    fc_fft2(a1, a3);
    a3 = {a3.y, -a3.x};                                                // * -i
    fc_fft2(a0, a1);
    fc_fft2(a2, a3);
}
// X[k] of the 8 points ends in v[bit reversal of k]
FC_HD void fc_fft8(cf* v) {
    constexpr float h = 0.70710678118654752440f;
    fc_fft2(v[0], v[4]);
    fc_fft2(v[1], v[5]);
    fc_fft2(v[2], v[6]);
    fc_fft2(v[3], v[7]);
    v[5] = {(v[5].x + v[5].y) * h, (v[5].y - v[5].x) * h};             // * (1 - i) / sqrt 2
    v[6] = {v[6].y, -v[6].x};                                          // * -i
    v[7] = {(v[7].y - v[7].x) * h, -(v[7].x + v[7].y) * h};            // * (-1 - i) / sqrt 2
    fc_fft4(v[0], v[1], v[2], v[3]);
    fc_fft4(v[4], v[5], v[6], v[7]);
}

// a radix-8 pass in registers: v[t] = point j + 256 t of the pass's input; NS = the product of the radices before it
template <int NS>
FC_HD void fc_pass8(int j, cf* v) {
    if (NS > 1) {
        const int r = j & (NS - 1);
#pragma unroll
        for (int t = 1; t < 8; ++t) v[t] = fc_mul(v[t], fc_twid(r * t, NS * 8));
    }
    fc_fft8(v);
}
template <int NS>
FC_HD void fc_store8(int j, const cf* v, cf* s) {
    const int base = (j / NS) * NS * 8 + (j & (NS - 1));
    s[fc_pad(base + 0 * NS)] = v[0];
    s[fc_pad(base + 1 * NS)] = v[4];
    s[fc_pad(base + 2 * NS)] = v[2];
    s[fc_pad(base + 3 * NS)] = v[6];
    s[fc_pad(base + 4 * NS)] = v[1];
    s[fc_pad(base + 5 * NS)] = v[5];
    s[fc_pad(base + 6 * NS)] = v[3];
    s[fc_pad(base + 7 * NS)] = v[7];
}
FC_HD void fc_load8(int j, cf* v, const cf* s) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = s[fc_pad(j + FC_T * t)];
}

// the steps of one transform; a barrier stands between two of them.  In: v[t] = point tid + 256 t.  Out (after fc_step_last):
// v[m] = X[tid + 256 m].
FC_HD void fc_step_first(int tid, cf* v, cf* s) { fc_pass8<1>(tid, v); fc_store8<1>(tid, v, s); }
template <int NS>
FC_HD void fc_step_load(int tid, cf* v, const cf* s) { fc_load8(tid, v, s); fc_pass8<NS>(tid, v); }
template <int NS>
FC_HD void fc_step_store(int tid, const cf* v, cf* s) { fc_store8<NS>(tid, v, s); }
// the radix-4 pass (NS = 512): lane tid runs butterflies j = tid and tid + 256 on points j + 512 t = tid + 256 (u + 2 t)
FC_HD void fc_step_last(int tid, cf* v, const cf* s) {
    fc_load8(tid, v, s);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = tid + FC_T * u;
        cf a0 = v[u], a1 = fc_mul(v[u + 2], fc_twid(j, FC_N)), a2 = fc_mul(v[u + 4], fc_twid(2 * j, FC_N)), a3 = fc_mul(v[u + 6], fc_twid(3 * j, FC_N));
        fc_fft4(a0, a1, a2, a3);
        v[u] = a0; v[u + 2] = a2; v[u + 4] = a1; v[u + 6] = a3;
    }
}

// Z = the transform of z[n] = x[2n] + i x[2n+1]  ->  bin k of the transform X of the 2 FC_N real samples, from Z[k] and Z[FC_N - k].
// Bin 0 carries (X[0], X[FC_N]), both real.
FC_HD cf fc_split(int k, cf zk, cf zm) {
    if (k == 0) return {zk.x + zk.y, zk.x - zk.y};
    const cf e = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const cf o = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    const cf w = fc_twid(k, 2 * FC_N);
    return {e.x + fmaf(w.x, o.x, -(w.y * o.y)), e.y + fmaf(w.x, o.y, w.y * o.x)};
}
// the way back: conj(Z[k]) / (2 FC_N) from Y[k] and Y[FC_N - k]; the forward transform of these, conjugated, is z
FC_HD cf fc_merge(int k, cf yk, cf ym) {
    constexpr float sc = 0.5f / (float)FC_N;
    if (k == 0) return {(yk.x + yk.y) * sc, -(yk.x - yk.y) * sc};
    const cf e = {yk.x + ym.x, yk.y - ym.y};
    const cf d = {yk.x - ym.x, yk.y + ym.y};
    const cf w = fc_twid(k, 2 * FC_N);                                  // o = d * conj(w)
    const cf o = {fmaf(d.x, w.x, d.y * w.y), fmaf(d.y, w.x, -(d.x * w.y))};
    return {(e.x - o.y) * sc, -(e.y + o.x) * sc};
}
// product of two packed spectra at bin k, added to a
FC_HD void fc_mac_bin(int k, cf& a, cf x, cf h) {
    if (k == 0) { a.x = fmaf(x.x, h.x, a.x); a.y = fmaf(x.y, h.y, a.y); }
    else fc_mac(a, x, h);
}
