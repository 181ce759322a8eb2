// DeepFilterNet's two normalised input features (cruse_df_feat): the ERB feature (log band power minus its
// exponential mean, test/test_erb.py:97-106 with the repair out = (x - state) / 40) and the complex feature (the lowest nb_df bins over
// the root of their exponentially smoothed magnitude, ExponentialUnitNorm.forward, test/test_norm.py:52-61).  Both are first-order
// recurrences along time per clip and column; the states go in and out, so frame-by-frame calls give the bits of one offline call.
//
// Parallel over clips and columns, sequential along time.  One workgroup of 256 lanes owns a clip and up to 64 columns (bands, or bins
// of the complex feature) and walks the clip in tiles of TC = 64 frames:
//   1 all four waves compute what does not depend on the chain, u[t][c] = (1 - alpha) * e[t][c] (ERB: e = 10 log10(mean band power +
//     log_eps), one lane per (frame, band), the band's bins added in ascending order; unit norm: e = sqrt(max(re^2 + im^2, unit_eps)),
//     a wave per frame, lanes on consecutive bins), every load of the tile issued before the first use, and stage u in LDS
//   2 wave 0, a lane per column, walks the chain  s <- fma(alpha, s, u[t][c])  over the tile's frames and leaves s[t][c] where u was
//   3 all four waves write the outputs from s[t][c]: (e - m) / erb_scale, or (re, im) / sqrt(s) with re, im still in registers
// The state stays in wave 0's registers between tiles.  Every value is one fixed f32 expression of the incoming state and the frames up
// to its own (no contraction is left to the compiler, sqrt and division are the correctly rounded ones), and which lane computes a
// frame does not enter it: any split of the frames over calls gives the same bits.  No atomics, no workspace, plain vector stores.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TC = CRUSE_DF_FEAT_TC, COLS = 64;                      // frames of a tile, columns of a workgroup
constexpr int KF = TC / WAVES;                                     // frames of a tile per wave (unit norm)
static_assert(TC % WAVES == 0 && COLS == 64, "a wave per frame, a lane per column");

struct DfFeatArgs {
    const float* re; const float* im; long long es, fs;            // element strides between bins and between frames
    int T, F;
    const int* starts; int nb_erb, nb_df, erb_jobs, jobs;
    float alpha, oma, log_eps, erb_scale, unit_eps;
    float* erb_state; float* unit_state; float* feat_erb; float* feat_spec;
};

__device__ __forceinline__ float power(float re, float im) { return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)); }

// wave 0: the chain over the tile's n frames, s[t][c] left where u[t][c] was
__device__ __forceinline__ void walk(float* u, int n, int lane, float alpha, float& s) {
#pragma unroll 8
    for (int t = 0; t < n; ++t) {
        s = fmaf(alpha, s, u[t * COLS + lane]);
        u[t * COLS + lane] = s;
    }
}

__global__ void __launch_bounds__(THREADS) df_feat_kernel(const DfFeatArgs a) {
    __shared__ float u[TC * COLS];                                 // (1 - alpha) e, then the state, [frame of the tile][column]
    __shared__ float ev[TC * COLS];                                // ERB: e itself, for the output
    __shared__ int blo[COLS], bw[COLS];                            // ERB: first bin and width of the workgroup's bands
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / a.jobs, job = blockIdx.x % a.jobs;
    const size_t clip = (size_t)b * a.T;                           // frame index of the clip's first frame
    const int T = a.T;

    if (job < a.erb_jobs) {
        // ---------------------------------------------------------------- ERB feature: bands j0 .. j0 + nc
        const int j0 = job * COLS, nc = min(COLS, a.nb_erb - j0);
        if (tid < nc) {                                            // every entry clamped into [0, F]: no load leaves a row
            const int lo = min(max(a.starts[j0 + tid], 0), a.F), hi = min(max(a.starts[j0 + tid + 1], lo), a.F);
            blo[tid] = lo;
            bw[tid] = hi - lo;
        }
        float m = 0.0f;
        if (wv == 0 && lane < nc) m = a.erb_state[(size_t)b * a.nb_erb + j0 + lane];
        __syncthreads();
        for (int t0 = 0; t0 < T; t0 += TC) {
            const int n = min(TC, T - t0);
            for (int i = tid; i < n * nc; i += THREADS) {
                const int tl = i / nc, c = i - tl * nc, lo = blo[c], w = bw[c];
                const size_t row = (size_t)((clip + t0 + tl) * a.fs);
                const float* pr = a.re + row + (size_t)lo * a.es;
                const float* pi = a.im + row + (size_t)lo * a.es;
                float acc = 0.0f;
#pragma unroll 4
                for (int k = 0; k < w; ++k) acc = __fadd_rn(acc, power(pr[(size_t)k * a.es], pi[(size_t)k * a.es]));
                const float mean = w > 0 ? __fmul_rn(acc, __fdiv_rn(1.0f, (float)w)) : 0.0f;
                const float e = __fmul_rn(10.0f, log10f(__fadd_rn(mean, a.log_eps)));
                ev[tl * COLS + c] = e;
                u[tl * COLS + c] = __fmul_rn(e, a.oma);
            }
            __syncthreads();
            if (wv == 0 && lane < nc) walk(u, n, lane, a.alpha, m);
            __syncthreads();
            for (int i = tid; i < n * nc; i += THREADS) {
                const int tl = i / nc, c = i - tl * nc;
                a.feat_erb[(clip + t0 + tl) * a.nb_erb + j0 + c] = __fdiv_rn(__fsub_rn(ev[tl * COLS + c], u[tl * COLS + c]), a.erb_scale);
            }
            __syncthreads();
        }
        if (wv == 0 && lane < nc) a.erb_state[(size_t)b * a.nb_erb + j0 + lane] = m;
        return;
    }

    // -------------------------------------------------------------------- complex feature: bins f0 .. f0 + 64
    const int f = (job - a.erb_jobs) * COLS + lane;
    const bool live = f < a.nb_df;
    float s = 0.0f;
    if (wv == 0 && live) s = a.unit_state[(size_t)b * a.nb_df + f];
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int n = min(TC, T - t0);
        float re[KF], im[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) {                             // frame wv + WAVES k of the tile: 2 KF loads in flight per lane
            const int tl = wv + WAVES * k;
            const bool in = live && tl < n;
            const size_t at = (size_t)((clip + t0 + (in ? tl : 0)) * a.fs) + (size_t)(in ? f : 0) * a.es;
            re[k] = in ? a.re[at] : 0.0f;
            im[k] = in ? a.im[at] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < KF; ++k)
            u[(wv + WAVES * k) * COLS + lane] = __fmul_rn(__fsqrt_rn(fmaxf(power(re[k], im[k]), a.unit_eps)), a.oma);
        __syncthreads();
        if (wv == 0) walk(u, n, lane, a.alpha, s);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            const int tl = wv + WAVES * k;
            if (live && tl < n) {
                const float q = __fsqrt_rn(u[tl * COLS + lane]);
                float2 o;
                o.x = __fdiv_rn(re[k], q);
                o.y = __fdiv_rn(im[k], q);
                reinterpret_cast<float2*>(a.feat_spec)[(clip + t0 + tl) * a.nb_df + f] = o;
            }
        }
        __syncthreads();
    }
    if (wv == 0 && live) a.unit_state[(size_t)b * a.nb_df + f] = s;
}

}  // namespace

extern "C" int cruse_df_feat(const float* re, const float* im, long long bin_stride, long long frame_stride, int B, int T, int F,
                             const int* starts, int nb_erb, int nb_df, double alpha, float log_eps, float erb_scale, float unit_eps,
                             float* erb_state, float* unit_state, float* feat_erb, float* feat_spec, void* stream) {
    CRUSE_REQUIRE(B >= 1 && T >= 0 && F >= 1 && F <= CRUSE_BAND_MAX_F, CRUSE_E_SHAPE, "df_feat: B = %d, T = %d, F = %d (F at most %d)", B, T, F,
                  CRUSE_BAND_MAX_F);
    CRUSE_REQUIRE(nb_erb >= 0 && nb_erb <= F, CRUSE_E_SHAPE, "df_feat: nb_erb = %d outside 0..F = %d", nb_erb, F);
    CRUSE_REQUIRE(nb_df >= 0 && nb_df <= F, CRUSE_E_SHAPE, "df_feat: nb_df = %d outside 0..F = %d", nb_df, F);
    CRUSE_REQUIRE(nb_erb > 0 || nb_df > 0, CRUSE_E_SHAPE, "df_feat: nb_erb = 0 and nb_df = 0, no output is requested");
    CRUSE_REQUIRE(alpha >= 0.0 && alpha < 1.0, CRUSE_E_SHAPE, "df_feat: alpha = %g outside [0, 1)", alpha);
    CRUSE_REQUIRE(log_eps >= 0.0f && unit_eps >= 0.0f && erb_scale != 0.0f && erb_scale == erb_scale, CRUSE_E_SHAPE,
                  "df_feat: log_eps = %g and unit_eps = %g must be >= 0, erb_scale = %g non-zero", (double)log_eps, (double)unit_eps,
                  (double)erb_scale);
    CRUSE_REQUIRE(re && im, CRUSE_E_SHAPE, "df_feat: null spectrum (re %p, im %p)", (const void*)re, (const void*)im);
    CRUSE_REQUIRE(nb_erb == 0 || (starts && erb_state && feat_erb), CRUSE_E_SHAPE,
                  "df_feat: nb_erb = %d needs starts, erb_state and feat_erb (got %p, %p, %p)", nb_erb, (const void*)starts, (void*)erb_state,
                  (void*)feat_erb);
    CRUSE_REQUIRE(nb_df == 0 || (unit_state && feat_spec), CRUSE_E_SHAPE, "df_feat: nb_df = %d needs unit_state and feat_spec (got %p, %p)", nb_df,
                  (void*)unit_state, (void*)feat_spec);
    CRUSE_REQUIRE(bin_stride >= 1 && bin_stride <= (1 << 20), CRUSE_E_SHAPE, "df_feat: bin_stride = %lld outside 1..2^20", bin_stride);
    CRUSE_REQUIRE(frame_stride >= (long long)(F - 1) * bin_stride + 1 && frame_stride <= (1LL << 40), CRUSE_E_SHAPE,
                  "df_feat: frame_stride = %lld, F = %d bins %lld elements apart need at least %lld", frame_stride, F, bin_stride,
                  (long long)(F - 1) * bin_stride + 1);
    CRUSE_REQUIRE((long long)B * T <= (1LL << 31), CRUSE_E_SHAPE, "df_feat: B * T = %lld frames, at most 2^31", (long long)B * T);
    CRUSE_REQUIRE(nb_df == 0 || ((uintptr_t)feat_spec & 7) == 0, CRUSE_E_ALIGN, "df_feat: feat_spec not 8-byte aligned");
    if (T == 0) return CRUSE_OK;                                       // nothing written, the states stay
    DfFeatArgs a;
    a.re = re; a.im = im; a.es = bin_stride; a.fs = frame_stride;
    a.T = T; a.F = F;
    a.starts = starts; a.nb_erb = nb_erb; a.nb_df = nb_df;
    a.erb_jobs = cdiv(nb_erb, COLS);
    a.jobs = a.erb_jobs + cdiv(nb_df, COLS);
    a.alpha = (float)alpha; a.oma = (float)(1.0 - alpha);        // both rounded from the double, as torch rounds test_norm.py:59's Python scalars
    a.log_eps = log_eps; a.erb_scale = erb_scale; a.unit_eps = unit_eps;
    a.erb_state = erb_state; a.unit_state = unit_state; a.feat_erb = feat_erb; a.feat_spec = feat_spec;
    CRUSE_REQUIRE((long long)B * a.jobs <= 2147483647LL, CRUSE_E_SHAPE, "df_feat: B = %d clips of %d workgroups exceed the grid", B, a.jobs);
    hipLaunchKernelGGL(df_feat_kernel, dim3((unsigned)(B * a.jobs)), dim3(THREADS), 0, (hipStream_t)stream, a);
    CRUSE_LAUNCH_CHECK("cruse_df_feat");
    return CRUSE_OK;
}
