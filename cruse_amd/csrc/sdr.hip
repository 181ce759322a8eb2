// bss_eval SDR of one source on the device (cruse_sdr): SDR of train_base/metrics.py:55-57, mir_eval.separation.bss_eval_sources for a
// single source, as DESIGN section 13g defines it.  For a clip of n samples and a filter of K taps:
//   raa[k] = sum_i ref[i] ref[i+k], rab[k] = sum_i ref[i] est[i+k]  (0 <= k < K, zero outside [0, n))
//   toeplitz(raa) C = rab;  s[m] = sum_k C[k] ref[m-k], e[m] = est[m] - s[m]  (0 <= m < n + K - 1);  10 log10(sum s^2 / sum e^2)
// f32 inputs; every product, sum, the solve and the projection in f64.  Every sum runs in an order that follows from n and K alone (never
// from B or the row length L), no atomics: a clip scores bit for bit the same alone, inside a batch, and from run to run.  No sample at an
// index >= n is loaded.  One call = four dependent launches on one stream, none of which the host waits for:
//   1 sdr_corr     grid (NC, ceil(K/256), B)   chunk c of CHUNK samples (+ K of look-ahead) of ref and est in LDS, one lag per thread:
//                                              part[b][c][2][K] f64.  A chunk at or beyond n leaves at once; its partials are never read
//   2 sdr_solve    grid (B)                    sums the chunk partials in ascending chunk order, then Levinson's recursion with every
//                                              vector in LDS: C[b][K], status[b] (1: r[0] or a prediction error not positive, n = 0)
//   3 sdr_project  grid (NT, B)                tile t of TILE outputs: C (f64) and the ref window in LDS, 8 outputs per thread, taps in
//                                              ascending order; the tile's sums of s^2 and e^2 by a fixed tree: en[b][t][2]
//   4 sdr_score    grid (B)                    sums the tile partials in ascending order, the log, NaN where status != 0; the dbg copy
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = CRUSE_SDR_CHUNK;            // samples of a correlation chunk and outputs of a projection tile
constexpr int TILE = CHUNK;
constexpr int PT = TILE / THREADS;                // outputs a thread of sdr_project holds
constexpr int MAXK = CRUSE_SDR_MAX_TAPS;
constexpr int MAX_L = 1 << 28;                    // n + K - 1 < 2^31
constexpr int MAX_B = 65535;                      // gridDim.y / .z
static_assert(TILE % THREADS == 0, "a tile is a whole number of outputs per thread");

// the workspace, in 8-byte units: part [B][NC][2][K] f64 | C [B][K] f64 | en [B][NT][2] f64 | status [B] int (padded to 8 bytes)
struct SdrLayout { int NC, NT; size_t part, c, en, status, total; };

int make_layout(const char* who, int B, int L, int K, SdrLayout& Y) {
    CRUSE_REQUIRE(B >= 1 && L >= 1 && K >= 1, CRUSE_E_SHAPE, "%s: B = %d, L = %d, K = %d", who, B, L, K);
    CRUSE_REQUIRE(B <= MAX_B && L <= MAX_L && K <= MAXK, CRUSE_E_SHAPE, "%s: B = %d > %d, L = %d > %d or K = %d > %d", who, B, MAX_B, L, MAX_L,
                  K, MAXK);
    Y.NC = cdiv(L, CHUNK);
    Y.NT = cdiv(L + K - 1, TILE);
    size_t o = 0;
    Y.part = o; o += (size_t)B * Y.NC * 2 * K;
    Y.c = o;    o += (size_t)B * K;
    Y.en = o;   o += (size_t)B * Y.NT * 2;
    Y.status = o; o += ((size_t)B + 1) / 2;
    Y.total = o;
    return CRUSE_OK;
}

__device__ __forceinline__ int clip_len(const int* __restrict__ len, int b, int L) { return len ? min(max(len[b], 0), L) : L; }

// sums of a and b over the workgroup in a fixed tree; valid in every thread.  red: 2 * THREADS doubles
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = a;
    red[THREADS + tid] = b;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            red[THREADS + tid] += red[THREADS + tid + o];
        }
        __syncthreads();
    }
    a = red[0];
    b = red[THREADS];
}

// ---- 1: lagged correlations of one chunk -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) sdr_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                           const int* __restrict__ len, int Lrow, int K, SdrLayout Y, double* __restrict__ ws) {
    __shared__ float sr[CHUNK + MAXK];
    __shared__ float se[CHUNK + MAXK];
    const int c = blockIdx.x, b = blockIdx.z, tid = threadIdx.x;
    const int n = clip_len(len, b, Lrow);
    const int c0 = c * CHUNK;
    if (c0 >= n) return;
    const float* r = ref + (size_t)b * Lrow;
    const float* e = est + (size_t)b * Lrow;
    for (int i = tid; i < CHUNK + K; i += THREADS) {                   // c0 + i < n <= Lrow: nothing beyond the clip is loaded
        const bool in = c0 + i < n;
        sr[i] = in ? r[c0 + i] : 0.f;
        se[i] = in ? e[c0 + i] : 0.f;
    }
    __syncthreads();
    const int k = blockIdx.y * THREADS + tid;
    const int kk = min(k, K - 1);                                      // a thread past the last lag reads inside the arrays, writes nothing
    const int m = min(CHUNK, n - c0);                                  // i + kk <= CHUNK - 1 + K - 1
    double aa = 0.0, ab = 0.0;
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
        const double x = (double)sr[i];
        aa = fma(x, (double)sr[i + kk], aa);
        ab = fma(x, (double)se[i + kk], ab);
    }
    if (k < K) {
        double* p = ws + Y.part + ((size_t)b * Y.NC + c) * 2 * K;
        p[k] = aa;
        p[K + k] = ab;
    }
}

// ---- 2: chunk sums and the Toeplitz solve ------------------------------------------------------------------------------------------
// Levinson: a = the order-m forward predictor (a[0] = 1), E its error, x the solution of the leading (m x m) system.  Step m:
//   k = -(r[m] + sum_{j=1}^{m-1} a[j] r[m-j]) / E;  a[j] += k a[m-j] (pairs j, m-j updated together), a[m] = k;  E *= 1 - k^2
//   lambda = (d[m] - sum_{j=0}^{m-1} x[j] r[m-j]) / E;  x[j] += lambda a[m-j], x[m] = lambda
__global__ void __launch_bounds__(THREADS) sdr_solve_kernel(const int* __restrict__ len, int Lrow, int K, SdrLayout Y, double* __restrict__ ws,
                                                            double* __restrict__ dbg) {
    __shared__ double r[MAXK], d[MAXK], a[MAXK], x[MAXK];
    __shared__ double red[2 * THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clip_len(len, b, Lrow);
    const int nc = (n + CHUNK - 1) / CHUNK;
    const double* part = ws + Y.part + (size_t)b * Y.NC * 2 * K;
    for (int k = tid; k < K; k += THREADS) {
        double aa = 0.0, ab = 0.0;
        for (int c = 0; c < nc; ++c) {
            aa += part[(size_t)c * 2 * K + k];
            ab += part[(size_t)c * 2 * K + K + k];
        }
        r[k] = aa;
        d[k] = ab;
        a[k] = 0.0;
        x[k] = 0.0;
    }
    __syncthreads();
    double E = r[0];
    bool ok = E > 0.0;                                                 // uniform: every thread reads the same E (NaN is not > 0)
    if (ok && tid == 0) {
        a[0] = 1.0;
        x[0] = d[0] / E;
    }
    __syncthreads();
    for (int m = 1; m < K && ok; ++m) {
        double sa = 0.0, sx = 0.0;
        for (int j = tid; j < m; j += THREADS) {
            const double rr = r[m - j];
            sa = fma(a[j], rr, sa);                                    // j = 0: a[0] r[m]
            sx = fma(x[j], rr, sx);
        }
        block_sum2(sa, sx, red);
        const double kr = -sa / E;
        const double En = E * (1.0 - kr * kr);
        ok = En > 0.0;
        if (!ok) break;                                                // uniform
        for (int j = 1 + tid; 2 * j <= m - 1; j += THREADS) {          // the pairs (j, m - j), j < m - j
            const double u = a[j], v = a[m - j];
            a[j] = fma(kr, v, u);
            a[m - j] = fma(kr, u, v);
        }
        if (tid == 0) {
            if ((m & 1) == 0) a[m / 2] = fma(kr, a[m / 2], a[m / 2]);  // the middle one pairs with itself
            a[m] = kr;
        }
        E = En;
        __syncthreads();
        const double lam = (d[m] - sx) / E;
        for (int j = tid; j < m; j += THREADS) x[j] = fma(lam, a[m - j], x[j]);
        if (tid == 0) x[m] = lam;
        __syncthreads();
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* C = ws + Y.c + (size_t)b * K;
    for (int k = tid; k < K; k += THREADS) C[k] = ok ? x[k] : nan;
    if (tid == 0) ((int*)(ws + Y.status))[b] = ok ? 0 : 1;
    if (dbg) {
        double* g = dbg + (size_t)b * (3 * (size_t)K + 2);
        for (int k = tid; k < K; k += THREADS) {
            g[k] = r[k];
            g[K + k] = d[k];
            g[2 * K + k] = ok ? x[k] : nan;
        }
    }
}

// ---- 3: projection and energies of one tile ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) sdr_project_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                              const int* __restrict__ len, int Lrow, int K, SdrLayout Y, double* __restrict__ ws) {
    __shared__ double C[MAXK];
    __shared__ float sr[TILE + MAXK];                                  // sr[i] = ref[m0 - (K - 1) + i]
    __shared__ double red[2 * THREADS];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = clip_len(len, b, Lrow);
    const int m0 = t * TILE;
    if (n == 0 || m0 >= n + K - 1) return;                             // tiles beyond the clip's n + K - 1 outputs are never read
    if (((const int*)(ws + Y.status))[b] != 0) return;                 // no solution: the score is NaN whatever is here
    const float* r = ref + (size_t)b * Lrow;
    const float* e = est + (size_t)b * Lrow;
    for (int k = tid; k < K; k += THREADS) C[k] = ws[Y.c + (size_t)b * K + k];
    const int base = m0 - (K - 1);
    for (int i = tid; i < TILE + K - 1; i += THREADS) {
        const int g = base + i;
        sr[i] = (g >= 0 && g < n) ? r[g] : 0.f;
    }
    __syncthreads();
    double acc[PT];
#pragma unroll
    for (int q = 0; q < PT; ++q) acc[q] = 0.0;
    for (int k = 0; k < K; ++k) {                                      // s[m] += C[k] ref[m - k]; sr index m - k - base = (m - m0) + K - 1 - k
        const double c = C[k];
        const float* w = sr + (K - 1 - k) + tid;
#pragma unroll
        for (int q = 0; q < PT; ++q) acc[q] = fma(c, (double)w[q * THREADS], acc[q]);
    }
    double ss = 0.0, ee = 0.0;
#pragma unroll
    for (int q = 0; q < PT; ++q) {
        const int m = m0 + q * THREADS + tid;
        if (m < n + K - 1) {
            const double y = m < n ? (double)e[m] : 0.0;
            const double dlt = y - acc[q];
            ss = fma(acc[q], acc[q], ss);
            ee = fma(dlt, dlt, ee);
        }
    }
    block_sum2(ss, ee, red);
    if (tid == 0) {
        double* p = ws + Y.en + ((size_t)b * Y.NT + t) * 2;
        p[0] = ss;
        p[1] = ee;
    }
}

// ---- 4: the score ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) sdr_score_kernel(const int* __restrict__ len, int Lrow, int K, SdrLayout Y, const double* __restrict__ ws,
                                                       float* __restrict__ out, double* __restrict__ dbg) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int n = clip_len(len, b, Lrow);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double ss = nan, ee = nan;
    if (n > 0 && ((const int*)(ws + Y.status))[b] == 0) {
        const int nt = (n + K - 1 + TILE - 1) / TILE;
        const double* p = ws + Y.en + (size_t)b * Y.NT * 2;
        ss = 0.0;
        ee = 0.0;
        for (int t = 0; t < nt; ++t) {
            ss += p[2 * t];
            ee += p[2 * t + 1];
        }
    }
    out[b] = (float)(10.0 * log10(ss / ee));                           // NaN stays NaN; ee = 0 with ss > 0 is +inf, as numpy
    if (dbg) {
        double* g = dbg + (size_t)b * (3 * (size_t)K + 2) + 3 * (size_t)K;
        g[0] = ss;
        g[1] = ee;
    }
}

}  // namespace

extern "C" size_t cruse_sdr_ws_bytes(int B, int L, int K) {
    SdrLayout Y;
    return make_layout("sdr_ws_bytes", B, L, K, Y) ? 0 : Y.total * 8;
}

extern "C" int cruse_sdr(const float* ref, const float* est, const int* len, int B, int L, int K, void* ws, float* out, double* dbg,
                         void* stream) {
    CRUSE_REQUIRE(ref && est && ws && out, CRUSE_E_SHAPE, "sdr: null buffer");
    SdrLayout Y;
    const int rc = make_layout("sdr", B, L, K, Y);
    if (rc) return rc;
    CRUSE_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)dbg & 7) == 0, CRUSE_E_ALIGN, "sdr: workspace or dbg not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* w = (double*)ws;
    hipLaunchKernelGGL(sdr_corr_kernel, dim3(Y.NC, cdiv(K, THREADS), B), dim3(THREADS), 0, s, ref, est, len, L, K, Y, w);
    CRUSE_LAUNCH_CHECK("cruse_sdr (correlation)");
    hipLaunchKernelGGL(sdr_solve_kernel, dim3(B), dim3(THREADS), 0, s, len, L, K, Y, w, dbg);
    CRUSE_LAUNCH_CHECK("cruse_sdr (solve)");
    hipLaunchKernelGGL(sdr_project_kernel, dim3(Y.NT, B), dim3(THREADS), 0, s, ref, est, len, L, K, Y, w);
    CRUSE_LAUNCH_CHECK("cruse_sdr (projection)");
    hipLaunchKernelGGL(sdr_score_kernel, dim3(B), dim3(64), 0, s, len, L, K, Y, (const double*)w, out, dbg);
    CRUSE_LAUNCH_CHECK("cruse_sdr (score)");
    return CRUSE_OK;
}
