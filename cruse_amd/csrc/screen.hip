// Per-file statistics of a flat f32 pool of recordings (cruse_screen_clips, cruse_rt60): what the reference's list
// builder (dataset/preprocess_dataset.py) needs to reject a file -- peak and clipped samples (feature.is_clipped), level
// (feature.tailor_dB_FS), the DNS-Challenge activity fraction (feature.activity_detector) and a reverberation time from the Schroeder
// integral of an impulse response (the quantity utils.cal_rt60 aims at).  Utterance i is pool[start[i] .. start[i] + len[i]); start is
// arbitrary, nothing outside an utterance is ever loaded, every sum is f64 in one fixed order, no atomics.
//
// cruse_screen_clips, two launches:
//   window pass   the grid runs over the flat list of analysis windows (win_first = exclusive prefix of ceil(len / window)); ONE
//                 WAVEFRONT per window reads its samples once (16-byte loads over the aligned middle, scalar loads for the head and
//                 the tail) and leaves one 16-byte row of ws: sum x^2 (f64), max |x|, #{|x| > clip_thr}
//   finish pass   one workgroup per utterance adds its rows (thread-strided, then a fixed tree), forms rms and the scale to target_db,
//                 and evaluates the detector per window from the rows of that window and the one before it
// cruse_rt60, one launch, one workgroup per response: the peak, the chunk sums of h^2 from the peak on, their suffixes, then two sweeps
// that rebuild E[t] chunk by chunk with the same instructions (so both see the same bits): the counts of D > lo_db / hi_db, and the
// regression sums over [t_lo, t_hi).
#include <math.h>
#include "common.h"

namespace {

constexpr int SCREEN_THREADS = 256;
constexpr int SCREEN_WPB = SCREEN_THREADS / 64;            // windows per workgroup of the window pass: one per wavefront
constexpr long long SCREEN_MAX_WINDOWS = CRUSE_SCREEN_MAX_WINDOWS;
constexpr int SCREEN_MAX_WINDOW = 1 << 30;

struct WinRow {
    double s;      // sum of x^2 over the window
    float peak;    // max |x| (NaN if the window holds one)
    int nclip;     // #{|x| > clip_thr}
};
static_assert(sizeof(WinRow) == CRUSE_SCREEN_WS_ROW, "window row size");

struct ScreenArgs {
    const float* pool;
    const long long* start;
    const long long* len;
    const long long* win_first;    // [n + 1]
    int n;
    long long total;
    int window;
    float clip_thr;
    double target_db, act_thr;
    WinRow* ws;
    double* out;                   // [n][6]
};

// max that keeps a NaN once it has one (fmaxf would drop it: a read outside an utterance has to show)
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

struct WinAcc {
    double s;
    float pk;
    int nc;
    __device__ __forceinline__ void take(float v, float thr) {
        const float av = fabsf(v);
        s += (double)v * (double)v;                       // exact product, f64 sum
        pk = max_nan(pk, av);
        nc += av > thr ? 1 : 0;
    }
};

__global__ void __launch_bounds__(SCREEN_THREADS) screen_window_kernel(ScreenArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SCREEN_WPB + (threadIdx.x >> 6);
    if (w >= a.total) return;                             // whole wavefronts leave together
    int lo = 0, hi = a.n;                                 // win_first[lo] <= w < win_first[hi]; empty utterances repeat an entry
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.win_first[mid] <= w) lo = mid; else hi = mid;
    }
    const long long off = (w - a.win_first[lo]) * (long long)a.window;
    const long long left = a.len[lo] - off;
    const int m = (int)(left < (long long)a.window ? left : (long long)a.window);       // the last window of an utterance is short
    WinAcc acc = {0.0, 0.f, 0};
    if (m > 0) {
        const float* __restrict__ x = a.pool + a.start[lo] + off;
        const int mis = (int)(((uintptr_t)x >> 2) & 3);
        int head = (4 - mis) & 3;                         // samples in front of the first 16-byte boundary
        if (head > m) head = m;
        const int nvec = (m - head) >> 2;
        const int tail0 = head + 4 * nvec;
        if (lane < head) acc.take(x[lane], a.clip_thr);
        const f32x4* __restrict__ xv = reinterpret_cast<const f32x4*>(x + head);
        for (int v = lane; v < nvec; v += 64) {
            const f32x4 q = xv[v];
            acc.take(q[0], a.clip_thr); acc.take(q[1], a.clip_thr); acc.take(q[2], a.clip_thr); acc.take(q[3], a.clip_thr);
        }
        if (lane < m - tail0) acc.take(x[tail0 + lane], a.clip_thr);
    }
    double s = wave_sum_d(acc.s);
    float pk = acc.pk;
    int nc = acc.nc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pk = max_nan(pk, __shfl_xor(pk, o, 64));
        nc += __shfl_xor(nc, o, 64);
    }
    if (lane == 0) a.ws[w] = {s, pk, nc};
}

// sums over a workgroup of SCREEN_THREADS in one fixed order: the xor tree of a wavefront, then the wavefronts ascending
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();                                      // sh may still be read from the call before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int k = 1; k < SCREEN_THREADS / 64; ++k) t += sh[k];
    return t;
}

__device__ __forceinline__ double window_prob(double s, double sc2) {
    const double e = 20.0 * log10(sc2 * s + 1e-6);
    return 1.0 / (1.0 + exp(-(-1.0 + 0.2 * e)));
}

__global__ void __launch_bounds__(SCREEN_THREADS) screen_finish_kernel(ScreenArgs a) {
    __shared__ double sh[SCREEN_THREADS / 64];
    __shared__ float shp[SCREEN_THREADS / 64];
    const int u = blockIdx.x, tid = threadIdx.x;
    const long long w0 = a.win_first[u], nw = a.win_first[u + 1] - w0, L = a.len[u];
    const WinRow* __restrict__ rows = a.ws + w0;
    double s = 0.0, nc = 0.0;                             // counts as doubles: exact below 2^53
    float pk = 0.f;
    for (long long i = tid; i < nw; i += SCREEN_THREADS) {
        const WinRow r = rows[i];
        s += r.s;
        nc += (double)r.nclip;
        pk = max_nan(pk, r.peak);
    }
    s = block_sum_d(s, sh);
    nc = block_sum_d(nc, sh);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = max_nan(pk, __shfl_xor(pk, o, 64));
    if ((tid & 63) == 0) shp[tid >> 6] = pk;
    __syncthreads();
    pk = shp[0];
#pragma unroll
    for (int k = 1; k < SCREEN_THREADS / 64; ++k) pk = max_nan(pk, shp[k]);
    const double rms = L > 0 ? sqrt(s / (double)L) : 0.0;
    const double scalar = pow(10.0, a.target_db / 20.0) / (rms + 1e-6);
    const double sc2 = scalar * scalar;
    double na = 0.0;
    for (long long i = tid; i < nw; i += SCREEN_THREADS) {
        const double p = window_prob(rows[i].s, sc2);
        const double q = i > 0 ? window_prob(rows[i - 1].s, sc2) : 0.0;          // the UNSMOOTHED value of the window before
        const double sm = p > q ? p * 0.8 + q * (1.0 - 0.8) : p * 0.05 + q * (1.0 - 0.05);
        na += sm > a.act_thr ? 1.0 : 0.0;
    }
    na = block_sum_d(na, sh);
    if (tid == 0) {
        double* o = a.out + 6 * (size_t)u;
        o[0] = (double)pk;
        o[1] = nc;
        o[2] = rms;
        o[3] = (double)nw;
        o[4] = na;
        o[5] = nw > 0 ? na / (double)nw : nan("");
    }
}

// ---- RT60 --------------------------------------------------------------------------------------------------------------------------
constexpr int RT_THREADS = 256, RT_PER = 8;
constexpr int RT_CHUNK = RT_THREADS * RT_PER;
static_assert(RT_CHUNK == CRUSE_RT60_CHUNK, "chunk size");
static_assert(RT_THREADS == SCREEN_THREADS, "block_sum_d");

struct RtArgs {
    const float* pool;
    const long long* start;
    const long long* len;
    int n, max_len, sr;
    double lo_db, hi_db;
    double* ws;                    // [n][ws_stride] chunk suffixes
    int ws_stride;
    double* out;                   // [n][3]
};

// E[t] of the 8 samples a thread holds in the chunk that starts at sample `base`: E = after + (off + local suffix), off = the sum over
// the threads behind this one, added one by one from the last thread (so E never rises with falling t, bit for bit).  -> the chunk's sum
__device__ __forceinline__ double chunk_edc(const float* __restrict__ h, long long base, long long L, double after, double (&E)[RT_PER],
                                            double* tot) {
    const int tid = threadIdx.x;
    const long long t = base + (long long)RT_PER * tid;
    double ls[RT_PER];                                    // the sums from sample j of this thread to its last
    double behind = 0.0;
#pragma unroll
    for (int j = RT_PER - 1; j >= 0; --j) {
        const double v = t + j < L ? (double)h[t + j] : 0.0;
        behind = v * v + behind;
        ls[j] = behind;
    }
    __syncthreads();                                      // tot may still be read from the chunk before
    tot[tid] = ls[0];
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int i = RT_THREADS - 1; i >= 0; --i) {
            const double v = tot[i];
            tot[i] = run;
            run += v;
        }
        tot[RT_THREADS] = run;
    }
    __syncthreads();
    const double off = tot[tid];
#pragma unroll
    for (int j = 0; j < RT_PER; ++j) E[j] = after + (off + ls[j]);
    return tot[RT_THREADS];
}

__global__ void __launch_bounds__(RT_THREADS) rt60_kernel(RtArgs a) {
    __shared__ double tot[RT_THREADS + 1];
    __shared__ double sh[RT_THREADS / 64];
    __shared__ float shm[RT_THREADS / 64];
    __shared__ long long shi[RT_THREADS / 64];
    __shared__ double sh_e0, sh_floor;
    const int u = blockIdx.x, tid = threadIdx.x;
    const long long L = a.len[u];
    const float* __restrict__ h = a.pool + a.start[u];
    double* __restrict__ suf = a.ws + (size_t)u * a.ws_stride;
    double* o = a.out + 3 * (size_t)u;
    const double qnan = nan("");
    if (L <= 0 || L > (long long)a.max_len) {             // beyond max_len the workspace row would not hold the chunks
        if (tid == 0) { o[0] = qnan; o[1] = qnan; o[2] = qnan; }
        return;
    }
    // t0: the first index of max |h|
    float bm = -1.f;
    long long bi = 0;
    for (long long i = tid; i < L; i += RT_THREADS) {
        const float av = fabsf(h[i]);
        if (av > bm) { bm = av; bi = i; }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        const float om = __shfl_xor(bm, k, 64);
        const long long oi = __shfl_xor(bi, k, 64);
        if (om > bm || (om == bm && oi < bi)) { bm = om; bi = oi; }
    }
    if ((tid & 63) == 0) { shm[tid >> 6] = bm; shi[tid >> 6] = bi; }
    __syncthreads();
    bm = shm[0]; bi = shi[0];
#pragma unroll
    for (int k = 1; k < RT_THREADS / 64; ++k)
        if (shm[k] > bm || (shm[k] == bm && shi[k] < bi)) { bm = shm[k]; bi = shi[k]; }
    const long long t0 = bm >= 0.f ? bi : 0;              // all NaN: index 0, and every result below is NaN
    const int nch = (int)((L - t0 + RT_CHUNK - 1) / RT_CHUNK);      // <= ws_stride: L <= max_len
    double E[RT_PER];
    // chunk sums, then their suffixes (the sum of everything behind chunk c) in place
    for (int c = 0; c < nch; ++c) {
        const double sc = chunk_edc(h, t0 + (long long)c * RT_CHUNK, L, 0.0, E, tot);
        if (tid == 0) suf[c] = sc;
    }
    if (tid == 0) {
        double run = 0.0;
        for (int c = nch - 1; c >= 0; --c) {
            const double v = suf[c];
            suf[c] = run;
            run += v;
        }
        sh_e0 = run;                                      // = E[t0] as chunk_edc forms it: suf[0] + (0 + the sum of chunk 0)
        sh_floor = qnan;
    }
    __threadfence_block();
    __syncthreads();
    const double e0 = sh_e0;
    if (!(e0 > 0.0)) {                                    // an all-zero (or NaN) response
        if (tid == 0) { o[0] = qnan; o[1] = (double)t0; o[2] = qnan; }
        return;
    }
    double clo = 0.0, chi = 0.0;
    for (int c = 0; c < nch; ++c) {
        const long long t = t0 + (long long)c * RT_CHUNK + (long long)RT_PER * tid;
        chunk_edc(h, t0 + (long long)c * RT_CHUNK, L, suf[c], E, tot);
#pragma unroll
        for (int j = 0; j < RT_PER; ++j) {
            if (t + j >= L) continue;
            const double D = 10.0 * log10(E[j] / e0);
            clo += D > a.lo_db ? 1.0 : 0.0;
            chi += D > a.hi_db ? 1.0 : 0.0;
            if (t + j == L - 1) sh_floor = D;
        }
    }
    clo = block_sum_d(clo, sh);
    chi = block_sum_d(chi, sh);
    const long long tlo = t0 + (long long)clo, thi = t0 + (long long)chi;
    const bool fit = thi - tlo >= 2 && thi < L;           // thi == L: the decay never reaches hi_db
    double sxy = 0.0, sxx = 0.0;
    if (fit) {
        const double mid = 0.5 * (double)(tlo + thi - 1);
        for (int c = (int)((tlo - t0) / RT_CHUNK); c <= (int)((thi - 1 - t0) / RT_CHUNK); ++c) {
            const long long t = t0 + (long long)c * RT_CHUNK + (long long)RT_PER * tid;
            chunk_edc(h, t0 + (long long)c * RT_CHUNK, L, suf[c], E, tot);
#pragma unroll
            for (int j = 0; j < RT_PER; ++j) {
                if (t + j < tlo || t + j >= thi) continue;
                const double x = (double)(t + j) - mid;
                sxy += x * (10.0 * log10(E[j] / e0));
                sxx += x * x;
            }
        }
    }
    sxy = block_sum_d(sxy, sh);
    sxx = block_sum_d(sxx, sh);
    if (tid == 0) {
        o[0] = fit ? -60.0 / ((sxy / sxx) * (double)a.sr) : qnan;
        o[1] = (double)t0;
        o[2] = sh_floor;
    }
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" long long cruse_screen_ws_bytes(int n, long long total_windows) {
    if (n < 0 || total_windows < 0 || total_windows > SCREEN_MAX_WINDOWS) return -1;
    return total_windows * (long long)sizeof(WinRow);
}

extern "C" long long cruse_rt60_ws_bytes(int n, int max_len) {
    if (n < 0 || max_len < 0 || max_len > CRUSE_RT60_MAX_LEN) return -1;
    return (long long)n * (long long)cdiv(max_len, RT_CHUNK) * (long long)sizeof(double);
}

extern "C" int cruse_screen_clips(const float* pool, const long long* start, const long long* len, const long long* win_first, int n,
                                  long long total_windows, int window, float clip_thr, double target_db, double act_thr, void* ws, double* out,
                                  void* stream) {
    const char* who = "cruse_screen_clips";
    CRUSE_REQUIRE(n >= 0, CRUSE_E_SHAPE, "%s: n = %d (need n >= 0)", who, n);
    CRUSE_REQUIRE(window >= 1 && window <= SCREEN_MAX_WINDOW, CRUSE_E_SHAPE, "%s: window = %d (1..%d samples)", who, window, SCREEN_MAX_WINDOW);
    CRUSE_REQUIRE(total_windows >= 0 && total_windows <= SCREEN_MAX_WINDOWS, CRUSE_E_SHAPE, "%s: total_windows = %lld (0..%lld)", who,
                  total_windows, SCREEN_MAX_WINDOWS);
    CRUSE_REQUIRE(pool && start && len && win_first && ws && out, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(aligned(pool, 4) && aligned(start, 8) && aligned(len, 8) && aligned(win_first, 8) && aligned(ws, 8) && aligned(out, 8),
                  CRUSE_E_ALIGN, "%s: pool must be 4-byte, the tables, ws and out 8-byte aligned", who);
    if (n == 0) return CRUSE_OK;
    const ScreenArgs a = {pool, start, len, win_first, n, total_windows, window, clip_thr, target_db, act_thr, (WinRow*)ws, out};
    const hipStream_t st = (hipStream_t)stream;
    if (total_windows > 0) {
        hipLaunchKernelGGL(screen_window_kernel, dim3((unsigned)cdivl(total_windows, SCREEN_WPB)), dim3(SCREEN_THREADS), 0, st, a);
        CRUSE_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(screen_finish_kernel, dim3(n), dim3(SCREEN_THREADS), 0, st, a);
    CRUSE_LAUNCH_CHECK(who);
    return CRUSE_OK;
}

extern "C" int cruse_rt60(const float* pool, const long long* start, const long long* len, int n, int max_len, int sr, double lo_db,
                          double hi_db, void* ws, double* out, void* stream) {
    const char* who = "cruse_rt60";
    CRUSE_REQUIRE(n >= 0, CRUSE_E_SHAPE, "%s: n = %d (need n >= 0)", who, n);
    CRUSE_REQUIRE(max_len >= 0 && max_len <= CRUSE_RT60_MAX_LEN, CRUSE_E_SHAPE, "%s: max_len = %d (0..%d samples)", who, max_len,
                  CRUSE_RT60_MAX_LEN);
    CRUSE_REQUIRE(sr >= 1, CRUSE_E_SHAPE, "%s: sr = %d (need sr >= 1)", who, sr);
    CRUSE_REQUIRE(lo_db > hi_db, CRUSE_E_SHAPE, "%s: lo_db = %g <= hi_db = %g (the fit runs from lo_db down to hi_db)", who, lo_db, hi_db);
    CRUSE_REQUIRE(pool && start && len && ws && out, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(aligned(pool, 4) && aligned(start, 8) && aligned(len, 8) && aligned(ws, 8) && aligned(out, 8), CRUSE_E_ALIGN,
                  "%s: pool must be 4-byte, the tables, ws and out 8-byte aligned", who);
    if (n == 0) return CRUSE_OK;
    const RtArgs a = {pool, start, len, n, max_len, sr, lo_db, hi_db, (double*)ws, cdiv(max_len, RT_CHUNK), out};
    hipLaunchKernelGGL(rt60_kernel, dim3(n), dim3(RT_THREADS), 0, (hipStream_t)stream, a);
    CRUSE_LAUNCH_CHECK(who);
    return CRUSE_OK;
}
