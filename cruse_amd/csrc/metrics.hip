// Validation metrics on the device (cruse_si_sdr, cruse_stoi*): the two closed-form metrics of train_base/metrics.py, SI_SDR (:60-82)
// and the classic STOI (Taal, Hendriks, Heusdens, Jensen 2011), whose definition DESIGN section 13 restates.  Nothing here is shared
// with the training step or the streaming chains.  f32 storage; every sum runs in a fixed order, no atomics, so a result is
// bit-identical from run to run and a clip scores the same alone and inside a batch.
//
// STOI, one call = six dependent launches on one stream, none of which the host waits for (every kernel after the mask reads the
// clip's n_kept from the workspace, so the call captures into a HIP graph):
//   1 stoi_resample   grid (ceil(L10/256), 2, B)   16 kHz -> 10 kHz, the 51 / 52 contributing taps of the 257-tap prototype per output
//   2 stoi_energy     grid (ceil(nF/4), B)         one wave per 256-sample frame of ref10: e[i] in dB
//   3 stoi_mask       grid (B)                     max(e), the ordered list of kept frames (ballot prefix), n_kept
//   4 stoi_spectra    grid (nF-1, B)               gathers frame g of the compacted ref and est, windows it, direct 512-point DFT of the
//                                                  bins the 15 bands cover against an LDS cos / sin table, band sums -> tob
//   5 stoi_segments   grid (ceil(nSeg/256), 15, B) one thread per (segment, band): clip, centre, normalise, correlate; block tree in f64
//   6 stoi_final      grid (B)                     sums the block partials in order -> out[b]
//
// Ragged batches (cruse_si_sdr_ragged, cruse_stoi_ragged): clip b is ref[b][0 : len[b]], len a DEVICE array that only the kernels read.
// si_sdr, stoi_resample, stoi_energy and stoi_mask exist a second time (RAG = true) with the clip's own length, L10 and nF in place of
// the batch's; every later stage reads n_kept already.  Same taps, same trees: a clip scores the same in a ragged batch and alone.
// extended != 0 (ESTOI, Jensen & Taal 2016) replaces launch 5:
//   5e stoi_eseg      grid (ceil(nSeg/256), B)     half a wave per segment, lane = frame: rows then columns normalised, f64 block tree
#include <math.h>
#include <algorithm>
#include <string.h>
#include <mutex>
#include "common.h"

namespace {

constexpr int TAPS = 257;                 // prototype low-pass on the 80 kHz grid
constexpr int UP = 5, DOWN = 8;           // 16 kHz * 5 / 8 = 10 kHz
constexpr int FRAME = 256, HOPF = 128;    // 25.6 ms frames at 10 kHz, half overlap
constexpr int NFFT = 512;
constexpr int NBANDS = 15;
constexpr int SEG = 30;                   // frames of an intermediate intelligibility segment (384 ms)
constexpr int THREADS = 256;
constexpr float DYN_RANGE = 40.0f;        // dB below the loudest frame of ref at which a frame counts as silent
constexpr float EPS = 2.220446049250313e-16f;   // 2^-52: numpy's float64 eps, representable in f32
constexpr float SHORT_SCORE = 1e-5f;      // a clip without a full segment (pystoi returns the same value)
constexpr int MAX_L = 1 << 28;            // 5 L + 135 < 2^31: every per-clip index fits an int
constexpr int MAX_B = 65535;              // gridDim.y / .z

// table offsets (floats): prototype taps | window hanning(258)[1:-1] | cos, sin(2 pi j / 512)
constexpr int TB_H = 0, TB_W = 260, TB_COS = 516, TB_SIN = 1028, TB_TOTAL = 1540;

// cruse_stoi_layout(): all ints, in the order of the header's description; offsets in 4-byte units from the workspace base
struct StoiLayout {
    int L10, nF, nGs, nSB;                // 10 kHz samples, frames, row stride of tob (= max(nF - 1, 1)), segment blocks per band
    int x10, e, nk, kept, tob, part;      // [B][2][L10] f32 | [B][nF'] f32 | [B] int | [B][nF'] int | [B][2][15][nGs] f32 | [B][15][nSB] f64
    int total;                            // nF' = max(nF, 1)
};
static_assert(sizeof(StoiLayout) == CRUSE_STOI_LAYOUT_INTS * sizeof(int), "StoiLayout and CRUSE_STOI_LAYOUT_INTS disagree");

struct Bands { int lo[NBANDS], hi[NBANDS]; };

int make_layout(const char* who, int B, int L, StoiLayout& Y) {
    CRUSE_REQUIRE(B >= 1 && L >= 1, CRUSE_E_SHAPE, "%s: B = %d, L = %d", who, B, L);
    CRUSE_REQUIRE(B <= MAX_B && L <= MAX_L, CRUSE_E_SHAPE, "%s: B = %d > %d or L = %d > %d", who, B, MAX_B, L, MAX_L);
    const long long L10 = (5LL * L + 7) / 8;
    const long long nF = L10 >= FRAME ? (L10 - FRAME) / HOPF + 1 : 0, nFa = nF > 0 ? nF : 1;
    const long long nGs = nF > 1 ? nF - 1 : 1, nSB = (std::max(nGs - (SEG - 1), 1LL) + THREADS - 1) / THREADS;
    long long o = 0;
    Y.L10 = (int)L10; Y.nF = (int)nF; Y.nGs = (int)nGs; Y.nSB = (int)nSB;
    const long long x10 = o; o += 2LL * B * L10;
    const long long e = o;   o += (long long)B * nFa;
    const long long nk = o;  o += B;
    const long long kept = o; o += (long long)B * nFa;
    const long long tob = o; o += 2LL * NBANDS * B * nGs;
    o += o & 1;                                                        // f64 partials: 8-byte aligned
    const long long part = o; o += 2LL * NBANDS * B * nSB;
    CRUSE_REQUIRE(o < (1LL << 31), CRUSE_E_SHAPE, "%s: B = %d clips of L = %d need a workspace of %lld bytes, beyond 8 GiB", who, B, L, 4 * o);
    Y.x10 = (int)x10; Y.e = (int)e; Y.nk = (int)nk; Y.kept = (int)kept; Y.tob = (int)tob; Y.part = (int)part; Y.total = (int)o;
    return CRUSE_OK;
}

// band k covers bins [argmin |f - 150 * 2^((2k-1)/6)|, argmin |f - 150 * 2^((2k+1)/6)|), f = j * 10000 / 512
const Bands& bands() {
    static Bands b;
    static std::once_flag once;
    std::call_once(once, [] {
        auto nearest = [](double f) {
            int best = 0;
            for (int j = 1; j <= NFFT / 2; ++j)
                if (fabs(j * 10000.0 / NFFT - f) < fabs(best * 10000.0 / NFFT - f)) best = j;       // first minimum, as argmin
            return best;
        };
        for (int k = 0; k < NBANDS; ++k) {
            b.lo[k] = nearest(150.0 * pow(2.0, (2 * k - 1) / 6.0));
            b.hi[k] = nearest(150.0 * pow(2.0, (2 * k + 1) / 6.0));
        }
    });
    return b;
}

// modified Bessel function I0 by its power series (all terms positive: no cancellation)
double bessel_i0(double x) {
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= (x / 2.0) * (x / 2.0) / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// sum of `v` over the workgroup in a fixed tree; the result is valid in every thread.  red: THREADS doubles
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// the ragged kernels' view of clip b: its length clamped to [0, L], and the stage sizes that follow from it
__device__ __forceinline__ int clip_len(const int* __restrict__ len, int b, int L) { return min(max(len[b], 0), L); }
__device__ __forceinline__ int clip_l10(int n) { return (UP * n + DOWN - 1) / DOWN; }                  // n <= 2^28
__device__ __forceinline__ int clip_frames(int l10) { return l10 >= FRAME ? (l10 - FRAME) / HOPF + 1 : 0; }

// ---- SI-SDR: one workgroup per clip, f64 sums --------------------------------------------------------------------------------------
template <bool RAG>
__global__ void __launch_bounds__(THREADS) si_sdr_kernel(const float* __restrict__ ref, const float* __restrict__ est, int Lrow,
                                                         const int* __restrict__ len, float* __restrict__ out) {
    __shared__ double red[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* r = ref + (size_t)b * Lrow;
    const float* e = est + (size_t)b * Lrow;
    const int L = RAG ? clip_len(len, b, Lrow) : Lrow;                 // 0: 0 / 0 = NaN, as numpy
    double sre = 0.0, srr = 0.0;
    for (int i = tid; i < L; i += THREADS) {
        const double x = r[i], y = e[i];
        sre = fma(x, y, sre);
        srr = fma(x, x, srr);
    }
    sre = block_sum_d(sre, red);
    srr = block_sum_d(srr, red);
    const double alpha = sre / srr;
    double sn = 0.0;
    for (int i = tid; i < L; i += THREADS) {
        const double d = (double)e[i] - alpha * (double)r[i];
        sn = fma(d, d, sn);
    }
    sn = block_sum_d(sn, red);
    if (tid == 0) out[b] = (float)(10.0 * log10(alpha * alpha * srr / sn));
}

// ---- STOI ------------------------------------------------------------------------------------------------------------------------
// x10[n] = 5 sum_k h[k] v[8 n + 128 - k], v[5 i] = u[i]: the taps k = k0 + 5 j with 8 n + 128 - k = 5 i, ascending
template <bool RAG>
__global__ void __launch_bounds__(THREADS) stoi_resample_kernel(const float* __restrict__ ref, const float* __restrict__ est, int Lrow,
                                                                const int* __restrict__ len, StoiLayout Y, const float* __restrict__ tab,
                                                                float* __restrict__ ws) {
    __shared__ float h[TAPS];
    const int tid = threadIdx.x, b = blockIdx.z, r = blockIdx.y;
    const int L = RAG ? clip_len(len, b, Lrow) : Lrow;                 // samples >= L are outside the clip: never loaded
    const int L10 = RAG ? clip_l10(L) : Y.L10;                         // outputs beyond the clip's own L10 stay unwritten
    if (RAG && blockIdx.x * THREADS >= L10) return;
    for (int k = tid; k < TAPS; k += THREADS) h[k] = tab[TB_H + k];
    __syncthreads();
    const int n = blockIdx.x * THREADS + tid;
    if (n >= L10) return;
    const float* u = (r == 0 ? ref : est) + (size_t)b * Lrow;
    const int m = DOWN * n + (TAPS - 1) / 2;                           // <= 5 L + 134
    const int k0 = m % UP;
    int i = (m - k0) / UP;                                             // the input sample under tap k0; one less per step
    float acc = 0.f;
    for (int k = k0; k < TAPS; k += UP, --i) {
        if (i < 0) break;
        if (i < L) acc = fmaf(h[k], u[i], acc);
    }
    ws[Y.x10 + ((size_t)b * 2 + r) * Y.L10 + n] = (float)UP * acc;
}

// e[i] = 20 log10(|| w * ref10[128 i : 128 i + 256] || + eps): one wave per frame
template <bool RAG>
__global__ void __launch_bounds__(THREADS) stoi_energy_kernel(StoiLayout Y, int Lrow, const int* __restrict__ len,
                                                              const float* __restrict__ tab, float* __restrict__ ws) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (i >= (RAG ? clip_frames(clip_l10(clip_len(len, b, Lrow))) : Y.nF)) return;
    const float* x = ws + Y.x10 + (size_t)b * 2 * Y.L10 + (size_t)i * HOPF;            // the last frame ends at 128 (nF - 1) + 256 <= L10
    float s = 0.f;
    for (int q = 0; q < FRAME / 64; ++q) {
        const float v = tab[TB_W + q * 64 + lane] * x[q * 64 + lane];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) ws[Y.e + (size_t)b * max(Y.nF, 1) + i] = 20.0f * log10f(sqrtf(s) + EPS);
}

// kept = the frames with e[i] > max(e) - 40, ascending; nk = their count
template <bool RAG>
__global__ void __launch_bounds__(THREADS) stoi_mask_kernel(StoiLayout Y, int Lrow, const int* __restrict__ len, float* __restrict__ ws) {
    __shared__ float wmax[THREADS / 64];
    __shared__ int wcnt[THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nFa = max(Y.nF, 1), nF = RAG ? clip_frames(clip_l10(clip_len(len, b, Lrow))) : Y.nF;
    const float* e = ws + Y.e + (size_t)b * nFa;
    int* kept = (int*)ws + Y.kept + (size_t)b * nFa;
    float mx = -INFINITY;
    for (int i = tid; i < nF; i += THREADS) mx = fmaxf(mx, e[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float thr = mx - DYN_RANGE;
    int base = 0;
    for (int i0 = 0; i0 < nF; i0 += THREADS) {
        const int i = i0 + tid;
        const bool keep = i < nF && e[i] > thr;
        const unsigned long long bal = __ballot(keep);
        __syncthreads();                                               // wcnt of the previous round has been read
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int off = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) off += wcnt[w];
        if (keep) kept[off] = i;
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    if (tid == 0) ((int*)ws)[Y.nk + b] = base;
}

// frame g of the compacted signals: sample j = 128 g + t sums the (at most two) kept frames c = j / 128 - 1, j / 128 that cover it
__global__ void __launch_bounds__(THREADS) stoi_spectra_kernel(StoiLayout Y, Bands bd, const float* __restrict__ tab,
                                                               float* __restrict__ ws) {
    __shared__ float cs[2 * NFFT];
    __shared__ float fr[2][FRAME];
    __shared__ float pw[2][FRAME];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nk = ((const int*)ws)[Y.nk + b];
    if (g >= nk - 1) return;                                           // nG = nk - 1 frames
    const int* kept = (const int*)ws + Y.kept + (size_t)b * max(Y.nF, 1);
    for (int j = tid; j < 2 * NFFT; j += THREADS) cs[j] = tab[TB_COS + j];
    {
        const int c1 = g + (tid >> 7), t1 = tid & (HOPF - 1), c0 = c1 - 1, t0 = t1 + HOPF;      // c1 <= g + 1 <= nk - 1
        const float w = tab[TB_W + tid];
        for (int r = 0; r < 2; ++r) {
            const float* x = ws + Y.x10 + ((size_t)b * 2 + r) * Y.L10;
            float y = 0.f;
            if (c0 >= 0) y = tab[TB_W + t0] * x[(size_t)kept[c0] * HOPF + t0];
            y += tab[TB_W + t1] * x[(size_t)kept[c1] * HOPF + t1];
            fr[r][tid] = w * y;
        }
    }
    __syncthreads();
    // bins below the first band and from the last band's end on (up to 256) enter no band: not computed
    if (tid >= bd.lo[0] && tid < bd.hi[NBANDS - 1]) {
        float re0 = 0.f, im0 = 0.f, re1 = 0.f, im1 = 0.f;
        int j = 0;
        for (int n = 0; n < FRAME; ++n) {
            const float c = cs[j], s = cs[NFFT + j], x0 = fr[0][n], x1 = fr[1][n];
            re0 = fmaf(x0, c, re0);
            im0 = fmaf(x0, s, im0);
            re1 = fmaf(x1, c, re1);
            im1 = fmaf(x1, s, im1);
            j = (j + tid) & (NFFT - 1);
        }
        pw[0][tid] = re0 * re0 + im0 * im0;
        pw[1][tid] = re1 * re1 + im1 * im1;
    }
    __syncthreads();
    if (tid < 2 * NBANDS) {
        const int r = tid / NBANDS, k = tid - r * NBANDS;
        float s = 0.f;
        for (int j = bd.lo[k]; j < bd.hi[k]; ++j) s += pw[r][j];
        ws[Y.tob + (((size_t)b * 2 + r) * NBANDS + k) * Y.nGs + g] = sqrtf(s);
    }
}

// segment s = frames [s, s + 30) of band k: one thread each; the block's sum of correlations -> part[b][k][block]
__global__ void __launch_bounds__(THREADS) stoi_segments_kernel(StoiLayout Y, float* __restrict__ ws) {
    __shared__ double red[THREADS];
    const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int nSeg = ((const int*)ws)[Y.nk + b] - 1 - (SEG - 1);       // nG - 29
    if (blockIdx.x * THREADS >= nSeg) return;
    const int s = blockIdx.x * THREADS + tid;
    float d = 0.f;
    if (s < nSeg) {
        const float* X = ws + Y.tob + (((size_t)b * 2 + 0) * NBANDS + k) * Y.nGs + s;
        const float* Yr = ws + Y.tob + (((size_t)b * 2 + 1) * NBANDS + k) * Y.nGs + s;
        float x[SEG], y[SEG];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            x[i] = X[i];
            y[i] = Yr[i];
            sx = fmaf(x[i], x[i], sx);
            sy = fmaf(y[i], y[i], sy);
        }
        const float alpha = sqrtf(sx) / (sqrtf(sy) + EPS);
        const float clip = 1.0f + 5.623413251903491f;                  // 1 + 10^(15 / 20)
        float mx = 0.f, my = 0.f;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            y[i] = fminf(alpha * y[i], x[i] * clip);
            mx += x[i];
            my += y[i];
        }
        mx /= (float)SEG;
        my /= (float)SEG;
        float nx = 0.f, ny = 0.f;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            x[i] -= mx;
            y[i] -= my;
            nx = fmaf(x[i], x[i], nx);
            ny = fmaf(y[i], y[i], ny);
        }
        const float ix = sqrtf(nx) + EPS, iy = sqrtf(ny) + EPS;
#pragma unroll
        for (int i = 0; i < SEG; ++i) d = fmaf(x[i] / ix, y[i] / iy, d);
    }
    const double t = block_sum_d((double)d, red);
    if (tid == 0) ((double*)(ws + Y.part))[((size_t)b * NBANDS + k) * Y.nSB + blockIdx.x] = t;
}

// sum of `v` over the 32 lanes of a half wave in a fixed xor tree (no lane leaves its half); every lane of the half holds the result
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ESTOI's normalisation of a 15 x 30 segment, lane = frame, v[k] = band k: every row (a band over its 30 frames) less its mean over
// (its norm + eps), by half-wave trees; then every column (a frame over its 15 bands) the same, in registers.  A lane that holds no
// frame carries zeros in and out.
__device__ __forceinline__ void estoi_normalise(float (&v)[NBANDS], bool live) {
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) {
        const float mean = half_sum(v[k]) / (float)SEG;
        const float c = live ? v[k] - mean : 0.f;
        v[k] = c / (sqrtf(half_sum(c * c)) + EPS);
    }
    float m = 0.f, n = 0.f;
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) m += v[k];
    m /= (float)NBANDS;
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) {
        v[k] -= m;
        n = fmaf(v[k], v[k], n);
    }
    const float inv = sqrtf(n) + EPS;
#pragma unroll
    for (int k = 0; k < NBANDS; ++k) v[k] /= inv;
}

// ESTOI (extended != 0) in place of stoi_segments: segment s = frames [s, s + 30) of all 15 bands, half a wave each.  No clipping and no
// alpha: X and Y normalised as above, the segment scores sum(X^ Y^) / 30.  A workgroup owns 256 consecutive segments, half wave h of its
// eight the segments h, h + 8, ...: their f64 sum in that order, then the eight sums in a fixed tree -> part[b][0][block].  The order of
// every sum follows from the segment index alone, so a score does not depend on B; no atomics.
__global__ void __launch_bounds__(THREADS) stoi_eseg_kernel(StoiLayout Y, float* __restrict__ ws) {
    __shared__ double red[THREADS / 32];
    const int b = blockIdx.y, tid = threadIdx.x, f = tid & 31, hw = tid >> 5;
    const int nSeg = ((const int*)ws)[Y.nk + b] - 1 - (SEG - 1);       // nG - 29
    const int s0 = blockIdx.x * THREADS;
    if (s0 >= nSeg) return;
    const float* X = ws + Y.tob + (size_t)b * 2 * NBANDS * Y.nGs;
    const float* Yr = X + (size_t)NBANDS * Y.nGs;
    double acc = 0.0;
    for (int j = 0; j < 32 && s0 + 8 * j < nSeg; ++j) {                // the bound is the workgroup's: every lane takes every shuffle
        const int s = s0 + 8 * j + hw;
        const bool live = s < nSeg && f < SEG;                         // s + f <= nSeg - 1 + 29 = nG - 1
        float x[NBANDS], y[NBANDS];
#pragma unroll
        for (int k = 0; k < NBANDS; ++k) {
            x[k] = live ? X[(size_t)k * Y.nGs + s + f] : 0.f;
            y[k] = live ? Yr[(size_t)k * Y.nGs + s + f] : 0.f;
        }
        estoi_normalise(x, live);
        estoi_normalise(y, live);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < NBANDS; ++k) d = fmaf(x[k], y[k], d);
        acc += (double)(half_sum(d) / (float)SEG);                     // a half wave past the last segment adds 0
    }
    if (f == 0) red[hw] = acc;
    __syncthreads();
    if (tid == 0)
        ((double*)(ws + Y.part))[(size_t)b * NBANDS * Y.nSB + blockIdx.x] =
            ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

// EXT: the partials of stoi_eseg (one row of blocks, part[b][0][.]) over nSeg; else those of stoi_segments over 15 nSeg
template <bool EXT>
__global__ void __launch_bounds__(THREADS) stoi_final_kernel(StoiLayout Y, const float* __restrict__ ws, float* __restrict__ out) {
    __shared__ double red[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nSeg = ((const int*)ws)[Y.nk + b] - 1 - (SEG - 1);
    if (nSeg < 1) {                                                    // nF < 1 or nG < 30
        if (tid == 0) out[b] = SHORT_SCORE;
        return;
    }
    const int nb = (nSeg + THREADS - 1) / THREADS;
    const double* part = (const double*)(ws + Y.part) + (size_t)b * NBANDS * Y.nSB;
    double acc = 0.0;
    constexpr int ROWS = EXT ? 1 : NBANDS;
    for (int i = tid; i < ROWS * nb; i += THREADS) acc += part[(size_t)(i / nb) * Y.nSB + i % nb];
    acc = block_sum_d(acc, red);
    if (tid == 0) out[b] = (float)(acc / ((double)ROWS * (double)nSeg));
}

// the launches of cruse_stoi (RAG = false: len and extended unused) and cruse_stoi_ragged, after the same refusals
template <bool RAG>
int stoi_run(const char* who, const float* ref, const float* est, int B, int L, const int* len, int extended, const float* tab, void* ws,
             size_t ws_bytes, float* out, void* stream) {
    CRUSE_REQUIRE(ref && est && tab && ws && out, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(!RAG || len, CRUSE_E_SHAPE, "%s: null len (the clips' lengths, int[B] on the device)", who);
    StoiLayout Y;
    const int rc = make_layout(who, B, L, Y);
    if (rc) return rc;
    CRUSE_REQUIRE(ws_bytes >= (size_t)Y.total * 4, CRUSE_E_SHAPE, "%s: workspace of %zu bytes, cruse_stoi_ws_bytes(%d, %d) = %zu", who, ws_bytes, B,
                  L, (size_t)Y.total * 4);
    CRUSE_REQUIRE(((uintptr_t)ws & 7) == 0, CRUSE_E_ALIGN, "%s: workspace not 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    float* w = (float*)ws;
    const Bands& bd = bands();
    hipLaunchKernelGGL(stoi_resample_kernel<RAG>, dim3(cdiv(Y.L10, THREADS), 2, B), dim3(THREADS), 0, s, ref, est, L, len, Y, tab, w);
    CRUSE_LAUNCH_CHECK("cruse_stoi (resample)");
    if (Y.nF >= 1) {
        hipLaunchKernelGGL(stoi_energy_kernel<RAG>, dim3(cdiv(Y.nF, THREADS / 64), B), dim3(THREADS), 0, s, Y, L, len, tab, w);
        CRUSE_LAUNCH_CHECK("cruse_stoi (energy)");
    }
    hipLaunchKernelGGL(stoi_mask_kernel<RAG>, dim3(B), dim3(THREADS), 0, s, Y, L, len, w);         // nF = 0: writes nk = 0
    CRUSE_LAUNCH_CHECK("cruse_stoi (mask)");
    if (Y.nF >= 2) {
        hipLaunchKernelGGL(stoi_spectra_kernel, dim3(Y.nF - 1, B), dim3(THREADS), 0, s, Y, bd, tab, w);
        CRUSE_LAUNCH_CHECK("cruse_stoi (spectra)");
    }
    if (Y.nF - 1 >= SEG) {                                              // else no clip can hold a segment
        if (RAG && extended) hipLaunchKernelGGL(stoi_eseg_kernel, dim3(Y.nSB, B), dim3(THREADS), 0, s, Y, w);
        else hipLaunchKernelGGL(stoi_segments_kernel, dim3(Y.nSB, NBANDS, B), dim3(THREADS), 0, s, Y, w);
        CRUSE_LAUNCH_CHECK("cruse_stoi (segments)");
    }
    if (RAG && extended) hipLaunchKernelGGL(stoi_final_kernel<true>, dim3(B), dim3(THREADS), 0, s, Y, (const float*)w, out);
    else hipLaunchKernelGGL(stoi_final_kernel<false>, dim3(B), dim3(THREADS), 0, s, Y, (const float*)w, out);
    CRUSE_LAUNCH_CHECK("cruse_stoi (final)");
    return CRUSE_OK;
}

template <bool RAG>
int si_sdr_run(const char* who, const float* ref, const float* est, int B, int L, const int* len, float* out, void* stream) {
    CRUSE_REQUIRE(ref && est && out, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(!RAG || len, CRUSE_E_SHAPE, "%s: null len (the clips' lengths, int[B] on the device)", who);
    CRUSE_REQUIRE(B >= 1 && L >= 1, CRUSE_E_SHAPE, "%s: B = %d, L = %d", who, B, L);
    CRUSE_REQUIRE(L <= MAX_L, CRUSE_E_SHAPE, "%s: L = %d > %d", who, L, MAX_L);
    hipLaunchKernelGGL(si_sdr_kernel<RAG>, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, ref, est, L, len, out);
    CRUSE_LAUNCH_CHECK("cruse_si_sdr");
    return CRUSE_OK;
}

}  // namespace

extern "C" int cruse_si_sdr(const float* ref, const float* est, int B, int L, float* out, void* stream) {
    return si_sdr_run<false>("si_sdr", ref, est, B, L, nullptr, out, stream);
}

extern "C" int cruse_si_sdr_ragged(const float* ref, const float* est, int B, int L, const int* len, float* out, void* stream) {
    return si_sdr_run<true>("si_sdr_ragged", ref, est, B, L, len, out, stream);
}

extern "C" int cruse_stoi_layout(int B, int L, int* out) {
    CRUSE_REQUIRE(out, CRUSE_E_SHAPE, "stoi_layout: null output");
    StoiLayout Y;
    const int rc = make_layout("stoi_layout", B, L, Y);
    if (rc) return rc;
    memcpy(out, &Y, sizeof(Y));
    return CRUSE_OK;
}

extern "C" size_t cruse_stoi_ws_bytes(int B, int L) {
    StoiLayout Y;
    return make_layout("stoi_ws_bytes", B, L, Y) ? 0 : (size_t)Y.total * 4;
}

extern "C" int cruse_stoi_tables(float* tab, void* stream) {
    CRUSE_REQUIRE(tab, CRUSE_E_SHAPE, "stoi_tables: null table");
    // built on the host in double precision, rounded once, then copied: 1540 floats
    static float t[TB_TOTAL];
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.14159265358979323846, beta = 9.0, fc = 0.9 * 0.5 / DOWN;
        double h[TAPS], sum = 0.0;
        for (int k = 0; k < TAPS; ++k) {
            const double n = k - (TAPS - 1) / 2, a = 2.0 * fc * n;
            const double sinc = n == 0 ? 1.0 : sin(pi * a) / (pi * a);
            const double r = 2.0 * k / (TAPS - 1) - 1.0;
            h[k] = 2.0 * fc * sinc * bessel_i0(beta * sqrt(fmax(1.0 - r * r, 0.0))) / bessel_i0(beta);
            sum += h[k];
        }
        for (int k = 0; k < TAPS; ++k) t[TB_H + k] = (float)(h[k] / sum);
        for (int n = 0; n < FRAME; ++n) t[TB_W + n] = (float)(0.5 - 0.5 * cos(2.0 * pi * (n + 1) / (FRAME + 1)));
        for (int j = 0; j < NFFT; ++j) {
            t[TB_COS + j] = (float)cos(2.0 * pi * j / NFFT);
            t[TB_SIN + j] = (float)sin(2.0 * pi * j / NFFT);
        }
    });
    CRUSE_HIP(hipMemcpyAsync(tab, t, sizeof(t), hipMemcpyHostToDevice, (hipStream_t)stream), "stoi_tables");
    CRUSE_HIP(hipStreamSynchronize((hipStream_t)stream), "stoi_tables");
    return CRUSE_OK;
}

extern "C" int cruse_stoi(const float* ref, const float* est, int B, int L, const float* tab, void* ws, size_t ws_bytes, float* out,
                          void* stream) {
    return stoi_run<false>("stoi", ref, est, B, L, nullptr, 0, tab, ws, ws_bytes, out, stream);
}

extern "C" int cruse_stoi_ragged(const float* ref, const float* est, int B, int L, const int* len, int extended, const float* tab, void* ws,
                                 size_t ws_bytes, float* out, void* stream) {
    return stoi_run<true>("stoi_ragged", ref, est, B, L, len, extended, tab, ws, ws_bytes, out, stream);
}
