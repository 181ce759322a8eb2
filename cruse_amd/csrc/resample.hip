// The two kernels under the file-list dataset (cruse_amd/filepairs.py: DeviceFilePairs).
//
// cruse_resample_poly: a ragged batch of recordings at one source rate -> the 16 kHz pool, by a rational polyphase FIR.  With
// (up, down) reduced, q = max(up, down), N = 32 q + 1 taps h (cruse_amd/resample_design.py), v[up i] = x[i] and zero elsewhere,
//     y[n] = up * sum_k h[k] v[n down + 16 q - k],   0 <= n < Lout = ceil(L up / down)
// which is scipy.signal.resample_poly(x, up, down, window=h).  Only k = p + up j with p = (n down + 16 q) mod up meet a sample:
//     y[n] = up * sum_{j < T} hp[p][j] x[i0 - j],     i0 = floor((n down + 16 q) / up),  T = ceil(N / up)
// where hp[p][j] = h[p + up j] is the phase-major table the host lays out (rows of `tap_stride` floats, a multiple of 4, so a
// thread reads its taps as float4).  j ascending is k ascending; the sum is f32 fmaf from 0 and there are no atomics: a result is
// bit-identical from run to run and a clip converts the same alone and inside a batch.
// A workgroup of 256 lanes owns a tile of CRUSE_RESAMPLE_TILE consecutive outputs of one clip (lane t the outputs t + 256 r: stores
// are coalesced).  The inputs the tile needs, (TILE - 1) down / up + T + 1 samples at most, are staged once in LDS -- int16 PCM is
// de-interleaved and scaled by 1 / 32768 on the way in, samples outside the clip are zeros -- whenever that window fits WIN_MAX
// floats (every ratio down / up below ~7: 8 ... 96 kHz); a steeper ratio (192 kHz) reads the clip directly with the same arithmetic.
// up = down = 1 is the conversion alone: no taps, y = x (x / 32768 for PCM, exact).
//
// cruse_assemble_clips: out[b][dst + j] = pool[src + j] inside the segments of clip b, 0.0f elsewhere -- utterances stitched with
// silence gaps and cropped, as the host planned it (filepairs.plan_clip).  Every sample of out is written exactly once.
#include "common.h"

namespace {

constexpr int THREADS = 256, PER = 4, TILE = THREADS * PER;
constexpr int WIN_MAX = 8192;                                          // floats of LDS for the staged window (32 KiB)
constexpr int MAX_RATIO = 1024;
constexpr int FMT_F32 = 0, FMT_S16 = 1;                                 // the in_fmt of the streaming _io entry points
constexpr long long MAX_LEN = (1ll << 31) - 1 - TILE;                  // tile * TILE + TILE stays an int
static_assert(TILE == CRUSE_RESAMPLE_TILE, "CRUSE_RESAMPLE_TILE is THREADS * PER");

__device__ __forceinline__ float load_src(const void* src, int fmt, int channels, int chan, long long i) {
    if (fmt == FMT_F32) return static_cast<const float*>(src)[i];
    return (float)static_cast<const short*>(src)[i * channels + chan] * (1.0f / 32768.0f);
}

__global__ void __launch_bounds__(THREADS) resample_copy_kernel(const void* __restrict__ src, int fmt, int channels, int chan,
                                                                const long long* __restrict__ off_in, const long long* __restrict__ off_out,
                                                                int tiles_per_clip, float* __restrict__ out) {
    const int b = blockIdx.x / tiles_per_clip, n0 = (blockIdx.x % tiles_per_clip) * TILE;
    const long long in0 = off_in[b], o0 = off_out[b];
    const int Lout = (int)(off_out[b + 1] - o0);
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int n = n0 + threadIdx.x + r * THREADS;
        if (n < Lout) out[o0 + n] = load_src(src, fmt, channels, chan, in0 + n);
    }
}

__global__ void __launch_bounds__(THREADS) resample_poly_kernel(const void* __restrict__ src, int fmt, int channels, int chan,
                                                                const long long* __restrict__ off_in, const long long* __restrict__ off_out,
                                                                int tiles_per_clip, int up, int down, int centre, int T, int tap_stride,
                                                                const float* __restrict__ taps, int staged, float* __restrict__ out) {
    __shared__ float win[WIN_MAX];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_clip, n0 = (blockIdx.x % tiles_per_clip) * TILE;
    const long long in0 = off_in[b], o0 = off_out[b];
    const int L = (int)(off_in[b + 1] - in0), Lout = (int)(off_out[b + 1] - o0);
    if (n0 >= Lout) return;                                            // workgroup-uniform: the grid is sized for the longest clip
    const int n1 = min(n0 + TILE, Lout);
    // the window: inputs w0 .. w0 + W - 1 of the clip (w0 may be negative, the end may pass L: zeros there)
    const long long w0 = ((long long)n0 * down + centre) / up - (T - 1);
    if (staged) {
        const int W = (int)(((long long)(n1 - 1) * down + centre) / up - w0) + 1;      // <= WIN_MAX: the host checked the ratio
        for (int w = tid; w < W; w += THREADS) {
            const long long i = w0 + w;
            win[w] = (i >= 0 && i < L) ? load_src(src, fmt, channels, chan, in0 + i) : 0.0f;
        }
        __syncthreads();
    }
    const float gain = (float)up;
#pragma unroll 1
    for (int r = 0; r < PER; ++r) {
        const int n = n0 + tid + r * THREADS;
        if (n >= n1) break;
        const long long m = (long long)n * down + centre, i0 = m / up;
        const float* hp = taps + (size_t)(int)(m - i0 * up) * tap_stride;
        float acc = 0.0f;
        if (staged) {
            const float* xw = win + (int)(i0 - w0);                    // in [T - 1, W - 1]
            int j = 0;
            for (; j + 4 <= T; j += 4) {
                const float4 h4 = *reinterpret_cast<const float4*>(hp + j);
                acc = fmaf(h4.x, xw[-j], acc);
                acc = fmaf(h4.y, xw[-j - 1], acc);
                acc = fmaf(h4.z, xw[-j - 2], acc);
                acc = fmaf(h4.w, xw[-j - 3], acc);
            }
            for (; j < T; ++j) acc = fmaf(hp[j], xw[-j], acc);
        } else {
            for (int j = 0; j < T; ++j) {
                const long long i = i0 - j;
                const float xv = (i >= 0 && i < L) ? load_src(src, fmt, channels, chan, in0 + i) : 0.0f;
                acc = fmaf(hp[j], xv, acc);
            }
        }
        out[o0 + n] = gain * acc;
    }
}

__global__ void __launch_bounds__(THREADS) assemble_clips_kernel(const float* __restrict__ pool, const long long* __restrict__ seg,
                                                                 const int* __restrict__ seg_first, int tiles_per_clip, int L,
                                                                 float* __restrict__ out) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_clip, j0 = (blockIdx.x % tiles_per_clip) * TILE;
    const int j1 = min(j0 + TILE, L);
    const int s1 = seg_first[b + 1];
    float v[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) v[r] = 0.0f;                         // the silence gaps, and everything past the last segment
    for (int s = seg_first[b]; s < s1; ++s) {                          // ascending in dst: all conditions are workgroup-uniform
        const long long src = seg[3 * (size_t)s];
        const int dst = (int)seg[3 * (size_t)s + 1], len = (int)seg[3 * (size_t)s + 2];
        if (dst + len <= j0) continue;
        if (dst >= j1) break;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int j = j0 + tid + r * THREADS;
            if (j >= dst && j < dst + len) v[r] = pool[src + (j - dst)];
        }
    }
    float* ob = out + (size_t)b * L;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int j = j0 + tid + r * THREADS;
        if (j < j1) ob[j] = v[r];
    }
}

long long gcdll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

}  // namespace

extern "C" int cruse_resample_poly(const void* src, int fmt, int channels, int chan, const long long* off_in_host, const long long* off_out_host,
                                   const long long* off_in, const long long* off_out, int B, int up, int down, const float* taps, int ntap,
                                   int tap_stride, float* out, void* stream) {
    CRUSE_REQUIRE(src && off_in_host && off_out_host && off_in && off_out && out, CRUSE_E_SHAPE, "resample_poly: null buffer");
    CRUSE_REQUIRE(B >= 1, CRUSE_E_SHAPE, "resample_poly: B = %d", B);
    CRUSE_REQUIRE(up >= 1 && down >= 1 && up <= MAX_RATIO && down <= MAX_RATIO, CRUSE_E_SHAPE, "resample_poly: up = %d, down = %d must lie in 1..%d",
                  up, down, MAX_RATIO);
    CRUSE_REQUIRE(gcdll(up, down) == 1, CRUSE_E_SHAPE, "resample_poly: up = %d, down = %d are not reduced", up, down);
    CRUSE_REQUIRE(fmt == FMT_F32 || fmt == FMT_S16, CRUSE_E_SHAPE, "resample_poly: unknown sample format %d", fmt);
    CRUSE_REQUIRE(channels >= 1 && channels <= 1024 && chan >= 0 && chan < channels, CRUSE_E_SHAPE, "resample_poly: channel %d of %d", chan, channels);
    CRUSE_REQUIRE(fmt == FMT_S16 || channels == 1, CRUSE_E_SHAPE, "resample_poly: f32 input is mono, channels = %d", channels);
    const bool copy = up == 1 && down == 1;
    const int q = up > down ? up : down, T = copy ? 0 : (32 * q + 1 + up - 1) / up;
    if (!copy) {
        CRUSE_REQUIRE(taps, CRUSE_E_SHAPE, "resample_poly: null tap table");
        CRUSE_REQUIRE(ntap == 32 * q + 1, CRUSE_E_SHAPE, "resample_poly: %d taps, expected 32 * %d + 1", ntap, q);
        CRUSE_REQUIRE(tap_stride >= T && tap_stride % 4 == 0, CRUSE_E_SHAPE, "resample_poly: tap_stride = %d, expected a multiple of 4 >= %d", tap_stride, T);
        CRUSE_REQUIRE(((uintptr_t)taps & 15) == 0, CRUSE_E_ALIGN, "resample_poly: tap table not 16-byte aligned");
    }
    CRUSE_REQUIRE(off_in_host[0] >= 0 && off_out_host[0] >= 0, CRUSE_E_SHAPE, "resample_poly: negative first offset");
    long long max_out = 0;
    for (int b = 0; b < B; ++b) {
        const long long L = off_in_host[b + 1] - off_in_host[b], Lout = off_out_host[b + 1] - off_out_host[b];
        CRUSE_REQUIRE(L >= 1 && L <= MAX_LEN, CRUSE_E_SHAPE, "resample_poly: clip %d has %lld input samples", b, L);
        CRUSE_REQUIRE(Lout == (L * up + down - 1) / down && Lout <= MAX_LEN, CRUSE_E_SHAPE,
                      "resample_poly: clip %d: %lld outputs for %lld inputs at %d / %d", b, Lout, L, up, down);
        if (Lout > max_out) max_out = Lout;
    }
    CRUSE_REQUIRE(off_in_host[B] <= (1ll << 50) && off_out_host[B] <= (1ll << 50), CRUSE_E_SHAPE, "resample_poly: offsets beyond 2^50");
    const long long tpc = cdivl(max_out, TILE), blocks = tpc * B;
    CRUSE_REQUIRE(blocks <= 0x7fffffffll, CRUSE_E_SHAPE, "resample_poly: %lld workgroups", blocks);
    if (copy) {
        hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, src, fmt, channels, chan, off_in, off_out,
                           (int)tpc, out);
    } else {
        const int staged = ((long long)(TILE - 1) * down) / up + T + 2 <= WIN_MAX;
        hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, src, fmt, channels, chan, off_in, off_out,
                           (int)tpc, up, down, 16 * q, T, tap_stride, taps, staged, out);
    }
    CRUSE_LAUNCH_CHECK("cruse_resample_poly");
    return CRUSE_OK;
}

extern "C" int cruse_assemble_clips(const float* pool, const long long* seg, const int* seg_first, int nseg, int B, int L, float* out, void* stream) {
    CRUSE_REQUIRE(pool && seg_first && out && (seg || nseg == 0), CRUSE_E_SHAPE, "assemble_clips: null buffer");
    CRUSE_REQUIRE(B >= 1 && L >= 1 && nseg >= 0 && L <= MAX_LEN, CRUSE_E_SHAPE, "assemble_clips: B = %d, L = %d, nseg = %d", B, L, nseg);
    const long long tpc = cdivl(L, TILE), blocks = tpc * B;
    CRUSE_REQUIRE(blocks <= 0x7fffffffll, CRUSE_E_SHAPE, "assemble_clips: %lld workgroups", blocks);
    hipLaunchKernelGGL(assemble_clips_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, pool, seg, seg_first, (int)tpc, L, out);
    CRUSE_LAUNCH_CHECK("cruse_assemble_clips");
    return CRUSE_OK;
}
