// Sample-rate conversion at the boundary of the streaming chains (cruse_stream_resample_*): the server's I/O at 8 / 32 / 48 kHz
// around the 16 kHz kernels of stream.hip, which this file neither includes nor changes.  One polyphase-free FIR per side, with
// q = 2 (8 k, 32 k) or 3 (48 k) and N = 32 q + 1 taps h (a Kaiser-windowed sinc, designed on the host and read from `taps`):
//   decimate by q, phase 0:  D_q(u)[n] = sum_{k=0}^{N-1} h[k] u[q n - k]                     (history: N - 1 input samples)
//   interpolate by q:        I_q(x)[m] = q sum_i h[m - q i] x[i],  0 <= m - q i <= N - 1      (history: (N - 1) / q input samples)
// Both causal with zero initial history; sums run over k (respectively i) ascending, fmaf, f32.  32 k / 48 k: D_q on the input side,
// I_q on the output side; 8 k: I_2 on the input side, D_2 on the output side.
//
// One workgroup per slot.  A slot's blocks are walked one after the other with [history | block] and the taps in LDS, so a packet
// carries the history from block to block inside the workgroup and gives the bits of as many single hops.
#include <type_traits>
#include "stream_common.h"

namespace {

using namespace cruse_stream;

constexpr int HOP = 160;                  // a 16 kHz block
constexpr int RS_THREADS = 256;
constexpr int TAPS_PAD = 100;             // N = 97 at q = 3, padded
constexpr int MAX_HIST = 96;              // N - 1 at q = 3
constexpr int MAX_BLOCK = 480;            // 10 ms at 48 kHz
enum { SIDE_IN = 0, SIDE_OUT = 1 };

// The sample formats of DESIGN 12c.  ld_sample / st_sample live in stream.hip, which stays as it is: the two one-liners are restated.
__device__ __forceinline__ float ld_sample(const float* p, int i) { return p[i]; }
__device__ __forceinline__ float ld_sample(const short* p, int i) { return (float)p[i] / 32768.0f; }      // exact

// stores y; true where a PCM sample was clamped: clamp(rint(y * 32768), -32768, 32767), ties to even
__device__ __forceinline__ bool st_sample(float* p, int i, float y) {
    p[i] = y;
    return false;
}
__device__ __forceinline__ bool st_sample(short* p, int i, float y) {
    const float r = rintf(y * 32768.0f);
    const float c = fminf(fmaxf(r, -32768.0f), 32767.0f);
    p[i] = (short)__float2int_rn(c);
    return c != r;
}

struct RsArgs {
    const int* ctl;            // single hop: the main chain's mode[S]; packets: pk[2][S]
    int S, hops;               // hops = 0: single hop
    int side;                  // SIDE_IN / SIDE_OUT
    int q, N;                  // rate ratio, taps
    int nin, nout, H;          // samples of an input / output block of this side, history samples
    const float* taps;         // h[N]
    float* hist;               // slot 0's history of this side; rs_stride floats between slots
    int rs_stride;
    const void* in;            // [S][stride_blocks][nin]
    void* out;                 // [S][stride_blocks][nout]
    int stride_blocks;         // blocks between two slots' rows of `in` and of `out`
    int* clip;                 // [S] or null
};

// blocks slot s converts in this launch
__device__ __forceinline__ int blocks_of(const RsArgs& a, int s) {
    if (a.hops == 0) {
        const int m = a.ctl[s];
        if (a.side == SIDE_IN) return m == CRUSE_STREAM_MODE_STORE || m == CRUSE_STREAM_MODE_FRAME;
        return m == CRUSE_STREAM_MODE_FRAME || m == CRUSE_STREAM_MODE_END;
    }
    const Pkt p = packet_of(a.ctl, a.S, s, a.hops);
    return a.side == SIDE_IN ? p.c : max(p.nf - p.f0, 0);              // frame 0 of a clip yields no output block
}

template <typename IN, typename OUT, bool DECIM>
__global__ void __launch_bounds__(RS_THREADS) stream_rs_kernel(RsArgs a) {
    __shared__ float h[TAPS_PAD];
    __shared__ float buf[MAX_HIST + MAX_BLOCK];
    __shared__ float red[RS_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nb = blocks_of(a, s);
    if (nb == 0) return;                                               // inactive / SKIP: history and output untouched
    const int q = a.q, N = a.N, H = a.H, nin = a.nin, nout = a.nout;
    float* hist = a.hist + (size_t)s * a.rs_stride;
    const IN* in = (const IN*)a.in + (size_t)s * a.stride_blocks * nin;
    OUT* out = (OUT*)a.out + (size_t)s * a.stride_blocks * nout;
    for (int i = tid; i < N; i += RS_THREADS) h[i] = a.taps[i];
    if (tid < H) buf[tid] = hist[tid];
    int nclip = 0;
    for (int b = 0; b < nb; ++b) {
        for (int i = tid; i < nin; i += RS_THREADS) buf[H + i] = ld_sample(in + (size_t)b * nin, i);
        __syncthreads();
        for (int m = tid; m < nout; m += RS_THREADS) {
            float acc = 0.f;
            if (DECIM) {                                               // H = N - 1: the oldest sample read is buf[q m]
                const float* u = buf + H + q * m;
                for (int k = 0; k < N; ++k) acc = fmaf(h[k], u[-k], acc);
            } else {                                                   // H = (N - 1) / q: i from ihi - jmax >= -H
                const int ihi = m / q, r = m - q * ihi, jmax = (N - 1 - r) / q;
                const float* x = buf + H + ihi;
                for (int j = jmax; j >= 0; --j) acc = fmaf(h[r + q * j], x[-j], acc);
                acc *= (float)q;
            }
            nclip += st_sample(out + (size_t)b * nout, m, acc);
        }
        __syncthreads();
        if (tid < H) buf[tid] = buf[nin + tid];                        // nin >= H: the two ranges are disjoint
        __syncthreads();
    }
    if (tid < H) hist[tid] = buf[tid];
    if constexpr (!std::is_same<OUT, float>::value) {
        // clip[s] += the samples this launch clamped.  One workgroup per slot and launch, launches ordered: a plain store.
        if (a.clip != nullptr) {
            const float n = wave_sum((float)nclip);                    // at most a few thousand: exact in f32
            if ((tid & 63) == 0) red[tid >> 6] = n;
            __syncthreads();
            if (tid == 0) {
                float t = 0.f;
                for (int w = 0; w < RS_THREADS / 64; ++w) t += red[w];
                a.clip[s] += (int)t;
            }
        }
    }
}

template <typename IN, typename OUT>
int launch(const RsArgs& a, bool decim, const char* name, void* stream) {
    if (decim) hipLaunchKernelGGL((stream_rs_kernel<IN, OUT, true>), dim3(a.S), dim3(RS_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((stream_rs_kernel<IN, OUT, false>), dim3(a.S), dim3(RS_THREADS), 0, (hipStream_t)stream, a);
    CRUSE_LAUNCH_CHECK(name);
    return CRUSE_OK;
}

// every check of the four entry points, before any launch; hops = 0: single hop
int resample_any(const char* who, const char* name, int side, const int* ctl, int S, int hops, int stride_blocks, int io_rate,
                 const void* in, const float* taps, float* rs_state, int rs_stride, void* out, int fmt, int* clip, void* stream) {
    CRUSE_REQUIRE(S > 0 && ctl && in && taps && rs_state && out, CRUSE_E_SHAPE, "%s: S = %d or a null buffer", who, S);
    CRUSE_REQUIRE(io_rate == 8000 || io_rate == 32000 || io_rate == 48000, CRUSE_E_SHAPE,
                  "%s: unknown io_rate %d (8000, 32000 or 48000; 16000 needs no resampling)", who, io_rate);
    const int rc = side == SIDE_OUT ? out_args(who, fmt, clip) : fmt_args(who, fmt);
    if (rc) return rc;
    if (hops != 0) {
        CRUSE_REQUIRE(hops >= 1, CRUSE_E_SHAPE, "%s: hops = %d", who, hops);
        CRUSE_REQUIRE(stride_blocks >= hops, CRUSE_E_SHAPE, "%s: %s = %d < hops = %d", who, side == SIDE_IN ? "in_hops" : "out_hops",
                      stride_blocks, hops);
    }
    const int q = io_rate == 48000 ? 3 : 2, N = 32 * q + 1, B = io_rate / 100;
    const bool up = io_rate < 16000;                                   // 8 k: interpolate in, decimate out
    const int h_in = up ? (N - 1) / q : N - 1, h_out = up ? N - 1 : (N - 1) / q;
    CRUSE_REQUIRE(rs_stride >= h_in + h_out, CRUSE_E_SHAPE, "%s: rs_stride = %d < %d + %d history samples of io_rate %d", who, rs_stride,
                  h_in, h_out, io_rate);
    RsArgs a;
    a.ctl = ctl; a.S = S; a.hops = hops; a.side = side; a.q = q; a.N = N;
    a.nin = side == SIDE_IN ? B : HOP; a.nout = side == SIDE_IN ? HOP : B;
    a.H = side == SIDE_IN ? h_in : h_out;
    a.taps = taps;
    a.hist = rs_state + (side == SIDE_IN ? 0 : h_in); a.rs_stride = rs_stride;
    a.in = in; a.out = out; a.stride_blocks = hops == 0 ? 1 : stride_blocks;
    a.clip = clip;
    const bool decim = (side == SIDE_IN) != up;
    if (side == SIDE_IN) return fmt == FMT_S16 ? launch<short, float>(a, decim, name, stream) : launch<float, float>(a, decim, name, stream);
    return fmt == FMT_S16 ? launch<float, short>(a, decim, name, stream) : launch<float, float>(a, decim, name, stream);
}

}  // namespace

extern "C" int cruse_stream_resample_in(const int* mode, int S, int io_rate, const void* in, int in_fmt, const float* taps, float* rs_state,
                                        int rs_stride, float* blocks, void* stream) {
    return resample_any("stream_resample_in", "cruse_stream_resample_in", SIDE_IN, mode, S, 0, 1, io_rate, in, taps, rs_state, rs_stride, blocks,
                        in_fmt, nullptr, stream);
}

extern "C" int cruse_stream_resample_out(const int* mode, int S, int io_rate, const float* out16, const float* taps, float* rs_state,
                                         int rs_stride, void* out, int out_fmt, int* clip, void* stream) {
    return resample_any("stream_resample_out", "cruse_stream_resample_out", SIDE_OUT, mode, S, 0, 1, io_rate, out16, taps, rs_state, rs_stride,
                        out, out_fmt, clip, stream);
}

extern "C" int cruse_stream_resample_in_n(const int* pk, int S, int hops, int in_hops, int io_rate, const void* in, int in_fmt,
                                          const float* taps, float* rs_state, int rs_stride, float* blocks, void* stream) {
    CRUSE_REQUIRE(hops >= 1, CRUSE_E_SHAPE, "stream_resample_in_n: hops = %d", hops);
    return resample_any("stream_resample_in_n", "cruse_stream_resample_in_n", SIDE_IN, pk, S, hops, in_hops, io_rate, in, taps, rs_state,
                        rs_stride, blocks, in_fmt, nullptr, stream);
}

extern "C" int cruse_stream_resample_out_n(const int* pk, int S, int hops, int out_hops, int io_rate, const float* out16, const float* taps,
                                           float* rs_state, int rs_stride, void* out, int out_fmt, int* clip, void* stream) {
    CRUSE_REQUIRE(hops >= 1, CRUSE_E_SHAPE, "stream_resample_out_n: hops = %d", hops);
    return resample_any("stream_resample_out_n", "cruse_stream_resample_out_n", SIDE_OUT, pk, S, hops, out_hops, io_rate, out16, taps,
                        rs_state, rs_stride, out, out_fmt, clip, stream);
}
