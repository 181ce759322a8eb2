// Frame-by-frame streaming inference of unet_2 (n_fft = win = 320, hop = 160): one hop of every active slot is
// encode -> GRU layer 1 -> GRU layer 2 -> decode, four dependent launches on one stream (cruse_stream_* in cruse_hip.h).
//
// The model is causal in time: the encoder convs are (2,3) with time padding 1 and the trailing frame cropped, so frame t
// reads input rows t-1 and t of each level (the previous row is per-slot state); skip and decoder convs are (1,3); both
// GRU layers are uni-directional; eval-mode BatchNorm is a per-channel affine, folded into the conv weights by the host.
// All arithmetic is f32 with f32 accumulation.  Every kernel reads the per-slot mode (CRUSE_STREAM_MODE_*) from device
// memory; a slot whose mode is SKIP is not touched.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <mutex>
#include <tuple>
#include <type_traits>
#include "postfilter.h"
#include "stream_common.h"

namespace {

using namespace cruse_stream;

constexpr int NFFT = 320, HOP = 160, NB = 161, F0 = 160;
// one workgroup per slot in encode / decode: 16 waves, so that the per-slot chain of small convolutions has enough loads in
// flight (256 threads: 174 / 81 us per launch, latency-bound on the weight loads)
constexpr int FRAME_THREADS = 1024;

// the layout of cruse_stream_layout(): all ints, in the order of the header's description
struct Layout {
    int ch[5], F[5], H;
    int encW[5], encB[5], skW[5], decW[5], decB[5], ln1g, ln1b, ln2g, ln2b, wtotal;
    int st_hist, st_tail, st_prev[4], st_h1, st_h2, st_stride;
    int wk_re, wk_im, wk_x, wk_skip[5], wk_h1n, wk_h2n, wk_mask, wk_stride;
};
static_assert(sizeof(Layout) == CRUSE_STREAM_LAYOUT_INTS * sizeof(int), "layout size");

int make_layout(int c0, int c1, int c2, int c3, int c4, Layout& L) {
    const int c[5] = {c0, c1, c2, c3, c4};
    memset(&L, 0, sizeof(L));
    for (int k = 0; k < 5; ++k) {
        CRUSE_REQUIRE(c[k] > 0 && c[k] <= 512, CRUSE_E_SHAPE, "stream: channel count ch[%d] = %d out of range", k, c[k]);
        L.ch[k] = c[k];
        L.F[k] = F0 >> k;
    }
    CRUSE_REQUIRE(c0 == 1, CRUSE_E_SHAPE, "stream: ch[0] must be 1 (magnitude input), got %d", c0);
    for (int k = 1; k < 5; ++k)
        CRUSE_REQUIRE(L.ch[k] * L.F[k] <= 2048, CRUSE_E_SHAPE, "stream: level %d row of %d floats exceeds 2048", k, L.ch[k] * L.F[k]);
    L.H = L.ch[4] * L.F[4];
    int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    for (int k = 1; k < 5; ++k) {
        L.encW[k] = take(L.ch[k] * L.ch[k - 1] * 6);
        L.encB[k] = take(L.ch[k]);
        L.skW[k] = take(L.ch[k] * L.ch[k] * 3);
    }
    for (int k = 4; k >= 1; --k) {
        L.decW[k] = take(L.ch[k] * L.ch[k - 1] * 3);
        L.decB[k] = take(L.ch[k - 1]);
    }
    L.ln1g = take(L.H); L.ln1b = take(L.H); L.ln2g = take(L.H); L.ln2b = take(L.H);
    L.wtotal = o;
    o = 0;
    L.st_hist = take(NB);
    L.st_tail = take(HOP);
    for (int k = 0; k < 4; ++k) L.st_prev[k] = take(L.ch[k] * L.F[k]);
    L.st_h1 = take(L.H);
    L.st_h2 = take(L.H);
    L.st_stride = o;
    o = 0;
    L.wk_re = take(NB);
    L.wk_im = take(NB);
    L.wk_x = take(L.H);
    for (int k = 1; k < 5; ++k) L.wk_skip[k] = take(L.ch[k] * L.F[k]);
    L.wk_h1n = take(L.H);
    L.wk_h2n = take(L.H);
    L.wk_mask = take(F0);
    L.wk_stride = o;
    return CRUSE_OK;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// ---- the sample formats of the I/O forms (cruse_stream_*_io): the boundary kernels are templates on the element type of `in` / `out`,
// float or short (16-bit PCM), and decode on LIM (the per-slot attenuation limit).  <float> / <float, false> are what the plain entry
// points launch; every form shares all arithmetic between the load of a sample and the store of one.
__device__ __forceinline__ float ld_sample(const float* p, int i) { return p[i]; }
__device__ __forceinline__ float ld_sample(const short* p, int i) { return (float)p[i] / 32768.0f; }      // exact

// stores y; true where a PCM sample was clamped: clamp(rint(y * 32768), -32768, 32767), ties to even
__device__ __forceinline__ bool st_sample(float* p, size_t i, float y) {
    p[i] = y;
    return false;
}
__device__ __forceinline__ bool st_sample(short* p, size_t i, float y) {
    const float r = rintf(y * 32768.0f);
    const float c = fminf(fmaxf(r, -32768.0f), 32767.0f);
    p[i] = (short)__float2int_rn(c);
    return c != r;
}

// clip[s] += the samples this launch clamped for slot s.  One workgroup per slot and launch, launches ordered: a plain store.
__device__ __forceinline__ void count_clipped(int* __restrict__ clip, int s, int mine, float* red) {
    if (clip == nullptr) return;                          // uniform over the workgroup
    const float n = block_sum((float)mine, red);          // at most a few thousand: exact in f32
    if (threadIdx.x == 0) clip[s] += (int)n;
}

// The convolutions run over the nf frames of a packet (nf = 1: the single hop); frame f's rows are fs floats apart.  Weight rows are ws
// floats apart: the packed stride from global memory (single hop), one more in the padded LDS copy of the packet kernels.  The helpers
// are inlined, so the single hop's literal nf = 1 folds the frame index away.

// level-k encoder conv (2,3), stride (1,2), frequency padding 1, BN folded, ReLU: dst[f][co][fo] from input rows [Cin][Fin] f-1 and f
// of src; row -1 is `prev`.  W: [Cout][ws], ws >= Cin*6
__device__ __forceinline__ void enc_conv(const float* __restrict__ W, int ws, const float* __restrict__ b, const float* prev, const float* src, float* dst, int fs,
                                         int nf, int Cin, int Fin, int Cout, int Fout) {
    const int per = Cout * Fout;
    for (int idx = threadIdx.x; idx < nf * per; idx += blockDim.x) {
        const int f = nf == 1 ? 0 : idx / per, r = idx - f * per, co = r / Fout, fo = r - co * Fout;
        const float* pr = f == 0 ? prev : src + (f - 1) * fs;
        const float* cu = src + f * fs;
        float acc = b[co];
        for (int ci = 0; ci < Cin; ++ci) {
            const float* w = W + co * ws + ci * 6;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int fi = 2 * fo - 1 + kw;
                if (fi < 0 || fi >= Fin) continue;
                acc = fmaf(w[kw], pr[ci * Fin + fi], acc);
                acc = fmaf(w[3 + kw], cu[ci * Fin + fi], acc);
            }
        }
        dst[f * fs + r] = fmaxf(acc, 0.f);
    }
}

// skip conv (1,3), padding (0,1), no bias: [C][F] -> [C][F]; frame f's result goes to out + f * os.  W: [C][ws], ws >= C*3
__device__ __forceinline__ void skip_conv(const float* __restrict__ W, int ws, const float* src, int fs, float* out, size_t os, int nf, int C, int F) {
    const int per = C * F;
    for (int idx = threadIdx.x; idx < nf * per; idx += blockDim.x) {
        const int f = nf == 1 ? 0 : idx / per, r = idx - f * per, co = r / F, fo = r - co * F;
        const float* e = src + f * fs;
        float acc = 0.f;
        for (int ci = 0; ci < C; ++ci) {
            const float* w = W + co * ws + ci * 3;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int fi = fo - 1 + kw;
                if (fi >= 0 && fi < F) acc = fmaf(w[kw], e[ci * F + fi], acc);
            }
        }
        out[f * os + r] = acc;
    }
}

// ConvTranspose (1,3), stride (1,2), last column cropped: [Cin][Fin] -> [Cout][2*Fin]; W packed [Cin][Cout][3] (BN folded)
// act 0: ReLU then + add[f * as + co*Fout + fo] (the frame's skip row); act 1: sigmoid
__device__ __forceinline__ void dec_convt(const float* __restrict__ W, const float* __restrict__ b, const float* src, float* dst, int fs,
                                          const float* __restrict__ add, size_t as,
                                          int nf, int Cin, int Fin, int Cout, int act) {
    const int Fout = 2 * Fin, per = Cout * Fout;
    for (int idx = threadIdx.x; idx < nf * per; idx += blockDim.x) {
        const int f = nf == 1 ? 0 : idx / per, r = idx - f * per, co = r / Fout, fo = r - co * Fout;
        const float* in = src + f * fs;
        const int fi = fo >> 1;
        float acc = b[co];
        if (fo & 1) {
            for (int ci = 0; ci < Cin; ++ci) acc = fmaf(W[(ci * Cout + co) * 3 + 1], in[ci * Fin + fi], acc);
        } else {
            for (int ci = 0; ci < Cin; ++ci) {
                acc = fmaf(W[(ci * Cout + co) * 3 + 0], in[ci * Fin + fi], acc);
                if (fi >= 1) acc = fmaf(W[(ci * Cout + co) * 3 + 2], in[ci * Fin + fi - 1], acc);
            }
        }
        dst[f * fs + r] = act == 0 ? fmaxf(acc, 0.f) + add[f * as + r] : 1.0f / (1.0f + expf(-acc));
    }
}

// nearest x2 FreqUpsample + Conv2d (1,3), padding (0,1) (cust_conv.py:163-166,177-184): [Cin][Fin] -> [Cout][2*Fin]; W packed
// [Cout][Cin][3], the Conv2d order (BN folded).  With u[i] = in[i >> 1] the taps of column fo are u[fo-1], u[fo], u[fo+1]: rows
// (j-1, j, j) of `in` for fo = 2j and (j, j, j+1) for fo = 2j+1; u[-1] and u[2*Fin] are the zero padding.  Three FMAs per input
// channel in tap order, the order of the conv on the upsampled row.  act as dec_convt
__device__ __forceinline__ void dec_upconv(const float* __restrict__ W, const float* __restrict__ b, const float* src, float* dst, int fs,
                                           const float* __restrict__ add, size_t as,
                                           int nf, int Cin, int Fin, int Cout, int act) {
    const int Fout = 2 * Fin, per = Cout * Fout;
    for (int idx = threadIdx.x; idx < nf * per; idx += blockDim.x) {
        const int f = nf == 1 ? 0 : idx / per, r = idx - f * per, co = r / Fout, fo = r - co * Fout;
        const float* in = src + f * fs;
        const float* w = W + co * Cin * 3;
        const bool left = fo >= 1, right = fo + 1 < Fout;
        const int lo = left ? (fo - 1) >> 1 : 0, mid = fo >> 1, hi = right ? (fo + 1) >> 1 : 0;
        float acc = b[co];
        for (int ci = 0; ci < Cin; ++ci) {
            const float* x = in + ci * Fin;
            if (left) acc = fmaf(w[ci * 3 + 0], x[lo], acc);
            acc = fmaf(w[ci * 3 + 1], x[mid], acc);
            if (right) acc = fmaf(w[ci * 3 + 2], x[hi], acc);
        }
        dst[f * fs + r] = act == 0 ? fmaxf(acc, 0.f) + add[f * as + r] : 1.0f / (1.0f + expf(-acc));
    }
}

// the decoder of the decode kernels: the ConvTranspose levels of unet_2 or the upsample levels of CRUSE4MagAddSkipUpsample
enum { DEC_CONVT = 0, DEC_UPCONV = 1 };

template <int DEC>
__device__ __forceinline__ void dec_level(const float* __restrict__ W, const float* __restrict__ b, const float* src, float* dst, int fs,
                                          const float* __restrict__ add, size_t as, int nf, int Cin, int Fin, int Cout, int act) {
    if constexpr (DEC == DEC_UPCONV) dec_upconv(W, b, src, dst, fs, add, as, nf, Cin, Fin, Cout, act);
    else dec_convt(W, b, src, dst, fs, add, as, nf, Cin, Fin, Cout, act);
}

// tables: [0,320) periodic Hann, [320,640) cos(2 pi j / 320), [640,960) sin(2 pi j / 320), [960,1120) 1 / (w^2(m) + w^2(m+160))
constexpr int TB_WIN = 0, TB_COS = 320, TB_SIN = 640, TB_IENV = 960, TB_TOTAL = 1120;

// bin k of the 320-point real DFT of fr[320]; cs: cos[320] | sin[320] (tab + TB_COS, or its LDS copy)
__device__ __forceinline__ void rdft320(const float* fr, const float* cs, int k, float& re, float& im) {
    re = 0.f;
    im = 0.f;
    int j = 0;
    for (int n = 0; n < NFFT; ++n) {
        re = fmaf(fr[n], cs[j], re);
        im = fmaf(-fr[n], cs[NFFT + j], im);
        j += k;
        if (j >= NFFT) j -= NFFT;
    }
}

// sample n of the 320-point inverse real DFT of re[161], im[161] (imaginary parts of bins 0 and 160 ignored, as irfft)
__device__ __forceinline__ float irdft320(const float* re, const float* im, const float* cs, int n) {
    float acc = 0.f;
    int j = n;
    for (int k = 1; k < F0; ++k) {
        acc = fmaf(re[k], cs[j], acc);
        acc = fmaf(-im[k], cs[NFFT + j], acc);
        j += n;
        if (j >= NFFT) j -= NFFT;
    }
    return (re[0] + 2.0f * acc + ((n & 1) ? -re[F0] : re[F0])) * (1.0f / NFFT);
}

template <typename IN>
__global__ void __launch_bounds__(1024) stream_encode_kernel(const int* __restrict__ mode, Layout L, const IN* __restrict__ in,
                                                            const float* __restrict__ tab, const float* __restrict__ w,
                                                            float* __restrict__ state, float* __restrict__ work) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, m = mode[s];
    if (m == CRUSE_STREAM_MODE_SKIP) return;
    float* st = state + (size_t)s * L.st_stride;
    float* wk = work + (size_t)s * L.wk_stride;
    const IN* blk = in + (size_t)s * HOP;
    const int tid = threadIdx.x;
    if (m == CRUSE_STREAM_MODE_STORE) {
        for (int i = tid; i < HOP; i += blockDim.x) st[L.st_hist + 1 + i] = ld_sample(blk, i);
        return;
    }
    // LDS: frame[320] | rows of levels 0..4 (current) | previous rows of levels 0..3 | re[161] | im[161]
    float* fr = sm;
    float* cur[5];
    float* prv[4];
    int o = NFFT;
    for (int k = 0; k < 5; ++k) { cur[k] = sm + o; o += L.ch[k] * L.F[k]; }
    for (int k = 0; k < 4; ++k) { prv[k] = sm + o; o += L.ch[k] * L.F[k]; }
    float* spec = sm + o;     // re[161] | im[161]
    o += 2 * NB;
    // frame assembly (hist[0] = the sample before the last stored block, hist[1..160] = that block)
    const float* hist = st + L.st_hist;
    for (int i = tid; i < HOP; i += blockDim.x) {
        float a, bq;
        if (m == CRUSE_STREAM_MODE_FRAME0) {          // x[160], x[159], ..., x[1] | x[0..159]
            a = i == 0 ? ld_sample(blk, 0) : hist[161 - i];
            bq = hist[1 + i];
        } else if (m == CRUSE_STREAM_MODE_END) {      // last block | x[L-2], ..., x[L-161]
            a = hist[1 + i];
            bq = hist[159 - i];
        } else {                                      // previous block | this block
            a = hist[1 + i];
            bq = ld_sample(blk, i);
        }
        fr[i] = a * tab[TB_WIN + i];
        fr[HOP + i] = bq * tab[TB_WIN + HOP + i];
    }
    for (int k = 0; k < 4; ++k)
        for (int i = tid; i < L.ch[k] * L.F[k]; i += blockDim.x) prv[k][i] = st[L.st_prev[k] + i];
    __syncthreads();
    if (m == CRUSE_STREAM_MODE_FRAME) {               // history: the last sample of the old block, then this block
        const float last = hist[HOP];
        __syncthreads();
        if (tid == 0) st[L.st_hist] = last;
        for (int i = tid; i < HOP; i += blockDim.x) st[L.st_hist + 1 + i] = ld_sample(blk, i);
    }
    // 320-point real DFT, bins 0..160; magnitude of bins 0..159
    for (int k = tid; k < NB; k += blockDim.x) {
        float re, im;
        rdft320(fr, tab + TB_COS, k, re, im);
        spec[k] = re;
        spec[NB + k] = im;
        wk[L.wk_re + k] = re;
        wk[L.wk_im + k] = im;
        if (k < F0) cur[0][k] = sqrtf(re * re + im * im + 1e-8f);
    }
    __syncthreads();
    for (int k = 1; k < 5; ++k) {
        enc_conv(w + L.encW[k], L.ch[k - 1] * 6, w + L.encB[k], prv[k - 1], cur[k - 1], cur[k], 0, 1, L.ch[k - 1], L.F[k - 1], L.ch[k], L.F[k]);
        __syncthreads();
    }
    for (int k = 1; k < 5; ++k) skip_conv(w + L.skW[k], L.ch[k] * 3, cur[k], 0, wk + L.wk_skip[k], 0, 1, L.ch[k], L.F[k]);
    for (int i = tid; i < L.H; i += blockDim.x) wk[L.wk_x + i] = cur[4][i];        // GRU input row, c*F4+f
    for (int k = 0; k < 4; ++k)
        for (int i = tid; i < L.ch[k] * L.F[k]; i += blockDim.x) st[L.st_prev[k] + i] = cur[k][i];
}

// One GGRU layer over the rows of GruArgs (stream_common.h), in three kinds.  STEP: one time step for every slot whose mode computes a
// frame.  PROJ: gi[row] = W_ih . x + bias for every (slot, frame) of a packet, with b_ih + b_hh folded for the gates r and z and b_in
// for n; rows behind a slot's last frame are not computed.  REC: frame `frame` of the packet for every slot that computes it: W_hh . h,
// gates, new h into the frame's work row.  Workgroup: 4 waves, wave w owns hidden unit blockIdx.y*4 + w (all three gates); its lanes
// hold that unit's weight rows (W_ih and / or W_hh x r,z,n) in registers, k = lane + 64q, and loop over tiles of SB rows whose input /
// state chunks are staged in LDS.  Layer 2 (ln_g != nullptr) stages the whole layer-1 output row and applies LN1 to the interleaved
// vector v[j*g+i] = h1[i*Hg+j] on the fly.  A kind holds only the registers and LDS regions it uses.
constexpr int SB = 8;

template <int KIND, int KQ>
__global__ void __launch_bounds__(256) stream_gru_f32_kernel(GruArgs a) {
    extern __shared__ float sm[];
    constexpr bool HAS_X = KIND != KIND_REC, HAS_H = KIND != KIND_PROJ;
    constexpr int XQ = HAS_X ? KQ : 1, HQ = HAS_H ? KQ : 1;
    const int g = a.g, Hg = a.Hg, H = g * Hg;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.y * 4 + wv;          // unit of the whole layer: group gidx, unit j within it
    const int gidx = u / Hg, j = u - gidx * Hg;
    const bool ln = HAS_X && a.ln_g != nullptr;
    const int xw = HAS_X ? (ln ? H : Hg) : 0;   // floats staged per row for the input
    float* xs = sm;                             // [SB][xw]
    float* hs = sm + SB * xw;                   // [SB][Hg]
    float* st = hs + (HAS_H ? SB * Hg : 0);     // [SB][2] mean, rstd
    const size_t gsz = (size_t)3 * Hg * Hg;
    const float* Wih = a.pack + gidx * gsz;
    const float* Whh = a.pack + g * gsz + gidx * gsz;
    const float* bih = a.pack + 2 * g * gsz + gidx * 3 * Hg;
    const float* bhh = a.pack + 2 * g * gsz + g * 3 * Hg + gidx * 3 * Hg;
    float wi[3][XQ], wh[3][HQ], lg[XQ], lb[XQ];
    int src[XQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = lane + 64 * q;
        const bool ok = k < Hg;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (HAS_X) wi[c][q] = ok ? Wih[(size_t)(c * Hg + j) * Hg + k] : 0.f;
            if constexpr (HAS_H) wh[c][q] = ok ? Whh[(size_t)(c * Hg + j) * Hg + k] : 0.f;
        }
        if constexpr (HAS_X) {
            const int p = gidx * Hg + k;          // position in the LN1 output vector this layer-2 group reads
            src[q] = ok ? (ln ? (p % g) * Hg + p / g : k) : 0;
            lg[q] = (ln && ok) ? a.ln_g[p] : 0.f;
            lb[q] = (ln && ok) ? a.ln_b[p] : 0.f;
        }
    }
    float br = 0.f, bz = 0.f, bin = 0.f, bhn = 0.f;
    if constexpr (HAS_X) { br = bih[j] + bhh[j]; bz = bih[Hg + j] + bhh[Hg + j]; bin = bih[2 * Hg + j]; }
    if constexpr (HAS_H) bhn = bhh[2 * Hg + j];
    const int ntiles = (a.R + SB - 1) / SB;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int r0 = t * SB;
        __syncthreads();
        if constexpr (HAS_X) {
            for (int i = threadIdx.x; i < SB * xw; i += blockDim.x) {
                const int ss = i / xw, k = i - ss * xw, r = r0 + ss;
                xs[i] = r < a.R ? a.x[row_index<KIND>(a, r) * a.x_stride + a.x_off + (ln ? 0 : gidx * Hg) + k] : 0.f;
            }
        }
        if constexpr (HAS_H) {
            for (int i = threadIdx.x; i < SB * Hg; i += blockDim.x) {
                const int ss = i / Hg, k = i - ss * Hg, r = r0 + ss;
                hs[i] = r < a.R ? a.h[row_index<KIND>(a, r) * a.h_stride + a.h_off + gidx * Hg + k] : 0.f;
            }
        }
        __syncthreads();
        if (ln) {                               // LN1 statistics of each staged row (two passes, biased variance)
            for (int ss = wv; ss < SB; ss += 4) {
                float s1 = 0.f;
                for (int k = lane; k < H; k += 64) s1 += xs[ss * H + k];
                const float mean = wave_sum(s1) / H;
                float v = 0.f;
                for (int k = lane; k < H; k += 64) { const float d = xs[ss * H + k] - mean; v = fmaf(d, d, v); }
                const float var = wave_sum(v) / H;
                if (lane == 0) { st[2 * ss] = mean; st[2 * ss + 1] = 1.0f / sqrtf(var + a.ln_eps); }
            }
            __syncthreads();
        }
        for (int ss = 0; ss < SB; ++ss) {
            const int r = r0 + ss;
            if (r >= a.R) break;
            long long rr;
            if (!row_of<KIND>(a, r, rr)) continue;
            // r and z: the input and the recurrent product share one accumulator, interleaved per q
            float ar = 0.f, az = 0.f, ain = 0.f, ahn = 0.f;
            const float mean = ln ? st[2 * ss] : 0.f, rstd = ln ? st[2 * ss + 1] : 0.f;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int k = lane + 64 * q;
                if (k >= Hg) continue;
                float xv = 0.f, hv = 0.f;
                if constexpr (HAS_X) {
                    xv = xs[ss * xw + src[q]];
                    if (ln) xv = fmaf((xv - mean) * rstd, lg[q], lb[q]);
                }
                if constexpr (HAS_H) hv = hs[ss * Hg + k];
                if constexpr (HAS_X) ar = fmaf(wi[0][q], xv, ar);
                if constexpr (HAS_H) ar = fmaf(wh[0][q], hv, ar);
                if constexpr (HAS_X) az = fmaf(wi[1][q], xv, az);
                if constexpr (HAS_H) az = fmaf(wh[1][q], hv, az);
                if constexpr (HAS_X) ain = fmaf(wi[2][q], xv, ain);
                if constexpr (HAS_H) ahn = fmaf(wh[2][q], hv, ahn);
            }
            ar = wave_sum(ar); az = wave_sum(az);
            if constexpr (HAS_X) ain = wave_sum(ain);
            if constexpr (HAS_H) ahn = wave_sum(ahn);
            if (lane != 0) continue;
            if constexpr (KIND == KIND_PROJ) {
                float* o = a.gi + rr * a.gi_stride + u;
                o[0] = ar + br;
                o[H] = az + bz;
                o[2 * H] = ain + bin;
            } else {
                float pr, pz, pn;
                if constexpr (KIND == KIND_STEP) {
                    pr = ar + br; pz = az + bz; pn = ain + bin;
                } else {
                    const float* gv = a.gi + rr * a.gi_stride + u;
                    pr = gv[0] + ar; pz = gv[H] + az; pn = gv[2 * H];
                }
                const float r_ = 1.0f / (1.0f + expf(-pr));
                const float z = 1.0f / (1.0f + expf(-pz));
                const float n = tanhf(pn + r_ * (ahn + bhn));
                a.out[rr * a.o_stride + a.o_off + u] = (1.0f - z) * n + z * hs[ss * Hg + j];
            }
        }
    }
}

// lim[s] (LIM): the slot's attenuation limit as a gain, the output is lim * noisy + (1 - lim) * enhanced, mixed on the spectrum;
// clip[s] (PCM out, may be null): the count of clamped samples
// pf_tau[s], pf_kind (PF): the slot's perceptual post-filter (postfilter.h), applied to the mask value before the limit's mix:
// gain = lim + (1 - lim) * pf(mask); pf_tau[s] == 0 is the bypass.  The wk_mask row keeps the raw mask.  PF = false reads neither.
// DEC: the decoder's four levels (dec_level); everything around them is the same code for both kinds.
template <int DEC, typename OUT, bool LIM, bool PF>
__global__ void __launch_bounds__(1024) stream_decode_kernel(const int* __restrict__ mode, Layout L, const float* __restrict__ tab,
                                                            const float* __restrict__ w, float ln_eps, float* __restrict__ state,
                                                            float* __restrict__ work, OUT* __restrict__ out,
                                                            const float* __restrict__ lim, int* __restrict__ clip, int pf_kind,
                                                            const float* __restrict__ pf_tau) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, m = mode[s];
    if (!mode_computes_frame(m)) return;
    float* st = state + (size_t)s * L.st_stride;
    float* wk = work + (size_t)s * L.wk_stride;
    const int tid = threadIdx.x;
    // LDS: rows of levels 4..0 | re[161] | im[161] | y[320] | red[one per wave]
    float* row[5];
    int o = 0;
    for (int k = 4; k >= 0; --k) { row[k] = sm + o; o += L.ch[k] * L.F[k]; }
    float* re = sm + o; o += NB;
    float* im = sm + o; o += NB;
    float* y = sm + o; o += NFFT;
    float* red = sm + o;
    // LN2 over the layer-2 output, + skip4 -> decoder input [C4][F4] (the GRU output viewed as c*F4+f)
    const float* h2 = wk + L.wk_h2n;
    float a = 0.f;
    for (int i = tid; i < L.H; i += blockDim.x) a += h2[i];
    const float mean = block_sum(a, red) / L.H;
    float v = 0.f;
    for (int i = tid; i < L.H; i += blockDim.x) { const float d = h2[i] - mean; v = fmaf(d, d, v); }
    const float rstd = 1.0f / sqrtf(block_sum(v, red) / L.H + ln_eps);
    for (int i = tid; i < L.H; i += blockDim.x)
        row[4][i] = fmaf((h2[i] - mean) * rstd, w[L.ln2g + i], w[L.ln2b + i]) + wk[L.wk_skip[4] + i];
    for (int i = tid; i < NB; i += blockDim.x) { re[i] = wk[L.wk_re + i]; im[i] = wk[L.wk_im + i]; }
    // the recurrent state of this hop becomes the state of the next
    for (int i = tid; i < L.H; i += blockDim.x) {
        st[L.st_h1 + i] = wk[L.wk_h1n + i];
        st[L.st_h2 + i] = h2[i];
    }
    __syncthreads();
    for (int k = 4; k >= 1; --k) {
        dec_level<DEC>(w + L.decW[k], w + L.decB[k], row[k], row[k - 1], 0, k > 1 ? wk + L.wk_skip[k - 1] : nullptr, 0, 1, L.ch[k], L.F[k],
                       L.ch[k - 1], k > 1 ? 0 : 1);
        __syncthreads();
    }
    // mask on bins 0..159 (bin 160 zero), 320-point inverse real DFT (imaginary parts of bins 0 and 160 ignored, as irfft)
    if constexpr (LIM) {                                  // gain = lim + (1 - lim) * mask; bin 160 keeps lim of the input
        const float lm = lim[s];
        [[maybe_unused]] float tau = 0.f;
        if constexpr (PF) tau = pf_tau[s];
        for (int i = tid; i < F0; i += blockDim.x) {
            wk[L.wk_mask + i] = row[0][i];
            float g = row[0][i];
            if constexpr (PF) g = cruse_pf::post_filter(g, tau, pf_kind);
            const float gain = fmaf(1.0f - lm, g, lm);
            re[i] *= gain;
            im[i] *= gain;
        }
        if (tid == 0) { re[F0] *= lm; im[F0] *= lm; }
    } else if constexpr (PF) {
        const float tau = pf_tau[s];
        for (int i = tid; i < F0; i += blockDim.x) {
            wk[L.wk_mask + i] = row[0][i];
            const float g = cruse_pf::post_filter(row[0][i], tau, pf_kind);
            re[i] *= g;
            im[i] *= g;
        }
        if (tid == 0) { re[F0] = 0.f; im[F0] = 0.f; }
    } else {
        for (int i = tid; i < F0; i += blockDim.x) {
            wk[L.wk_mask + i] = row[0][i];
            re[i] *= row[0][i];
            im[i] *= row[0][i];
        }
        if (tid == 0) { re[F0] = 0.f; im[F0] = 0.f; }
    }
    __syncthreads();
    for (int n = tid; n < NFFT; n += blockDim.x)
        y[n] = irdft320(re, im, tab + TB_COS, n) * tab[TB_WIN + n];
    __syncthreads();
    // overlap-add with the stored tail, divide by the window envelope: output block; the second half becomes the tail
    int nclip = 0;
    for (int i = tid; i < HOP; i += blockDim.x) {
        nclip += st_sample(out, (size_t)s * HOP + i, (st[L.st_tail + i] + y[i]) * tab[TB_IENV + i]);
        st[L.st_tail + i] = y[HOP + i];
    }
    // the frame-0 chain's block lies in front of the clip (the main chain of the same push overwrites it): not counted
    if constexpr (!std::is_same<OUT, float>::value) count_clipped(clip, s, m == CRUSE_STREAM_MODE_FRAME0 ? 0 : nclip, red);
}

template <int KIND, int KQ>
int launch(const GruArgs& a, const char* name, hipStream_t st) {
    constexpr bool HAS_X = KIND != KIND_REC, HAS_H = KIND != KIND_PROJ;
    // enough workgroups to cover the device, each keeping its unit's weights in registers across several row tiles
    const int H = a.g * a.Hg, units = H / 4, ntiles = (a.R + SB - 1) / SB;
    const int grid_x = std::max(1, std::min(ntiles, (2048 + units - 1) / units));
    const size_t lds = (size_t)((HAS_X ? SB * (a.ln_g ? H : a.Hg) + 2 * SB : 0) + (HAS_H ? SB * a.Hg : 0)) * sizeof(float);
    int rc = cruse_ensure_dyn_lds((const void*)stream_gru_f32_kernel<KIND, KQ>, lds, name);
    if (rc) return rc;
    hipLaunchKernelGGL((stream_gru_f32_kernel<KIND, KQ>), dim3(grid_x, units), dim3(256), lds, st, a);
    CRUSE_LAUNCH_CHECK(name);
    return CRUSE_OK;
}

// KQ: the 64-lane slices of a group's row a lane holds in registers
template <int KIND>
int dispatch_kq(const GruArgs& a, const char* name, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (a.Hg <= 192) return launch<KIND, 3>(a, name, st);
    if (a.Hg <= 320) return launch<KIND, 5>(a, name, st);
    if (a.Hg <= 640) return launch<KIND, 10>(a, name, st);
    return launch<KIND, 16>(a, name, st);
}


// ---- packets: up to `hops` blocks per slot and call (cruse_stream_*_n) ---------------------------------------------------------
// Everything of a hop except the two GRU steps is feed-forward in time, so the frames of a packet are computed side by side:
// one workgroup per slot walks the phases level by level over all frames, with the level's folded weights (or the DFT tables)
// staged in LDS once per packet.  pk[s] = start (0: the slot holds no block, 1: one block, 2: two or more), pk[S + s] = count of
// blocks slot s consumes; both live in device memory.  Frame f of slot s has its own work row, work[(s * work_frames + f) * WS],
// WS = packet_work_stride().
constexpr int PACKET_LDS_BYTES = 128 * 1024;

int packet_row_max(const Layout& L) {
    int m = 2 * NB + 2;                                   // a masked spectrum (re | im) has to fit a row
    for (int k = 0; k < 5; ++k) m = std::max(m, L.ch[k] * L.F[k]);
    return m;
}

// floats of the LDS staging area: the largest padded weight block of any phase, or the cos / sin tables
int packet_wcap(const Layout& L) {
    int m = 2 * NFFT;
    for (int k = 1; k < 5; ++k) {
        m = std::max(m, L.ch[k] * (L.ch[k - 1] * 6 + 1) + L.ch[k]);
        m = std::max(m, L.ch[k] * (L.ch[k] * 3 + 1));
        m = std::max(m, L.ch[k] * L.ch[k - 1] * 3 + L.ch[k - 1]);
    }
    return m;
}

// a frame's work row in a packet: the single-hop work row, then e1 | e2 | e3 (a single hop keeps these in the state rows only)
int packet_work_stride(const Layout& L, int* eoff) {
    int o = L.wk_stride;
    for (int k = 1; k < 4; ++k) {
        if (eoff) eoff[k] = o;
        o += (L.ch[k] * L.F[k] + 3) & ~3;
    }
    return o;
}

// largest number of frames whose rows fit the LDS budget beside the staging area (encode needs one more row than decode)
int packet_max_frames(const Layout& L) {
    const int avail = PACKET_LDS_BYTES / (int)sizeof(float) - packet_wcap(L) - packet_row_max(L) - 64;
    return avail <= 0 ? 0 : avail / (2 * packet_row_max(L));
}

template <typename IN>
__global__ void __launch_bounds__(1024) stream_encode_n_kernel(const int* __restrict__ pk, int S, int hops, int in_hops, int NFW,
                                                              Layout L, int WS, int e1, int e2, int e3, int rowmax, int wcap,
                                                              const IN* __restrict__ in, const float* __restrict__ tab, const float* __restrict__ w,
                                                              float* __restrict__ state, float* __restrict__ work) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const Pkt p = packet_of(pk, S, s, hops);
    if (p.c == 0) return;
    float* st = state + (size_t)s * L.st_stride;
    float* wk = work + (size_t)s * NFW * WS;
    const int eoff[4] = {0, e1, e2, e3};
    const IN* blk = in + (size_t)s * in_hops * HOP;
    float* hist = st + L.st_hist;
    if (p.nf == 0) {                                      // block 0 of a clip alone: stored, no frame
        for (int i = tid; i < HOP; i += nt) hist[1 + i] = ld_sample(blk, i);
        return;
    }
    const int nf = p.nf;
    // LDS: A[NFW][rowmax] | B[NFW][rowmax] | P[rowmax] (row t-1 of the packet's first frame) | Wb[wcap]
    float* A = sm;
    float* B = A + NFW * rowmax;
    float* P = B + NFW * rowmax;
    float* Wb = P + rowmax;
    // block v of the sequence (the stored block first where the slot holds one), sample i
    auto vget = [&](int v, int i) -> float {
        if (p.hist) return v == 0 ? hist[1 + i] : ld_sample(blk, (v - 1) * HOP + i);
        return ld_sample(blk, v * HOP + i);
    };
    const int nv = p.hist + p.c, off = p.f0 ? 0 : 1;
    for (int idx = tid; idx < nf * HOP; idx += nt) {
        const int f = idx / HOP, i = idx - f * HOP;
        float a, bq;
        if (p.f0 && f == 0) {                             // x[160], x[159], ..., x[1] | x[0..159]
            a = i == 0 ? vget(1, 0) : vget(0, HOP - i);
            bq = vget(0, i);
        } else {
            a = vget(f - 1 + off, i);
            bq = vget(f + off, i);
        }
        B[f * rowmax + i] = a * tab[TB_WIN + i];
        B[f * rowmax + HOP + i] = bq * tab[TB_WIN + HOP + i];
    }
    for (int i = tid; i < 2 * NFFT; i += nt) Wb[i] = tab[TB_COS + i];      // cos | sin
    for (int i = tid; i < F0; i += nt) P[i] = st[L.st_prev[0] + i];
    const float before = nv >= 2 ? vget(nv - 2, HOP - 1) : hist[0];        // the sample in front of the last block
    __syncthreads();
    if (tid == 0) hist[0] = before;
    for (int i = tid; i < HOP; i += nt) hist[1 + i] = ld_sample(blk, (p.c - 1) * HOP + i);
    // 320-point real DFT of every frame, bins 0..160; magnitude of bins 0..159
    for (int idx = tid; idx < nf * NB; idx += nt) {
        const int f = idx / NB, k = idx - f * NB;
        float re, im;
        rdft320(B + f * rowmax, Wb, k, re, im);
        wk[(size_t)f * WS + L.wk_re + k] = re;
        wk[(size_t)f * WS + L.wk_im + k] = im;
        if (k < F0) A[f * rowmax + k] = sqrtf(re * re + im * im + 1e-8f);
    }
    __syncthreads();
    for (int i = tid; i < F0; i += nt) st[L.st_prev[0] + i] = A[(nf - 1) * rowmax + i];
    float* src = A;
    float* dst = B;
    for (int k = 1; k < 5; ++k) {
        const int Cin = L.ch[k - 1], Cout = L.ch[k], Fin = L.F[k - 1], Fout = L.F[k], per = Cout * Fout;
        for (int i = tid; i < Cout * Cin * 6; i += nt) Wb[(i / (Cin * 6)) * (Cin * 6 + 1) + i % (Cin * 6)] = w[L.encW[k] + i];
        for (int i = tid; i < Cout; i += nt) Wb[Cout * (Cin * 6 + 1) + i] = w[L.encB[k] + i];
        __syncthreads();
        enc_conv(Wb, Cin * 6 + 1, Wb + Cout * (Cin * 6 + 1), P, src, dst, rowmax, nf, Cin, Fin, Cout, Fout);
        __syncthreads();
        for (int i = tid; i < Cout * Cout * 3; i += nt) Wb[(i / (Cout * 3)) * (Cout * 3 + 1) + i % (Cout * 3)] = w[L.skW[k] + i];
        if (k < 4)
            for (int i = tid; i < per; i += nt) P[i] = st[L.st_prev[k] + i];
        __syncthreads();
        skip_conv(Wb, Cout * 3 + 1, dst, rowmax, wk + L.wk_skip[k], WS, nf, Cout, Fout);
        if (k < 4)
            for (int i = tid; i < per; i += nt) st[L.st_prev[k] + i] = dst[(nf - 1) * rowmax + i];
        const int eo = k < 4 ? eoff[k] : L.wk_x;                           // e1..e3 of every frame; e4 is the GRU input row, c*F4+f
        for (int idx = tid; idx < nf * per; idx += nt) {
            const int f = idx / per, r = idx - f * per;
            wk[(size_t)f * WS + eo + r] = dst[f * rowmax + r];
        }
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
}

template <int DEC, typename OUT, bool LIM, bool PF>
__global__ void __launch_bounds__(1024) stream_decode_n_kernel(const int* __restrict__ pk, int S, int hops, int out_hops, int NFW,
                                                              Layout L, int WS, int rowmax, int wcap, const float* __restrict__ tab,
                                                              const float* __restrict__ w, float ln_eps, float* __restrict__ state,
                                                              float* __restrict__ work, OUT* __restrict__ out,
                                                              const float* __restrict__ lim, int* __restrict__ clip, int pf_kind,
                                                              const float* __restrict__ pf_tau) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const Pkt p = packet_of(pk, S, s, hops);
    const int nf = p.nf;
    if (nf == 0) return;
    float* st = state + (size_t)s * L.st_stride;
    float* wk = work + (size_t)s * NFW * WS;
    // LDS: A[NFW][rowmax] | B[NFW][rowmax] | Wb[wcap] | stats[NFW][2]
    float* A = sm;
    float* B = A + NFW * rowmax;
    float* Wb = B + NFW * rowmax;
    float* stats = Wb + wcap;
    const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    // LN2 statistics of every frame's layer-2 output (one wave per frame, two passes, biased variance)
    for (int f = wv; f < nf; f += nw) {
        const float* h2 = wk + (size_t)f * WS + L.wk_h2n;
        float a = 0.f;
        for (int i = lane; i < L.H; i += 64) a += h2[i];
        const float mean = wave_sum(a) / L.H;
        float v = 0.f;
        for (int i = lane; i < L.H; i += 64) { const float d = h2[i] - mean; v = fmaf(d, d, v); }
        const float var = wave_sum(v) / L.H;
        if (lane == 0) { stats[2 * f] = mean; stats[2 * f + 1] = 1.0f / sqrtf(var + ln_eps); }
    }
    __syncthreads();
    // LN2 + skip4 -> decoder input [C4][F4] of every frame
    for (int idx = tid; idx < nf * L.H; idx += nt) {
        const int f = idx / L.H, i = idx - f * L.H;
        const float* row = wk + (size_t)f * WS;
        A[f * rowmax + i] = fmaf((row[L.wk_h2n + i] - stats[2 * f]) * stats[2 * f + 1], w[L.ln2g + i], w[L.ln2b + i]) + row[L.wk_skip[4] + i];
    }
    // the recurrent state of the packet's last frame becomes the state of the next call
    for (int i = tid; i < L.H; i += nt) {
        st[L.st_h1 + i] = wk[(size_t)(nf - 1) * WS + L.wk_h1n + i];
        st[L.st_h2 + i] = wk[(size_t)(nf - 1) * WS + L.wk_h2n + i];
    }
    float* src = A;
    float* dst = B;
    for (int k = 4; k >= 1; --k) {
        const int nwf = L.ch[k] * L.ch[k - 1] * 3;
        for (int i = tid; i < nwf; i += nt) Wb[i] = w[L.decW[k] + i];
        for (int i = tid; i < L.ch[k - 1]; i += nt) Wb[nwf + i] = w[L.decB[k] + i];
        __syncthreads();
        dec_level<DEC>(Wb, Wb + nwf, src, dst, rowmax, wk + (k > 1 ? L.wk_skip[k - 1] : 0), WS, nf, L.ch[k], L.F[k], L.ch[k - 1],
                       k > 1 ? 0 : 1);
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
    // src: the masks.  Masked spectrum re[161] | im[161] of every frame into dst (bin 160 zero), cos / sin tables into Wb
    if constexpr (LIM) {                                  // gain = lim + (1 - lim) * mask; bin 160 keeps lim of the input
        const float lm = lim[s];
        [[maybe_unused]] float tau = 0.f;
        if constexpr (PF) tau = pf_tau[s];
        for (int idx = tid; idx < nf * NB; idx += nt) {
            const int f = idx / NB, k = idx - f * NB;
            float* row = wk + (size_t)f * WS;
            float m = k < F0 ? src[f * rowmax + k] : 0.f;
            if (k < F0) row[L.wk_mask + k] = m;
            if constexpr (PF) m = cruse_pf::post_filter(m, tau, pf_kind);       // (bin 160: pf(0) = 0, and the gain below is lim)
            const float gain = k < F0 ? fmaf(1.0f - lm, m, lm) : lm;
            dst[f * rowmax + k] = row[L.wk_re + k] * gain;
            dst[f * rowmax + NB + k] = row[L.wk_im + k] * gain;
        }
    } else {
        [[maybe_unused]] float tau = 0.f;
        if constexpr (PF) tau = pf_tau[s];
        for (int idx = tid; idx < nf * NB; idx += nt) {
            const int f = idx / NB, k = idx - f * NB;
            float* row = wk + (size_t)f * WS;
            float m = k < F0 ? src[f * rowmax + k] : 0.f;
            if (k < F0) row[L.wk_mask + k] = m;
            if constexpr (PF) m = cruse_pf::post_filter(m, tau, pf_kind);       // (bin 160: pf(0) = 0)
            dst[f * rowmax + k] = row[L.wk_re + k] * m;
            dst[f * rowmax + NB + k] = row[L.wk_im + k] * m;
        }
    }
    for (int i = tid; i < 2 * NFFT; i += nt) Wb[i] = tab[TB_COS + i];
    __syncthreads();
    // 320-point inverse real DFT (imaginary parts of bins 0 and 160 ignored, as irfft) and window: y of every frame into src
    for (int idx = tid; idx < nf * NFFT; idx += nt) {
        const int f = idx / NFFT, n = idx - f * NFFT;
        const float* re = dst + f * rowmax;
        src[f * rowmax + n] = irdft320(re, re + NB, Wb, n) * tab[TB_WIN + n];
    }
    __syncthreads();
    // overlap-add: a chain over the packet's frames (tail -> block -> new tail), division by the window envelope
    int nclip = 0;
    for (int i = tid; i < HOP; i += nt) {
        float tail = st[L.st_tail + i];
        const float ienv = tab[TB_IENV + i];
        for (int f = 0; f < nf; ++f) {
            const float o = (tail + src[f * rowmax + i]) * ienv;
            const int ob = f - p.f0;                                       // frame 0's block lies in front of the clip
            if (ob >= 0) nclip += st_sample(out, ((size_t)s * out_hops + ob) * HOP + i, o);
            tail = src[f * rowmax + HOP + i];
        }
        st[L.st_tail + i] = tail;
    }
    if constexpr (!std::is_same<OUT, float>::value) count_clipped(clip, s, nclip, Wb);      // the tables in Wb are no longer read
}

// shared argument checks of the packet entry points
int packet_args(const char* who, int S, int hops, int NFW, const Layout& L) {
    CRUSE_REQUIRE(S > 0 && hops >= 1 && NFW >= hops + 1, CRUSE_E_SHAPE, "%s: S = %d, hops = %d, work_frames = %d (need work_frames >= hops + 1)",
                  who, S, hops, NFW);
    const int maxf = packet_max_frames(L);
    CRUSE_REQUIRE(NFW <= maxf, CRUSE_E_SHAPE, "%s: %d frames per slot exceed the %d whose rows fit in LDS (max_hops %d for these channels)", who,
                  NFW, maxf, maxf - 1);
    return CRUSE_OK;
}

// ---- host side of the boundary kernels (encode, decode, the DeepFilter head).  Each of the 14 entry points lists its arguments by group
// into a BoundaryArgs and calls its family's function, which checks and launches, single hop or packet.  A group an entry point has no
// arguments for stays zero: f32 samples, no limit, no counter, no post-filter -> the <float> / <float, false, false> kernels.
struct Slots { const char* name; const int* ctl; int S; };      // the entry point's name ("cruse_stream_..."); mode[S], packets: pk[2][S]
struct Packet { bool packet; int hops, io_hops, work_frames; };
struct Net { std::array<int, 5> ch; const float *tab, *w; float ln_eps, *state, *work; };
struct Samples { const void* io; int fmt; const float* lim; int* clip; };       // io: encode's in, decode's and the head's out
struct PostFilter { bool pf_required; int pf_kind; const float* pf_tau; int dec; };      // pf_required: pf_kind 0 is refused; dec: DEC_*
// the head's work rows (DfRows), state rows and inspection rows (dw, single hop: floats between two rows; packets: rows per slot), instance
struct Head { int drain; const float* rows; int wk_stride, wk_re, wk_im, wk_mask; float* df_state; int st_stride;
              float* df_work; int dw, t_dim, f_dim; };
struct BoundaryArgs : Slots, Packet, Net, Samples, PostFilter, Head { Layout L; };       // L: of ch, by chain_args

const char* who_of(const BoundaryArgs& a) { return a.name + 6; }        // the family's messages leave out the "cruse_"

// cruse_stream_boundary_plan calls the entry point itself with plan_out set: launch_* then write what they were about to launch (family:
// 0 encode, 2 decode, 4 head, + 1 for packets) and return
thread_local int* plan_out = nullptr;
struct Plan { int family, dec, s16, lim, pf, grid, block, lds, WS, rowmax, wcap; };
static_assert(sizeof(Plan) == CRUSE_STREAM_PLAN_INTS * sizeof(int), "plan size");

int planned(const Plan& p) { return memcpy(plan_out, &p, sizeof(p)), CRUSE_OK; }

// (fmt, lim, pf_kind) -> f(OUT(), LIM, PF) with LIM, PF as std::true_type / false_type: the one place the kernel instance is chosen.
// WITH_PF false: the kernels have no PF axis
template <bool WITH_PF, typename F>
int with_form(const BoundaryArgs& a, F&& f) {
    auto pf = [&](auto out, auto lim) {
        if (WITH_PF && a.pf_kind != 0) return f(out, lim, std::bool_constant<WITH_PF>());
        return f(out, lim, std::false_type());
    };
    auto lim = [&](auto out) { return a.lim ? pf(out, std::true_type()) : pf(out, std::false_type()); };
    return a.fmt == FMT_S16 ? lim(short()) : lim(float());
}

// the perceptual post-filter in the gain line (utils/utils.py:345-362): the kind and the per-slot tau.  allow_none (every entry point
// but the _pf ones): pf_kind 0 is no post-filter, and pf_tau is not read
int pf_args(const char* who, int pf_kind, const float* pf_tau, bool allow_none) {
    if (allow_none && pf_kind == 0) return CRUSE_OK;
    const int rc = cruse_pf::kind_args(who, pf_kind);
    if (rc) return rc;
    CRUSE_REQUIRE(pf_tau != nullptr, CRUSE_E_SHAPE, "%s: null pf_tau", who);
    return CRUSE_OK;
}

// the layout and the checks encode and decode share; io_hops: what the entry point calls the block stride of its samples
int chain_args(BoundaryArgs& a, const char* io_hops) {
    const char* who = who_of(a);
    int rc = make_layout(a.ch[0], a.ch[1], a.ch[2], a.ch[3], a.ch[4], a.L);
    if (rc) return rc;
    const bool bufs = a.ctl && a.io && a.tab && a.w && a.state && a.work;
    CRUSE_REQUIRE(a.packet || (a.S > 0 && bufs), CRUSE_E_SHAPE, "%s: S = %d or a null buffer", who, a.S);
    if (!a.packet) return CRUSE_OK;
    CRUSE_REQUIRE(bufs, CRUSE_E_SHAPE, "%s: null buffer", who);
    rc = packet_args(who, a.S, a.hops, a.work_frames, a.L);
    if (rc) return rc;
    CRUSE_REQUIRE(a.io_hops >= a.hops, CRUSE_E_SHAPE, "%s: %s = %d < hops = %d", who, io_hops, a.io_hops, a.hops);
    return CRUSE_OK;
}

template <typename IN>
int launch_encode(const BoundaryArgs& a, hipStream_t st) {
    const Layout& L = a.L;
    int rows = NFFT + 2 * NB;                             // single hop: frame | rows of levels 0..4 | previous rows 0..3 | re | im
    for (int k = 0; k < 5; ++k) rows += L.ch[k] * L.F[k];
    for (int k = 0; k < 4; ++k) rows += L.ch[k] * L.F[k];
    const int rowmax = a.packet ? packet_row_max(L) : 0, wcap = a.packet ? packet_wcap(L) : 0;
    int eoff[4] = {0, 0, 0, 0};
    const int WS = a.packet ? packet_work_stride(L, eoff) : 0;
    const size_t lds = (size_t)(a.packet ? (2 * a.work_frames + 1) * rowmax + wcap : rows) * sizeof(float);
    if (plan_out) return planned({0 + a.packet, 0, std::is_same<IN, short>::value, 0, 0, a.S, FRAME_THREADS, (int)lds, WS, rowmax, wcap});
    const void* fn = a.packet ? (const void*)stream_encode_n_kernel<IN> : (const void*)stream_encode_kernel<IN>;
    const int rc = cruse_ensure_dyn_lds(fn, lds, a.name);
    if (rc) return rc;
    if (a.packet)
        hipLaunchKernelGGL(stream_encode_n_kernel<IN>, dim3(a.S), dim3(FRAME_THREADS), lds, st, a.ctl, a.S, a.hops, a.io_hops,
                           a.work_frames, L, WS, eoff[1], eoff[2], eoff[3], rowmax, wcap, (const IN*)a.io, a.tab, a.w, a.state, a.work);
    else
        hipLaunchKernelGGL(stream_encode_kernel<IN>, dim3(a.S), dim3(FRAME_THREADS), lds, st, a.ctl, L, (const IN*)a.io, a.tab, a.w, a.state, a.work);
    CRUSE_LAUNCH_CHECK(a.name);
    return CRUSE_OK;
}

int encode_any(BoundaryArgs a, void* stream) {
    int rc = chain_args(a, "in_hops");
    if (rc) return rc;
    rc = fmt_args(who_of(a), a.fmt);
    if (rc) return rc;
    return a.fmt == FMT_S16 ? launch_encode<short>(a, (hipStream_t)stream) : launch_encode<float>(a, (hipStream_t)stream);
}

template <int DEC, typename OUT, bool LIM, bool PF>
int launch_decode(const BoundaryArgs& a, hipStream_t st) {
    const Layout& L = a.L;
    int rows = 2 * NB + NFFT + FRAME_THREADS / 64;        // single hop: rows of levels 4..0 | re | im | y | red
    for (int k = 0; k < 5; ++k) rows += L.ch[k] * L.F[k];
    const int rowmax = a.packet ? packet_row_max(L) : 0, wcap = a.packet ? packet_wcap(L) : 0, WS = a.packet ? packet_work_stride(L, nullptr) : 0;
    const size_t lds = (size_t)(a.packet ? 2 * a.work_frames * rowmax + wcap + 2 * a.work_frames : rows) * sizeof(float);
    if (plan_out) return planned({2 + a.packet, DEC, std::is_same<OUT, short>::value, LIM, PF, a.S, FRAME_THREADS, (int)lds, WS, rowmax, wcap});
    const void* fn = a.packet ? (const void*)stream_decode_n_kernel<DEC, OUT, LIM, PF> : (const void*)stream_decode_kernel<DEC, OUT, LIM, PF>;
    const int rc = cruse_ensure_dyn_lds(fn, lds, a.name);
    if (rc) return rc;
    const int pf_kind = PF ? a.pf_kind : 0;               // an instance without PF reads neither
    const float* pf_tau = PF ? a.pf_tau : nullptr;
    if (a.packet)
        hipLaunchKernelGGL((stream_decode_n_kernel<DEC, OUT, LIM, PF>), dim3(a.S), dim3(FRAME_THREADS), lds, st, a.ctl, a.S, a.hops, a.io_hops,
                           a.work_frames, L, WS, rowmax, wcap, a.tab, a.w, a.ln_eps, a.state, a.work, (OUT*)a.io, a.lim, a.clip, pf_kind, pf_tau);
    else
        hipLaunchKernelGGL((stream_decode_kernel<DEC, OUT, LIM, PF>), dim3(a.S), dim3(FRAME_THREADS), lds, st, a.ctl, L, a.tab, a.w, a.ln_eps, a.state,
                           a.work, (OUT*)a.io, a.lim, a.clip, pf_kind, pf_tau);
    CRUSE_LAUNCH_CHECK(a.name);
    return CRUSE_OK;
}

int decode_any(BoundaryArgs a, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    int rc = pf_args(a.name, a.pf_kind, a.pf_tau, !a.pf_required);      // comes first, and names the entry point in full
    if (rc) return rc;
    rc = chain_args(a, "out_hops");
    if (rc) return rc;
    rc = out_args(who_of(a), a.fmt, a.clip);
    if (rc) return rc;
    return with_form<true>(a, [&](auto out, auto lim, auto pf) {
        constexpr bool LIM = decltype(lim)::value, PF = decltype(pf)::value;
        return a.dec == DEC_UPCONV ? launch_decode<DEC_UPCONV, decltype(out), LIM, PF>(a, st) : launch_decode<DEC_CONVT, decltype(out), LIM, PF>(a, st);
    });
}

// ---- the DeepFilter(1, 5) head on the stream (cruse_stream_df_head / _df_head_n) -------------------------------------------------
// A config-4 model's output is the real filter field of DeepFilter(t_dim = 1, f_dim = 5): with P[t] = mask[t] * N[t] on bins 0..159
// (bin 160 zero), the enhanced row is E[t] = sum_{dt = -1..1} sum_{df = -5..5} P[t + dt][f + df], zero outside the spectrum and the
// clip.  E[t] needs frame t + 1, so this kernel runs one frame behind the chain: it follows decode, reads the mask and the noisy
// spectrum decode / encode left in the frame's work row, and keeps in a state row of its own P[t-2], P[t-1], N[t-1] (the attenuation
// limit mixes against it), an overlap-add tail and the count of rows taken since the clip began (saturating at 2).  A step takes row
// t, emits E[t-1] (inspection row, inverse DFT, window, overlap-add with its own tail: the arithmetic of the decode kernels) and
// shifts the rows.  The step of the clip's frame 0 starts from a zero history and emits nothing; the block of E[0] lies in front of the
// clip (as the mask path's frame-0 block) and is neither stored nor counted; a drain step takes an all-zero row and so emits E[T-1].
// One workgroup per slot, no communication between workgroups; the frame loop is bounded by the packet's frame count (<= hops + 1).
//
// Bit contract: the window sum runs in f32 from 0.0f, frame offset outer, bin offset inner, both ascending, over products formed by one
// multiplication each: the order of df_head.hip, so E has the bits of cruse_df_head_apply on the stacked rows.
constexpr int DF_FD = 5, DF_PW = NB + 2 * DF_FD;          // a product plane with its zero halo of f_dim bins on either side
constexpr int DF_THREADS = 384;
constexpr int DF_PLANE = (NB + 3) & ~3;                   // floats between the re and the im plane of a state row pair
// the largest hops any channel set's packet layout admits (packet_max_frames with the smallest row and staging area) bounds `hops`
constexpr int DF_MAX_HOPS = (PACKET_LDS_BYTES / (int)sizeof(float) - 2 * NFFT - (2 * NB + 2) - 64) / (2 * (2 * NB + 2)) - 1;

// the layout of cruse_stream_df_layout(): all ints, in the order of the header's description
struct DfLayout {
    int p2, p1, n1, tail, count, plane, stride;
};
static_assert(sizeof(DfLayout) == CRUSE_STREAM_DF_LAYOUT_INTS * sizeof(int), "df layout size");

void make_df_layout(DfLayout& D) {
    int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    D.plane = DF_PLANE;
    D.p2 = take(2 * DF_PLANE);
    D.p1 = take(2 * DF_PLANE);
    D.n1 = take(2 * DF_PLANE);
    D.tail = take(HOP);
    D.count = take(1);
    D.stride = o;
}

// floats of LDS: three product rows (re | im, with halo) | N[t-1] | N[t] | the spectrum into the inverse DFT | y | tail | cos, sin | red
constexpr int DF_LDS = 3 * 2 * DF_PW + 3 * 2 * NB + NFFT + HOP + 2 * NFFT + DF_THREADS / 64;

// where the work rows of a call lie, as the caller's layout says
struct DfRows {
    const float* work;      // the slot's first row (null: a drain step, the row is all zero)
    int WS, re, im, mask;   // floats between two frames' rows; offsets of the noisy spectrum and the mask in a row
};

// E[t-1] from the three product rows: sp (the spectrum for the inverse DFT; with LIM lim * N[t-1] + (1 - lim) * E) and the inspection row
template <bool LIM>
__device__ __forceinline__ void df_window(const float* p2, const float* p1, const float* pc, const float* n1, float lm, float* sp,
                                          float* __restrict__ dfw) {
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < 2 * NB; i += blockDim.x) {
        const int pl = i >= NB, f = i - pl * NB;
        const float* q[3] = {p2 + pl * DF_PW + f, p1 + pl * DF_PW + f, pc + pl * DF_PW + f};     // q[dt][df]: bin f - 5 + df
        float acc = 0.f;
#pragma unroll
        for (int dt = 0; dt < 3; ++dt)
#pragma unroll
            for (int df = 0; df <= 2 * DF_FD; ++df) acc += q[dt][df];
        dfw[i] = acc;
        if constexpr (LIM) sp[i] = lm * n1[i] + (1.0f - lm) * acc;
        else sp[i] = acc;
    }
}

// nf frames of slot s from rows R: f0: the first one is frame 0 of the clip.  dfw: the slot's inspection rows (one per emitted E),
// out + o_at: the slot's output blocks (one per emitted E but E[0]).  st: the slot's state row.
template <typename OUT, bool LIM>
__device__ __forceinline__ void df_frames(float* sm, int s, int nf, bool f0, const DfRows R, const float* __restrict__ tab,
                                          float* __restrict__ st, const DfLayout D, float* __restrict__ dfw, OUT* __restrict__ out,
                                          size_t o_at, const float* __restrict__ lim, int* __restrict__ clip) {
    const int tid = threadIdx.x, nt = blockDim.x;
    float* p2 = sm;
    float* p1 = p2 + 2 * DF_PW;
    float* pc = p1 + 2 * DF_PW;
    float* n1 = pc + 2 * DF_PW;
    float* nc = n1 + 2 * NB;
    float* sp = nc + 2 * NB;
    float* y = sp + 2 * NB;
    float* tail = y + NFFT;
    float* cs = tail + HOP;
    float* red = cs + 2 * NFFT;
    float lm = 0.f;
    if constexpr (LIM) lm = lim[s];
    int cnt = (int)st[D.count];                           // uniform: rows taken since the clip began, 2: two or more
    for (int i = tid; i < 3 * 2 * DF_PW; i += nt) sm[i] = 0.f;          // the halos stay zero from here on
    __syncthreads();
    for (int i = tid; i < 2 * NB; i += nt) {
        const int pl = i >= NB, f = i - pl * NB;
        p2[pl * DF_PW + DF_FD + f] = st[D.p2 + pl * D.plane + f];
        p1[pl * DF_PW + DF_FD + f] = st[D.p1 + pl * D.plane + f];
        n1[i] = st[D.n1 + pl * D.plane + f];
    }
    for (int i = tid; i < HOP; i += nt) tail[i] = st[D.tail + i];
    for (int i = tid; i < 2 * NFFT; i += nt) cs[i] = tab[TB_COS + i];
    int nclip = 0, e = 0, ob = 0;
    for (int fr = 0; fr < nf; ++fr) {
        if (fr == 0 && f0) {                              // frame 0 of the clip: the history is zero, whatever the state row held
            __syncthreads();
            for (int i = tid; i < 2 * NB; i += nt) {
                const int pl = i >= NB, f = i - pl * NB;
                p2[pl * DF_PW + DF_FD + f] = 0.f;
                p1[pl * DF_PW + DF_FD + f] = 0.f;
                n1[i] = 0.f;
            }
            for (int i = tid; i < HOP; i += nt) tail[i] = 0.f;
            cnt = 0;
        }
        // row t: P[t] = mask * N[t] on bins 0..159, bin 160 zero
        const float* row = R.work ? R.work + (size_t)fr * R.WS : nullptr;
        for (int i = tid; i < 2 * NB; i += nt) {
            const int pl = i >= NB, f = i - pl * NB;
            const float n = row ? row[(pl ? R.im : R.re) + f] : 0.f;
            nc[i] = n;
            pc[pl * DF_PW + DF_FD + f] = row && f < F0 ? row[R.mask + f] * n : 0.f;
        }
        __syncthreads();
        if (cnt >= 1) {                                   // E[t-1]
            df_window<LIM>(p2, p1, pc, n1, lm, sp, dfw + (size_t)e * 2 * NB);
            ++e;
            __syncthreads();
            for (int n = tid; n < NFFT; n += nt) y[n] = irdft320(sp, sp + NB, cs, n) * tab[TB_WIN + n];
            __syncthreads();
            const bool keep = cnt >= 2;                   // E[0]'s block lies in front of the clip
            for (int i = tid; i < HOP; i += nt) {
                const float o = (tail[i] + y[i]) * tab[TB_IENV + i];
                if (keep) nclip += st_sample(out, o_at + (size_t)ob * HOP + i, o);
                tail[i] = y[HOP + i];
            }
            ob += keep;
            __syncthreads();
        }
        // shift the rows
        float* t = p2; p2 = p1; p1 = pc; pc = t;
        t = n1; n1 = nc; nc = t;
        cnt = min(cnt + 1, 2);
    }
    for (int i = tid; i < 2 * NB; i += nt) {
        const int pl = i >= NB, f = i - pl * NB;
        st[D.p2 + pl * D.plane + f] = p2[pl * DF_PW + DF_FD + f];
        st[D.p1 + pl * D.plane + f] = p1[pl * DF_PW + DF_FD + f];
        st[D.n1 + pl * D.plane + f] = n1[i];
    }
    for (int i = tid; i < HOP; i += nt) st[D.tail + i] = tail[i];
    if (tid == 0) st[D.count] = (float)cnt;
    if constexpr (!std::is_same<OUT, float>::value) count_clipped(clip, s, nclip, red);
}

// drain: only slots whose mode is END step, on an all-zero row
template <typename OUT, bool LIM>
__global__ void __launch_bounds__(DF_THREADS) stream_df_head_kernel(const int* __restrict__ mode, int drain, DfRows R,
                                                                   const float* __restrict__ tab, float* __restrict__ state, int SS,
                                                                   DfLayout D, float* __restrict__ dfw, int DWS, OUT* __restrict__ out,
                                                                   const float* __restrict__ lim, int* __restrict__ clip) {
    __shared__ float sm[DF_LDS];
    const int s = blockIdx.x, m = mode[s];
    if (drain ? m != CRUSE_STREAM_MODE_END : !mode_computes_frame(m)) return;
    R.work = drain ? nullptr : R.work + (size_t)s * R.WS;
    df_frames<OUT, LIM>(sm, s, 1, !drain && m == CRUSE_STREAM_MODE_FRAME0, R, tab, state + (size_t)s * SS, D, dfw + (size_t)s * DWS, out,
                        (size_t)s * HOP, lim, clip);
}

template <typename OUT, bool LIM>
__global__ void __launch_bounds__(DF_THREADS) stream_df_head_n_kernel(const int* __restrict__ pk, int S, int hops, int out_hops, int NFW,
                                                                     DfRows R, const float* __restrict__ tab, float* __restrict__ state,
                                                                     int SS, DfLayout D, float* __restrict__ dfw, int DWF,
                                                                     OUT* __restrict__ out, const float* __restrict__ lim,
                                                                     int* __restrict__ clip) {
    __shared__ float sm[DF_LDS];
    const int s = blockIdx.x;
    const Pkt p = packet_of(pk, S, s, hops);
    if (p.nf == 0) return;
    R.work += (size_t)s * NFW * R.WS;
    // at most nf - f0 <= hops rows are emitted: dfw holds DWF >= hops rows per slot, out out_hops >= hops blocks
    df_frames<OUT, LIM>(sm, s, p.nf, p.f0, R, tab, state + (size_t)s * SS, D, dfw + (size_t)s * DWF * 2 * NB, out,
                        (size_t)s * out_hops * HOP, lim, clip);
}

template <typename OUT, bool LIM>
int launch_df_head(const BoundaryArgs& a, const DfLayout& D, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (plan_out) return planned({4 + a.packet, 0, std::is_same<OUT, short>::value, LIM, 0, a.S, DF_THREADS, 0, 0, 0, 0});
    const DfRows R = {a.rows, a.wk_stride, a.wk_re, a.wk_im, a.wk_mask};
    if (a.packet)
        hipLaunchKernelGGL((stream_df_head_n_kernel<OUT, LIM>), dim3(a.S), dim3(DF_THREADS), 0, st, a.ctl, a.S, a.hops, a.io_hops, a.work_frames, R,
                           a.tab, a.df_state, a.st_stride, D, a.df_work, a.dw, (OUT*)a.io, a.lim, a.clip);
    else
        hipLaunchKernelGGL((stream_df_head_kernel<OUT, LIM>), dim3(a.S), dim3(DF_THREADS), 0, st, a.ctl, a.drain != 0, R, a.tab, a.df_state,
                           a.st_stride, D, a.df_work, a.dw, (OUT*)a.io, a.lim, a.clip);
    CRUSE_LAUNCH_CHECK(a.name);
    return CRUSE_OK;
}

int df_head_any(const BoundaryArgs& a, void* stream) {
    const char* who = who_of(a);
    CRUSE_REQUIRE(a.t_dim == 1 && a.f_dim == DF_FD, CRUSE_E_SHAPE, "%s: (t_dim, f_dim) = (%d, %d): only the DeepFilter(1, %d) instance is built", who,
                  a.t_dim, a.f_dim, DF_FD);
    CRUSE_REQUIRE(a.S >= 1, CRUSE_E_SHAPE, "%s: S = %d (need S >= 1)", who, a.S);
    CRUSE_REQUIRE(a.ctl && a.rows && a.tab && a.df_state && a.df_work && a.io, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(a.wk_stride >= 2 * NB + F0 && a.wk_re >= 0 && a.wk_re + NB <= a.wk_stride && a.wk_im >= 0 && a.wk_im + NB <= a.wk_stride &&
                  a.wk_mask >= 0 && a.wk_mask + F0 <= a.wk_stride, CRUSE_E_SHAPE,
                  "%s: wk_re %d / wk_im %d (+ %d) / wk_mask %d (+ %d) do not lie in a work row of %d floats (>= %d)", who, a.wk_re, a.wk_im, NB,
                  a.wk_mask, F0, a.wk_stride, 2 * NB + F0);
    DfLayout D;
    make_df_layout(D);
    CRUSE_REQUIRE(a.st_stride >= D.stride, CRUSE_E_SHAPE, "%s: df_state rows of %d floats, the layout needs %d", who, a.st_stride, D.stride);
    const int rc = out_args(who, a.fmt, a.clip);
    if (rc) return rc;
    if (a.packet)
        CRUSE_REQUIRE(a.hops >= 1 && a.hops <= DF_MAX_HOPS && a.work_frames >= a.hops + 1 && a.io_hops >= a.hops && a.dw >= a.hops, CRUSE_E_SHAPE,
                      "%s: hops = %d (1..%d), work_frames = %d (>= hops + 1), out_hops = %d, dw_frames = %d (>= hops)", who, a.hops, DF_MAX_HOPS,
                      a.work_frames, a.io_hops, a.dw);
    else
        CRUSE_REQUIRE(a.dw >= 2 * NB, CRUSE_E_SHAPE, "%s: df_work rows of %d floats, need %d", who, a.dw, 2 * NB);
    return with_form<false>(a, [&](auto out, auto lim, auto) { return launch_df_head<decltype(out), decltype(lim)::value>(a, D, stream); });
}

}  // namespace

extern "C" int cruse_stream_df_layout(int* out) {
    CRUSE_REQUIRE(out, CRUSE_E_SHAPE, "stream_df_layout: null output");
    DfLayout D;
    make_df_layout(D);
    memcpy(out, &D, sizeof(D));
    return CRUSE_OK;
}

extern "C" int cruse_stream_df_head(const int* mode, int S, int drain, const float* work, int wk_stride, int wk_re, int wk_im, int wk_mask,
                                    const float* tab, float* df_state, int st_stride, float* df_work, int dw_stride, void* out, int out_fmt,
                                    const float* lim, int* clip, int t_dim, int f_dim, void* stream) {
    return df_head_any({{"cruse_stream_df_head", mode, S}, {}, {{}, tab}, {out, out_fmt, lim, clip}, {},
                        {drain, work, wk_stride, wk_re, wk_im, wk_mask, df_state, st_stride, df_work, dw_stride, t_dim, f_dim}}, stream);
}

extern "C" int cruse_stream_df_head_n(const int* pk, int S, int hops, int out_hops, int work_frames, const float* work, int wk_stride,
                                      int wk_re, int wk_im, int wk_mask, const float* tab, float* df_state, int st_stride, float* df_work,
                                      int dw_frames, void* out, int out_fmt, const float* lim, int* clip, int t_dim, int f_dim,
                                      void* stream) {
    return df_head_any({{"cruse_stream_df_head_n", pk, S}, {true, hops, out_hops, work_frames}, {{}, tab}, {out, out_fmt, lim, clip}, {},
                        {0, work, wk_stride, wk_re, wk_im, wk_mask, df_state, st_stride, df_work, dw_frames, t_dim, f_dim}}, stream);
}

extern "C" int cruse_stream_layout(int c0, int c1, int c2, int c3, int c4, int* out) {
    CRUSE_REQUIRE(out, CRUSE_E_SHAPE, "stream_layout: null output");
    Layout L;
    const int rc = make_layout(c0, c1, c2, c3, c4, L);
    if (rc) return rc;
    memcpy(out, &L, sizeof(L));
    return CRUSE_OK;
}

extern "C" int cruse_stream_tables(float* tab, void* stream) {
    CRUSE_REQUIRE(tab, CRUSE_E_SHAPE, "stream_tables: null table");
    // built on the host in double precision, then copied: 1120 floats
    static float h[TB_TOTAL];
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.14159265358979323846;
        for (int n = 0; n < NFFT; ++n) {
            h[TB_WIN + n] = (float)(0.5 - 0.5 * cos(2.0 * pi * n / NFFT));
            h[TB_COS + n] = (float)cos(2.0 * pi * n / NFFT);
            h[TB_SIN + n] = (float)sin(2.0 * pi * n / NFFT);
        }
        for (int m = 0; m < HOP; ++m) {
            const double a = 0.5 - 0.5 * cos(2.0 * pi * m / NFFT), b = 0.5 - 0.5 * cos(2.0 * pi * (m + HOP) / NFFT);
            h[TB_IENV + m] = (float)(1.0 / (a * a + b * b));
        }
    });
    CRUSE_HIP(hipMemcpyAsync(tab, h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)stream), "stream_tables");
    CRUSE_HIP(hipStreamSynchronize((hipStream_t)stream), "stream_tables");
    return CRUSE_OK;
}

extern "C" int cruse_stream_encode(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* in, const float* tab,
                                   const float* w, float* state, float* work, void* stream) {
    return encode_any({{"cruse_stream_encode", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, 0.f, state, work}, {in}}, stream);
}

extern "C" int cruse_stream_encode_io(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const void* in, int in_fmt,
                                      const float* tab, const float* w, float* state, float* work, void* stream) {
    return encode_any({{"cruse_stream_encode_io", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, 0.f, state, work}, {in, in_fmt}}, stream);
}

extern "C" int cruse_stream_gru(const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                                const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                                const float* pack, float* hout, int o_stride, int o_off, void* stream) {
    GruArgs a = {};
    const int rc = gru_step_args("stream_gru", mode, S, layer, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off, pack,
                                 hout, o_stride, o_off, a);
    return rc ? rc : dispatch_kq<KIND_STEP>(a, "cruse_stream_gru", stream);
}

extern "C" int cruse_stream_decode(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                                   float ln_eps, float* state, float* work, float* out, void* stream) {
    return decode_any({{"cruse_stream_decode", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out}}, stream);
}

extern "C" int cruse_stream_decode_io(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                                      float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                                      void* stream) {
    return decode_any({{"cruse_stream_decode_io", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work},
                       {out, out_fmt, lim, clip}}, stream);
}

// the perceptual post-filter in the gain line (utils/utils.py:345-362): the _io arguments plus the kind and the per-slot tau
extern "C" int cruse_stream_decode_pf(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                                      float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                                      int pf_kind, const float* pf_tau, void* stream) {
    return decode_any({{"cruse_stream_decode_pf", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out, out_fmt, lim, clip},
                       {true, pf_kind, pf_tau}}, stream);
}

extern "C" int cruse_stream_packet_layout(int c0, int c1, int c2, int c3, int c4, int* out) {
    CRUSE_REQUIRE(out, CRUSE_E_SHAPE, "stream_packet_layout: null output");
    Layout L;
    const int rc = make_layout(c0, c1, c2, c3, c4, L);
    if (rc) return rc;
    int eoff[4] = {0, 0, 0, 0};
    out[0] = std::max(0, packet_max_frames(L) - 1);
    out[1] = packet_work_stride(L, eoff);
    for (int k = 1; k < 4; ++k) out[1 + k] = eoff[k];
    return CRUSE_OK;
}

extern "C" int cruse_stream_encode_n(const int* pk, int S, int hops, int in_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                     const float* in, const float* tab, const float* w, float* state, float* work, void* stream) {
    return encode_any({{"cruse_stream_encode_n", pk, S}, {true, hops, in_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, 0.f, state, work}, {in}}, stream);
}

extern "C" int cruse_stream_encode_n_io(const int* pk, int S, int hops, int in_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                        const void* in, int in_fmt, const float* tab, const float* w, float* state, float* work,
                                        void* stream) {
    return encode_any({{"cruse_stream_encode_n_io", pk, S}, {true, hops, in_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, 0.f, state, work}, {in, in_fmt}}, stream);
}

extern "C" int cruse_stream_gru_proj_n(const int* pk, int S, int hops, int work_frames, int layer, int g, int Hg, const float* work,
                                       int wk_stride, int x_off, const float* ln_g, const float* ln_b, float ln_eps, const float* pack,
                                       float* gi, void* stream) {
    GruArgs a = {};
    const int rc = gru_proj_args("stream_gru_proj_n", pk, S, hops, work_frames, layer, g, Hg, work, wk_stride, x_off, ln_g, ln_b, ln_eps,
                                 pack, gi, a);
    return rc ? rc : dispatch_kq<KIND_PROJ>(a, "cruse_stream_gru_proj_n", stream);
}

extern "C" int cruse_stream_gru_rec_n(const int* pk, int S, int hops, int work_frames, int frame, int g, int Hg, const float* gi,
                                      const float* state, int st_stride, int st_off, const float* pack, float* work, int wk_stride,
                                      int h_off, void* stream) {
    GruArgs a = {};
    const int rc = gru_rec_args("stream_gru_rec_n", pk, S, hops, work_frames, frame, g, Hg, gi, state, st_stride, st_off, pack, work,
                                wk_stride, h_off, a);
    return rc ? rc : dispatch_kq<KIND_REC>(a, "cruse_stream_gru_rec_n", stream);
}

extern "C" int cruse_stream_decode_n(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                     const float* tab, const float* w, float ln_eps, float* state, float* work, float* out, void* stream) {
    return decode_any({{"cruse_stream_decode_n", pk, S}, {true, hops, out_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out}}, stream);
}

extern "C" int cruse_stream_decode_n_io(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                        const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                                        const float* lim, int* clip, void* stream) {
    return decode_any({{"cruse_stream_decode_n_io", pk, S}, {true, hops, out_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out, out_fmt, lim, clip}}, stream);
}

extern "C" int cruse_stream_decode_n_pf(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                        const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                                        const float* lim, int* clip, int pf_kind, const float* pf_tau, void* stream) {
    return decode_any({{"cruse_stream_decode_n_pf", pk, S}, {true, hops, out_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out, out_fmt, lim, clip}, {true, pf_kind, pf_tau}}, stream);
}

// ---- the upsample decoder of CRUSE4MagAddSkipUpsample (cust_conv.py:163-166,177-184): the _pf argument lists, every form in one pair.
// pf_kind 0: no post-filter, pf_tau is not read; out_fmt 0, null lim and null clip: the plain form.
extern "C" int cruse_stream_decode_up(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                                      float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                                      int pf_kind, const float* pf_tau, void* stream) {
    return decode_any({{"cruse_stream_decode_up", mode, S}, {}, {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out, out_fmt, lim, clip},
                       {false, pf_kind, pf_tau, DEC_UPCONV}}, stream);
}

extern "C" int cruse_stream_decode_n_up(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                                        const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                                        const float* lim, int* clip, int pf_kind, const float* pf_tau, void* stream) {
    return decode_any({{"cruse_stream_decode_n_up", pk, S}, {true, hops, out_hops, work_frames},
                       {{c0, c1, c2, c3, c4}, tab, w, ln_eps, state, work}, {out, out_fmt, lim, clip}, {false, pf_kind, pf_tau, DEC_UPCONV}}, stream);
}

// What a call of an entry point launches: calls fn itself, with plan_out set, on its ints from v in their order, 0 for a float (ln_eps)
// and the null stream.  Bit i of null_mask: its i-th pointer argument is null; the others get a stand-in, which nothing on the host
// reads through.
template <typename... A>
static int plan_call(int (*fn)(A...), const int* v, int null_mask, int* out) {
    static float standin[4];
    int bit = 0;
    auto arg = [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        if constexpr (std::is_pointer<T>::value) return (T)((null_mask >> bit++ & 1) ? nullptr : standin);
        else return std::is_floating_point<T>::value ? T(0) : T(*v++);
    };
    std::tuple<A...> args{arg((A*)nullptr)...};           // a braced list: evaluated left to right
    std::get<sizeof...(A) - 1>(args) = nullptr;           // the stream
    plan_out = out;
    const int rc = std::apply(fn, args);
    plan_out = nullptr;
    return rc;
}

template <auto FN>
static int plan_of(const int* v, int null_mask, int* out) { return plan_call(FN, v, null_mask, out); }

extern "C" int cruse_stream_boundary_plan(int entry, const int* v, int null_mask, int* out) {
    static int (*const entries[])(const int*, int, int*) = {       // in the order of CRUSE_STREAM_ENTRY_*
        plan_of<cruse_stream_encode>, plan_of<cruse_stream_encode_io>, plan_of<cruse_stream_decode>, plan_of<cruse_stream_decode_io>,
        plan_of<cruse_stream_decode_pf>, plan_of<cruse_stream_decode_up>, plan_of<cruse_stream_encode_n>, plan_of<cruse_stream_encode_n_io>,
        plan_of<cruse_stream_decode_n>, plan_of<cruse_stream_decode_n_io>, plan_of<cruse_stream_decode_n_pf>, plan_of<cruse_stream_decode_n_up>,
        plan_of<cruse_stream_df_head>, plan_of<cruse_stream_df_head_n>};
    static_assert(sizeof(entries) / sizeof(*entries) == CRUSE_STREAM_ENTRY_N, "one per entry point");
    CRUSE_REQUIRE(entry >= 0 && entry < CRUSE_STREAM_ENTRY_N && v && out, CRUSE_E_SHAPE, "stream_boundary_plan: entry %d or a null array", entry);
    return entries[entry](v, null_mask, out);
}
