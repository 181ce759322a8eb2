// Frame-by-frame streaming inference of unet_2 (n_fft = win = 320, hop = 160): one hop of every active slot is
// encode -> GRU layer 1 -> GRU layer 2 -> decode, four dependent launches on one stream (cruse_stream_* in cruse_hip.h).
//
// The model is causal in time: the encoder convs are (2,3) with time padding 1 and the trailing frame cropped, so frame t
// reads input rows t-1 and t of each level (the previous row is per-slot state); skip and decoder convs are (1,3); both
// GRU layers are uni-directional; eval-mode BatchNorm is a per-channel affine, folded into the conv weights by the host.
// All arithmetic is f32 with f32 accumulation.  Every kernel reads the per-slot mode (CRUSE_STREAM_MODE_*) from device
// memory; a slot whose mode is SKIP is not touched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include "common.h"

namespace {

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

// level-k encoder conv (2,3), stride (1,2), frequency padding 1, BN folded, ReLU: out[co][f] from the previous and current
// input rows [Cin][Fin]
__device__ void enc_conv(const float* __restrict__ W, const float* __restrict__ b, const float* prev, const float* cur,
                         float* out, int Cin, int Fin, int Cout, int Fout) {
    for (int idx = threadIdx.x; idx < Cout * Fout; idx += blockDim.x) {
        const int co = idx / Fout, f = idx - co * Fout;
        float acc = b[co];
        for (int ci = 0; ci < Cin; ++ci) {
            const float* w = W + (co * Cin + ci) * 6;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int fi = 2 * f - 1 + kw;
                if (fi < 0 || fi >= Fin) continue;
                acc = fmaf(w[kw], prev[ci * Fin + fi], acc);
                acc = fmaf(w[3 + kw], cur[ci * Fin + fi], acc);
            }
        }
        out[idx] = fmaxf(acc, 0.f);
    }
}

// skip conv (1,3), padding (0,1), no bias: [C][F] -> [C][F]
__device__ void skip_conv(const float* __restrict__ W, const float* e, float* out, int C, int F) {
    for (int idx = threadIdx.x; idx < C * F; idx += blockDim.x) {
        const int co = idx / F, f = idx - co * F;
        float acc = 0.f;
        for (int ci = 0; ci < C; ++ci) {
            const float* w = W + (co * C + ci) * 3;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int fi = f - 1 + kw;
                if (fi >= 0 && fi < F) acc = fmaf(w[kw], e[ci * F + fi], acc);
            }
        }
        out[idx] = acc;
    }
}

// ConvTranspose (1,3), stride (1,2), last column cropped: [Cin][Fin] -> [Cout][2*Fin]; W packed [Cin][Cout][3] (BN folded)
// act 0: ReLU then + add[co][fo]; act 1: sigmoid
__device__ void dec_convt(const float* __restrict__ W, const float* __restrict__ b, const float* in, float* out,
                          const float* __restrict__ add, int Cin, int Fin, int Cout, int act) {
    const int Fout = 2 * Fin;
    for (int idx = threadIdx.x; idx < Cout * Fout; idx += blockDim.x) {
        const int co = idx / Fout, fo = idx - co * Fout;
        float acc = b[co];
        if (fo & 1) {
            const int fi = fo >> 1;
            for (int ci = 0; ci < Cin; ++ci) acc = fmaf(W[(ci * Cout + co) * 3 + 1], in[ci * Fin + fi], acc);
        } else {
            const int fi = fo >> 1;
            for (int ci = 0; ci < Cin; ++ci) {
                acc = fmaf(W[(ci * Cout + co) * 3 + 0], in[ci * Fin + fi], acc);
                if (fi >= 1) acc = fmaf(W[(ci * Cout + co) * 3 + 2], in[ci * Fin + fi - 1], acc);
            }
        }
        out[idx] = act == 0 ? fmaxf(acc, 0.f) + add[idx] : 1.0f / (1.0f + expf(-acc));
    }
}

// tables: [0,320) periodic Hann, [320,640) cos(2 pi j / 320), [640,960) sin(2 pi j / 320), [960,1120) 1 / (w^2(m) + w^2(m+160))
constexpr int TB_WIN = 0, TB_COS = 320, TB_SIN = 640, TB_IENV = 960, TB_TOTAL = 1120;

__global__ void __launch_bounds__(1024) stream_encode_kernel(const int* __restrict__ mode, Layout L, const float* __restrict__ in,
                                                            const float* __restrict__ tab, const float* __restrict__ w,
                                                            float* __restrict__ state, float* __restrict__ work) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, m = mode[s];
    if (m == CRUSE_STREAM_MODE_SKIP) return;
    float* st = state + (size_t)s * L.st_stride;
    float* wk = work + (size_t)s * L.wk_stride;
    const float* blk = in + (size_t)s * HOP;
    const int tid = threadIdx.x;
    if (m == CRUSE_STREAM_MODE_STORE) {
        for (int i = tid; i < HOP; i += blockDim.x) st[L.st_hist + 1 + i] = blk[i];
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
            a = i == 0 ? blk[0] : hist[161 - i];
            bq = hist[1 + i];
        } else if (m == CRUSE_STREAM_MODE_END) {      // last block | x[L-2], ..., x[L-161]
            a = hist[1 + i];
            bq = hist[159 - i];
        } else {                                      // previous block | this block
            a = hist[1 + i];
            bq = blk[i];
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
        for (int i = tid; i < HOP; i += blockDim.x) st[L.st_hist + 1 + i] = blk[i];
    }
    // 320-point real DFT, bins 0..160; magnitude of bins 0..159
    for (int k = tid; k < NB; k += blockDim.x) {
        float re = 0.f, im = 0.f;
        int j = 0;
        for (int n = 0; n < NFFT; ++n) {
            re = fmaf(fr[n], tab[TB_COS + j], re);
            im = fmaf(-fr[n], tab[TB_SIN + j], im);
            j += k;
            if (j >= NFFT) j -= NFFT;
        }
        spec[k] = re;
        spec[NB + k] = im;
        wk[L.wk_re + k] = re;
        wk[L.wk_im + k] = im;
        if (k < F0) cur[0][k] = sqrtf(re * re + im * im + 1e-8f);
    }
    __syncthreads();
    for (int k = 1; k < 5; ++k) {
        enc_conv(w + L.encW[k], w + L.encB[k], prv[k - 1], cur[k - 1], cur[k], L.ch[k - 1], L.F[k - 1], L.ch[k], L.F[k]);
        __syncthreads();
    }
    for (int k = 1; k < 5; ++k) skip_conv(w + L.skW[k], cur[k], wk + L.wk_skip[k], L.ch[k], L.F[k]);
    for (int i = tid; i < L.H; i += blockDim.x) wk[L.wk_x + i] = cur[4][i];        // GRU input row, c*F4+f
    for (int k = 0; k < 4; ++k)
        for (int i = tid; i < L.ch[k] * L.F[k]; i += blockDim.x) st[L.st_prev[k] + i] = cur[k][i];
}

// One GGRU layer, one time step, for every slot whose mode computes a frame.  Workgroup: 4 waves, wave w owns hidden unit
// blockIdx.y*4 + w (all three gates); its lanes hold that unit's six weight rows (W_ih, W_hh x r,z,n) in registers, k = lane + 64q,
// and loop over tiles of SB slots whose input / state chunks are staged in LDS.  Layer 2 (LN1 != nullptr) stages the whole
// layer-1 output row and applies LN1 to the interleaved vector v[j*g+i] = h1[i*Hg+j] on the fly.
constexpr int SB = 8;

template <int KQ>
__global__ void __launch_bounds__(256) stream_gru_kernel(const int* __restrict__ mode, int S, int g, int Hg,
                                                         const float* __restrict__ x, int x_stride, int x_off,
                                                         const float* __restrict__ ln_g, const float* __restrict__ ln_b, float ln_eps,
                                                         const float* __restrict__ hprev, int h_stride, int h_off,
                                                         const float* __restrict__ pack, float* __restrict__ hout, int o_stride, int o_off) {
    extern __shared__ float sm[];
    const int H = g * Hg;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.y * 4 + wv;          // unit of the whole layer: group gi, unit j within it
    const int gi = u / Hg, j = u - gi * Hg;
    const bool ln = ln_g != nullptr;
    const int xw = ln ? H : Hg;                 // floats staged per slot for the input
    float* xs = sm;                             // [SB][xw]
    float* hs = sm + SB * xw;                   // [SB][Hg]
    float* st = hs + SB * Hg;                   // [SB][2] mean, rstd
    const size_t gsz = (size_t)3 * Hg * Hg;
    const float* Wih = pack + gi * gsz;
    const float* Whh = pack + g * gsz + gi * gsz;
    const float* bih = pack + 2 * g * gsz + gi * 3 * Hg;
    const float* bhh = pack + 2 * g * gsz + g * 3 * Hg + gi * 3 * Hg;
    float wi[3][KQ], wh[3][KQ], lg[KQ], lb[KQ];
    int src[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = lane + 64 * q;
        const bool ok = k < Hg;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            wi[c][q] = ok ? Wih[(size_t)(c * Hg + j) * Hg + k] : 0.f;
            wh[c][q] = ok ? Whh[(size_t)(c * Hg + j) * Hg + k] : 0.f;
        }
        const int p = gi * Hg + k;              // position in the LN1 output vector this layer-2 group reads
        src[q] = ok ? (ln ? (p % g) * Hg + p / g : k) : 0;
        lg[q] = (ln && ok) ? ln_g[p] : 0.f;
        lb[q] = (ln && ok) ? ln_b[p] : 0.f;
    }
    const float br = bih[j] + bhh[j], bz = bih[Hg + j] + bhh[Hg + j], bin = bih[2 * Hg + j], bhn = bhh[2 * Hg + j];
    const int ntiles = (S + SB - 1) / SB;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int s0 = t * SB;
        __syncthreads();
        for (int i = threadIdx.x; i < SB * xw; i += blockDim.x) {
            const int ss = i / xw, k = i - ss * xw, s = s0 + ss;
            xs[i] = s < S ? x[(size_t)s * x_stride + x_off + (ln ? 0 : gi * Hg) + k] : 0.f;
        }
        for (int i = threadIdx.x; i < SB * Hg; i += blockDim.x) {
            const int ss = i / Hg, k = i - ss * Hg, s = s0 + ss;
            hs[i] = s < S ? hprev[(size_t)s * h_stride + h_off + gi * Hg + k] : 0.f;
        }
        __syncthreads();
        if (ln) {                               // LN1 statistics of each staged row (two passes, biased variance)
            for (int ss = wv; ss < SB; ss += 4) {
                float a = 0.f;
                for (int k = lane; k < H; k += 64) a += xs[ss * H + k];
                const float mean = wave_sum(a) / H;
                float v = 0.f;
                for (int k = lane; k < H; k += 64) { const float d = xs[ss * H + k] - mean; v = fmaf(d, d, v); }
                const float var = wave_sum(v) / H;
                if (lane == 0) { st[2 * ss] = mean; st[2 * ss + 1] = 1.0f / sqrtf(var + ln_eps); }
            }
            __syncthreads();
        }
        for (int ss = 0; ss < SB; ++ss) {
            const int s = s0 + ss;
            if (s >= S) break;
            const int m = mode[s];
            if (m != CRUSE_STREAM_MODE_FRAME && m != CRUSE_STREAM_MODE_FRAME0 && m != CRUSE_STREAM_MODE_END) continue;
            float ar = 0.f, az = 0.f, ain = 0.f, ahn = 0.f;
            const float mean = ln ? st[2 * ss] : 0.f, rstd = ln ? st[2 * ss + 1] : 0.f;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int k = lane + 64 * q;
                if (k >= Hg) continue;
                float xv = xs[ss * xw + src[q]];
                if (ln) xv = fmaf((xv - mean) * rstd, lg[q], lb[q]);
                const float hv = hs[ss * Hg + k];
                ar = fmaf(wi[0][q], xv, ar); ar = fmaf(wh[0][q], hv, ar);
                az = fmaf(wi[1][q], xv, az); az = fmaf(wh[1][q], hv, az);
                ain = fmaf(wi[2][q], xv, ain);
                ahn = fmaf(wh[2][q], hv, ahn);
            }
            ar = wave_sum(ar); az = wave_sum(az); ain = wave_sum(ain); ahn = wave_sum(ahn);
            if (lane == 0) {
                const float r = 1.0f / (1.0f + expf(-(ar + br)));
                const float z = 1.0f / (1.0f + expf(-(az + bz)));
                const float n = tanhf(ain + bin + r * (ahn + bhn));
                const float hp = hs[ss * Hg + j];
                hout[(size_t)s * o_stride + o_off + u] = (1.0f - z) * n + z * hp;
            }
        }
    }
}

__global__ void __launch_bounds__(1024) stream_decode_kernel(const int* __restrict__ mode, Layout L, const float* __restrict__ tab,
                                                            const float* __restrict__ w, float ln_eps, float* __restrict__ state,
                                                            float* __restrict__ work, float* __restrict__ out) {
    extern __shared__ float sm[];
    const int s = blockIdx.x, m = mode[s];
    if (m != CRUSE_STREAM_MODE_FRAME && m != CRUSE_STREAM_MODE_FRAME0 && m != CRUSE_STREAM_MODE_END) return;
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
        dec_convt(w + L.decW[k], w + L.decB[k], row[k], row[k - 1], k > 1 ? wk + L.wk_skip[k - 1] : nullptr, L.ch[k], L.F[k],
                  L.ch[k - 1], k > 1 ? 0 : 1);
        __syncthreads();
    }
    // mask on bins 0..159 (bin 160 zero), 320-point inverse real DFT (imaginary parts of bins 0 and 160 ignored, as irfft)
    for (int i = tid; i < F0; i += blockDim.x) {
        wk[L.wk_mask + i] = row[0][i];
        re[i] *= row[0][i];
        im[i] *= row[0][i];
    }
    if (tid == 0) { re[F0] = 0.f; im[F0] = 0.f; }
    __syncthreads();
    for (int n = tid; n < NFFT; n += blockDim.x) {
        float acc = 0.f;
        int j = n;
        for (int k = 1; k < F0; ++k) {
            acc = fmaf(re[k], tab[TB_COS + j], acc);
            acc = fmaf(-im[k], tab[TB_SIN + j], acc);
            j += n;
            if (j >= NFFT) j -= NFFT;
        }
        y[n] = (re[0] + 2.0f * acc + ((n & 1) ? -re[F0] : re[F0])) * (1.0f / NFFT) * tab[TB_WIN + n];
    }
    __syncthreads();
    // overlap-add with the stored tail, divide by the window envelope: output block; the second half becomes the tail
    for (int i = tid; i < HOP; i += blockDim.x) {
        out[(size_t)s * HOP + i] = (st[L.st_tail + i] + y[i]) * tab[TB_IENV + i];
        st[L.st_tail + i] = y[HOP + i];
    }
}

template <int KQ>
int launch_gru(const int* mode, int S, int g, int Hg, const float* x, int xs, int xo, const float* lng, const float* lnb, float eps,
               const float* hp, int hs, int ho, const float* pack, float* out, int os, int oo, int grid_x, hipStream_t st) {
    const int H = g * Hg;
    const size_t lds = (size_t)(SB * ((lng ? H : Hg) + Hg) + 2 * SB) * sizeof(float);
    int rc = cruse_ensure_dyn_lds((const void*)stream_gru_kernel<KQ>, lds, "cruse_stream_gru");
    if (rc) return rc;
    hipLaunchKernelGGL(stream_gru_kernel<KQ>, dim3(grid_x, H / 4), dim3(256), lds, st, mode, S, g, Hg, x, xs, xo, lng, lnb, eps, hp, hs,
                       ho, pack, out, os, oo);
    CRUSE_LAUNCH_CHECK("cruse_stream_gru");
    return CRUSE_OK;
}

}  // namespace

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
    Layout L;
    int rc = make_layout(c0, c1, c2, c3, c4, L);
    if (rc) return rc;
    CRUSE_REQUIRE(S > 0 && mode && in && tab && w && state && work, CRUSE_E_SHAPE, "stream_encode: S = %d or a null buffer", S);
    int n = NFFT + 2 * NB;
    for (int k = 0; k < 5; ++k) n += L.ch[k] * L.F[k];
    for (int k = 0; k < 4; ++k) n += L.ch[k] * L.F[k];
    const size_t lds = (size_t)n * sizeof(float);
    rc = cruse_ensure_dyn_lds((const void*)stream_encode_kernel, lds, "cruse_stream_encode");
    if (rc) return rc;
    hipLaunchKernelGGL(stream_encode_kernel, dim3(S), dim3(FRAME_THREADS), lds, (hipStream_t)stream, mode, L, in, tab, w, state, work);
    CRUSE_LAUNCH_CHECK("cruse_stream_encode");
    return CRUSE_OK;
}

extern "C" int cruse_stream_gru(const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                                const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                                const float* pack, float* hout, int o_stride, int o_off, void* stream) {
    CRUSE_REQUIRE(S > 0 && g > 0 && Hg > 0 && Hg % 4 == 0 && Hg <= 1024, CRUSE_E_SHAPE,
                  "stream_gru: S = %d, g = %d, Hg = %d (need Hg %% 4 == 0, Hg <= 1024)", S, g, Hg);
    CRUSE_REQUIRE(layer == 1 || layer == 2, CRUSE_E_SHAPE, "stream_gru: layer %d", layer);
    CRUSE_REQUIRE(mode && x && hprev && pack && hout && (layer == 1 || (ln_g && ln_b)), CRUSE_E_SHAPE, "stream_gru: null buffer");
    if (layer == 1) ln_g = ln_b = nullptr;
    // enough workgroups to cover the device, each keeping its unit's weights in registers across several slot tiles
    const int units = g * Hg / 4, ntiles = (S + SB - 1) / SB;
    const int grid_x = std::max(1, std::min(ntiles, (2048 + units - 1) / units));
    hipStream_t st = (hipStream_t)stream;
    if (Hg <= 192) return launch_gru<3>(mode, S, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off, pack, hout, o_stride, o_off, grid_x, st);
    if (Hg <= 320) return launch_gru<5>(mode, S, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off, pack, hout, o_stride, o_off, grid_x, st);
    if (Hg <= 640) return launch_gru<10>(mode, S, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off, pack, hout, o_stride, o_off, grid_x, st);
    return launch_gru<16>(mode, S, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off, pack, hout, o_stride, o_off, grid_x, st);
}

extern "C" int cruse_stream_decode(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                                   float ln_eps, float* state, float* work, float* out, void* stream) {
    Layout L;
    int rc = make_layout(c0, c1, c2, c3, c4, L);
    if (rc) return rc;
    CRUSE_REQUIRE(S > 0 && mode && tab && w && state && work && out, CRUSE_E_SHAPE, "stream_decode: S = %d or a null buffer", S);
    int n = 2 * NB + NFFT + FRAME_THREADS / 64;
    for (int k = 0; k < 5; ++k) n += L.ch[k] * L.F[k];
    const size_t lds = (size_t)n * sizeof(float);
    rc = cruse_ensure_dyn_lds((const void*)stream_decode_kernel, lds, "cruse_stream_decode");
    if (rc) return rc;
    hipLaunchKernelGGL(stream_decode_kernel, dim3(S), dim3(FRAME_THREADS), lds, (hipStream_t)stream, mode, L, tab, w, ln_eps, state, work, out);
    CRUSE_LAUNCH_CHECK("cruse_stream_decode");
    return CRUSE_OK;
}
