// The DeepFilter head of BASELINE config 4 at inference, in ONE launch (model/deep_filter.py:15-41 with the filter field unet_2 emits:
// one real channel on the first Fn bins).  With P = mask * N on [0,T) x [0,Fn) and zero elsewhere (bins Fn..Fs-1: the zero Nyquist bin,
// repair R8; outside the spectrum: the reference's zero padding),
//
//     E[b,t,f] = sum_{dt = -t_dim..t_dim} sum_{df = -f_dim..f_dim} P[b,t+dt,f+df]        (real and imaginary plane separately)
//
// It replaces, for a trained model, the training composition of engine._deepfilter_loss
//
//     mask_apply_kernel(mask, ones, zeros) -> hr     deepfilter_kernel<0>(nre, nim, hr, zeros) -> E
//
// which reads a plane of ones and two of zeros and writes and re-reads the padded mask: about eleven [B,T,Fs] planes of HBM traffic
// where this kernel moves five (mask, nre, nim in; ere, eim out).  A workgroup owns DH_TF frames x up to DH_FW bins of one clip, forms
// the products of the tile and its halo once in LDS and every thread then sums its window.
//
// Bit contract: the result is the composition's, bit for bit, on finite data.  deepfilter_kernel<0>, called with the two axes exchanged,
// adds its window sequentially from 0.0f with the frame offset as the outer and the bin offset as the inner loop, both ascending; so
// does this kernel.  Its products nre * hr - nim * 0 and nre * 0 + nim * hr equal the single products formed here (an accumulator that
// starts at +0 never becomes -0, so the sign of a zero addend cannot show); contraction is off so that no product is fused into an add.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DH_TF = 16;            // frames per tile
constexpr int DH_FW = 192;           // bins per tile (161 bins: one tile holds the whole frame)
constexpr int DH_THREADS = 256;
constexpr int DH_TD_MAX = 8, DH_FD_MAX = 16;

// TD, FD >= 0: the window is a compile-time constant (the loops unroll into LDS reads at immediate offsets); -1: taken from td, fd.
template <int TD, int FD>
__global__ __launch_bounds__(DH_THREADS) void df_head_kernel(const float* __restrict__ mask, const float* __restrict__ nre,
                                                             const float* __restrict__ nim, int T, int Fn, int Fs, int td_, int fd_,
                                                             int fw, int ntt, int nft, float* __restrict__ ere, float* __restrict__ eim) {
    extern __shared__ float sm[];
    const int td = TD >= 0 ? TD : td_, fd = FD >= 0 ? FD : fd_;
    const int HF = fw + 2 * fd, HT = DH_TF + 2 * td;
    float* pr = sm;
    float* pi = sm + HT * HF;
    const int ft = blockIdx.x % nft, bt = blockIdx.x / nft;
    const int tt = bt % ntt, b = bt / ntt;
    const int t0 = tt * DH_TF, f0 = ft * fw;
    const long long row_b = (long long)b * T;
    // the products of the tile and its halo; every global element under its own bounds test (rows of 161 floats are not 16-byte aligned)
    for (int i = threadIdx.x; i < HT * HF; i += DH_THREADS) {
        const int lt = i / HF, lf = i - lt * HF;
        const int t = t0 - td + lt, f = f0 - fd + lf;
        float a = 0.f, c = 0.f;
        if (t >= 0 && t < T && f >= 0 && f < Fn) {               // (Fn <= Fs: bins Fn .. Fs - 1 stay zero)
            const long long row = row_b + t;
            const float m = mask[row * Fn + f];
            a = m * nre[row * Fs + f];
            c = m * nim[row * Fs + f];
        }
        pr[i] = a; pi[i] = c;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DH_TF * fw; i += DH_THREADS) {
        const int lt = i / fw, lf = i - lt * fw;
        const int t = t0 + lt, f = f0 + lf;
        if (t >= T || f >= Fs) continue;
        const float* qr = pr + lt * HF + lf;
        const float* qi = pi + lt * HF + lf;
        float sr = 0.f, si = 0.f;
        if constexpr (TD >= 0 && FD >= 0) {
#pragma unroll
            for (int dt = 0; dt <= 2 * TD; ++dt)
#pragma unroll
                for (int df = 0; df <= 2 * FD; ++df) {
                    sr += qr[dt * HF + df];
                    si += qi[dt * HF + df];
                }
        } else {
            for (int dt = 0; dt <= 2 * td; ++dt)
                for (int df = 0; df <= 2 * fd; ++df) {
                    sr += qr[dt * HF + df];
                    si += qi[dt * HF + df];
                }
        }
        const long long o = (row_b + t) * Fs + f;
        ere[o] = sr; eim[o] = si;
    }
}

}  // namespace

extern "C" int cruse_df_head_apply(const float* mask, const float* nre, const float* nim, int B, int T, int Fn, int Fs, int t_dim,
                                   int f_dim, float* ere, float* eim, void* stream) {
    CRUSE_REQUIRE(B > 0 && T > 0 && Fn > 0 && Fs > 0, CRUSE_E_SHAPE, "df_head_apply: empty shape B=%d T=%d Fn=%d Fs=%d", B, T, Fn, Fs);
    CRUSE_REQUIRE(Fn <= Fs, CRUSE_E_SHAPE, "df_head_apply: the mask has Fn=%d bins, the spectrum only Fs=%d", Fn, Fs);
    CRUSE_REQUIRE(t_dim >= 0 && t_dim <= DH_TD_MAX && f_dim >= 0 && f_dim <= DH_FD_MAX, CRUSE_E_SHAPE,
                  "df_head_apply: t_dim=%d (0..%d), f_dim=%d (0..%d)", t_dim, DH_TD_MAX, f_dim, DH_FD_MAX);
    CRUSE_REQUIRE(mask && nre && nim && ere && eim, CRUSE_E_SHAPE, "df_head_apply: a tensor is NULL");
    const int fw = Fs < DH_FW ? Fs : DH_FW;
    const int ntt = cdiv(T, DH_TF), nft = cdiv(Fs, fw);
    const long long grid = (long long)B * ntt * nft;
    CRUSE_REQUIRE(grid <= 0x7fffffffLL, CRUSE_E_SHAPE, "df_head_apply: B=%d T=%d Fs=%d is %lld tiles, more than one grid holds", B, T, Fs, grid);
    const size_t lds = (size_t)2 * (DH_TF + 2 * t_dim) * (fw + 2 * f_dim) * sizeof(float);       // <= 2 * 32 * 224 * 4 = 56 KB
    hipStream_t st = (hipStream_t)stream;
    if (t_dim == 1 && f_dim == 5)
        hipLaunchKernelGGL((df_head_kernel<1, 5>), dim3((unsigned)grid), dim3(DH_THREADS), lds, st, mask, nre, nim, T, Fn, Fs, t_dim, f_dim, fw,
                           ntt, nft, ere, eim);
    else {
        const int rc = cruse_ensure_dyn_lds(reinterpret_cast<const void*>(df_head_kernel<-1, -1>), lds, "df_head_apply");
        if (rc) return rc;
        hipLaunchKernelGGL((df_head_kernel<-1, -1>), dim3((unsigned)grid), dim3(DH_THREADS), lds, st, mask, nre, nim, T, Fn, Fs, t_dim, f_dim, fw,
                           ntt, nft, ere, eim);
    }
    CRUSE_LAUNCH_CHECK("df_head_apply");
    return CRUSE_OK;
}
