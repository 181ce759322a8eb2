/* libcruse_hip.so -- C ABI of the MI355X (gfx950) CRUSE hot path.
 *
 * The reference (Okrio/CRUSE) is pure Python and has no FFI; its extension point
 * is dotted-path module loading (train_base/utils.py:68-100).  Every entry point
 * below therefore replaces a *PyTorch library op at one of the reference's call
 * sites* (SURVEY.md section 2b); the call site is cited on each declaration.
 * Host code (cruse_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - extern "C"; every function returns int: 0 = ok, <0 = CRUSE_E_*;
 *     cruse_last_error() returns a thread-local message.
 *   - all buffers are caller-allocated DEVICE pointers (f32 unless noted); the
 *     library never frees or retains them beyond the call.
 *   - last argument is the hipStream_t (passed as void*); calls are asynchronous
 *     and re-entrant per stream; no global mutable state.
 *   - activation layout is "frame-major": [B, T, C, F] contiguous, i.e. one row of
 *     C*F floats per spectrogram frame.  For C == 1 this is the reference's
 *     [B,1,T,F]; GGRU's [B,T,C*F] view (model/cruse_net.py:39-40) is this layout
 *     with no copy.
 *   - "+=" outputs accumulate into the caller's buffer (gradient buffers).
 */
#ifndef CRUSE_HIP_H
#define CRUSE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRUSE_ABI_VERSION 15

enum {
    CRUSE_OK = 0,
    CRUSE_E_SHAPE = -1,
    CRUSE_E_ALIGN = -2,
    CRUSE_E_DTYPE = -3,
    CRUSE_E_HIP = -4,
    CRUSE_E_TIMEOUT = -5
};

/* precision of the MFMA contractions (GEMMs and GRU recurrence) */
enum {
    CRUSE_PREC_F32 = 0,    /* v_mfma_f32_16x16x4_f32: exact f32                         */
    CRUSE_PREC_BF16X3 = 1, /* split bf16 hi+lo, 3 bf16 MFMAs: ~2^-17 relative           */
    CRUSE_PREC_BF16 = 2,   /* operands rounded to bf16, f32 accumulate                  */
    CRUSE_PREC_F16 = 3     /* v_mfma_f32_16x16x32_f16: operands rounded to f16, f32 accumulate (cruse_gemm; BASELINE config 5) */
};

/* storage type of the activation tensors of the general [B,C,H,W] blocks (cruse_conv2d_nchw, cruse_bn_nchw_*, ...):
 * BASELINE config 5 ("MTFAA ... fp16") keeps them in f16 -- the blocks are HBM-bound, so the bytes are what fp16 buys --
 * with f32 parameters, parameter gradients, accumulation and statistics; its pointwise convolutions run on
 * v_mfma_f32_16x16x32_f16. */
enum {
    CRUSE_DT_F32 = 0,
    CRUSE_DT_F16 = 1,
    CRUSE_DT_BF16 = 2     /* backward-only tensors of the bf16 mode (x_dtype / a_dtype / bt_dtype / dy_dtype below) */
};

int cruse_abi_version(void);
const char* cruse_last_error(void);
/* Library options -- kernel-selection A/B switches and profiling aids, set EXPLICITLY by the host (the library reads no
 * environment variables).  The 17 names (any other is refused): "gru_bwd_rs" / "gru_fwd_lean" 0 = the generic recurrence kernels
 * in bf16 mode; "gru_tf" 0 = the tagged hand-off kernels; "gru_poll_fwd" / "gru_poll_bwd" poll delay of the hand-off; "gru_wlo"
 * 0 / 1 = W_hh low plane of the lean forward recurrence off / on for every Hg (unset: on for Hg <= 320); "gru_dbg", "cm_dbg",
 * "wg_dbg" phase-skip / phase-stamp profiling; "cm_nw", "cm_grid", "wg_grid" launch geometry overrides; "cm_kint", "cm_swap",
 * "wg_rd" 0 = without the k-interleaved weights / swapped operand roles / direct-read weight gradient; "pw_valu" 1 = VALU kernels
 * for the NCHW convolutions in f16 storage, 2 = their gather pointwise MFMA kernel; "dw_nolds" 1 = the f16 depthwise kernels
 * without the LDS image.  unset != 0 restores the default. */
int cruse_set_option(const char* name, int value, int unset);
int cruse_get_option(const char* name, int* value, int* is_set);

/* ---- acoustic front end ---------------------------------------------------- */

/* torch.stft(y, n_fft, hop, win=n_fft, window=hann_window(n_fft), center=True,
 * return_complex=True) at train_base/acoustics/feature.py:22-30, fused with the
 * [B,T,F] transposition and magnitude of utils/utils.py:397-400.
 * wave [B,L] -> re, im [B,T,n_fft/2+1] (either may be NULL),
 *               mag [B,T,mag_bins] = sqrt(re^2+im^2+mag_eps) for the first mag_bins bins (may be NULL).
 * T = 1 + L/hop.  Reflect padding of n_fft/2.  n_fft == 320 runs the radix-5 x 64
 * wavefront-shuffle FFT; any other even n_fft <= 2048 a direct DFT. */
int cruse_stft_fwd(const float* wave, int B, int L, int n_fft, int hop,
                   float* re, float* im, float* mag, int mag_bins, float mag_eps, void* stream);

/* torch.istft(X, n_fft, hop, win=n_fft, window=hann_window(n_fft), center=True, length=L)
 * at feature.py:53-61 / utils/utils.py:448-454.  re, im [B,T,n_fft/2+1] -> wave [B,L]. */
int cruse_istft_fwd(const float* re, const float* im, int B, int T, int n_fft, int hop, int L,
                    float* wave, void* stream);
/* adjoint of cruse_istft_fwd: dwave [B,L] -> dre, dim [B,T,n_fft/2+1].  A sample whose window-square envelope is <= 1e-11 (every sample
 * hop * t at hop = n_fft, where the Hann window is 0) is 0 in the forward for any spectrum and so contributes 0 here: the outputs are
 * finite.  L > hop * (T - 1) + n_fft/2 is refused (CRUSE_E_SHAPE) as the forward refuses it.  dim of bins 0 and n_fft/2 is 0. */
int cruse_istft_bwd(const float* dwave, int B, int T, int n_fft, int hop, int L,
                    float* dre, float* dim, void* stream);

/* ---- convolutions (nn.Conv2d / nn.ConvTranspose2d at model/cruse_net.py:138-143,149-164) */

/* gather form:
 *   y[b,t,co,fo] (+)= act(bias[co] + sum_{ci,kt,kf} W(co,ci,kt,kf) * x[b, t-(KT-1)+kt, ci, fo*S - pad + kf])
 * zero outside the clip.  kf in 0..2.  w_layout 0: W = w[co][ci][kt][kf] (Conv2d weight, or a
 * ConvTranspose2d weight read as [out=Cin_t][in=Cout_t] for its backward-data).
 * w_layout 1 (KT == 1, S == 1): W(co,ci,0,kf) = w[ci][co][0][2-kf] (backward-data of a stride-1 conv).
 * act 0 none, 1 sigmoid.  accum != 0: y += result (act must be 0). bias may be NULL.
 * prec: CRUSE_PREC_* selects the MFMA implicit-GEMM kernel (Cin % 8 == 0, 8 <= Cout <= 64);
 * prec < 0, or an ineligible shape (Cin == 1, Cout == 1), runs the exact-f32 VALU kernel. */
int cruse_conv_gather(const float* x, const float* w, const float* bias, float* y,
                      int B, int T, int Cin, int Fin, int Cout, int Fout,
                      int KT, int S, int pad, int w_layout, int act, int accum, int prec, int x_dtype, int y_dtype, void* stream);

/* scatter form, frequency stride 2:
 *   y[b,t,co,fo] (+)= act(bias[co] + sum_{cs,kt,kf : (fo+pad-kf) even} w[cs][co][kt][kf] *
 *                                     g[b, t+(KT-1)-kt, cs, (fo+pad-kf)/2])
 * ConvTranspose2d((1,3), stride (1,2)) forward with the [..., :-1] crop (cruse_net.py:161-164):
 * KT=1, pad=0, Fout=2*Fg.  Backward-data of the (2,3)/(1,2) encoder conv: KT=2, pad=1. */
int cruse_conv_scatter2(const float* g, const float* w, const float* bias, float* y,
                        int B, int T, int Cs, int Fg, int Cout, int Fout,
                        int KT, int pad, int act, int accum, int prec, int x_dtype, int y_dtype, void* stream);

/* Both forms with the batch statistics of the BatchNorm2d that follows every encoder / decoder conv
 * (cruse_net.py:139,150) accumulated by the conv's own epilogue: y = conv (no activation, no accumulate), and what
 * cruse_bn_stats(y) would add -- sum_{b,t,f} y and sum y^2 per channel -- without the extra pass over y.
 * sums is [CRUSE_BN_STAT_REPLICAS][2*Cout] doubles: a workgroup adds its partial sums to replica (block id mod
 * replicas), so the f64 atomics of ~1000 workgroups do not queue on 2*Cout addresses (that queue cost 15-30 us per
 * layer); the statistic is the sum over the replicas -- cruse_bn_finalize_act_fwd(sum_replicas) folds them.  The
 * partial sums are f32-valued, so the f64 additions are exact and the result does not depend on their order.
 * zeroed != 0: the caller has cleared sums (else cleared here, on `stream`). */
#define CRUSE_BN_STAT_REPLICAS 16
int cruse_conv_gather_bnstats(const float* x, const float* w, const float* bias, float* y,
                              int B, int T, int Cin, int Fin, int Cout, int Fout,
                              int KT, int S, int pad, int prec, double* sums, int zeroed, void* stream);
int cruse_conv_scatter2_bnstats(const float* g, const float* w, const float* bias, float* y,
                                int B, int T, int Cs, int Fg, int Cout, int Fout,
                                int KT, int pad, int prec, double* sums, int zeroed, void* stream);

/* FORWARD convolutions that apply the BatchNorm2d(train) + ReLU of the layer BELOW to their input while staging it (ABI 7; the
 * BN -> ReLU -> conv chains of cruse_net.py:149-152,161-163): x_pre / g_pre is the PRE-BatchNorm tensor [B,T,Cin,Fin]; every workgroup
 * derives mean / rstd from that layer's batch sums in_sums [in_replicas][2*Cin] (in_count = rows*Fin elements per channel) and stages
 * e = relu((x - mean)*rstd*gamma + beta) [+ in_add, the decoder's skip tensor] -- cruse_bn_finalize_act_fwd's arithmetic, so the
 * normalised tensor never exists in HBM.  in_mean / in_rstd (nullable pair): block 0 publishes the statistics (the backward pass
 * reads them) and, with in_running_mean / in_running_var, updates the running statistics -- ONE consumer of a layer passes them.
 * in_copy_bf16 (nullable): a bf16 copy of the transformed rows, the operand the weight gradients of the bf16 mode read.
 * out_sums (nullable): the batch sums of y as cruse_conv_*_bnstats.  MFMA kernel only: prec == CRUSE_PREC_BF16X3 (the forward
 * convs of the bf16 mode), Cin a power of two in 8..64, 8 <= Cout <= 64; anything else is refused (run the unfused passes). */
int cruse_conv_gather_bnin(const float* x_pre, const double* in_sums, int in_replicas, long long in_count, float eps, float momentum,
                           const float* in_gamma, const float* in_beta, float* in_mean, float* in_rstd, float* in_running_mean,
                           float* in_running_var, const float* in_add, void* in_copy_bf16,
                           const float* w, const float* bias, float* y, int B, int T, int Cin, int Fin, int Cout, int Fout,
                           int KT, int S, int pad, int prec, double* out_sums, int zeroed, void* stream);
int cruse_conv_scatter2_bnin(const float* g_pre, const double* in_sums, int in_replicas, long long in_count, float eps, float momentum,
                             const float* in_gamma, const float* in_beta, float* in_mean, float* in_rstd, float* in_running_mean,
                             float* in_running_var, const float* in_add, void* in_copy_bf16,
                             const float* w, const float* bias, float* y, int B, int T, int Cs, int Fg, int Cout, int Fout,
                             int KT, int pad, int prec, double* out_sums, int zeroed, void* stream);

/* x_dtype / a_dtype / bt_dtype / dy_dtype (ABI 7; CRUSE_DT_F32 or CRUSE_DT_BF16): BACKWARD-ONLY tensors of the bf16 mode -- the
 * BatchNorm-backward output dy, which its two consumers (the data-gradient conv and the weight gradient) round to bf16 operands
 * anyway -- may be stored as bf16 in the same [B,T,C,F] layout: half the bytes written once and read twice, the same bits into
 * the MFMAs.  bf16 inputs need the MFMA kernels (CRUSE_PREC_BF16 for the weight gradient); the VALU fall-backs refuse them.
 * y_dtype / dout_dtype: the data gradients themselves (de, du: conv output -> BatchNorm-backward input, skip-path leaves) as bf16
 * too -- sums and accumulation stay f32, the stored value is rounded once per pass; a bf16 output goes with a bf16 input and
 * the swapped-role (vector-store) forms of the MFMA conv. */
/* DATA-GRADIENT convolutions whose output y is the gradient wrt the OUTPUT of a BatchNorm2d(+ReLU) (the backward pass of
 * cruse_net.py:139-142,149-152 walks conv -> BN -> ReLU stacks, so every data gradient but the first feeds a BatchNorm
 * backward): the conv's epilogue also accumulates what cruse_bn_act_bwd_reduce(dout = y, bn_y, ...) would -- sum g and
 * sum g*xhat per channel, g = y masked by the ReLU, xhat from the pre-BN tensor bn_y [B,T,Cout,Fout] -- into
 * sums [CRUSE_BN_STAT_REPLICAS][2*Cout] (cruse_bn_act_bwd_apply(sum_replicas) folds them): that pass over (y, bn_y), 132 MB
 * and ~47 us per level at the bench shape, is not needed.  No bias, no activation; accum != 0: y += conv (the skip path's
 * gradient is already there) and the statistics are those of the sum.  Shapes without the MFMA kernel run the conv and
 * then the reduce pass (into replica 0).  The per-workgroup partial sums are f32, added in f64: independent of order. */
int cruse_conv_gather_bnbwd(const float* x, const float* w, float* y, int B, int T, int Cin, int Fin, int Cout, int Fout,
                            int KT, int S, int pad, int w_layout, int accum, int prec,
                            const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            int relu, double* sums, int zeroed, int x_dtype, int y_dtype, void* stream);
int cruse_conv_scatter2_bnbwd(const float* g, const float* w, float* y, int B, int T, int Cs, int Fg, int Cout, int Fout,
                              int KT, int pad, int accum, int prec,
                              const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                              int relu, double* sums, int zeroed, int x_dtype, int y_dtype, void* stream);

/* (ABI 8) DATA-GRADIENT convolutions that also apply the BatchNorm2d(+ReLU) BACKWARD of their INPUT: dout is the gradient wrt the OUTPUT of
 * the BatchNorm above the convolution being differentiated (cruse_net.py:139-142,149-152: conv -> BN -> ReLU), in_y that BatchNorm's pre-BN
 * tensor [B,T,Cin,Fin], in_sums its backward batch sums [in_replicas][2*Cin] (sum g, sum g*xhat -- from cruse_conv_*_bnbwd or
 * cruse_bn_act_bwd_reduce).  One call = cruse_bn_act_bwd_apply(dout -> dy_bf16; in_dgamma / in_dbeta / in_dbias += ...) followed by
 * cruse_conv_gather / _scatter2 [_bnbwd] (dy_bf16 -> y): in the bf16 data-gradient mode with a bf16 dout the MFMA kernel forms dy while it
 * stages its tiles (the arithmetic of cruse_bn_act_bwd_apply, rounded to bf16 once) and writes dy_bf16 [B,T,Cin,Fin] -- the operand of the weight
 * gradient -- on the way: the separate pass over (dout, in_y), 132 MB and 40-95 us per level in the step, is gone.  Any other shape / dtype runs
 * the two calls.  bn_y / mean / ... / sums: the OUTPUT-side statistics of cruse_conv_*_bnbwd (bn_y == NULL and sums == NULL: none). */
int cruse_conv_gather_bnbwd_in(const void* dout, int dout_dtype, const float* in_y, const float* in_mean, const float* in_rstd,
                               const float* in_gamma, const float* in_beta, const double* in_sums, int in_replicas, int in_relu,
                               int in_training, void* dy_bf16, float* in_dgamma, float* in_dbeta, float* in_dbias,
                               const float* w, void* y, int B, int T, int Cin, int Fin, int Cout, int Fout, int KT, int S, int pad,
                               int w_layout, int accum, int prec,
                               const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                               double* sums, int zeroed, int y_dtype, void* stream);
int cruse_conv_scatter2_bnbwd_in(const void* dout, int dout_dtype, const float* in_y, const float* in_mean, const float* in_rstd,
                                 const float* in_gamma, const float* in_beta, const double* in_sums, int in_replicas, int in_relu,
                                 int in_training, void* dy_bf16, float* in_dgamma, float* in_dbeta, float* in_dbias,
                                 const float* w, void* y, int B, int T, int Cs, int Fg, int Cout, int Fout, int KT, int pad, int accum,
                                 int prec,
                                 const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                                 double* sums, int zeroed, int y_dtype, void* stream);

/* profiling aid: with cruse_set_option("cm_dbg", 1) workgroup 0 of an MFMA convolution launch stamps s_memtime at its phase
 * boundaries; this copies the sums of the LAST such launch to out8 (host memory, 8 values: prologue, tile staging incl. the wait
 * for the prefetch, k-loops, epilogues, tiles, N-tiles of wave 0, total; cycles) -- tools/conv_probe.py */
int cruse_conv_mfma_stamps(unsigned long long* out8);

/* (ABI 14) Host-only, touches no device: what a frame-major convolution call of this shape, mode and forms launches -- the decision the ten
 * entry points above make, without the launch.  scatter: 0 cruse_conv_gather*, 1 cruse_conv_scatter2* (then Cin = Cs, Fin = Fg, S = 2,
 * w_layout = 0); forms: which of the fused forms the call carries -- SUMS (_bnstats, out_sums of _bnin), BNB (_bnbwd; implies SUMS), BNI (_bnin),
 * BBI (_bnbwd_in; x_dtype is then dout_dtype).  Tensors are taken as 16-byte aligned.  out[7]:
 *   [0] route: 0 VALU kernel, 1 MFMA kernel          [1] BBI: 1 the fused kernel takes the call, 0 the two-call fallback (out = its conv)
 *   [2] mt (16-row tiles of Cout: 1, 2, 4)  [3] nw (waves per workgroup)      -- MFMA route, else 0
 *   [4] grid (workgroups)                   [5] dynamic LDS bytes             -- of the route taken
 *   [6] CO_T, the outputs per thread the VALU kernel is instantiated for (4 / 1 gather, 2 / 1 scatter2)   -- VALU route, else 0
 * Returns what the entry point would: an error code and cruse_last_error() where the call is refused. */
enum { CRUSE_CONV_FORM_SUMS = 1, CRUSE_CONV_FORM_BNB = 2, CRUSE_CONV_FORM_BNI = 4, CRUSE_CONV_FORM_BBI = 8 };
int cruse_conv_plan(int scatter, int Cin, int Fin, int Cout, int Fout, int KT, int S, int pad, int w_layout,
                    int B, int T, int prec, int x_dtype, int y_dtype, int act, int accum, int forms, int* out);

/* weight gradient of either form:
 *   dw[ca][cb][kt][kf] += sum_{b,t,fa} a[b,t,ca,fa] * bt[b, t-(KT-1)+kt, cb, fa*S - pad + kf]
 * ws: scratch of cruse_conv_wgrad_ws_bytes() bytes; a / bt hold a_dtype / bt_dtype elements (CRUSE_DT_F32 or CRUSE_DT_BF16).  One of three
 * kernels takes the call; they are asked in this order and cruse_conv_wgrad_plan tells which one answers (DESIGN.md section 4 has the table):
 *   register-direct MFMA (wgrad_rd.hip; fragments loaded straight from the two tensors): prec == CRUSE_PREC_BF16, Ca <= 64,
 *     KT * ceil(Cb / 16) <= 4, rows of >= 8 (even) positions, Fb == S * Fa, not (S 1, pad 0), both tensors 4-byte aligned
 *   LDS-staged MFMA (wgrad_mfma.hip; the patch matrix is materialised in LDS): prec >= 0, Ca <= 64, KT * 3 * Cb <= 192, Fa even, both
 *     tensors 16-byte aligned with rows of whole float4s, a frame tile that fits the LDS; bf16 operands only with CRUSE_PREC_BF16
 *   f32 VALU (conv.hip): everything else -- f32 operands, Ca a multiple of 4, Cb a multiple of 4 or 1; refused otherwise. */
size_t cruse_conv_wgrad_ws_bytes(int Ca, int Cb, int KT);
int cruse_conv_wgrad(const float* a, const float* bt, float* dw,
                     int B, int T, int Ca, int Fa, int Cb, int Fb,
                     int KT, int S, int pad, int prec, int a_dtype, int bt_dtype, void* ws, void* stream);

/* Host-only, touches no device: what a cruse_conv_wgrad call of this shape, mode and operand dtypes launches -- the decision the entry
 * point makes, without the launches.  a_misalign / bt_misalign: the addresses of a / bt modulo 16 (alignment selects between the kernels);
 * ws_bytes: the size of ws, 0 = cruse_conv_wgrad_ws_bytes(Ca, Cb, KT), which is what the entry point assumes.  Honours the options
 * "wg_rd" and "wg_grid".  out[14]:
 *   [0] kernel: 0 VALU, 1 LDS-staged MFMA, 2 register-direct MFMA
 *   [1..4] its template integers: VALU CB_T, KT | LDS-staged TFW (frames per tile), MT, NTW | register-direct MTW, NWP, U and
 *          1 where the instance that converts f32 operands is used; unused ones are 0
 *   [5] grid (workgroups)   [6] block (threads)   [7] dynamic LDS bytes   [8] partial slabs written to ws
 *   [9] TG, the workgroups that share a slab, and [10] frames per slab    -- register-direct kernel, else 0
 *   [11] the reduce kernel that follows: 1 wgrad_reduce_kernel, 2 wgrad_rd_reduce_kernel   [12] its grid x   [13] its grid y (chunks of 16 slabs)
 * Returns what the entry point would: an error code and cruse_last_error() where the call is refused. */
int cruse_conv_wgrad_plan(int B, int T, int Ca, int Fa, int Cb, int Fb, int KT, int S, int pad, int prec, int a_dtype, int bt_dtype,
                          int a_misalign, int bt_misalign, size_t ws_bytes, int* out);

/* out[c] += sum_{rows,f} g[row,c,f]   (bias gradients; F=1 gives a column sum) */
int cruse_channel_sum(const float* g, long long rows, int C, int F, float* out, void* stream);
/* out[j] += sum_rows g[row*ld + j], j < ncol  (GRU bias gradients: a column slice of dgi / dgh) */
int cruse_col_sum(const float* g, long long rows, int ncol, int ld, float* out, void* stream);

/* ---- BatchNorm2d (+ReLU, + skip add) (cruse_net.py:141-142,149-152,161-163) ---- */

/* sums[0..C) = sum y, sums[C..2C) = sum y^2 over rows x F (f64).  zeroed != 0: the caller hands over accumulators that are
 * already zero (the step's scratch arena, cleared by ONE cruse_zero per step) -- otherwise the callee clears them first. */
int cruse_bn_stats(const float* y, long long rows, int C, int F, double* sums, int zeroed, void* stream);
/* training: mean/rstd from sums (biased var), running stats updated with momentum and
 * unbiased var when running_mean != NULL (torch BatchNorm2d semantics). */
int cruse_bn_finalize(const double* sums, long long count, int C, float eps, float momentum,
                      float* mean, float* rstd, float* running_mean, float* running_var, void* stream);
/* eval: mean = running_mean, rstd = 1/sqrt(running_var+eps) */
int cruse_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps,
                        float* mean, float* rstd, void* stream);
/* out = [relu]((y-mean)*rstd*gamma+beta) [+ skip] */
int cruse_bn_act_fwd(const float* y, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* skip, float* out,
                     long long rows, int C, int F, int relu, void* stream);
/* out_bf16 (nullable): also a bf16 copy of out, [rows, C*F] -- the operand of the gate GEMM that reads the encoder's last
 * level, saving a cast pass.
 * cruse_bn_finalize + cruse_bn_act_fwd as one launch (training): mean / rstd come from the batch sums inside the kernel,
 * are also written out (the backward pass needs them) and the running statistics are updated.  sums is
 * [sum_replicas][2*C] and the statistic the sum over the replicas: 1 after cruse_bn_stats, CRUSE_BN_STAT_REPLICAS after
 * cruse_conv_*_bnstats. */
int cruse_bn_finalize_act_fwd(const float* y, const double* sums, int sum_replicas, long long count, float eps, float momentum,
                              const float* gamma, const float* beta, const float* skip, float* out, void* out_bf16,
                              float* mean, float* rstd, float* running_mean, float* running_var,
                              long long rows, int C, int F, int relu, void* stream);
/* sums[0..C) = sum g, sums[C..2C) = sum g*xhat with g = dout * [bn(y) > 0]; `zeroed` as for cruse_bn_stats */
/* (ABI 9) the same with the element type of the 2-byte operand copy chosen: copy_dtype = CRUSE_DT_BF16 (the function above) or
 * CRUSE_DT_F16 -- the operand of the single-pass f16 gate projection cruse_gemm_f16_nt. */
int cruse_bn_finalize_act_fwd_c(const float* y, const double* sums, int sum_replicas, long long count, float eps, float momentum,
                                const float* gamma, const float* beta, const float* skip, float* out, void* out_copy, int copy_dtype,
                                float* mean, float* rstd, float* running_mean, float* running_var,
                                long long rows, int C, int F, int relu, void* stream);
int cruse_bn_act_bwd_reduce(const float* dout, const float* y, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, long long rows, int C, int F,
                            int relu, double* sums, int zeroed, void* stream);
/* dy = gamma*rstd*(g - [training](sum_g + xhat*sum_gx)/count); dgamma += sum_gx; dbeta += sum_g;
 * dbias (nullable) += per-channel sum of dy -- the gradient of the bias of the conv that feeds this BN -- in closed
 * form from the sums: gamma*rstd*sum_g with running statistics, and exactly 0 with batch statistics (sum xhat = 0:
 * the bias is cancelled by the mean subtraction; autograd leaves rounding noise there)
 * sums is [sum_replicas][2*C] (1 after cruse_bn_act_bwd_reduce, CRUSE_BN_STAT_REPLICAS after cruse_conv_*_bnbwd). */
int cruse_bn_act_bwd_apply(const float* dout, const float* y, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, const double* sums, int sum_replicas,
                           long long rows, int C, int F, int relu, int training, int dout_dtype,
                           void* dy, int dy_dtype, float* dgamma, float* dbeta, float* dbias, void* stream);

/* ---- LayerNorm (+ group interleave, + residual) (cruse_net.py:32-33,43-51,160) -- */

/* y[row, P(c)] = (x[row,c]-mean)*rstd*gamma[P(c)] + beta[P(c)] (+ res[row,P(c)])
 * P(i*Hg + j) = j*g + i with Hg = H/g is the stack(dim=-1)+flatten of cruse_net.py:43-45
 * (interleave_g = g; 1 = identity / the plain cat of :49-50). eps = 1e-5.
 * y_bf16 (nullable): also a bf16 copy of y [rows, H] (the next gate GEMM's operand).
 * seg_len > 0 (interleave_g == 1): ROW SEGMENTS -- logical row r of every row-indexed array is physical row
 * (r / seg_len) * seg_stride + seg_off + r % seg_len: frames [seg_off, seg_off + seg_len) of every clip of [B, T = seg_stride]
 * tensors, i.e. one TIME CHUNK of the batch (run beside the recurrence of the next chunk); rows = B * seg_len.
 * Alignment: 16-byte aligned x, y, gamma, beta, res (with interleave_g == 1, H % 4 == 0) take the vector kernel, anything else the
 * 4-byte one; a y_bf16 that is 8-byte aligned is written by the vector kernel itself, any other by one more pass.  Row segments need
 * the vector kernel (CRUSE_E_SHAPE) and an 8-byte aligned y_bf16 (CRUSE_E_ALIGN); a refused call has written nothing. */
int cruse_ln_fwd(const float* x, const float* gamma, const float* beta, const float* res,
                 float* y, void* y_bf16, float* mean, float* rstd, long long rows, int H, int interleave_g,
                 float eps, int seg_len, long long seg_stride, long long seg_off, void* stream);
/* (ABI 9) cruse_ln_fwd with the element type of the operand copy chosen (CRUSE_DT_BF16 or CRUSE_DT_F16; f16 needs interleave_g == 1) */
int cruse_ln_fwd_c(const float* x, const float* gamma, const float* beta, const float* res,
                   float* y, void* y_copy, int copy_dtype, float* mean, float* rstd, long long rows, int H, int interleave_g,
                   float eps, int seg_len, long long seg_stride, long long seg_off, void* stream);
int cruse_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                 const float* gamma, long long rows, int H, int interleave_g,
                 float* dx, float* dgamma, float* dbeta, void* stream);

/* ---- MFMA GEMM (GRU gate projections nn.GRU at cruse_net.py:23-31; their dX / dW) -- */

/* C[M,N] (=|+=) op(A) * op(B) (+ bias[n]);  op(A) is [M,K]: transA==0 -> A[m*lda+k], else A[k*lda+m];
 * op(B) is [K,N]: transB==0 -> B[k*ldb+n], else B[n*ldb+k].
 * accumulate != 0: C += ...; splitk > 1 splits K over blockIdx.z and adds atomically (implies +=).
 * b_shift_T > 0 (transB==0 only): row k of B is read from row k-1 and is zero when k % b_shift_T == 0
 * (the h_{t-1} operand of dW_hh). prec: CRUSE_PREC_*. */
int cruse_gemm(int transA, int transB, int M, int N, int K,
               const float* A, int lda, const float* B, int ldb, float* C, int ldc,
               const float* bias, int accumulate, int splitk, int b_shift_T, int prec, void* stream);

/* bf16-operand form of the same products for CRUSE_PREC_BF16: C[M,N] (=|+=) A[M,K] . B[N,K]^T (+ bias[n]), C f32,
 * K % 64 == 0.  Operand element (m, k) is A[(k/64)*a_kstride + m*lda + k%64]: a_kstride == 64 is plain row-major
 * (lda >= K); the K-TILED time-major layout of cruse_transpose_bf16 / cruse_gru_gate_grads_bf16 has lda == 64 and
 * a_kstride == 64 * (number of lines).  Same for B.  splitk > 1 adds atomically and needs accumulate != 0;
 * splitk < -1 is |splitk| k-slices with slice z computed entirely on XCD z % 8 (all output tiles of a slice share that
 * XCD's L2: the long-K weight gradients then read every operand byte from HBM about once).
 * Operand values are the RNE roundings cruse_gemm forms internally. */
int cruse_gemm_bf16_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride,
                       const void* B, long long ldb, long long b_kstride,
                       float* C, long long ldc, const float* bias, int accumulate, int splitk, void* stream);
/* The split-K weight-gradient form without atomics: C[M,N] += A . B^T with |splitk| k-slices (splitk < -1: pinned to XCDs as
 * above), every slice STORING its partial sums to its own [M][N] slab of `scratch` (cruse_gemm_bf16_slab_bytes(M, N, splitk)
 * bytes, 16-byte aligned) and one kernel adding the slabs to C in slice order.  The f32 atomics of the splitk form from the 8 XCDs
 * meet at the memory side (9.8 M per gate weight gradient: 0.14 ms of the training step), and their order made dW differ from run
 * to run in the last bits; this form is reproducible.  N % 4 == 0. */
size_t cruse_gemm_bf16_slab_bytes(int M, int N, int splitk);
int cruse_gemm_bf16_nt_slabs(int M, int N, int K, const void* A, long long lda, long long a_kstride,
                             const void* B, long long ldb, long long b_kstride,
                             float* C, long long ldc, int splitk, void* scratch, size_t scratch_bytes, void* stream);
/* (ABI 9) Up to three products that share N, K, the operand strides and the A tensor, concatenated along M into ONE launch and ONE output:
 *   C[sum M_i, N] += cat_i( A[a_rows[i] .. a_rows[i] + M_i) . B_i^T )      slab form as above (a product whose M_i is not a multiple of 128 still starts on a
 *   row tile of its own; the output rows stay contiguous).
 * The three weight-gradient products of an nn.GRU layer (cruse_net.py:23-31: dW_ih += (r, z, n_i)^T x, dW_hh += (r, z)^T h_{t-1} and
 * n_h^T h_{t-1}) are such a set: their A rows are slabs of the one time-major gate-gradient tensor, and dW_ih / dW_hh lie back to back in
 * the flat gradient buffer.  Ms, a_rows, Bs: HOST arrays of nprob (1..3) entries. */
int cruse_gemm_bf16_nt_slabs_cat(int nprob, const int* Ms, int N, int K, const void* A, const long long* a_rows, long long lda,
                                 long long a_kstride, const void* const* Bs, long long ldb, long long b_kstride,
                                 float* C, long long ldc, int splitk, void* scratch, size_t scratch_bytes, void* stream);
/* (ABI 9) G products of the same shape in ONE launch, side by side along N -- the GRU groups of one layer (GGRU with rnn_groups > 1,
 * cruse_net.py:14-55):  C[:, q * c_gstep + (0..N)] (+)= A[:, q * a_gstep + (0..K)] . B_q^T + bias_q,  B_q = B + q * b_gstep, bias_q = bias + q * bias_gstep.
 * A row-major (planes A_hi / A_lo nullable as in cruse_gemm_bf16x3_nt), B as in cruse_gemm_bf16_nt (B_lo nullable, same group stride).  Used for
 * the forward gate projections and the input gradients of the grouped configurations: G launches of 2-4 column tiles each become one. */
int cruse_gemm_bf16_nt_groups(int M, int N, int K, int G, const void* A_hi, const void* A_lo, long long lda, long long a_gstep,
                              const void* B_hi, const void* B_lo, long long ldb, long long b_kstride, long long b_gstep,
                              float* C, long long ldc, long long c_gstep, const float* bias, long long bias_gstep, int accumulate,
                              void* stream);
/* cruse_gemm_bf16_nt / cruse_gemm_bf16x3_nt (A_lo, B_lo nullable: plain bf16) on a TIME CHUNK of the batch: logical row m of A
 * (row-major, lda) and of C is physical row (m / seg_len) * seg_stride + seg_off + m % seg_len; M = B * seg_len.  The gate
 * projection gi = x W_ih^T of frames [seg_off, seg_off + seg_len) of every clip then runs beside the recurrence of the
 * frames before them (model/cruse_net.py:44,50 chunked in time; results identical to the unchunked call). */
int cruse_gemm_bf16_nt_seg(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda,
                           const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                           float* C, long long ldc, const float* bias, int accumulate,
                           int seg_len, long long seg_stride, long long seg_off, void* stream);
/* y[i] = bf16(x[i]), n % 4 == 0 */
int cruse_cast_bf16(const float* x, void* y, long long n, void* stream);
/* K-tiling without transposition: y[(k/64)*rows*64 + n*64 + k%64] = bf16(x[n*ld + k]), zero for cols <= k < ceil64(cols):
 * a K-contiguous operand (W_ih [3Hg, Hg]) whose K is not a multiple of 64.  y_lo (nullable): the low plane
 * bf16(x - y) of the split-bf16 x3 form, same layout. */
int cruse_ktile_bf16(const float* x, int rows, int cols, long long ld, void* y, void* y_lo, void* stream);
/* (ABI 9) the same K-tiled layout with IEEE-f16 elements: the B operand of cruse_gemm_f16_nt */
int cruse_ktile_f16(const float* x, int rows, int cols, long long ld, void* y, void* stream);
/* (ABI 12) ... with the low plane y_lo = f16(x - f16(x)), same layout: the B_lo operand of cruse_gemm_f16x2_nt */
int cruse_ktile_f16_split(const float* x, int rows, int cols, long long ld, void* y, void* y_lo, void* stream);
/* (ABI 13; first in ABI 9-10) C[M,N] (+)= A[M,K] . B[N,K]^T with A read from its TIME-MAJOR K-tiled image -- element (m, k) at
 * A_T[(m / 64) * a_mb_stride + k * 64 + m % 64], n_mb 64-row blocks present -- the layout of the gate-gradient tensor dgT the weight-gradient GEMMs
 * consume: the input gradient dX = dgi . W_ih of nn.GRU's backward (model/cruse_net.py:23-31,44,50) straight from it, so that the row-major copy dgi
 * (98 MB per layer at the bench shape) is never written.  B as cruse_gemm_bf16_nt; plain bf16, one pass, K % 64 == 0.  Bit-identical to the row-major form. */
int cruse_gemm_bf16_nt_atr(int M, int N, int K, const void* A_T, long long a_mb_stride, int n_mb,
                           const void* B, long long ldb, long long b_kstride,
                           float* C, long long ldc, int accumulate, void* stream);
/* (ABI 13) The forward gate projections with a 2-BYTE RESULT: C[M,N] = (A_hi + A_lo) . (B_hi + B_lo)^T + bias stored as IEEE f16 (out_dtype =
 * CRUSE_DT_F16) or bf16 (CRUSE_DT_BF16) rows [M, ldc] -- gi is the largest tensor of the forward pass (197 MB in f32 at the bench shape), written once
 * here and read once by cruse_gru_seq_fwd_gi16.  operands_f16 = 0: bf16 operand planes in the layouts of cruse_gemm_bf16_nt / cruse_gemm_bf16x3_nt
 * (A_lo, B_lo nullable; A_lo needs B_lo); 1: IEEE-f16 planes (cruse_gemm_f16_nt / cruse_gemm_f16x2_nt; no A_lo).  f32 accumulation, ONE rounding at
 * the store.  Replaces the output side of nn.GRU's input projection (model/cruse_net.py:23-31,44,50). */
int cruse_gemm_nt_out16(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda, long long a_kstride,
                        const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                        void* C, long long ldc, const float* bias, int operands_f16, int out_dtype, void* stream);
/* (ABI 9) C[M,N] = A[M,K] . B[N,K]^T + bias[n] with IEEE-f16 operands in the layouts of cruse_gemm_bf16_nt, f32 accumulation
 * (v_mfma_f32_16x16x32_f16): the FORWARD gate projection gi = x W_ih^T (cruse_net.py:23-31,44,50) in ONE pass -- 11 significant bits
 * on both operands, where the split-bf16 form above spends a second pass to correct W_ih only and keeps x at 8 bits.  The operands
 * are O(1) activations (BatchNorm + ReLU / LayerNorm outputs) and |W_ih| <= 1 / sqrt(Hg): inside f16's range. */
int cruse_gemm_f16_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride,
                      const void* B, long long ldb, long long b_kstride,
                      float* C, long long ldc, const float* bias, void* stream);
/* (ABI 12) C = A . (B_hi + B_lo)^T + bias[n]: f16 activations against TWO f16 planes of the weights in one launch (the k-range is walked twice on the
 * same accumulators) -- the forward gate projection of GGRU layer 1 (nn.GRU input projection, cruse_net.py:23-31): 11 bits on x, ~20 on W_ih. */
int cruse_gemm_f16x2_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride,
                        const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                        float* C, long long ldc, const float* bias, void* stream);
/* y = bf16(x) and y_lo = bf16(x - y) (nullable) */
int cruse_cast_bf16_split(const float* x, void* y, void* y_lo, long long n, void* stream);
/* Split-bf16 x3 form of cruse_gemm_bf16_nt: A = A_hi + A_lo, B = B_hi + B_lo (bf16 planes, same layout each);
 * C = A_hi.B_hi + A_hi.B_lo [+ A_lo.B_hi] accumulated in one pass.  A_lo may be NULL: two passes, only B's rounding
 * is corrected.  Used for the FORWARD gate projection gi = x W_ih^T: the bf16 rounding of W_ih dominates the
 * forward error of CRUSE_PREC_BF16 (enhanced spectrum 1.25e-3; 5.1e-4 with W split, 4.8e-4 with both).  No split-K. */
int cruse_gemm_bf16x3_nt(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda, long long a_kstride,
                         const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                         float* C, long long ldc, const float* bias, int accumulate, void* stream);
/* (ABI 15) Host-only, touches no device: what a call of the ten bf16 / f16 GEMM entry points above launches -- the decision they make, without
 * the launch.  form: whose checks run first (PLAIN cruse_gemm_bf16_nt, X3 cruse_gemm_bf16x3_nt, F16 / F16X2 cruse_gemm_f16_nt / _f16x2_nt, OUT16
 * cruse_gemm_nt_out16, ATR / GROUPS / SLABS / SLABS_CAT / SEG cruse_gemm_bf16_nt_<form>).  planes: bit 0 A_lo present, bit 1 B_lo present, bit 2 the
 * low planes lie 2 bytes off their 16-byte alignment; has_bias: a bias is given; every other tensor counts as present and 16-byte aligned.
 * accumulate, splitk, operands_f16, out_dtype as the entry points take them.  A scalar the form's entry point has no argument for reaches the
 * shared checks as given, except what defines the form (ATR: lda, a_kstride; GROUPS, SEG: a_kstride = 64; the slab forms accumulate; out_dtype
 * counts for OUT16 alone; F16 / F16X2 are operands_f16).  extras (HOST, NULL for the forms before ATR), the form's own numbers:
 *   ATR {a_mb_stride, n_mb}   GROUPS {G, a_gstep, b_gstep, c_gstep, bias_gstep}   SLABS {scratch_bytes}   SEG {seg_len, seg_stride, seg_off}
 *   SLABS_CAT {scratch_bytes, nprob, Ms[3], a_rows[3]} (8 numbers whatever nprob; M is ignored)
 * out[16]:
 *   [0] MODE of the kernel (0 store, 1 add, 2 atomic split-K, 3 2-byte rows, 4 slabs)   [1] LDS stages (2, 3)   [2] f16 operands   [3] time-major A
 *   [4] grid (workgroups)   [5] dynamic LDS bytes   [6] k-slices after clamping   [7] k-tiles per slice   [8] 1: the slices are pinned to XCDs
 *   [9] row tiles   [10] column tiles (all groups)   [11] units   [12] tiles per unit        -- the kernel's XCD-aware tile order
 *   [13] output rows   [14] floats between two slabs, [15] workgroups of the slab sum        -- 0 without slabs
 * Returns what the entry point would: an error code and cruse_last_error() where the call is refused. */
enum { CRUSE_GEMM_FORM_PLAIN, CRUSE_GEMM_FORM_X3, CRUSE_GEMM_FORM_F16, CRUSE_GEMM_FORM_F16X2, CRUSE_GEMM_FORM_OUT16, CRUSE_GEMM_FORM_ATR,
       CRUSE_GEMM_FORM_GROUPS, CRUSE_GEMM_FORM_SLABS, CRUSE_GEMM_FORM_SLABS_CAT, CRUSE_GEMM_FORM_SEG, CRUSE_GEMM_FORM_N };
int cruse_gemm_bf16_plan(int form, int M, int N, int K, long long lda, long long a_kstride, long long ldb, long long b_kstride, long long ldc,
                         int planes, int has_bias, int accumulate, int splitk, int operands_f16, int out_dtype,
                         const long long* extras, int* out);
/* K-tiled time-major transpose: yT[(r/64)*cols*64 + c*64 + r%64] = bf16(x[(r - s)*ld + c]) with s = 0, or s = 1
 * when shift_T > 0 (then 0 where r % shift_T == 0: the h_{t-1} operand of dW_hh); frames rows <= r < ldT are
 * zero-filled (ldT % 64 == 0). */
int cruse_transpose_bf16(const float* x, long long rows, int cols, long long ld, void* yT, long long ldT,
                         int shift_T, void* stream);

/* ---- grouped-GRU recurrence (nn.GRU forward/backward at cruse_net.py:44,50) ----- */

/* Persistent recurrence.  gi [B,T,G,3*Hg] = x W_ih^T + b_ih (gate order r,z,n) from cruse_gemm;
 * w_hh[g] -> [3*Hg,Hg], b_hh[g] -> [3*Hg] (HOST arrays of G device pointers); h0 = 0.
 * Output h [B,T,G*Hg] in "cat" layout (feature = g*Hg + j).  For backward (all three or none):
 *   coef [B,T,G,3*Hg] = d(W_hh h + b_hh)-gradient coefficients (c_r, c_z, c_n): dgh_t = dh_t * coef_t
 *                       (bf16 elements when prec == CRUSE_PREC_BF16, f32 otherwise),
 *   an   [B,T,G*Hg]   = dgi_n coefficient ((1-z)(1-n^2)),   z [B,T,G*Hg] = update gate.
 * Hg % 32 == 0, Hg <= 1024 (the BACKWARD recurrence keeps a [16][3*Hg] operand image in LDS: Hg <= 800 in the f32 and split-bf16
 * modes, 1024 in CRUSE_PREC_BF16; larger is refused with CRUSE_E_SHAPE).  ws: cruse_gru_ws_bytes() bytes of device scratch.  Its first 256 bytes are a STICKY
 * header the CALLER zeroes once when it allocates the buffer: word 0 becomes non-zero if a hand-off ever timed out
 * (the launch then completes unsynchronised and its outputs are garbage) and is never cleared by the library, so it
 * can be polled once per epoch and handed to cruse_adam_step_guarded as skip_flag.  The hand-off panels behind the
 * header are zeroed by the callee on every call. */
size_t cruse_gru_ws_bytes(int B, int G, int Hg);
/* The launch plan cruse_gru_seq_fwd (fwd != 0) / cruse_gru_seq_bwd take for this shape and precision with h0 = 0 and no explicit chain width:
 * out[0] clips per chain (8, or 16: the wide-chain kernels of gru_w16.hip), out[1] chains per group, out[2] chains per group and launch,
 * out[3] launches, out[4] workgroups per chain (Hg / 32), out[5] 1 = wide-chain kernels.  A query: no device work.  Replaces nothing in the
 * reference (nn.GRU has no launch plan, model/cruse_net.py:23-31); it lets tests and bench.py state which kernels a batch size runs on. */
int cruse_gru_plan(int B, int G, int Hg, int prec, int fwd, int* out);
int cruse_gru_seq_fwd(const float* gi, const float* const* w_hh, const float* const* b_hh,
                      float* h, void* coef, float* an, float* z,
                      int B, int T, int G, int Hg, int prec, void* ws, void* stream);
/* dout = dL/dh [B,T,G*Hg] -> dh [B,T,G*Hg] = total gradient reaching h_t (incl. the recurrent path):
 * dh_s = dout_s + z_{s+1}*dh_{s+1} + (dh_{s+1}*coef_{s+1}) W_hh. */
int cruse_gru_seq_bwd(const float* dout, const float* const* w_hh, const void* coef, const float* z,
                      float* dh, int B, int T, int G, int Hg, int prec, void* ws, void* stream);
/* The same two launches for CONCURRENT recurrences (half batches on two streams, so that the projections / layer norms
 * of one half run beside the recurrence of the other): the workspace is given as a per-launch panel scratch of
 * cruse_gru_ws_bytes(B,G,Hg) - 256 bytes (zeroed here) plus a caller-owned sticky status word that several launches may
 * share, and chain c of the launch runs on XCD (c + xcd_rot) % 8 instead of c % 8.  A recurrence workgroup owns its CU;
 * two launches of <= 4 chains with xcd_rot 0 and 4 occupy disjoint XCDs and are co-resident, with the same xcd_rot they
 * would queue for the same CUs.  cruse_gru_seq_fwd/bwd(ws) == _on(ws + 256, (unsigned*)ws, 0).
 * _bwd_on: dgi != NULL (CRUSE_PREC_BF16, with the a_n rows `an`): also writes the bf16 gate gradients
 * dgi [B,T,G,3*Hg] = dh * (c_r, c_z, a_n) -- the dgi output of cruse_gru_gate_grads_bf16 -- from inside the recurrence, so
 * that dX = dgi W_ih can start right behind it; cruse_gru_gate_grads_bf16(dgi = NULL) then only makes dgT / the bias sums. */
int cruse_gru_seq_fwd_on(const float* gi, const float* const* w_hh, const float* const* b_hh,
                         float* h, void* coef, float* an, float* z,
                         int B, int T, int G, int Hg, int prec, void* panels, unsigned* status, int xcd_rot, void* stream);
int cruse_gru_seq_bwd_on(const float* dout, const float* const* w_hh, const void* coef, const float* z,
                         float* dh, const float* an, void* dgi, int B, int T, int G, int Hg, int prec,
                         void* panels, unsigned* status, int xcd_rot, void* stream);
/* SUB-SEQUENCES and INITIAL STATE (cust_conv.py:305-325 passes h0 explicitly; GroupGRU.forward(input, state) :392-416).
 * T steps of tensors whose clips are TS >= T frames apart; every pointer is already advanced to the first frame of the run.
 *   _fwd_ex: h0 [B][G*Hg] ("cat" feature layout, clips h0_bstride floats apart, 16-byte aligned) or NULL (= 0).  A long
 *            sequence can be run as consecutive time chunks: chunk [t0, t0+n) is (gi + t0*G*3*Hg, h + t0*G*Hg, ..., h0 =
 *            h + (t0-1)*G*Hg with h0_bstride = TS*G*Hg, T = n) -- the results are those of the single launch.  Bit for bit: in the f32 and
 *            split-bf16 modes, and wherever the launch it is compared with was given an h0 as well (the same kernel then serves every chunk).
 *            Not in CRUSE_PREC_BF16 at Hg = 160 / 320 on chains of 8 against a launch from h0 == NULL: that launch runs gru_fwd_tf_kernel (its
 *            hand-off needs |h| < 1; every wave walks the whole K), a continuation gru_fwd_lean_kernel (K split over four waves) -- the f32 sums
 *            are formed in another order; the results agree to the bf16 operands' precision.  (Observed once, unexplained: at Hg = 160 a
 *            difference of bits remained with "gru_tf" = 0, the lean kernel on both sides -- no promise is made for that case either.)
 *   _bwd_ex: carry != 0: the first iteration takes dh of the run's LAST frame from the dh buffer (written by the run that
 *            follows it in time) instead of forming it from dout: chunk [t0, t0+n) of a longer sequence is run as the
 *            n + 1 frames [t0, t0+n] with carry = 1 (the last chunk: n frames, carry = 0).  dgi on a sub-sequence is
 *            supported by the reduce-scatter kernels only (CRUSE_PREC_BF16, Hg <= 640).
 *            dg_slabs: 3 = dgi rows [G][3][Hg] (r, z, n_i); 4 = [G][4][Hg] with slab 3 = dh * c_n, the n gate of
 *            dgh = dh * (c_r, c_z, c_n) (reduce-scatter kernel): one row-major tensor that is the A operand of
 *            dX = dgi W_ih (K = 3*Hg of every 4*Hg) (the row-major TN weight-gradient products that also read it are gone: measured slower, r3).
 *   panels_zeroed: the caller has cleared the panel scratch (cruse_gru_ws_bytes() - 256 bytes at `panels`) since its last use, on
 *            this stream or ordered before it; 0: the call clears it itself (one memset launch in front of the recurrence).  A
 *            training step clears the scratches of its four recurrences with one launch at its top.
 *   chain_clips: clips served by one team of Hg/32 workgroups.  0 = the library's plan: chains of 8 while the batch's chains fit
 *            the CUs; beyond that (B > 96 at Hg = 640) WIDE chains of 16 (half the workgroups per clip, the full 16 columns of the
 *            MFMA; CRUSE_PREC_BF16, Hg % 128 == 0, Hg <= 640, h0 == NULL) where that needs fewer launches.
 *            8 / 16 force the width: with 16 a batch of 64 at Hg = 640 takes 80 CUs, so the recurrences of BOTH GGRU layers are
 *            co-resident (measured slower than one after the other on chains of 8: DESIGN.md section 8).  The forward
 *            results do not depend on the width (same sums in the same order); the backward ones up to the f32 summation order.
 *            chain_clips = 16 WITH h0: the caller vouches for |h0| < 1 (the wide kernels' hand-off keeps the epoch bit in the top
 *            exponent bit of every exchanged bf16) -- true for the continuation of a sequence that started from h0 = 0. */
int cruse_gru_seq_fwd_ex(const float* gi, const float* const* w_hh, const float* const* b_hh,
                         float* h, void* coef, float* an, float* z, const float* h0, long long h0_bstride,
                         int B, int T, int TS, int G, int Hg, int prec, int chain_clips, void* panels,
                         int panels_zeroed, unsigned* status, int xcd_rot, void* stream);
int cruse_gru_seq_bwd_ex(const float* dout, const float* const* w_hh, const void* coef, const float* z,
                         float* dh, const float* an, void* dgi, int dg_slabs, int carry, int B, int T, int TS, int G,
                         int Hg, int prec, int chain_clips, void* panels, int panels_zeroed, unsigned* status, int xcd_rot,
                         void* stream);
/* (ABI 13) gi rows stored as IEEE f16 ([B,T,G,3*Hg] halves, written by cruse_gemm_nt_out16): half the bytes of the largest tensor of the forward
 * pass.  gi_dtype: CRUSE_DT_F16, or CRUSE_DT_F32 (then exactly cruse_gru_seq_fwd_ex with h0 = NULL, chain_clips = 0).  f16 rows are served where the
 * bench step runs -- CRUSE_PREC_BF16, Hg = 640, chains of 8 clips (cruse_gru_plan: B <= 96) -- and refused with CRUSE_E_SHAPE elsewhere.
 * Replaces the recurrence of nn.GRU (model/cruse_net.py:23-31, :41-51) like cruse_gru_seq_fwd_ex. */
int cruse_gru_seq_fwd_gi16(const void* gi, int gi_dtype, const float* const* w_hh, const float* const* b_hh,
                           float* h, void* coef, float* an, float* z,
                           int B, int T, int TS, int G, int Hg, int prec, void* panels,
                           int panels_zeroed, unsigned* status, int xcd_rot, void* stream);
/* dgi = dh*(c_r,c_z,a_n) (gradient wrt gi), dgh = dh*(c_r,c_z,c_n) (gradient wrt W_hh h + b_hh), both
 * [rows,G,3*Hg]; dW_ih, dW_hh, dX and the bias gradients follow from cruse_gemm / cruse_col_sum. */
int cruse_gru_gate_grads(const float* dh, const void* coef, const float* an, float* dgi, float* dgh,
                         long long rows, int G, int Hg, int prec, void* stream);
/* CRUSE_PREC_BF16 form feeding cruse_gemm_bf16_nt (coef bf16).  dgi and dgh share the r and z gates, so four
 * slabs (r, z, n_i, n_h) carry both: dgi [rows,G,3,Hg] bf16 = (r,z,n_i) row-major; dgT [ldT/64,G,4,Hg,64] bf16 =
 * the K-tiled time-major transpose (ldT = rows rounded up to 64, zero padded): dW_ih uses slabs 0-2, dW_hh 0,1,3.
 * db_ih / db_hh: HOST arrays of G device pointers (or NULL) to [3*Hg] bias gradients, ACCUMULATED from f32. */
/* dgi or dgT may be NULL (not both): only the other output (and the bias sums) is produced */
int cruse_gru_gate_grads_bf16(const float* dh, const void* coef, const float* an, void* dgi, void* dgT,
                              long long ldT, float* const* db_ih, float* const* db_hh,
                              long long rows, int G, int Hg, void* stream);

/* ---- mask application + weighted spectral loss ------------------------------- */

/* PreProcess.masking "mag_mapping" (utils/utils.py:418-420) fused with WO-MALE
 * (loss_func/loss.py:121-148, alpha/(beta+iam), gamma = 1) and its gradient.
 * mask [rows,Fn]; nre, nim [rows,Fs] noisy spectrum; cmag [rows,Fs] = |clean|; bins Fn..Fs-1 of the
 * estimate are zero.  loss_sum[0] = sum W*|log10(|est|+1) - log10(|ref|+1)| (f64, zeroed by callee;
 * the loss is loss_sum/(rows*Fs)).  Optional outputs: dmask [rows,Fn] = d(loss)/d(mask),
 * dlogit [rows,Fn] = dmask*mask*(1-mask), est_re/est_im [rows,Fs]. */
int cruse_mask_loss_fwd(const float* mask, const float* nre, const float* nim, const float* cmag,
                        long long rows, int Fn, int Fs, float alpha, float beta,
                        double* loss_sum, float* dmask, float* dlogit, float* est_re, float* est_im,
                        void* stream);

/* The mask head of the training step in one launch (csrc/mask_head.hip; additive entry point):
 *   cruse_bn_finalize_act_fwd(v, bn_sums, ..., skip)          -> u [B,T,C,F1], mean, rstd [C], running statistics (nullable pair)
 *   cruse_conv_scatter2(u, w [C][1][1][3], bias, KT 1, pad 0, sigmoid)  -> mask [B*T, 2*F1]
 *   cruse_mask_loss_fwd(mask, nre, nim, cmag [B*T, Fs], Fs = 2*F1 + 1)  -> loss_sum, dlogit [B*T, 2*F1]
 *   cruse_conv_gather_bnbwd(dlogit, w, Cin 1, S 2, pad 0; bn_y = v)     -> du [B,T,C,F1], bwd_sums [bwd_replicas][2*C] (sum g, sum g*xhat)
 * with the bits of those calls in every tensor; loss_sum and bwd_sums are f64 atomics (free order) and are ADDED to when
 * loss_zeroed / bwd_zeroed != 0, cleared first otherwise.  C <= 16, F1 % 4 == 0, C * F1 <= 640; v, skip, u, du 16-byte aligned.
 * max_blocks: 0, or a cap on the grid (a workgroup then walks several tiles of 8 frames). */
int cruse_mask_head_fwd_bwd(const float* v, const double* bn_sums, int sum_replicas, float eps, float momentum,
                            const float* gamma, const float* beta, const float* skip, const float* w, const float* bias,
                            const float* nre, const float* nim, const float* cmag,
                            int B, int T, int C, int F1, int Fs, float loss_alpha, float loss_beta,
                            float* u, float* mean, float* rstd, float* running_mean, float* running_var,
                            float* mask, float* dlogit, float* du, double* loss_sum, int loss_zeroed,
                            double* bwd_sums, int bwd_replicas, int bwd_zeroed, int max_blocks, void* stream);

/* ---- time-domain loss in the loop ---------------------------- */

/* PreProcess.masking "mag_mapping" alone (utils/utils.py:418-420): est = mask * noisy spectrum on the first Fn
 * bins, zero above.  mask [rows,Fn]; nre, nim, est_re, est_im [rows,Fs]. */
int cruse_mask_apply(const float* mask, const float* nre, const float* nim, long long rows, int Fn, int Fs,
                     float* est_re, float* est_im, void* stream);
/* its backward: dout[rows,Fn] = (dre*nre + dim*nim) [* mask*(1-mask) when through_sigmoid != 0] */
int cruse_mask_apply_bwd(const float* dre, const float* dim, const float* nre, const float* nim,
                         const float* mask, long long rows, int Fn, int Fs, int through_sigmoid,
                         float* dout, void* stream);
/* SNR-weighted speech-distortion loss `sdnr` (loss_func/loss.py:151-175, vad == 1) with the mask as gain:
 * loss = loss_sum[0] / (B*Fs) = alpha*L_speech + (1-alpha)*L_noise, alpha = 10^(snr/10)/(10^(snr/10)+10^(beta/10)).
 * cre/cim clean, nre/nim noisy spectra [rows,Fs] (noise = noisy - clean); optional dmask / dlogit [rows,Fn]. */
int cruse_mask_sdnr_fwd(const float* mask, const float* cre, const float* cim, const float* nre, const float* nim,
                        long long rows, int Fn, int Fs, int B, float snr_db, float beta_db,
                        double* loss_sum, float* dmask, float* dlogit, void* stream);
/* si_snr_loss of train_base/loss.py:7-25 on waveforms x (estimate), s (target) [B,L]:
 * loss[0] = -mean_b 20 log10(eps + |t|/(|x_zm - t| + eps)) (f64; zeroed by the callee).
 * mom [B,5] f64 scratch; coef [B,4] f32 receives the per-clip gradient scalars for cruse_sisnr_bwd. */
int cruse_sisnr_fwd(const float* x, const float* s, int B, int L, float eps,
                    double* mom, double* loss, float* coef, void* stream);
/* dx = grad_scale * d loss / d x */
int cruse_sisnr_bwd(const float* x, const float* s, const float* coef, int B, int L, float grad_scale,
                    float* dx, void* stream);
/* l1_loss / mse_loss = torch.nn.L1Loss / MSELoss (train_base/loss.py:3-4; selected by tools/train_stand.py:73-75) on waveforms:
 * loss_sum[0] = sum |est - ref| (mse = 0) or sum (est - ref)^2 (mse = 1) over n samples (f64; zeroed by the callee);
 * dest (optional, n floats) = grad_scale * sign(est - ref)  resp.  grad_scale * 2 (est - ref): pass 1/n for reduction "mean". */
int cruse_wave_l1_mse(const float* est, const float* ref, long long n, int mse, float grad_scale,
                      double* loss_sum, float* dest, void* stream);

/* ---- DeepFilter head (model/deep_filter.py:15-41, BASELINE config 4) --------------- */
/* out[b,f,t] = sum over the (2*f_dim+1) x (2*t_dim+1) neighbourhood of X*H (complex, zero outside); all
 * tensors [B,F,T] in the reference's layout.  Imaginary part = xr*hi + xi*hr (decision: SURVEY 8a a15). */
int cruse_deepfilter_fwd(const float* xr, const float* xi, const float* hr, const float* hi,
                         int B, int F, int T, int f_dim, int t_dim, float* out_r, float* out_i, void* stream);
int cruse_deepfilter_bwd(const float* dout_r, const float* dout_i, const float* xr, const float* xi,
                         const float* hr, const float* hi, int B, int F, int T, int f_dim, int t_dim,
                         float* dxr, float* dxi, float* dhr, float* dhi, void* stream);

/* The DeepFilter head at inference in one launch (csrc/df_head.hip; model/deep_filter.py:15-41 with the one real filter channel
 * unet_2 emits; additive entry point).  mask [B*T, Fn] (sigmoid output), nre / nim / ere / eim [B, T, Fs] frame-major:
 *   P = mask * N on [0,T) x [0,Fn), zero on bins Fn..Fs-1 (repair R8) and outside the spectrum
 *   E[b,t,f] = sum_{dt=-t_dim..t_dim} sum_{df=-f_dim..f_dim} P[b,t+dt,f+df]      (real and imaginary plane separately)
 * f32 adds from 0.0f, dt the outer and df the inner loop, both ascending: the bits of cruse_mask_apply(mask, ones, zeros) followed
 * by cruse_deepfilter_fwd(nre, nim, hr, zeros, F = T, T = Fs, f_dim = t_dim, t_dim = f_dim) on finite data.  Fn <= Fs, t_dim <= 8,
 * f_dim <= 16; no alignment is required, no workspace is used. */
int cruse_df_head_apply(const float* mask, const float* nre, const float* nim, int B, int T, int Fn, int Fs, int t_dim, int f_dim,
                        float* ere, float* eim, void* stream);

/* backward of nn.Sigmoid (cruse_net.py:164): dlogit = dmask * mask * (1 - mask) */
int cruse_sigmoid_bwd(const float* dmask, const float* mask, float* dlogit, long long n, void* stream);

/* out = a*x + b*y elementwise (x or y may alias out) */
int cruse_axpby(float* out, const float* x, const float* y, float a, float b, long long n, void* stream);

/* ---- general NCHW blocks: the reference's other conv-recurrent modules (cust_conv.py, mtfaa.py) ---------------- */

/* nn.Conv2d / nn.ConvTranspose2d with arbitrary kernel, stride, dilation, groups and zero padding on [B,C,H,W]
 * (model/based_model/cust_conv.py:47-55,94-104,150-166; model/mtfaa.py:60-73,170-183), optional nearest
 * FreqUpsample folded into the gather index (cust_conv.py:163-166,177-184) and a fused ReLU / PReLU.
 *   transposed 0: y[b,co,ho,wo] = bias[co] + sum w[co][ci_l][kh][kw] * X[b,ci, ho*sh-pt+kh*dh, wo*sw-pl+kw*dw],
 *                 X = zero-padded x (W index divided by up_w when up_w > 1; Win is the size before upsampling)
 *   transposed 1: gather form of ConvTranspose2d(padding=(pt,pl)), weight [Cin][Cout/g][KH][KW]
 * The data gradient of either form is the other form with the same weight tensor.  act 0 none, 1 ReLU, 2 PReLU(slope[co]).
 * dtype (CRUSE_DT_*): storage type of x / y (and of S, Bg, dy, dx in the functions below); weights, bias, dw stay f32. */
int cruse_conv2d_nchw(const void* x, const float* w, const float* bias, void* y,
                      int B, int Cin, int Hin, int Win, int Cout, int Hout, int Wout,
                      int KH, int KW, int sh, int sw, int dh, int dw, int pt, int pl,
                      int groups, int up_w, int transposed, int act, const float* slope, int accumulate, int dtype,
                      void* stream);
/* dw[ca][cb_l][kh][kw] += sum_{n,h,w} S[n,ca,h,w] * Bg[n, g*CB/groups + cb_l, h*sh-pt+kh*dh, (w*sw-pl+kw*dw_)/up_w]
 * Conv2d: S = dy, Bg = x.  ConvTranspose2d: S = x, Bg = dy. */
int cruse_conv2d_nchw_wgrad(const void* S, const void* Bg, float* dw,
                            int N, int CA, int HS, int WS, int CB, int HB, int WB,
                            int KH, int KW, int sh, int sw, int dh, int dw_, int pt, int pl,
                            int groups, int up_w, int dtype, void* stream);
/* (round 5, ABI 11) the same for nn.Conv2d (S = dy) with the bias gradient db[ca] += sum_{n,h,w} dy[n,ca,h,w] in the same call: inside the
 * pointwise MFMA kernel (the constant 1 rides a spare column of the last column tile), else by cruse_nchw_channel_sum.  db nullable. */
int cruse_conv2d_nchw_wgrad_ex(const void* S, const void* Bg, float* dw, float* db,
                               int N, int CA, int HS, int WS, int CB, int HB, int WB,
                               int KH, int KW, int sh, int sw, int dh, int dw_, int pt, int pl,
                               int groups, int up_w, int dtype, void* stream);
/* out[c] += sum_{n,hw} x[n,c,hw] (conv bias gradient) */
int cruse_nchw_channel_sum(const void* x, int N, int C, int HW, float* out, int dtype, void* stream);
/* gradient of the nearest FreqUpsample: dx[..,w] = sum_{j<up} dxu[.., w*up + j] */
int cruse_downsum_w(const void* dxu, long long rows, int W, int up, void* dx, int dtype, void* stream);
/* nearest FreqUpsample (cust_conv.py:177-184) of a tensor whose last axis is W: xu[.., w*up + j] = x[.., w]; the frame-major
   upsample decoder (model/cruse.py:14, convkxf mode="upsample") materialises it for its (1,3) conv and that conv's weight gradient */
int cruse_upsample_w(const void* x, long long rows, int W, int up, void* xu, int dtype, void* stream);
/* nn.BatchNorm2d (+ nn.ReLU / nn.PReLU(C) / nn.Sigmoid: act 1 / 2 / 3) on [N,C,HW]: batch sums for cruse_bn_finalize; y = act(gamma*(x-mean)*rstd+beta)
 * (mean == NULL: activation only); backward with the PReLU slope gradient.  scratch: 3*C doubles. */
int cruse_bn_nchw_stats(const void* x, int N, int C, int HW, double* sums, int dtype, void* stream);
int cruse_bn_nchw_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* slope, int act, int N, int C, int HW, void* y, int dtype, void* stream);
int cruse_bn_nchw_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, const float* slope, int act, int training, int N, int C, int HW,
                      double* scratch, void* dx, float* dgamma, float* dbeta, float* dslope, int dtype, void* stream);

/* Round 5 (ABI 11): the same two passes with their small companions folded in.
 * cruse_bn_nchw_fwd_train: training-mode nn.BatchNorm2d (+ act) from the batch sums of cruse_bn_nchw_stats -- mean / rstd are formed inside the
 *   kernel and published to mean_out / rstd_out, running_mean / running_var (nullable pair: momentum, unbiased variance) and
 *   num_batches_tracked (nullable, += 1) are updated: cruse_bn_finalize + cruse_counters_add + cruse_bn_nchw_fwd in one launch
 *   (nn.Conv2d -> nn.BatchNorm2d -> nn.PReLU of TFCM_Block, mtfaa.py:166-193; Conv2dNormAct, cust_conv.py:15-111).
 *   sums may be sum_replicas x [2C] (cruse_conv2d_nchw_ex): the statistic is the sum over the replicas.
 * cruse_conv2d_nchw_ex: cruse_conv2d_nchw (no accumulation) with what follows a convolution in the reference's blocks folded in, both optional:
 *   residual != NULL: y = conv(x) + residual (TFCM_Block, mtfaa.py:191) in the epilogue of the f16 LDS-transposed pointwise kernel (else by
 *   cruse_add_nchw); bn_sums != NULL: the batch sums of the output into bn_sums [bn_nrep][2*Cout] f64 (cleared by the caller) from the
 *   epilogue of the f16 pointwise-MFMA / LDS-depthwise kernels (else the statistics pass over y into replica 0).  Not both.
 * cruse_bn_nchw_bwd_ex: cruse_bn_nchw_bwd (scratch: 4*C doubles) whose apply pass also adds the parameter gradients and, when dx_sum != NULL,
 *   dx_sum[c] += sum over the channel of dx -- the bias gradient of the convolution in front of the BatchNorm -- in closed form from the
 *   reduce pass's sums (training: -gamma rstd mean(d xhat) sum(xhat), the rounding of the batch mean; eval: gamma rstd sum(d)) instead of a
 *   channel-sum pass over dx. */
int cruse_bn_nchw_fwd_train(const void* x, const double* sums, int sum_replicas, float eps, float momentum, const float* gamma, const float* beta,
                            const float* slope, int act, int N, int C, int HW, void* y, float* mean_out, float* rstd_out,
                            float* running_mean, float* running_var, long long* num_batches_tracked, int dtype, void* stream);
int cruse_conv2d_nchw_ex(const void* x, const float* w, const float* bias, const void* residual, void* y,
                         int B, int Cin, int Hin, int Win, int Cout, int Hout, int Wout,
                         int KH, int KW, int sh, int sw, int dh, int dw, int pt, int pl,
                         int groups, int up_w, int transposed, int act, const float* slope,
                         double* bn_sums, int bn_nrep, int dtype, void* stream);
int cruse_bn_nchw_bwd_ex(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, const float* slope, int act, int training, int N, int C, int HW,
                         double* scratch, int scratch_zeroed, int sums_replicas, void* dx, float* dgamma, float* dbeta, float* dslope, float* dx_sum,
                         int dtype, void* stream);
/* The data gradient of a convolution whose INPUT was a BatchNorm2d (+ act) output: y = conv(x) (no bias / act / accumulation) is the gradient wrt that
 * output; the f16 pointwise-MFMA / LDS-depthwise kernels also accumulate the BatchNorm's backward sums of the stored y against bn_x (its input) into
 * r [r_nrep][4][Cout] f64 (cleared by the caller): cruse_bn_nchw_bwd_ex(scratch = r, sums_replicas = r_nrep) then skips its reduce pass.
 * *delivered = 0: the form that ran has no such epilogue -- run the plain backward (sums_replicas = 0).
 * Replaces autograd's conv_backward(input) + the reduction half of batch_norm_backward for nn.Conv2d after nn.BatchNorm2d + nn.PReLU
 * (TFCM_Block, mtfaa.py:170-183; Conv2dNormAct, cust_conv.py:15-111). */
int cruse_conv2d_nchw_bnbwd(const void* x, const float* w, void* y,
                            int B, int Cin, int Hin, int Win, int Cout, int Hout, int Wout,
                            int KH, int KW, int sh, int sw, int dh, int dw, int pt, int pl, int groups, int transposed,
                            const void* bn_x, const float* bn_mean, const float* bn_rstd, const float* bn_gamma, const float* bn_beta,
                            const float* bn_slope, int bn_act, double* r, int r_nrep, int* delivered, int dtype, void* stream);
/* Host-only, touches no device: what cruse_conv2d_nchw / _ex / _bnbwd (wgrad = 0) or cruse_conv2d_nchw_wgrad / _wgrad_ex (wgrad = 1) launch for
 * a call -- the same validation and the same decision as the call, without the launches.  The geometry is that of the entry point (wgrad:
 * B, Cin, Hin, Win, Cout, Hout, Wout = N, CA, HS, WS, CB, HB, WB, dw = dw_; transposed, act, accumulate = 0).  requests: the optional outputs
 * the call asks for -- BN_SUMS / RESIDUAL (cruse_conv2d_nchw_ex: bn_sums, residual), BNBWD (cruse_conv2d_nchw_bnbwd), DB (wgrad_ex: db) -- and
 * with them the entry point; an argument that entry point does not have must be neutral.  out[11]:
 *   [0] kernel form: conv 0 f16 pointwise MFMA, operand transposed through LDS; 1 f16 pointwise MFMA, gather; 2 pointwise VALU;
 *       3 f16 depthwise on an LDS image; 4 depthwise; 5 general -- wgrad 0 f16 pointwise MFMA; 1 f16 depthwise on an LDS image; 2 depthwise;
 *       3 a row pair in LDS; 4 one block row per weight
 *   [1] [2] the kernel's template integers (16-row tiles x 32-deep k-steps; MAXCO of form 2; else 0)   [3] [4] [5] grid x, y, z   [6] block
 *   [7] dynamic LDS bytes    [8] conv form 0: epilogue instance (0 plain, 1 batch sums, 2 BatchNorm-backward sums); wgrad form 0: positions
 *       per block, form 2: positions per thread
 *   [9] the requests served in the kernel's epilogue (cruse_conv2d_nchw_bnbwd's *delivered is its BNBWD bit)
 *   [10] the pass owed for the others: 0 none, 1 cruse_add_nchw after, 2 cruse_bn_nchw_stats_ex after, 3 cruse_nchw_channel_sum before
 * Returns what the entry point would: an error code and cruse_last_error() where the call is refused. */
enum { CRUSE_NCHW_REQ_BN_SUMS = 1, CRUSE_NCHW_REQ_RESIDUAL = 2, CRUSE_NCHW_REQ_BNBWD = 4, CRUSE_NCHW_REQ_DB = 1 };
int cruse_conv2d_nchw_plan(int wgrad, int B, int Cin, int Hin, int Win, int Cout, int Hout, int Wout,
                           int KH, int KW, int sh, int sw, int dh, int dw, int pt, int pl,
                           int groups, int up_w, int transposed, int act, int accumulate, int dtype, int requests, int* out);

/* cruse_bn_nchw_stats into sums the caller cleared itself (zeroed != 0; like scratch_zeroed above: one fill launch per pool chunk of
 * accumulators instead of one per call) */
int cruse_bn_nchw_stats_ex(const void* x, int N, int C, int HW, double* sums, int zeroed, int dtype, void* stream);

/* out = a + b on n elements of storage type dtype (TFCM_Block residual, mtfaa.py:191; GroupGRU add_outputs, cust_conv.py:411-412) */
int cruse_add_nchw(const void* a, const void* b, void* out, long long n, int dtype, void* stream);
/* f32 -> f16 (to_f16 != 0) or f16 -> f32 copy of n elements: where the fp16 part of a model (BASELINE config 5) begins / ends */
int cruse_cast_f16(const void* src, void* dst, long long n, int to_f16, void* stream);

/* ---- other STFT formulations (feature.py:272-398 CustomSTFT/CustomISTFT, conv_stft.py:8-129, mtfaa.py:8-37) ------- */
/* X[b,t,f] = scale * sum_{n<win_len} window[n] * x_pad[b, t*hop + n + win_off - pad] * exp(-2 pi i f (n + win_off)/n_fft),
 * f = 0..n_fft/2; x_pad: pad_mode 0 zeros / 1 reflect outside the clip.  re, im [B,T,n_fft/2+1]. */
int cruse_stft_framed(const float* wave, const float* window, int B, int L, int n_fft, int win_len, int win_off,
                      int hop, int pad, int pad_mode, int T, float scale, float* re, float* im, void* stream);
/* overlap-add adjoint: out[b,m] = post[m] * sum_{t,n: t*hop+n+win_off-pad == m} window[n]*scale*sum_f c_f (re cos - im sin);
 * hermitian 0: c_f = 1 (conv_transpose1d with the analysis kernel, feature.py:395); 1: c_f = 1,2,..,2,1 (inverse DFT of a
 * one-sided spectrum, conv_stft.py:106-122).  post: L per-sample factors (1 / window-overlap envelope) or NULL. */
int cruse_istft_framed(const float* re, const float* im, const float* window, const float* post, int B, int T,
                       int n_fft, int win_len, int win_off, int hop, int pad, int L, float scale, int hermitian,
                       float* out, void* stream);

/* ---- masks, further losses, data synthesis ------------------------------------------------------------------------ */
/* train_base/acoustics/mask.py:8-63.  mode 0 IRM (a = noisy_mag, c = clean_mag), 1 cIRM (a,b = noisy re,im; c,d = clean
 * re,im; out [n,2]), 2 compress_cIRM(a), 3 decompress_cIRM(a), 4 complex_mul (a + ib)(c + id) -> out, out2;
 * PreProcess (utils/utils.py:414-423): 5 pair product out = a*c, out2 = b*d ("complex_mapping"), 6 out = log(a).
 * Adjoints (the reference's ops are plain torch, hence differentiable): 7 out = c * compress'(a), 8 out = c * decompress'(a)
 * (c = upstream gradient), 9 (a + ib) conj(c + id) -> out, out2 (both gradients of mode 4). */
int cruse_mask_ops(int mode, const float* a, const float* b, const float* c, const float* d, long long n,
                   float K, float C, float limit, float* out, float* out2, void* stream);
/* mode 0: (re, im) -> (sqrt(re^2+im^2+eps)**alpha, atan2(im, re)) (feature.py:363-364, mtfaa.py:136-137,162);
 * mode 1: (mag, phase) -> (mag cos, mag sin) (feature.py:386-387); mode 2: gradient of mode 0 (g = d mag, g2 = d phase,
 * either may be NULL) -> (d re, d im); mode 3: gradient of mode 1 (a, b = mag, phase; g, g2 = d re, d im) -> (d mag, d phase). */
int cruse_polar(int mode, const float* a, const float* b, const float* g, const float* g2, long long n, float eps, float alpha,
                float* o1, float* o2, void* stream);
/* rmse (loss_func/loss.py:59-78): loss_sum = sum |est - ref| (divide by B*T*F); dest = sign(est-ref)*grad_scale (may be NULL) */
int cruse_rmse(const float* ref, const float* est, long long n, float grad_scale, double* loss_sum, float* dest, void* stream);
/* c_rmse (loss_func/loss.py:88-118) as written; ref, est [B,2,TF]; dest = d loss / d est (may be NULL) */
int cruse_c_rmse(const float* ref, const float* est, int B, long long TF, float c, float beta, double* loss_sum, float* dest,
                 void* stream);
/* wo_male (loss_func/loss.py:121-148) on explicit spectra ref, est, unproc: element (b, j) has its real part at
 * b*bstride + j and its imaginary part pstride further ([B,2,TF]: 2*TF, TF; [2,B,TF]: TF, B*TF).  loss_sum (divide by
 * B*T*F) and dest = grad_scale * d loss_sum / d est (may be NULL).  The mask-only step uses the fused cruse_mask_loss_fwd;
 * the DeepFilter step (BASELINE config 4) uses this form on the filtered spectrum. */
int cruse_wo_male_spec(const float* ref, const float* est, const float* unproc, int B, long long TF, long long bstride,
                       long long pstride, float alpha, float beta, float grad_scale, double* loss_sum, float* dest, void* stream);
/* sisnr (loss_func/loss.py:48-56, no mean removal) from the moments cruse_sisnr_fwd's first pass leaves in `mom`:
 * value = mean_b 10 log10(.), coef [B,4] for cruse_sisnr_bwd (gradient of the VALUE; the loss is its negative) */
int cruse_sisnr_plain_finalize(const double* mom, int B, float eps, double* value, float* coef, void* stream);
/* synthetic clips: y[b,n] = gain*(1-a) * sum_{k<taps} a^k x[b,n-k], a one-pole low-pass as a truncated FIR */
int cruse_onepole_fir(const float* x, int B, int L, float a, int taps, float gain, float* y, void* stream);
/* y[b,n] = sum_{k < R, k <= n} h[b or 0][k] x[b,n-k] = scipy.signal.fftconvolve(x, h)[:L]: the room-impulse-response
 * convolution at the top of SynDataset.snr_mix (dataset/dataset.py:245-248).  h_bstride = 0: one tap row for all clips,
 * else tap rows h_bstride >= R floats apart.  Out of place. */
int cruse_fir_causal(const float* x, const float* h, long long h_bstride, int B, int L, int R, float* y, void* stream);
/* SynDataset.snr_mix (dataset/dataset.py:236-264) for B clips at once: peak-normalise both, scale the noise to snr_db[b]
 * from the RMS ratio, mix.  scratch: 24*B bytes.  clean_out / noise_out may be NULL. */
int cruse_snr_mix(const float* clean, const float* noise, const float* snr_db, int B, int L, float eps,
                  void* scratch, float* clean_out, float* noise_out, float* noisy, void* stream);

/* ---- scheduling aids ------------------------------------------------------------------------------------------------ */
/* a HIP stream restricted to the CUs whose bit is set in mask[0..nwords) (hipExtStreamCreateWithCUMask) */
int cruse_stream_create_masked(void** stream_out, const unsigned* mask, int nwords);
/* out[2*b], out[2*b+1] = HW_REG_XCC_ID, HW_REG_HW_ID of block b (each block idles `spin` clock ticks): placement census */
int cruse_cu_census(unsigned* out, int nblocks, unsigned spin, void* stream);
/* test / probe rig: nblocks workgroups that each HOLD a CU (128 KB of LDS) for `ticks` shader clocks -- what a collective's
 * channels or another tenant do to the persistent recurrences, whose teams must be co-resident (tests/test_gpu_ddp.py) */
int cruse_cu_hog(int nblocks, unsigned long long ticks, void* stream);

/* ---- stream-ordered bookkeeping (keeps the training step free of library kernels) ---- */
/* zero-fill `bytes` (multiple of 4) with a KERNEL node (hipMemsetAsync nodes raced inside captured graphs) --
 * optimizer.zero_grad() at the top of the step */
int cruse_zero(void* p, size_t bytes, void* stream);
/* acc[i] += x[i] (f64): running loss sum of an epoch without a host synchronisation per step */
int cruse_accum_f64(double* acc, const double* x, int n, void* stream);
/* *counters[i] += v for a HOST array of n <= 32 device int64 pointers: BatchNorm2d.num_batches_tracked */
int cruse_counters_add(long long* const* counters, int n, long long v, void* stream);

/* ---- optimizer (torch.optim.Adam at tools/train_stand.py:68-71) -------------- */
/* One fused Adam step over a flat parameter buffer; g is multiplied by grad_scale first
 * (1/world_size after a sum all-reduce). step >= 1. */
int cruse_adam_step(float* p, const float* g, float* m, float* v, long long n,
                    float lr, float beta1, float beta2, float eps, float weight_decay,
                    int step, float grad_scale, void* stream);
/* The same step behind device-side guards, so that one bad batch cannot poison the parameters and no host
 * synchronisation is needed to decide (all pointers optional):
 *   skip_flag  : n_skip_words u32 words; any non-zero word skips the step (the sticky GRU hand-off status word of
 *                cruse_gru_seq_fwd, or the -- possibly all-reduced -- health words of cruse_step_health);
 *   loss_check : a non-finite *loss_check skips the step (the reference has no such check: a 0/0 bin in wo_male,
 *                loss_func/loss.py:141, would turn every parameter into NaN);
 *   gsumsq     : sum of squares of g (cruse_sumsq); a non-finite norm skips the step; with max_norm > 0 the gradient is
 *                scaled by min(1, max_norm / (sqrt(gsumsq)*grad_scale + 1e-6)) = torch.nn.utils.clip_grad_norm_
 *                (train_base/trainer/base_trainer.py:75 `clip_grad_norm_value`);
 *   skipped    : skipped[0] += 1 for every skipped step; with n_skip_words > 1 also skipped[1 + i] += 1 for each
 *                non-zero word i (per-reason counters).  The bias corrections use step - skipped[0] (the value BEFORE this
 *                call): a skipped step does not advance Adam's step, as if torch.optim.Adam.step() had not been called;
 *   loss_sum / loss_acc (ABI 7): when the step is APPLIED, loss_acc[0] += *loss_sum * loss_scale and loss_acc[1] += 1 --
 *                the running epoch loss counts exactly the steps that reached the parameters (a timed-out step's loss is
 *                garbage even when finite), each with its own normalisation. */
int cruse_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n,
                            float lr, float beta1, float beta2, float eps, float weight_decay,
                            int step, float grad_scale, float max_norm, const double* gsumsq,
                            const unsigned* skip_flag, int n_skip_words, const double* loss_check, unsigned* skipped,
                            const double* loss_sum, double loss_scale, double* loss_acc, void* stream);
/* Per-step health of a training step, decided on the device (no reference counterpart: train/trainer_casual.py is empty
 * and base_trainer.py has no guard).  health[0] = the GRU status word was set -- and CLEARS it, so one transient
 * hand-off time-out costs the step it happened in, not every later one; health[1] = *loss_sum is not finite.
 * loss_acc (optional) += *loss_sum * loss_scale when finite (the running epoch loss, each step with its own norm).
 * Data-parallel callers all-reduce health[0..1] with MAX before handing it to cruse_adam_step_guarded, so that every
 * rank takes the same skip decision.  gru_status may be NULL. */
int cruse_step_health(unsigned* gru_status, const double* loss_sum, unsigned* health, double* loss_acc,
                      double loss_scale, void* stream);
/* out (+)= sum x[i]^2 in f64 (total gradient norm for clip_grad_norm_); x 16-byte aligned */
int cruse_sumsq(const float* x, long long n, double* out, int accumulate, void* stream);

/* ---- frame-by-frame streaming inference of unet_2 (n_fft = win = 320, hop = 160; ABI 13, additive) ---------------------
 * One hop of S independent streams ("slots"): cruse_stream_encode -> cruse_stream_gru (layer 1) -> cruse_stream_gru (layer 2)
 * -> cruse_stream_decode, dependent launches on one stream.  mode[S] (device, int) says what each slot does in this chain;
 * a SKIP slot is not touched.  Per-slot state and work rows are laid out by cruse_stream_layout.  f32 throughout.
 * Stands for, one frame at a time: feature.stft + PreProcess.pre_stft (train_base/acoustics/feature.py:10-30,
 * utils/utils.py:397-405), unet_2.forward with GGRU (model/cruse_net.py:14-55,147-165), PreProcess.masking
 * (utils/utils.py:417-420) and feature.istft (train_base/acoustics/feature.py:33-61). */
enum {
    CRUSE_STREAM_MODE_SKIP = 0,   /* slot not active in this chain                                                      */
    CRUSE_STREAM_MODE_STORE = 1,  /* block 0: store the block in the analysis history, no frame                          */
    CRUSE_STREAM_MODE_FRAME = 2,  /* frame b from the previous block and this one; the history advances                  */
    CRUSE_STREAM_MODE_FRAME0 = 3, /* frame 0 (first half reflected, x[160] from this block); the history does not advance */
    CRUSE_STREAM_MODE_END = 4     /* the end frame: last block and its end reflection; no input                          */
};
#define CRUSE_STREAM_LAYOUT_INTS 62
/* out[CRUSE_STREAM_LAYOUT_INTS] (HOST array): ch[5], F[5], H, packed-weight offsets encW[5], encB[5], skW[5], decW[5], decB[5]
 * (index = level, 0 unused), ln1g, ln1b, ln2g, ln2b, weight floats; state-row offsets hist, tail, prev[4] (mag, e1, e2, e3), h1,
 * h2, state stride; work-row offsets re, im, x (GRU input, c*F4+f), skip[5], h1 (new), h2 (new), mask, work stride (floats).
 * Rejects ch[0] != 1. */
int cruse_stream_layout(int c0, int c1, int c2, int c3, int c4, int* out);
/* tab[1120] (device) <- periodic Hann(320), cos / sin(2 pi j / 320), 1 / (w^2(m) + w^2(m+160)); synchronises `stream` */
int cruse_stream_tables(float* tab, void* stream);
/* frame assembly from the history, Hann window, 320-point real DFT (re / im of 161 bins -> work), mag = sqrt(re^2+im^2+1e-8) of
 * bins 0..159, the four encoder convs (2,3) on (previous row, this row) with BatchNorm folded into w and ReLU, the four skip
 * convs (1,3), the GRU input row; updates history and previous rows.  in[S][160]: this hop's blocks (model/cruse_net.py:147-156,
 * train_base/acoustics/feature.py:10-30, utils/utils.py:397-405) */
int cruse_stream_encode(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* in, const float* tab,
                        const float* w, float* state, float* work, void* stream);
/* one GGRU layer (model/cruse_net.py:22-50), one time step: g groups of Hg units (Hg % 4 == 0, Hg <= 1024), gate order r,z,n,
 * b_hn inside r*(.).  pack = W_ih [g][3Hg][Hg] | W_hh [g][3Hg][Hg] | b_ih [g][3Hg] | b_hh [g][3Hg].  Slot s reads
 * x[s*x_stride + x_off + ...] and hprev[s*h_stride + h_off + i*Hg + j], writes hout[s*o_stride + o_off + i*Hg + j].  layer 1:
 * group i reads x chunk i.  layer 2: x is layer 1's output row (group-contiguous); LN1 (ln_g, ln_b, ln_eps) is applied to its
 * interleaved view v[j*g+i] (cruse_net.py:43-46) and group i reads chunk i of LN1(v).  Refused with CRUSE_E_SHAPE before any launch:
 * S < 1, g < 1, Hg % 4 != 0, Hg > 1024, and x_off / h_off / o_off < 0 or + g*Hg beyond x_stride / h_stride / o_stride */
int cruse_stream_gru(const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                     const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                     const float* pack, float* hout, int o_stride, int o_off, void* stream);
/* LN2 of the layer-2 output + skip4, the four ConvTranspose (1,3) stride 2 levels (last column cropped, BatchNorm folded, ReLU,
 * + skip; the last one sigmoid: model/cruse_net.py:158-164), the mask on bins 0..159 with bin 160 zero (utils/utils.py:417-420),
 * 320-point inverse real DFT, window, overlap-add with the stored tail and division by the window envelope
 * (train_base/acoustics/feature.py:33-61) -> out[S][160]; copies the new GRU states into the state rows */
int cruse_stream_decode(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                        float ln_eps, float* state, float* work, float* out, void* stream);

/* ---- packets: up to `hops` blocks per slot in one chain (additive; state rows and cruse_stream_layout are shared with the
 * single-hop entry points above, so both kinds of call may be mixed on a slot) -------------------------------------------------
 * pk[2*S] (device, int): pk[s] = blocks slot s held before the call, clamped to 2 (0: none, 1: block 0 only, 2: two or more);
 * pk[S + s] = count of blocks slot s consumes, 0..hops (0: the slot is not touched).  A slot computes nf frames: count if it
 * held two or more blocks, count + 1 if it held one (frame 0 and the frames of the new blocks), count if it held none and
 * count >= 2 (frames 0..count-1), none if it held none and count == 1 (the block is stored).  Frame f of slot s has its own work
 * row work[(s * work_frames + f) * WS] (work_frames >= hops + 1): the row of cruse_stream_layout followed by e1 | e2 | e3.  The chain is encode_n -> gru_proj_n (layer 1) ->
 * gru_rec_n for frame 0..nf_max-1 -> gru_proj_n (layer 2) -> gru_rec_n ... -> decode_n, dependent launches on one stream.
 * One workgroup per slot holds two rows per frame and one level's weights in LDS (128 KiB budget), which bounds work_frames;
 * more is CRUSE_E_SHAPE. */
/* out[5] (HOST array): the largest supported hops (work_frames - 1), the packet work-row stride WS (floats), the offsets of
 * e1, e2, e3 in that row */
int cruse_stream_packet_layout(int c0, int c1, int c2, int c3, int c4, int* out);
/* cruse_stream_encode for every frame of the packet, level by level over the frames with the level's folded weights staged in
 * LDS: frames from the history and in[S][in_hops][160] (frame 0's reflection where the packet starts a clip), DFT, magnitude,
 * encoder and skip convs, GRU input rows; history and previous rows advance to the last consumed block / frame */
int cruse_stream_encode_n(const int* pk, int S, int hops, int in_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                          const float* in, const float* tab, const float* w, float* state, float* work, void* stream);
/* input products of one GGRU layer (pack as cruse_stream_gru) for every (slot, frame): gi[(s * work_frames + f) * 3H + c*H + u] =
 * W_ih[c][u] . x + b_ih (+ b_hh for c = r, z), x = the frame's work row at x_off (layer 2: LN1 of its interleaved view first).
 * Refused with CRUSE_E_SHAPE: the shapes cruse_stream_gru refuses, hops < 1, work_frames < hops + 1, x_off + g*Hg beyond wk_stride,
 * S * (hops + 1) beyond INT_MAX */
int cruse_stream_gru_proj_n(const int* pk, int S, int hops, int work_frames, int layer, int g, int Hg, const float* work,
                            int wk_stride, int x_off, const float* ln_g, const float* ln_b, float ln_eps, const float* pack,
                            float* gi, void* stream);
/* recurrent step `frame` of that layer for every slot with frame < nf: h' from gi, W_hh . h and b_hn into the frame's work row at
 * h_off; h is the state row at st_off for frame 0, the previous frame's work row else.  Refused with CRUSE_E_SHAPE: as gru_proj_n, frame
 * outside [0, hops], st_off + g*Hg beyond st_stride, h_off + g*Hg beyond wk_stride */
int cruse_stream_gru_rec_n(const int* pk, int S, int hops, int work_frames, int frame, int g, int Hg, const float* gi,
                           const float* state, int st_stride, int st_off, const float* pack, float* work, int wk_stride, int h_off,
                           void* stream);
/* cruse_stream_decode for every frame of the packet side by side, then the overlap-add as a chain over the frames:
 * out[S][out_hops][160], slot s's blocks in order from index 0 (frame 0 of a clip yields none); the GRU rows of the slot's last
 * frame become its state */
int cruse_stream_decode_n(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                          const float* tab, const float* w, float ln_eps, float* state, float* work, float* out, void* stream);

/* ---- sample formats and the per-slot attenuation limit in the boundary kernels (additive; the entry points above are unchanged and
 * launch the same kernels as before) ---------------------------------------------------------------------------------------------
 * Each takes its sibling's arguments plus: in_fmt / out_fmt: 0 = f32, 1 = s16 (16-bit PCM) -- the element type of `in` / `out`.  An s16
 * input sample v is read as v / 32768.0f (exact); an s16 output sample is clamp(rint(y * 32768), -32768, 32767), ties to even.
 * lim[S] (device, may be NULL: no limit): the slot's attenuation limit as a linear gain, lim = 10^(-dB / 20) in [0, 1]; the output is
 * lim * noisy + (1 - lim) * enhanced, mixed on the spectrum: bins 0..159 are scaled by fmaf(1 - lim, mask, lim) and bin 160 by lim
 * (DeepFilterNet's atten_lim_db).  The mask row of the work buffer keeps the model's mask.  lim = 0 gives the sibling's output.
 * clip[S] (device int, may be NULL: not counted; needs out_fmt 1): clip[s] += the s16 samples of slot s this launch clamped.
 * Slots that compute no frame are neither written nor counted.  Refused with CRUSE_E_SHAPE before any launch: what the sibling
 * refuses, an unknown format, a clip counter with f32 output. */
int cruse_stream_encode_io(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const void* in, int in_fmt,
                           const float* tab, const float* w, float* state, float* work, void* stream);
int cruse_stream_decode_io(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                           float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                           void* stream);
int cruse_stream_encode_n_io(const int* pk, int S, int hops, int in_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                             const void* in, int in_fmt, const float* tab, const float* w, float* state, float* work,
                             void* stream);
int cruse_stream_decode_n_io(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                             const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                             const float* lim, int* clip, void* stream);

/* ---- the perceptual post-filter (additive; every entry point above is unchanged and launches the same kernels with the same
 * arguments) ------------------------------------------------------------------------------------------------------------------------
 * The reference's numpy post-filters of a mask value g in [0, 1] (utils/utils.py:345-362), in closed form; s = sin(pi g / 2), tau >= 0:
 *   pf_kind 1, "iam"      (postfiltering, utils/utils.py:345-349):           pf = g (1 + tau) s^2 / (s^2 + tau)
 *   pf_kind 2, "envelope" (envelope_postfiltering, utils/utils.py:352-362):  pf = g s sqrt((1 + tau) s / (s^2 + tau))
 * pf(0) = 0 (the reference's "iam" form is 0 / 0 there), pf(1) = 1; the "envelope" form's eps term, its only use of the unprocessed
 * magnitude, is dropped.  tau == 0 is a bypass: pf = g to the bit.
 * cruse_stream_decode_pf / _n_pf (utils/utils.py:345-362): the _io sibling's arguments plus pf_kind and pf_tau[S] (device; the slot's
 * tau, 0: off).  The gain of bins 0..159 is pf(mask) without a limit and fmaf(1 - lim, pf(mask), lim) with one (DeepFilterNet's order);
 * bin 160 as in the sibling; the mask row of the work buffer keeps the model's mask.  With every pf_tau 0 the output is the sibling's.
 * Refused with CRUSE_E_SHAPE before any launch: what the sibling refuses, pf_kind outside {1, 2}, a null pf_tau. */
int cruse_stream_decode_pf(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                           float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                           int pf_kind, const float* pf_tau, void* stream);
int cruse_stream_decode_n_pf(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                             const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                             const float* lim, int* clip, int pf_kind, const float* pf_tau, void* stream);
/* the same function on a whole mask tensor (utils/utils.py:345-362), one pointwise launch: out[r][f] = pf(mask[r][f], tau[r /
 * rows_per_tau]) for r < rows, f < F; rows_per_tau = 0: tau[0] serves every row (a scalar tau), else tau holds ceil(rows /
 * rows_per_tau) values (a [B,1,T,F] mask with a tau per clip: rows = B * T, rows_per_tau = T).  tau is device memory; its values must
 * be >= 0 (not checked: the call does not synchronise).  out may be mask.  16-byte accesses where mask and out are 16-byte aligned,
 * scalar over the last rows * F % 4 elements and everywhere else; deterministic, capturable.  Refused with CRUSE_E_SHAPE before the
 * launch: kind outside {1, 2}, rows < 1, F < 1, rows_per_tau outside [0, rows], a null pointer. */
int cruse_mask_postfilter(int kind, const float* mask, long long rows, long long F, const float* tau, long long rows_per_tau,
                          float* out, void* stream);

/* ---- the upsample decoder (additive; every entry point above is unchanged) ---------------------------------------------------------
 * cruse_stream_decode_up / _n_up: cruse_stream_decode_pf / _n_pf for model/cruse.py's CRUSE4MagAddSkipUpsample, whose decoder levels are
 * convkxf(mode="upsample") (model/based_model/cust_conv.py:163-166,177-184): nearest x2 FreqUpsample along frequency, then Conv2d (1,3),
 * padding (0,1), [Cin][Fin] -> [Cout][2*Fin].  With u[i] = in[i >> 1] for 0 <= i < 2*Fin and zero outside,
 *   out[co][fo] = b[co] + sum_ci sum_kw W[co][ci][kw] * u[fo - 1 + kw]
 * (fo = 2j reads in[j-1], in[j], in[j]; fo = 2j+1 reads in[j], in[j], in[j+1]), BatchNorm folded into W and b, ReLU then + skip on
 * levels 4..2, sigmoid on level 1.  The weights at decW[k] are packed [Cout][Cin][3], the Conv2d order (cruse_stream_decode's are
 * ConvTranspose2d's [Cin][Cout][3]); the float counts are equal, so cruse_stream_layout and cruse_stream_packet_layout serve both
 * decoders.  Encode, the GRU layers, the resamplers and the DeepFilter head are the same calls for both models.  Everything of the
 * kernels but the four decoder levels is cruse_stream_decode's code.
 * One pair covers every form: out_fmt 0 with null lim and clip is the plain form, out_fmt / lim / clip as in the _io siblings, pf_kind
 * 0: no post-filter (pf_tau is not read), pf_kind 1 / 2 with pf_tau[S] as in the _pf siblings.  Refused with CRUSE_E_SHAPE before any
 * launch: what the _io siblings refuse, pf_kind outside {0, 1, 2}, pf_kind != 0 with a null pf_tau. */
int cruse_stream_decode_up(const int* mode, int S, int c0, int c1, int c2, int c3, int c4, const float* tab, const float* w,
                           float ln_eps, float* state, float* work, void* out, int out_fmt, const float* lim, int* clip,
                           int pf_kind, const float* pf_tau, void* stream);
int cruse_stream_decode_n_up(const int* pk, int S, int hops, int out_hops, int work_frames, int c0, int c1, int c2, int c3, int c4,
                             const float* tab, const float* w, float ln_eps, float* state, float* work, void* out, int out_fmt,
                             const float* lim, int* clip, int pf_kind, const float* pf_tau, void* stream);

/* ---- f16-operand MFMA GRU of the streaming chains (additive; rows, mode / pk semantics and the f32 pack are those above, so these
 * may replace their f32 counterparts call by call) ------------------------------------------------------------------------------
 * pack16 (device, f16): the layer's weights as MFMA A fragments, [W_ih | W_hh][g][gate r,z,n][UT][KS][64 lanes][8], UT =
 * ceil(Hg / 16) unit tiles, KS = ceil(Hg / 32) k steps; lane l of (ut, ks) holds W[gate][ut*16 + (l & 15)][ks*32 + (l >> 4)*8 + 0..7],
 * zero where the unit or k is >= Hg.  Rounded to f16: the operand copies of x (after LN1 in layer 2), of h and the weights; accumulation,
 * biases (read from `pack`), LN1 statistics, gates and every row written are f32, and the gates read h_prev in f32.
 * The refusals are those of the f32 entry point of the same kind (one check serves both), plus a null pack16; all before any launch. */
/* cruse_stream_gru on v_mfma_f32_16x16x32_f16: one GGRU layer (model/cruse_net.py:22-50), one time step */
int cruse_stream_gru_f16(const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                         const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                         const float* pack, const void* pack16, float* hout, int o_stride, int o_off, void* stream);
/* cruse_stream_gru_proj_n on the same MFMA: the input products of every (slot, frame) of a packet; gi stays f32 */
int cruse_stream_gru_proj_n_f16(const int* pk, int S, int hops, int work_frames, int layer, int g, int Hg, const float* work,
                                int wk_stride, int x_off, const float* ln_g, const float* ln_b, float ln_eps, const float* pack,
                                const void* pack16, float* gi, void* stream);
/* cruse_stream_gru_rec_n on the same MFMA: W_hh . h and the gates of frame `frame` of a packet */
int cruse_stream_gru_rec_n_f16(const int* pk, int S, int hops, int work_frames, int frame, int g, int Hg, const float* gi,
                               const float* state, int st_stride, int st_off, const float* pack, const void* pack16, float* work,
                               int wk_stride, int h_off, void* stream);

/* ---- 8 / 32 / 48 kHz I/O: sample-rate conversion around the 16 kHz chains (additive; nothing above changes) ----------------------
 * io_rate: 8000, 32000 or 48000.  q = 3 for 48000, else 2; N = 32 q + 1 taps; a block is B = io_rate / 100 samples (10 ms).
 * taps[N] (device, f32): the low-pass h, designed by the host (cruse_amd/inferencer/resample.py: Kaiser-windowed sinc, unit DC gain).
 *   decimate by q, phase 0:  D_q(u)[n] = sum_{k=0}^{N-1} h[k] u[q n - k]
 *   interpolate by q:        I_q(x)[m] = q sum_i h[m - q i] x[i] over 0 <= m - q i <= N - 1
 * both causal from a zero history, summed over k (i) ascending with fmaf in f32.  32000 / 48000: the input side is D_q, the output side
 * I_q; 8000: the input side is I_2, the output side D_2.  rs_state[S][rs_stride] (device, f32) carries the slot's last input samples
 * of each side: [in-side history | out-side history], N - 1 | (N - 1) / q samples at 32000 / 48000 and (N - 1) / 2 | N - 1 at 8000;
 * rs_stride >= their sum.  Zero it where the slot's state row is zeroed.  One workgroup per slot; a slot that converts nothing
 * leaves its history, its output row and its counter untouched.  in_fmt / out_fmt, the s16 conversions and clip[S] are those of
 * the _io entry points.  Refused with CRUSE_E_SHAPE before any launch: S < 1, a null buffer, an unknown io_rate (16000 included) or
 * format, a clip counter with f32 output, rs_stride too small, hops < 1, in_hops / out_hops < hops. */
/* before cruse_stream_encode: a slot whose mode (the MAIN chain's row) is STORE or FRAME reads its block in[s][B] and writes the 160
 * samples blocks[s][160] that cruse_stream_encode reads */
int cruse_stream_resample_in(const int* mode, int S, int io_rate, const void* in, int in_fmt, const float* taps, float* rs_state,
                             int rs_stride, float* blocks, void* stream);
/* after cruse_stream_decode of the main chain: a slot whose mode is FRAME or END reads out16[s][160] and writes out[s][B] */
int cruse_stream_resample_out(const int* mode, int S, int io_rate, const float* out16, const float* taps, float* rs_state,
                              int rs_stride, void* out, int out_fmt, int* clip, void* stream);
/* before cruse_stream_encode_n: slot s converts its pk[S + s] blocks in[s][0..][B] -> blocks[s][0..][160], both [S][in_hops][.] */
int cruse_stream_resample_in_n(const int* pk, int S, int hops, int in_hops, int io_rate, const void* in, int in_fmt, const float* taps,
                               float* rs_state, int rs_stride, float* blocks, void* stream);
/* after cruse_stream_decode_n: slot s converts the output blocks its packet yields (its frames, less frame 0 of a clip; the count
 * follows from pk alone) out16[s][0..][160] -> out[s][0..][B], both [S][out_hops][.] */
int cruse_stream_resample_out_n(const int* pk, int S, int hops, int out_hops, int io_rate, const float* out16, const float* taps,
                                float* rs_state, int rs_stride, void* out, int out_fmt, int* clip, void* stream);

/* ---- the DeepFilter(1, 5) head on the stream (additive; nothing above changes, the kernels above launch as before) ---------------
 * A model trained against the DeepFilter loss emits the real filter field of DeepFilter(t_dim = 1, f_dim = 5), not a mask: with
 * P[t][f] = mask[t][f] * N[t][f] on bins 0..159 and P[t][160] = 0, the enhanced row is E[t][f] = sum_{dt=-1..1} sum_{df=-5..5}
 * P[t+dt][f+df] on all 161 bins, terms outside the spectrum or the clip zero (cruse_df_head_apply, bit for bit: f32 from 0.0f, frame
 * offset outer, bin offset inner, ascending).  These kernels follow cruse_stream_decode / _decode_n in a chain and read nothing but
 * what the chain leaves in the frame's work row: the mask (160 floats at wk_mask) and the noisy spectrum (161 at wk_re, 161 at
 * wk_im), rows wk_stride floats apart -- the offsets of cruse_stream_layout, with the stride of cruse_stream_packet_layout for packets.
 * E[t] needs frame t + 1: a step takes row t, emits E[t-1] (written to df_work, then inverse DFT, window, overlap-add and envelope
 * as cruse_stream_decode, with a tail of its own) and shifts the rows.  The step of a clip's frame 0 (mode FRAME0; a packet's first
 * frame where pk says the slot held at most one block) starts from a zero history and emits nothing.  The block of E[0] lies in front
 * of the clip: it is neither stored nor counted.  df_state[S][st_stride] (device, f32; zero at the start of a clip; st_stride >= the
 * stride of cruse_stream_df_layout) holds P[t-2], P[t-1], N[t-1] (re | im planes), the tail and the count of rows taken (0, 1, 2 = two
 * or more).  out / out_fmt / lim / clip are those of the _io entry points; with lim the spectrum that is inverted is
 * lim * N[t-1] + (1 - lim) * E[t-1] on all 161 bins.  One workgroup per slot.  Refused with CRUSE_E_SHAPE before any launch: a null
 * buffer (lim and clip may be null), S < 1, wk_re / wk_im / wk_mask that do not lie in a row of wk_stride floats or a row shorter than
 * 161 + 161 + 160, st_stride or the df_work rows too small, an unknown format, a clip counter with f32 output, hops outside
 * [1, 47] (the largest any packet layout admits), work_frames < hops + 1, out_hops or dw_frames < hops, and (t_dim, f_dim) other than
 * (1, 5): only that instance is built. */
#define CRUSE_STREAM_DF_LAYOUT_INTS 7
/* out[CRUSE_STREAM_DF_LAYOUT_INTS] (HOST array): offsets in a df_state row of P[t-2], P[t-1], N[t-1] (each re plane, then the im
 * plane `plane` floats on), the tail (160), the count (one float); floats between the planes of a pair; the row stride */
int cruse_stream_df_layout(int* out);
/* after cruse_stream_decode: drain = 0: every slot whose mode computes a frame (FRAME, FRAME0, END) takes its work row; drain = 1:
 * every slot whose mode is END takes an all-zero row, which emits the clip's last row E[T-1].  df_work[S][dw_stride] (dw_stride >=
 * 322): E re | im of the slot's step; out[S][160] */
int cruse_stream_df_head(const int* mode, int S, int drain, const float* work, int wk_stride, int wk_re, int wk_im, int wk_mask,
                         const float* tab, float* df_state, int st_stride, float* df_work, int dw_stride, void* out, int out_fmt,
                         const float* lim, int* clip, int t_dim, int f_dim, void* stream);
/* after cruse_stream_decode_n: the same step for the frames of the slot's packet, in order (the frame set cruse_stream_decode_n
 * derives from pk).  df_work[S][dw_frames][322]: one row per emitted E, from index 0; out[S][out_hops][160]: the emitted blocks in
 * order from index 0 (E[0]'s is not among them) */
int cruse_stream_df_head_n(const int* pk, int S, int hops, int out_hops, int work_frames, const float* work, int wk_stride, int wk_re,
                           int wk_im, int wk_mask, const float* tab, float* df_state, int st_stride, float* df_work, int dw_frames,
                           void* out, int out_fmt, const float* lim, int* clip, int t_dim, int f_dim, void* stream);

/* ---- per-slot level meters and voice activity on the stream (additive; csrc/stream_meter.hip) ---------------
 * One more kernel at the end of a chain tells the caller what the server heard, frame by frame, without reading a block back: the level
 * of the input, the level of the enhanced output and an energy voice-activity decision on the enhanced frame.  On the device they
 * replace the reference's host numpy code utils/utils.py:143-183 (activitydetector: log-energy -> logistic -> attack / release smoothing
 * -> threshold), :82-103 (active_rms: the level over active windows only) and :37-41 (normalize, which a stream cannot do: level_db is
 * absolute and per slot).  The kernels follow cruse_stream_decode / _decode_n and read nothing but what the chain leaves in a frame's
 * work row: the noisy spectrum N (161 floats at wk_re, 161 at wk_im) and the raw mask m (160 at wk_mask), rows wk_stride floats apart.
 * Per computed frame:
 *   G_f    the decode kernels' gain: pf(m_f) on bins 0..159 and 0 on bin 160; with lim: lim[s] + (1 - lim[s]) pf(m_f), and lim[s] on bin
 *          160.  pf is the post-filter pf_kind (1 iam, 2 envelope) with tau pf_tau[s]; the identity where pf_kind == 0 or tau == 0.
 *   P_in   (|N_0|^2 + 2 sum_{f=1..159} |N_f|^2 + |N_160|^2) / (320 W2), W2 the sum of the squared window of tab (cruse_stream_tables);
 *          P_out the same of G_f N_f;  L = 10 log10(P + 1e-12) dBFS
 *   p      p_prev + alpha (p_raw - p_prev), p_raw = 1 / (1 + exp(-(L_out - level_db))), alpha = attack where p_raw > p_prev else release
 *   vad    p > threshold
 * vad_par[S][4] (device, f32): level_db, threshold, attack, release per slot.  A frame writes the meter row [L_in, L_out, p, vad] (f32;
 * vad 0.0 / 1.0) and adds to meter_acc[S][4] (device, f64): frames, active frames (vad = 1), the sums of P_in and of P_out over active
 * frames.  meter_state[S][st_stride] (device, f32; st_stride >= the stride of cruse_stream_meter_layout) holds p_prev.  The frame 0 of a
 * clip (mode FRAME0; a packet's first frame where pk says the slot held at most one block) resets p_prev and the accumulators whatever
 * they held, takes part in the recursion and writes no row and no count: its block lies in front of the clip.  A slot that computes no
 * frame leaves its rows, state and accumulators untouched.  One workgroup per slot, f32 sums in one fixed order in both forms, no
 * atomics: a frame has the same bits from either entry point.  Refused with CRUSE_E_SHAPE before any launch: S < 1, a null buffer
 * (lim may be null; pf_tau may be null where pf_kind == 0), wk_re / wk_im / wk_mask that do not lie in a row of wk_stride floats or a row
 * shorter than 161 + 161 + 160, a pf_kind other than 0, 1, 2, st_stride or the out rows too small, hops outside [1, 64],
 * work_frames < hops + 1, out_hops < hops. */
#define CRUSE_STREAM_METER_LAYOUT_INTS 4
/* out[CRUSE_STREAM_METER_LAYOUT_INTS] (HOST array): the offset of p_prev in a meter_state row, the row stride (floats), the doubles of a
 * meter_acc row, the floats of a meter row */
int cruse_stream_meter_layout(int* out);
/* after cruse_stream_decode: every slot whose mode computes a frame (FRAME, FRAME0, END) takes its work row; the row of slot s goes to
 * out + s * out_stride (out_stride >= 4 floats) */
int cruse_stream_meter(const int* mode, int S, const float* work, int wk_stride, int wk_re, int wk_im, int wk_mask, const float* tab,
                       const float* lim, int pf_kind, const float* pf_tau, const float* vad_par, float* meter_state, int st_stride,
                       double* meter_acc, float* out, int out_stride, void* stream);
/* after cruse_stream_decode_n: the same for the frames of the slot's packet, in order (the frame set cruse_stream_decode_n derives from
 * pk); the rows of slot s go to out + s * out_stride from index 0, aligned with its output blocks (out_stride >= 4 out_hops floats) */
int cruse_stream_meter_n(const int* pk, int S, int hops, int out_hops, int work_frames, const float* work, int wk_stride, int wk_re,
                         int wk_im, int wk_mask, const float* tab, const float* lim, int pf_kind, const float* pf_tau,
                         const float* vad_par, float* meter_state, int st_stride, double* meter_acc, float* out, int out_stride,
                         void* stream);

/* ---- what a boundary entry point launches (additive; host-only: nothing is launched) ---------------------------------------------
 * Runs entry point `entry` (encode, decode, the DeepFilter head: 14 in all) up to its launch.  ints (HOST): its int arguments in its own
 * order; bit i of null_mask: its i-th pointer argument is null (pointers are only compared with null).  Returns the entry point's refusal
 * (code and cruse_last_error()), else CRUSE_OK and out[CRUSE_STREAM_PLAN_INTS] (HOST): [0] kernel family (0 encode, 2 decode, 4 df_head;
 * + 1 for _n)  [1] DEC (1: upsample levels)  [2] s16  [3] LIM  [4] PF  [5] grid x  [6] block x  [7] dynamic LDS bytes  [8] floats of a
 * frame's work row, [9] of an LDS row, [10] of the LDS staging area (the last three: 0 for a single hop and for the head) */
enum { CRUSE_STREAM_ENTRY_ENCODE, CRUSE_STREAM_ENTRY_ENCODE_IO, CRUSE_STREAM_ENTRY_DECODE, CRUSE_STREAM_ENTRY_DECODE_IO,
       CRUSE_STREAM_ENTRY_DECODE_PF, CRUSE_STREAM_ENTRY_DECODE_UP, CRUSE_STREAM_ENTRY_ENCODE_N, CRUSE_STREAM_ENTRY_ENCODE_N_IO,
       CRUSE_STREAM_ENTRY_DECODE_N, CRUSE_STREAM_ENTRY_DECODE_N_IO, CRUSE_STREAM_ENTRY_DECODE_N_PF, CRUSE_STREAM_ENTRY_DECODE_N_UP,
       CRUSE_STREAM_ENTRY_DF_HEAD, CRUSE_STREAM_ENTRY_DF_HEAD_N, CRUSE_STREAM_ENTRY_N };
#define CRUSE_STREAM_PLAN_INTS 11
int cruse_stream_boundary_plan(int entry, const int* ints, int null_mask, int* out);

/* ---- validation metrics on the device (ABI 13, additive; csrc/metrics.hip) -------------------------------------------------------
 * The two closed-form metrics of train_base/metrics.py, scored per clip of a batch ref[B][L], est[B][L] (f32) into out[B] (f32).
 * Every sum runs in a fixed order and there are no atomics: a result is bit-identical from run to run, and a clip scores the same
 * alone and inside a batch.  Refused with CRUSE_E_SHAPE before any HIP call: a null buffer, B < 1, L < 1, L > 2^28. */
/* SI_SDR (train_base/metrics.py:60-82): alpha = <ref, est> / <ref, ref>, p = alpha ref, 10 log10(sum p^2 / sum (est - p)^2), the
 * three sums in f64.  One launch, one workgroup per clip, so no clip spans several workgroups and there is no second launch. */
int cruse_si_sdr(const float* ref, const float* est, int B, int L, float* out, void* stream);
/* Classic (non-extended) STOI of 16 kHz clips, as DESIGN.md section 13 defines it stage by stage (Taal et al. 2011; STOI of
 * train_base/metrics.py:85-86): 16 -> 10 kHz by a zero-phase 257-tap polyphase FIR, removal of the frames of ref more than 40 dB under
 * its loudest, 512-point spectra of 256-sample Hann frames in 15 third-octave bands, clipped and normalised correlation over all
 * 30-frame segments.  A clip that keeps fewer than 31 frames scores 1e-5.  Bounds: B <= 65535, L <= 2^28 and a workspace below 8 GiB
 * (CRUSE_E_SHAPE beyond).  Six launches at most, none waited for by the host: the call captures into a HIP graph.
 * cruse_stoi_layout: out[CRUSE_STOI_LAYOUT_INTS] (HOST array) = L10 (10 kHz samples per clip), nF (frames before removal), nGs (row
 * stride of tob, max(nF - 1, 1)), nSB (segment blocks per band), then the workspace offsets in 4-byte units of the stage arrays
 * x10 [B][2][L10] f32 (ref, est at 10 kHz), e [B][max(nF,1)] f32 (frame energies of ref in dB), nk [B] int (kept frames), kept
 * [B][max(nF,1)] int (their indices, ascending; nk[b] valid), tob [B][2][15][nGs] f32 (band magnitudes; nk[b] - 1 valid per row),
 * part [B][15][nSB] f64 (block partial sums), and the workspace size in the same units. */
#define CRUSE_STOI_LAYOUT_INTS 11
int cruse_stoi_layout(int B, int L, int* out);
/* bytes of device workspace of cruse_stoi(B, L); 0 where cruse_stoi_layout refuses the shape */
size_t cruse_stoi_ws_bytes(int B, int L);
/* tab[1540] (device) <- prototype taps h[257] at 0, window hanning(258)[1:-1] at 260, cos / sin(2 pi j / 512) at 516 / 1028, built in
 * double on the host and rounded once; synchronises `stream` */
int cruse_stoi_tables(float* tab, void* stream);
/* ws: 8-byte aligned (CRUSE_E_ALIGN), ws_bytes >= cruse_stoi_ws_bytes(B, L) (CRUSE_E_SHAPE); its contents need no initialisation */
int cruse_stoi(const float* ref, const float* est, int B, int L, const float* tab, void* ws, size_t ws_bytes, float* out, void* stream);
/* Ragged batches and extended STOI (additive).  ref, est [B][L] as above; len: int[B] on the DEVICE, read by the
 * kernels only and never by the host, so a captured graph replays with whatever lengths the array then holds.  Clip b is scored as the
 * clip ref[b][0 : n], n = len[b] clamped to [0, L]: no sample at an index >= n is loaded (the padding may hold anything), the STOI
 * stages use the clip's own L10 = (5 n + 7) / 8 and nF, and a clip scores bit for bit what cruse_si_sdr / cruse_stoi give it alone at
 * L = n.  n = 0: SI-SDR NaN (0 / 0), STOI 1e-5.  extended != 0 scores ESTOI (Jensen & Taal 2016): stages 1 - 3 unchanged, then per
 * 30-frame segment the 15 x 30 band matrices of ref and est, rows then columns less their mean and over (norm + 2^-52), no clipping;
 * the segment scores sum(X^ Y^) / 30, the clip the mean over its segments (1e-5 without one).  Workspace, tables, bounds, refusals
 * and the six launches are cruse_stoi's; a null len is refused too (CRUSE_E_SHAPE), all before any HIP call. */
int cruse_si_sdr_ragged(const float* ref, const float* est, int B, int L, const int* len, float* out, void* stream);
int cruse_stoi_ragged(const float* ref, const float* est, int B, int L, const int* len, int extended, const float* tab, void* ws,
                      size_t ws_bytes, float* out, void* stream);
/* bss_eval SDR of one source (additive; csrc/sdr.hip): SDR of train_base/metrics.py:55-57, which is
 * mir_eval.separation.bss_eval_sources(reference[None, :], estimation[None, :]) -- the estimate may be any K-tap time-invariant
 * filtering of the reference before anything counts as error.  Per clip of n samples (n = len[b] clamped to [0, L]; len null: n = L;
 * len is an int[B] DEVICE array that only the kernels read) and K taps, 1 <= K <= CRUSE_SDR_MAX_TAPS (bss_eval_sources uses 512):
 *   raa[k] = sum_i ref[i] ref[i+k], rab[k] = sum_i ref[i] est[i+k], 0 <= k < K, samples outside [0, n) zero;  toeplitz(raa) C = rab;
 *   s[m] = sum_k C[k] ref[m-k], e[m] = est[m] - s[m] (est zero from n on), 0 <= m < n + K - 1;  out[b] = 10 log10(sum s^2 / sum e^2).
 * f32 in, every product, sum, the solve (Levinson) and the projection in f64, out f32.  out[b] = NaN, and nothing faults, for n = 0, an
 * all-zero ref, or a solve that meets a non-positive r[0] / prediction error (mir_eval raises or falls back to lstsq there).  No sample
 * at an index >= n is loaded; the order of every sum follows from n and K alone, no atomics: a clip scores bit for bit the same alone,
 * in a batch and from run to run.  Four launches, none waited for by the host: the call captures into a HIP graph.
 * ws: cruse_sdr_ws_bytes(B, L, K) bytes (0 where the shape is refused), 8-byte aligned (CRUSE_E_ALIGN), no initialisation needed.
 * dbg (nullable, 8-byte aligned): per clip 3 K + 2 doubles: raa[K], rab[K], C[K] (NaN without a solution), sum s^2, sum e^2.
 * The correlations are summed per chunk of CRUSE_SDR_CHUNK samples and the chunks in ascending order.  Refused with CRUSE_E_SHAPE before
 * any HIP call: null ref / est / ws / out, B < 1 or > 65535, L < 1 or > 2^28, K < 1 or > CRUSE_SDR_MAX_TAPS. */
#define CRUSE_SDR_CHUNK 2048
#define CRUSE_SDR_MAX_TAPS 1024
size_t cruse_sdr_ws_bytes(int B, int L, int K);
int cruse_sdr(const float* ref, const float* est, const int* len, int B, int L, int K, void* ws, float* out, double* dbg, void* stream);

/* ---- biquad cascade over whole clips (ABI 13, additive; csrc/biquad.hip) -----------------------------------
 * The lfilter under the reference's EQ augmentation (train_base/acoustics/audioAug.py:149-178; torchaudio.functional.lfilter there).
 * x, y [B][L] f32, contiguous.  coef: S sections of (b0, b1, b2, a0, a1, a2) in FLOAT64 (device), [B][S][6] with coef_stride = 6 S or
 * one shared [S][6] with coef_stride = 0 (cruse_fir_causal's hs convention); 8-byte aligned (CRUSE_E_ALIGN).  One section is
 * scipy.signal.lfilter(b / a0, [1, a1 / a0, a2 / a0], x) from a zero state, evaluated in float64; with clamp != 0 its output is then
 * clipped to [-1, 1] (lfilter's clamp=True) before it enters the next section -- never inside a section's feedback.  What one
 * section hands the next stays float64; the last output is rounded once to f32.
 * One launch, one workgroup per clip; a lane holds CRUSE_BIQUAD_CHUNK consecutive samples, a workgroup CRUSE_BIQUAD_TILE, and a longer
 * clip goes through tiles in order inside its workgroup.  No allocation, no host synchronisation, no host read of coef (the call
 * captures into a HIP graph); results are bit-identical from run to run.  Refused with CRUSE_E_SHAPE before any HIP call: B < 1,
 * L < 1, L > 2^30, S < 1, S > 8, a null x / coef / y, a coef_stride other than 0 or 6 S. */
#define CRUSE_BIQUAD_CHUNK 32
#define CRUSE_BIQUAD_TILE 32768
/* bytes of device workspace of cruse_biquad_cascade(B, L, S): 0, no clip leaves its workgroup (ws may then be null).  Host only. */
size_t cruse_biquad_ws_bytes(int B, int L, int S);
int cruse_biquad_cascade(const float* x, const double* coef, int coef_stride, int B, int L, int S, int clamp, void* ws, float* y,
                         void* stream);

/* ---- FFT convolution with a bank of filters (ABI 13, additive; csrc/fftconv.hip) ---------------------------
 * y[b][n] = sum_{k < R, k <= n} h[f(b)][k] x[b][n - k], n < L: scipy.signal.fftconvolve(x, h)[:L], the room-impulse-response step of
 * SynDataset.snr_mix (dataset/dataset.py:244-247) and both convolutions of SynDataset.add_reverb (:226-228), by uniformly partitioned
 * overlap-save convolution in f32.  Optionally y_early[b][n] = the same sum over k < early_len[f(b)]: add_reverb's
 * fftconvolve(cln_wav, rir[:et]) (:221, :228), from the same input spectra.
 * Partitions of CRUSE_FFTCONV_PART samples, transforms of twice that.  One spectrum is CRUSE_FFTCONV_PART complex f32 values (bins
 * 1 .. PART - 1, and the real bins 0 and PART together in bin 0) = 8 PART bytes.
 *   spec: [1 or 2][NR][npart] spectra, npart = ceil(R / PART); the second half holds the early filters.
 *   ws:   [B][nblk] spectra, nblk = ceil(L / PART); needs no initialisation, holds the input spectra after the call.
 * x, y, y_early [B][L] f32 and h [NR][R] f32, contiguous; spec and ws 8-byte aligned (CRUSE_E_ALIGN).  No atomics and one summation
 * order: results are bit-identical from run to run and a clip convolves the same alone and inside a batch.  No allocation, no host
 * synchronisation, no host read of a device buffer: the calls capture into a HIP graph.  Refused with CRUSE_E_SHAPE before any HIP
 * call, cruse_last_error naming the argument: a null x / h / spec / ws / y, B, L, NR or R < 1, L or R > 2^30, NR > 65535 (prepare),
 * B * nblk > 2^31 - 1, NR neither 1 nor B with a null h_index, spec_bytes or ws_bytes too small. */
#define CRUSE_FFTCONV_PART 2048
/* bytes of a prepared bank (early != 0: with the early spectra) and of the input-spectrum workspace; 0 for a size < 1.  Host only. */
size_t cruse_fftconv_spec_bytes(int NR, int R, int early);
size_t cruse_fftconv_ws_bytes(int B, int L);
/* spec <- the spectra of the zero-padded partitions of h[NR][R]; with early_len (int32 [NR] on the device, may be NULL) also those of
 * every filter cut to its first clamp(early_len[r], 0, R) taps (0: a silent early output).  One launch. */
int cruse_fftconv_prepare(const float* h, int NR, int R, const int* early_len, void* spec, size_t spec_bytes, void* stream);
/* f(b) = h_index[b] (int32 [B] on the device); with h_index NULL, b if NR == B and 0 if NR == 1 (cruse_fir_causal's two cases).  A
 * clip whose index is negative -- or >= NR, which the host cannot know -- passes through: y[b] (and y_early[b]) are x[b] bit for bit
 * and its transforms are skipped.  y_early may be NULL; not NULL, spec must hold the early spectra.  Out of place.  Two launches. */
int cruse_fftconv_apply(const float* x, int B, int L, const void* spec, size_t spec_bytes, int NR, int R, const int* h_index, void* ws,
                        size_t ws_bytes, float* y, float* y_early, void* stream);
/* y[b] = x[b] * (1 / (max |ref[b]| + eps)): the scale SynDataset.snr_mix gives the speech (dataset/dataset.py:251), applied to
 * another tensor -- the early-reflection target beside the reverberant speech that sets the peak.  x, ref, y [B][L], out of place. */
int cruse_peak_scale(const float* x, const float* ref, int B, int L, float eps, float* y, void* stream);

/* ---- recordings -> training clips (ABI 13, additive; csrc/resample.hip) ------------------------------------
 * cruse_resample_poly: one launch converts a ragged batch of B recordings at one source rate to the rate of the pools.  (up, down) is
 * (dst_rate, src_rate) REDUCED, q = max(up, down), taps: the N = 32 q + 1 low-pass taps h (cruse_amd/resample_design.py: the Kaiser
 * design of cruse_stream_resample_*, unit DC gain) laid out phase-major, table[p][j] = h[p + up j] (0 beyond N), up rows of tap_stride
 * floats, tap_stride a multiple of 4 >= ceil(N / up), 16-byte aligned (CRUSE_E_ALIGN).  With v[up i] = x[i], zero elsewhere and
 * outside the clip,
 *     y[n] = up * sum_k h[k] v[n down + 16 q - k],   0 <= n < Lout = ceil(L up / down)
 * = scipy.signal.resample_poly(x, up, down, window=h): zero-phase, zero-padded edges.  f32 fmaf over k ascending from 0, no atomics:
 * bit-identical from run to run, and a clip gives the same samples alone and inside a batch.
 * src: fmt 0 = f32 mono (channels = 1) or fmt 1 = int16 PCM interleaved; clip b is the frames [off_in[b], off_in[b + 1]) and sample i
 * of it is src[(off_in[b] + i) * channels + chan] (/ 32768.0f for PCM, exact).  out: f32; clip b fills [off_out[b], off_out[b + 1])
 * and every sample of [off_out[0], off_out[B]) is written exactly once.  off_in / off_out: int64 [B + 1] on the DEVICE; the same
 * arrays on the HOST as off_in_host / off_out_host, which size the grid and are judged here -- the kernel trusts the device copies.
 * up = down = 1: the conversion / de-interleave alone, y = x bit for bit; taps may be NULL.
 * One launch, no allocation, no host synchronisation (the call captures into a HIP graph).  Refused with CRUSE_E_SHAPE before any
 * HIP call: a null buffer, B < 1, up or down outside 1..1024 or not reduced, an unknown fmt, channels outside 1..1024, chan outside
 * 0..channels-1, f32 with channels != 1, ntap != 32 q + 1, a tap_stride too small or no multiple of 4, a negative first offset, a clip
 * with L < 1 or L, Lout > 2^31 - 1025, Lout != ceil(L up / down) (non-monotone offsets included), offsets beyond 2^50. */
#define CRUSE_RESAMPLE_TILE 1024
int cruse_resample_poly(const void* src, int fmt, int channels, int chan, const long long* off_in_host, const long long* off_out_host,
                        const long long* off_in, const long long* off_out, int B, int up, int down, const float* taps, int ntap,
                        int tap_stride, float* out, void* stream);
/* cruse_assemble_clips: out[b][dst + j] = pool[src + j] for j < len over the segments seg_first[b] .. seg_first[b + 1] - 1 of clip b, and
 * 0.0f everywhere else (silence gaps): SynDataset._select_clean_y / _select_noise_y (dataset/dataset.py:147-203) as a gather.  pool: flat
 * f32; out [B][L] f32, every sample written exactly once; seg: int64 [nseg][3] rows (src, dst, len), per clip ascending in dst and
 * non-overlapping inside [0, L); seg_first: int32 [B + 1]; both on the device.  The device validates nothing: the plan is judged on
 * the host from the arrays it was built from (cruse_amd.ops.check_clip_plan).  One launch, capturable.  Refused with CRUSE_E_SHAPE
 * before any HIP call: a null pool / seg_first / out, a null seg with nseg > 0, B < 1, L < 1, L > 2^31 - 1025, nseg < 0. */
int cruse_assemble_clips(const float* pool, const long long* seg, const int* seg_first, int nseg, int B, int L, float* out, void* stream);

/* ---- grouped linears and band pooling (ABI 14, additive; csrc/grouped_linear.hip) ----------------------------
 * G independent linears over the feature slices of x [rows][G Ig]: group g maps columns [g Ig, (g + 1) Ig) to Hg outputs with
 * w[g w_sg + i w_si + j w_so] (element strides, all >= 1), so one kernel serves GroupedLinearEinsum's weight [G][Ig][Hg]
 * (model/based_model/cust_conv.py:517-522, :536; strides (Ig Hg, Hg, 1)) and the stacked nn.Linear weights [G][Hg][Ig] of
 * GroupedLinear (:565-573; strides (Hg Ig, 1, Ig)).  bias [G Hg] (group-major, nullable), then ReLU if relu != 0.  Output j of group g
 * goes to column g Hg + j (CRUSE_GL_CAT: the flatten of :537, the cat of :574) or, CRUSE_GL_SHUFFLED, to where GroupedLinear's
 * view(-1, Hg, G).transpose(-1, -2) (:575-578) moves it: with c = g Hg + j, column (c % G) Hg + c / G -- applied in the store index.
 * Exact f32 (v_mfma_f32_16x16x4_f32), no atomics, one summation order: bit-identical from run to run.  No allocation, no host
 * synchronisation (the calls capture into a HIP graph).  Any rows, Ig, Hg >= 1: fragments are padded with zeros in registers and
 * nothing is read or written outside x, w, bias, y.  Refused with CRUSE_E_SHAPE before any HIP call: a null x / w / y / dy / dx / dw,
 * rows, G, Ig or Hg < 1, rows > 2^30, G Ig or G Hg >= 2^31, a stride < 1, an unknown out_map, G * ceil(max(Ig, Hg) / 64) > 65535,
 * relu != 0 with a null y (backward), a workspace that is missing or too small. */
#define CRUSE_GL_CAT 0
#define CRUSE_GL_SHUFFLED 1
int cruse_grouped_linear_fwd(const float* x, const float* w, long long w_sg, long long w_si, long long w_so, const float* bias, int rows,
                             int G, int Ig, int Hg, int relu, int out_map, float* y, void* stream);
/* dx [rows][G Ig] = (dy under the ReLU mask y > 0 when relu != 0; dy and y in the forward's column map) times the groups' weights
 * transposed.  One launch. */
int cruse_grouped_linear_bwd_dx(const float* dy, const float* y, const float* w, long long w_sg, long long w_si, long long w_so, int rows,
                                int G, int Ig, int Hg, int relu, int out_map, float* dx, void* stream);
/* dw[g w_sg + i w_si + j w_so] = sum over rows of x[row][g Ig + i] dy'[row][g, j], db[g Hg + j] = sum over rows of dy'[row][g, j]
 * (db nullable), dy' = dy under the ReLU mask; both are WRITTEN, not added to.  One launch covers all groups; when the rows are
 * split over parts (a function of the shape alone) every part writes its own slab of ws and a second launch adds the slabs in
 * ascending order of the part.  ws: cruse_grouped_linear_dw_ws_bytes() bytes (0: ws may be null), needs no initialisation. */
size_t cruse_grouped_linear_dw_ws_bytes(int rows, int G, int Ig, int Hg);
int cruse_grouped_linear_bwd_dw(const float* dy, const float* y, const float* x, int rows, int G, int Ig, int Hg, int relu, int out_map,
                                float* dw, long long w_sg, long long w_si, long long w_so, float* db, void* ws, size_t ws_bytes,
                                void* stream);
/* The products with erb_fb_use's matrices (model/based_model/cust_conv.py:187-207) as sums over contiguous bands.  starts: int32
 * [n_bands + 1] on the device, band b = bins [starts[b], starts[b + 1]); the kernels clamp every entry into [0, F] and never touch
 * memory outside a row whatever the table holds (a bin no band covers expands to 0).  w_b = 1 / width_b if mean != 0, else 1.
 *   cruse_band_pool:   y[r][b] = w_b sum_{f in band b} x[r][f]      x [rows][F]       -> y [rows][n_bands]   (x @ fb, :197-206)
 *   cruse_band_expand: y[r][f] = w_b(f) m[r][b(f)]                  m [rows][n_bands] -> y [rows][F]         (m @ fb.t(), :200-203)
 * Each is the other's adjoint at the same `mean`, so each is the other's backward.  One pass, f32 adds in ascending f and one
 * multiply, 16-byte accesses on the [rows][F] side when its base is 16-byte aligned (a block holds 4 rows, which start on a 16-byte
 * boundary for any F).  One launch, capturable.  Refused with CRUSE_E_SHAPE before any HIP call: a null pointer, rows outside
 * 1..2^30, F outside 1..CRUSE_BAND_MAX_F, n_bands outside 1..F. */
#define CRUSE_BAND_MAX_F 2048
int cruse_band_pool(const float* x, const int* starts, int rows, int F, int n_bands, int mean, float* y, void* stream);
int cruse_band_expand(const float* m, const int* starts, int rows, int F, int n_bands, int mean, float* y, void* stream);

/* ---- per-file statistics of a pool of recordings (ABI 15, additive; csrc/screen.hip) ---------------------------
 * What the reference's list builder (dataset/preprocess_dataset.py:118-153) needs to reject a file; its four tests are stubs set to 0
 * there (:130-133).  pool: flat f32 on the device (filepairs.load_pool); utterance i is pool[start[i] .. start[i] + len[i]); start, len:
 * int64 [n] on the device, start arbitrary (no alignment assumed), len >= 0.  The device validates neither: the tables are judged on the
 * host from the arrays they were uploaded from (cruse_amd.ops.ragged_plan).  No sample outside an utterance is loaded.  Every sum is
 * f64 in an order that follows from the tables alone, no atomics: bit-identical from run to run.  No allocation, no host synchronisation,
 * no host read of a device buffer: the calls capture into a HIP graph.  ws needs no initialisation.
 *
 * cruse_screen_clips -> out f64 [n][6] = peak = max |x| (train_base/acoustics/feature.py:106-107 is_clipped's operand), n_clipped =
 * #{|x| > clip_thr} compared in f32 (:107; is_clipped = n_clipped > 0), rms = sqrt(mean x^2) (:100 tailor_dB_FS), n_windows =
 * ceil(len / window), n_active, activity = n_active / n_windows (:194-236 activity_detector's perc_active, line for line in f64):
 *     scalar = 10^(target_db / 20) / (rms + 1e-6)                        (:101; the scaling of :102 is folded into the window sums)
 *     e_w = 20 log10(scalar^2 S_w + 1e-6), S_w = the window's sum of x^2  (:221)
 *     p_w = 1 / (1 + exp(-(-1 + 0.2 e_w)))                               (:222)
 *     smoothed_w = 0.8 p_w + 0.2 p_{w-1} if p_w > p_{w-1} else 0.05 p_w + 0.95 p_{w-1}, p_{-1} = 0     (:224-227, :231)
 *     active where smoothed_w > act_thr                                  (:229)
 * The smoother reads the UNSMOOTHED p of the window before (:231), so windows are independent.  len = 0: the row 0, 0, 0, 0, 0, NaN.
 * win_first: int64 [n + 1] on the device, the exclusive prefix of ceil(len / window), win_first[n] = total_windows (the host's sum: it
 * sizes the grid).  Two launches: one wavefront per window reads its samples once and writes one row of CRUSE_SCREEN_WS_ROW bytes of
 * ws; one workgroup per utterance finishes.  ws: cruse_screen_ws_bytes(n, total_windows) bytes.
 *
 * cruse_rt60 -> out f64 [n][3] = rt60 in seconds, t_peak = t0 = the first index of max |h|, edc_floor_db = D at the last sample:
 *     E[t] = sum_{m >= t} h[m]^2, t >= t0 (Schroeder's backward integral);  D[t] = 10 log10(E[t] / E[t0])
 *     t_lo = t0 + #{t : D[t] > lo_db}, t_hi = t0 + #{t : D[t] > hi_db}    (E does not rise, so the counts are the crossings)
 *     slope = least-squares slope of D on t over [t_lo, t_hi), t centred on the range's midpoint;  rt60 = -60 / (slope sr)
 * lo_db = -5, hi_db = -25 is T20 of ISO 3382-2.  This stands where utils/utils.py:270-320 cal_rt60 stands in the reference; that
 * function cannot run (stats.Linregress, :314) and its band mask zeroes every bin below hifreq (:292-293), so its 15 third-octave
 * bands, 2500-sample smoothing and median are NOT restated: the quantity here is broadband.  rt60 = NaN, nothing faults: len = 0 (all
 * three NaN), an all-zero response, fewer than 2 points in the range, a decay that never reaches hi_db, len > max_len.  One launch, one
 * workgroup per response; E is rebuilt chunk by chunk (CRUSE_RT60_CHUNK samples) from per-chunk suffix sums kept in ws:
 * cruse_rt60_ws_bytes(n, max_len) bytes, max_len >= every len.
 *
 * Refused with CRUSE_E_SHAPE before any launch, cruse_last_error naming the argument: n < 0, window < 1 or > 2^30, total_windows < 0 or
 * > CRUSE_SCREEN_MAX_WINDOWS, max_len < 0 or > CRUSE_RT60_MAX_LEN, sr < 1, lo_db <= hi_db, a null pointer; CRUSE_E_ALIGN: pool not
 * 4-byte, a table, ws or out not 8-byte aligned.  The two _ws_bytes return -1 for a shape the calls refuse.  n = 0 launches nothing. */
#define CRUSE_SCREEN_MAX_WINDOWS 2147483647LL
#define CRUSE_SCREEN_WS_ROW 16
#define CRUSE_RT60_CHUNK 2048
#define CRUSE_RT60_MAX_LEN 16777216
long long cruse_screen_ws_bytes(int n, long long total_windows);
int cruse_screen_clips(const float* pool, const long long* start, const long long* len, const long long* win_first, int n,
                       long long total_windows, int window, float clip_thr, double target_db, double act_thr, void* ws, double* out,
                       void* stream);
long long cruse_rt60_ws_bytes(int n, int max_len);
int cruse_rt60(const float* pool, const long long* start, const long long* len, int n, int max_len, int sr, double lo_db, double hi_db,
               void* ws, double* out, void* stream);

/* ---- multi-resolution spectral loss (cruse_amd/csrc/mrspec.hip) --------------------------------------------------
 * MultResSpecLoss of test/test_loss.py:193-229 (with Stft :140-165 and angle :232-243; its two one-token repairs: torch.zeros() -> a
 * scalar zero, save_for_backend -> save_for_backward) on waveforms est, ref [B,L] f32:
 *     loss = sum_r factor * mean (|Y|^g - |S|^g)^2 + f_complex[r] * mean |(|Y|^g e^{i arg Y}) - (|S|^g e^{i arg S})|^2
 * Y = STFT_N(est), S = STFT_N(ref) as torch.stft(n_fft = N, hop = N / 4, periodic Hann, center = True (reflect), normalized = True,
 * onesided) for every N of n_ffts (HOST array of R values, each a power of two in [CRUSE_MRSPEC_MIN_N, CRUSE_MRSPEC_MAX_N]); |.| is clamped
 * at 1e-12 before the power unless gamma == 1, where the terms are (|Y| - |S|)^2 and |Y - S|^2.  f_complex: HOST array of R weights or
 * NULL (no complex term).  loss (device, f64[1]) receives the value; dest (device [B,L], or NULL: evaluation, the inverse half is
 * skipped) receives grad_scale * dloss/dest as torch autograd gives it on that code (angle.backward's clamp_min(1e-10) on |x|^2,
 * clamp_min's zero gradient below 1e-12, abs's zero gradient at 0): est == ref and all-zero inputs give loss 0 and an all-zero gradient,
 * nothing is ever NaN or Inf.  No gradient wrt ref.
 * Deterministic (owner computes, no float atomics); R + 2 launches on `stream` (R + 1 without dest), no allocation, no synchronisation,
 * capturable.  ws: cruse_mrspec_ws_bytes(B, L, n_ffts, R) bytes, 256-byte aligned, laid out as
 *     | f64 loss partial sums, resolution after resolution: B * runs_r each | up to a multiple of 256 bytes |
 *     | f32 padded gradients [B, L + N_r] per resolution, each rounded up to a multiple of 256 bytes |
 * with runs_r = ceil((L + N_r) / (hops(N_r) * N_r / 4)) and hops(128 .. 2048) = 29, 13, 13, 9, 8.
 * Refused with CRUSE_E_SHAPE before any device call, cruse_last_error naming the argument and its value: a null est, ref, ws or loss;
 * B < 1 or > CRUSE_MRSPEC_MAX_B; R outside 1..CRUSE_MRSPEC_MAX_R; an N that is not such a power of two; L <= max N / 2 (reflect padding)
 * or > 2^30; B * L > 2^36; gamma <= 0; ws_bytes too small.  cruse_mrspec_ws_bytes returns 0 for a shape the call refuses. */
#define CRUSE_MRSPEC_MIN_N 128
#define CRUSE_MRSPEC_MAX_N 2048
#define CRUSE_MRSPEC_MAX_R 8
#define CRUSE_MRSPEC_MAX_B 65535
size_t cruse_mrspec_ws_bytes(int B, int L, const int* n_ffts, int R);
int cruse_mrspec_loss(const float* est, const float* ref, int B, int L, const int* n_ffts, int R, float gamma, float factor,
                      const float* f_complex, void* ws, size_t ws_bytes, double* loss, float* dest, float grad_scale, void* stream);

/* ---- DeepFilterNet's normalised input features (ABI 15, additive; csrc/df_feat.hip) ---------------------------------
 * The spectrum is two f32 planes re, im of B clips, T frames and F bins: element (b, t, f) sits at ((b T + t) frame_stride + f bin_stride)
 * of each.  Planar [B,T,F] planes are (1, F); re = x, im = x + 1 of an interleaved [B,T,F,2] tensor are (2, 2 F): neither is copied.
 * ERB feature (nb_erb > 0; band j = bins [starts[j], starts[j + 1]) of width w_j, starts: int32 [nb_erb + 1] on the device, every entry
 * clamped into [0, F] by the kernel, an empty band has mean power 0):
 *     e[t,j] = 10 log10((1 / w_j) sum_f (re^2 + im^2) + log_eps)          DeepFilterNet's published front end (not in the reference)
 *     m[t,j] = e[t,j] (1 - alpha) + alpha m[t-1,j],  m[-1] = erb_state     test/test_erb.py:104
 *     feat_erb[t,j] = (e[t,j] - m[t,j]) / erb_scale                        :105-106 REPAIRED: the reference starts out_xs from zeros, not
 *                                                                          from xs, and so returns -state / 40
 * Complex feature (nb_df > 0, bins f < nb_df), ExponentialUnitNorm.forward line for line (test/test_norm.py:52-61):
 *     a[t,f] = sqrt(max(re^2 + im^2, unit_eps))                            :54-55
 *     s[t,f] = a[t,f] (1 - alpha) + alpha s[t-1,f],  s[-1] = unit_state    :59
 *     feat_spec[t,f] = (re, im) / sqrt(s[t,f])                             :61
 * (band_unit_norm's norm(x) (1 - alpha + s alpha), test_erb.py:116, is a misplaced parenthesis and is not restated.)
 * erb_state [B, nb_erb] and unit_state [B, nb_df] are read as the state before frame 0 and overwritten with the state after frame T - 1;
 * feat_erb [B,T,nb_erb]; feat_spec [B,T,nb_df,2] interleaved, 8-byte aligned.  nb_erb = 0 / nb_df = 0 skips that feature: its pointers
 * may be null and nothing of it is read or written.
 * alpha is a double because the reference's line 59 multiplies by the Python scalars alpha and 1 - alpha, each rounded to f32 on its own:
 * 1 - (float)alpha is off by up to 1e-6 of 1 - alpha at alpha = 0.99.  Split invariance: with alpha_f = (float)alpha and oma =
 * (float)(1 - alpha) rounded on the host, every step is, in f32 with no contraction other than the fma written here (alpha there is
 * alpha_f) and correctly rounded sqrt and division,
 *     p = re re + im im (two products, one add);  mean = (p_lo + p_lo+1 + ... added in ascending f from 0) * (1 / w_j)
 *     e = 10 * log10f(mean + log_eps);  m = fma(alpha, m, e * oma);  feat_erb = (e - m) / erb_scale
 *     a = sqrt(max(p, unit_eps));       s = fma(alpha, s, a * oma);  feat_spec = re / sqrt(s), im / sqrt(s)
 * so the values of frame t and the states depend on the incoming state and the frames up to t alone, never on T or on where a frame
 * falls in the kernel's tiles of CRUSE_DF_FEAT_TC frames: one call over T frames and calls over T1 + T2 + ... frames with the state
 * carried write the same bits, down to one frame per call.  No atomics, no workspace, one launch, no synchronisation: capturable.
 * An all-zero spectrum gives feat_spec = 0 and a finite feat_erb from any non-negative state (unit_eps > 0 keeps s > 0).
 * T = 0 writes nothing, leaves the states and returns CRUSE_OK.  Refused before any launch, cruse_last_error naming the argument
 * (CRUSE_E_SHAPE): B < 1, T < 0, F outside 1..CRUSE_BAND_MAX_F; nb_erb or nb_df outside 0..F, or both 0; alpha outside [0, 1) (NaN
 * included); log_eps or unit_eps < 0, erb_scale 0; a null re or im, a null starts / state / output of a requested feature; bin_stride
 * < 1, frame_stride < (F - 1) bin_stride + 1; B * T > 2^31.  CRUSE_E_ALIGN: feat_spec not 8-byte aligned.  Whether starts covers
 * [0, F] is judged on the host where the table is built (cruse_amd _band_table). */
#define CRUSE_DF_FEAT_TC 64
int cruse_df_feat(const float* re, const float* im, long long bin_stride, long long frame_stride, int B, int T, int F, const int* starts,
                  int nb_erb, int nb_df, double alpha, float log_eps, float erb_scale, float unit_eps, float* erb_state, float* unit_state,
                  float* feat_erb, float* feat_spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CRUSE_HIP_H */
