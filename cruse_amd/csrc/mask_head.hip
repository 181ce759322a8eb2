// The mask head of the training step in ONE launch: last decoder BatchNorm (bn2_t) + ReLU + skip -> u_1, the 1x3 stride-2 transposed
// conv to one channel + sigmoid -> mask, WO-MALE against the clean magnitude -> loss, dL/dlogit, and the data gradient of that conv
// du_1 = W^T dlogit with the backward sums of bn2_t.  It replaces, on the main stream,
//
//     bn_fin_act_fwd_kernel -> conv_scatter2_kernel<1> -> cruse_zero -> mask_loss_kernel -> conv_gather_kernel<4> -> bn_act_bwd_reduce_kernel
//
// which write u_1, the mask, dlogit and du_1 to HBM and read each of them (and v_2 twice more) straight back.  Here a workgroup keeps a
// tile of MH_TF whole frames of one clip: u_1 and dlogit go through LDS, v_2 stays in the registers that loaded it.  The conv has KT = 1:
// no time halo.  Every per-element expression is the one of the kernel it replaces (same operands, same order), so the tensors come out
// bit-identical; only the three atomic sums (loss, sum g, sum g*xhat) are formed in another order (the backward sums with every addend in f64).
//
// Which products of those expressions the compiler fuses into an FMA is its choice, and it differs from kernel to kernel (the
// scatter conv's are not fused at all).  This file therefore turns contraction off and spells every FMA of the replaced kernels
// out with fmaf(), as read from their gfx950 code.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MH_TF = 8;            // frames per tile
constexpr int MH_THREADS = 256;
constexpr int MH_NI = 5;            // float4 items per thread and tile: MH_TF * C * F1 / 4 <= MH_NI * MH_THREADS
constexpr int MH_CMAX = 16;
constexpr int MH_MAX_BLOCKS = 4096;

struct MaskHeadArgs {
    const float* v; const double* sums; int nrep; double inv_count, unb; float eps, momentum;
    const float* gamma; const float* beta; const float* skip; const float* w; const float* bias;
    const float* nre; const float* nim; const float* cmag;
    int B, T, C, F1, Fs; float alpha, beta_l;
    float* u; float* mean_o; float* rstd_o; float* rmean; float* rvar; float* mask; float* dlogit; float* du;
    double* loss_sum; double* bwd_sums; int bwd_nrep;
};

// one WO-MALE term (mask_loss_kernel's expressions): returns w * |d|, dm = d term / d mask
__device__ __forceinline__ float wo_male_term(const float m, const float re, const float im, const float mag_ref, const float alpha,
                                              const float beta, const float inv_n, float& dm) {
    const float inv_ln10 = 0.43429448190325176f;
    const float er = m * re, ei = m * im;
    const float mag_est = sqrtf(fmaf(er, er, ei * ei));
    const float mag_unp = sqrtf(fmaf(re, re, im * im));
    const float iam = mag_ref / mag_unp;
    const float w = expf(alpha / (beta + iam));
    const float d = log10f(mag_est + 1.f) - log10f(mag_ref + 1.f);
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    dm = w * sgn * inv_ln10 / (mag_est + 1.f) * mag_unp * inv_n;
    return w * fabsf(d);
}

__global__ __launch_bounds__(MH_THREADS) void mask_head_kernel(MaskHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float tab[4][MH_CMAX];
    __shared__ float wl[MH_CMAX * 3];
    __shared__ double s_stat[2][MH_CMAX];
    __shared__ double sred[MH_THREADS / 64];
    const int tid = threadIdx.x;
    const int C = a.C, F1 = a.F1, CF = C * F1, VPR = CF >> 2, F1P = F1 + 4, Fn = 2 * F1, FnP = Fn + 8, Fs = a.Fs;
    float* ul = smem + 4;                                    // u_1 tile [MH_TF][C][F1P] (4 floats in front: the m - 1 read of the first row)
    float* dl = ul + MH_TF * C * F1P;                        // dlogit tile [MH_TF][FnP], columns Fn, Fn + 1 zero (the gather's right pad)
    double* part = reinterpret_cast<double*>(smem);          // [2][MH_TF * VPR] backward partials; reuses the u_1 tile once the mask is out

    // BatchNorm finalise: the arithmetic of bn_fin_act_fwd_kernel; block 0 publishes and updates the running statistics
    if (tid < C) {
        const int c = tid;
        double t1 = 0.0, t2 = 0.0;
        for (int r = 0; r < a.nrep; ++r) { t1 += a.sums[(long long)r * 2 * C + c]; t2 += a.sums[(long long)r * 2 * C + C + c]; }
        const double m = t1 * a.inv_count;
        double var = fma(t2, a.inv_count, -(m * m));
        if (var < 0.0) var = 0.0;
        const float mf = (float)m, rs = (float)(1.0 / sqrt(var + (double)a.eps));
        tab[0][c] = mf; tab[1][c] = rs; tab[2][c] = a.gamma[c]; tab[3][c] = a.beta[c];
        if (blockIdx.x == 0) {
            a.mean_o[c] = mf; a.rstd_o[c] = rs;
            if (a.rmean) {
                a.rmean[c] = (float)fma((double)a.momentum, m, (1.0 - a.momentum) * a.rmean[c]);
                a.rvar[c] = (float)fma(a.momentum * var, a.unb, (1.0 - a.momentum) * a.rvar[c]);
            }
        }
    }
    if (tid < 3 * C) wl[tid] = a.w[tid];                     // conv1_t.weight [C][1][1][3]
    const float bv = a.bias ? a.bias[0] : 0.f;
    const long long rows = (long long)a.B * a.T;
    const float inv_n = (float)(1.0 / (double)(rows * Fs));
    const int ntile_t = (a.T + MH_TF - 1) / MH_TF;
    const long long ntiles = (long long)a.B * ntile_t;
    // loss: f32 runs of up to 32 terms per thread, then f64 -- mask_loss_kernel's scheme.  The f64 additions of such partials (24-bit values of
    // similar size) are exact, so the sum does not depend on the order of the atomics: the loss is the same from run to run
    double lacc = 0.0;
    float lpart = 0.f;
    int lcnt = 0;

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / ntile_t), t0 = (int)(tile % ntile_t) * MH_TF;
        const int nfr = min(MH_TF, a.T - t0);
        const long long row0 = (long long)b * a.T + t0;
        const int nitem = nfr * VPR;
        __syncthreads();                                     // the tables; the previous tile's LDS reads
        if (tid < 2 * MH_CMAX) (&s_stat[0][0])[tid] = 0.0;

        // ---- u_1 = relu(bn(v_2)) + skip_1: float4 per item, all loads first; v_2 stays in registers for the backward sums
        float4 vv[MH_NI], ss[MH_NI];
#pragma unroll
        for (int k = 0; k < MH_NI; ++k) {
            const int i = tid + k * MH_THREADS;
            if (i < nitem) {
                vv[k] = *reinterpret_cast<const float4*>(a.v + row0 * CF + (long long)i * 4);
                ss[k] = *reinterpret_cast<const float4*>(a.skip + row0 * CF + (long long)i * 4);
            } else { vv[k] = make_float4(0.f, 0.f, 0.f, 0.f); ss[k] = vv[k]; }
        }
#pragma unroll
        for (int k = 0; k < MH_NI; ++k) {
            const int i = tid + k * MH_THREADS;
            if (i < nitem) {
                const int r = i / VPR, j = (i - r * VPR) * 4, c = j / F1, f = j - c * F1;      // F1 % 4 == 0: the four share c
                const float pm = tab[0][c], pr = tab[1][c], pg = tab[2][c], pb = tab[3][c];
                const float in[4] = {vv[k].x, vv[k].y, vv[k].z, vv[k].w}, sk[4] = {ss[k].x, ss[k].y, ss[k].z, ss[k].w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = fmaf((in[e] - pm) * pr, pg, pb);
                    t = fmaxf(t, 0.f);
                    o[e] = t + sk[e];
                }
                const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(a.u + row0 * CF + (long long)i * 4) = o4;
                *reinterpret_cast<float4*>(ul + (r * C + c) * F1P + f) = o4;
            }
        }
        __syncthreads();

        // ---- mask = sigmoid(convT(u_1) + bias) (conv_scatter2_kernel<1>: outputs 2m, 2m + 1 from u[m], u[m - 1]), WO-MALE, dL/dlogit.
        // Item m == F1 of a frame is spectrum bin Fs - 1, which the network does not cover: mask 0, a loss term, no gradient
        const int F1e = F1 + 1;
        for (int q = tid; q < nfr * F1e; q += MH_THREADS) {
            const int r = q / F1e, m = q - r * F1e;
            const long long grow = row0 + r;
            if (m < F1) {
                float acc0 = bv, acc1 = bv;
                for (int cs = 0; cs < C; ++cs) {
                    const float* up = ul + (r * C + cs) * F1P + m;
                    const float g0 = up[0], gm1 = m > 0 ? up[-1] : 0.f;
                    const float w0 = wl[cs * 3], w1 = wl[cs * 3 + 1], w2 = wl[cs * 3 + 2];
                    acc0 += w0 * g0 + w2 * gm1;              // (three roundings each: no FMA in the scatter kernel)
                    acc1 += w1 * g0;
                }
                const float m0 = sigmoid_acc(acc0), m1 = sigmoid_acc(acc1);
                *reinterpret_cast<float2*>(a.mask + grow * Fn + 2 * m) = make_float2(m0, m1);
                const long long i0 = grow * Fs + 2 * m;
                float dm0, dm1;
                const float l0 = wo_male_term(m0, a.nre[i0], a.nim[i0], a.cmag[i0], a.alpha, a.beta_l, inv_n, dm0);
                const float l1 = wo_male_term(m1, a.nre[i0 + 1], a.nim[i0 + 1], a.cmag[i0 + 1], a.alpha, a.beta_l, inv_n, dm1);
                lpart += l0;
                lpart += l1;
                lcnt += 2;
                const float2 dd = make_float2(dm0 * m0 * (1.f - m0), dm1 * m1 * (1.f - m1));
                *reinterpret_cast<float2*>(a.dlogit + grow * Fn + 2 * m) = dd;
                *reinterpret_cast<float2*>(dl + r * FnP + 2 * m) = dd;
            } else {
                const long long i0 = grow * Fs + Fn;
                float dm0;
                lpart += wo_male_term(0.f, a.nre[i0], a.nim[i0], a.cmag[i0], a.alpha, a.beta_l, inv_n, dm0);
                lcnt += 1;
                *reinterpret_cast<float2*>(dl + r * FnP + Fn) = make_float2(0.f, 0.f);
            }
        }
        if (lcnt >= 32) { lacc += (double)lpart; lpart = 0.f; lcnt = 0; }
        __syncthreads();

        // ---- du_1[c, fo] = sum_kf W[c][kf] dlogit[2 fo + kf] (conv_gather_kernel<4> at Cin = 1, S = 2, pad 0) for the four elements the
        // item loaded, and their share of the bn2_t backward sums (bn_act_bwd_reduce_kernel's g and g * xhat, each added in f64)
#pragma unroll
        for (int k = 0; k < MH_NI; ++k) {
            const int i = tid + k * MH_THREADS;
            if (i < MH_TF * VPR) {
                double d1 = 0.0, d2 = 0.0;
                if (i < nitem) {
                    const int r = i / VPR, j = (i - r * VPR) * 4, c = j / F1, f = j - c * F1;
                    const float pm = tab[0][c], pr = tab[1][c], pg = tab[2][c], pb = tab[3][c];
                    const float w0 = wl[c * 3], w1 = wl[c * 3 + 1], w2 = wl[c * 3 + 2];
                    const float* xp = dl + r * FnP + 2 * f;
                    const float4 xa = *reinterpret_cast<const float4*>(xp), xb = *reinterpret_cast<const float4*>(xp + 4);
                    const float2 xc = *reinterpret_cast<const float2*>(xp + 8);
                    const float xs[10] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w, xc.x, xc.y};
                    const float in[4] = {vv[k].x, vv[k].y, vv[k].z, vv[k].w};
                    float o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x0 = xs[2 * e], x1 = xs[2 * e + 1], x2 = xs[2 * e + 2];
                        float acc = 0.f;                         // (the gather kernel's bias-less start: -0 becomes +0)
                        acc += fmaf(w2, x2, fmaf(w0, x0, w1 * x1));
                        o[e] = acc;
                        const float xh = (in[e] - pm) * pr;
                        float gr = acc;
                        if (!(fmaf(xh, pg, pb) > 0.f)) gr = 0.f;
                        d1 += (double)gr;
                        d2 += (double)(gr * xh);
                    }
                    *reinterpret_cast<float4*>(a.du + row0 * CF + (long long)i * 4) = make_float4(o[0], o[1], o[2], o[3]);
                }
                part[i] = d1; part[MH_TF * VPR + i] = d2;
            }
        }
        __syncthreads();
        // one thread per (sum, frame, channel) folds the channel's F1 / 4 partials in order; MH_TF adds per LDS cell, one atomic per
        // cell and tile into the tile's replica
        {
            const int per = F1 >> 2;
            for (int s = tid; s < 2 * MH_TF * C; s += MH_THREADS) {
                const int which = s / (MH_TF * C), rem = s - which * (MH_TF * C), r = rem / C, c = rem - r * C;
                const double* p = part + which * (MH_TF * VPR) + r * VPR + c * per;
                double t = 0.0;
                for (int j = 0; j < per; ++j) t += p[j];
                atomicAdd(&s_stat[which][c], t);
            }
        }
        __syncthreads();
        if (tid < 2 * C) {
            const int which = tid / C, c = tid - which * C;
            atomicAdd(a.bwd_sums + (size_t)(tile % a.bwd_nrep) * 2 * C + which * C + c, s_stat[which][c]);
        }
    }
    lacc += (double)lpart;
    lacc = wave_sum_d(lacc);
    if ((tid & 63) == 0) sred[tid >> 6] = lacc;
    __syncthreads();
    if (tid == 0) atomicAdd(a.loss_sum, sred[0] + sred[1] + sred[2] + sred[3]);
}

}  // namespace

extern "C" int cruse_mask_head_fwd_bwd(const float* v, const double* bn_sums, int sum_replicas, float eps, float momentum,
                                       const float* gamma, const float* beta, const float* skip, const float* w, const float* bias,
                                       const float* nre, const float* nim, const float* cmag,
                                       int B, int T, int C, int F1, int Fs, float loss_alpha, float loss_beta,
                                       float* u, float* mean, float* rstd, float* running_mean, float* running_var,
                                       float* mask, float* dlogit, float* du, double* loss_sum, int loss_zeroed,
                                       double* bwd_sums, int bwd_replicas, int bwd_zeroed, int max_blocks, void* stream) {
    CRUSE_REQUIRE(B > 0 && T > 0 && C > 0 && F1 > 0, CRUSE_E_SHAPE, "mask_head: empty shape B=%d T=%d C=%d F1=%d", B, T, C, F1);
    CRUSE_REQUIRE(C <= MH_CMAX && F1 % 4 == 0 && MH_TF * C * F1 / 4 <= MH_NI * MH_THREADS && Fs == 2 * F1 + 1, CRUSE_E_SHAPE,
                  "mask_head: C=%d (<= %d), F1=%d (multiple of 4, C*F1 <= %d), Fs=%d (2*F1 + 1)", C, MH_CMAX, F1,
                  MH_NI * MH_THREADS * 4 / MH_TF, Fs);
    CRUSE_REQUIRE(v && bn_sums && gamma && beta && skip && w && nre && nim && cmag && u && mean && rstd && mask && dlogit && du && loss_sum && bwd_sums,
                  CRUSE_E_SHAPE, "mask_head: a tensor is NULL");
    CRUSE_REQUIRE(sum_replicas >= 1 && bwd_replicas >= 1 && max_blocks >= 0, CRUSE_E_SHAPE, "mask_head: replicas %d / %d, max_blocks %d",
                  sum_replicas, bwd_replicas, max_blocks);
    CRUSE_REQUIRE((running_mean == nullptr) == (running_var == nullptr), CRUSE_E_SHAPE, "mask_head: the running statistics come in pairs");
    CRUSE_REQUIRE(((uintptr_t)v % 16 | (uintptr_t)skip % 16 | (uintptr_t)u % 16 | (uintptr_t)du % 16 | (uintptr_t)mask % 8 | (uintptr_t)dlogit % 8) == 0,
                  CRUSE_E_ALIGN, "mask_head: v, skip, u, du must be 16-byte aligned, mask and dlogit 8-byte aligned");
    CRUSE_REQUIRE((((uintptr_t)bn_sums | (uintptr_t)loss_sum | (uintptr_t)bwd_sums) & 7) == 0, CRUSE_E_ALIGN,
                  "mask_head: bn_sums, loss_sum and bwd_sums must be 8-byte aligned (f64 accesses)");
    hipStream_t st = (hipStream_t)stream;
    if (!loss_zeroed) { int rc = cruse_zero_async(loss_sum, sizeof(double), st, "mask_head loss memset"); if (rc) return rc; }
    if (!bwd_zeroed) { int rc = cruse_zero_async(bwd_sums, 2 * (size_t)C * bwd_replicas * sizeof(double), st, "mask_head sums memset"); if (rc) return rc; }
    const long long count = (long long)B * T * F1;
    MaskHeadArgs a{v, bn_sums, sum_replicas, 1.0 / (double)count, count > 1 ? (double)count / (double)(count - 1) : 1.0, eps, momentum,
                   gamma, beta, skip, w, bias, nre, nim, cmag, B, T, C, F1, Fs, loss_alpha, loss_beta,
                   u, mean, rstd, running_mean, running_var, mask, dlogit, du, loss_sum, bwd_sums, bwd_replicas};
    const long long ntiles = (long long)B * cdiv(T, MH_TF);
    const int cap = max_blocks > 0 ? max_blocks : MH_MAX_BLOCKS;
    const int grid = (int)(ntiles < cap ? ntiles : cap);
    const size_t lds = (size_t)(4 + MH_TF * C * (F1 + 4) + MH_TF * (2 * F1 + 8)) * sizeof(float);
    hipLaunchKernelGGL(mask_head_kernel, dim3(grid), dim3(MH_THREADS), lds, st, a);
    CRUSE_LAUNCH_CHECK("mask_head");
    return CRUSE_OK;
}
