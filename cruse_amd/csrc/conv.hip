// Frame-major direct convolutions for the CRUSE encoder / decoder / skip paths.
//
// Replaces nn.Conv2d((2,3),(1,2),(1,1)) + causal crop, nn.Conv2d((1,3)) skip and
// nn.ConvTranspose2d((1,3),(1,2)) + crop of model/cruse_net.py:138-143,149-164 and
// their autograd backward.  Activations are [B,T,C,F]: one row of C*F (= 640 at every
// U-Net level) floats per frame, so every global access is a contiguous frame row.
//
// Round-1 form: f32 VALU, weights + a tile of frames staged in LDS, register tiles
// of CO_T output channels x TT frames per thread.  HBM-bound in principle
// (2 x 640 floats per frame per layer); see DESIGN.md for the roofline.
#include "common.h"

namespace {

constexpr int TF = 8;        // frames per workgroup tile
constexpr int TT = 4;        // frames per thread item
constexpr int NSET = TF / TT;
constexpr int CONV_THREADS = 320;

struct ConvArgs {
    const float* x; const float* w; const float* bias; float* y;
    int B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, act, accum;
    double* sums;            // gather form only: BatchNorm batch sums of y ([2][Cout]) accumulated by the epilogue, or null
};

__device__ __forceinline__ float apply_act(float v, int act) {
    return act == 1 ? sigmoid_acc(v) : v;
}

// Stage `nrows` frame rows ([Cin][Fin] floats each, frames t_first .. of clip b; zero outside the clip) into LDS rows
// [Cin][Fin + 2] with a zero column on either side.  float4 global loads, several in flight per thread before the
// first LDS store (the element-wise loop it replaces issued one 4-byte load per iteration and waited for it: 16
// serialised HBM round trips per workgroup on the 8 -> 1 decoder layer, 59 us for a kernel that moves 82 MB).
__device__ __forceinline__ void stage_rows(float* xl, const float* x, int b, int t_first, int nrows, int Cin, int Fin, int T,
                                           int tid) {
    const int FinP = Fin + 2, rowraw = Cin * Fin, rowlen = Cin * FinP;
    for (int i = tid; i < nrows * Cin; i += CONV_THREADS) {          // the pad columns
        xl[i * FinP] = 0.f;
        xl[i * FinP + Fin + 1] = 0.f;
    }
    if ((Fin & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
        constexpr int SV = 4;
        const int nvec = nrows * rowraw / 4;
        for (int base = 0; base < nvec; base += CONV_THREADS * SV) {
            float4 v[SV];
            int rr[SV];
#pragma unroll
            for (int q = 0; q < SV; ++q) {
                const int i = base + tid + q * CONV_THREADS;
                v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                rr[q] = 0;
                if (i < nvec) {
                    const int r = (i * 4) / rowraw;
                    const int t = t_first + r;
                    rr[q] = r;
                    if (t >= 0 && t < T)
                        v[q] = *reinterpret_cast<const float4*>(x + ((long long)b * T + t) * rowraw + (i * 4 - r * rowraw));
                }
            }
#pragma unroll
            for (int q = 0; q < SV; ++q) {
                const int i = base + tid + q * CONV_THREADS;
                if (i < nvec) {
                    const int j = i * 4 - rr[q] * rowraw;
                    const int ci = j / Fin, f = j - ci * Fin;            // Fin % 4 == 0: the four elements share ci
                    float* d = xl + rr[q] * rowlen + ci * FinP + 1 + f;
                    d[0] = v[q].x; d[1] = v[q].y; d[2] = v[q].z; d[3] = v[q].w;
                }
            }
        }
    } else {
        for (int i = tid; i < nrows * rowraw; i += CONV_THREADS) {
            const int r = i / rowraw, j = i - r * rowraw;
            const int ci = j / Fin, f = j - ci * Fin;
            const int t = t_first + r;
            xl[r * rowlen + ci * FinP + 1 + f] = (t >= 0 && t < T) ? x[((long long)b * T + t) * rowraw + j] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// gather form
// ---------------------------------------------------------------------------
template <int CO_T>
__global__ __launch_bounds__(CONV_THREADS) void conv_gather_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int FinP = a.Fin + 2;                 // [left zero][Fin][right zero]
    const int nrows = TF + a.KT - 1;            // LDS frame 0 <-> t0-(KT-1)
    const int K3 = a.Cin * a.KT * 3;
    float* wl = smem;                           // [K3][Cout]
    float* xl = smem + ((K3 * a.Cout + 3) & ~3); // [nrows][Cin][FinP]
    const int tid = threadIdx.x;
    const int ntile = (a.T + TF - 1) / TF;
    const int b = blockIdx.x / ntile;
    const int t0 = (blockIdx.x % ntile) * TF;
    // f64 cells: adding f32-valued partials in f64 is exact, so the result does not depend on the order of the atomics
    // (f32 cells made the batch mean vary by an ulp from run to run -- enough to flip a ReLU decision sitting on it)
    __shared__ double s_stat[2][64];
    if (a.sums && tid < 128) (&s_stat[0][0])[tid] = 0.0;        // ordered by the staging barrier below

    // stage weights: wl[(ci*KT+kt)*3+kf][co]
    for (int i = tid; i < K3 * a.Cout; i += CONV_THREADS) {
        const int co = i % a.Cout;
        const int k = i / a.Cout;
        const int kf = k % 3, kt = (k / 3) % a.KT, ci = k / (3 * a.KT);
        float v;
        if (a.w_layout == 0) v = a.w[((co * a.Cin + ci) * a.KT + kt) * 3 + kf];
        else v = a.w[(ci * a.Cout + co) * 3 + (2 - kf)];
        wl[i] = v;
    }
    // stage input frames (zero outside the clip and in the pad columns)
    stage_rows(xl, a.x, b, t0 - (a.KT - 1), nrows, a.Cin, a.Fin, a.T, tid);
    __syncthreads();

    const int tpf = (a.Cout / CO_T) * a.Fout;
    // wave-uniform trip count (the statistics epilogue below uses wave reductions): lanes past the end idle
    for (int base = 0; base < NSET * tpf; base += CONV_THREADS) {
        const int item = base + tid;
        const bool valid = item < NSET * tpf;
        const int set = valid ? item / tpf : 0;
        const int o = valid ? item % tpf : 0;
        const int cq = o / a.Fout, fo = o % a.Fout;
        const int co0 = cq * CO_T;
        float st1[CO_T], st2[CO_T];
#pragma unroll
        for (int c = 0; c < CO_T; ++c) { st1[c] = 0.f; st2[c] = 0.f; }
        if (valid) {
        float acc[TT][CO_T];
#pragma unroll
        for (int c = 0; c < CO_T; ++c) {
            const float bv = a.bias ? a.bias[co0 + c] : 0.f;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt][c] = bv;
        }
        const int fbase = fo * a.S - a.pad + 1;
        for (int ci = 0; ci < a.Cin; ++ci) {
            for (int kt = 0; kt < a.KT; ++kt) {
                float wv[3][CO_T];
                const float* wp = wl + ((ci * a.KT + kt) * 3) * a.Cout + co0;
#pragma unroll
                for (int kf = 0; kf < 3; ++kf) {
                    if constexpr (CO_T == 4) {
                        const float4 q = *reinterpret_cast<const float4*>(wp + kf * a.Cout);
                        wv[kf][0] = q.x; wv[kf][1] = q.y; wv[kf][2] = q.z; wv[kf][3] = q.w;
                    } else {
#pragma unroll
                        for (int c = 0; c < CO_T; ++c) wv[kf][c] = wp[kf * a.Cout + c];
                    }
                }
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    const float* xp = xl + ((set * TT + tt + kt) * a.Cin + ci) * FinP + fbase;
                    const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
#pragma unroll
                    for (int c = 0; c < CO_T; ++c)
                        acc[tt][c] += wv[0][c] * x0 + wv[1][c] * x1 + wv[2][c] * x2;
                }
            }
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const int t = t0 + set * TT + tt;
            if (t >= a.T) continue;
#pragma unroll
            for (int c = 0; c < CO_T; ++c) {
                const long long idx = (((long long)b * a.T + t) * a.Cout + co0 + c) * a.Fout + fo;
                float v = acc[tt][c];
                if (a.accum) v += a.y[idx]; else v = apply_act(v, a.act);
                a.y[idx] = v;
                st1[c] += v; st2[c] += v * v;
            }
        }
        }   // valid
        if (a.sums) {
            // a wave's 64 consecutive items span at most a few channel groups: one wave reduction (fixed order) per
            // group present, then ONE lane adds the group's 2 x CO_T sums to the LDS cells.  (Every lane adding its own
            // values made 320 threads queue on 16 cells: 95 us for the 1 -> 8 layer against 53 without statistics.)
            unsigned long long left = __ballot(1);
            while (left) {
                const int lead = __ffsll((long long)left) - 1;
                const int key = __shfl(cq, lead, 64);
                const bool mine = cq == key;
                float r1[CO_T], r2[CO_T];
#pragma unroll
                for (int c = 0; c < CO_T; ++c) { r1[c] = wave_sum(mine ? st1[c] : 0.f); r2[c] = wave_sum(mine ? st2[c] : 0.f); }
                if ((int)(threadIdx.x & 63) == lead) {
#pragma unroll
                    for (int c = 0; c < CO_T; ++c) {
                        atomicAdd(&s_stat[0][key * CO_T + c], (double)r1[c]);
                        atomicAdd(&s_stat[1][key * CO_T + c], (double)r2[c]);
                    }
                }
                left &= ~__ballot(mine);
            }
        }
    }
    if (a.sums) {       // Cout <= 64 (host-checked): 8 frames x Fout values per channel in f32, then one f64 atomic each
        __syncthreads();
        if (tid < 2 * a.Cout) {
            const int which = tid / a.Cout, co = tid - which * a.Cout;
            atomicAdd(a.sums + (size_t)(blockIdx.x % CRUSE_BN_STAT_REPLICAS) * 2 * a.Cout + which * a.Cout + co, s_stat[which][co]);
        }
    }
}

// ---------------------------------------------------------------------------
// scatter form, frequency stride 2 (outputs handled as (2m, 2m+1) pairs)
// ---------------------------------------------------------------------------
template <int CO_T>
__global__ __launch_bounds__(CONV_THREADS) void conv_scatter2_kernel(ConvArgs a) {
    // here: Cin = Cs (summed channels), Fin = Fg, Fout = 2*Fg
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int FgP = a.Fin + 2;
    const int nrows = TF + a.KT - 1;            // LDS frame 0 <-> t0
    const int K3 = a.Cin * a.KT * 3;
    float* wl = smem;                           // [K3][Cout]
    float* gl = smem + ((K3 * a.Cout + 3) & ~3);
    const int tid = threadIdx.x;
    const int ntile = (a.T + TF - 1) / TF;
    const int b = blockIdx.x / ntile;
    const int t0 = (blockIdx.x % ntile) * TF;

    for (int i = tid; i < K3 * a.Cout; i += CONV_THREADS) {
        const int co = i % a.Cout;
        const int k = i / a.Cout;               // (cs*KT+kt)*3+kf
        const int cs = k / (3 * a.KT), rem = k % (3 * a.KT);
        wl[i] = a.w[(cs * a.Cout + co) * (a.KT * 3) + rem];
    }
    stage_rows(gl, a.x, b, t0, nrows, a.Cin, a.Fin, a.T, tid);
    __syncthreads();

    const int Fg = a.Fin;
    const int tpf = (a.Cout / CO_T) * Fg;
    for (int item = tid; item < NSET * tpf; item += CONV_THREADS) {
        const int set = item / tpf;
        const int o = item % tpf;
        const int cq = o / Fg, m = o % Fg;
        const int co0 = cq * CO_T;
        float acc0[TT][CO_T], acc1[TT][CO_T];   // fo = 2m, 2m+1
#pragma unroll
        for (int c = 0; c < CO_T; ++c) {
            const float bv = a.bias ? a.bias[co0 + c] : 0.f;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) { acc0[tt][c] = bv; acc1[tt][c] = bv; }
        }
        for (int cs = 0; cs < a.Cin; ++cs) {
            for (int kt = 0; kt < a.KT; ++kt) {
                float wv[3][CO_T];
                const float* wp = wl + ((cs * a.KT + kt) * 3) * a.Cout + co0;
#pragma unroll
                for (int kf = 0; kf < 3; ++kf)
#pragma unroll
                    for (int c = 0; c < CO_T; ++c) wv[kf][c] = wp[kf * a.Cout + c];
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    const int r = set * TT + tt + (a.KT - 1) - kt;
                    const float* gp = gl + (r * a.Cin + cs) * FgP + m;   // gp[0]=g[m-1], gp[1]=g[m], gp[2]=g[m+1]
                    const float gm1 = gp[0], g0 = gp[1], gp1 = gp[2];
                    if (a.pad == 0) {
#pragma unroll
                        for (int c = 0; c < CO_T; ++c) {
                            acc0[tt][c] += wv[0][c] * g0 + wv[2][c] * gm1;
                            acc1[tt][c] += wv[1][c] * g0;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < CO_T; ++c) {
                            acc0[tt][c] += wv[1][c] * g0;
                            acc1[tt][c] += wv[0][c] * gp1 + wv[2][c] * g0;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const int t = t0 + set * TT + tt;
            if (t >= a.T) continue;
#pragma unroll
            for (int c = 0; c < CO_T; ++c) {
                const long long idx = (((long long)b * a.T + t) * a.Cout + co0 + c) * a.Fout + 2 * m;
                float v0 = acc0[tt][c], v1 = acc1[tt][c];
                if (a.accum) { v0 += a.y[idx]; v1 += a.y[idx + 1]; }
                else { v0 = apply_act(v0, a.act); v1 = apply_act(v1, a.act); }
                *reinterpret_cast<float2*>(a.y + idx) = make_float2(v0, v1);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
struct WgradArgs {
    const float* a; const float* bt; float* partial;
    int B, T, Ca, Fa, Cb, Fb, S, pad, ntiles_total;
};

constexpr int WG_THREADS = 256;

template <int CB_T, int KT>
__global__ __launch_bounds__(WG_THREADS) void conv_wgrad_kernel(WgradArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int CA_T = 4;
    constexpr int NACC = CA_T * CB_T * KT * 3;
    const int CaP = p.Ca + 4;                         // channel-fastest rows, 16B aligned
    const int CbP = (CB_T == 4) ? p.Cb + 4 : p.Cb;
    const int FbP = p.Fb + 2;
    const int nrowb = TF + KT - 1;
    float* al = smem;                                 // [TF][Fa][CaP]
    float* bl = smem + TF * p.Fa * CaP;               // [nrowb][FbP][CbP]
    const int tid = threadIdx.x;
    const int nta = p.Ca / CA_T, ntb = p.Cb / CB_T;
    const int NT = nta * ntb;
    const int ntile_t = (p.T + TF - 1) / TF;

    float acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.f;

    const int npos = TF * p.Fa;
    for (int tile = blockIdx.x; tile < p.ntiles_total; tile += gridDim.x) {
        const int b = tile / ntile_t;
        const int t0 = (tile % ntile_t) * TF;
        __syncthreads();
        for (int i = tid; i < TF * p.Ca * p.Fa; i += WG_THREADS) {
            const int fa = i % p.Fa, ca = (i / p.Fa) % p.Ca, r = i / (p.Fa * p.Ca);
            const int t = t0 + r;
            float v = 0.f;
            if (t < p.T) v = p.a[(((long long)b * p.T + t) * p.Ca + ca) * p.Fa + fa];
            al[(r * p.Fa + fa) * CaP + ca] = v;
        }
        for (int i = tid; i < nrowb * p.Cb * FbP; i += WG_THREADS) {
            const int fp = i % FbP, cb = (i / FbP) % p.Cb, r = i / (FbP * p.Cb);
            const int t = t0 - (KT - 1) + r;
            float v = 0.f;
            if (t >= 0 && t < p.T && fp >= 1 && fp <= p.Fb)
                v = p.bt[(((long long)b * p.T + t) * p.Cb + cb) * p.Fb + (fp - 1)];
            bl[(r * FbP + fp) * CbP + cb] = v;
        }
        __syncthreads();
        // work items: (tile-of-outputs, position); output tile fastest so a wave shares a position
        for (int w = tid; w < NT * npos; w += WG_THREADS) {
            const int ot = w % NT, pos = w / NT;
            const int ia = ot / ntb, ib = ot % ntb;
            const int r = pos / p.Fa, fa = pos % p.Fa;
            const float4 av = *reinterpret_cast<const float4*>(al + (r * p.Fa + fa) * CaP + ia * CA_T);
            const float a4[4] = {av.x, av.y, av.z, av.w};
            const int fb0 = fa * p.S - p.pad + 1;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
                for (int kf = 0; kf < 3; ++kf) {
                    const int fidx = fb0 + kf;
                    float bv[CB_T];
                    if (fidx >= 0 && fidx < FbP) {
                        const float* bp = bl + ((r + kt) * FbP + fidx) * CbP + ib * CB_T;
                        if constexpr (CB_T == 4) {
                            const float4 q = *reinterpret_cast<const float4*>(bp);
                            bv[0] = q.x; bv[1] = q.y; bv[2] = q.z; bv[3] = q.w;
                        } else {
                            bv[0] = bp[0];
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < CB_T; ++c) bv[c] = 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < CA_T; ++i)
#pragma unroll
                        for (int j = 0; j < CB_T; ++j)
                            acc[((i * CB_T + j) * KT + kt) * 3 + kf] += a4[i] * bv[j];
                }
            }
        }
    }
    // NOTE: with w = tid + n*256 and NT dividing 256 (or 256 dividing NT*k) a thread keeps the
    // same output tile for all its items only when 256 % NT == 0; the host guarantees that.
    __syncthreads();
    float* red = smem;                                   // [Ca*Cb*KT*3]
    const int nout = p.Ca * p.Cb * KT * 3;
    for (int i = tid; i < nout; i += WG_THREADS) red[i] = 0.f;
    __syncthreads();
    {
        const int ot = tid % NT;
        const int ia = ot / ntb, ib = ot % ntb;
#pragma unroll
        for (int i = 0; i < CA_T; ++i)
#pragma unroll
            for (int j = 0; j < CB_T; ++j)
#pragma unroll
                for (int k = 0; k < KT * 3; ++k) {
                    const int ca = ia * CA_T + i, cb = ib * CB_T + j;
                    atomicAdd(&red[(ca * p.Cb + cb) * (KT * 3) + k], acc[(i * CB_T + j) * (KT * 3) + k]);
                }
    }
    __syncthreads();
    for (int i = tid; i < nout; i += WG_THREADS) p.partial[(long long)blockIdx.x * nout + i] = red[i];
}

__global__ void wgrad_reduce_kernel(const float* partial, int nblk, int nout, float* dw) {
    // blockIdx.y owns a chunk of 16 partial slabs; one atomic per output and chunk
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nout) return;
    const int k0 = blockIdx.y * 16, k1 = min(nblk, k0 + 16);
    float s = 0.f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += partial[(long long)k * nout + i];
    atomicAdd(&dw[i], s);
}

// ---------------------------------------------------------------------------
// channel sum: out[c] += sum_{rows,f} g[row,c,f]
// ORDERED (a grid of one workgroup, few rows): no sum depends on the order in which atomics land -- a thread's column sum runs over
// the rows in ascending order, a channel's columns are added in ascending order by one thread, and out[c] receives one addend --
// so the result has the same bits from run to run.  Otherwise f32 atomics in LDS and across the grid's workgroups: the order is free.
// ---------------------------------------------------------------------------
template <bool ORDERED>
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* g, long long rows, int C, int F, int ld,
                                                          float* out) {
    // grid.x strides over rows; each thread owns a fixed column j of the C*F-wide row (row stride ld);
    // 4 independent accumulators keep 4 loads in flight per thread
    __shared__ float sacc[2048];
    [[maybe_unused]] __shared__ float scol[256];
    const int CF = C * F;
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) sacc[c] = 0.f;
    __syncthreads();
    const long long G = gridDim.x;
    for (int j0 = 0; j0 < CF; j0 += 256) {
        const int j = j0 + tid;
        if (j < CF) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            long long r = blockIdx.x;
            for (; r + 3 * G < rows; r += 4 * G) {
                s0 += g[r * ld + j]; s1 += g[(r + G) * ld + j]; s2 += g[(r + 2 * G) * ld + j]; s3 += g[(r + 3 * G) * ld + j];
            }
            for (; r < rows; r += G) s0 += g[r * ld + j];
            if constexpr (ORDERED) scol[tid] = (s0 + s1) + (s2 + s3);
            else atomicAdd(&sacc[j / F], (s0 + s1) + (s2 + s3));
        }
        if constexpr (ORDERED) {                // thread t: channel c_lo + t of the <= 256 channels that have columns in this chunk
            __syncthreads();
            const int j1 = min(j0 + 256, CF), c = j0 / F + tid;
            if (c <= (j1 - 1) / F) {
                float a = sacc[c];
                for (int k = max(c * F, j0); k < min((c + 1) * F, j1); ++k) a += scol[k - j0];
                sacc[c] = a;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) atomicAdd(&out[c], sacc[c]);
}

constexpr long long CHANNEL_SUM_ORDERED_ROWS = 64;      // cruse_channel_sum: at most this many rows run as one ordered workgroup

template <typename K>
int set_smem(K kern, size_t bytes, const char* name) {
    return cruse_ensure_dyn_lds(reinterpret_cast<const void*>(kern), bytes, name);
}

}  // namespace

extern "C" int cruse_bn_act_bwd_apply(const float* dout, const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                      const double* sums, int sum_replicas, long long rows, int C, int F, int relu, int training, int dout_dtype,
                                      void* dy, int dy_dtype, float* dgamma, float* dbeta, float* dbias, void* stream);
extern "C" int cruse_bn_act_bwd_reduce(const float* dout, const float* y, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, long long rows, int C, int F,
                                       int relu, double* sums, int zeroed, void* stream);

namespace {

// conv_run's "the fused BatchNorm-backward input was not taken": the caller runs the separate pass (conv_bnbwd_in)
constexpr int CONV_NOT_FUSED = 1;

// Operands on which a kernel of this path does 8- or 16-byte accesses without choosing a route from the address: refused when misaligned,
// ahead of every launch (the memset of the sums included).  x and the f32 gather output are not here: they select a route (stage_rows,
// cm_plan, launch_mt).  bn_y: the swapped-role MFMA forms and the VALU path's statistics pass read it in vectors.
int conv_aligned(const char* who, const CruseConvCall& c, const CruseBnBwd* bnb, const CruseBnIn* bni, const CruseBnBwdIn* bbi) {
    auto off = [](const void* p, unsigned m) { return ((uintptr_t)p & (m - 1)) != 0; };
    CRUSE_REQUIRE(!off(c.sums, 8), CRUSE_E_ALIGN, "%s: sums must be 8-byte aligned (f64 atomics)", who);
    CRUSE_REQUIRE(!(c.scatter && off(c.y, 8)), CRUSE_E_ALIGN, "%s: out must be 8-byte aligned (the scatter kernels store pairs)", who);
    CRUSE_REQUIRE(!(bnb && off(bnb->y, 16)), CRUSE_E_ALIGN, "%s: bn_y must be 16-byte aligned", who);
    CRUSE_REQUIRE(!(bni && off(bni->sums, 8)), CRUSE_E_ALIGN, "%s: in_sums must be 8-byte aligned (f64 loads)", who);
    CRUSE_REQUIRE(!(bni && off(bni->add, 16)), CRUSE_E_ALIGN, "%s: in_add must be 16-byte aligned", who);
    CRUSE_REQUIRE(!(bni && off(bni->copy_bf16, 16)), CRUSE_E_ALIGN, "%s: the bf16 copy must be 16-byte aligned", who);
    CRUSE_REQUIRE(!(bbi && off(bbi->sums, 8)), CRUSE_E_ALIGN, "%s: bb_sums must be 8-byte aligned (f64 loads)", who);
    CRUSE_REQUIRE(!(bbi && off(bbi->y, 16)), CRUSE_E_ALIGN, "%s: bb_y must be 16-byte aligned", who);
    CRUSE_REQUIRE(!(bbi && off(bbi->copy_bf16, 16)), CRUSE_E_ALIGN, "%s: dy_bf16 must be 16-byte aligned", who);
    return CRUSE_OK;
}

// The one host path of the ten entry points: validate, try the MFMA kernel, else the VALU kernel and the statistics pass it lacks.
// plan != null (cruse_conv_plan): decide the same way, write what would be launched and launch nothing.
// Where the two forms differ they branch on c.scatter; every such branch is behaviour, not an oversight.
int conv_run(const CruseConvCall& c, int* plan = nullptr) {
    const char* who = c.scatter ? "conv_scatter2" : "conv_gather";
    const char* cin = c.scatter ? "Cs" : "Cin";
    CRUSE_REQUIRE((c.x_dtype == CRUSE_DT_F32 || c.x_dtype == CRUSE_DT_BF16) && (c.y_dtype == CRUSE_DT_F32 || c.y_dtype == CRUSE_DT_BF16), CRUSE_E_DTYPE,
                  "%s: x_dtype %d / y_dtype %d (f32 or bf16)", who, c.x_dtype, c.y_dtype);
    if (c.scatter) {
        CRUSE_REQUIRE(c.B > 0 && c.T > 0 && c.Cin > 0 && c.Cout > 0 && c.Fin > 0, CRUSE_E_SHAPE, "conv_scatter2: empty shape");
        CRUSE_REQUIRE(c.Fout == 2 * c.Fin, CRUSE_E_SHAPE, "conv_scatter2: Fout=%d must be 2*Fg=%d", c.Fout, 2 * c.Fin);
        CRUSE_REQUIRE((c.KT == 1 || c.KT == 2) && (c.pad == 0 || c.pad == 1), CRUSE_E_SHAPE, "conv_scatter2: unsupported KT=%d pad=%d", c.KT, c.pad);
    } else {
        CRUSE_REQUIRE(c.B > 0 && c.T > 0 && c.Cin > 0 && c.Cout > 0 && c.Fin > 0 && c.Fout > 0, CRUSE_E_SHAPE,
                      "conv_gather: empty shape B=%d T=%d Cin=%d Cout=%d Fin=%d Fout=%d", c.B, c.T, c.Cin, c.Cout, c.Fin, c.Fout);
        CRUSE_REQUIRE((c.KT == 1 || c.KT == 2) && (c.S == 1 || c.S == 2) && (c.pad == 0 || c.pad == 1), CRUSE_E_SHAPE,
                      "conv_gather: unsupported KT=%d S=%d pad=%d", c.KT, c.S, c.pad);
        CRUSE_REQUIRE((c.Fout - 1) * c.S - c.pad + 2 <= c.Fin, CRUSE_E_SHAPE, "conv_gather: Fout=%d reads past Fin=%d (+1 zero column)", c.Fout, c.Fin);
        CRUSE_REQUIRE(c.w_layout == 0 || (c.KT == 1 && c.S == 1), CRUSE_E_SHAPE, "conv_gather: w_layout 1 needs KT=1,S=1");
    }
    CRUSE_REQUIRE(!(c.accum && c.act), CRUSE_E_SHAPE, "%s: accum with activation", who);
    if (const int arc = conv_aligned(who, c, c.bnb, c.bni, c.bbi)) return arc;
    if (plan) plan[CRUSE_CP_FUSED] = c.bbi != nullptr;
    if (c.prec >= 0) {
        const int r = cruse_conv_mfma_try(c, plan);
        if (r > 0 && plan) { plan[CRUSE_CP_ROUTE] = 1; plan[CRUSE_CP_CO_T] = 0; }
        if (r != 0) return r < 0 ? r : CRUSE_OK;
    }
    if (c.bbi != nullptr) return CONV_NOT_FUSED;
    CRUSE_REQUIRE(c.bni == nullptr, CRUSE_E_SHAPE, "%s_bnin: the fused input BatchNorm needs the MFMA kernel in the bf16 mode (%s %d, Cout %d, prec %d)",
                  who, cin, c.Cin, c.Cout, c.prec);
    CRUSE_REQUIRE(c.x_dtype == CRUSE_DT_F32 && c.y_dtype == CRUSE_DT_F32, CRUSE_E_DTYPE,
                  "%s: a bf16 input / output needs the MFMA kernel in the bf16 data-gradient mode (%s %d, Cout %d, prec %d)", who, cin, c.Cin, c.Cout, c.prec);
    // the VALU gather kernel has a statistics epilogue for up to 64 channels, the VALU scatter kernel has none
    const bool fuse = !c.scatter && c.sums && c.Cout <= 64 && c.bnb == nullptr;
    const float* x = static_cast<const float*>(c.x);
    float* y = static_cast<float*>(c.y);
    ConvArgs a{x, c.w, c.bias, y, c.B, c.T, c.Cin, c.Fin, c.Cout, c.Fout, c.KT, c.S, c.pad, c.w_layout, c.act, c.accum, fuse ? c.sums : nullptr};
    const size_t lds = (((size_t)c.Cin * c.KT * 3 * c.Cout + 3) & ~(size_t)3) * 4 + (size_t)(TF + c.KT - 1) * c.Cin * (c.Fin + 2) * 4;
    CRUSE_REQUIRE(lds <= 160 * 1024, CRUSE_E_SHAPE, "%s: tile needs %zu B of LDS", who, lds);
    const int grid = c.B * cdiv(c.T, TF);
    const int co_t = c.scatter ? (c.Cout % 2 == 0 ? 2 : 1) : (c.Cout % 4 == 0 ? 4 : 1);      // outputs per thread: <4>/<1> gather, <2>/<1> scatter
    if (plan) {
        plan[CRUSE_CP_ROUTE] = 0; plan[CRUSE_CP_MT] = 0; plan[CRUSE_CP_NW] = 0; plan[CRUSE_CP_GRID] = grid; plan[CRUSE_CP_LDS] = (int)lds;
        plan[CRUSE_CP_CO_T] = co_t;
        return CRUSE_OK;
    }
    void (*kern)(ConvArgs) = !c.scatter ? (co_t == 4 ? conv_gather_kernel<4> : conv_gather_kernel<1>)
                                        : (co_t == 2 ? conv_scatter2_kernel<2> : conv_scatter2_kernel<1>);
    int rc;
    if ((rc = set_smem(kern, lds, who))) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(CONV_THREADS), lds, c.stream, a);
    CRUSE_LAUNCH_CHECK(who);
    // no (or no such) statistics epilogue on this path: one more pass over y (the backward sums go to replica 0, the others stay zero)
    const long long rows = (long long)c.B * c.T;
    if (c.bnb) return cruse_bn_act_bwd_reduce(y, c.bnb->y, c.bnb->mean, c.bnb->rstd, c.bnb->gamma, c.bnb->beta, rows, c.Cout, c.Fout,
                                              c.bnb->relu, c.sums, 1, c.stream);
    if (c.sums && !fuse) return cruse_bn_stats(y, rows, c.Cout, c.Fout, c.sums, 1, c.stream);
    return CRUSE_OK;
}

// the forms: what each pair of entry points checks and adds before conv_run.  `who` is the entry point's name in messages.
int prep_sums(const char* who, const CruseConvCall& c, int zeroed) {
    CRUSE_REQUIRE(c.sums != nullptr, CRUSE_E_SHAPE, "%s: sums is NULL", who);
    if (!zeroed) return cruse_zero_async(c.sums, 2 * (size_t)c.Cout * CRUSE_BN_STAT_REPLICAS * sizeof(double), c.stream, who);
    return CRUSE_OK;
}

int conv_bnstats(const char* who, const CruseConvCall& c, int zeroed) {
    if (const int arc = conv_aligned(who, c, nullptr, nullptr, nullptr)) return arc;
    const int rc = prep_sums(who, c, zeroed);
    return rc ? rc : conv_run(c);
}

int conv_bnbwd(const char* who, CruseConvCall c, const CruseBnBwd& bnb, int zeroed) {
    CRUSE_REQUIRE(bnb.y && bnb.mean && bnb.rstd && bnb.gamma && bnb.beta, CRUSE_E_SHAPE, "%s: BatchNorm tensors missing", who);
    if (const int arc = conv_aligned(who, c, &bnb, nullptr, nullptr)) return arc;
    const int rc = prep_sums(who, c, zeroed);
    if (rc) return rc;
    c.bnb = &bnb;
    return conv_run(c);
}

int conv_bnin(const char* who, CruseConvCall c, const CruseBnIn& bni, int zeroed) {
    CRUSE_REQUIRE(c.x && bni.sums && bni.gamma && bni.beta && bni.nrep >= 1 && bni.count > 0, CRUSE_E_SHAPE, "%s: input BatchNorm tensors missing", who);
    CRUSE_REQUIRE((bni.mean_o == nullptr) == (bni.rstd_o == nullptr) && (bni.rmean == nullptr) == (bni.rvar == nullptr), CRUSE_E_SHAPE,
                  "%s: mean / rstd and the running statistics come in pairs", who);
    if (const int arc = conv_aligned(who, c, nullptr, &bni, nullptr)) return arc;
    if (c.sums) { const int rc = prep_sums(who, c, zeroed); if (rc) return rc; }
    c.bni = &bni;
    return conv_run(c);
}

// Data-gradient convolutions with the BatchNorm(+ReLU) BACKWARD of their input applied while staging (see CruseBnBwdIn): one entry point =
// cruse_bn_act_bwd_apply(dout -> dy_bf16, parameter gradients) + cruse_conv_*[_bnbwd](dy_bf16 -> y).  Shapes / modes the MFMA kernel does not
// take run exactly those two calls.  c.x / c.x_dtype: dout; bnb.y null: no output-side sums.
int conv_bnbwd_in(const char* who, CruseConvCall c, CruseBnBwdIn bb, const CruseBnBwd& bnb, int zeroed, int* plan = nullptr) {
    CRUSE_REQUIRE(c.x && bb.y && bb.mean && bb.rstd && bb.gamma && bb.beta && bb.sums && bb.nrep >= 1, CRUSE_E_SHAPE,
                  "%s: input BatchNorm tensors missing", who);
    CRUSE_REQUIRE((bnb.y == nullptr) == (c.sums == nullptr), CRUSE_E_SHAPE, "%s: bn_y and sums come together", who);
    if (const int arc = conv_aligned(who, c, bnb.y ? &bnb : nullptr, nullptr, &bb)) return arc;
    if (c.sums) { const int rc = prep_sums(who, c, zeroed); if (rc) return rc; }
    bb.count = (long long)c.B * c.T * c.Fin;
    c.bnb = bnb.y ? &bnb : nullptr;
    const int dout_dtype = c.x_dtype;
    if (dout_dtype == CRUSE_DT_BF16) {
        c.bbi = &bb;
        const int rc = conv_run(c, plan);
        if (rc != CONV_NOT_FUSED) return rc;
        c.bbi = nullptr;
    }
    CRUSE_REQUIRE(bb.copy_bf16 != nullptr, CRUSE_E_SHAPE, "conv_*_bnbwd_in: dy_bf16 is required");
    if (!plan) {
        const int rc = cruse_bn_act_bwd_apply(static_cast<const float*>(c.x), bb.y, bb.mean, bb.rstd, bb.gamma, bb.beta, bb.sums, bb.nrep, (long long)c.B * c.T,
                                              c.Cin, c.Fin, bb.relu, bb.training, dout_dtype, bb.copy_bf16, CRUSE_DT_BF16, bb.dgamma, bb.dbeta, bb.dbias,
                                              c.stream);
        if (rc) return rc;
    }
    c.x = bb.copy_bf16; c.x_dtype = CRUSE_DT_BF16;
    return conv_run(c, plan);
}

}  // namespace

// The ten entry points: each fills the descriptor from its own argument list (the scatter2 lists have no S / w_layout) and hands it to its form.
extern "C" int cruse_conv_gather(const float* x, const float* w, const float* bias, float* y,
                                 int B, int T, int Cin, int Fin, int Cout, int Fout,
                                 int KT, int S, int pad, int w_layout, int act, int accum, int prec, int x_dtype, int y_dtype, void* stream) {
    return conv_run({0, x, w, bias, y, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, act, accum, prec, x_dtype, y_dtype, nullptr, (hipStream_t)stream});
}

extern "C" int cruse_conv_scatter2(const float* g, const float* w, const float* bias, float* y,
                                   int B, int T, int Cs, int Fg, int Cout, int Fout,
                                   int KT, int pad, int act, int accum, int prec, int x_dtype, int y_dtype, void* stream) {
    return conv_run({1, g, w, bias, y, B, T, Cs, Fg, Cout, Fout, KT, 2, pad, 0, act, accum, prec, x_dtype, y_dtype, nullptr, (hipStream_t)stream});
}

extern "C" int cruse_conv_gather_bnstats(const float* x, const float* w, const float* bias, float* y,
                                         int B, int T, int Cin, int Fin, int Cout, int Fout,
                                         int KT, int S, int pad, int prec, double* sums, int zeroed, void* stream) {
    return conv_bnstats("conv_gather_bnstats", {0, x, w, bias, y, B, T, Cin, Fin, Cout, Fout, KT, S, pad, 0, 0, 0, prec, CRUSE_DT_F32, CRUSE_DT_F32, sums, (hipStream_t)stream}, zeroed);
}

extern "C" int cruse_conv_scatter2_bnstats(const float* g, const float* w, const float* bias, float* y,
                                           int B, int T, int Cs, int Fg, int Cout, int Fout,
                                           int KT, int pad, int prec, double* sums, int zeroed, void* stream) {
    return conv_bnstats("conv_scatter2_bnstats", {1, g, w, bias, y, B, T, Cs, Fg, Cout, Fout, KT, 2, pad, 0, 0, 0, prec, CRUSE_DT_F32, CRUSE_DT_F32, sums, (hipStream_t)stream}, zeroed);
}

extern "C" int cruse_conv_gather_bnbwd(const float* x, const float* w, float* y, int B, int T, int Cin, int Fin, int Cout, int Fout,
                                       int KT, int S, int pad, int w_layout, int accum, int prec,
                                       const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                       int relu, double* sums, int zeroed, int x_dtype, int y_dtype, void* stream) {
    return conv_bnbwd("conv_gather_bnbwd", {0, x, w, nullptr, y, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, 0, accum, prec, x_dtype, y_dtype, sums, (hipStream_t)stream}, {bn_y, mean, rstd, gamma, beta, relu}, zeroed);
}

extern "C" int cruse_conv_scatter2_bnbwd(const float* g, const float* w, float* y, int B, int T, int Cs, int Fg, int Cout, int Fout,
                                         int KT, int pad, int accum, int prec,
                                         const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         int relu, double* sums, int zeroed, int x_dtype, int y_dtype, void* stream) {
    return conv_bnbwd("conv_scatter2_bnbwd", {1, g, w, nullptr, y, B, T, Cs, Fg, Cout, Fout, KT, 2, pad, 0, 0, accum, prec, x_dtype, y_dtype, sums, (hipStream_t)stream}, {bn_y, mean, rstd, gamma, beta, relu}, zeroed);
}

extern "C" int cruse_conv_gather_bnin(const float* x_pre, const double* in_sums, int in_replicas, long long in_count, float eps, float momentum,
                                      const float* in_gamma, const float* in_beta, float* in_mean, float* in_rstd, float* in_running_mean,
                                      float* in_running_var, const float* in_add, void* in_copy_bf16,
                                      const float* w, const float* bias, float* y, int B, int T, int Cin, int Fin, int Cout, int Fout,
                                      int KT, int S, int pad, int prec, double* out_sums, int zeroed, void* stream) {
    return conv_bnin("conv_gather_bnin", {0, x_pre, w, bias, y, B, T, Cin, Fin, Cout, Fout, KT, S, pad, 0, 0, 0, prec, CRUSE_DT_F32, CRUSE_DT_F32, out_sums, (hipStream_t)stream},
                     {in_sums, in_replicas, in_count, eps, momentum, in_gamma, in_beta, in_mean, in_rstd, in_running_mean, in_running_var, in_add,
                      in_copy_bf16}, zeroed);
}

extern "C" int cruse_conv_scatter2_bnin(const float* g_pre, const double* in_sums, int in_replicas, long long in_count, float eps, float momentum,
                                        const float* in_gamma, const float* in_beta, float* in_mean, float* in_rstd, float* in_running_mean,
                                        float* in_running_var, const float* in_add, void* in_copy_bf16,
                                        const float* w, const float* bias, float* y, int B, int T, int Cs, int Fg, int Cout, int Fout,
                                        int KT, int pad, int prec, double* out_sums, int zeroed, void* stream) {
    return conv_bnin("conv_scatter2_bnin", {1, g_pre, w, bias, y, B, T, Cs, Fg, Cout, Fout, KT, 2, pad, 0, 0, 0, prec, CRUSE_DT_F32, CRUSE_DT_F32, out_sums, (hipStream_t)stream},
                     {in_sums, in_replicas, in_count, eps, momentum, in_gamma, in_beta, in_mean, in_rstd, in_running_mean, in_running_var, in_add,
                      in_copy_bf16}, zeroed);
}

extern "C" int cruse_conv_gather_bnbwd_in(const void* dout, int dout_dtype, const float* in_y, const float* in_mean, const float* in_rstd,
                                          const float* in_gamma, const float* in_beta, const double* in_sums, int in_replicas, int in_relu,
                                          int in_training, void* dy_bf16, float* in_dgamma, float* in_dbeta, float* in_dbias,
                                          const float* w, void* y, int B, int T, int Cin, int Fin, int Cout, int Fout, int KT, int S, int pad,
                                          int w_layout, int accum, int prec,
                                          const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                                          double* sums, int zeroed, int y_dtype, void* stream) {
    return conv_bnbwd_in("conv_gather_bnbwd_in", {0, dout, w, nullptr, y, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, 0, accum, prec, dout_dtype, y_dtype, sums, (hipStream_t)stream},
                         {in_y, in_sums, in_replicas, 0, in_mean, in_rstd, in_gamma, in_beta, in_relu, in_training, dy_bf16, in_dgamma, in_dbeta, in_dbias},
                         {bn_y, mean, rstd, gamma, beta, relu}, zeroed);
}

extern "C" int cruse_conv_scatter2_bnbwd_in(const void* dout, int dout_dtype, const float* in_y, const float* in_mean, const float* in_rstd,
                                            const float* in_gamma, const float* in_beta, const double* in_sums, int in_replicas, int in_relu,
                                            int in_training, void* dy_bf16, float* in_dgamma, float* in_dbeta, float* in_dbias,
                                            const float* w, void* y, int B, int T, int Cs, int Fg, int Cout, int Fout, int KT, int pad, int accum,
                                            int prec,
                                            const float* bn_y, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                                            double* sums, int zeroed, int y_dtype, void* stream) {
    return conv_bnbwd_in("conv_scatter2_bnbwd_in", {1, dout, w, nullptr, y, B, T, Cs, Fg, Cout, Fout, KT, 2, pad, 0, 0, accum, prec, dout_dtype, y_dtype, sums, (hipStream_t)stream},
                         {in_y, in_sums, in_replicas, 0, in_mean, in_rstd, in_gamma, in_beta, in_relu, in_training, dy_bf16, in_dgamma, in_dbeta, in_dbias},
                         {bn_y, mean, rstd, gamma, beta, relu}, zeroed);
}

// Host-only (no device is touched): what a call of this shape, mode and forms would launch -- conv_run's own decision with the launches left
// out.  forms: CRUSE_CONV_FORM_* bits; BNB implies output-side sums; with BBI, x_dtype is the dtype of dout and the two-call fallback reports
// the plan of its data-gradient call.  Pointers are taken as 16-byte aligned.
extern "C" int cruse_conv_plan(int scatter, int Cin, int Fin, int Cout, int Fout, int KT, int S, int pad, int w_layout,
                               int B, int T, int prec, int x_dtype, int y_dtype, int act, int accum, int forms, int* out) {
    CRUSE_REQUIRE(out != nullptr && forms >= 0 && forms < 16, CRUSE_E_SHAPE, "conv_plan: out is NULL or forms = %d", forms);
    CRUSE_REQUIRE(!scatter || (S == 2 && w_layout == 0), CRUSE_E_SHAPE, "conv_plan: the scatter2 form has S = 2 and w_layout = 0");
    alignas(16) static float buf[4];                 // stands for every tensor: never dereferenced
    static double dsums[1];
    const CruseBnBwd bnb = {buf, buf, buf, buf, buf, 1};
    const CruseBnIn bni = {dsums, 1, (long long)B * T * Fin, 1e-5f, 0.1f, buf, buf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const CruseBnBwdIn bbi = {buf, dsums, 1, 0, buf, buf, buf, buf, 1, 1, buf, nullptr, nullptr, nullptr};
    const bool has_bnb = (forms & CRUSE_CONV_FORM_BNB) != 0;
    CruseConvCall c = {scatter ? 1 : 0, buf, buf, nullptr, buf, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, act, accum, prec, x_dtype, y_dtype,
                       (forms & CRUSE_CONV_FORM_SUMS) || has_bnb ? dsums : nullptr, nullptr, has_bnb ? &bnb : nullptr,
                       (forms & CRUSE_CONV_FORM_BNI) ? &bni : nullptr};
    for (int i = 0; i < CRUSE_CP_N; ++i) out[i] = 0;
    if (forms & CRUSE_CONV_FORM_BBI) return conv_bnbwd_in(scatter ? "conv_scatter2_bnbwd_in" : "conv_gather_bnbwd_in", c, bbi, has_bnb ? bnb : CruseBnBwd{}, 1, out);
    return conv_run(c, out);
}

extern "C" size_t cruse_conv_wgrad_ws_bytes(int Ca, int Cb, int KT) {
    // partial slabs: [slab][Ca][Cb][KT][3] (LDS-staged and VALU kernels) or accumulator images of 16 x 16 tiles (register-direct kernel)
    return (size_t)CRUSE_WGRAD_MAX_SLABS * ((Ca + 15) / 16 * 16) * ((Cb + 15) / 16 * 16) * KT * 3 * sizeof(float);
}

namespace {

// the VALU kernel's decider: it is asked last, so what it cannot take is refused (f32 operands, 4-channel output tiles that divide the block)
int wgrad_valu_plan(const CruseWgradCall& c, CruseWgradPlan& p) {
    CRUSE_REQUIRE(c.a_dtype == CRUSE_DT_F32 && c.bt_dtype == CRUSE_DT_F32, CRUSE_E_DTYPE,
                  "conv_wgrad: bf16 operands need the MFMA kernel (Ca %d, Cb %d, prec %d)", c.Ca, c.Cb, c.prec);
    CRUSE_REQUIRE(c.Ca % 4 == 0 && (c.Cb % 4 == 0 || c.Cb == 1), CRUSE_E_SHAPE,
                  "conv_wgrad: Ca=%d must be a multiple of 4 and Cb=%d a multiple of 4 or 1", c.Ca, c.Cb);
    const int cbt = (c.Cb % 4 == 0) ? 4 : 1;
    const int NT = (c.Ca / 4) * (c.Cb / cbt);
    // a thread must keep one output tile: items w = tid + n*256 have ot = w % NT = tid % NT iff 256 % NT == 0
    CRUSE_REQUIRE(WG_THREADS % NT == 0, CRUSE_E_SHAPE,
                  NT % WG_THREADS == 0 ? "conv_wgrad: %d output tiles > %d threads" : "conv_wgrad: %d output tiles do not divide the %d-thread block",
                  NT, WG_THREADS);
    const int CaP = c.Ca + 4, CbP = (cbt == 4) ? c.Cb + 4 : c.Cb;
    const size_t lds_stage = ((size_t)TF * c.Fa * CaP + (size_t)(TF + c.KT - 1) * (c.Fb + 2) * CbP) * 4;
    const size_t lds_red = (size_t)c.Ca * c.Cb * c.KT * 3 * 4;
    const size_t lds = lds_stage > lds_red ? lds_stage : lds_red;
    CRUSE_REQUIRE(lds <= 160 * 1024, CRUSE_E_SHAPE, "conv_wgrad: needs %zu B of LDS", lds);
    const int ntiles = c.B * cdiv(c.T, TF);
    const int grid = ntiles < CRUSE_WGRAD_MAX_SLABS ? ntiles : CRUSE_WGRAD_MAX_SLABS;
    int* v = p.v;
    v[CRUSE_WP_KERNEL] = CRUSE_WK_VALU;
    v[CRUSE_WP_T0] = cbt; v[CRUSE_WP_T1] = c.KT; v[CRUSE_WP_T2] = 0; v[CRUSE_WP_T3] = 0;
    v[CRUSE_WP_GRID] = grid; v[CRUSE_WP_BLOCK] = WG_THREADS; v[CRUSE_WP_LDS] = (int)lds;
    v[CRUSE_WP_SLABS] = grid; v[CRUSE_WP_TG] = 0; v[CRUSE_WP_FPW] = 0;
    v[CRUSE_WP_REDUCE] = CRUSE_WR_SLABS; v[CRUSE_WP_RGX] = cdiv(c.Ca * c.Cb * c.KT * 3, 256); v[CRUSE_WP_RGY] = cdiv(grid, 16);
    return 1;
}

int wgrad_valu_launch(const CruseWgradCall& c, const CruseWgradPlan& pl) {
    const int* v = pl.v;
    WgradArgs p{(const float*)c.a, (const float*)c.bt, (float*)c.ws, c.B, c.T, c.Ca, c.Fa, c.Cb, c.Fb, c.S, c.pad, c.B * cdiv(c.T, TF)};
    void (*kern)(WgradArgs) = v[CRUSE_WP_T0] == 4 ? (c.KT == 2 ? conv_wgrad_kernel<4, 2> : conv_wgrad_kernel<4, 1>)
                                                  : (c.KT == 2 ? conv_wgrad_kernel<1, 2> : conv_wgrad_kernel<1, 1>);
    const int rc = set_smem(kern, v[CRUSE_WP_LDS], "conv_wgrad");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(v[CRUSE_WP_GRID]), dim3(v[CRUSE_WP_BLOCK]), v[CRUSE_WP_LDS], c.stream, p);
    return CRUSE_OK;
}

// The one host path of cruse_conv_wgrad: validate, ask the three deciders in turn (register-direct: the plain bf16 mode, the bench shapes;
// LDS-staged MFMA; VALU), launch the kernel that took the call and the reduce that sums its slabs into dw.
// plan != null (cruse_conv_wgrad_plan): decide the same way, write what would be launched and launch nothing.
int wgrad_run(const CruseWgradCall& c, int* plan = nullptr) {
    CRUSE_REQUIRE(c.B > 0 && c.T > 0 && c.Ca > 0 && c.Cb > 0, CRUSE_E_SHAPE, "conv_wgrad: empty shape");
    CRUSE_REQUIRE((c.a_dtype == CRUSE_DT_F32 || c.a_dtype == CRUSE_DT_BF16) && (c.bt_dtype == CRUSE_DT_F32 || c.bt_dtype == CRUSE_DT_BF16),
                  CRUSE_E_DTYPE, "conv_wgrad: operand dtypes %d / %d (f32 or bf16)", c.a_dtype, c.bt_dtype);
    CRUSE_REQUIRE((c.KT == 1 || c.KT == 2) && (c.S == 1 || c.S == 2) && (c.pad == 0 || c.pad == 1), CRUSE_E_SHAPE,
                  "conv_wgrad: unsupported KT=%d S=%d pad=%d", c.KT, c.S, c.pad);
    CruseWgradPlan p = {};
    int r = 0;
    if (c.prec >= 0) {
        r = cruse_wgrad_rd_plan(c, p);
        if (r == 0) r = cruse_wgrad_mfma_plan(c, p);
    }
    if (r == 0) r = wgrad_valu_plan(c, p);
    if (r < 0) return r;
    if (plan) {
        for (int i = 0; i < CRUSE_WP_N; ++i) plan[i] = p.v[i];
        return CRUSE_OK;
    }
    const int kernel = p.v[CRUSE_WP_KERNEL];
    const int rc = kernel == CRUSE_WK_RD ? cruse_wgrad_rd_launch(c, p) : kernel == CRUSE_WK_MFMA ? cruse_wgrad_mfma_launch(c, p) : wgrad_valu_launch(c, p);
    if (rc) return rc;
    CRUSE_LAUNCH_CHECK(kernel == CRUSE_WK_RD ? "wgrad_rd" : kernel == CRUSE_WK_MFMA ? "wgrad_mfma" : "conv_wgrad");
    if (p.v[CRUSE_WP_REDUCE] == CRUSE_WR_RD) {
        cruse_wgrad_rd_reduce(c, p);
        CRUSE_LAUNCH_CHECK("wgrad_rd_reduce");
    } else {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(p.v[CRUSE_WP_RGX], p.v[CRUSE_WP_RGY]), dim3(256), 0, c.stream, (const float*)c.ws,
                           p.v[CRUSE_WP_SLABS], c.Ca * c.Cb * c.KT * 3, c.dw);
        CRUSE_LAUNCH_CHECK("conv_wgrad_reduce");
    }
    return CRUSE_OK;
}

}  // namespace

extern "C" int cruse_conv_wgrad(const float* a, const float* bt, float* dw,
                                int B, int T, int Ca, int Fa, int Cb, int Fb,
                                int KT, int S, int pad, int prec, int a_dtype, int bt_dtype, void* ws, void* stream) {
    return wgrad_run({a, bt, a_dtype, bt_dtype, dw, ws, cruse_conv_wgrad_ws_bytes(Ca, Cb, KT), B, T, Ca, Fa, Cb, Fb, KT, S, pad, prec, (hipStream_t)stream});
}

// Host-only (no device is touched): what a weight-gradient call of this shape, mode and operand dtypes would launch -- wgrad_run's own
// decision with the launches left out.  a_misalign / bt_misalign: the operand addresses modulo 16 (alignment selects between the kernels);
// ws_bytes 0: the workspace of cruse_conv_wgrad_ws_bytes, as the entry point assumes.
extern "C" int cruse_conv_wgrad_plan(int B, int T, int Ca, int Fa, int Cb, int Fb, int KT, int S, int pad, int prec, int a_dtype, int bt_dtype,
                                     int a_misalign, int bt_misalign, size_t ws_bytes, int* out) {
    CRUSE_REQUIRE(out != nullptr && a_misalign >= 0 && a_misalign < 16 && bt_misalign >= 0 && bt_misalign < 16, CRUSE_E_SHAPE,
                  "conv_wgrad_plan: out is NULL or misalignments %d / %d (0..15)", a_misalign, bt_misalign);
    alignas(16) static char buf[32];                 // stands for every tensor: never dereferenced
    for (int i = 0; i < CRUSE_WP_N; ++i) out[i] = 0;
    return wgrad_run({buf + a_misalign, buf + bt_misalign, a_dtype, bt_dtype, nullptr, buf, ws_bytes ? ws_bytes : cruse_conv_wgrad_ws_bytes(Ca, Cb, KT),
                      B, T, Ca, Fa, Cb, Fb, KT, S, pad, prec, nullptr}, out);
}

extern "C" int cruse_channel_sum(const float* g, long long rows, int C, int F, float* out, void* stream) {
    CRUSE_REQUIRE(rows > 0 && C > 0 && F > 0 && C <= 2048, CRUSE_E_SHAPE,
                  "channel_sum: bad shape rows=%lld C=%d F=%d (C <= 2048)", rows, C, F);
    // few rows (a training step of a few short clips): one workgroup walks them all, in a fixed order; there is no parallelism to lose
    if (rows <= CHANNEL_SUM_ORDERED_ROWS) {
        hipLaunchKernelGGL(channel_sum_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, g, rows, C, F, C * F, out);
    } else {
        long long nb = rows < 512 ? rows : 512;
        hipLaunchKernelGGL(channel_sum_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, g, rows, C, F, C * F, out);
    }
    CRUSE_LAUNCH_CHECK("channel_sum");
    return CRUSE_OK;
}

extern "C" int cruse_col_sum(const float* g, long long rows, int ncol, int ld, float* out, void* stream) {
    CRUSE_REQUIRE(rows > 0 && ncol > 0 && ncol <= 2048 && ld >= ncol, CRUSE_E_SHAPE,
                  "col_sum: bad shape rows=%lld ncol=%d ld=%d (ncol <= 2048)", rows, ncol, ld);
    long long nb = rows < 512 ? rows : 512;
    hipLaunchKernelGGL(channel_sum_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, g, rows, ncol, 1, ld, out);
    CRUSE_LAUNCH_CHECK("col_sum");
    return CRUSE_OK;
}
