// Multi-resolution spectral loss (MultResSpecLoss / Stft / angle of test/test_loss.py:140-243 with its two one-token
// repairs): for every resolution N (power of two, 128..2048; hop N/4, periodic Hann, center = True with reflect padding, normalized)
//   loss += factor * mean (|Y|^g - |S|^g)^2 + f_complex * mean |Y|^g e^{i arg Y} - |S|^g e^{i arg S}|^2,   Y = STFT_N(est), S = STFT_N(ref)
// and its gradient wrt est, without the spectra ever leaving the chip.
//
// One workgroup of 256 lanes owns a run of MR_K hops of the PADDED time axis (L + N samples) of one clip at one resolution and runs every
// frame that touches the run, MR_P = 2048 / N frames at a time:
//   gather (reflect, window, N^-1/2)  ->  two N/2-point complex FFTs per frame (est and ref, each as z[n] = x[2n] + i x[2n+1]; the same
//   instructions on both signals, so est == ref gives Y == S bit for bit)  ->  split to the one-sided bins, loss terms (counted by the run
//   that owns the frame's first sample) and G = dloss/dY  ->  the adjoint of the windowed real FFT as ONE N/2-point FFT per frame  ->
//   window and overlap-add into the run's own samples in LDS, frames in ascending order.
// Owner computes: no float atomics anywhere.  Loss partial sums are f64, one per workgroup; mrspec_finalize_kernel adds them in a fixed
// order.  mrspec_fold_kernel folds the reflected ends of the padded gradients back and sums the resolutions in call order.
// FFT: Stockham autosort radix 4 (+ one radix-2 pass where log2(N/2) is odd) between two padded LDS images, twiddles from a per-workgroup
// table of sincospif of exact rationals, every sum of products written with fmaf (the scheme of fftconv_core.h, size-templated).
#include "common.h"

// No contraction of a * b + c anywhere in this file: every fused product is written as fmaf.  The exact zeros of est == ref rest on it
// (a * u - s * v must round both products; hipcc's default would fuse one of them, and __fmul_rn is a plain product to it).
#pragma clang fp contract(off)

namespace {

struct cf { float x, y; };

constexpr int MR_T = 256;                    // lanes of a workgroup
constexpr int MR_PTS = 2048;                 // complex points of the two LDS images = samples of the frames in flight
constexpr int MR_IMG = MR_PTS + MR_PTS / 32; // cf elements of a padded image
constexpr int MR_MAX_R = 8;

// hops of a run: MR_K + 3 frames touch it, a multiple of the MR_P frames in flight
__host__ __device__ constexpr int mr_hops(int log2n) { return log2n == 7 ? 29 : log2n == 8 ? 13 : log2n == 9 ? 13 : log2n == 10 ? 9 : 8; }

// image index of point i: one cf of padding after every 32 (a radix-4 pass with Ns = 1 writes lanes 4 points apart)
__device__ __forceinline__ int mr_pad(int i) { return i + (i >> 5); }
__device__ __forceinline__ cf mr_mul(cf a, cf b) { return {fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)}; }
__device__ __forceinline__ cf mr_mulc(cf a, cf b) { return {fmaf(a.x, b.x, a.y * b.y), fmaf(a.y, b.x, -(a.x * b.y))}; }      // a * conj(b)

// nb transforms of M = 2^LOG2M points each, transform f at points f * M .. of `src`; returns the image that holds the result (natural order).
// tw[k] = exp(-2 pi i k / (2 M)).  Ends with a barrier.
template <int LOG2M>
__device__ __forceinline__ cf* mr_fft(cf* src, cf* dst, const cf* tw, int nb, int tid) {
    constexpr int M = 1 << LOG2M, Q = M / 4;
    int Ns = 1;
#pragma unroll
    for (int pass = 0; pass < LOG2M / 2; ++pass) {
        for (int jj = tid; jj < nb * Q; jj += MR_T) {
            const int base = (jj >> (LOG2M - 2)) * M, j = jj & (Q - 1), r = j & (Ns - 1);
            cf a0 = src[mr_pad(base + j)], a1 = src[mr_pad(base + j + Q)], a2 = src[mr_pad(base + j + 2 * Q)], a3 = src[mr_pad(base + j + 3 * Q)];
            if (pass > 0) {
                const int q = r * (2 * M / (4 * Ns));
                a1 = mr_mul(a1, tw[q]); a2 = mr_mul(a2, tw[2 * q]); a3 = mr_mul(a3, tw[3 * q]);
            }
            const cf s02 = {a0.x + a2.x, a0.y + a2.y}, d02 = {a0.x - a2.x, a0.y - a2.y};
            const cf s13 = {a1.x + a3.x, a1.y + a3.y}, d13 = {a1.y - a3.y, -(a1.x - a3.x)};          // (a1 - a3) * -i
            const int o = base + (j - r) * 4 + r;
            dst[mr_pad(o)] = {s02.x + s13.x, s02.y + s13.y};
            dst[mr_pad(o + Ns)] = {d02.x + d13.x, d02.y + d13.y};
            dst[mr_pad(o + 2 * Ns)] = {s02.x - s13.x, s02.y - s13.y};
            dst[mr_pad(o + 3 * Ns)] = {d02.x - d13.x, d02.y - d13.y};
        }
        __syncthreads();
        cf* t = src; src = dst; dst = t;
        Ns *= 4;
    }
    if (LOG2M & 1) {                                                                                   // radix 2, Ns = M / 2
        constexpr int Hf = M / 2;
        for (int jj = tid; jj < nb * Hf; jj += MR_T) {
            const int base = (jj >> (LOG2M - 1)) * M, j = jj & (Hf - 1);
            const cf a0 = src[mr_pad(base + j)], a1 = mr_mul(src[mr_pad(base + j + Hf)], tw[2 * j]);
            dst[mr_pad(base + j)] = {a0.x + a1.x, a0.y + a1.y};
            dst[mr_pad(base + j + Hf)] = {a0.x - a1.x, a0.y - a1.y};
        }
        __syncthreads();
        cf* t = src; src = dst; dst = t;
    }
    return src;
}

struct MrTerms { float gamma, fm, fc2; int unit; };        // fm = factor / (B F T), fc2 = f_complex / (2 B F T), unit: gamma == 1

// loss terms of one bin (added to `acc` when `count`) and G = dloss/dY as autograd gives it on the reference's code: abs has gradient 0 at
// 0, clamp_min(1e-12) gradient 0 below its bound, angle.backward divides by max(|Y|^2, 1e-10).  The phase factor is Y / |Y| under a guard
// (atan2(0, 0) = 0: the factor is 1 there).
struct MrPolar { float r, rc, a; cf u; };
// |Z|, its clamped value, the compressed magnitude and the phase factor of one bin.  NOT inlined, and so the same instructions for the
// estimate and the reference: bit-identical spectra give bit-identical terms, which is what makes est == ref an exact zero
__device__ __noinline__ MrPolar mr_polar(cf Z, float gamma, int unit) {
    MrPolar o;
    o.r = sqrtf(fmaf(Z.x, Z.x, Z.y * Z.y));
    o.u = o.r > 0.f ? cf{Z.x / o.r, Z.y / o.r} : cf{1.f, 0.f};
    o.rc = unit ? o.r : fmaxf(o.r, 1e-12f);
    o.a = unit ? o.r : powf(o.rc, gamma);
    return o;
}
// bins k and M - k of the N-point spectrum of a real frame from bins k and M - k of its packed M-point transform (NOT inlined, as above)
__device__ __noinline__ void mr_split(cf zk, cf zm, cf wk, cf* y0, cf* y1) {
    const cf E = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)}, O = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    const cf wo = mr_mul(O, wk);
    *y0 = {E.x + wo.x, E.y + wo.y};
    *y1 = {E.x - wo.x, -(E.y - wo.y)};
}

__device__ __forceinline__ cf mr_bin(cf Y, cf S, const MrTerms& p, bool count, float& acc) {
    const MrPolar py = mr_polar(Y, p.gamma, p.unit), ps = mr_polar(S, p.gamma, p.unit);
    const float r = py.r, a = py.a, s = ps.a;
    const cf uY = py.u, uS = ps.u;
    const cf sgn = r > 0.f ? uY : cf{0.f, 0.f};
    const float d = a - s;
    if (p.unit) {
        const cf D = {Y.x - S.x, Y.y - S.y};
        if (count) acc += fmaf(p.fm * d, d, p.fc2 * fmaf(D.x, D.x, D.y * D.y));
        const float ga = 2.f * p.fm * d;
        return {fmaf(ga, sgn.x, 2.f * p.fc2 * D.x), fmaf(ga, sgn.y, 2.f * p.fc2 * D.y)};
    }
    // both products rounded before the difference (contraction is off): Y == S bit for bit gives D == 0 exactly
    const cf D = {a * uY.x - s * uS.x, a * uY.y - s * uS.y};
    if (count) acc += fmaf(p.fm * d, d, p.fc2 * fmaf(D.x, D.x, D.y * D.y));
    const cf w = mr_mulc(D, uY);
    const float ga = fmaf(2.f * p.fm, d, 2.f * p.fc2 * w.x);
    const float gphi = 2.f * p.fc2 * a * w.y / fmaxf(r * r, 1e-10f);
    const float gr = r >= 1e-12f ? ga * p.gamma * (a / py.rc) : 0.f;
    return {fmaf(gr, sgn.x, -(gphi * Y.y)), fmaf(gr, sgn.y, gphi * Y.x)};
}

// grid = (runs, B).  part[b * runs + run] receives the workgroup's loss sum; gpad ([B, L + N], null: evaluation) the run's gradient samples
template <int LOG2N>
__global__ __launch_bounds__(MR_T) void mrspec_kernel(const float* __restrict__ est, const float* __restrict__ ref, int L, MrTerms terms,
                                                      double* __restrict__ part, float* __restrict__ gpad) {
    constexpr int N = 1 << LOG2N, M = N / 2, H = N / 4, P = MR_PTS / N, K = mr_hops(LOG2N), C = K * H, HB = M / 2 + 1;
    __shared__ cf img0[MR_IMG], img1[MR_IMG];
    __shared__ cf tw[3 * N / 4];
    __shared__ float ola[C];
    __shared__ double red[MR_T / 64];
    const int tid = threadIdx.x, run = blockIdx.x, b = blockIdx.y;
    const int T = 1 + L / H, Lp = L + N;
    const float* eb = est + (size_t)b * L;
    const float* rb = ref + (size_t)b * L;
    const bool grad = gpad != nullptr;
    const int tb = run * K;                                   // the frames this run owns: tb .. tb + K - 1
    // evaluation keeps the grouping of the gradient call, so that the f32 partial sums add up in the same order (the same loss bits), and
    // leaves out the frames it does not own
    const int tfirst = tb - 3, nframes = K + 3;
    const float rsq = rsqrtf((float)N);

    for (int k = tid; k < 3 * N / 4; k += MR_T) {
        float s, c;
        sincospif((float)(-2 * k) / (float)N, &s, &c);
        tw[k] = {c, s};
    }
    for (int i = tid; i < C; i += MR_T) ola[i] = 0.f;
    __syncthreads();

    double acc = 0.0;
    for (int t0 = tfirst; t0 < tfirst + nframes; t0 += P) {
        if (!grad && (t0 + P <= tb || t0 >= tb + K)) continue;                   // (uniform) no owned frame in this group
        // ---- gather: transform 2 f = est, 2 f + 1 = ref of frame t0 + f, z[n] = x[2n] + i x[2n+1], windowed and scaled
        for (int e = tid; e < P * M; e += MR_T) {
            const int f = e >> (LOG2N - 1), n = e & (M - 1), t = t0 + f;
            cf ze = {0.f, 0.f}, zr = {0.f, 0.f};
            if (t >= 0 && t < T && (grad || (t >= tb && t < tb + K))) {
                float xe[2], xr[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int m = 2 * n + u;
                    int i = t * H + m - M;
                    if (i < 0) i = -i;
                    if (i >= L) i = 2 * (L - 1) - i;
                    const float w = (0.5f - 0.5f * tw[m <= M ? m : N - m].x) * rsq;
                    xe[u] = eb[i] * w;
                    xr[u] = rb[i] * w;
                }
                ze = {xe[0], xe[1]}; zr = {xr[0], xr[1]};
            }
            img0[mr_pad((2 * f) * M + n)] = ze;
            img0[mr_pad((2 * f + 1) * M + n)] = zr;
        }
        __syncthreads();
        cf* Z = mr_fft<LOG2N - 1>(img0, img1, tw, 2 * P, tid);
        cf* W = Z == img0 ? img1 : img0;
        // ---- bins k and M - k of every frame: Y, S, loss terms, G, and the packed spectrum of the adjoint (conjugated: the transform below
        //      is the forward one).  Bin 0 pairs with the Nyquist bin M; bin M / 2 with itself.
        float part_f = 0.f;
        for (int e = tid; e < P * HB; e += MR_T) {
            const int f = e / HB, k = e - f * HB, t = t0 + f;
            const bool valid = t >= 0 && t < T && (grad || (t >= tb && t < tb + K));
            const bool count = valid && t >= tb && t < tb + K;
            cf G0 = {0.f, 0.f}, G1 = {0.f, 0.f};
            const cf wk = tw[k];
            if (valid) {
                cf Yk[2], Sk[2];
#pragma unroll
                for (int sgl = 0; sgl < 2; ++sgl) {
                    const cf zk = Z[mr_pad((2 * f + sgl) * M + k)], zm = Z[mr_pad((2 * f + sgl) * M + ((M - k) & (M - 1)))];
                    cf y0, y1;                                                                          // bins k and M - k
                    mr_split(zk, zm, wk, &y0, &y1);
                    if (sgl == 0) { Yk[0] = y0; Yk[1] = y1; } else { Sk[0] = y0; Sk[1] = y1; }
                }
                G0 = mr_bin(Yk[0], Sk[0], terms, count, part_f);
                if (2 * k != M) G1 = mr_bin(Yk[1], Sk[1], terms, count, part_f);
            }
            if (grad) {
                // X[k] = G[k] / 2 (real part of G at bins 0 and M); A = X[k] + conj X[M-k], D = X[k] - conj X[M-k];
                // Zt[k] = A + i conj(w^k) D, Zt[M-k] = conj(A - i conj(w^k) D)
                cf X0, X1;
                if (k == 0) { X0 = {G0.x, 0.f}; X1 = {G1.x, 0.f}; }
                else if (2 * k == M) { X0 = {0.5f * G0.x, 0.5f * G0.y}; X1 = X0; }
                else { X0 = {0.5f * G0.x, 0.5f * G0.y}; X1 = {0.5f * G1.x, 0.5f * G1.y}; }
                const cf A = {X0.x + X1.x, X0.y - X1.y}, D = {X0.x - X1.x, X0.y + X1.y};
                const cf cd = mr_mulc(D, wk);                                                        // conj(w^k) D
                const cf icd = {-cd.y, cd.x};
                W[mr_pad(f * M + k)] = {A.x + icd.x, -(A.y + icd.y)};                              // conj(Zt[k])
                if (k != 0 && 2 * k != M) W[mr_pad(f * M + M - k)] = {A.x - icd.x, A.y - icd.y};    // conj(Zt[M-k]) = A - i conj(w^k) D
            }
        }
        acc += (double)part_f;
        __syncthreads();
        if (grad) {
            const cf* X = mr_fft<LOG2N - 1>(W, Z, tw, P, tid);
            // ---- x[2n] = Re, x[2n+1] = -Im of the transform; window, scale, add to the run's samples: frames in ascending order
            for (int pl = tid; pl < C; pl += MR_T) {
                const int p = run * C + pl;
                if (p >= Lp) break;
                const int hp = p / H;
                int lo = hp - 3, hi = hp;
                if (lo < 0) lo = 0;
                if (lo < t0) lo = t0;
                if (hi > T - 1) hi = T - 1;
                if (hi > t0 + P - 1) hi = t0 + P - 1;
                float v = ola[pl];
                for (int t = lo; t <= hi; ++t) {
                    const int n = p - t * H;
                    const cf z = X[mr_pad((t - t0) * M + (n >> 1))];
                    const float w = (0.5f - 0.5f * tw[n <= M ? n : N - n].x) * rsq;
                    v = fmaf((n & 1) ? -z.y : z.x, w, v);
                }
                ola[pl] = v;
            }
            __syncthreads();
        }
    }
    if (grad) {
        float* gb = gpad + (size_t)b * Lp;
        for (int pl = tid; pl < C; pl += MR_T) {
            const int p = run * C + pl;
            if (p < Lp) gb[p] = ola[pl];
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[(size_t)b * gridDim.x + run] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct MrFold { const float* g[MR_MAX_R]; int n[MR_MAX_R]; int R; };

// dest[b, i] = grad_scale * sum_r (centre + left reflection + right reflection of the padded gradient of resolution r), r ascending
__global__ __launch_bounds__(256) void mrspec_fold_kernel(MrFold fo, int L, float gscale, float* __restrict__ dest) {
    const int b = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < L; i += gridDim.x * 256) {
        float v = 0.f;
        for (int r = 0; r < fo.R; ++r) {
            const int N = fo.n[r], M = N / 2;
            const float* g = fo.g[r] + (size_t)b * (L + N);
            float s = g[i + M];
            if (i >= 1 && i <= M) s += g[M - i];                                   // padded sample p = M - i reads sample i
            if (i <= L - 2 && i >= L - 1 - M) s += g[2 * (L - 1) - i + M];         // p = 2 (L - 1) - i + M
            v += s;
        }
        dest[(size_t)b * L + i] = v * gscale;
    }
}

// loss[0] = the n partial sums, added in a fixed order
__global__ __launch_bounds__(256) void mrspec_finalize_kernel(const double* __restrict__ part, long long n, double* __restrict__ loss) {
    __shared__ double red[256];
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) a += part[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0];
}

inline int mr_log2(int n) {
    for (int l = 7; l <= 11; ++l) if (n == (1 << l)) return l;
    return 0;
}
inline size_t mr_up256(size_t v) { return (v + 255) / 256 * 256; }
constexpr int MR_MAX_L = 1 << 30;
constexpr int MR_MAX_B = 65535;
constexpr long long MR_MAX_BL = 1ll << 36;

// workspace: | f64 partial sums, resolution after resolution: B * runs_r each | rounded up to 256 bytes | f32 [B, L + N_r] per resolution,
// each rounded up to 256 bytes |;  runs_r = ceil((L + N_r) / (hops(N_r) * N_r / 4))
struct MrLayout { long long runs[MR_MAX_R]; size_t part_off[MR_MAX_R], grad_off[MR_MAX_R], bytes; long long nparts; };

// 0 when the shape is fine, else the message in `why`
int mr_layout(int B, int L, const int* n_ffts, int R, MrLayout* lay, char* why, size_t nwhy) {
    if (B <= 0 || B > MR_MAX_B) { snprintf(why, nwhy, "mrspec: B=%d outside 1..%d", B, MR_MAX_B); return 1; }
    if (R < 1 || R > MR_MAX_R) { snprintf(why, nwhy, "mrspec: R=%d outside 1..%d", R, MR_MAX_R); return 1; }
    if (n_ffts == nullptr) { snprintf(why, nwhy, "mrspec: n_ffts is null"); return 1; }
    int nmax = 0;
    for (int r = 0; r < R; ++r) {
        if (!mr_log2(n_ffts[r])) { snprintf(why, nwhy, "mrspec: n_ffts[%d]=%d is not a power of two in [128, 2048]", r, n_ffts[r]); return 1; }
        if (n_ffts[r] > nmax) nmax = n_ffts[r];
    }
    if (L <= nmax / 2) { snprintf(why, nwhy, "mrspec: L=%d must exceed max n_fft / 2 = %d (reflect padding)", L, nmax / 2); return 1; }
    if (L > MR_MAX_L) { snprintf(why, nwhy, "mrspec: L=%d above %d", L, MR_MAX_L); return 1; }
    if ((long long)B * L > MR_MAX_BL) { snprintf(why, nwhy, "mrspec: B*L=%lld above %lld", (long long)B * L, MR_MAX_BL); return 1; }
    size_t off = 0;
    lay->nparts = 0;
    for (int r = 0; r < R; ++r) {
        const int N = n_ffts[r], C = mr_hops(mr_log2(N)) * (N / 4);
        lay->runs[r] = ((long long)L + N + C - 1) / C;
        lay->part_off[r] = off;
        off += (size_t)B * lay->runs[r] * sizeof(double);
        lay->nparts += (long long)B * lay->runs[r];
    }
    off = mr_up256(off);
    for (int r = 0; r < R; ++r) {
        lay->grad_off[r] = off;
        off = mr_up256(off + (size_t)B * ((size_t)L + n_ffts[r]) * sizeof(float));
    }
    lay->bytes = off;
    return 0;
}

}  // namespace

extern "C" size_t cruse_mrspec_ws_bytes(int B, int L, const int* n_ffts, int R) {
    MrLayout lay;
    char why[160];
    if (mr_layout(B, L, n_ffts, R, &lay, why, sizeof(why))) { cruse_set_error("%s", why); return 0; }
    return lay.bytes;
}

extern "C" int cruse_mrspec_loss(const float* est, const float* ref, int B, int L, const int* n_ffts, int R, float gamma, float factor,
                                 const float* f_complex, void* ws, size_t ws_bytes, double* loss, float* dest, float grad_scale,
                                 void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CRUSE_REQUIRE(est != nullptr, CRUSE_E_SHAPE, "mrspec: est is null");
    CRUSE_REQUIRE(ref != nullptr, CRUSE_E_SHAPE, "mrspec: ref is null");
    CRUSE_REQUIRE(ws != nullptr, CRUSE_E_SHAPE, "mrspec: ws is null");
    CRUSE_REQUIRE(loss != nullptr, CRUSE_E_SHAPE, "mrspec: loss is null");
    MrLayout lay;
    char why[160];
    CRUSE_REQUIRE(mr_layout(B, L, n_ffts, R, &lay, why, sizeof(why)) == 0, CRUSE_E_SHAPE, "%s", why);
    CRUSE_REQUIRE(gamma > 0.f, CRUSE_E_SHAPE, "mrspec: gamma=%g must be positive", (double)gamma);
    CRUSE_REQUIRE(ws_bytes >= lay.bytes, CRUSE_E_SHAPE, "mrspec: ws_bytes=%zu below cruse_mrspec_ws_bytes = %zu", ws_bytes, lay.bytes);
    char* base = (char*)ws;
    MrFold fo;
    fo.R = R;
    for (int r = 0; r < R; ++r) {
        const int N = n_ffts[r], l2 = mr_log2(N);
        const double cnt = (double)B * (double)(N / 2 + 1) * (double)(1 + L / (N / 4));
        MrTerms tm;
        tm.gamma = gamma;
        tm.unit = gamma == 1.f;
        tm.fm = (float)((double)factor / cnt);
        tm.fc2 = f_complex ? (float)((double)f_complex[r] / (2.0 * cnt)) : 0.f;
        double* part = (double*)(base + lay.part_off[r]);
        float* gpad = dest ? (float*)(base + lay.grad_off[r]) : nullptr;
        fo.g[r] = gpad;
        fo.n[r] = N;
        const dim3 grid((unsigned)lay.runs[r], (unsigned)B);
        switch (l2) {
            case 7: hipLaunchKernelGGL(mrspec_kernel<7>, grid, dim3(MR_T), 0, stream, est, ref, L, tm, part, gpad); break;
            case 8: hipLaunchKernelGGL(mrspec_kernel<8>, grid, dim3(MR_T), 0, stream, est, ref, L, tm, part, gpad); break;
            case 9: hipLaunchKernelGGL(mrspec_kernel<9>, grid, dim3(MR_T), 0, stream, est, ref, L, tm, part, gpad); break;
            case 10: hipLaunchKernelGGL(mrspec_kernel<10>, grid, dim3(MR_T), 0, stream, est, ref, L, tm, part, gpad); break;
            default: hipLaunchKernelGGL(mrspec_kernel<11>, grid, dim3(MR_T), 0, stream, est, ref, L, tm, part, gpad); break;
        }
        CRUSE_LAUNCH_CHECK("mrspec");
    }
    hipLaunchKernelGGL(mrspec_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)base, lay.nparts, loss);
    CRUSE_LAUNCH_CHECK("mrspec_finalize");
    if (dest) {
        int gx = (L + 1023) / 1024;
        if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(mrspec_fold_kernel, dim3(gx, B), dim3(256), 0, stream, fo, L, grad_scale, dest);
        CRUSE_LAUNCH_CHECK("mrspec_fold");
    }
    return CRUSE_OK;
}
