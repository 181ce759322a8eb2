// Biquad cascade over whole clips (cruse_biquad_cascade): the on-device replacement of torchaudio.functional.lfilter under the
// reference's EQ augmentation (train_base/acoustics/audioAug.py:149-178), DESIGN section 14.  Samples are f32 in HBM; coefficients,
// states, the recurrence and every value handed from one section to the next are f64.  No atomics and a fixed evaluation order:
// a result is bit-identical from run to run and a clip filters the same alone and inside a batch.
//
// A second-order recurrence is a dependent chain along time, made parallel here as a scan of affine maps.  One workgroup of 1024
// lanes owns a clip; a lane owns CHUNK = 32 consecutive samples in registers (as f64: 64 VGPRs), a tile is 1024 * 32 samples.
// Per section, with the transposed direct form II that scipy.signal.lfilter runs,
//     y = b0 x + z0;  z0 <- b1 x + z1 - a1 y;  z1 <- b2 x - a2 y,         state s = (z0, z1),  A = [[-a1, 1], [-a2, 0]]:
//   1 each lane runs its chunk from a zero state and keeps the end state p: over a chunk s_out = M s_in + p with M = A^32, the
//     same matrix for every chunk of the (clip, section)
//   2 an inclusive scan of (M^k, p) over the 64 lanes of a wave (6 shuffle steps, the uniform matrices M^1, M^2 .. M^32 come from an
//     LDS table designed once per workgroup), wave totals through LDS, the 16 totals chained with M^64 from the tile's incoming state
//   3 each lane runs its chunk again from its true state, clips if asked, and the outputs are the next section's inputs, still in
//     registers.  The second run is exact; nothing but the 2-component states crosses lanes.
// A clip longer than a tile goes through tiles in order inside the same workgroup; the S end states are carried in LDS.  No
// workgroup waits for another, x is read once and y written once.  A lane's chunk is contiguous in memory, so rows are loaded and
// stored coalesced (one 256-byte row per wave instruction) and transposed through a wave-private LDS image with a row stride of
// 33 floats: the row-wise writes and the chunk-wise reads are both free of bank conflicts.
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int CHUNK = CRUSE_BIQUAD_CHUNK, LOG2_CHUNK = 5;
constexpr int TILE = THREADS * CHUNK;
constexpr int LSTR = CHUNK + 1;            // floats between two lanes' chunks in the staging image
constexpr int MAXS = 8;
static_assert(CHUNK == 1 << LOG2_CHUNK && CHUNK <= 64, "the chunk is a power of two (M = A^CHUNK by squaring, staging rows of 64)");
static_assert(TILE == CRUSE_BIQUAD_TILE, "CRUSE_BIQUAD_TILE is THREADS * CRUSE_BIQUAD_CHUNK");

// one section as the workgroup uses it: b0 b1 b2 a1 a2 over a0, then M^(2^d), d = 0..6, row-major 2x2
struct SecTab { double c[5]; double mp[7][4]; };
constexpr int TAB_D = (int)(sizeof(SecTab) / sizeof(double));

// LDS, in doubles then floats: tab[MAXS] | tot[2][WAVES][2] | carry[2][MAXS][2] | stage[THREADS * LSTR] f32
constexpr int OFF_TOT = MAXS * TAB_D, OFF_CARRY = OFF_TOT + 2 * WAVES * 2, OFF_STAGE = OFF_CARRY + 2 * MAXS * 2;
constexpr size_t LDS_BYTES = (size_t)OFF_STAGE * sizeof(double) + (size_t)THREADS * LSTR * sizeof(float);
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup's LDS");

__device__ __forceinline__ void mat_sq(double* m) {
    const double a = m[0], b = m[1], c = m[2], d = m[3];
    m[0] = fma(a, a, b * c);
    m[1] = fma(a, b, b * d);
    m[2] = fma(c, a, d * c);
    m[3] = fma(c, b, d * d);
}

// u <- m u
__device__ __forceinline__ void mat_vec(const double* m, double& u0, double& u1) {
    const double t0 = fma(m[0], u0, m[1] * u1), t1 = fma(m[2], u0, m[3] * u1);
    u0 = t0;
    u1 = t1;
}

__global__ void __launch_bounds__(THREADS) biquad_cascade_kernel(const float* __restrict__ x, const double* __restrict__ coef, int coef_stride,
                                                                 int L, int S, int clamp, float* __restrict__ y) {
    extern __shared__ double lds[];
    SecTab* tab = reinterpret_cast<SecTab*>(lds);
    double* tot = lds + OFF_TOT;
    double* carry = lds + OFF_CARRY;
    float* stage = reinterpret_cast<float*>(lds + OFF_STAGE);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* xb = x + (size_t)blockIdx.x * L;
    float* yb = y + (size_t)blockIdx.x * L;

    if (tid < S) {                                                     // design: once per workgroup
        const double* c = coef + (size_t)blockIdx.x * coef_stride + 6 * tid;
        const double a0 = c[3], a1 = c[4] / a0, a2 = c[5] / a0;
        SecTab& t = tab[tid];
        t.c[0] = c[0] / a0; t.c[1] = c[1] / a0; t.c[2] = c[2] / a0; t.c[3] = a1; t.c[4] = a2;
        double m[4] = {-a1, 1.0, -a2, 0.0};
        for (int i = 0; i < LOG2_CHUNK; ++i) mat_sq(m);                // M = A^CHUNK
        for (int d = 0; d < 7; ++d) {
            t.mp[d][0] = m[0]; t.mp[d][1] = m[1]; t.mp[d][2] = m[2]; t.mp[d][3] = m[3];
            mat_sq(m);
        }
        carry[2 * tid] = 0.0;                                          // carry[0][tid]: the clip starts from rest
        carry[2 * tid + 1] = 0.0;
    }
    __syncthreads();

    float* wst = stage + wv * 64 * LSTR;                               // this wave's image: 64 chunks
    double v[CHUNK];
    const int ntiles = (L + TILE - 1) / TILE;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int wbase = tile * TILE + wv * 64 * CHUNK;               // < L + TILE: L <= MAX_L keeps it an int
        // rows of 64 consecutive samples -> image; sample g of the wave's region sits at g + g / CHUNK
        {
            float r[CHUNK];
            if (wbase + 64 * CHUNK <= L) {                             // wave-uniform: the whole region lies inside the clip
                const float* xp = xb + wbase + lane;
#pragma unroll
                for (int k = 0; k < CHUNK; ++k) r[k] = xp[k * 64];
            } else {
#pragma unroll
                for (int k = 0; k < CHUNK; ++k) {
                    const int idx = wbase + k * 64 + lane;
                    const float val = xb[min(idx, L - 1)];
                    r[k] = idx < L ? val : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) {
                const int g = k * 64 + lane;
                wst[g + (g >> LOG2_CHUNK)] = r[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) v[j] = (double)wst[lane * LSTR + j];

        const int par = tile & 1;
        for (int s = 0; s < S; ++s) {
            const SecTab& t = tab[s];
            const double b0 = t.c[0], b1 = t.c[1], b2 = t.c[2], a1 = t.c[3], a2 = t.c[4];
            // 1: the chunk from rest -> p
            double z0 = 0.0, z1 = 0.0;
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) {
                const double xi = v[j], yo = fma(b0, xi, z0);
                z0 = fma(-a1, yo, fma(b1, xi, z1));
                z1 = fma(b2, xi, -a2 * yo);
            }
            // 2: inclusive scan over the wave; after step d lane i holds the map of chunks (i - 2^(d+1), i]
            double p0 = z0, p1 = z1;
#pragma unroll 1
            for (int d = 0; d < 6; ++d) {
                double q0 = __shfl_up(p0, 1 << d, 64), q1 = __shfl_up(p1, 1 << d, 64);
                mat_vec(t.mp[d], q0, q1);
                if (lane >= (1 << d)) { p0 += q0; p1 += q1; }
            }
            double e0 = __shfl_up(p0, 1, 64), e1 = __shfl_up(p1, 1, 64);      // exclusive: the chunks of the wave before this lane
            if (lane == 0) { e0 = 0.0; e1 = 0.0; }
            double* tt = tot + (s & 1) * WAVES * 2;
            if (lane == 63) { tt[2 * wv] = p0; tt[2 * wv + 1] = p1; }
            __syncthreads();
            // the tile's incoming state through the 16 wave totals; every lane ends with the tile's outgoing state
            double c0 = carry[(par * MAXS + s) * 2], c1 = carry[(par * MAXS + s) * 2 + 1], u0 = 0.0, u1 = 0.0;
#pragma unroll 1
            for (int w = 0; w < WAVES; ++w) {
                if (w == wv) { u0 = c0; u1 = c1; }
                mat_vec(t.mp[6], c0, c1);
                c0 += tt[2 * w];
                c1 += tt[2 * w + 1];
            }
            if (tid == 0) { carry[((par ^ 1) * MAXS + s) * 2] = c0; carry[((par ^ 1) * MAXS + s) * 2 + 1] = c1; }
            // M^lane on the wave's incoming state, by the bits of the lane (powers of one matrix commute)
#pragma unroll 1
            for (int d = 0; d < 6; ++d) {
                double n0 = u0, n1 = u1;
                mat_vec(t.mp[d], n0, n1);
                if ((lane >> d) & 1) { u0 = n0; u1 = n1; }
            }
            z0 = u0 + e0;
            z1 = u1 + e1;
            // 3: the chunk from its true state
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) {
                const double xi = v[j];
                double yo = fma(b0, xi, z0);
                z0 = fma(-a1, yo, fma(b1, xi, z1));
                z1 = fma(b2, xi, -a2 * yo);
                if (clamp) yo = fmin(fmax(yo, -1.0), 1.0);
                v[j] = yo;
            }
        }
        // chunks -> image -> rows
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) wst[lane * LSTR + j] = (float)v[j];
        __syncthreads();
        if (wbase + 64 * CHUNK <= L) {
            float* yp = yb + wbase + lane;
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) {
                const int g = k * 64 + lane;
                yp[k * 64] = wst[g + (g >> LOG2_CHUNK)];
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < CHUNK; ++k) {
                const int g = k * 64 + lane, idx = wbase + g;
                if (idx < L) yb[idx] = wst[g + (g >> LOG2_CHUNK)];
            }
        }
        __syncthreads();
    }
}

constexpr int MAX_L = (1 << 30);           // tile * TILE + 64 * CHUNK * 16 stays below 2^31

int check_shape(const char* who, int B, int L, int S) {
    CRUSE_REQUIRE(B >= 1 && L >= 1 && S >= 1, CRUSE_E_SHAPE, "%s: B = %d, L = %d, S = %d", who, B, L, S);
    CRUSE_REQUIRE(S <= MAXS, CRUSE_E_SHAPE, "%s: S = %d sections, at most %d", who, S, MAXS);
    CRUSE_REQUIRE(L <= MAX_L, CRUSE_E_SHAPE, "%s: L = %d > %d", who, L, MAX_L);
    return CRUSE_OK;
}

}  // namespace

extern "C" size_t cruse_biquad_ws_bytes(int B, int L, int S) {
    (void)B; (void)L; (void)S;                                         // no shape needs one (and none is judged here: cruse_last_error stays)
    return 0;                                                          // a clip never leaves its workgroup: nothing to hand over
}

extern "C" int cruse_biquad_cascade(const float* x, const double* coef, int coef_stride, int B, int L, int S, int clamp, void* ws, float* y,
                                    void* stream) {
    (void)ws;
    CRUSE_REQUIRE(x && coef && y, CRUSE_E_SHAPE, "biquad_cascade: null buffer");
    const int rc = check_shape("biquad_cascade", B, L, S);
    if (rc) return rc;
    CRUSE_REQUIRE(coef_stride == 0 || coef_stride == 6 * S, CRUSE_E_SHAPE, "biquad_cascade: coef_stride = %d, expected 0 (shared) or %d", coef_stride,
                  6 * S);
    CRUSE_REQUIRE(((uintptr_t)coef & 7) == 0, CRUSE_E_ALIGN, "biquad_cascade: coefficients not 8-byte aligned");
    const int rl = cruse_ensure_dyn_lds(reinterpret_cast<const void*>(biquad_cascade_kernel), LDS_BYTES, "biquad_cascade");
    if (rl) return rl;
    hipLaunchKernelGGL(biquad_cascade_kernel, dim3(B), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, x, coef, coef_stride, L, S, clamp, y);
    CRUSE_LAUNCH_CHECK("cruse_biquad_cascade");
    return CRUSE_OK;
}
