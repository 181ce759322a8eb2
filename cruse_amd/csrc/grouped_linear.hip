// Grouped linears and band pooling for the DeepFilterNet-style blocks of model/based_model/cust_conv.py:
//   GroupedLinearEinsum (:503-538), GroupedLinear (:545-579) -- G independent [Ig -> Hg] linears over feature slices, one launch
//   for all groups, forward / input gradient / weight gradient -- and the ERB filterbank products of erb_fb_use (:187-207) as sums
//   over contiguous bands instead of a GEMM with a [F, n_bands] matrix of zeros.
// Exact f32: v_mfma_f32_16x16x4_f32, f32 accumulation, one summation order (no atomics): results are bit-identical from run to run.
// A block is 4 waves and owns a 64 x 64 output tile of one group; the reduction index goes through LDS in chunks of 32.  Every
// element of a tile is fetched under its own bounds test and is 0.0f outside: no width, row count or stride is assumed to be a
// multiple of anything, and nothing is read or written beyond a row or a tensor.
#include "common.h"

namespace {

constexpr int TM = 64, TN = 64, TK = 32;
constexpr int LDA = TK + 1, LDB = TN + 1;        // LDS row pitches: odd, so the fragment reads below spread over the banks
constexpr int NLD = TM * TK / 256;               // elements of one operand tile a thread carries (8)

// column of output j of group g in a [rows][G * W] tensor.  "cat": g W + j.  "shuffled": GroupedLinear(shuffle=True),
// cust_conv.py:575-578 -- view(-1, W, G).transpose(-1, -2) moves cat[q G + p] to p W + q, so the cat index c = g W + j = q G + p
// lands at (c % G) W + c / G
__device__ __forceinline__ int gl_col(int map, int g, int j, int G, int W) {
    if (map == CRUSE_GL_CAT) return g * W + j;
    const int c = g * W + j;
    return (c % G) * W + c / G;
}

// acc[j] += As[16 rows of wave wv][TK] * Bs[TK][16 columns of sub-tile j], j < nsub (block-uniform)
__device__ __forceinline__ void gl_mma_chunk(const float* As, const float* Bs, int wv, int lane, int nsub, f32x4 (&acc)[4]) {
    const float* a = As + (wv * 16 + (lane & 15)) * LDA + (lane >> 4);
    const float* b = Bs + (lane >> 4) * LDB + (lane & 15);
#pragma unroll
    for (int kk = 0; kk < TK; kk += 4) {
        const float av = a[kk];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nsub) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[kk * LDB + j * 16], acc[j], 0, 0, 0);
    }
}

// ---- rows x group products: forward (a = x, w strides (in, out)) and input gradient (a = dy under the ReLU mask, strides swapped) ----
struct GlRowsArgs {
    const float* a; const float* mask; const float* w; const float* bias; float* c;
    long long sg, sk, sn;                        // w[g sg + k sk + n sn]
    int rows, G, Kg, Ng, a_map, c_map, relu, tiles_n;
};

__global__ __launch_bounds__(256) void gl_rows_kernel(GlRowsArgs p) {
    __shared__ float As[TM * LDA];
    __shared__ float Bs[TK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = blockIdx.y / p.tiles_n, n0 = (blockIdx.y % p.tiles_n) * TN;
    const int m0 = blockIdx.x * TM;
    const long long lda = (long long)p.G * p.Kg, ldc = (long long)p.G * p.Ng;
    const bool kfast = p.sk == 1 && p.sn != 1;   // the stacked nn.Linear layout: consecutive lanes follow the contiguous index
    const int nsub = min(4, (p.Ng - n0 + 15) >> 4);
    const float* wg = p.w + (long long)g * p.sg;

    float ra[NLD], rb[NLD];
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int idx = tid + 256 * q;
            const int gm = m0 + (idx >> 5), gk = k0 + (idx & 31);
            float v = 0.f;
            if (gm < p.rows && gk < p.Kg) {
                const long long off = (long long)gm * lda + gl_col(p.a_map, g, gk, p.G, p.Kg);
                v = p.a[off];
                if (p.mask != nullptr && !(p.mask[off] > 0.f)) v = 0.f;
            }
            ra[q] = v;
        }
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int idx = tid + 256 * q;
            const int k = kfast ? (idx & 31) : (idx >> 6), n = kfast ? (idx >> 5) : (idx & 63);
            const int gk = k0 + k, gn = n0 + n;
            rb[q] = (gk < p.Kg && gn < p.Ng) ? wg[(long long)gk * p.sk + (long long)gn * p.sn] : 0.f;
        }
    };
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    gload(0);
    for (int k0 = 0; k0 < p.Kg; k0 += TK) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int idx = tid + 256 * q;
            As[(idx >> 5) * LDA + (idx & 31)] = ra[q];
            const int k = kfast ? (idx & 31) : (idx >> 6), n = kfast ? (idx >> 5) : (idx & 63);
            Bs[k * LDB + n] = rb[q];
        }
        __syncthreads();
        if (k0 + TK < p.Kg) gload(k0 + TK);
        gl_mma_chunk(As, Bs, wv, lane, nsub, acc);
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (j >= nsub || n >= p.Ng) continue;
        const float bv = p.bias != nullptr ? p.bias[g * p.Ng + n] : 0.f;
        const int col = gl_col(p.c_map, g, n, p.G, p.Ng);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wv * 16 + (lane >> 4) * 4 + r;
            if (m >= p.rows) continue;
            float v = acc[j][r] + bv;
            if (p.relu) v = fmaxf(v, 0.f);
            p.c[(long long)m * ldc + col] = v;
        }
    }
}

// ---- weight gradient: dW[g][i][j] = sum_rows x[row][g Ig + i] dy[row][col(g, j)], db[g Hg + j] = sum_rows dy[row][col(g, j)] ---------
// grid (tiles of Ig x Hg, G, parts): with parts > 1 every part writes its own slab of the workspace and gl_dw_reduce_kernel sums
// the slabs in ascending order of the part
struct GlDwArgs {
    const float* x; const float* dy; const float* mask; float* dw; float* db; float* ws_w; float* ws_b;
    long long sg, si, so;
    int rows, G, Ig, Hg, map, tiles_n, parts, kchunk;
};

__global__ __launch_bounds__(256) void gl_dw_kernel(GlDwArgs p) {
    __shared__ float As[TM * LDA];
    __shared__ float Bs[TK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = blockIdx.y, part = blockIdx.z;
    const int m0 = (blockIdx.x / p.tiles_n) * TM, n0 = (blockIdx.x % p.tiles_n) * TN;
    const int kbeg = part * p.kchunk, kend = min(p.rows, kbeg + p.kchunk);
    const long long ldx = (long long)p.G * p.Ig, ldy = (long long)p.G * p.Hg;
    const int nsub = min(4, (p.Hg - n0 + 15) >> 4);
    const bool want_db = p.db != nullptr && m0 == 0 && tid < TN;

    float ra[NLD], rb[NLD];
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int idx = tid + 256 * q;
            const int gk = k0 + (idx >> 6), gm = m0 + (idx & 63), gn = n0 + (idx & 63);
            ra[q] = (gk < kend && gm < p.Ig) ? p.x[(long long)gk * ldx + g * p.Ig + gm] : 0.f;
            float v = 0.f;
            if (gk < kend && gn < p.Hg) {
                const long long off = (long long)gk * ldy + gl_col(p.map, g, gn, p.G, p.Hg);
                v = p.dy[off];
                if (p.mask != nullptr && !(p.mask[off] > 0.f)) v = 0.f;
            }
            rb[q] = v;
        }
    };
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;

    gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += TK) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int idx = tid + 256 * q;
            As[(idx & 63) * LDA + (idx >> 6)] = ra[q];
            Bs[(idx >> 6) * LDB + (idx & 63)] = rb[q];
        }
        __syncthreads();
        if (k0 + TK < kend) gload(k0 + TK);
        gl_mma_chunk(As, Bs, wv, lane, nsub, acc);
        if (want_db) {
#pragma unroll
            for (int k = 0; k < TK; ++k) dbacc += Bs[k * LDB + tid];
        }
        __syncthreads();
    }

    const long long slab = ((long long)part * p.G + g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (j >= nsub || n >= p.Hg) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wv * 16 + (lane >> 4) * 4 + r;
            if (m >= p.Ig) continue;
            if (p.parts == 1) p.dw[(long long)g * p.sg + (long long)m * p.si + (long long)n * p.so] = acc[j][r];
            else p.ws_w[(slab * p.Ig + m) * p.Hg + n] = acc[j][r];
        }
    }
    if (want_db && n0 + tid < p.Hg) {
        if (p.parts == 1) p.db[g * p.Hg + n0 + tid] = dbacc;
        else p.ws_b[slab * p.Hg + n0 + tid] = dbacc;
    }
}

__global__ __launch_bounds__(256) void gl_dw_reduce_kernel(GlDwArgs p) {
    const long long nw = (long long)p.G * p.Ig * p.Hg, nb = p.db != nullptr ? (long long)p.G * p.Hg : 0;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < nw) {
        float s = 0.f;
        for (int z = 0; z < p.parts; ++z) s += p.ws_w[z * nw + e];
        const int j = (int)(e % p.Hg), i = (int)((e / p.Hg) % p.Ig), g = (int)(e / ((long long)p.Hg * p.Ig));
        p.dw[(long long)g * p.sg + (long long)i * p.si + (long long)j * p.so] = s;
    } else if (e < nw + nb) {
        const long long c = e - nw, nbb = (long long)p.G * p.Hg;
        float s = 0.f;
        for (int z = 0; z < p.parts; ++z) s += p.ws_b[z * nbb + c];
        p.db[c] = s;
    }
}

// rows of a part: a multiple of TK, at least 256 (a shorter slice does not pay for its slab), at most 64 parts, and no more
// parts than fill the device about twice
int gl_dw_parts(int rows, int G, int Ig, int Hg, int* kchunk) {
    const long long tiles = (long long)G * cdiv(Ig, TM) * cdiv(Hg, TN);
    long long parts = cdivl(512, tiles);
    if (parts > 64) parts = 64;
    if (parts > cdiv(rows, 256)) parts = cdiv(rows, 256);
    if (parts < 1) parts = 1;
    const int kc = cdiv(cdiv(rows, (int)parts), TK) * TK;
    *kchunk = kc;
    return cdiv(rows, kc);
}

int gl_check(const char* who, int rows, int G, int Ig, int Hg, long long sg, long long si, long long so, int out_map) {
    CRUSE_REQUIRE(rows >= 1 && G >= 1 && Ig >= 1 && Hg >= 1, CRUSE_E_SHAPE, "%s: rows=%d G=%d Ig=%d Hg=%d must all be >= 1", who, rows, G, Ig, Hg);
    CRUSE_REQUIRE(rows <= (1 << 30), CRUSE_E_SHAPE, "%s: rows=%d > 2^30", who, rows);
    CRUSE_REQUIRE((long long)G * Ig < (1ll << 31) && (long long)G * Hg < (1ll << 31), CRUSE_E_SHAPE, "%s: G*Ig or G*Hg >= 2^31", who);
    CRUSE_REQUIRE(sg >= 1 && si >= 1 && so >= 1, CRUSE_E_SHAPE, "%s: weight strides (%lld, %lld, %lld) must be >= 1", who, sg, si, so);
    CRUSE_REQUIRE(out_map == CRUSE_GL_CAT || out_map == CRUSE_GL_SHUFFLED, CRUSE_E_SHAPE, "%s: unknown out_map %d", who, out_map);
    CRUSE_REQUIRE(G <= 65535 && (long long)G * cdiv(Ig, TN) <= 65535 && (long long)G * cdiv(Hg, TN) <= 65535, CRUSE_E_SHAPE,
                  "%s: G times the column tiles exceeds the grid (G=%d Ig=%d Hg=%d)", who, G, Ig, Hg);
    return CRUSE_OK;
}

// ---- band pooling -----------------------------------------------------------------------------------------------------------------
constexpr int BAND_ROWS = 4;                     // rows a block holds: 4 rows of any F start on a 16-byte boundary

__device__ __forceinline__ void band_range(const int* starts, int b, int F, int& lo, int& hi) {
    lo = min(max(starts[b], 0), F);              // the table is the caller's; whatever it holds, nothing outside a row is touched
    hi = min(max(starts[b + 1], lo), F);
}

// y[r][b] = w_b sum_{f in band b} x[r][f]
__global__ __launch_bounds__(256) void band_pool_kernel(const float* x, const int* starts, int rows, int F, int nb, int mean, int vec, float* y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [BAND_ROWS][F]
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * BAND_ROWS, nr = min(BAND_ROWS, rows - r0);
    const float* src = x + (long long)r0 * F;
    const int span = nr * F, n4 = vec ? span >> 2 : 0;
    for (int i = tid; i < n4; i += 256) reinterpret_cast<float4*>(sm)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int i = n4 * 4 + tid; i < span; i += 256) sm[i] = src[i];
    __syncthreads();
    for (int e = tid; e < nr * nb; e += 256) {
        const int r = e / nb, b = e % nb;
        int lo, hi;
        band_range(starts, b, F, lo, hi);
        float s = 0.f;
        for (int f = lo; f < hi; ++f) s += sm[r * F + f];
        if (mean) s = hi > lo ? s * (1.0f / (float)(hi - lo)) : 0.f;
        y[(long long)r0 * nb + e] = s;
    }
}

// y[r][f] = w_b(f) m[r][b(f)]; a bin no band covers gets 0
__global__ __launch_bounds__(256) void band_expand_kernel(const float* m, const int* starts, int rows, int F, int nb, int mean, int vec, float* y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // int band_of[F]; float w[nb]; float ms[BAND_ROWS][nb]
    int* band_of = reinterpret_cast<int*>(sm);
    float* wb = sm + F;
    float* ms = wb + nb;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * BAND_ROWS, nr = min(BAND_ROWS, rows - r0);
    for (int f = tid; f < F; f += 256) band_of[f] = -1;
    for (int i = tid; i < nr * nb; i += 256) ms[i] = m[(long long)r0 * nb + i];
    __syncthreads();
    for (int b = tid; b < nb; b += 256) {
        int lo, hi;
        band_range(starts, b, F, lo, hi);
        wb[b] = mean ? (hi > lo ? 1.0f / (float)(hi - lo) : 0.f) : 1.0f;
        for (int f = lo; f < hi; ++f) band_of[f] = b;
    }
    __syncthreads();
    auto value = [&](int e) {
        const int r = e / F, b = band_of[e - r * F];
        return b < 0 ? 0.f : wb[b] * ms[r * nb + b];
    };
    float* dst = y + (long long)r0 * F;
    const int span = nr * F, n4 = vec ? span >> 2 : 0;
    for (int i = tid; i < n4; i += 256)
        reinterpret_cast<float4*>(dst)[i] = make_float4(value(4 * i), value(4 * i + 1), value(4 * i + 2), value(4 * i + 3));
    for (int i = n4 * 4 + tid; i < span; i += 256) dst[i] = value(i);
}

int band_check(const char* who, const void* in, const int* starts, int rows, int F, int nb, const void* out) {
    CRUSE_REQUIRE(in != nullptr && starts != nullptr && out != nullptr, CRUSE_E_SHAPE, "%s: null input, table or output", who);
    CRUSE_REQUIRE(rows >= 1 && rows <= (1 << 30), CRUSE_E_SHAPE, "%s: rows=%d outside 1..2^30", who, rows);
    CRUSE_REQUIRE(F >= 1 && F <= CRUSE_BAND_MAX_F, CRUSE_E_SHAPE, "%s: F=%d outside 1..%d", who, F, CRUSE_BAND_MAX_F);
    CRUSE_REQUIRE(nb >= 1 && nb <= F, CRUSE_E_SHAPE, "%s: n_bands=%d outside 1..F=%d", who, nb, F);
    return CRUSE_OK;
}

}  // namespace

extern "C" int cruse_grouped_linear_fwd(const float* x, const float* w, long long w_sg, long long w_si, long long w_so, const float* bias,
                                        int rows, int G, int Ig, int Hg, int relu, int out_map, float* y, void* stream) {
    CRUSE_REQUIRE(x != nullptr && w != nullptr && y != nullptr, CRUSE_E_SHAPE, "grouped_linear_fwd: null x, w or y");
    if (int rc = gl_check("grouped_linear_fwd", rows, G, Ig, Hg, w_sg, w_si, w_so, out_map)) return rc;
    GlRowsArgs p;
    p.a = x; p.mask = nullptr; p.w = w; p.bias = bias; p.c = y;
    p.sg = w_sg; p.sk = w_si; p.sn = w_so;
    p.rows = rows; p.G = G; p.Kg = Ig; p.Ng = Hg; p.a_map = CRUSE_GL_CAT; p.c_map = out_map; p.relu = relu ? 1 : 0;
    p.tiles_n = cdiv(Hg, TN);
    hipLaunchKernelGGL(gl_rows_kernel, dim3(cdiv(rows, TM), G * p.tiles_n), dim3(256), 0, (hipStream_t)stream, p);
    CRUSE_LAUNCH_CHECK("grouped_linear_fwd");
    return CRUSE_OK;
}

extern "C" int cruse_grouped_linear_bwd_dx(const float* dy, const float* y, const float* w, long long w_sg, long long w_si, long long w_so,
                                           int rows, int G, int Ig, int Hg, int relu, int out_map, float* dx, void* stream) {
    CRUSE_REQUIRE(dy != nullptr && w != nullptr && dx != nullptr, CRUSE_E_SHAPE, "grouped_linear_bwd_dx: null dy, w or dx");
    CRUSE_REQUIRE(!relu || y != nullptr, CRUSE_E_SHAPE, "grouped_linear_bwd_dx: the ReLU mask needs the saved y");
    if (int rc = gl_check("grouped_linear_bwd_dx", rows, G, Ig, Hg, w_sg, w_si, w_so, out_map)) return rc;
    GlRowsArgs p;
    p.a = dy; p.mask = relu ? y : nullptr; p.w = w; p.bias = nullptr; p.c = dx;
    p.sg = w_sg; p.sk = w_so; p.sn = w_si;       // the transposed product: the reduction runs over the outputs
    p.rows = rows; p.G = G; p.Kg = Hg; p.Ng = Ig; p.a_map = out_map; p.c_map = CRUSE_GL_CAT; p.relu = 0;
    p.tiles_n = cdiv(Ig, TN);
    hipLaunchKernelGGL(gl_rows_kernel, dim3(cdiv(rows, TM), G * p.tiles_n), dim3(256), 0, (hipStream_t)stream, p);
    CRUSE_LAUNCH_CHECK("grouped_linear_bwd_dx");
    return CRUSE_OK;
}

extern "C" size_t cruse_grouped_linear_dw_ws_bytes(int rows, int G, int Ig, int Hg) {
    if (rows < 1 || G < 1 || Ig < 1 || Hg < 1) return 0;
    int kc;
    const int parts = gl_dw_parts(rows, G, Ig, Hg, &kc);
    return parts == 1 ? 0 : (size_t)parts * G * ((size_t)Ig * Hg + Hg) * sizeof(float);
}

extern "C" int cruse_grouped_linear_bwd_dw(const float* dy, const float* y, const float* x, int rows, int G, int Ig, int Hg, int relu,
                                           int out_map, float* dw, long long w_sg, long long w_si, long long w_so, float* db, void* ws,
                                           size_t ws_bytes, void* stream) {
    CRUSE_REQUIRE(dy != nullptr && x != nullptr && dw != nullptr, CRUSE_E_SHAPE, "grouped_linear_bwd_dw: null dy, x or dw");
    CRUSE_REQUIRE(!relu || y != nullptr, CRUSE_E_SHAPE, "grouped_linear_bwd_dw: the ReLU mask needs the saved y");
    if (int rc = gl_check("grouped_linear_bwd_dw", rows, G, Ig, Hg, w_sg, w_si, w_so, out_map)) return rc;
    GlDwArgs p;
    p.parts = gl_dw_parts(rows, G, Ig, Hg, &p.kchunk);
    const size_t need = cruse_grouped_linear_dw_ws_bytes(rows, G, Ig, Hg);
    CRUSE_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), CRUSE_E_SHAPE,
                  "grouped_linear_bwd_dw: workspace of %zu bytes, %zu needed", ws == nullptr ? (size_t)0 : ws_bytes, need);
    CRUSE_REQUIRE(need == 0 || ((uintptr_t)ws % 4) == 0, CRUSE_E_ALIGN, "grouped_linear_bwd_dw: workspace not 4-byte aligned");
    p.x = x; p.dy = dy; p.mask = relu ? y : nullptr; p.dw = dw; p.db = db;
    p.ws_w = (float*)ws; p.ws_b = p.ws_w == nullptr ? nullptr : p.ws_w + (size_t)p.parts * G * Ig * Hg;
    p.sg = w_sg; p.si = w_si; p.so = w_so;
    p.rows = rows; p.G = G; p.Ig = Ig; p.Hg = Hg; p.map = out_map; p.tiles_n = cdiv(Hg, TN);
    const long long tiles = (long long)cdiv(Ig, TM) * p.tiles_n;
    CRUSE_REQUIRE(tiles < (1ll << 31), CRUSE_E_SHAPE, "grouped_linear_bwd_dw: grid too large");
    hipLaunchKernelGGL(gl_dw_kernel, dim3((unsigned)tiles, G, p.parts), dim3(256), 0, (hipStream_t)stream, p);
    CRUSE_LAUNCH_CHECK("grouped_linear_bwd_dw");
    if (p.parts > 1) {
        const long long n = (long long)G * Ig * Hg + (db != nullptr ? (long long)G * Hg : 0);
        CRUSE_REQUIRE(cdivl(n, 256) < (1ll << 31), CRUSE_E_SHAPE, "grouped_linear_bwd_dw: grid too large");
        hipLaunchKernelGGL(gl_dw_reduce_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
        CRUSE_LAUNCH_CHECK("grouped_linear_bwd_dw (reduce)");
    }
    return CRUSE_OK;
}

extern "C" int cruse_band_pool(const float* x, const int* starts, int rows, int F, int n_bands, int mean, float* y, void* stream) {
    if (int rc = band_check("band_pool", x, starts, rows, F, n_bands, y)) return rc;
    const int vec = ((uintptr_t)x % 16) == 0 ? 1 : 0;
    hipLaunchKernelGGL(band_pool_kernel, dim3(cdiv(rows, BAND_ROWS)), dim3(256), (size_t)BAND_ROWS * F * sizeof(float), (hipStream_t)stream,
                       x, starts, rows, F, n_bands, mean ? 1 : 0, vec, y);
    CRUSE_LAUNCH_CHECK("band_pool");
    return CRUSE_OK;
}

extern "C" int cruse_band_expand(const float* m, const int* starts, int rows, int F, int n_bands, int mean, float* y, void* stream) {
    if (int rc = band_check("band_expand", m, starts, rows, F, n_bands, y)) return rc;
    const int vec = ((uintptr_t)y % 16) == 0 ? 1 : 0;
    const size_t lds = ((size_t)F + n_bands + (size_t)BAND_ROWS * n_bands) * sizeof(float);
    hipLaunchKernelGGL(band_expand_kernel, dim3(cdiv(rows, BAND_ROWS)), dim3(256), lds, (hipStream_t)stream,
                       m, starts, rows, F, n_bands, mean ? 1 : 0, vec, y);
    CRUSE_LAUNCH_CHECK("band_expand");
    return CRUSE_OK;
}
