// f16-operand MFMA variants of the three streaming GRU kernels of stream.hip (cruse_stream_gru_f16 / _gru_proj_n_f16 / _gru_rec_n_f16),
// for servers with many slots.  State / work rows, `mode` and `pk` semantics are those of stream.hip, so encode / decode are shared.
//
// Per group the step is a [3*Hg x Hg] . [Hg x rows] product on v_mfma_f32_16x16x32_f16: the weights are the A operand (a wave owns 16
// hidden units and all three gates), a tile of 16 rows (slots, or (slot, frame) pairs in the packet projection) is the B operand, staged
// in LDS as f16 with K fastest so that a fragment is one 16-byte read.  What is rounded to f16: the operand copies of x (after LN1 for
// layer 2), of h, and the weights.  Accumulation, biases, LayerNorm statistics, sigmoid / tanh and every row another kernel reads are f32;
// the gate math reads h_prev in f32 from its row.
//
// Weights: one packed f16 buffer per layer, [ih | hh][group][gate][unit tile][k step][lane][8], i.e. each (unit tile, k step) is the
// 1 KB A fragment of a wave in lane order; units padded with zeros to a multiple of 16 and K to a multiple of 32.  A wave re-reads its
// fragments from L2 for every pass over NT row tiles (holding them in registers across tiles is impossible at Hg = 640; a layer's
// pack is 1.2 MB at the default shape and stays in L2).  Measurements: DESIGN 12b.
#include <algorithm>
#include "stream_common.h"

namespace {

using namespace cruse_stream;

// workgroups of a launch before its columns stride over the row tiles (two per CU).  A first choice: not swept
constexpr int GRID_WG = 512;

struct Args : GruArgs {
    const _Float16* pack16;
    int Kp, UT;                     // K padded to 32, unit tiles of 16
};

template <int KIND, int NT>
__global__ void __launch_bounds__(256) stream_gru_f16_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    constexpr int RT = NT * 16;
    constexpr bool HAS_X = KIND != KIND_REC, HAS_H = KIND != KIND_PROJ;
    const int Hg = a.Hg, g = a.g, H = g * Hg, Kp = a.Kp, LDW = Kp + 8, KS = Kp / 32;
    _Float16* xs = (_Float16*)smraw;                                 // [RT][LDW]
    _Float16* hs = xs + (HAS_X ? RT * LDW : 0);                      // [RT][LDW]
    float* st = (float*)(hs + (HAS_H ? RT * LDW : 0));               // [RT][2] mean, rstd
    int* ok = (int*)(st + 2 * RT);                                   // [RT] the row computes
    long long* rix = (long long*)(ok + RT);                          // [RT] its index into the row arrays
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int UB = (a.UT + 3) / 4;
    const int gidx = blockIdx.y / UB, ut = (blockIdx.y - gidx * UB) * 4 + wv;
    const bool active = ut < a.UT;
    const bool ln = HAS_X && a.ln_g != nullptr;
    const size_t gsz = (size_t)3 * Hg * Hg;
    const float* bih = a.pack + 2 * g * gsz + (size_t)gidx * 3 * Hg;
    const float* bhh = bih + (size_t)g * 3 * Hg;
    // this lane's four units (accumulator layout: column = row of the tile l & 15, units (l >> 4) * 4 + reg)
    const int u0 = ut * 16 + (lane >> 4) * 4;
    const bool uok = active && u0 < Hg;                              // Hg % 4 == 0: all four or none
    float br[4], bz[4], bni[4], bnh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = u0 + i;
        br[i] = bz[i] = bni[i] = bnh[i] = 0.f;
        if (uok) {
            if (KIND == KIND_STEP) { br[i] = bih[u] + bhh[u]; bz[i] = bih[Hg + u] + bhh[Hg + u]; bni[i] = bih[2 * Hg + u]; bnh[i] = bhh[2 * Hg + u]; }
            if (KIND == KIND_PROJ) { br[i] = bih[u] + bhh[u]; bz[i] = bih[Hg + u] + bhh[Hg + u]; bni[i] = bih[2 * Hg + u]; }
            if (KIND == KIND_REC) bnh[i] = bhh[2 * Hg + u];
        }
    }
    // A fragments of this wave: [m][g][3][UT][KS][64][8]
    const size_t tile = (size_t)KS * 64 * 8;
    const f16x8_t* Aih = (const f16x8_t*)(a.pack16 + ((size_t)(gidx * 3) * a.UT + (active ? ut : 0)) * tile) + lane;
    const f16x8_t* Ahh = (const f16x8_t*)(a.pack16 + ((size_t)((g + gidx) * 3) * a.UT + (active ? ut : 0)) * tile) + lane;
    const size_t gate = (size_t)a.UT * KS * 64;                      // fragments between two gates
    const int ntiles = (a.R + RT - 1) / RT;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int r0 = t * RT;
        __syncthreads();
        if (tid < RT) {
            long long rr = 0;
            const int r = r0 + tid;
            const bool v = r < a.R && row_of<KIND>(a, r, rr);
            ok[tid] = v;
            rix[tid] = rr;
        }
        __syncthreads();
        if (ln) {                                                    // LN1 statistics of each input row (two passes, biased variance)
            for (int ss = wv; ss < RT; ss += 4) {
                if (!ok[ss]) continue;
                const float* row = a.x + rix[ss] * a.x_stride + a.x_off;
                float s1 = 0.f;
                for (int k = lane; k < H; k += 64) s1 += row[k];
                const float mean = wave_sum(s1) / H;
                float s2 = 0.f;
                for (int k = lane; k < H; k += 64) { const float d = row[k] - mean; s2 = fmaf(d, d, s2); }
                const float var = wave_sum(s2) / H;
                if (lane == 0) { st[2 * ss] = mean; st[2 * ss + 1] = 1.0f / sqrtf(var + a.ln_eps); }
            }
            __syncthreads();
        }
        // operands, rounded to f16; zeros in the K padding and in rows that compute nothing (never read out of bounds)
        if (HAS_X) {
            for (int i = tid; i < RT * Kp; i += 256) {
                const int ss = i / Kp, k = i - ss * Kp;
                float v = 0.f;
                if (k < Hg && ok[ss]) {
                    const float* row = a.x + rix[ss] * a.x_stride + a.x_off;
                    if (ln) {                                        // v[j*g + i] = h1[i*Hg + j], then LN1
                        const int p = gidx * Hg + k;
                        v = fmaf((row[(p % g) * Hg + p / g] - st[2 * ss]) * st[2 * ss + 1], a.ln_g[p], a.ln_b[p]);
                    } else {
                        v = row[gidx * Hg + k];
                    }
                }
                xs[ss * LDW + k] = (_Float16)v;
            }
        }
        if (HAS_H) {
            for (int i = tid; i < RT * Kp; i += 256) {
                const int ss = i / Kp, k = i - ss * Kp;
                float v = 0.f;
                if (k < Hg && ok[ss]) v = a.h[rix[ss] * a.h_stride + a.h_off + gidx * Hg + k];
                hs[ss * LDW + k] = (_Float16)v;
            }
        }
        __syncthreads();
        if (!active) continue;
        f32x4 ar[NT], az[NT], ani[NT], anh[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) ar[n] = az[n] = ani[n] = anh[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int boff = (lane & 15) * LDW + (lane >> 4) * 8;
        for (int ks = 0; ks < KS; ++ks) {
            Frag<CRUSE_PREC_F16> wi[3], wh[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (HAS_X) wi[c].h = Aih[c * gate + (size_t)ks * 64];
                if (HAS_H) wh[c].h = Ahh[c * gate + (size_t)ks * 64];
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                Frag<CRUSE_PREC_F16> bx, bh;
                if (HAS_X) {
                    bx.h = *(const f16x8_t*)(xs + n * 16 * LDW + boff + ks * 32);
                    ar[n] = mma(wi[0], bx, ar[n]);
                    az[n] = mma(wi[1], bx, az[n]);
                    ani[n] = mma(wi[2], bx, ani[n]);
                }
                if (HAS_H) {
                    bh.h = *(const f16x8_t*)(hs + n * 16 * LDW + boff + ks * 32);
                    ar[n] = mma(wh[0], bh, ar[n]);
                    az[n] = mma(wh[1], bh, az[n]);
                    anh[n] = mma(wh[2], bh, anh[n]);
                }
            }
        }
        if (!uok) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int ss = n * 16 + (lane & 15);
            if (!ok[ss]) continue;                                   // rows beyond R and rows that compute no frame: masked at the store
            const long long rr = rix[ss];
            const int u = gidx * Hg + u0;                            // unit of the whole layer
            if (KIND == KIND_PROJ) {
                float* o = a.gi + rr * a.gi_stride + u;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = ar[n][i] + br[i];
                    o[H + i] = az[n][i] + bz[i];
                    o[2 * H + i] = ani[n][i] + bni[i];
                }
                continue;
            }
            const float* hp = a.h + rr * a.h_stride + a.h_off + u;
            float* o = a.out + rr * a.o_stride + a.o_off + u;
            const float* gv = KIND == KIND_REC ? a.gi + rr * a.gi_stride + u : nullptr;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float pr = ar[n][i] + br[i], pz = az[n][i] + bz[i], pn = ani[n][i] + bni[i];
                if (KIND == KIND_REC) { pr += gv[i]; pz += gv[H + i]; pn = gv[2 * H + i]; }
                const float r = 1.0f / (1.0f + expf(-pr));
                const float z = 1.0f / (1.0f + expf(-pz));
                const float nn = tanhf(pn + r * (anh[n][i] + bnh[i]));
                o[i] = (1.0f - z) * nn + z * hp[i];
            }
        }
    }
}

template <int KIND, int NT>
int launch(const Args& a, const char* name, hipStream_t st) {
    constexpr int RT = NT * 16;
    const int mats = KIND == KIND_STEP ? 2 : 1;
    const size_t lds = (size_t)mats * RT * (a.Kp + 8) * sizeof(_Float16) + RT * (2 * sizeof(float) + sizeof(int) + sizeof(long long));
    int rc = cruse_ensure_dyn_lds((const void*)stream_gru_f16_kernel<KIND, NT>, lds, name);
    if (rc) return rc;
    // workgroup columns stride over the row tiles once the grid covers the device a few times over
    const int by = a.g * ((a.UT + 3) / 4), ntiles = (a.R + RT - 1) / RT;
    const int grid_x = std::max(1, std::min(ntiles, (GRID_WG + by - 1) / by));
    hipLaunchKernelGGL((stream_gru_f16_kernel<KIND, NT>), dim3(grid_x, by), dim3(256), lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        cruse_set_error("%s: HIP launch failed: %s", name, hipGetErrorString(e));
        return CRUSE_E_HIP;
    }
    return CRUSE_OK;
}

// Two row tiles per pass (half the weight traffic) where there are rows for them and the padded K is <= 512.  Dynamic LDS is
// mats * RT * (Kp + 8) * 2 + RT * 20 bytes: at most 67,200 B for the step kernel with two tiles at Kp = 512 and 66,368 B with one tile
// at Kp = 1024.  Both are ABOVE 64 KB: they rely on the 160 KB of LDS per CU of gfx950 (cruse_ensure_dyn_lds raises the limit) and leave
// two workgroups per CU by LDS; a 64 KB part needs other thresholds.  The thresholds (R > 16, Kp <= 512) are first choices, not swept.
template <int KIND>
int dispatch(Args& a, const void* pack16, const char* name, hipStream_t st) {
    CRUSE_REQUIRE(pack16, CRUSE_E_SHAPE, "%s: null pack16", name);
    a.pack16 = (const _Float16*)pack16;
    a.Kp = (a.Hg + 31) & ~31;
    a.UT = (a.Hg + 15) / 16;
    if (a.R > 16 && a.Kp <= 512) return launch<KIND, 2>(a, name, st);
    return launch<KIND, 1>(a, name, st);
}

}  // namespace

extern "C" int cruse_stream_gru_f16(const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                                    const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                                    const float* pack, const void* pack16, float* hout, int o_stride, int o_off, void* stream) {
    Args a = {};
    const int rc = gru_step_args("stream_gru_f16", mode, S, layer, g, Hg, x, x_stride, x_off, ln_g, ln_b, ln_eps, hprev, h_stride, h_off,
                                 pack, hout, o_stride, o_off, a);
    return rc ? rc : dispatch<KIND_STEP>(a, pack16, "cruse_stream_gru_f16", (hipStream_t)stream);
}

extern "C" int cruse_stream_gru_proj_n_f16(const int* pk, int S, int hops, int work_frames, int layer, int g, int Hg, const float* work,
                                           int wk_stride, int x_off, const float* ln_g, const float* ln_b, float ln_eps, const float* pack,
                                           const void* pack16, float* gi, void* stream) {
    Args a = {};
    const int rc = gru_proj_args("stream_gru_proj_n_f16", pk, S, hops, work_frames, layer, g, Hg, work, wk_stride, x_off, ln_g, ln_b,
                                 ln_eps, pack, gi, a);
    return rc ? rc : dispatch<KIND_PROJ>(a, pack16, "cruse_stream_gru_proj_n_f16", (hipStream_t)stream);
}

extern "C" int cruse_stream_gru_rec_n_f16(const int* pk, int S, int hops, int work_frames, int frame, int g, int Hg, const float* gi,
                                          const float* state, int st_stride, int st_off, const float* pack, const void* pack16,
                                          float* work, int wk_stride, int h_off, void* stream) {
    Args a = {};
    const int rc = gru_rec_args("stream_gru_rec_n_f16", pk, S, hops, work_frames, frame, g, Hg, gi, state, st_stride, st_off, pack, work,
                                wk_stride, h_off, a);
    return rc ? rc : dispatch<KIND_REC>(a, pack16, "cruse_stream_gru_rec_n_f16", (hipStream_t)stream);
}
