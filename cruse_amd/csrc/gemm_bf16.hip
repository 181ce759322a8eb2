// bf16-operand MFMA GEMM for the GRU gate projections in CRUSE_PREC_BF16 mode (nn.GRU at
// model/cruse_net.py:23-31,44,50), plus the layout kernels that feed it:
//   C[M,N] (+)= A[M,K] . B[N,K]^T (+ bias[n])          A, B bf16 with K contiguous, C f32
// Every gate GEMM of the step is brought to this one NT form by keeping bf16 copies of the operands in the
// orientation the product needs (row-major for gi / dX, time-major transposes for the weight gradients):
//   gi     = x_bf   . W_ih_bf^T            dX     = dgi_bf . (W_ih^T)_bf^T
//   dW_ih += dgT    . (x^T)_bf^T           dW_hh += dgT    . (h_{t-1}^T)_bf^T
// The values are the same RNE-rounded bf16 operands the f32-input kernel in gemm.hip forms on the fly, so
// both kernels produce the same products; this one moves half the bytes and stages tiles with LDS-DMA.
//
// 128x128x64 block tile, 4 wavefronts as 2x2 (64x64 = 4x4 MFMA 16x16x32 tiles each), two LDS buffers filled by
// global_load_lds (16 B per lane, 1 KiB per wave instruction).  The LDS image of a tile is [128 rows][8 chunks
// of 16 B]; chunk c of row r sits at position c ^ (r & 7) -- the swizzle is applied on the per-lane global
// SOURCE address (the LDS-DMA destination is lane-linear) and undone in the fragment read address.
#include "common.h"
#include <stdlib.h>

extern "C" int cruse_cast_bf16_split(const float* x, void* y, void* y_lo, long long n, void* stream);

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;      // 16 KiB

typedef __attribute__((address_space(3))) void lds_ptr_t;
typedef const __attribute__((address_space(1))) void glb_ptr_t;

struct GbArgs {
    const __bf16* A; const __bf16* B; float* C; const float* bias;
    long long a_lo, b_lo;                    // element offsets of the LOW planes (split-bf16 x3 form), 0 = plain bf16
    int M, N, K;
    long long lda, ldb, ldc, a_ks, b_ks;     // *_ks: elements between consecutive 64-deep k-tiles of one row
    int accumulate, splitk, kt_chunk;
    int tiles_m, tiles_n, nunits, inner;
    int xcdk;                                // split-K with the k-slices PINNED to XCDs (see the kernel's tile order)
    long long slab;                          // MODE 4: elements between the partial-sum slabs of consecutive k-slices
    // ROW SEGMENTS on the M side: logical row m of A and C is physical row (m / seg_len) * seg_stride + seg_off + m % seg_len --
    // frames [seg_off, seg_off + seg_len) of every clip of a [B, T = seg_stride] tensor, i.e. a TIME CHUNK of the batch
    // (the gate projections of one chunk run beside the recurrence of the previous one).  seg_len == 0: identity.
    int seg_len; long long seg_stride, seg_off;
    // CONCATENATED products (cruse_gemm_bf16_nt_slabs_cat): row tiles [0, tm_b1) are product 0 (A, B as above), [tm_b1, tm_b2) product 1,
    // [tm_b2, ..) product 2 -- each with its own B operand and its own first A row (a_shift*: elements added to the A address of the
    // VIRTUAL row), all sharing N, K, the strides and one output [sum of the M_i, N].  tm_b1 = tm_b2 = INT_MAX: one product.
    int tm_b1, tm_b2; long long a_shift1, a_shift2; const __bf16* B1; const __bf16* B2;
    // (products whose M_i is not a multiple of 128 occupy whole row tiles all the same: m_end* = end of product's VIRTUAL rows -- rows past it are
    // computed and dropped --, c_rows* = output row of a virtual row minus that virtual row)
    int m_end0, m_end1, m_end2; int c_rows1, c_rows2;
    // GROUPS along N (cruse_gemm_bf16_nt_groups): the column tiles [q * tn_per_g, (q + 1) * tn_per_g) are product q -- N columns each, A columns
    // a_gstep further right, B / bias / C columns b_gstep / bias_gstep / c_gstep elements further on -- the GRU groups of one layer in ONE launch.
    int tn_per_g; long long a_gstep, b_gstep, c_gstep, bias_gstep;
    // ATR (cruse_gemm_bf16_nt_atr): A is read from its TIME-MAJOR K-tiled image -- element (m, k) at A[(m / 64) * a_mbs + k * 64 + m % 64], the
    // layout of the gate-gradient tensor dgT the weight-gradient GEMMs consume -- so the row-major copy dgi need not exist.  a_ks = 64 * 64.
    long long a_mbs; int a_mb_last;
    int c_f16;                               // MODE 3: the 2-byte result rows are IEEE f16 (0: bf16)
};

__device__ __forceinline__ long long seg_row(const GbArgs& g, int m) {
    if (g.seg_len == 0) return m;
    const int q = m / g.seg_len;
    return (long long)q * g.seg_stride + g.seg_off + (m - q * g.seg_len);
}

// ATR: one A fragment from the k-major LDS image (see the kernel's header) -- two transposing reads, k-rows 4 apart
__device__ __forceinline__ bf16x8 read_a_tr(const unsigned char* p) {
    typedef __attribute__((ext_vector_type(4))) short s16x4_;
    typedef __attribute__((address_space(3))) s16x4_ lds_s16x4;
    typedef __attribute__((ext_vector_type(8))) short s16x8_;
    const s16x4_ lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4_ hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * 128));
    const s16x8_ both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
}

// MODE: C update -- 0 store, 1 read-add-store, 2 atomic add (split-K), 3 store as bf16 (C is then a bf16 tensor, ldc in its elements),
// 4 split-K with every k-slice STORING its partial sums to its own slab C + tz * slab (summed by gemm_slab_reduce_kernel): the
// f32 atomics of MODE 2 from the 8 XCDs meet at the memory side -- 9.8 M of them per weight-gradient product, 0.14 ms per step.
// NST: LDS stages.  2 = one k-tile of prefetch, two blocks per CU (the short-K products, whose epilogues then
// overlap the other block's k-loop); 3 = two k-tiles in flight behind counted vmcnt waits and one raw barrier per
// k-tile, one block per CU (the split-K weight gradients: hundreds of k-tiles streamed once, where the k-loop is
// bound by the latency of the next tile's loads).
// (A 256 x 128 tile on 8 wavefronts and a pinned MFMA / LDS-read schedule were measured and not kept: DESIGN.md section 8.)
// F16: the operands are IEEE f16 (same bytes per element, same staging and fragment layout; v_mfma_f32_16x16x32_f16): the forward gate
// projection as ONE pass -- 11 significant bits on both operands against 8 + the W_ih low-plane pass of the split-bf16 form (cruse_gemm_f16_nt).
// ATR: the A tile is staged from a k-major source ([64 k][64 m] per 64-row block: 8 KB contiguous per block and k-tile, lane-linear LDS-DMA as
// ever) and its MFMA fragments are TRANSPOSING LDS reads: ds_read_b64_tr_b16 hands lane c of a 16-lane group the four k of column c of a [4 k][16 m]
// block whose rows the lanes 4 r .. 4 r + 3 address (measured, tools/probes/tr16_probe.hip) -- two reads per fragment.  The k-rows of the image are 128
// bytes (32 banks) apart, and a 32-lane service group reads rows {0..3} + 8 kg of one parity class each: the 16-byte chunks of row k are XOR-swizzled
// (on the global SOURCE address, as for the row-major image) by ((k >> 1 & 1) | (k >> 3 & 1) << 1) << 1, which puts the four same-parity rows of a
// group on four different 32-byte bank windows -- conflict-free.
template <int MODE, int NST, bool F16 = false, bool ATR = false>
__global__ __launch_bounds__(256, NST == 2 ? 2 : 1) void gemm_bf16_nt_kernel(const GbArgs g) {
    static_assert(!ATR || !F16, "transposed-A staging: bf16");
    constexpr int STAGE_BYTES = 2 * TILE_BYTES;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_dyn[];
    auto As_ = [&](int buf) -> unsigned char* { return smem_dyn + (size_t)buf * STAGE_BYTES; };            // [stage][A | B]
    auto Bs_ = [&](int buf) -> unsigned char* { return smem_dyn + (size_t)buf * STAGE_BYTES + TILE_BYTES; };
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    // XCD-aware tile order, as in gemm.hip: a unit -- the n-tiles of one m-tile, or with split-K the m-tiles of one
    // (k-slice, n-tile) -- stays on one XCD, so the operand panel its tiles share is fetched into that L2 once
    // xcdk (the K = 25 664 weight gradients): k-slice z is computed ENTIRELY on XCD z % 8 -- all its output tiles, m-major, so
    // the blocks resident on that XCD at one time walk the same k-range together and share every operand k-tile through
    // that XCD's L2: each operand byte leaves HBM about once.  (With (k-slice, n-tile) units spread round-robin the big
    // operand was fetched once per n-tile: 506 MB per launch for 131 MB of operands, PMC r01.)
    const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
    int tm, tn, tz;
    if (g.xcdk) {
        const int ntile = g.tiles_m * g.tiles_n;
        tz = (qq / ntile) * 8 + xcd;
        if (tz >= g.splitk) return;
        const int tl = qq % ntile;
        tm = tl / g.tiles_n; tn = tl % g.tiles_n;
    } else {
        const int inner = qq % g.inner, unit = (qq / g.inner) * 8 + xcd;
        if (unit >= g.nunits) return;
        if (g.splitk > 1) { tz = unit / g.tiles_n; tn = unit % g.tiles_n; tm = inner; }
        else { tz = 0; tm = unit; tn = inner; }
    }
    const int gq = g.tn_per_g > 0 ? tn / g.tn_per_g : 0;                  // product (GRU group) of this column tile
    if (g.tn_per_g > 0) tn -= gq * g.tn_per_g;
    const int m0 = tm * BM, n0 = tn * BN;
    const __bf16* Abase = g.A + gq * g.a_gstep;
    const __bf16* Bbase = g.B + gq * g.b_gstep;
    int m_lim = g.m_end0, c_sh = 0;
    if (tm >= g.tm_b2) { Abase += g.a_shift2; Bbase = g.B2; m_lim = g.m_end2; c_sh = g.c_rows2; }
    else if (tm >= g.tm_b1) { Abase += g.a_shift1; Bbase = g.B1; m_lim = g.m_end1; c_sh = g.c_rows1; }
    const int nkt = g.K / BK;
    const int kt0 = tz * g.kt_chunk, kt1 = min(nkt, kt0 + g.kt_chunk);
    // split-bf16 forms: the k-range is walked again on the same accumulators for every correction term -- (A_hi, B_lo)
    // when B has a low plane, (A_lo, B_hi) when A has one too -- as extra virtual k-tiles of ONE staging pipeline
    const int nreal = kt1 - kt0;
    const int nvirt = (g.b_lo ? (g.a_lo ? 3 : 2) : 1) * nreal;      // (hi,hi) [, (hi,lo) [, (lo,hi)]]

    // staging: wave wv fills rows [wv*32, wv*32+32) of the A tile and of the B tile, 8 rows (1 KiB) per instruction
    const __bf16* ap[4];
    const __bf16* bp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (ATR) {
            const int j = wv * 4 + i;                            // instruction j fills k-rows (j & 7) * 8 .. + 8 of 64-row block j >> 3
            const int krow = (j & 7) * 8 + (lane >> 3);
            const int ch = (lane & 7) ^ ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 1);
            const int mb = min(2 * tm + (j >> 3), g.a_mb_last);  // (rows past M: the last block again -- computed, never stored)
            ap[i] = Abase + (long long)mb * g.a_mbs + krow * 64 + ch * 8;
        } else {
            const int r = (wv * 4 + i) * 8 + (lane >> 3);
            const int ch = (lane & 7) ^ (lane >> 3);
            ap[i] = Abase + seg_row(g, min(m0 + r, m_lim - 1)) * g.lda + ch * 8;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wv * 4 + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ (lane >> 3);
        bp[i] = Bbase + (long long)min(n0 + r, g.N - 1) * g.ldb + ch * 8;
    }
    auto stage = [&](int v, int buf) {               // v: virtual k-tile index in [0, nvirt)
        const int seg = v >= 2 * nreal ? 2 : (v >= nreal ? 1 : 0);
        const int kt = kt0 + v - seg * nreal;
        const long long oa = (long long)kt * g.a_ks + (seg == 2 ? g.a_lo : 0);
        const long long ob = (long long)kt * g.b_ks + (seg == 1 ? g.b_lo : 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)(ap[i] + oa), (lds_ptr_t*)(As_(buf) + (wv * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)(bp[i] + ob), (lds_ptr_t*)(Bs_(buf) + (wv * 4 + i) * 1024), 16, 0, 0);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment byte offsets inside a tile: row (lane & 15) of each 16-row sub-tile, chunk kk*4 + (lane >> 4)
    int offa[2], offb[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int c = (kk * 4 + (lane >> 4)) ^ (lane & 7);
        offa[kk] = (wm * 64 + (lane & 15)) * 128 + c * 16;
        offb[kk] = (wn * 64 + (lane & 15)) * 128 + c * 16;
    }

    // ATR: byte offset of this lane's 8-byte piece for sub-tile i (k-row kg * 8 + q of the half (kk, h) added as a constant)
    int offt[4];
    if constexpr (ATR) {
        const int c15 = lane & 15, q = c15 >> 2, kg = lane >> 4;
        const int gsw = ((q >> 1) & 1) | ((kg & 1) << 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            offt[i] = wm * 8192 + (kg * 8 + q) * 128 + (((i ^ gsw) * 2 + ((c15 & 3) >> 1)) * 16) + (c15 & 1) * 8;
    }

    // one k-tile = two 32-deep halves of 16 MFMAs per wave
    auto compute = [&](int buf) {
        const unsigned char* As = As_(buf);
        const unsigned char* Bs = Bs_(buf);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (ATR) fa[i] = read_a_tr(As + offt[i] + kk * 32 * 128);
                else fa[i] = *reinterpret_cast<const bf16x8*>(As + offa[kk] + i * 16 * 128);
                fb[i] = *reinterpret_cast<const bf16x8*>(Bs + offb[kk] + i * 16 * 128);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if constexpr (F16) {
                        typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_, fa[i]), __builtin_bit_cast(f16x8_, fb[j]),
                                                                           acc[i][j], 0, 0, 0);
                    } else {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
                    }
        }
    };
    if constexpr (NST == 2) {
        if (nvirt > 0) stage(0, 0);
        for (int v = 0; v < nvirt; ++v) {
            const int buf = v & 1;
            __syncthreads();                   // tile v landed (vmcnt(0) + barrier); buffer buf^1 is free again
            if (v + 1 < nvirt) stage(v + 1, buf ^ 1);
            compute(buf);
        }
    } else {
        // each stage() is 8 LDS-DMA loads per wave, retired in order: vmcnt(8) == "all but the newest tile landed"
        if (nvirt > 0) stage(0, 0);
        if (nvirt > 1) stage(1, 1);
        int buf = 0;
        for (int v = 0; v < nvirt; ++v) {
            if (v + 1 < nvirt) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();      // tile v is in LDS for every wave; stage (v+2)%3 == (v-1)%3 is drained
            if (v + 2 < nvirt) stage(v + 2, buf == 0 ? 2 : buf - 1);
            compute(buf);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            buf = buf == 2 ? 0 : buf + 1;
        }
    }

    // epilogue: each wave turns its 64x64 accumulator block into row-contiguous float4 accesses through its own
    // 32 x 68-float LDS patch (two halves), so C is written in 256-byte row segments
    __syncthreads();                           // everyone is done with the operand tiles
    float* patch = reinterpret_cast<float*>(smem_dyn) + wv * (32 * 68);
    const bool add_bias = g.bias != nullptr && tz == 0;
    const int nq = n0 + wn * 64 + (lane & 15) * 4;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (add_bias) {
        const float* bias = g.bias + gq * g.bias_gstep;
        bv.x = nq < g.N ? bias[nq] : 0.f; bv.y = nq + 1 < g.N ? bias[nq + 1] : 0.f;
        bv.z = nq + 2 < g.N ? bias[nq + 2] : 0.f; bv.w = nq + 3 < g.N ? bias[nq + 3] : 0.f;
    }
    const bool vec = (g.ldc % 4 == 0) && (g.c_gstep % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 15) == 0) && nq + 3 < g.N;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    patch[(ii * 16 + (lane >> 4) * 4 + r) * 68 + j * 16 + (lane & 15)] = acc[half * 2 + ii][j][r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rr = p * 4 + (lane >> 4);
            const int m = m0 + wm * 64 + half * 32 + rr;
            float4 v = *reinterpret_cast<const float4*>(patch + rr * 68 + (lane & 15) * 4);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            if (m < m_lim) {
                if constexpr (MODE == 3) {                 // bf16 rows: 8-byte stores, 128-byte row segments
                    // (the two bodies below differ in the element type alone; written as one generic lambda they compile to other instructions)
                    __bf16* cb = reinterpret_cast<__bf16*>(g.C) + seg_row(g, m) * g.ldc + nq;
                    if (g.c_f16) {                          // (same rows, IEEE f16 elements: the gi rows cruse_gru_seq_fwd_gi16 reads)
                        _Float16* ch = reinterpret_cast<_Float16*>(cb);
                        if (nq + 3 < g.N && (g.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 7) == 0)) {
                            typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_;
                            const f16x4_ o = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
                            *reinterpret_cast<f16x4_*>(ch) = o;
                        } else {
                            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (nq + q < g.N) ch[q] = (_Float16)e[q];
                        }
                        continue;
                    }
                    if (nq + 3 < g.N && (g.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 7) == 0)) {
                        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_;
                        const bf16x4_ o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
                        *reinterpret_cast<bf16x4_*>(cb) = o;
                    } else {
                        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (nq + q < g.N) cb[q] = (__bf16)e[q];
                    }
                    continue;
                }
                float* c = g.C + (MODE == 4 ? (long long)tz * g.slab : 0ll) + (seg_row(g, m) + c_sh) * g.ldc + gq * g.c_gstep + nq;
                if (MODE == 2) {
                    if (nq < g.N) atomicAdd(c, v.x);
                    if (nq + 1 < g.N) atomicAdd(c + 1, v.y);
                    if (nq + 2 < g.N) atomicAdd(c + 2, v.z);
                    if (nq + 3 < g.N) atomicAdd(c + 3, v.w);
                } else if (vec) {
                    if (MODE == 1) {
                        const float4 o = *reinterpret_cast<const float4*>(c);
                        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                    }
                    *reinterpret_cast<float4*>(c) = v;
                } else {
                    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (nq + q < g.N) c[q] = (MODE == 1 ? c[q] : 0.f) + e[q];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// y = bf16(x), same layout; y_lo (optional) = bf16(x - y): the low plane of the split-bf16 x3 form
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* x, __bf16* y, __bf16* y_lo, long long n4) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16x4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h[e] = (__bf16)f[e]; l[e] = (__bf16)(f[e] - (float)h[e]); }
        reinterpret_cast<bf16x4*>(y)[i] = h;
        if (y_lo) reinterpret_cast<bf16x4*>(y_lo)[i] = l;
    }
}

// Time-major K-TILED transpose: element (c, r) of x^T lives at yT[(r/64)*cols*64 + c*64 + r%64], i.e. the 64-frame
// k-tile of every line is one 128-byte run and a whole k-tile of the operand is one contiguous block (a row-major
// [cols][ldT] image made every k-tile of a GEMM operand tile touch 128 pages 51 KB apart).  Values:
// bf16(x[r - shift][c]) for r < rows (0 where shift and r is the first frame of its clip), 0 for rows <= r < ldT.
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const float* x, long long rows, int cols, long long ld,
                                                             __bf16* yT, long long ldT, int shiftT) {
    __shared__ float tile[64][65];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    // in: 16-byte loads along the columns where the rows allow it (4 per thread), 4-byte ones otherwise
    const bool vec = (ld & 3) == 0 && (cols & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    if (vec) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = p * 256 + tid, rr = idx >> 4, c4 = (idx & 15) * 4;
            const long long r = r0 + rr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && c0 + c4 < cols) {
                if (shiftT == 0) v = *reinterpret_cast<const float4*>(x + r * ld + c0 + c4);
                else if (r % shiftT != 0) v = *reinterpret_cast<const float4*>(x + (r - 1) * ld + c0 + c4);
            }
            tile[rr][c4] = v.x; tile[rr][c4 + 1] = v.y; tile[rr][c4 + 2] = v.z; tile[rr][c4 + 3] = v.w;
        }
    } else {
        const int cc = tid & 63;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int rr = p * 4 + (tid >> 6);
            const long long r = r0 + rr;
            float v = 0.f;
            if (r < rows && c0 + cc < cols) {
                if (shiftT == 0) v = x[r * ld + c0 + cc];
                else if (r % shiftT != 0) v = x[(r - 1) * ld + c0 + cc];
            }
            tile[rr][cc] = v;
        }
    }
    __syncthreads();
    {
        // out: a lane writes 8 consecutive rows of one column = 16 bytes; 8 lanes cover the 128 bytes of a column's 64 rows
        typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_;
        const int j = tid & 7;                   // row group
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int cc = p * 32 + (tid >> 3);
            if (c0 + cc < cols) {
                bf16x8_ h;
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = (__bf16)tile[8 * j + e][cc];
                *reinterpret_cast<bf16x8_*>(yT + (r0 >> 6) * ((long long)cols * 64) + (long long)(c0 + cc) * 64 + 8 * j) = h;
            }
        }
    }
}

// K-tiling WITHOUT transposition: element (n, k) of x [rows n][cols k] goes to y[(k/64)*rows*64 + n*64 + k%64];
// k in [cols, kp) is zero-filled (kp = cols rounded up to 64) -- the K-contiguous operand whose K is not a
// multiple of 64 (W_ih with Hg = 160)
template <bool F16>
__global__ __launch_bounds__(256) void ktile_bf16_kernel(const float* x, int rows, int cols, long long ld, __bf16* y,
                                                         __bf16* y_lo, int kp) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    const int kq = kp >> 2;
    const long long n4 = (long long)rows * kq;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / kq), k = (int)(i - (long long)n * kq) * 4;
        const long long o = (long long)(k >> 6) * rows * 64 + (long long)n * 64 + (k & 63);
        if constexpr (F16) {                     // (y_lo: the low plane f16(x - f16(x)) of the two-pass form cruse_gemm_f16x2_nt)
            f16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float f = (k + e < cols) ? x[n * ld + k + e] : 0.f;
                h[e] = (_Float16)f; l[e] = (_Float16)(f - (float)h[e]);
            }
            *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(y) + o) = h;
            if (y_lo) *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(y_lo) + o) = l;
        } else {
            bf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float f = (k + e < cols) ? x[n * ld + k + e] : 0.f;
                h[e] = (__bf16)f; l[e] = (__bf16)(f - (float)h[e]);
            }
            *reinterpret_cast<bf16x4*>(y + o) = h;
            if (y_lo) *reinterpret_cast<bf16x4*>(y_lo + o) = l;
        }
    }
}

// C[m*ldc + n] += sum_z slabs[z*slab + m*N + n]: the k-slices' partial sums in a fixed order (run-to-run reproducible)
__global__ __launch_bounds__(256) void gemm_slab_reduce_kernel(const float* slabs, int nz, long long slab, int M, int N, float* C,
                                                               long long ldc) {
    const int nq = N >> 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * nq) return;
    const int m = (int)(i / nq), q = (int)(i - (long long)m * nq);
    const float* p = slabs + (long long)m * N + 4 * q;
    float4 s = *reinterpret_cast<const float4*>(p);
    for (int z = 1; z < nz; ++z) {
        const float4 v = *reinterpret_cast<const float4*>(p + (long long)z * slab);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float* c = C + (long long)m * ldc + 4 * q;
    c[0] += s.x; c[1] += s.y; c[2] += s.z; c[3] += s.w;
}

}  // namespace

namespace {

// One GEMM call, whichever of the ten entry points it came through.  The optional forms are nested members whose zero value means "absent";
// an entry point names the fields it uses and leaves the others out.
struct GbSeg { int len; long long stride, off; };                                   // row segments (GbArgs::seg_*); len == 0: none
struct GbSlabs { float* scratch; size_t bytes; };                                   // split-K partial sums stored, then summed in slice order
struct GbCat { int tm_b1, tm_b2; long long a_shift1, a_shift2; const __bf16* B1; const __bf16* B2; int m_end[3], c_rows[3], M_out; };   // M_out == 0: none
struct GbAtr { long long mb_stride; int mb_last; };                                 // time-major A (GbArgs::a_mbs); mb_stride == 0: none
struct GbGroups { int G; long long a_gstep, b_gstep, c_gstep, bias_gstep; };        // G == 0: none
struct GbCall {
    int M, N, K;
    const void* A; const void* A_lo; long long lda, a_kstride;
    const void* B; const void* B_lo; long long ldb, b_kstride;
    void* C; long long ldc; int c_dtype;                                            // CRUSE_DT_F32, or _F16 / _BF16 rows (stored, never accumulated)
    const float* bias; int accumulate, splitk; bool operands_f16; void* stream;
    GbSeg seg; GbSlabs slabs; GbCat cat; GbAtr atr; GbGroups grp;
};

// what a call launches, as cruse_gemm_bf16_plan reports it
enum { GB_P_MODE, GB_P_NST, GB_P_F16, GB_P_ATR, GB_P_GRID, GB_P_LDS, GB_P_SPLITK, GB_P_KT_CHUNK, GB_P_XCDK, GB_P_TILES_M, GB_P_TILES_N, GB_P_NUNITS,
       GB_P_INNER, GB_P_M_OUT, GB_P_SLAB, GB_P_REDUCE_GRID, GB_P_N };

struct GbVariant { int mode, nst; bool f16, atr; const char* name; };
constexpr int variant_key(int mode, int nst, bool f16 = false, bool atr = false) { return mode * 8 + (nst - 2) * 4 + (f16 ? 2 : 0) + (atr ? 1 : 0); }

// which of the 14 instantiated kernels a call takes.  deep (long k-loops): three stages, one block per CU -- the f16 and ATR forms stay on two
GbVariant gemm_variant(const GbCall& c, int splitk, int kt_chunk, bool use_slabs) {
    const bool out16 = c.c_dtype != CRUSE_DT_F32;
    const int nst = kt_chunk >= 64 ? 3 : 2;
    if (use_slabs) return {4, nst, false, false, "gemm_bf16_nt"};
    if (c.atr.mb_stride != 0) return {c.accumulate ? 1 : 0, 2, false, true, "gemm_bf16_nt_atr"};
    if (c.operands_f16) return {out16 ? 3 : 0, 2, true, false, out16 ? "gemm_nt_out16" : "gemm_f16_nt"};
    return {out16 ? 3 : splitk > 1 ? 2 : c.accumulate ? 1 : 0, nst, false, false, "gemm_bf16_nt"};
}

template <int MODE, int NST, bool F16 = false, bool ATR = false>
int gemm_launch(const GbArgs& g, unsigned nblk, size_t lds, hipStream_t st, const char* name) {
    const int rc = cruse_ensure_dyn_lds(reinterpret_cast<const void*>(gemm_bf16_nt_kernel<MODE, NST, F16, ATR>), lds, name);
    if (rc) return rc;
    hipLaunchKernelGGL((gemm_bf16_nt_kernel<MODE, NST, F16, ATR>), dim3(nblk), dim3(256), lds, st, g);
    CRUSE_LAUNCH_CHECK(name);
    return CRUSE_OK;
}

// The one host path of the ten entry points: admission, geometry, kernel selection and launch.
// plan != null (cruse_gemm_bf16_plan): decide the same way, write what would be launched and launch nothing.
int gemm_run(const GbCall& c, int* plan = nullptr) {
    const bool out16 = c.c_dtype != CRUSE_DT_F32, atr = c.atr.mb_stride != 0, cat = c.cat.M_out != 0;
    const int M = c.M, N = c.N, K = c.K;
    // ---- admission: the forms that exclude each other, then shape, strides and alignment
    CRUSE_REQUIRE(c.grp.G == 0 || (!out16 && !c.slabs.scratch && c.splitk == 1 && !cat && !atr && c.seg.len == 0 && c.a_kstride == BK), CRUSE_E_SHAPE,
                  "gemm_bf16_nt_groups: row-major A, f32 result, no split-K");
    CRUSE_REQUIRE(!atr || (!c.A_lo && !c.B_lo && !out16 && !c.slabs.scratch && c.splitk == 1 && !c.operands_f16 && !cat && c.seg.len == 0), CRUSE_E_SHAPE,
                  "gemm_bf16_nt_atr: plain bf16, one pass, no split-K");
    CRUSE_REQUIRE(!c.operands_f16 || (!c.A_lo && !c.slabs.scratch && c.splitk == 1 && !c.accumulate), CRUSE_E_SHAPE,
                  "gemm_f16_nt: f32 result stored (no A low plane, no split-K, no accumulation)");
    CRUSE_REQUIRE(!out16 || (!c.accumulate && c.splitk == 1), CRUSE_E_SHAPE, "gemm_bf16_nt: a bf16 result is stored, not accumulated");
    CRUSE_REQUIRE(c.seg.len >= 0 && (c.seg.len == 0 || (c.seg.stride >= c.seg.len && c.seg.off >= 0 && M % c.seg.len == 0 && c.a_kstride == BK)),
                  CRUSE_E_SHAPE, "gemm_bf16_nt: bad row segments (len %d stride %lld off %lld, M %d; row-major A only)", c.seg.len,
                  c.seg.stride, c.seg.off, M);
    CRUSE_REQUIRE(M > 0 && N > 0 && K > 0, CRUSE_E_SHAPE, "gemm_bf16_nt: empty shape M=%d N=%d K=%d", M, N, K);
    CRUSE_REQUIRE(K % BK == 0, CRUSE_E_SHAPE, "gemm_bf16_nt: K=%d must be a multiple of %d (pad with zeros)", K, BK);
    CRUSE_REQUIRE(c.a_kstride >= BK && c.b_kstride >= BK && c.ldc >= N, CRUSE_E_SHAPE, "gemm_bf16_nt: strides too small");
    CRUSE_REQUIRE((c.a_kstride == BK ? c.lda >= K : c.lda >= BK) && (c.b_kstride == BK ? c.ldb >= K : c.ldb >= BK), CRUSE_E_SHAPE,
                  "gemm_bf16_nt: lda=%lld / ldb=%lld too small for the operand layout", c.lda, c.ldb);
    CRUSE_REQUIRE(c.lda % 8 == 0 && c.ldb % 8 == 0 && c.a_kstride % 8 == 0 && c.b_kstride % 8 == 0, CRUSE_E_ALIGN,
                  "gemm_bf16_nt: operands need 16-byte aligned rows and k-tiles (strides multiples of 8)");
    CRUSE_REQUIRE(((uintptr_t)c.A % 16) == 0, CRUSE_E_ALIGN, "gemm_bf16_nt: A must be 16-byte aligned");
    CRUSE_REQUIRE(((uintptr_t)c.B % 16) == 0, CRUSE_E_ALIGN, "gemm_bf16_nt: B must be 16-byte aligned");
    // (the k-slices and the grid they make, on which the last checks rest: plain arithmetic, filled into GbArgs below)
    const int nkt = K / BK;
    const bool pinned = c.splitk < -1;         // negative: |splitk| k-slices pinned to XCDs
    int splitk = pinned ? -c.splitk : c.splitk;
    if (splitk < 1) splitk = 1;
    if (splitk > nkt) splitk = nkt;
    const int kt_chunk = cdiv(nkt, splitk);
    splitk = cdiv(nkt, kt_chunk);
    const int xcdk = (pinned && splitk > 1) ? 1 : 0;
    const int M_out = cat ? c.cat.M_out : M;   // rows of the output (cat: the products' rows without the tile padding between them)
    const int tiles_m = cdiv(M, BM), tiles_n = cdiv(N, BN) * (c.grp.G ? c.grp.G : 1);
    const int nunits = splitk > 1 ? splitk * tiles_n : tiles_m, inner = splitk > 1 ? tiles_m : tiles_n;
    const long long nblk = xcdk ? (long long)cdiv(splitk, 8) * 8 * tiles_m * tiles_n : (long long)cdiv(nunits, 8) * 8 * inner;
    const bool use_slabs = c.slabs.scratch != nullptr && splitk > 1;
    if (use_slabs) {                           // partial sums [slice][M][N] in the caller's scratch, then one ordered sum into C
        CRUSE_REQUIRE(N % 4 == 0 && c.seg.len == 0, CRUSE_E_ALIGN, "gemm_bf16_nt: slab form needs N %% 4 == 0");
        CRUSE_REQUIRE(((uintptr_t)c.slabs.scratch % 16) == 0, CRUSE_E_ALIGN, "gemm_bf16_nt: the slab scratch must be 16-byte aligned");
        CRUSE_REQUIRE((size_t)splitk * M_out * N * sizeof(float) <= c.slabs.bytes, CRUSE_E_SHAPE,
                      "gemm_bf16_nt: %d slabs of %d x %d floats do not fit the %zu-byte scratch", splitk, M_out, N, c.slabs.bytes);
        CRUSE_REQUIRE(c.bias == nullptr, CRUSE_E_SHAPE, "gemm_bf16_nt: slab form has no bias");
    }
    CRUSE_REQUIRE(nblk < (1ll << 31), CRUSE_E_SHAPE, "gemm_bf16_nt: grid too large");
    CRUSE_REQUIRE(splitk == 1 || c.accumulate, CRUSE_E_SHAPE, "gemm_bf16_nt: split-K adds into C (accumulate = 1)");

    // ---- geometry
    GbArgs g;
    g.A = (const __bf16*)c.A; g.B = (const __bf16*)c.B; g.C = (float*)c.C; g.bias = c.bias;
    g.a_lo = c.A_lo ? (const __bf16*)c.A_lo - g.A : 0;
    g.b_lo = c.B_lo ? (const __bf16*)c.B_lo - g.B : 0;
    g.M = M; g.N = N; g.K = K; g.lda = c.lda; g.ldb = c.ldb; g.ldc = c.ldc; g.a_ks = c.a_kstride; g.b_ks = c.b_kstride;
    g.accumulate = c.accumulate; g.splitk = splitk; g.kt_chunk = kt_chunk;
    g.tiles_m = tiles_m; g.tiles_n = tiles_n; g.nunits = nunits; g.inner = inner; g.xcdk = xcdk;
    g.seg_len = c.seg.len; g.seg_stride = c.seg.stride; g.seg_off = c.seg.off;
    g.a_mbs = c.atr.mb_stride; g.a_mb_last = c.atr.mb_last;
    g.c_f16 = c.c_dtype == CRUSE_DT_F16 ? 1 : 0;
    g.tn_per_g = c.grp.G ? tiles_n / c.grp.G : 0;
    g.a_gstep = c.grp.a_gstep; g.b_gstep = c.grp.b_gstep; g.c_gstep = c.grp.c_gstep; g.bias_gstep = c.grp.bias_gstep;
    g.tm_b1 = cat ? c.cat.tm_b1 : 0x7fffffff; g.tm_b2 = cat ? c.cat.tm_b2 : 0x7fffffff;
    g.a_shift1 = c.cat.a_shift1; g.a_shift2 = c.cat.a_shift2; g.B1 = c.cat.B1; g.B2 = c.cat.B2;
    g.m_end0 = cat ? c.cat.m_end[0] : M; g.m_end1 = cat ? c.cat.m_end[1] : M; g.m_end2 = cat ? c.cat.m_end[2] : M;
    g.c_rows1 = c.cat.c_rows[1]; g.c_rows2 = c.cat.c_rows[2];
    g.slab = 0;
    if (use_slabs) { g.C = c.slabs.scratch; g.ldc = N; g.slab = (long long)M_out * N; g.bias = nullptr; }
    const long long reduce_blk = use_slabs ? ((long long)M_out * (N / 4) + 255) / 256 : 0;

    // ---- selection and launch
    const GbVariant v = gemm_variant(c, splitk, kt_chunk, use_slabs);
    const size_t lds = (size_t)v.nst * 2 * TILE_BYTES;
    if (plan) {
        const int p[GB_P_N] = {v.mode, v.nst, v.f16, v.atr, (int)nblk, (int)lds, splitk, kt_chunk, xcdk, tiles_m, tiles_n, nunits, inner, M_out,
                               (int)g.slab, (int)reduce_blk};
        for (int i = 0; i < GB_P_N; ++i) plan[i] = p[i];
        return CRUSE_OK;
    }
    hipStream_t st = (hipStream_t)c.stream;
    const unsigned grid = (unsigned)nblk;
    int rc = CRUSE_OK;
    switch (variant_key(v.mode, v.nst, v.f16, v.atr)) {
        case variant_key(0, 2): rc = gemm_launch<0, 2>(g, grid, lds, st, v.name); break;
        case variant_key(0, 3): rc = gemm_launch<0, 3>(g, grid, lds, st, v.name); break;
        case variant_key(1, 2): rc = gemm_launch<1, 2>(g, grid, lds, st, v.name); break;
        case variant_key(1, 3): rc = gemm_launch<1, 3>(g, grid, lds, st, v.name); break;
        case variant_key(2, 2): rc = gemm_launch<2, 2>(g, grid, lds, st, v.name); break;
        case variant_key(2, 3): rc = gemm_launch<2, 3>(g, grid, lds, st, v.name); break;
        case variant_key(3, 2): rc = gemm_launch<3, 2>(g, grid, lds, st, v.name); break;
        case variant_key(3, 3): rc = gemm_launch<3, 3>(g, grid, lds, st, v.name); break;
        case variant_key(4, 2): rc = gemm_launch<4, 2>(g, grid, lds, st, v.name); break;
        case variant_key(4, 3): rc = gemm_launch<4, 3>(g, grid, lds, st, v.name); break;
        case variant_key(0, 2, false, true): rc = gemm_launch<0, 2, false, true>(g, grid, lds, st, v.name); break;
        case variant_key(1, 2, false, true): rc = gemm_launch<1, 2, false, true>(g, grid, lds, st, v.name); break;
        case variant_key(0, 2, true): rc = gemm_launch<0, 2, true>(g, grid, lds, st, v.name); break;
        case variant_key(3, 2, true): rc = gemm_launch<3, 2, true>(g, grid, lds, st, v.name); break;
        default: CRUSE_REQUIRE(false, CRUSE_E_SHAPE, "gemm_bf16_nt: no kernel for mode %d with %d stages", v.mode, v.nst);
    }
    if (rc || !use_slabs) return rc;
    hipLaunchKernelGGL(gemm_slab_reduce_kernel, dim3((unsigned)reduce_blk), dim3(256), 0, st, c.slabs.scratch, splitk, g.slab, M_out, N,
                       (float*)c.C, c.ldc);
    CRUSE_LAUNCH_CHECK("gemm_slab_reduce");
    return CRUSE_OK;
}

// what an entry point (form: CRUSE_GEMM_FORM_*) checks of its own arguments, then the path they share; cruse_gemm_bf16_plan comes the same way
int gemm_enter(int form, const GbCall& c, int* plan = nullptr) {
    const bool lo_aligned = ((uintptr_t)c.A_lo % 16) == 0 && ((uintptr_t)c.B_lo % 16) == 0;
    const int n_mb = c.atr.mb_last + 1;
    switch (form) {
    case CRUSE_GEMM_FORM_X3:
        CRUSE_REQUIRE(c.B_lo != nullptr && c.A_lo != c.A && c.B_lo != c.B, CRUSE_E_SHAPE, "gemm_bf16x3_nt: B_lo missing");
        CRUSE_REQUIRE(lo_aligned, CRUSE_E_ALIGN, "gemm_bf16x3_nt: unaligned low planes");
        break;
    case CRUSE_GEMM_FORM_F16X2:
        CRUSE_REQUIRE(c.B_lo != nullptr, CRUSE_E_SHAPE, "gemm_f16x2_nt: B_lo is required (one plane: cruse_gemm_f16_nt)");
        break;
    case CRUSE_GEMM_FORM_OUT16:
        CRUSE_REQUIRE(c.c_dtype == CRUSE_DT_F16 || c.c_dtype == CRUSE_DT_BF16, CRUSE_E_DTYPE, "gemm_nt_out16: out_dtype %d (CRUSE_DT_F16, CRUSE_DT_BF16)", c.c_dtype);
        CRUSE_REQUIRE((c.A_lo == nullptr || (c.B_lo != nullptr && !c.operands_f16)) && lo_aligned, CRUSE_E_ALIGN,
                      "gemm_nt_out16: low planes (A_lo needs B_lo and bf16 operands; 16-byte aligned)");
        break;
    case CRUSE_GEMM_FORM_ATR:
        CRUSE_REQUIRE(c.atr.mb_stride >= (long long)c.K * 64 && c.atr.mb_stride % 8 == 0 && n_mb >= 1 && (long long)n_mb * 64 >= c.M, CRUSE_E_SHAPE,
                      "gemm_bf16_nt_atr: a_mb_stride=%lld n_mb=%d for M=%d K=%d", c.atr.mb_stride, n_mb, c.M, c.K);
        break;
    case CRUSE_GEMM_FORM_GROUPS:
        CRUSE_REQUIRE(c.grp.G >= 1 && c.grp.a_gstep % 8 == 0 && c.grp.b_gstep % 8 == 0 && c.grp.c_gstep >= c.N &&
                      (long long)(c.grp.G - 1) * c.grp.c_gstep + c.N <= c.ldc, CRUSE_E_SHAPE,
                      "gemm_bf16_nt_groups: G=%d a_gstep=%lld b_gstep=%lld c_gstep=%lld", c.grp.G, c.grp.a_gstep, c.grp.b_gstep, c.grp.c_gstep);
        CRUSE_REQUIRE((c.A_lo == nullptr || c.B_lo != nullptr) && lo_aligned, CRUSE_E_ALIGN, "gemm_bf16_nt_groups: low planes (A_lo needs B_lo; 16-byte aligned)");
        break;
    case CRUSE_GEMM_FORM_SLABS:
        CRUSE_REQUIRE(c.slabs.scratch != nullptr, CRUSE_E_SHAPE, "gemm_bf16_nt_slabs: scratch is NULL");
        break;
    case CRUSE_GEMM_FORM_SEG:
        CRUSE_REQUIRE(c.seg.len > 0, CRUSE_E_SHAPE, "gemm_bf16_nt_seg: seg_len=%d", c.seg.len);
        CRUSE_REQUIRE((c.A_lo == nullptr || c.B_lo != nullptr) && lo_aligned, CRUSE_E_ALIGN, "gemm_bf16_nt_seg: low planes (A_lo needs B_lo; 16-byte aligned)");
        break;
    }
    return gemm_run(c, plan);
}

// cruse_gemm_bf16_nt_slabs_cat: c holds A (the whole tensor), the strides and the scratch; this checks the products and sets c.cat, M (the virtual
// rows: a product starts on a row tile, the rows that pad its last tile are computed and dropped) and A, B of product 0
int gemm_enter_cat(GbCall c, int nprob, const int* Ms, const long long* a_rows, const void* const* Bs, int* plan = nullptr) {
    CRUSE_REQUIRE(nprob >= 1 && nprob <= 3 && Ms && a_rows && Bs && c.slabs.scratch, CRUSE_E_SHAPE, "gemm_bf16_nt_slabs_cat: 1..3 products");
    GbCat& cat = c.cat;
    int tiles = 0, rows = 0, first[3] = {0, 0, 0};
    for (int i = 0; i < nprob; ++i) {
        CRUSE_REQUIRE(Ms[i] > 0 && a_rows[i] >= 0 && Bs[i] != nullptr && ((uintptr_t)Bs[i] % 16) == 0, CRUSE_E_SHAPE,
                      "gemm_bf16_nt_slabs_cat: product %d (M = %d)", i, Ms[i]);
        first[i] = tiles * BM;
        cat.m_end[i] = first[i] + Ms[i];
        cat.c_rows[i] = rows - first[i];
        tiles += cdiv(Ms[i], BM); rows += Ms[i];
    }
    cat.M_out = rows;
    cat.tm_b1 = nprob > 1 ? first[1] / BM : 0x7fffffff; cat.tm_b2 = nprob > 2 ? first[2] / BM : 0x7fffffff;
    // virtual row m of product i is A row a_rows[i] + (m - first[i]); the kernel adds m * lda itself
    cat.a_shift1 = nprob > 1 ? (a_rows[1] - a_rows[0] - first[1]) * c.lda : 0;
    cat.a_shift2 = nprob > 2 ? (a_rows[2] - a_rows[0] - first[2]) * c.lda : 0;
    cat.B1 = nprob > 1 ? (const __bf16*)Bs[1] : nullptr; cat.B2 = nprob > 2 ? (const __bf16*)Bs[2] : nullptr;
    CRUSE_REQUIRE(c.a_kstride > BK, CRUSE_E_SHAPE, "gemm_bf16_nt_slabs_cat: K-tiled A operand (rows lda apart inside a k-tile)");
    c.A = (const __bf16*)c.A + a_rows[0] * c.lda; c.B = Bs[0]; c.M = first[nprob - 1] + Ms[nprob - 1];
    return gemm_run(c, plan);
}

}  // namespace

// The ten entry points (include/cruse_hip.h says what each computes): each names the descriptor fields its argument list carries.
extern "C" int cruse_gemm_bf16_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride, const void* B, long long ldb, long long b_kstride,
                                  float* C, long long ldc, const float* bias, int accumulate, int splitk, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_PLAIN, {.M = M, .N = N, .K = K, .A = A, .lda = lda, .a_kstride = a_kstride, .B = B, .ldb = ldb, .b_kstride = b_kstride,
                                              .C = C, .ldc = ldc, .bias = bias, .accumulate = accumulate, .splitk = splitk, .stream = stream});
}

// B = B_hi + B_lo (two f16 planes, same layout), the second k-range on the same accumulators: the rounding of W_ih is the same in every frame and
// does not average out of the gradients the way the per-frame rounding of x does
extern "C" int cruse_gemm_f16x2_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride,
                                   const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                                   float* C, long long ldc, const float* bias, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_F16X2, {.M = M, .N = N, .K = K, .A = A, .lda = lda, .a_kstride = a_kstride, .B = B_hi, .B_lo = B_lo, .ldb = ldb,
                                              .b_kstride = b_kstride, .C = C, .ldc = ldc, .bias = bias, .splitk = 1, .operands_f16 = true, .stream = stream});
}

// a 2-byte result (f16 or bf16 rows): the f32 accumulation of the entry points above, rounded once at the store
extern "C" int cruse_gemm_nt_out16(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda, long long a_kstride,
                                   const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                                   void* C, long long ldc, const float* bias, int operands_f16, int out_dtype, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_OUT16, {.M = M, .N = N, .K = K, .A = A_hi, .A_lo = A_lo, .lda = lda, .a_kstride = a_kstride, .B = B_hi, .B_lo = B_lo,
                                              .ldb = ldb, .b_kstride = b_kstride, .C = C, .ldc = ldc, .c_dtype = out_dtype, .bias = bias, .splitk = 1,
                                              .operands_f16 = operands_f16 != 0, .stream = stream});
}

extern "C" int cruse_gemm_f16_nt(int M, int N, int K, const void* A, long long lda, long long a_kstride, const void* B, long long ldb, long long b_kstride,
                                 float* C, long long ldc, const float* bias, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_F16, {.M = M, .N = N, .K = K, .A = A, .lda = lda, .a_kstride = a_kstride, .B = B, .ldb = ldb, .b_kstride = b_kstride,
                                            .C = C, .ldc = ldc, .bias = bias, .splitk = 1, .operands_f16 = true, .stream = stream});
}

// A given as its TIME-MAJOR K-tiled image (GbArgs::a_mbs), n_mb 64-row blocks present (rows M <= m < 64 * n_mb hold finite values): the layout of
// the gate-gradient tensor dgT [ceil(rows / 64)][G][4][Hg][64] (A_T = dgT + group * 4 * Hg * 64, a_mb_stride = G * 4 * Hg * 64)
extern "C" int cruse_gemm_bf16_nt_atr(int M, int N, int K, const void* A_T, long long a_mb_stride, int n_mb, const void* B, long long ldb, long long b_kstride,
                                      float* C, long long ldc, int accumulate, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_ATR, {.M = M, .N = N, .K = K, .A = A_T, .lda = 64, .a_kstride = 64 * 64, .B = B, .ldb = ldb, .b_kstride = b_kstride,
                                            .C = C, .ldc = ldc, .accumulate = accumulate, .splitk = 1, .stream = stream, .atr = {a_mb_stride, n_mb - 1}});
}

// G products of the same shape in ONE launch, side by side along N (GbArgs::tn_per_g) -- the GRU groups of a layer, which were G launches of
// [rows x 3 Hg or Hg] each: 2 to 4 column tiles, 400 to 800 blocks
extern "C" int cruse_gemm_bf16_nt_groups(int M, int N, int K, int G, const void* A_hi, const void* A_lo, long long lda, long long a_gstep,
                                         const void* B_hi, const void* B_lo, long long ldb, long long b_kstride, long long b_gstep,
                                         float* C, long long ldc, long long c_gstep, const float* bias, long long bias_gstep, int accumulate, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_GROUPS, {.M = M, .N = N, .K = K, .A = A_hi, .A_lo = A_lo, .lda = lda, .a_kstride = BK, .B = B_hi, .B_lo = B_lo, .ldb = ldb,
                                               .b_kstride = b_kstride, .C = C, .ldc = ldc, .bias = bias, .accumulate = accumulate, .splitk = 1,
                                               .stream = stream, .grp = {G, a_gstep, b_gstep, c_gstep, bias_gstep}});
}

extern "C" size_t cruse_gemm_bf16_slab_bytes(int M, int N, int splitk) {
    const int z = splitk < 0 ? -splitk : splitk;
    return (size_t)(z < 1 ? 1 : z) * M * N * sizeof(float);
}

extern "C" int cruse_gemm_bf16_nt_slabs(int M, int N, int K, const void* A, long long lda, long long a_kstride, const void* B, long long ldb, long long b_kstride,
                                        float* C, long long ldc, int splitk, void* scratch, size_t scratch_bytes, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_SLABS, {.M = M, .N = N, .K = K, .A = A, .lda = lda, .a_kstride = a_kstride, .B = B, .ldb = ldb, .b_kstride = b_kstride,
                                              .C = C, .ldc = ldc, .accumulate = 1, .splitk = splitk, .stream = stream,
                                              .slabs = {reinterpret_cast<float*>(scratch), scratch_bytes}});
}

// Up to three slab products that share N, K, the operand strides and the A tensor, concatenated along M into ONE launch and one output -- the three
// weight-gradient products of a GRU layer: one launch walks all 150 output tiles of a k-slice on its XCD, the gate-gradient k-tiles are fetched once
// for the three products, and two launches + two reduce passes with their ramps and tails go
extern "C" int cruse_gemm_bf16_nt_slabs_cat(int nprob, const int* Ms, int N, int K, const void* A, const long long* a_rows, long long lda,
                                            long long a_kstride, const void* const* Bs, long long ldb, long long b_kstride,
                                            float* C, long long ldc, int splitk, void* scratch, size_t scratch_bytes, void* stream) {
    return gemm_enter_cat({.N = N, .K = K, .A = A, .lda = lda, .a_kstride = a_kstride, .ldb = ldb, .b_kstride = b_kstride, .C = C, .ldc = ldc, .accumulate = 1,
                           .splitk = splitk, .stream = stream, .slabs = {reinterpret_cast<float*>(scratch), scratch_bytes}}, nprob, Ms, a_rows, Bs);
}

extern "C" int cruse_gemm_bf16_nt_seg(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda,
                                      const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                                      float* C, long long ldc, const float* bias, int accumulate,
                                      int seg_len, long long seg_stride, long long seg_off, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_SEG, {.M = M, .N = N, .K = K, .A = A_hi, .A_lo = A_lo, .lda = lda, .a_kstride = BK, .B = B_hi, .B_lo = B_lo, .ldb = ldb,
                                            .b_kstride = b_kstride, .C = C, .ldc = ldc, .bias = bias, .accumulate = accumulate, .splitk = 1, .stream = stream,
                                            .seg = {seg_len, seg_stride, seg_off}});
}

extern "C" int cruse_gemm_bf16x3_nt(int M, int N, int K, const void* A_hi, const void* A_lo, long long lda, long long a_kstride,
                                    const void* B_hi, const void* B_lo, long long ldb, long long b_kstride,
                                    float* C, long long ldc, const float* bias, int accumulate, void* stream) {
    return gemm_enter(CRUSE_GEMM_FORM_X3, {.M = M, .N = N, .K = K, .A = A_hi, .A_lo = A_lo, .lda = lda, .a_kstride = a_kstride, .B = B_hi, .B_lo = B_lo,
                                           .ldb = ldb, .b_kstride = b_kstride, .C = C, .ldc = ldc, .bias = bias, .accumulate = accumulate, .splitk = 1,
                                           .stream = stream});
}

// Host-only (no device is touched): what a call of this form and these scalars would launch (include/cruse_hip.h) -- the entry point's own checks and
// gemm_run's decision, with the launches left out.  A static buffer stands for every tensor: never dereferenced.
extern "C" int cruse_gemm_bf16_plan(int form, int M, int N, int K, long long lda, long long a_kstride, long long ldb, long long b_kstride, long long ldc,
                                    int planes, int has_bias, int accumulate, int splitk, int operands_f16, int out_dtype, const long long* x, int* out) {
    CRUSE_REQUIRE(out != nullptr && form >= 0 && form < CRUSE_GEMM_FORM_N && (x != nullptr || form < CRUSE_GEMM_FORM_ATR), CRUSE_E_SHAPE,
                  "gemm_bf16_plan: out is NULL, form = %d, or the form's extras are missing", form);
    alignas(16) static unsigned char buf[80];
    const int off = (planes & 4) ? 2 : 0;
    const bool slab_form = form == CRUSE_GEMM_FORM_SLABS || form == CRUSE_GEMM_FORM_SLABS_CAT;
    GbCall c = {.M = M, .N = N, .K = K, .A = buf, .A_lo = (planes & 1) ? buf + 16 + off : nullptr, .lda = lda, .a_kstride = a_kstride,
                .B = buf + 32, .B_lo = (planes & 2) ? buf + 48 + off : nullptr, .ldb = ldb, .b_kstride = b_kstride, .C = buf, .ldc = ldc,
                .c_dtype = form == CRUSE_GEMM_FORM_OUT16 ? out_dtype : CRUSE_DT_F32, .bias = has_bias ? reinterpret_cast<const float*>(buf) : nullptr,
                .accumulate = slab_form ? 1 : accumulate, .splitk = splitk,
                .operands_f16 = operands_f16 != 0 || form == CRUSE_GEMM_FORM_F16 || form == CRUSE_GEMM_FORM_F16X2};
    for (int i = 0; i < GB_P_N; ++i) out[i] = 0;
    if (slab_form) c.slabs = {reinterpret_cast<float*>(buf), (size_t)x[0]};
    if (form == CRUSE_GEMM_FORM_ATR) { c.lda = 64; c.a_kstride = 64 * 64; c.atr = {x[0], (int)x[1] - 1}; }
    if (form == CRUSE_GEMM_FORM_GROUPS) { c.a_kstride = BK; c.grp = {(int)x[0], x[1], x[2], x[3], x[4]}; }
    if (form == CRUSE_GEMM_FORM_SEG) { c.a_kstride = BK; c.seg = {(int)x[0], x[1], x[2]}; }
    if (form != CRUSE_GEMM_FORM_SLABS_CAT) return gemm_enter(form, c, out);
    const int Ms[3] = {(int)x[2], (int)x[3], (int)x[4]};
    const void* const Bs[3] = {buf + 32, buf + 32, buf + 32};
    return gemm_enter_cat(c, (int)x[1], Ms, x + 5, Bs, out);
}

extern "C" int cruse_cast_bf16(const float* x, void* y, long long n, void* stream) {
    return cruse_cast_bf16_split(x, y, nullptr, n, stream);
}

extern "C" int cruse_cast_bf16_split(const float* x, void* y, void* y_lo, long long n, void* stream) {
    CRUSE_REQUIRE(n > 0 && n % 4 == 0, CRUSE_E_SHAPE, "cast_bf16: n=%lld must be a positive multiple of 4", n);
    CRUSE_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 8) == 0 && ((uintptr_t)y_lo % 8) == 0, CRUSE_E_ALIGN,
                  "cast_bf16: x must be 16-byte, y and y_lo 8-byte aligned");
    long long nb = (n / 4 + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y, (__bf16*)y_lo, n / 4);
    CRUSE_LAUNCH_CHECK("cast_bf16");
    return CRUSE_OK;
}

extern "C" int cruse_transpose_bf16(const float* x, long long rows, int cols, long long ld, void* yT, long long ldT,
                                    int shift_T, void* stream) {
    CRUSE_REQUIRE(rows > 0 && cols > 0 && ld >= cols, CRUSE_E_SHAPE, "transpose_bf16: bad shape");
    CRUSE_REQUIRE(ldT % 64 == 0 && ldT >= rows, CRUSE_E_SHAPE,
                  "transpose_bf16: ldT=%lld must be a multiple of 64 and >= rows=%lld", ldT, rows);
    CRUSE_REQUIRE(((uintptr_t)yT % 16) == 0, CRUSE_E_ALIGN, "transpose_bf16: yT must be 16-byte aligned");
    CRUSE_REQUIRE(shift_T >= 0 && (shift_T == 0 || rows % shift_T == 0), CRUSE_E_SHAPE,
                  "transpose_bf16: rows must be whole clips of shift_T frames");
    dim3 grid((unsigned)(ldT / 64), (unsigned)cdiv(cols, 64));
    hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, rows, cols, ld, (__bf16*)yT,
                       ldT, shift_T);
    CRUSE_LAUNCH_CHECK("transpose_bf16");
    return CRUSE_OK;
}

extern "C" int cruse_ktile_bf16(const float* x, int rows, int cols, long long ld, void* y, void* y_lo, void* stream) {
    CRUSE_REQUIRE(rows > 0 && cols > 0 && ld >= cols, CRUSE_E_SHAPE, "ktile_bf16: bad shape");
    CRUSE_REQUIRE(((uintptr_t)y % 8) == 0 && ((uintptr_t)y_lo % 8) == 0, CRUSE_E_ALIGN, "ktile_bf16: y and y_lo must be 8-byte aligned");
    const int kp = (cols + 63) / 64 * 64;
    long long nb = ((long long)rows * (kp / 4) + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(ktile_bf16_kernel<false>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, x, rows, cols, ld, (__bf16*)y,
                       (__bf16*)y_lo, kp);
    CRUSE_LAUNCH_CHECK("ktile_bf16");
    return CRUSE_OK;
}

// the same K-tiled layout with IEEE-f16 elements (the B operand of cruse_gemm_f16_nt)
static int ktile_f16_impl(const float* x, int rows, int cols, long long ld, void* y, void* y_lo, void* stream) {
    CRUSE_REQUIRE(rows > 0 && cols > 0 && ld >= cols, CRUSE_E_SHAPE, "ktile_f16: bad shape");
    CRUSE_REQUIRE(((uintptr_t)y % 8) == 0 && ((uintptr_t)y_lo % 8) == 0, CRUSE_E_ALIGN, "ktile_f16: y and y_lo must be 8-byte aligned");
    const int kp = (cols + 63) / 64 * 64;
    long long nb = ((long long)rows * (kp / 4) + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(ktile_bf16_kernel<true>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, x, rows, cols, ld, (__bf16*)y,
                       (__bf16*)y_lo, kp);
    CRUSE_LAUNCH_CHECK("ktile_f16");
    return CRUSE_OK;
}
extern "C" int cruse_ktile_f16(const float* x, int rows, int cols, long long ld, void* y, void* stream) {
    return ktile_f16_impl(x, rows, cols, ld, y, nullptr, stream);
}
extern "C" int cruse_ktile_f16_split(const float* x, int rows, int cols, long long ld, void* y, void* y_lo, void* stream) {
    CRUSE_REQUIRE(y_lo != nullptr, CRUSE_E_SHAPE, "ktile_f16_split: y_lo is required");
    return ktile_f16_impl(x, rows, cols, ld, y, y_lo, stream);
}

