// Per-slot level meters and voice activity at the end of a streaming chain (cruse_stream_meter / _meter_n).  The kernels
// follow cruse_stream_decode / _decode_n and read nothing but what the chain leaves in a frame's work row: the noisy spectrum N (161 bins
// at wk_re / wk_im) and the raw mask m (160 bins at wk_mask).  stream.hip is neither included nor changed.
//
// For every computed frame of a slot:
//   G_f      the gain the decode kernels apply (their gain line restated with the same header, postfilter.h):
//            no limit: G_f = pf(m_f) on bins 0..159, G_160 = 0; with lim[s]: G_f = lim + (1 - lim) pf(m_f), G_160 = lim
//   P_in     (|N_0|^2 + 2 sum_{f=1..159} |N_f|^2 + |N_160|^2) / (320 W2),  W2 = sum_n win[n]^2: the mean square of the frame's samples by
//            Parseval on the windowed frame;  P_out: the same of G_f N_f
//   L        10 log10(P + 1e-12) dBFS (silence: -120)
//   p        p_prev + alpha (p_raw - p_prev), p_raw = 1 / (1 + exp(-(L_out - level_db))), alpha = attack where p_raw > p_prev, else release
//   vad      p > threshold
// vad_par[s] = level_db, threshold, attack, release.  The frame writes the row [L_in, L_out, p, vad] and adds to the slot's accumulators
// (f64: frames, active frames, sum of P_in and of P_out over active frames).  Frame 0 of a clip resets p_prev and the accumulators, takes
// part in the recursion and yields neither a row nor a count: its block lies in front of the clip.
//
// One workgroup per slot, no atomics.  A frame's two sums are f32 and have one order in both forms: the bins in three segments of 64,
// each summed by the xor tree of wave_sum, the segments added in ascending order; floating-point contraction is off in every function
// here (the fused multiply-adds are written out), so that the compiler rounds both kernels' copies of a step alike.  So a frame has the
// same bits from the single-hop and from the packet kernel, and a slot's accumulators do not depend on how its frames were grouped
// into calls.
#include <cstring>
#include "postfilter.h"
#include "stream_common.h"

namespace {

using namespace cruse_stream;

// restated from stream.hip, which stays as it is: the frame, its bins, the window's place in the table of cruse_stream_tables
constexpr int NFFT = 320, NB = 161, F0 = 160;
constexpr int TB_WIN = 0;
constexpr int NSEG = (NB + 63) / 64;                      // segments of 64 bins
constexpr int METER_THREADS = 64 * NSEG;                  // single hop: one wave per segment
constexpr int METER_N_THREADS = 256;                      // packets: one wave per frame, cycling
constexpr int METER_MAX_HOPS = 64;                        // bounds the LDS rows of the packet kernel; above every packet layout's bound
constexpr int METER_ROW = 4, METER_ACC = 4;

// the layout of cruse_stream_meter_layout(): all ints, in the order of the header's description
struct MeterLayout {
    int p, stride, acc, row;
};
static_assert(sizeof(MeterLayout) == CRUSE_STREAM_METER_LAYOUT_INTS * sizeof(int), "meter layout size");

void make_meter_layout(MeterLayout& M) {
    M.p = 0;
    M.stride = 4;                                         // p_prev, then three floats of padding: rows stay 16-byte aligned
    M.acc = METER_ACC;
    M.row = METER_ROW;
}

struct MeterArgs {
    const int* ctl;            // single hop: mode[S]; packets: pk[2][S]
    int S, hops, NFW;          // packets: hops >= 1, work rows per slot
    const float* work;         // slot 0's first row
    int WS, re, im, mask;      // floats between two frames' rows; offsets in a row
    const float* tab;
    const float* lim;          // [S] or null
    int pf_kind;               // 0: no post-filter
    const float* pf_tau;       // [S] (pf_kind != 0)
    const float* vad_par;      // [S][4]
    float* state;              // [S][SS]
    int SS, p_off;
    double* acc;               // [S][4]
    float* out;                // rows of slot s from out + s * OS
    int OS;
};

// the gain line of the decode kernels for slot s
struct Gain {
    bool lim, pf;
    float lm, tau;
    int kind;
    __device__ __forceinline__ float operator()(float m, int f) const {
#pragma clang fp contract(off)
        if (f >= F0) return lim ? lm : 0.f;               // bin 160: the mask is zero there, a limit keeps lim of the input
        float g = m;
        if (pf) g = cruse_pf::post_filter(g, tau, kind);
        return lim ? fmaf(1.0f - lm, g, lm) : g;
    }
};

__device__ __forceinline__ Gain gain_of(const MeterArgs& a, int s) {
    Gain g;
    g.lim = a.lim != nullptr;
    g.pf = a.pf_kind != 0;
    g.lm = g.lim ? a.lim[s] : 0.f;
    g.tau = g.pf ? a.pf_tau[s] : 0.f;
    g.kind = a.pf_kind;
    return g;
}

// segment q of a row, by one wave: the weighted sums of |N_f|^2 and |G_f N_f|^2 over bins 64 q .. 64 q + 63 (below 161)
__device__ __forceinline__ void segment_power(const float* __restrict__ row, const MeterArgs& a, const Gain& G, int q, int lane, float& sin,
                                              float& sout) {
#pragma clang fp contract(off)
    const int f = 64 * q + lane;
    float ti = 0.f, to = 0.f;
    if (f < NB) {
        const float re = row[a.re + f], im = row[a.im + f];
        const float g = G(f < F0 ? row[a.mask + f] : 0.f, f);
        const float er = re * g, ei = im * g;             // what decode hands to the inverse DFT
        const float w = (f == 0 || f == F0) ? 1.0f : 2.0f;
        ti = w * fmaf(re, re, im * im);
        to = w * fmaf(er, er, ei * ei);
    }
    sin = wave_sum(ti);
    sout = wave_sum(to);
}

// W2 = sum of the squared window, by one wave
__device__ __forceinline__ float window_power(const float* __restrict__ tab, int lane) {
#pragma clang fp contract(off)
    float v = 0.f;
    for (int n = lane; n < NFFT; n += 64) v = fmaf(tab[TB_WIN + n], tab[TB_WIN + n], v);
    return wave_sum(v);
}

// what one lane carries through a slot's frames
struct MeterSlot {
    float p;
    double n, na, pin, pout;
};

// one step of the recursion on a frame's two sums; row: where the frame's meter row goes (not written for frame 0 of a clip)
__device__ __forceinline__ void meter_step(MeterSlot& m, float sin, float sout, float scale, const float* __restrict__ par, bool f0,
                                           float* __restrict__ row) {
#pragma clang fp contract(off)
    if (f0) { m.p = 0.f; m.n = m.na = m.pin = m.pout = 0.0; }           // whatever the state held
    const float pin = sin * scale, pout = sout * scale;
    const float lin = 10.0f * log10f(pin + 1e-12f), lout = 10.0f * log10f(pout + 1e-12f);
    const float praw = 1.0f / (1.0f + expf(-(lout - par[0])));
    const float alpha = praw > m.p ? par[2] : par[3];
    m.p = fmaf(alpha, praw - m.p, m.p);
    if (f0) return;
    const bool v = m.p > par[1];
    row[0] = lin; row[1] = lout; row[2] = m.p; row[3] = v ? 1.0f : 0.0f;
    m.n += 1.0;
    if (v) { m.na += 1.0; m.pin += (double)pin; m.pout += (double)pout; }
}

__device__ __forceinline__ MeterSlot load_slot(const MeterArgs& a, int s) {
    const double* c = a.acc + (size_t)s * METER_ACC;
    return {a.state[(size_t)s * a.SS + a.p_off], c[0], c[1], c[2], c[3]};
}

__device__ __forceinline__ void store_slot(const MeterArgs& a, int s, const MeterSlot& m) {
    double* c = a.acc + (size_t)s * METER_ACC;
    a.state[(size_t)s * a.SS + a.p_off] = m.p;
    c[0] = m.n; c[1] = m.na; c[2] = m.pin; c[3] = m.pout;
}

__global__ void __launch_bounds__(METER_THREADS) stream_meter_kernel(MeterArgs a) {
#pragma clang fp contract(off)
    __shared__ float red[NSEG][2];
    const int s = blockIdx.x, m = a.ctl[s];
    if (!mode_computes_frame(m)) return;                  // SKIP / STORE: row, state and accumulators untouched
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Gain G = gain_of(a, s);
    float si, so;
    segment_power(a.work + (size_t)s * a.WS, a, G, q, lane, si, so);
    if (lane == 0) { red[q][0] = si; red[q][1] = so; }
    float w2 = 0.f;
    if (q == 0) w2 = window_power(a.tab, lane);
    __syncthreads();
    if (threadIdx.x != 0) return;
    si = red[0][0]; so = red[0][1];
#pragma unroll
    for (int k = 1; k < NSEG; ++k) { si += red[k][0]; so += red[k][1]; }
    MeterSlot ms = load_slot(a, s);
    meter_step(ms, si, so, 1.0f / ((float)NFFT * w2), a.vad_par + 4 * (size_t)s, m == CRUSE_STREAM_MODE_FRAME0, a.out + (size_t)s * a.OS);
    store_slot(a, s, ms);
}

__global__ void __launch_bounds__(METER_N_THREADS) stream_meter_n_kernel(MeterArgs a) {
#pragma clang fp contract(off)
    __shared__ float pw[METER_MAX_HOPS + 1][2];
    const int s = blockIdx.x;
    const Pkt p = packet_of(a.ctl, a.S, s, a.hops);       // nf <= hops + 1 <= min(work_frames, METER_MAX_HOPS + 1): checked on the host
    if (p.nf == 0) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Gain G = gain_of(a, s);
    const float* rows = a.work + (size_t)s * a.NFW * a.WS;
    for (int fr = wv; fr < p.nf; fr += METER_N_THREADS / 64) {          // the frames' sums are independent: side by side
        float si = 0.f, so = 0.f;
#pragma unroll
        for (int q = 0; q < NSEG; ++q) {
            float ti, to;
            segment_power(rows + (size_t)fr * a.WS, a, G, q, lane, ti, to);
            si = q ? si + ti : ti;
            so = q ? so + to : to;
        }
        if (lane == 0) { pw[fr][0] = si; pw[fr][1] = so; }
    }
    float w2 = 0.f;
    if (wv == 0) w2 = window_power(a.tab, lane);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float scale = 1.0f / ((float)NFFT * w2);
    MeterSlot ms = load_slot(a, s);
    float* out = a.out + (size_t)s * a.OS;
    // frame 0 of a clip yields no row: at most nf - f0 <= hops rows, from index 0
    int j = 0;
    for (int fr = 0; fr < p.nf; ++fr) {
        const bool f0 = fr == 0 && p.f0;
        meter_step(ms, pw[fr][0], pw[fr][1], scale, a.vad_par + 4 * (size_t)s, f0, out + (size_t)j * METER_ROW);
        j += !f0;
    }
    store_slot(a, s, ms);
}

int meter_any(const char* who, bool packet, int out_hops, MeterArgs a, void* stream) {
    CRUSE_REQUIRE(a.S >= 1, CRUSE_E_SHAPE, "%s: S = %d (need S >= 1)", who, a.S);
    CRUSE_REQUIRE(a.ctl && a.work && a.tab && a.vad_par && a.state && a.acc && a.out, CRUSE_E_SHAPE, "%s: null buffer", who);
    CRUSE_REQUIRE(a.WS >= 2 * NB + F0 && a.re >= 0 && a.re + NB <= a.WS && a.im >= 0 && a.im + NB <= a.WS && a.mask >= 0 &&
                  a.mask + F0 <= a.WS, CRUSE_E_SHAPE,
                  "%s: wk_re %d / wk_im %d (+ %d) / wk_mask %d (+ %d) do not lie in a work row of %d floats (>= %d)", who, a.re, a.im, NB,
                  a.mask, F0, a.WS, 2 * NB + F0);
    if (a.pf_kind != 0) {
        const int rc = cruse_pf::kind_args(who, a.pf_kind);
        if (rc) return rc;
        CRUSE_REQUIRE(a.pf_tau, CRUSE_E_SHAPE, "%s: null buffer (pf_kind %d needs pf_tau)", who, a.pf_kind);
    }
    MeterLayout M;
    make_meter_layout(M);
    a.p_off = M.p;
    CRUSE_REQUIRE(a.SS >= M.stride, CRUSE_E_SHAPE, "%s: meter_state rows of %d floats, the layout needs %d", who, a.SS, M.stride);
    if (packet) {
        CRUSE_REQUIRE(a.hops >= 1 && a.hops <= METER_MAX_HOPS && a.NFW >= a.hops + 1 && out_hops >= a.hops, CRUSE_E_SHAPE,
                      "%s: hops = %d (1..%d), work_frames = %d (>= hops + 1), out_hops = %d (>= hops)", who, a.hops, METER_MAX_HOPS, a.NFW,
                      out_hops);
        CRUSE_REQUIRE(a.OS >= METER_ROW * out_hops, CRUSE_E_SHAPE, "%s: out rows of %d floats, %d meter rows need %d", who, a.OS, out_hops,
                      METER_ROW * out_hops);
    } else {
        CRUSE_REQUIRE(a.OS >= METER_ROW, CRUSE_E_SHAPE, "%s: out rows of %d floats, a meter row needs %d", who, a.OS, METER_ROW);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (packet) hipLaunchKernelGGL(stream_meter_n_kernel, dim3(a.S), dim3(METER_N_THREADS), 0, st, a);
    else hipLaunchKernelGGL(stream_meter_kernel, dim3(a.S), dim3(METER_THREADS), 0, st, a);
    CRUSE_LAUNCH_CHECK(who);
    return CRUSE_OK;
}

}  // namespace

extern "C" int cruse_stream_meter_layout(int* out) {
    CRUSE_REQUIRE(out, CRUSE_E_SHAPE, "stream_meter_layout: null output");
    MeterLayout M;
    make_meter_layout(M);
    memcpy(out, &M, sizeof(M));
    return CRUSE_OK;
}

extern "C" int cruse_stream_meter(const int* mode, int S, const float* work, int wk_stride, int wk_re, int wk_im, int wk_mask,
                                  const float* tab, const float* lim, int pf_kind, const float* pf_tau, const float* vad_par,
                                  float* meter_state, int st_stride, double* meter_acc, float* out, int out_stride, void* stream) {
    return meter_any("cruse_stream_meter", false, 0, {mode, S, 0, 1, work, wk_stride, wk_re, wk_im, wk_mask, tab, lim, pf_kind, pf_tau, vad_par,
                                                      meter_state, st_stride, 0, meter_acc, out, out_stride}, stream);
}

extern "C" int cruse_stream_meter_n(const int* pk, int S, int hops, int out_hops, int work_frames, const float* work, int wk_stride,
                                    int wk_re, int wk_im, int wk_mask, const float* tab, const float* lim, int pf_kind, const float* pf_tau,
                                    const float* vad_par, float* meter_state, int st_stride, double* meter_acc, float* out, int out_stride,
                                    void* stream) {
    return meter_any("cruse_stream_meter_n", true, out_hops, {pk, S, hops, work_frames, work, wk_stride, wk_re, wk_im, wk_mask, tab, lim, pf_kind,
                                                              pf_tau, vad_par, meter_state, st_stride, 0, meter_acc, out, out_stride}, stream);
}
