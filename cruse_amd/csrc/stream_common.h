// Shared pieces of the streaming kernels (stream.hip: f32 chain; stream_f16.hip: f16-operand MFMA GRU): the packet schedule, the
// "does this slot compute a frame" test, the launch arguments / row addressing / argument checks of the GRU entry points, and the
// sample-format checks of the boundary kernels and the resamplers (stream_rs.hip).
#pragma once
#include "common.h"

namespace cruse_stream {

__device__ __forceinline__ bool mode_computes_frame(int m) {
    return m == CRUSE_STREAM_MODE_FRAME || m == CRUSE_STREAM_MODE_FRAME0 || m == CRUSE_STREAM_MODE_END;
}

// ---- the packet schedule: what slot s does with pk[s] = start (0: the slot holds no block, 1: one block, 2: two or more) and
// pk[S + s] = count of blocks it consumes.  Every packet kernel asks this one function which frames exist.
struct Pkt {
    int c;       // blocks consumed
    int nf;      // frames computed
    int f0;      // 1: the first frame is frame 0 of the clip (its output block is dropped)
    int hist;    // 1: the stored block comes first in the sequence of blocks
};

__device__ __forceinline__ Pkt packet_of(const int* __restrict__ pk, int S, int s, int hops) {
    const int start = min(max(pk[s], 0), 2), c = min(max(pk[S + s], 0), hops);
    Pkt p;
    p.c = c;
    p.hist = start >= 1;
    p.f0 = start <= 1;
    p.nf = c == 0 ? 0 : start == 0 ? (c >= 2 ? c : 0) : start == 1 ? c + 1 : c;
    return p;
}

// ---- one GGRU layer over R rows.  STEP: one time step of the single-hop chain, row = slot.  PROJ: the input products of every
// (slot, frame) of a packet.  REC: one recurrent step (frame `frame`) of a packet, row = slot.
enum { KIND_STEP = 0, KIND_PROJ = 1, KIND_REC = 2 };

struct GruArgs {
    const int* ctl;                 // STEP: mode[S]; PROJ / REC: pk[2][S]
    int R, S, hops, NFW, frame;     // rows; PROJ: R = S * (hops + 1), row r is frame r % (hops + 1) of slot r / (hops + 1)
    int g, Hg;
    const float* x;                 // input rows: x + row * x_stride + x_off (STEP, PROJ)
    long long x_stride;
    int x_off;
    const float* ln_g;              // LN1 over the interleaved input row (layer 2), or null
    const float* ln_b;
    float ln_eps;
    const float* h;                 // previous h rows (STEP, REC)
    long long h_stride;
    int h_off;
    const float* pack;              // f32 pack of the layer: W_ih | W_hh | b_ih | b_hh
    float* out;                     // new h rows (STEP, REC)
    long long o_stride;
    int o_off;
    float* gi;                      // [.., 3H] input products: written by PROJ, read by REC
    long long gi_stride;
};

// index of row r (< R) into the row arrays
template <int KIND>
__device__ __forceinline__ long long row_index(const GruArgs& a, int r) {
    if (KIND != KIND_PROJ) return r;
    const int nfc = a.hops + 1, s = r / nfc;
    return (long long)s * a.NFW + (r - s * nfc);
}

// does row r (< R) compute anything; rr: row_index
template <int KIND>
__device__ __forceinline__ bool row_of(const GruArgs& a, int r, long long& rr) {
    rr = row_index<KIND>(a, r);
    if (KIND == KIND_STEP) return mode_computes_frame(a.ctl[r]);
    if (KIND == KIND_PROJ) {
        const int nfc = a.hops + 1, s = r / nfc;
        return r - s * nfc < packet_of(a.ctl, a.S, s, a.hops).nf;
    }
    return a.frame < packet_of(a.ctl, a.S, r, a.hops).nf;
}

// ---- host: the argument checks of the GRU entry points (`who` names the entry point in the message), filling GruArgs.  The f32 and
// the f16 entry point of a kind share one of these; every refusal comes before any launch.
inline int gru_shape_args(const char* who, int S, int g, int Hg) {
    CRUSE_REQUIRE(S > 0 && g > 0 && Hg > 0 && Hg % 4 == 0 && Hg <= 1024, CRUSE_E_SHAPE,
                  "%s: S = %d, g = %d, Hg = %d (need S >= 1, g >= 1, Hg %% 4 == 0, Hg <= 1024)", who, S, g, Hg);
    return CRUSE_OK;
}

inline int gru_packet_args(const char* who, int S, int hops, int work_frames, int g, int Hg) {
    CRUSE_REQUIRE(hops >= 1 && work_frames >= hops + 1, CRUSE_E_SHAPE, "%s: hops = %d, work_frames = %d (need hops >= 1, work_frames >= hops + 1)",
                  who, hops, work_frames);
    return gru_shape_args(who, S, g, Hg);
}

inline int gru_step_args(const char* who, const int* mode, int S, int layer, int g, int Hg, const float* x, int x_stride, int x_off,
                         const float* ln_g, const float* ln_b, float ln_eps, const float* hprev, int h_stride, int h_off,
                         const float* pack, float* hout, int o_stride, int o_off, GruArgs& a) {
    const int rc = gru_shape_args(who, S, g, Hg);
    if (rc) return rc;
    CRUSE_REQUIRE(layer == 1 || layer == 2, CRUSE_E_SHAPE, "%s: layer %d", who, layer);
    CRUSE_REQUIRE(x_off >= 0 && x_off + g * Hg <= x_stride && h_off >= 0 && h_off + g * Hg <= h_stride && o_off >= 0 &&
                  o_off + g * Hg <= o_stride, CRUSE_E_SHAPE, "%s: x_off %d / h_off %d / o_off %d + %d floats outside rows of %d / %d / %d",
                  who, x_off, h_off, o_off, g * Hg, x_stride, h_stride, o_stride);
    CRUSE_REQUIRE(mode && x && hprev && pack && hout && (layer == 1 || (ln_g && ln_b)), CRUSE_E_SHAPE, "%s: null buffer", who);
    a.ctl = mode; a.R = S; a.S = S; a.g = g; a.Hg = Hg;
    a.x = x; a.x_stride = x_stride; a.x_off = x_off;
    a.ln_g = layer == 2 ? ln_g : nullptr; a.ln_b = layer == 2 ? ln_b : nullptr; a.ln_eps = ln_eps;
    a.h = hprev; a.h_stride = h_stride; a.h_off = h_off;
    a.pack = pack;
    a.out = hout; a.o_stride = o_stride; a.o_off = o_off;
    return CRUSE_OK;
}

inline int gru_proj_args(const char* who, const int* pk, int S, int hops, int work_frames, int layer, int g, int Hg, const float* work,
                         int wk_stride, int x_off, const float* ln_g, const float* ln_b, float ln_eps, const float* pack, float* gi,
                         GruArgs& a) {
    const int rc = gru_packet_args(who, S, hops, work_frames, g, Hg);
    if (rc) return rc;
    CRUSE_REQUIRE(layer == 1 || layer == 2, CRUSE_E_SHAPE, "%s: layer %d", who, layer);
    CRUSE_REQUIRE(x_off >= 0 && x_off + g * Hg <= wk_stride, CRUSE_E_SHAPE, "%s: x_off %d + %d floats outside a work row of %d", who, x_off,
                  g * Hg, wk_stride);
    CRUSE_REQUIRE((long long)S * (hops + 1) <= 0x7fffffffLL, CRUSE_E_SHAPE, "%s: S * (hops + 1) overflows", who);
    CRUSE_REQUIRE(pk && work && pack && gi && (layer == 1 || (ln_g && ln_b)), CRUSE_E_SHAPE, "%s: null buffer", who);
    a.ctl = pk; a.R = S * (hops + 1); a.S = S; a.hops = hops; a.NFW = work_frames; a.g = g; a.Hg = Hg;
    a.x = work; a.x_stride = wk_stride; a.x_off = x_off;
    a.ln_g = layer == 2 ? ln_g : nullptr; a.ln_b = layer == 2 ? ln_b : nullptr; a.ln_eps = ln_eps;
    a.pack = pack;
    a.gi = gi; a.gi_stride = (long long)3 * g * Hg;
    return CRUSE_OK;
}

inline int gru_rec_args(const char* who, const int* pk, int S, int hops, int work_frames, int frame, int g, int Hg, const float* gi,
                        const float* state, int st_stride, int st_off, const float* pack, float* work, int wk_stride, int h_off,
                        GruArgs& a) {
    const int rc = gru_packet_args(who, S, hops, work_frames, g, Hg);
    if (rc) return rc;
    CRUSE_REQUIRE(frame >= 0 && frame <= hops, CRUSE_E_SHAPE, "%s: frame %d outside [0, %d]", who, frame, hops);
    CRUSE_REQUIRE(st_off >= 0 && st_off + g * Hg <= st_stride && h_off >= 0 && h_off + g * Hg <= wk_stride, CRUSE_E_SHAPE,
                  "%s: st_off %d / h_off %d + %d floats outside a state row of %d / work row of %d", who, st_off, h_off, g * Hg, st_stride,
                  wk_stride);
    CRUSE_REQUIRE(pk && gi && state && pack && work, CRUSE_E_SHAPE, "%s: null buffer", who);
    a.ctl = pk; a.R = S; a.S = S; a.hops = hops; a.NFW = work_frames; a.frame = frame; a.g = g; a.Hg = Hg;
    // h comes from the state row for the packet's first frame, else from the previous frame's work row
    const long long slot = (long long)work_frames * wk_stride;       // floats between two slots' work rows of one frame
    if (frame == 0) { a.h = state; a.h_stride = st_stride; a.h_off = st_off; }
    else { a.h = work + (size_t)(frame - 1) * wk_stride; a.h_stride = slot; a.h_off = h_off; }
    a.pack = pack;
    a.out = work + (size_t)frame * wk_stride; a.o_stride = slot; a.o_off = h_off;
    a.gi = const_cast<float*>(gi) + (size_t)frame * 3 * g * Hg; a.gi_stride = (long long)work_frames * 3 * g * Hg;
    return CRUSE_OK;
}

// ---- host: the sample formats of the I/O forms (in_fmt / out_fmt of the header: the boundary kernels of stream.hip, the resamplers of
// stream_rs.hip) and their checks
enum { FMT_F32 = 0, FMT_S16 = 1 };

inline int fmt_args(const char* who, int fmt) {
    CRUSE_REQUIRE(fmt == FMT_F32 || fmt == FMT_S16, CRUSE_E_SHAPE, "%s: unknown sample format %d (0: f32, 1: s16)", who, fmt);
    return CRUSE_OK;
}

// the clamp counter belongs to PCM output: f32 output is never clamped
inline int out_args(const char* who, int out_fmt, const int* clip) {
    const int rc = fmt_args(who, out_fmt);
    if (rc) return rc;
    CRUSE_REQUIRE(out_fmt == FMT_S16 || clip == nullptr, CRUSE_E_SHAPE, "%s: a clip counter needs s16 output (out_fmt 1), got out_fmt %d", who, out_fmt);
    return CRUSE_OK;
}

}  // namespace cruse_stream
