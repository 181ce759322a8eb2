"""Frame-by-frame streaming inference of unet_2: 160-sample blocks in, 160-sample enhanced blocks out, 20 ms behind.

The offline path (base_inferencer.Inferencer) enhances a whole clip: reflect-padded STFT (train_base/acoustics/feature.py:10-30),
unet_2 (model/cruse_net.py:129-165), mask on the noisy spectrum (utils/utils.py:417-420), iSTFT (feature.py:33-61).  CRUSE is causal
in time, so the same waveform can be produced one hop at a time: this class keeps, per slot (one independent stream), the previous
input row of each encoder level, the two GRU states, 161 samples of analysis history and the overlap-add tail, and runs one hop
of every active slot as four dependent HIP kernels (cruse_stream_encode / _gru x 2 / _decode), captured as one HIP graph.

Block contract (n_fft = win = 320, hop = 160), per slot:
  push #0 stores block 0 and returns nothing (valid = False);
  push #1 computes frame 0 (its first half is the reflection x[160..1], so it needs block 1) and frame 1, returns output block 0;
  push #b (b >= 2) computes frame b and returns output block b-1;
  flush computes the end frame (the last block and its end reflection), returns the last output block and resets the slot.
Pushes + flush return exactly L samples, equal to Inferencer.mag_mask_to_wave on the same clip when L is a multiple of 160
(the caller zero-pads a partial final block) and L >= 320.

Packets (max_hops > 1): push_packet consumes up to max_hops blocks per slot in one chain of cruse_stream_*_n kernels that computes
the feed-forward part of all frames of the packet side by side and walks only the GRU recurrences frame by frame; enhance()
runs whole clips through it in bounded memory.  The schedule is packets.packet_plan; state rows and the block counter are those
of push, so push, push_packet and flush may be mixed freely on a slot.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .. import ops
from . import resample
from .packets import df_packet_plan, packet_plan


def _bn_fold(bn):
    """eval-mode BatchNorm as y * s + shift (f64, host)"""
    gamma, beta = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    mean, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    s = gamma / torch.sqrt(var + bn.eps)
    return s, beta - mean * s


DECODERS = ops.STREAM_DECODERS


def pack_weights(model, lay, decoder: str = "transposed") -> torch.Tensor:
    """The conv and LayerNorm weights of `model` as the streaming kernels read them: a float64 host vector of lay["wtotal"] floats at the
    offsets of lay = ops.stream_layout(ch), eval-mode BatchNorm folded in float64 (running statistics, bn.eps).  Needs no device.
    decoder = "transposed": unet_2's children (conv{k} / bn{k}, skip_connect_{k}, conv{k}_t / bn{k}_t); decW{k} is ConvTranspose2d's
    [Cin][Cout][3].  decoder = "upsample": CRUSE4MagAddSkipUpsample's (enc{k}.1 / enc{k}.2, skip_connect_{k}, dec{k}.sconv / dec{k}.norm);
    decW{k} is Conv2d's [Cout][Cin][3]; dec2..4 have no conv bias (the folded shift is the bias), dec1 has a bias and no norm."""
    if decoder not in DECODERS:
        raise ValueError(f"pack_weights: decoder must be one of {DECODERS}, got {decoder!r}")
    m = model
    w = torch.zeros(lay["wtotal"], dtype=torch.float64)
    d = lambda t: t.detach().double().cpu()

    def put(name, t):
        t = d(t).reshape(-1)
        w[lay[name]:lay[name] + t.numel()] = t

    for k in range(1, 5):
        if decoder == "upsample":
            enc, dec = getattr(m, f"enc{k}"), getattr(m, f"dec{k}")
            conv, bn, sconv, norm = enc[1], enc[2], dec.sconv, getattr(dec, "norm", None)
        else:
            conv, bn, sconv, norm = getattr(m, f"conv{k}"), getattr(m, f"bn{k}"), getattr(m, f"conv{k}_t"), getattr(m, f"bn{k}_t", None)
        s, sh = _bn_fold(bn)
        put(f"encW{k}", d(conv.weight) * s.view(-1, 1, 1, 1))
        put(f"encB{k}", d(conv.bias) * s + sh)
        put(f"skW{k}", getattr(m, f"skip_connect_{k}").weight)
        if k > 1:
            s, sh = _bn_fold(norm)
            # the output channels: dim 0 of a Conv2d weight, dim 1 of a ConvTranspose2d weight
            put(f"decW{k}", d(sconv.weight) * (s.view(-1, 1, 1, 1) if decoder == "upsample" else s.view(1, -1, 1, 1)))
            put(f"decB{k}", sh if sconv.bias is None else d(sconv.bias) * s + sh)
        else:
            put(f"decW{k}", sconv.weight)
            put(f"decB{k}", sconv.bias)
    put("ln1g", m.gru.ln1.weight)
    put("ln1b", m.gru.ln1.bias)
    put("ln2g", m.gru.ln2.weight)
    put("ln2b", m.gru.ln2.bias)
    return w


class StreamingInferencer:
    """Streaming unet_2 (or, with decoder="upsample", CRUSE4MagAddSkipUpsample) over `n_slots` independent streams.

    precision = "f32" (default): f32 operands, f32 accumulation throughout.  precision = "f16": the two GRU layers run on f16-operand
    MFMA kernels (cruse_stream_gru*_f16) -- the operand copies of x, h and the GRU weights are rounded to f16; accumulation, biases,
    LayerNorm, the gates, the carried state and every row stage() shows stay f32, and encode / decode are the f32 kernels.  It is
    meant for servers with many slots.  The module's own `precision` is not consulted in either mode; BatchNorm uses
    the running statistics (eval mode).  Call refresh() after changing the module's weights.

    atten_lim = True: every slot has an attenuation limit (DeepFilterNet's atten_lim_db), set_atten_lim(db, slots): the slot's output
    is lim * noisy + (1 - lim) * enhanced with lim = 10^(-db / 20), mixed on the spectrum inside the decode kernels (bin 160 keeps lim of
    the input).  The limits live in the device tensor `lim` [n_slots] (zeros: no limit, today's output) that the kernels read, so a
    change is a copy into it and never re-captures a graph.  A limit belongs to the slot: reset() and flush() leave it alone.
    pcm_in = True: push / push_packet / enhance take torch.int16 samples, read as v / 32768 by the encode kernels.  pcm_out = True:
    they and flush return torch.int16, clamp(rint(y * 32768), -32768, 32767) written by the decode kernels, and clipped() counts the
    clamped samples per slot.  The three are independent and work with either precision; with all three off nothing changes.

    io_rate = 8000, 32000 or 48000 (default 16000, the model's rate: nothing changes): the server's samples are at io_rate.  A block is
    io_block = io_rate / 100 samples (10 ms: 80, 320 or 480): push takes and returns [n_slots, io_block], push_packet [n_slots, K,
    io_block], flush returns [len(slots), io_block], enhance pads to a multiple of io_block.  Two kernels per call convert between
    io_rate and 16 kHz around the unchanged chains (cruse_stream_resample_*; the filters: inferencer/resample.py), with the per-slot
    filter histories in `rs_state`, zeroed by reset() and flush() with the rest of the slot; pcm_in / pcm_out and clipped() then apply
    to the io_rate samples, and stage() keeps showing the 16 kHz rows.  With In / Out the two converters (causal, zero history) and E
    today's 16 kHz enhancement of a whole clip, pushes + flush, packets + flush and enhance return Out(E(In(u))) truncated to the
    input's length: the converters delay the signal by io_delay samples at io_rate (64 / 96 at 32 / 48 kHz = 2 ms; 32 at 8 kHz = 4 ms)
    on top of the chain's 20 ms, and the last io_delay samples of the filters' tail are dropped.

    head = "df" (default "mask": nothing changes): the model's output is the real filter field of DeepFilter(1, 5) (a unet_2 trained
    with wo_male_df_loss; a checkpoint does not say so, the server must be told) and is applied as Inferencer(head="df") applies it:
    E[t] = the 3 x 11 neighbourhood sum of mask * noisy.  E[t] needs frame t + 1, so one more kernel (cruse_stream_df_head / _n) ends
    every chain, one frame behind decode, with a state row of its own (`df_state`): the output is 30 ms behind instead of 20.  push is
    valid from the slot's third block on (push #b returns block b-2), push_packet follows packets.df_packet_plan, flush returns the last
    TWO blocks [len(slots), 320] (the end frame's, then a drain step's), enhance still returns [n, L].  atten_lim, pcm_out and clipped()
    work through the new kernel (limit 0 dB: the input, 30 ms late); precision and pcm_in are untouched.  stage_df(slot) shows the rows E.
    On an instance with max_hops > 1 a push runs as a packet of one block: pushes and packets of any split then give one set of bits
    (the single-hop chain, which max_hops = 1 and every flush's end frame use, rounds its GRU sums differently).
    Only df_dims = (1, 5) is built, and head="df" needs io_rate = 16000.

    post_filter = "iam" or "envelope" (default None: nothing changes): the reference's perceptual post-filter of the mask (postfiltering /
    envelope_postfiltering, utils/utils.py:345-362; the closed forms and their two repairs: DESIGN 12e), applied inside the decode kernels
    before the attenuation limit: gain = lim + (1 - lim) * pf(mask).  Every slot has a tau, set_post_filter(tau, slots), in the device
    tensor `pf` [n_slots] (zeros: off, the plain server's output to the bit) that the kernels read, so a change is a copy into it and never
    re-captures a graph; like a limit it belongs to the slot: reset() and flush() leave it alone.  push, push_packet, flush and enhance
    honour it, with either precision, atten_lim, pcm_in / pcm_out and every io_rate; stage()["mask"] keeps the raw mask.  head="df" refuses
    it: that model's output is a filter field, not a gain.

    decoder = "upsample" (default "transposed": nothing changes; the names are convkxf's modes): the model is model/cruse.py's
    CRUSE4MagAddSkipUpsample, whose decoder levels are nearest FreqUpsample + Conv2d (1,3) (cust_conv.py:163-166,177-184) in place of
    ConvTranspose2d.  Encoder, skips and GGRU are unet_2's, the decoder has time extent 1 and so no state of its own: the chains are the
    same but for their decode call (cruse_stream_decode_up / _n_up), and every option above composes as for unet_2.

    meters = True (default False: nothing is allocated, captured or launched that was not before): one more kernel ends every chain
    (cruse_stream_meter / _n) and tells, per slot and frame, what the server heard without a block being read back: a meter row
    [L_in dBFS, L_out dBFS, p, vad] for every output block -- the level of the input frame, the level of the enhanced frame (both by
    Parseval on the windowed frame, 10 log10(P + 1e-12): silence reads -120), the smoothed speech probability and the decision p > threshold
    of an energy detector on the ENHANCED frame (the reference's activitydetector, utils/utils.py:143-183, with three repairs: the
    recursion runs on the smoothed value, level_db is absolute and per slot instead of a whole-clip normalisation, and the constants are
    converted from 50 ms windows to the 10 ms hop).  last_meters() is the device tensor of the last call's rows, activity() reads the
    per-slot accumulators (frames, active frames, the level of the input and of the output over active frames: the reference's active_rms)
    and set_vad() changes a slot's detector; like a limit the detector's parameters belong to the slot, and no graph is captured again.
    L_out is the level of what decode put out: atten_lim and post_filter enter through the gain; precision, pcm_in / pcm_out and decoder do
    not reach the kernel.  At another io_rate the levels are those of the model's 16 kHz side, before the output converter.  head="df"
    refuses meters: that head's output is not mask * noisy and runs a frame behind.
    """

    HOP = 160

    def __init__(self, model: torch.nn.Module, n_slots: int, n_fft: int = 320, hop_length: int = 160, win_length: int = 320,
                 device="cuda", use_graph: bool = True, max_hops: int = 1, precision: str = "f32", atten_lim: bool = False,
                 pcm_in: bool = False, pcm_out: bool = False, io_rate: int = 16000, head: str = "mask", df_dims=(1, 5),
                 post_filter=None, decoder: str = "transposed", meters: bool = False):
        from ..model.cruse import CRUSE4MagAddSkipUpsample
        from ..model.cruse_net import unet_2
        io_rate = resample.check_rate(io_rate)
        if head not in ("mask", "df"):
            raise ValueError(f"StreamingInferencer head must be \"mask\" or \"df\", got {head!r}")
        pf_kind = None if post_filter is None else ops.post_filter_kind(post_filter)
        if pf_kind is not None and head == "df":
            raise ValueError("StreamingInferencer(head=\"df\") takes no post_filter: the model's output is a filter field, not a gain")
        if tuple(df_dims) != ops.STREAM_DF_DIMS:
            raise ValueError(f"StreamingInferencer streams the DeepFilter{ops.STREAM_DF_DIMS} head only (the one instance the kernels are "
                             f"built for), got df_dims = {tuple(df_dims)}")
        if head == "df" and io_rate != resample.MODEL_RATE:
            raise ValueError(f"StreamingInferencer(head=\"df\") runs at io_rate = {resample.MODEL_RATE} only (the output converter follows the "
                             f"main chain's modes, which are one block ahead of the head), got io_rate = {io_rate}")
        if meters and head == "df":
            raise ValueError("StreamingInferencer(head=\"df\") takes no meters: the head's output is not mask * noisy and its rows run one "
                             "frame behind the chain the meter reads")
        if (n_fft, hop_length, win_length) != (320, 160, 320):
            raise ValueError(f"StreamingInferencer supports n_fft = win_length = 320, hop_length = 160 only "
                             f"(got n_fft={n_fft}, hop_length={hop_length}, win_length={win_length})")
        if precision not in ("f32", "f16"):
            raise ValueError(f"StreamingInferencer precision must be \"f32\" or \"f16\", got {precision!r}")
        if decoder not in DECODERS:
            raise ValueError(f"StreamingInferencer decoder must be one of {DECODERS}, got {decoder!r}")
        if decoder == "upsample":
            if type(model) is not CRUSE4MagAddSkipUpsample:
                raise ValueError(f"StreamingInferencer(decoder=\"upsample\") streams cruse.CRUSE4MagAddSkipUpsample only, got "
                                 f"{type(model).__name__} (unet_2 takes decoder=\"transposed\", the default)")
            # (the class has no stride or in_feat attribute: its blocks are built with fstride 2, and f_net = in_feat // 16 * 16)
            if len(model.ch) != 5 or model.ch[0] != 1 or model.f_net != 160:
                raise ValueError(f"StreamingInferencer needs CRUSE4MagAddSkipUpsample with four levels, ch[0] == 1 and in_feat 161 "
                                 f"(got ch {model.ch}, {model.f_net} network bins)")
            self.g, self.H = model.gru.groups, model.gru.hidden_size
        else:
            if type(model) is not unet_2:
                raise ValueError(f"StreamingInferencer(decoder=\"transposed\") streams cruse_net.unet_2 only (the upsample decoder of "
                                 f"{type(model).__name__} is not supported"
                                 + (": pass decoder=\"upsample\")" if type(model) is CRUSE4MagAddSkipUpsample else ")"))
            if tuple(model.stride) != (1, 2) or len(model.ch) != 5 or model.ch[0] != 1 or model.in_feat != 161:
                raise ValueError(f"StreamingInferencer needs unet_2 with stride (1,2), four levels, ch[0] == 1 and in_feat 161 "
                                 f"(got stride {tuple(model.stride)}, ch {model.ch}, in_feat {model.in_feat})")
            self.g, self.H = model.rnn_groups, model.hidden_size
        self.decoder = decoder
        if n_slots < 1:
            raise ValueError(f"n_slots must be >= 1, got {n_slots}")
        self.model = model
        self.precision = precision
        self.head = head
        self._df = head == "df"
        self.S = int(n_slots)
        self.device = torch.device(device)
        self.ch = tuple(model.ch)
        if self.H % self.g or (self.H // self.g) % 4:
            raise ValueError(f"StreamingInferencer needs hidden_size / rnn_groups divisible by 4 (hidden {self.H}, groups {self.g})")
        self.Hg = self.H // self.g
        if self.Hg > ops.STREAM_MAX_HG:     # cruse_stream_gru* refuse it: say so here, not from the first push's graph capture
            raise ValueError(f"StreamingInferencer needs hidden_size / rnn_groups <= {ops.STREAM_MAX_HG} (hidden {self.H}, groups "
                             f"{self.g}: {self.Hg} per group; the GRU kernels hold a unit's weight rows in 16 registers per lane)")
        self.lay = ops.stream_layout(self.ch)
        self.use_graph = use_graph
        S, dev = self.S, self.device
        self.state = torch.zeros(S, self.lay["st_stride"], device=dev)
        self.work = torch.zeros(S, self.lay["wk_stride"], device=dev)
        self.atten_lim, self.pcm_in, self.pcm_out = bool(atten_lim), bool(pcm_in), bool(pcm_out)
        self.in_dtype = torch.int16 if self.pcm_in else torch.float32
        self.out_dtype = torch.int16 if self.pcm_out else torch.float32
        self._io_rate = io_rate
        self._rs = io_rate != resample.MODEL_RATE
        # the chains' own boundary tensors: the caller's formats, or f32 behind the converters
        self.blocks = torch.zeros(S, self.HOP, device=dev, dtype=torch.float32 if self._rs else self.in_dtype)
        self.out = torch.zeros(S, self.HOP, device=dev, dtype=torch.float32 if self._rs else self.out_dtype)
        self.rs_state = self.rs_taps = None
        if self._rs:
            self.io_blocks = torch.zeros(S, self.io_block, device=dev, dtype=self.in_dtype)
            self.io_out = torch.zeros(S, self.io_block, device=dev, dtype=self.out_dtype)
            self.rs_taps = ops.stream_resample_taps(io_rate, dev)
            self.rs_state = torch.zeros(S, sum(resample.history(io_rate)), device=dev)      # [in-side history | out-side history]
        if self._df:
            # the head's own rows: state (P[t-2], P[t-1], N[t-1], tail, count), the E rows of the last call (row 1: the drain step of a
            # flush), the drain step's block, and the block decode's mask path still computes (not returned)
            self.df_lay = ops.stream_df_layout()
            self.df_state = torch.zeros(S, self.df_lay["stride"], device=dev)
            self.df_work = torch.zeros(S, 2, ops.STREAM_DF_ROW, device=dev)
            self.out_drain = torch.zeros(S, self.HOP, device=dev, dtype=self.out_dtype)
            self._mask_out = torch.zeros(S, self.HOP, device=dev)
            self._df_rows = np.zeros(S, dtype=np.int64)                         # E rows the slot's last call wrote
        self.lim = torch.zeros(S, device=dev) if self.atten_lim else None       # per-slot gains 10^(-dB/20); 0: no limit
        self.post_filter = post_filter
        self.pf = torch.zeros(S, device=dev) if pf_kind is not None else None   # per-slot tau of the post-filter; 0: off
        self._pf_kind = pf_kind
        self.clip = torch.zeros(S, device=dev, dtype=torch.int32) if self.pcm_out else None     # clamped samples per slot
        self.meters = bool(meters)
        if self.meters:
            # the detector's parameters (level_db, threshold, attack, release), p_prev, the f64 accumulators, the last call's rows
            mlay = ops.stream_meter_layout()
            d = ops.stream_vad_defaults()
            self.vad_par = torch.tensor([[d["level_db"], d["threshold"], d["attack"], d["release"]]], dtype=torch.float64) \
                .to(torch.float32).repeat(S, 1).to(dev)
            self.meter_state = torch.zeros(S, mlay["stride"], device=dev)
            self.meter_acc = torch.zeros(S, mlay["acc"], device=dev, dtype=torch.float64)
            self.meter_out = torch.zeros(S, max(int(max_hops), 1), ops.STREAM_METER_ROW, device=dev)
        self.mode = torch.zeros(2, S, device=dev, dtype=torch.int32)            # row 0: the frame-0 chain, row 1: the main chain
        self._mode_host = [torch.zeros(2, S, dtype=torch.int32).pin_memory(), None]     # pinned twin, event: the last copy out of it is done
        self.tab = ops.stream_tables(dev)
        self.nblk = np.zeros(S, dtype=np.int64)                                 # blocks pushed per slot since its last reset
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.max_hops = int(max_hops)
        self._last_frames = np.zeros(S, dtype=np.int64)                         # frames of the slot's last packet (0: a push / flush)
        self._last_f0 = np.zeros(S, dtype=bool)                                 # that packet began with frame 0 of the clip
        if self.max_hops != 1:
            play = ops.stream_packet_layout(self.ch)
            if not 1 <= self.max_hops <= play["max_hops"]:
                raise ValueError(f"max_hops must be in [1, {play['max_hops']}] for ch = {self.ch} (the packet kernels keep "
                                 f"max_hops + 1 frames of a slot in LDS), got {max_hops}")
            K = self.max_hops
            self.play = play
            self.pblocks = torch.zeros(S, K, self.HOP, device=dev, dtype=self.blocks.dtype)
            self.pout = torch.zeros(S, K, self.HOP, device=dev, dtype=self.out.dtype)
            if self._rs:
                self.io_pblocks = torch.zeros(S, K, self.io_block, device=dev, dtype=self.in_dtype)
                self.io_pout = torch.zeros(S, K, self.io_block, device=dev, dtype=self.out_dtype)
            if self._df:
                self._mask_pout = torch.zeros(S, K, self.HOP, device=dev)
                self.df_pwork = torch.zeros(S, K, ops.STREAM_DF_ROW, device=dev)    # one E row per frame a packet emits
            self.pwork = torch.zeros(S, K + 1, play["wk_stride"], device=dev)   # one work row per frame of a packet
            self.gi = torch.zeros(S, K + 1, 3 * self.H, device=dev)             # GRU input products of the layer in flight
            self.pk = torch.zeros(2, S, device=dev, dtype=torch.int32)          # row 0: min(blocks held, 2), row 1: counts
            self._pk_host = [torch.zeros(2, S, dtype=torch.int32).pin_memory(), None]
        self.refresh()

    @property
    def io_rate(self) -> int:
        return self._io_rate

    @property
    def io_block(self) -> int:
        """samples of a block (10 ms) at io_rate"""
        return resample.io_block(self._io_rate)

    @property
    def io_delay(self) -> int:
        """samples at io_rate by which the two rate converters delay the output (0 at 16 kHz), beside the chain's own 20 ms"""
        return resample.io_delay(self._io_rate)

    # -- weights ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> None:
        """Re-pack the module's weights: pack_weights (BatchNorm folded into the convs; running statistics, bn.eps), GRU weights per layer as
        W_ih [g][3Hg][Hg] | W_hh | b_ih [g][3Hg] | b_hh; in f16 mode also each layer's weights as f16 MFMA fragments (ops.stream_pack_f16)."""
        m, lay = self.model, self.lay
        w = pack_weights(m, lay, self.decoder)
        self.ln1_eps, self.ln2_eps = float(m.gru.ln1.eps), float(m.gru.ln2.eps)
        w = w.float().to(self.device)
        packs, packs16 = [], []
        for lst in (m.gru.gru_list1, m.gru.gru_list2):
            parts = [torch.stack([gr.weight_ih_l0 for gr in lst]), torch.stack([gr.weight_hh_l0 for gr in lst]),
                     torch.stack([gr.bias_ih_l0 for gr in lst]), torch.stack([gr.bias_hh_l0 for gr in lst])]
            packs.append(torch.cat([p.detach().float().reshape(-1).to(self.device) for p in parts]))
            if self.precision == "f16":
                packs16.append(ops.stream_pack_f16(parts[0], parts[1]).to(self.device))
        if hasattr(self, "w"):                      # captured graphs hold these buffers: update them in place
            self.w.copy_(w)
            self.gru_pack1.copy_(packs[0])
            self.gru_pack2.copy_(packs[1])
        else:
            self.w, (self.gru_pack1, self.gru_pack2) = w, packs
        if packs16:
            if hasattr(self, "gru_pack1_f16"):
                self.gru_pack1_f16.copy_(packs16[0])
                self.gru_pack2_f16.copy_(packs16[1])
            else:
                self.gru_pack1_f16, self.gru_pack2_f16 = packs16
        # the two GRU layers of a chain: (layer, x_off, st_off, h_off, pack, pack16 or None, LN1 kwargs)
        ln1 = lambda n: self.w[lay[n]:lay[n] + self.H]
        self._layers = ((1, lay["wk_x"], lay["st_h1"], lay["wk_h1n"], self.gru_pack1, getattr(self, "gru_pack1_f16", None), {}),
                        (2, lay["wk_h1n"], lay["st_h2"], lay["wk_h2n"], self.gru_pack2, getattr(self, "gru_pack2_f16", None),
                         dict(ln_g=ln1("ln1g"), ln_b=ln1("ln1b"), ln_eps=self.ln1_eps)))

    # -- the hop ----------------------------------------------------------------------------------------------------------
    def _chain(self, row: int) -> None:
        mode, g, Hg = self.mode[row], self.g, self.Hg
        ops.stream_encode(mode, self.ch, self.blocks, self.tab, self.w, self.state, self.work)
        for layer, x_off, st_off, h_off, pack, pack16, ln1 in self._layers:
            ops.stream_gru(mode, layer, g, Hg, self.work, x_off, self.state, st_off, pack, self.work, h_off, pack16=pack16, **ln1)
        if self._df:        # decode leaves the mask in the work row; the head, one frame behind, writes the block
            ops.stream_decode(mode, self.ch, self.tab, self.w, self.ln2_eps, self.state, self.work, self._mask_out, decoder=self.decoder)
            ops.stream_df_head(mode, self.work, self.lay, self.tab, self.df_state, self.df_work[:, 0], self.out, lim=self.lim, clip=self.clip)
            return
        ops.stream_decode(mode, self.ch, self.tab, self.w, self.ln2_eps, self.state, self.work, self.out, lim=self.lim,
                          clip=None if self._rs else self.clip,             # behind the converters, resample_out counts
                          pf=self._pf(), decoder=self.decoder)
        if self.meters:
            ops.stream_meter(mode, self.work, self.lay, self.tab, self.vad_par, self.meter_state, self.meter_acc, self.meter_out[:, 0],
                             lim=self.lim, pf=self._pf())

    def _replay(self, key, fn) -> None:
        """run fn(): directly, or as the graph captured from it on the first call with this key"""
        if not self.use_graph:
            fn()
            return
        gr = self._graphs.get(key)
        if gr is None:
            torch.cuda.synchronize(self.device)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                fn()
            self._graphs[key] = gr
        gr.replay()

    def _launch(self, passes: int, drain: bool = False) -> None:
        rows = (0, 1) if passes == 2 else (1,)

        def hop():
            if self._rs:                                                        # once, on the main chain's modes
                ops.stream_resample_in(self.mode[1], self.io_rate, self.io_blocks, self.rs_taps, self.rs_state, self.blocks)
            for r in rows:
                self._chain(r)
            if self._rs:
                ops.stream_resample_out(self.mode[1], self.io_rate, self.out, self.rs_taps, self.rs_state, self.io_out, clip=self.clip)
            if drain:                                                           # head="df": the END slots' last row, on a zero row
                ops.stream_df_head(self.mode[1], self.work, self.lay, self.tab, self.df_state, self.df_work[:, 1], self.out_drain,
                                   lim=self.lim, clip=self.clip, drain=True)

        self._replay(("drain", passes) if drain else passes, hop)

    @staticmethod
    def _upload(dev: torch.Tensor, twin: list, row0, row1) -> None:
        """Rows 0 and 1 of the [2, S] device tensor dev (mode, pk) through twin = [pinned host tensor, event]: wait until the previous copy
        out of the host tensor is done, fill it, copy without blocking, record the event the next upload waits for."""
        if twin[1] is not None:
            twin[1].synchronize()
        h = twin[0].numpy()
        h[0], h[1] = row0, row1
        dev.copy_(twin[0], non_blocking=True)
        twin[1] = torch.cuda.Event()
        twin[1].record()

    def _run(self, m0: np.ndarray, m1: np.ndarray, drain: bool = False) -> None:
        self._upload(self.mode, self._mode_host, m0, m1)
        self._launch(2 if m0.any() else 1, drain)

    def _samples(self, t: torch.Tensor, who: str) -> torch.Tensor:
        """the input samples in the instance's input format: float32 (converted, as always), or int16 and nothing else with pcm_in"""
        if not self.pcm_in:
            return t.to(torch.float32)
        if t.dtype != torch.int16:
            raise ValueError(f"{who}: this StreamingInferencer was built with pcm_in=True and takes torch.int16 samples, got {t.dtype}")
        return t

    @torch.no_grad()
    def push(self, blocks: torch.Tensor, active=None):
        """blocks [n_slots, 160] (the next block of every active slot; rows of inactive slots are ignored); active: bool per slot
        (None: all).  Returns (out [n_slots, 160] on the device, valid [n_slots] bool on the host): out[s] is the next enhanced
        block of slot s where valid[s]; inactive slots keep their state untouched.  160: io_block at another io_rate."""
        S, B = self.S, self.io_block
        if tuple(blocks.shape) != (S, B):
            raise ValueError(f"push expects blocks of shape ({S}, {B}), got {tuple(blocks.shape)}")
        blocks = self._samples(blocks, "push")
        if active is None:
            act = np.ones(S, dtype=bool)
        else:
            act = (active.cpu().numpy() if torch.is_tensor(active) else np.asarray(active)).astype(bool).reshape(-1)
            if act.size != S:
                raise ValueError(f"active must have {S} entries, got {act.size}")
        if self._df and self.max_hops != 1:
            # an instance built for packets: a push is a packet of one block, so that a slot's output does not depend on how its blocks
            # were grouped into calls (the packet chain's GRU sums round differently from the single-hop chain's)
            out, n_out = self.push_packet(blocks.unsqueeze(1), act.astype(np.int64))
            return out[:, 0], n_out > 0
        (self.io_blocks if self._rs else self.blocks).copy_(blocks, non_blocking=True)
        b = self.nblk
        m0 = np.where(act & (b == 1), ops.STREAM_FRAME0, ops.STREAM_SKIP).astype(np.int32)
        m1 = np.where(act, np.where(b == 0, ops.STREAM_STORE, ops.STREAM_FRAME), ops.STREAM_SKIP).astype(np.int32)
        valid = act & (b >= (2 if self._df else 1))
        if self._df:
            self._df_rows[act] = (b >= 1)[act]
        self.nblk += act
        self._last_frames[act] = 0
        self._run(m0, m1)
        return (self.io_out if self._rs else self.out).clone(), torch.from_numpy(valid)

    @torch.no_grad()
    def flush(self, slots) -> torch.Tensor:
        """End the clip of each slot in `slots`: computes its end frame and returns its last output block ([len(slots), 160],
        device), then resets the slot.  A slot must hold at least two blocks.  head="df": the last two blocks, [len(slots), 320]."""
        if slots is None:
            raise TypeError("flush: slots is None (a flush names its slots)")
        slots = self._slot_list(slots)
        for s in slots:
            if self.nblk[s] < 2:
                raise ValueError(f"cannot flush slot {s}: it holds {self.nblk[s]} block(s), a clip needs at least 2 (L >= 320)")
        m1 = np.zeros(self.S, dtype=np.int32)
        m1[slots] = ops.STREAM_END
        self._last_frames[slots] = 0
        self._run(np.zeros(self.S, dtype=np.int32), m1, drain=self._df)
        idx = torch.tensor(slots, device=self.device, dtype=torch.long)
        last = (self.io_out if self._rs else self.out).index_select(0, idx)
        if self._df:                                                            # the end frame's block, then the drain step's
            last = torch.cat([last, self.out_drain.index_select(0, idx)], dim=1)
        self._reset(slots, keep_activity=True)
        if self._df:
            self._df_rows[slots] = 2
        return last

    @torch.no_grad()
    def reset(self, slots=None) -> None:
        """Zero the state of `slots` (None: all): the next push to such a slot is block 0 of a new clip.  meters=True: the detector's
        state and the slot's activity() accumulators are zeroed too (flush keeps the accumulators: they describe the clip just ended
        until the slot's next clip begins)."""
        self._reset(slots)

    def _reset(self, slots, keep_activity: bool = False) -> None:
        slots = self._slot_list(slots, in_range=False)                          # (as ever, reset leaves the range to the indexing)
        if slots:
            idx = torch.tensor(slots, device=self.device, dtype=torch.long)
            self.state.index_fill_(0, idx, 0.0)
            if self._rs:
                self.rs_state.index_fill_(0, idx, 0.0)
            if self._df:
                self.df_state.index_fill_(0, idx, 0.0)
            if self.meters:
                self.meter_state.index_fill_(0, idx, 0.0)
                if not keep_activity:
                    self.meter_acc.index_fill_(0, idx, 0.0)
        self.nblk[slots] = 0
        self._last_frames[slots] = 0

    # -- attenuation limit, clip counters -----------------------------------------------------------------------------------
    def _slot_list(self, slots, in_range: bool = True):
        if slots is None:
            return list(range(self.S))
        slots = [int(s) for s in (slots.tolist() if torch.is_tensor(slots) else slots)]
        for s in slots:
            if in_range and not 0 <= s < self.S:
                raise ValueError(f"slot {s} out of range [0, {self.S})")
        return slots

    def _set_per_slot(self, tensor: torch.Tensor, values, slots, convert, who: str) -> None:
        """tensor[slots] = convert(values): a scalar (or None) for all of `slots` (None: all), or one value per listed slot"""
        slots = self._slot_list(slots)
        if values is None or np.ndim(values) == 0:
            vals = [values] * len(slots)
        else:
            vals = list(values.tolist() if torch.is_tensor(values) or isinstance(values, np.ndarray) else values)
            if len(vals) != len(slots):
                raise ValueError(f"{who}: {len(vals)} values for {len(slots)} slots")
        vals = [convert(v) for v in vals]                                       # refuses negative and NaN before anything is copied
        if slots:
            idx = torch.tensor(slots, device=self.device, dtype=torch.long)
            tensor.index_copy_(0, idx, torch.tensor(vals, dtype=torch.float32).to(self.device))

    @torch.no_grad()
    def set_atten_lim(self, db, slots=None) -> None:
        """Attenuation limit in dB of `slots` (None: all): a scalar or None for all of them, or one value per listed slot.  None or
        inf: no limit (full suppression); 0: the input passes through, 20 ms late.  Takes effect with the next frame of the slot and
        stays until it is set again (reset and flush keep it).  Needs atten_lim=True at construction."""
        if not self.atten_lim:
            raise ValueError("set_atten_lim: this StreamingInferencer was built without atten_lim=True (its kernels read no limits)")
        self._set_per_slot(self.lim, db, slots, ops.atten_lim_gain, "set_atten_lim")

    def _pf(self):
        """the pf argument of the decode calls: None without a post-filter (the calls are then today's)"""
        return None if self.pf is None else (self._pf_kind, self.pf)

    @torch.no_grad()
    def set_post_filter(self, tau, slots=None) -> None:
        """The post-filter's tau of `slots` (None: all): a scalar for all of them, or one value per listed slot.  0: off (the slot's
        output is the unfiltered one, to the bit); the reference's default is 0.02.  Takes effect with the next frame of the slot and
        stays until it is set again (reset and flush keep it).  Needs post_filter="iam" or "envelope" at construction."""
        if self.pf is None:
            raise ValueError("set_post_filter: this StreamingInferencer was built without post_filter (its kernels read no tau)")
        self._set_per_slot(self.pf, tau, slots, ops.post_filter_tau, "set_post_filter")

    @torch.no_grad()
    def clipped(self, slots=None, reset: bool = False) -> np.ndarray:
        """int64 host array: the output samples of each slot in `slots` (None: all) that were clamped to the int16 range since the
        counter was last zeroed; reset=True zeroes the counters read.  Needs pcm_out=True (float output is never clamped)."""
        if not self.pcm_out:
            raise ValueError("clipped: this StreamingInferencer was built without pcm_out=True (float output is not clamped)")
        slots = self._slot_list(slots)
        idx = torch.tensor(slots, device=self.device, dtype=torch.long)
        n = self.clip.index_select(0, idx).cpu().numpy().astype(np.int64)
        if reset and slots:
            self.clip.index_fill_(0, idx, 0)
        return n

    # -- level meters, voice activity -------------------------------------------------------------------------------------------
    def _need_meters(self, who: str) -> None:
        if not self.meters:
            raise ValueError(f"{who}: this StreamingInferencer was built without meters=True (no meter kernel runs in its chains)")

    def last_meters(self) -> torch.Tensor:
        """The meter rows of the last call, [n_slots, max_hops, 4] on the device (the tensor the kernels write: no copy, no
        synchronisation; clone it to keep it past the next call): row [s, j] = [L_in dBFS, L_out dBFS, p, vad] belongs to the j-th block
        that call returned for slot s, and only as many rows as blocks are valid (push: row 0 where valid[s]; push_packet: n_out[s] rows;
        flush: row 0 of each flushed slot).  Needs meters=True."""
        self._need_meters("last_meters")
        return self.meter_out

    @torch.no_grad()
    def activity(self, slots=None, reset: bool = False) -> np.ndarray:
        """float64 host array [len(slots), 4] (slots None: all): frames metered, active frames (vad = 1), the level in dBFS of the input
        and of the enhanced output over the active frames only (10 log10(mean P + 1e-12): the reference's active_rms on the detector's
        own decisions; -120 without an active frame).  The accumulators start with a slot's clip (its frame 0 zeroes them), survive flush
        and are zeroed by reset() or reset=True.  A host read-back, like clipped().  Needs meters=True."""
        self._need_meters("activity")
        slots = self._slot_list(slots)
        idx = torch.tensor(slots, device=self.device, dtype=torch.long)
        acc = self.meter_acc.index_select(0, idx).cpu().numpy().astype(np.float64).reshape(len(slots), 4)
        if reset and slots:
            self.meter_acc.index_fill_(0, idx, 0.0)
        n = np.maximum(acc[:, 1], 1.0)
        out = acc.copy()
        out[:, 2:] = 10.0 * np.log10(acc[:, 2:] / n[:, None] + 1e-12)
        return out

    @torch.no_grad()
    def set_vad(self, level_db=None, threshold=None, attack=None, release=None, slots=None) -> None:
        """The detector of `slots` (None: all); every argument a scalar for all of them or one value per listed slot, None: unchanged.
        level_db: the output level in dBFS at which the raw speech probability is 1/2 (default -28.23, ops.stream_vad_defaults);
        threshold: vad = p > threshold (0.13); attack / release: the per-hop smoothing constants in (0, 1] towards a higher / lower
        probability.  Takes effect with the slot's next frame and stays (reset and flush keep it).  Needs meters=True."""
        self._need_meters("set_vad")

        def finite(name, lo=None, hi=None):
            def conv(v):
                v = float(v)
                if v != v or v in (float("inf"), float("-inf")) or (lo is not None and not v > lo) or (hi is not None and not v <= hi):
                    raise ValueError(f"set_vad: {name} must be a finite number" + (f" in ({lo}, {hi}]" if lo is not None else "") + f", got {v}")
                return v
            return conv

        for k, (name, val, conv) in enumerate((("level_db", level_db, finite("level_db")), ("threshold", threshold, finite("threshold")),
                                               ("attack", attack, finite("attack", 0.0, 1.0)),
                                               ("release", release, finite("release", 0.0, 1.0)))):
            if val is not None:
                self._set_per_slot(self.vad_par[:, k], val, slots, conv, f"set_vad({name})")

    # -- packets ----------------------------------------------------------------------------------------------------------
    def _packet_chain(self, hops: int, nf: int) -> None:
        """One linear chain for packets of up to `hops` blocks of which the longest slot computes `nf` frames."""
        pk, g, Hg, wk = self.pk, self.g, self.Hg, self.pwork
        if self._rs:
            ops.stream_resample_in_n(pk, hops, self.io_rate, self.io_pblocks, self.rs_taps, self.rs_state, self.pblocks)
        ops.stream_encode_n(pk, hops, self.ch, self.pblocks, self.tab, self.w, self.state, wk)
        if nf == 0:                                                             # nothing but first blocks to store
            return
        for layer, x_off, st_off, h_off, pack, pack16, ln1 in self._layers:
            ops.stream_gru_proj_n(pk, hops, layer, g, Hg, wk, x_off, pack, self.gi, pack16=pack16, **ln1)
            for f in range(nf):
                ops.stream_gru_rec_n(pk, hops, f, g, Hg, self.gi, self.state, st_off, pack, wk, h_off, pack16=pack16)
        if self._df:
            ops.stream_decode_n(pk, hops, self.ch, self.tab, self.w, self.ln2_eps, self.state, wk, self._mask_pout, decoder=self.decoder)
            ops.stream_df_head_n(pk, hops, wk, self.lay, self.tab, self.df_state, self.df_pwork, self.pout, lim=self.lim, clip=self.clip)
            return
        ops.stream_decode_n(pk, hops, self.ch, self.tab, self.w, self.ln2_eps, self.state, wk, self.pout, lim=self.lim,
                            clip=None if self._rs else self.clip, pf=self._pf(), decoder=self.decoder)
        if self.meters:
            ops.stream_meter_n(pk, hops, wk, self.lay, self.tab, self.vad_par, self.meter_state, self.meter_acc, self.meter_out,
                               lim=self.lim, pf=self._pf())
        if self._rs:
            ops.stream_resample_out_n(pk, hops, self.io_rate, self.pout, self.rs_taps, self.rs_state, self.io_pout, clip=self.clip)

    @torch.no_grad()
    def push_packet(self, blocks: torch.Tensor, counts=None):
        """blocks [n_slots, K, 160] or [n_slots, K*160], 1 <= K <= max_hops; counts: an int per slot in [0, K] (None: K for every
        slot; 0: the slot is inactive and its state untouched).  Slot s consumes its first counts[s] blocks.  Returns
        (out [n_slots, K, 160] on the device, n_out [n_slots] int64 on the host): out[s, :n_out[s]] are the next enhanced blocks
        of slot s, in order.  n_out[s] = counts[s] where the slot already held a block, else max(counts[s] - 1, 0).
        160: io_block at another io_rate."""
        S, HOP = self.S, self.io_block
        if blocks.dim() == 2 and blocks.shape[0] == S and blocks.shape[1] % HOP == 0 and blocks.shape[1] > 0:
            blocks = blocks.reshape(S, blocks.shape[1] // HOP, HOP)
        if blocks.dim() != 3 or blocks.shape[0] != S or blocks.shape[2] != HOP or blocks.shape[1] < 1:
            raise ValueError(f"push_packet expects blocks of shape ({S}, K, {HOP}) or ({S}, K*{HOP}), got {tuple(blocks.shape)}")
        blocks = self._samples(blocks, "push_packet")
        K = int(blocks.shape[1])
        if K > self.max_hops:
            raise ValueError(f"push_packet: a packet of {K} blocks exceeds max_hops = {self.max_hops}")
        if counts is None:
            cnt = np.full(S, K, dtype=np.int64)
        else:
            cnt = (counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).reshape(-1)
            if cnt.size != S:
                raise ValueError(f"counts must have {S} entries, got {cnt.size}")
            if not np.issubdtype(cnt.dtype, np.integer) and not np.all(cnt == np.floor(cnt)):
                raise ValueError("counts must be integers")
            cnt = cnt.astype(np.int64)
            if cnt.min() < 0 or cnt.max() > K:
                raise ValueError(f"counts must lie in [0, {K}] (the packet has {K} blocks), got min {cnt.min()}, max {cnt.max()}")
        if self.max_hops == 1:                                                  # one block per call: the single-hop chain
            out, valid = self.push(blocks[:, 0], cnt > 0)
            return out.unsqueeze(1), valid.to(torch.int64)
        plan = df_packet_plan if self._df else packet_plan
        plans = [plan(int(b), int(c)) for b, c in zip(self.nblk, cnt)]
        n_out = np.array([p.n_out for p in plans], dtype=np.int64)
        frames = np.array([p.n_frames for p in plans], dtype=np.int64)
        hops = int(cnt.max())
        if hops == 0:
            return torch.zeros(S, K, HOP, device=self.device, dtype=self.out_dtype), torch.from_numpy(n_out)
        (self.io_pblocks if self._rs else self.pblocks)[:, :K].copy_(blocks, non_blocking=True)
        self._upload(self.pk, self._pk_host, [p.start for p in plans], cnt)
        self.nblk += cnt
        act = cnt > 0
        self._last_frames[act] = frames[act]
        self._last_f0[act] = np.array([p.first_frame == 0 for p in plans])[act]
        if self._df:                                                            # every frame but a clip's frame 0 emits a row
            self._df_rows[act] = (frames - (self._last_f0 & (frames > 0)))[act]
        nf = int(frames.max())
        self._replay(("packet", hops, nf), lambda: self._packet_chain(hops, nf))
        return (self.io_pout if self._rs else self.pout)[:, :K].clone(), torch.from_numpy(n_out)

    @torch.no_grad()
    def enhance(self, waves: torch.Tensor, hops=None, with_meters: bool = False):
        """Whole clips waves [n, L] (n <= n_slots, L >= 320, device or host) through push_packet with `hops` (default max_hops)
        blocks per call, then flush; -> [n, L] on the device.  Uses slots 0..n-1: resets them first and leaves them reset.  When L
        is not a multiple of 160 the clip is zero-padded to the next multiple and the result trimmed to L, so it equals the
        offline result OF THE PADDED CLIP (the end reflection then mirrors the padding).  Only one packet of the clip is on the
        device's work buffers at a time: memory beyond the input and output waveforms does not grow with L.  At another io_rate
        320 and 160 read 2 * io_block and io_block.  with_meters=True (needs meters=True): -> (waves [n, L], meters [n, frames - 1, 4]),
        one meter row per block of the padded clip."""
        if with_meters:
            self._need_meters("enhance(with_meters=True)")
        if waves.dim() != 2:
            raise ValueError(f"enhance expects waves of shape (n, L), got {tuple(waves.shape)}")
        if self.pcm_in:
            self._samples(waves, "enhance")
        n, L = int(waves.shape[0]), int(waves.shape[1])
        hops = self.max_hops if hops is None else int(hops)
        if not 1 <= n <= self.S:
            raise ValueError(f"enhance: {n} clips for {self.S} slots")
        if L < 2 * self.io_block:
            raise ValueError(f"enhance: clips of {L} samples are shorter than {2 * self.io_block}")
        if not 1 <= hops <= self.max_hops:
            raise ValueError(f"enhance: hops = {hops} outside [1, max_hops = {self.max_hops}]")
        S, HOP = self.S, self.io_block
        nb = (L + HOP - 1) // HOP                                               # the last block zero-padded (packets.padded_blocks at 160)
        slots = list(range(n))
        self.reset(slots)
        res = torch.empty(n, nb * HOP, device=self.device, dtype=self.out_dtype)
        met = torch.empty(n, nb, ops.STREAM_METER_ROW, device=self.device) if with_meters else None
        pkt = torch.zeros(S, hops * HOP, device=self.device, dtype=self.in_dtype)
        counts = np.zeros(S, dtype=np.int64)
        done = 0                                                                # output blocks written
        for b0 in range(0, nb, hops):
            c = min(hops, nb - b0)
            lo, hi = b0 * HOP, min((b0 + c) * HOP, L)
            pkt[:n, :hi - lo].copy_(waves[:, lo:hi], non_blocking=True)
            if hi - lo < hops * HOP:
                pkt[:n, hi - lo:].zero_()
            counts[:n] = c
            out, n_out = self.push_packet(pkt, counts)
            k = int(n_out[0])
            res[:, done * HOP:(done + k) * HOP] = out[:n, :k].reshape(n, k * HOP)
            if with_meters:
                met[:, done:done + k] = self.meter_out[:n, :k]
            done += k
        res[:, done * HOP:] = self.flush(slots)
        if with_meters:
            met[:, done] = self.meter_out[:n, 0]
            return res[:, :L], met
        return res[:, :L]

    # -- inspection ---------------------------------------------------------------------------------------------------------
    def stage(self, slot: int, frame: int = -1) -> Dict[str, torch.Tensor]:
        """Views of one computed frame of slot `slot`: re / im (161), e1..e4, skip1..skip4, gru1 / gru2 (group-contiguous), mask.
        After push / flush: the frame just computed.  After push_packet: frame `frame` of the slot's packet (0 .. frames - 1 or
        negative from the end; default the last one) and its output block as "block" (absent for frame 0 of a clip)."""
        lay, ch, F = self.lay, self.ch, [160 >> k for k in range(5)]
        nfr = int(self._last_frames[slot])
        if nfr > 0:
            if not -nfr <= frame < nfr:
                raise ValueError(f"stage: frame {frame} outside the {nfr} frames of slot {slot}'s last packet")
            f = frame % nfr
            wk = e = self.pwork[slot, f]                                        # a packet keeps e1..e3 in the frame's work row
            eoff = {k: self.play[f"wk_e{k}"] for k in range(1, 4)}
        else:
            if frame not in (-1, 0):
                raise ValueError(f"stage: slot {slot}'s last call computed one frame, frame {frame} does not exist")
            wk, e = self.work[slot], self.state[slot]                           # a single hop in the state rows only
            eoff = {k: lay[f"st_prev{k}"] for k in range(1, 4)}
        out = {"re": wk[lay["wk_re"]:lay["wk_re"] + 161], "im": wk[lay["wk_im"]:lay["wk_im"] + 161],
               "gru1": wk[lay["wk_h1n"]:lay["wk_h1n"] + self.H], "gru2": wk[lay["wk_h2n"]:lay["wk_h2n"] + self.H],
               "mask": wk[lay["wk_mask"]:lay["wk_mask"] + 160], "e4": wk[lay["wk_x"]:lay["wk_x"] + self.H]}
        for k in range(1, 5):
            n = ch[k] * F[k]
            out[f"skip{k}"] = wk[lay[f"wk_skip{k}"]:lay[f"wk_skip{k}"] + n]
            if k < 4:
                out[f"e{k}"] = e[eoff[k]:eoff[k] + n]
        if nfr > 0 and not self._df:                                            # (head="df": pout holds the head's blocks, a frame behind)
            first = int(self._last_f0[slot])                                    # frame 0 of a clip yields no output block
            if f - first >= 0:
                out["block"] = self.pout[slot, f - first]
        return out

    def stage_df(self, slot: int) -> torch.Tensor:
        """head="df": the rows E (re[161] | im[161]) the head emitted for slot `slot` in its last call, [rows, 322] in frame order: one
        after a push that computed a frame (E[t-1] for frame t; none after the push of block 0), one per frame but a clip's frame 0 after
        push_packet, two after flush (the end frame's E[T-2] and the drain step's E[T-1])."""
        if not self._df:
            raise ValueError("stage_df: this StreamingInferencer was built with head=\"mask\" (there is no DeepFilter head to inspect)")
        if not 0 <= slot < self.S:
            raise ValueError(f"slot {slot} out of range [0, {self.S})")
        rows = self.df_pwork if self._last_frames[slot] > 0 else self.df_work
        return rows[slot, :int(self._df_rows[slot])]
