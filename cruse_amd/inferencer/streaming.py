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
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .. import ops


def _bn_fold(bn):
    """eval-mode BatchNorm as y * s + shift (f64, host)"""
    gamma, beta = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    mean, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    s = gamma / torch.sqrt(var + bn.eps)
    return s, beta - mean * s


class StreamingInferencer:
    """Streaming unet_2 over `n_slots` independent streams.

    Streaming always computes in f32 (f32 operands, f32 accumulation), whatever the module's `precision`; BatchNorm uses the
    running statistics (eval mode).  Call refresh() after changing the module's weights.
    """

    HOP = 160

    def __init__(self, model: torch.nn.Module, n_slots: int, n_fft: int = 320, hop_length: int = 160, win_length: int = 320,
                 device="cuda", use_graph: bool = True):
        from ..model.cruse_net import unet_2
        if (n_fft, hop_length, win_length) != (320, 160, 320):
            raise ValueError(f"StreamingInferencer supports n_fft = win_length = 320, hop_length = 160 only "
                             f"(got n_fft={n_fft}, hop_length={hop_length}, win_length={win_length})")
        if type(model) is not unet_2:
            raise ValueError(f"StreamingInferencer streams cruse_net.unet_2 only (the upsample decoder of "
                             f"{type(model).__name__} is not supported)")
        if tuple(model.stride) != (1, 2) or len(model.ch) != 5 or model.ch[0] != 1 or model.in_feat != 161:
            raise ValueError(f"StreamingInferencer needs unet_2 with stride (1,2), four levels, ch[0] == 1 and in_feat 161 "
                             f"(got stride {tuple(model.stride)}, ch {model.ch}, in_feat {model.in_feat})")
        if n_slots < 1:
            raise ValueError(f"n_slots must be >= 1, got {n_slots}")
        self.model = model
        self.S = int(n_slots)
        self.device = torch.device(device)
        self.ch = tuple(model.ch)
        self.g = model.rnn_groups
        self.H = model.hidden_size
        if self.H % self.g or (self.H // self.g) % 4:
            raise ValueError(f"StreamingInferencer needs hidden_size / rnn_groups divisible by 4 (hidden {self.H}, groups {self.g})")
        self.Hg = self.H // self.g
        self.lay = ops.stream_layout(self.ch)
        self.use_graph = use_graph
        S, dev = self.S, self.device
        self.state = torch.zeros(S, self.lay["st_stride"], device=dev)
        self.work = torch.zeros(S, self.lay["wk_stride"], device=dev)
        self.blocks = torch.zeros(S, self.HOP, device=dev)
        self.out = torch.zeros(S, self.HOP, device=dev)
        self.mode = torch.zeros(2, S, device=dev, dtype=torch.int32)            # row 0: the frame-0 chain, row 1: the main chain
        self._mode_host = torch.zeros(2, S, dtype=torch.int32).pin_memory()
        self._host_free = None                                                  # event: the last copy out of _mode_host is done
        self.tab = ops.stream_tables(dev)
        self.nblk = np.zeros(S, dtype=np.int64)                                 # blocks pushed per slot since its last reset
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.refresh()

    # -- weights ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> None:
        """Re-pack the module's weights: BatchNorm folded into the convs (running statistics, bn.eps), GRU weights per layer as
        W_ih [g][3Hg][Hg] | W_hh | b_ih [g][3Hg] | b_hh."""
        m, lay, ch = self.model, self.lay, self.ch
        w = torch.zeros(lay["wtotal"], dtype=torch.float64)

        def put(name, t):
            t = t.detach().double().cpu().reshape(-1)
            w[lay[name]:lay[name] + t.numel()] = t

        for k in range(1, 5):
            s, sh = _bn_fold(getattr(m, f"bn{k}"))
            conv = getattr(m, f"conv{k}")
            put(f"encW{k}", conv.weight.detach().double().cpu() * s.view(-1, 1, 1, 1))
            put(f"encB{k}", conv.bias.detach().double().cpu() * s + sh)
            put(f"skW{k}", getattr(m, f"skip_connect_{k}").weight)
            convt = getattr(m, f"conv{k}_t")
            if k > 1:
                s, sh = _bn_fold(getattr(m, f"bn{k}_t"))
                put(f"decW{k}", convt.weight.detach().double().cpu() * s.view(1, -1, 1, 1))
                put(f"decB{k}", convt.bias.detach().double().cpu() * s + sh)
            else:
                put(f"decW{k}", convt.weight)
                put(f"decB{k}", convt.bias)
        put("ln1g", m.gru.ln1.weight)
        put("ln1b", m.gru.ln1.bias)
        put("ln2g", m.gru.ln2.weight)
        put("ln2b", m.gru.ln2.bias)
        self.ln1_eps, self.ln2_eps = float(m.gru.ln1.eps), float(m.gru.ln2.eps)
        w = w.float().to(self.device)
        packs = []
        for lst in (m.gru.gru_list1, m.gru.gru_list2):
            parts = [torch.stack([gr.weight_ih_l0 for gr in lst]), torch.stack([gr.weight_hh_l0 for gr in lst]),
                     torch.stack([gr.bias_ih_l0 for gr in lst]), torch.stack([gr.bias_hh_l0 for gr in lst])]
            packs.append(torch.cat([p.detach().float().reshape(-1).to(self.device) for p in parts]))
        if hasattr(self, "w"):                      # captured graphs hold these buffers: update them in place
            self.w.copy_(w)
            self.gru_pack1.copy_(packs[0])
            self.gru_pack2.copy_(packs[1])
        else:
            self.w, (self.gru_pack1, self.gru_pack2) = w, packs

    # -- the hop ----------------------------------------------------------------------------------------------------------
    def _chain(self, row: int) -> None:
        mode, lay, g, Hg = self.mode[row], self.lay, self.g, self.Hg
        ops.stream_encode(mode, self.ch, self.blocks, self.tab, self.w, self.state, self.work)
        ops.stream_gru(mode, 1, g, Hg, self.work, lay["wk_x"], self.state, lay["st_h1"], self.gru_pack1, self.work, lay["wk_h1n"])
        ops.stream_gru(mode, 2, g, Hg, self.work, lay["wk_h1n"], self.state, lay["st_h2"], self.gru_pack2, self.work, lay["wk_h2n"],
                       ln_g=self.w[lay["ln1g"]:lay["ln1g"] + self.H], ln_b=self.w[lay["ln1b"]:lay["ln1b"] + self.H],
                       ln_eps=self.ln1_eps)
        ops.stream_decode(mode, self.ch, self.tab, self.w, self.ln2_eps, self.state, self.work, self.out)

    def _launch(self, passes: int) -> None:
        rows = (0, 1) if passes == 2 else (1,)
        if not self.use_graph:
            for r in rows:
                self._chain(r)
            return
        gr = self._graphs.get(passes)
        if gr is None:
            torch.cuda.synchronize(self.device)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for r in rows:
                    self._chain(r)
            self._graphs[passes] = gr
        gr.replay()

    def _run(self, m0: np.ndarray, m1: np.ndarray) -> None:
        if self._host_free is not None:
            self._host_free.synchronize()
        hm = self._mode_host.numpy()
        hm[0], hm[1] = m0, m1
        self.mode.copy_(self._mode_host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._host_free = ev
        self._launch(2 if m0.any() else 1)

    @torch.no_grad()
    def push(self, blocks: torch.Tensor, active=None):
        """blocks [n_slots, 160] (the next block of every active slot; rows of inactive slots are ignored); active: bool per slot
        (None: all).  Returns (out [n_slots, 160] on the device, valid [n_slots] bool on the host): out[s] is the next enhanced
        block of slot s where valid[s]; inactive slots keep their state untouched."""
        S = self.S
        if tuple(blocks.shape) != (S, self.HOP):
            raise ValueError(f"push expects blocks of shape ({S}, {self.HOP}), got {tuple(blocks.shape)}")
        if active is None:
            act = np.ones(S, dtype=bool)
        else:
            act = (active.cpu().numpy() if torch.is_tensor(active) else np.asarray(active)).astype(bool).reshape(-1)
            if act.size != S:
                raise ValueError(f"active must have {S} entries, got {act.size}")
        self.blocks.copy_(blocks.to(torch.float32), non_blocking=True)
        b = self.nblk
        m0 = np.where(act & (b == 1), ops.STREAM_FRAME0, ops.STREAM_SKIP).astype(np.int32)
        m1 = np.where(act, np.where(b == 0, ops.STREAM_STORE, ops.STREAM_FRAME), ops.STREAM_SKIP).astype(np.int32)
        valid = act & (b >= 1)
        self.nblk += act
        self._run(m0, m1)
        return self.out.clone(), torch.from_numpy(valid)

    @torch.no_grad()
    def flush(self, slots) -> torch.Tensor:
        """End the clip of each slot in `slots`: computes its end frame and returns its last output block ([len(slots), 160],
        device), then resets the slot.  A slot must hold at least two blocks."""
        slots = [int(s) for s in (slots.tolist() if torch.is_tensor(slots) else slots)]
        for s in slots:
            if not 0 <= s < self.S:
                raise ValueError(f"slot {s} out of range [0, {self.S})")
            if self.nblk[s] < 2:
                raise ValueError(f"cannot flush slot {s}: it holds {self.nblk[s]} block(s), a clip needs at least 2 (L >= 320)")
        m1 = np.zeros(self.S, dtype=np.int32)
        m1[slots] = ops.STREAM_END
        self._run(np.zeros(self.S, dtype=np.int32), m1)
        idx = torch.tensor(slots, device=self.device, dtype=torch.long)
        last = self.out.index_select(0, idx)
        self.reset(slots)
        return last

    @torch.no_grad()
    def reset(self, slots=None) -> None:
        """Zero the state of `slots` (None: all): the next push to such a slot is block 0 of a new clip."""
        if slots is None:
            slots = list(range(self.S))
        slots = [int(s) for s in (slots.tolist() if torch.is_tensor(slots) else slots)]
        if slots:
            self.state.index_fill_(0, torch.tensor(slots, device=self.device, dtype=torch.long), 0.0)
        self.nblk[slots] = 0

    # -- inspection ---------------------------------------------------------------------------------------------------------
    def stage(self, slot: int) -> Dict[str, torch.Tensor]:
        """Views of slot `slot`'s last computed frame: re / im (161), e1..e4, skip1..skip4, gru1 / gru2 (group-contiguous), mask."""
        lay, ch, F = self.lay, self.ch, [160 >> k for k in range(5)]
        wk, st = self.work[slot], self.state[slot]
        out = {"re": wk[lay["wk_re"]:lay["wk_re"] + 161], "im": wk[lay["wk_im"]:lay["wk_im"] + 161],
               "gru1": wk[lay["wk_h1n"]:lay["wk_h1n"] + self.H], "gru2": wk[lay["wk_h2n"]:lay["wk_h2n"] + self.H],
               "mask": wk[lay["wk_mask"]:lay["wk_mask"] + 160], "e4": wk[lay["wk_x"]:lay["wk_x"] + self.H]}
        for k in range(1, 5):
            n = ch[k] * F[k]
            out[f"skip{k}"] = wk[lay[f"wk_skip{k}"]:lay[f"wk_skip{k}"] + n]
            if k < 4:
                out[f"e{k}"] = st[lay[f"st_prev{k}"]:lay[f"st_prev{k}"] + n]
        return out
