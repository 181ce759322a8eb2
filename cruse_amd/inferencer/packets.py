"""The schedule of streaming inference in packets: which frames a slot computes and which output blocks become valid when it holds
`b` blocks and consumes `c` more in one call.  Pure Python (no torch, no device): StreamingInferencer.push_packet and the host
tests share it.

Frame t of a clip covers blocks t-1 and t (frame 0: the reflection of block 0 with x[160] from block 1, so it needs block 1); it
yields output block t-1.  The end frame nb (the last block and its end reflection) belongs to flush.
"""
from __future__ import annotations

from typing import NamedTuple

HOP = 160


class PacketPlan(NamedTuple):
    first_frame: int     # clip index of the first frame computed in this call
    n_frames: int        # frames computed, first_frame .. first_frame + n_frames - 1
    first_out: int       # clip index of the first output block returned
    n_out: int           # output blocks returned, in order
    start: int           # what the kernels are told about b: min(b, 2)


def packet_plan(b: int, c: int) -> PacketPlan:
    """Slot holds `b` blocks (since its last reset) and consumes `c >= 0` more."""
    if b < 0 or c < 0:
        raise ValueError(f"packet_plan: b = {b}, c = {c} must be >= 0")
    start = min(b, 2)
    if c == 0:
        return PacketPlan(b, 0, max(b - 1, 0), 0, start)
    if b == 0:           # block 0 is only stored; with c >= 2 frames 0 .. c-1 follow in the same call
        return PacketPlan(0, c if c >= 2 else 0, 0, c - 1, start)
    if b == 1:           # frame 0 became computable with the first new block: c + 1 frames for c output blocks
        return PacketPlan(0, c + 1, 0, c, start)
    return PacketPlan(b, c, b - 1, c, start)


def flush_plan(b: int) -> PacketPlan:
    """The end frame of a clip of `b >= 2` blocks: frame b, output block b-1."""
    if b < 2:
        raise ValueError(f"flush_plan: a clip needs at least 2 blocks, got {b}")
    return PacketPlan(b, 1, b - 1, 1, 2)


def df_packet_plan(b: int, c: int) -> PacketPlan:
    """packet_plan for the DeepFilter head (StreamingInferencer(head="df")): the same frames, but the head's row t needs frame t + 1,
    so a slot that has consumed b >= 2 blocks has returned b - 2 of them (30 ms behind instead of 20)."""
    p = packet_plan(b, c)
    first_out = max(b - 2, 0)
    return PacketPlan(p.first_frame, p.n_frames, first_out, max(b + c - 2, 0) - first_out, p.start)


def df_flush_plan(b: int) -> PacketPlan:
    """The end frame of a clip of `b >= 2` blocks and the drain step of the head: output blocks b-2 and b-1."""
    p = flush_plan(b)
    return PacketPlan(p.first_frame, p.n_frames, b - 2, 2, p.start)


def padded_blocks(L: int) -> int:
    """Blocks of a clip of L samples, its last block zero-padded to 160."""
    return (L + HOP - 1) // HOP
