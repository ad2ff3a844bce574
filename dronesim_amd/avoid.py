"""Velocity safety filter: the smallest change of a wished velocity that meets the control-barrier half-spaces of a drone's floor,
obstacle witnesses and neighbours (dsim_velocity_filter).

The nearest-neighbour observation, the obstacle witnesses and their velocities were made for this consumer.  Per drone the wished
velocity ``u`` becomes ``v = argmin |v - u|^2`` subject to ``a_j . v >= b_j`` for at most 25 rows, built inside the kernel from the
records: the floor (bit 0 of ``dropped``), the obstacle slots (bits 1 .. 8: ``h = clearance - buffer_obstacle``, the witness's
velocity on moving scenes) and the neighbour slots (bits 9 .. 24: ``h = dist - (R_i + R_j) - buffer_drone``, reciprocal — drone i
takes ``share`` of the change the pair needs).  Rows that cannot all be met are dropped greedily in that order, and ``v`` is the
exact projection onto the rows kept; a drone with nothing to change gets ``v == u`` bit for bit.  The rows, the drop rule and what
is no row are specified in include/dronesim_amd.h.  There is no speed cap in the program: whoever turns ``v`` into a command
clamps it, and that clamp can undo a row.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as nat
from .drone_targets import offsets_tensor

FLOOR_BIT, OBSTACLE_BIT, NEIGHBOR_BIT, ROWS = nat.FILTER_FLOOR_BIT, nat.FILTER_OBSTACLE_BIT, nat.FILTER_NEIGHBOR_BIT, nat.FILTER_ROWS


class Filtered(NamedTuple):
    """What :meth:`VelocityFilter.apply` answers, in storage order."""

    vel: torch.Tensor        # [3, n] float32: the filtered velocity
    dropped: torch.Tensor    # [n] int32: bit 0 the floor, 1 + s obstacle slot s, 9 + t neighbour slot t — rows that could not be kept


def check_options(alpha, buffer_drone=0.0, buffer_obstacle=0.0, share=0.5, floor=None):
    """The filter's constants as the library takes them, or ValueError: (alpha, buffer_drone, buffer_obstacle, share, floor)."""
    num = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
    if not num(alpha) or not math.isfinite(alpha) or not alpha > 0.0:
        raise ValueError(f"alpha must be finite and positive, got {alpha!r}")
    if not num(share) or not 0.0 < share <= 1.0:
        raise ValueError(f"share must lie in (0, 1], got {share!r}")
    for name, x in (("buffer_drone", buffer_drone), ("buffer_obstacle", buffer_obstacle)):
        if not num(x) or not math.isfinite(x) or x < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {x!r}")
    if floor is not None and (not num(floor) or not math.isfinite(floor)):
        raise ValueError(f"floor must be None or a finite height, got {floor!r}")
    return float(alpha), float(buffer_drone), float(buffer_obstacle), float(share), None if floor is None else float(floor)


class VelocityFilter:
    """``alpha`` [1/s]: the barrier's rate, ``h' + alpha h >= 0``.  ``buffer_drone`` / ``buffer_obstacle`` [m]: kept between two
    bounding spheres, and between a sphere and the world.  ``share`` in (0, 1]: the part of a pair's change this drone takes (1/2:
    both filter).  ``floor``: the height of a floor in the task frame, or None for no floor row.  ``offsets`` [N, 3] in the
    CALLER's numbering (the floor lies in the frame p_i - offset_i).  ``type_id``: uint8 [n_pad] on the device in STORAGE order,
    required with more than one type (the radii R_i, and R_j through the neighbours' indices).

    The object owns two device counters (:meth:`counters`) and, without ``out``, the outputs of the last call."""

    def __init__(self, ctx, state, alpha, buffer_drone=0.0, buffer_obstacle=0.0, share=0.5, floor=None, offsets=None, type_id=None):
        self.alpha, self.buffer_drone, self.buffer_obstacle, self.share, self.floor = check_options(alpha, buffer_drone, buffer_obstacle,
                                                                                                    share, floor)
        if len(ctx.types) > 1 and type_id is None:
            raise ValueError("type_id ([n_pad] uint8, storage order) is required with more than one type")
        if type_id is not None and (not isinstance(type_id, torch.Tensor) or type_id.dtype != torch.uint8
                                    or tuple(type_id.shape) != (state.n_pad,)):
            raise ValueError(f"type_id must be a uint8 tensor [{state.n_pad}]")
        self.ctx, self.state, self._type_id = ctx, state, type_id
        order = getattr(state, "order", None) or getattr(ctx, "order", None)
        self._off = offsets_tensor(offsets, state.n, state.n_pad, order, ctx.device)
        self._counters = self._vel = self._dropped = None

    def _padded(self, t, name, dtype, lead):
        """``t`` as the library reads it: [*lead, n_pad] contiguous, or its first n drones cut from such a tensor."""
        n, n_pad = self.state.n, self.state.n_pad
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"{name} must be a {dtype} tensor")
        full, cut = (*lead, n_pad), (*lead, n)
        strides = tuple(torch.empty(full, device="meta").stride())
        if not ((tuple(t.shape) == full or tuple(t.shape) == cut) and tuple(t.stride()) == strides):
            raise ValueError(f"{name} must be a contiguous {list(full)} in storage order, or its first {n} drones")
        return t

    def apply(self, u, neighbors=None, witnesses=None, out: Optional[Filtered] = None) -> Filtered:
        """Enqueues one dsim_velocity_filter on the current stream.  ``u`` float32 [3, n_pad] in storage order (or its first n
        drones).  ``neighbors``: a :class:`~dronesim_amd.downwash.Neighbors` record in storage order with dist, rel_pos and
        rel_vel (Downwash.nearest); ``witnesses``: an :class:`~dronesim_amd.obstacles.ObstacleWitnesses` record in storage order
        and world axes (obstacles.witnesses / witnesses_scenes), ``vel`` used when it is there.  At least one of the two, or a
        floor.  ``out``: a ``Filtered`` of pre-allocated tensors over the padded fleet (vel [3, n_pad] float32, dropped [n_pad]
        int32): the call writes them at their fixed addresses.  Returns views of the first n drones."""
        n, n_pad = self.state.n, self.state.n_pad
        u = self._padded(u, "u", torch.float32, (3,))
        a = nat.FilterArgs()
        if neighbors is not None:
            if neighbors.index is None or neighbors.dist is None or neighbors.rel_pos is None or neighbors.rel_vel is None:
                raise ValueError("the neighbour record needs index, dist, rel_pos and rel_vel (Downwash.nearest(rel_vel=True))")
            k = int(neighbors.index.shape[0])
            if not 1 <= k <= nat.KNN_MAX_K:
                raise ValueError(f"the neighbour record must have 1 .. {nat.KNN_MAX_K} slots")
            a.k = k
            a.nb_index = self._padded(neighbors.index, "neighbors.index", torch.int32, (k,)).data_ptr()
            a.nb_dist = self._padded(neighbors.dist, "neighbors.dist", torch.float32, (k,)).data_ptr()
            a.nb_rel_pos = self._padded(neighbors.rel_pos, "neighbors.rel_pos", torch.float32, (k, 3)).data_ptr()
            a.nb_rel_vel = self._padded(neighbors.rel_vel, "neighbors.rel_vel", torch.float32, (k, 3)).data_ptr()
        if witnesses is not None:
            if witnesses.clearance is None or witnesses.body is None or witnesses.rel is None:
                raise ValueError("the witness record needs clearance, body and rel")
            m = int(witnesses.clearance.shape[0])
            if not 1 <= m <= nat.WITNESSES_MAX:
                raise ValueError(f"the witness record must have 1 .. {nat.WITNESSES_MAX} slots")
            a.m = m
            a.wit_clearance = self._padded(witnesses.clearance, "witnesses.clearance", torch.float32, (m,)).data_ptr()
            a.wit_body = self._padded(witnesses.body, "witnesses.body", torch.int32, (m,)).data_ptr()
            a.wit_rel = self._padded(witnesses.rel, "witnesses.rel", torch.float32, (m, 3)).data_ptr()
            if witnesses.vel is not None:
                a.wit_vel = self._padded(witnesses.vel, "witnesses.vel", torch.float32, (m, 3)).data_ptr()
        if neighbors is None and witnesses is None and self.floor is None:
            raise ValueError("nothing to filter against: pass neighbors, witnesses or make the filter with a floor")
        if out is not None:
            vel = self._padded(out.vel, "out.vel", torch.float32, (3,))
            dropped = self._padded(out.dropped, "out.dropped", torch.int32, ())
            if tuple(vel.shape) != (3, n_pad) or tuple(dropped.shape) != (n_pad,):
                raise ValueError(f"out must hold vel [3, {n_pad}] float32 and dropped [{n_pad}] int32")
        else:
            if self._vel is None:
                self._vel = torch.zeros((3, n_pad), dtype=torch.float32, device=self.ctx.device)
                self._dropped = torch.zeros((n_pad,), dtype=torch.int32, device=self.ctx.device)
            vel, dropped = self._vel, self._dropped
        if self._counters is None:
            self._counters = torch.zeros((2,), dtype=torch.int64, device=self.ctx.device)
        a.u, a.v_out, a.dropped_out, a.counters = u.data_ptr(), vel.data_ptr(), dropped.data_ptr(), self._counters.data_ptr()
        a.offset = self._off.data_ptr() if self._off is not None else None
        a.type_id = self._type_id.data_ptr() if self._type_id is not None else None
        a.alpha, a.share, a.buffer_drone, a.buffer_obstacle = self.alpha, self.share, self.buffer_drone, self.buffer_obstacle
        a.floor, a.has_floor = (self.floor, 1) if self.floor is not None else (0.0, 0)
        self._inputs = (u, neighbors, witnesses, vel, dropped)        # (the kernel reads and writes these asynchronously on the stream)
        nat.check(self.ctx.lib.dsim_velocity_filter(self.ctx.handle, self.ctx.stream_ptr(), n, self.state.view(), ctypes.byref(a)))
        return Filtered(vel[:, :n], dropped[:n])

    def counters(self):
        """(drones whose velocity was changed, drones with a dropped row), summed over this object's calls (synchronises the stream)."""
        if self._counters is None:
            return 0, 0
        c = self._counters.cpu()
        return int(c[0]), int(c[1])
