"""Corridor clearance: is the way there free for a vehicle of my size?  (dsim_corridor_clearance)

Line of sight casts a segment of zero thickness: a drone that sees its goal through a 0.3 m slot still cannot fly there.  The swept
watch holds the arithmetic for a thick segment, but serves one fixed chord.  :class:`Corridor` asks, for k candidate segments per
drone, the clearance of the drone's bounding sphere swept along each — against the obstacle set, or the placements of the drone's
scene where they stand now, and the ground: the one primitive behind a fan of candidate velocities, a thick visibility graph or an
edge check of a sampling planner.  The segment, the pieces and the outputs are specified in include/dronesim_amd.h.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as nat
from .drone_targets import offsets_tensor
from .obstacles import DeviceObstacles, DeviceScenes, scene_ids_tensor

MAX_K = nat.CORRIDOR_MAX_K


class CorridorClearance(NamedTuple):
    """What :meth:`Corridor.query` found: slot t of drone i."""

    clearance: torch.Tensor            # [k, n] float32: min(margin, c); -inf for a slot that was not evaluated or not served
    body: Optional[torch.Tensor]       # [k, n] int32: the body that attains it (instance-major g n_bodies + body on scenes), -2 the
                                       # ground, -1 when c >= margin or the slot was not evaluated; None when not asked for


class Corridor:
    """``world``: a :class:`DeviceObstacles` or a :class:`DeviceScenes` already on the device — made with a reach of at least
    :func:`obstacles.corridor_reach` — or None with ``ground``.  ``k`` (1 .. 32): the slots of every query.  ``margin`` > 0: the
    clearance is reported up to it.  ``sag`` >= 0: added to every radius (a type of radius 0 still asks, with the radius ``sag``).
    ``ground``: the half-space z <= 0 of the task frame counts too, as body -2.  ``offsets`` [N, 3] and ``scene_id`` [N] are in the
    CALLER's numbering (the world lies in the frame p_i - offset_i; scene_id is required with scenes, an id outside [0, K) meaning
    no obstacles).  ``type_id``: uint8 device tensor [n_pad] in storage order, required with several types.

    The object owns its outputs, fixed-address tensors [k, n_pad] in STORAGE order that a graph can hold: ``clearance_out``
    float32 and ``body_out`` int32, and the device counter of unserved slots."""

    def __init__(self, ctx, state, world, k, margin, sag=0.0, ground=False, offsets=None, scene_id=None, type_id=None):
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be a whole number of slots in 1 .. {MAX_K}")
        margin, sag = float(margin), float(sag)
        if not (np.isfinite(margin) and margin > 0.0):
            raise ValueError("margin must be finite and positive")
        if not (np.isfinite(sag) and sag >= 0.0):
            raise ValueError("sag must be finite and >= 0")
        if world is None and not ground:
            raise ValueError("no world at all: world=None needs ground=True")
        if world is not None and not isinstance(world, (DeviceObstacles, DeviceScenes)):
            raise TypeError("world takes a DeviceObstacles, a DeviceScenes or None")
        self.placed = isinstance(world, DeviceScenes)
        if self.placed and scene_id is None:
            raise ValueError("scene_id is required with obstacle scenes")
        if not self.placed and scene_id is not None:
            raise ValueError("scene_id without obstacle scenes")
        if len(ctx.types) > 1 and type_id is None:
            raise ValueError("type_id is required with several drone types")
        self.ctx, self.state, self.set, self.k, self.margin, self.sag = ctx, state, world, int(k), margin, sag
        # the longest segment served: 32 pieces of 2 half (1 - 2^-10), half = reach - (R_max + sag + margin), in the library's numbers
        if world is None:
            self.half, self.max_length = float("inf"), float("inf")
        else:
            r_max = max(float(np.float32(t.collision_sphere)) for t in ctx.types)
            self.half = float(np.float32(world.reach)) - (r_max + float(np.float32(sag)) + float(np.float32(margin)))
            if not self.half >= float(np.float32(world.reach)) / 1024.0:
                raise ValueError("the device set's reach leaves nothing for the pieces: make it with obstacles.corridor_reach(...)")
            self.max_length = 2.0 * nat.CORRIDOR_MAX_PIECES * self.half * (1.0 - 2.0 ** -10)
        order = getattr(state, "order", None) or getattr(ctx, "order", None)
        n, n_pad, dev = state.n, state.n_pad, ctx.device
        self._scene_id = scene_ids_tensor(scene_id, n, n_pad, dev, order) if self.placed else None
        self._off = offsets_tensor(offsets, n, n_pad, order, dev)
        self._type_id = type_id
        self.clearance_out = torch.full((self.k, n_pad), float("-inf"), dtype=torch.float32, device=dev)
        self.body_out = torch.full((self.k, n_pad), -1, dtype=torch.int32, device=dev)
        self._unserved = torch.zeros((1,), dtype=torch.int64, device=dev)
        a = self.args = nat.CorridorArgs()
        a.k, a.flags = self.k, (nat.CORRIDOR_GROUND if ground else 0)
        a.offset = self._off.data_ptr() if self._off is not None else None
        a.type_id = type_id.data_ptr() if type_id is not None else None
        a.scenes = world.handle if self.placed else None
        a.scene_id = self._scene_id.data_ptr() if self.placed else None
        a.margin, a.sag = margin, sag
        a.clearance_out = self.clearance_out.data_ptr()
        a.unserved_out = self._unserved.data_ptr()

    def _padded(self, t, name, dtype, mid):
        """``t`` as the library reads it: [k, *mid, n_pad] contiguous, or its first n drones cut from such a tensor.  ValueError
        otherwise."""
        n, n_pad = self.state.n, self.state.n_pad
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.clearance_out.device:
            raise ValueError(f"{name} must be a {dtype} tensor on the fleet's device")
        full, cut = (self.k, *mid, n_pad), (self.k, *mid, n)
        strides = tuple(torch.empty(full, device="meta").stride())
        if not ((tuple(t.shape) == full or tuple(t.shape) == cut) and tuple(t.stride()) == strides):
            raise ValueError(f"{name} must be a contiguous {list(full)} in storage order, or its first {n} drones")
        return t

    def query(self, rel, index=None, body: bool = True) -> CorridorClearance:
        """Enqueues one dsim_corridor_clearance on the current stream (it may be captured into a graph).  ``rel`` float32
        [k, 3, n_pad] in storage order (or its first n drones, cut from such a tensor): slot t of drone i sweeps its sphere from
        p_i - offset_i along rel[t, :, i], to its end.  ``index`` int32 [k, n_pad] (likewise) or None: a slot whose index is
        negative is not evaluated.  Returns ``CorridorClearance(clearance, body)``: views [k, n] of the object's own tensors, in
        storage order, overwritten by the next query; ``body=False`` leaves that output unwritten (None is returned for it).  A slot
        that is not evaluated — a negative index, a non-finite rel or position — or not served — longer than ``max_length`` —
        reads -inf / -1."""
        rel = self._padded(rel, "rel", torch.float32, (3,))
        if index is not None:
            index = self._padded(index, "index", torch.int32, ())
        a = self.args
        a.rel, a.index = rel.data_ptr(), (index.data_ptr() if index is not None else None)
        a.body_out = self.body_out.data_ptr() if body else None
        self._inputs = (rel, index)                # (the kernel reads these asynchronously on the stream)
        world = self.set.handle if (self.set is not None and not self.placed) else None
        nat.check(self.ctx.lib.dsim_corridor_clearance(
            self.ctx.handle, self.ctx.stream_ptr(), self.state.n, self.state.view(), world, ctypes.byref(a)))
        n = self.state.n
        return CorridorClearance(self.clearance_out[:, :n], self.body_out[:, :n] if body else None)

    def unserved(self) -> int:
        """Slots x queries so far whose segment was longer than ``max_length`` (synchronises the stream): they read -inf."""
        return int(self._unserved.item())

    def fan(self, directions, length) -> torch.Tensor:
        """``directions`` [k, 3] (world axes, used as given: unit vectors for a fan of the radius ``length``) and a length [m] ->
        the ``rel`` tensor float32 [k, 3, n_pad] of a query in which every drone asks the same k segments."""
        d = np.asarray(directions, dtype=np.float64)
        if d.shape != (self.k, 3) or not np.isfinite(d).all():
            raise ValueError(f"directions must be a finite [{self.k}, 3]")
        if not (np.isfinite(length) and float(length) >= 0.0):
            raise ValueError("length must be finite and >= 0")
        rel = torch.from_numpy((d * float(length)).astype(np.float32)).to(self.clearance_out.device)
        return rel[:, :, None].expand(self.k, 3, self.state.n_pad).contiguous()

    def graph_keepalive(self):
        """What a captured query() holds the addresses of, for the owner of the graph to keep alive."""
        return (self.clearance_out, self.body_out, self._unserved, self._off, self._scene_id, self._type_id) + tuple(getattr(self, "_inputs", ()))

    def close(self) -> None:
        """Releases what the object holds (the world is the caller's and stays)."""
        self.clearance_out = self.body_out = self._unserved = self._off = self._scene_id = None
        self._inputs = ()
        self.set = None
