"""Targets' period of a fleet whose targets repeat (env replicas of one task) and the dsim_step_args.tgt_period it hands to the
fused step (CPU only: a Targets on host memory, a recording stand-in for the library)."""
import ctypes

import numpy as np
import torch

from dronesim_amd import _native as nat
from dronesim_amd.fleet import Targets, frozen

from .test_targets_hint_cpu import _fake_env

P, REPS = 4096, 4
N = P * REPS


def _ctx():
    import types
    return types.SimpleNamespace(device=torch.device("cpu"), order=None)


def _grid(n_task=P, reps=REPS, side=64):
    """bench.py's config-2 fleet: a side x side grid at 1 m pitch, z = 0.5, tiled `reps` times ([3, n])."""
    ij = np.arange(n_task)
    xyz = np.stack([(ij % side) * 1.0, (ij // side) * 1.0, np.full(n_task, 0.5)])
    return np.tile(xyz, (1, reps)).astype(np.float32)


def _bits(x):
    return [int(b) for b in np.asarray(x, dtype=np.float32).ravel().view(np.uint32)]


def test_tiled_grid_has_its_period():
    for layout in ("soa", "tile64", "tile256", "tile1024", "tile4096"):
        tg = Targets(_ctx(), N, layout)
        tg.set(pos=_grid(), yaw=0.4)
        assert tg.tgt_period() == P, layout
        a = nat.StepArgs()
        tg.fill_period_hint(a)
        assert a.tgt_period == P
    tg = Targets(_ctx(), N)
    tg.set(pos=torch.as_tensor(_grid()))                    # a CPU tensor is host memory too
    assert tg.tgt_period() == P


def test_fresh_and_constant_fleets_repeat_with_one_tile():
    assert Targets(_ctx(), N).tgt_period() == 256           # every group constant (+0.0): a period of 1, taken to a whole tile
    assert Targets(_ctx(), N, "tile1024").tgt_period() == 1024
    tg = Targets(_ctx(), N)
    tg.set(pos=[1.0, 2.0, 3.0], vel=np.zeros((3, N), np.float32), yaw=0.4)    # per drone but all equal
    assert tg.tgt_period() == 256
    assert Targets(_ctx(), 256).tgt_period() == 0           # one tile: no period below the fleet
    assert Targets(_ctx(), N, broadcast=True).tgt_period() == 0


def test_random_positions_have_none():
    tg = Targets(_ctx(), N)
    tg.set(pos=np.random.default_rng(1).uniform(-5, 5, (3, N)).astype(np.float32))
    assert tg.tgt_period() == 0
    a = nat.StepArgs()
    a.tgt_period = 77
    tg.fill_period_hint(a)
    assert a.tgt_period == 0


def test_a_coincidence_is_not_a_period():
    pos = _grid()
    pos[:, 1000] = pos[:, 0]                                # column 0 recurs early, but the fleet does not repeat with it
    tg = Targets(_ctx(), N)
    tg.set(pos=pos)
    assert tg.tgt_period() == 0
    pos = _grid()
    pos[2, N - 1] = 0.75                                    # the last replica differs in one float
    tg.set(pos=pos)
    assert tg.tgt_period() == 0


def test_signed_zero_is_compared_by_bits():
    pos = np.zeros((3, N), np.float32)
    pos[0, P:] = -0.0                                      # equal as floats, not as bits
    tg = Targets(_ctx(), N)
    tg.set(pos=pos)
    assert tg.tgt_period() == 0
    pos[0, :] = -0.0
    tg.set(pos=pos)
    assert tg.tgt_period() == 256


def test_ragged_fleet_has_none():
    n = N - 48
    tg = Targets(_ctx(), n)
    tg.set(pos=_grid()[:, :n], yaw=0.4)
    assert tg.n_pad > n and tg.tgt_period() == 0
    assert Targets(_ctx(), n).tgt_period() == 0


def test_period_not_a_multiple_of_256():
    # a task of 384 drones: the fleet repeats with lcm(384, 256) = 768 drones when that divides it, otherwise it has no period
    t = np.random.default_rng(2).uniform(-5, 5, (3, 384)).astype(np.float32)
    tg = Targets(_ctx(), 768 * 4)
    tg.set(pos=np.tile(t, (1, 8)))
    assert tg.tgt_period() == 768
    # a task of 300 drones on 19 200: lcm(300, 256) = 19 200 is the whole fleet, no period below it
    t3 = np.random.default_rng(5).uniform(-5, 5, (3, 300)).astype(np.float32)
    tg = Targets(_ctx(), 19200)
    tg.set(pos=np.tile(t3, (1, 64)))
    assert tg.n == tg.n_pad and tg.tgt_period() == 0
    # a task of 100 drones: lcm(100, 256) = 6 400
    t = np.random.default_rng(3).uniform(-5, 5, (3, 100)).astype(np.float32)
    tg = Targets(_ctx(), 12800)
    tg.set(pos=np.tile(t, (1, 128)))
    assert tg.tgt_period() == 6400
    # blocks larger than the task: the period of the tile4096 layout is a whole block
    tg = Targets(_ctx(), 8192, "tile4096")
    tg.set(pos=np.tile(_grid(1024, 1, 32), (1, 8)))
    assert tg.tgt_period() == 4096


def test_groups_combine_by_their_common_multiple():
    tg = Targets(_ctx(), N)
    tg.set(pos=_grid(), vel=np.tile(np.random.default_rng(4).uniform(-1, 1, (3, 512)).astype(np.float32), (1, N // 512)))
    assert tg.tgt_period() == P
    tg.set(pos=np.tile(_grid(1024, 1, 32), (1, N // 1024)))
    assert tg.tgt_period() == 1024
    tg.set(acc=frozen(torch.zeros(3, N)))                   # a Frozen: not known to repeat
    assert tg.tgt_period() == 0
    tg.set(acc=[0.0, 0.0, 0.0])                             # constant again
    assert tg.tgt_period() == 1024


def test_handed_out_or_written_behind_set_ends_it():
    for how in ("data", "fields", "raw_fields", "assign", "set_fields"):
        tg = Targets(_ctx(), N)
        tg.set(pos=_grid(), yaw=0.4)
        assert tg.tgt_period() == P
        if how == "data":
            tg.data[0, 5] = 1.0
        elif how == "fields":
            tg.fields(0, 10)
        elif how == "raw_fields":
            tg.raw_fields(0, 3)
        elif how == "assign":
            tg.data = torch.zeros_like(tg._data)
        else:
            tg.set_fields(9, torch.full((1, N), 0.4))
        assert tg.tgt_period() == 0, how
        tg.set(pos=_grid(), vel=[0.0, 0.0, 0.0], acc=[0.0, 0.0, 0.0], yaw=0.4)
        assert tg.tgt_period() == (P if how == "set_fields" else 0), how     # recorded again by set(); a hand-out is for good


def test_hint_epoch_and_const_hint_do_not_move_with_the_period():
    tg = Targets(_ctx(), N)
    tg.set(pos=_grid(), yaw=0.4)
    e, h = tg.hint_epoch, tg.const_hint()
    assert h == (0xE, [0] * 9 + _bits(0.4))
    for pos in (np.random.default_rng(6).uniform(-5, 5, (3, N)).astype(np.float32), _grid(), np.tile(_grid(1024, 1, 32), (1, 16))):
        tg.set(pos=pos)
        assert tg.hint_epoch == e and tg.const_hint() == h
    tg.set(vel=np.tile(_grid(256, 1, 16), (1, N // 256)))   # a constant group goes per drone (periodic): the epoch moves for that
    assert tg.hint_epoch == e + 1 and tg.tgt_period() == 1024
    tg.set(vel=np.random.default_rng(7).uniform(-5, 5, (3, N)).astype(np.float32))
    assert tg.hint_epoch == e + 1 and tg.tgt_period() == 0


class _Lib:
    def __init__(self):
        self.calls = []

    def dsim_step(self, h, s, n, sview, tview, ref):
        a = ref._obj
        self.calls.append((bool(a.options & nat.OPT_TGT_CONST), a.tgt_const_mask, a.tgt_period))
        return 0


def test_prepared_block_is_reused_with_its_period_refreshed():
    e = _fake_env(N)
    e.ctx.lib = _Lib()
    calls = e.ctx.lib.calls
    tg = Targets(e.ctx, N, "tile64")
    tg.set(pos=_grid(), yaw=0.4)
    e.step_fused(tg)
    e.step_fused(tg)                                        # the prepared block, replayed
    assert calls == [(True, 0xE, P)] * 2
    plan = e._fused_plan
    assert plan is not None
    tg.set(pos=np.random.default_rng(8).uniform(-5, 5, (3, N)).astype(np.float32))
    e.step_fused(tg)                                        # per-drone positions without a period: the same block, refreshed
    assert e._fused_plan is plan and calls[-1] == (True, 0xE, 0)
    tg.set(pos=np.tile(_grid(1024, 1, 32), (1, N // 1024)))
    e.step_fused(tg)
    assert e._fused_plan is plan and calls[-1] == (True, 0xE, 1024)
    tg.set(pos=_grid())
    e.step_fused(tg)
    assert e._fused_plan is plan and calls[-1] == (True, 0xE, P)
    tg.data[0, 0] = 1.0                                      # handed out: neither hint from the next call on
    e.step_fused(tg)
    e.step_fused(tg)
    assert calls[-2:] == [(False, 0, 0)] * 2


def test_binding_layout():
    assert nat.ABI_VERSION == 11
    assert nat.StepArgs.tgt_period.offset % 8 == 0
    assert nat.StepArgs.tgt_period.offset > nat.StepArgs.tgt_const.offset
    assert ctypes.sizeof(nat.StepArgs) == nat.StepArgs.tgt_period.offset + 8
