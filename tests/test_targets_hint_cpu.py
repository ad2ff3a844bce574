"""Targets' record of its constant field groups and the DSIM_OPT_TGT_CONST arguments built from it (CPU only: a Targets on
host memory, no library call)."""
import ctypes
import types

import numpy as np
import torch

from dronesim_amd import _native as nat
from dronesim_amd.fleet import Targets, frozen

N = 300          # a ragged fleet: n < n_pad


def _ctx():
    return types.SimpleNamespace(device=torch.device("cpu"), order=None)


def _args(tg):
    a = nat.StepArgs()
    tg.fill_const_hint(a)
    bits = list((ctypes.c_uint32 * 10).from_address(ctypes.addressof(a) + nat.StepArgs.tgt_const.offset))
    return bool(a.options & nat.OPT_TGT_CONST), a.tgt_const_mask, bits


def _bits(x):
    return [int(b) for b in np.asarray(x, dtype=np.float32).ravel().view(np.uint32)]


def _held(tg, f0, nf):
    return tg._data[f0:f0 + nf, :N]


def test_fresh_object_is_all_zero_constants():
    tg = Targets(_ctx(), N)
    assert tg.const_hint() == (0xF, [0] * 10)
    assert _args(tg) == (True, 0xF, [0] * 10)
    assert _args(Targets(_ctx(), N, broadcast=True))[0] is False


def test_constant_per_drone_constant():
    tg = Targets(_ctx(), N)
    pos = np.arange(3 * N, dtype=np.float32).reshape(3, N)
    tg.set(pos=pos, yaw=0.4)
    assert _args(tg) == (True, 0xE, [0] * 9 + _bits(0.4))
    v0 = tg.version
    tg.set(yaw=0.4, vel=[0.0, 0.0, 0.0])          # the same bits: no fill
    assert tg.version == v0
    tg.set(vel=torch.ones(3, N))                   # per drone
    assert _args(tg)[:2] == (True, 0xC)
    assert torch.equal(_held(tg, 3, 3), torch.ones(3, N))
    tg.set(vel=[1.0, 2.0, 3.0])                    # constant again
    assert _args(tg) == (True, 0xE, [0, 0, 0] + _bits([1, 2, 3]) + [0, 0, 0] + _bits(0.4))
    assert torch.equal(_held(tg, 3, 3), torch.tensor([1.0, 2.0, 3.0]).reshape(3, 1).expand(3, N))
    assert tg.version > v0
    tg.set(pos=[1.0, 1.0, 1.0])
    assert _args(tg)[1] == 0xF
    fz = frozen(torch.zeros(3, N))                  # a Frozen tensor is per-drone data
    tg.set(pos=fz)
    assert _args(tg)[1] == 0xE


def test_signed_zero_and_nan_bits():
    tg = Targets(_ctx(), N)
    v0 = tg.version
    tg.set(vel=[-0.0, 0.0, 0.0])                   # differs from +0.0 in its bits: filled, recorded
    assert tg.version == v0 + 1
    assert _args(tg)[2][3:6] == _bits([-0.0, 0.0, 0.0])
    assert _bits(_held(tg, 3, 1)[0, :1].numpy()) == _bits(-0.0)
    tg.set(vel=[-0.0, 0.0, 0.0])
    assert tg.version == v0 + 1
    nan = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]
    tg.set(yaw=nan)
    assert _args(tg)[2][9] == 0x7FC00001
    assert _bits(_held(tg, 9, 1)[0, :1].numpy()) == [0x7FC00001]
    v1 = tg.version
    tg.set(yaw=nan)                                 # the same bits: nothing to fill
    assert tg.version == v1
    tg.set(yaw=np.array([0x7FC00002], dtype=np.uint32).view(np.float32)[0])
    assert tg.version == v1 + 1 and _args(tg)[2][9] == 0x7FC00002


def test_set_fields_clears_every_group():
    tg = Targets(_ctx(), N)
    tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
    tg.set_fields(9, torch.full((1, N), 0.4))
    assert tg.const_hint() is None and _args(tg) == (False, 0, [0] * 10)
    tg.set(vel=[0.0, 0.0, 0.0], acc=[0.0, 0.0, 0.0], yaw=0.4)     # recorded again by set()
    assert _args(tg)[1] == 0xE


def test_handed_out_tensor_ends_the_hint():
    for how in ("data", "fields", "raw_fields", "assign"):
        tg = Targets(_ctx(), N)
        tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
        e0 = tg.hint_epoch
        if how == "data":
            tg.data[3, :] = 1.0
        elif how == "fields":
            tg.fields(0, 10)
        elif how == "raw_fields":
            tg.raw_fields(3, 3)
        else:
            tg.data = torch.zeros_like(tg._data)
        assert tg.const_hint() is None and _args(tg)[0] is False, how
        assert tg.hint_epoch == e0 + 1, how                # (prepared launches keyed on the hint are rebuilt)
        tg.set(yaw=0.5)
        assert tg.const_hint() is None, how            # for good
    tiled = Targets(_ctx(), 512, layout="tile256")
    tiled.fields(0, 3)                                 # a gathered copy: nothing handed out
    assert tiled.const_hint()[0] == 0xF


def test_reallocation_keeps_the_record():
    tg = Targets(_ctx(), N)
    tg.set(pos=np.ones((3, N), np.float32), yaw=0.4)
    before = _args(tg)
    keep = torch.empty_like(tg._data)                  # what placement does: copy into the chosen block, swap the private tensor
    keep.copy_(tg._data)
    tg._data = keep
    assert _args(tg) == before
    assert tg._data.data_ptr() == keep.data_ptr()



def test_hint_epoch_moves_with_the_hint_only():
    tg = Targets(_ctx(), N)
    tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
    e = tg.hint_epoch
    tg.set(pos=np.ones((3, N), np.float32))                # per-drone data again: a fill, the hint unchanged
    assert tg.hint_epoch == e and tg.version > 0
    tg.set(yaw=0.4)
    assert tg.hint_epoch == e
    tg.set(yaw=0.5)
    assert tg.hint_epoch == e + 1
    tg.set(acc=torch.zeros(3, N))                           # a constant group goes per drone
    assert tg.hint_epoch == e + 2
    tg.set_fields(0, torch.zeros(3, N))
    assert tg.hint_epoch == e + 3 and tg.const_hint() is None


# ---- the arguments the env's fused step and the controller build, with a recording stand-in for the library ----------------

class _Lib:
    def __init__(self):
        self.calls = []

    def _rec(self, name, ref):
        a = ref._obj
        bits = list((ctypes.c_uint32 * 10).from_address(ctypes.addressof(a) + nat.StepArgs.tgt_const.offset))
        self.calls.append((name, bool(a.options & nat.OPT_TGT_CONST), a.tgt_const_mask, bits))
        return 0

    def dsim_step(self, h, s, n, sview, tview, ref):
        return self._rec("step", ref)

    def dsim_control2(self, h, s, n, sview, tview, ref, *outs):
        return self._rec("control", ref)


def _fake_ctx():
    return types.SimpleNamespace(device=torch.device("cpu"), order=None, n_fields=nat.NF_QUAD, n_act=4, placement=False,
                                 lib=_Lib(), handle=None, stream_ptr=lambda: None, read_room=None)


def _fake_env(n=N):
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import FleetState
    e = CtrlAviary.__new__(CtrlAviary)
    ctx = _fake_ctx()
    e.ctx, e.NUM_DRONES, e.state = ctx, n, FleetState(ctx, n)
    e.AGGR_PHY_STEPS, e.TIMESTEP, e._phys_options, e._tuning, e.noise_seed, e._env_steps = 1, 1 / 240, 0, 0, 0, 0
    e._downwash = e._fb_event = e._fb_stream = e._runs = e.order = e._dyn_rates = e._type_id = None
    e._fused_plan = e._fused_plan_dw = None
    e._chained_enabled = e._chain_live = e._graph_made = False
    e._chain_ok, e.n_act, e.step_counter, e._use_last_action = True, 4, 0, False
    return e


def test_env_fused_step_args_for_each_history():
    e = _fake_env()
    calls = e.ctx.lib.calls
    tg = Targets(e.ctx, N)
    tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
    e.step_fused(tg)
    e.step_fused(tg)                                        # the prepared block, replayed
    assert calls[-2:] == [("step", True, 0xE, [0] * 9 + _bits(0.4))] * 2
    assert e._fused_plan is not None
    plan = e._fused_plan
    tg.set(pos=np.ones((3, N), np.float32))                 # new per-drone positions: still the prepared block
    e.step_fused(tg)
    assert e._fused_plan is plan and calls[-1][1:3] == (True, 0xE)
    tg.set(acc=[0.1, -0.2, 0.3], yaw=-0.25)                  # a constant changed: the block is rebuilt with the new bits
    e.step_fused(tg)
    assert e._fused_plan is not plan
    assert calls[-1] == ("step", True, 0xE, [0, 0, 0] + [0, 0, 0] + _bits([0.1, -0.2, 0.3]) + _bits(-0.25))
    e.step_fused(tg)
    assert calls[-1] == calls[-2]
    tg.set(vel=torch.ones(3, N))                             # vel per drone: the mask says so (the library then reads the view)
    e.step_fused(tg)
    assert calls[-1][1:3] == (True, 0xC)
    tg.set(vel=[0.0, 0.0, 0.0])
    e.step_fused(tg)
    assert calls[-1][1:3] == (True, 0xE)
    tg.data[3, :] = 1.0                                      # handed out: no hint from the next call on
    e.step_fused(tg)
    e.step_fused(tg)
    assert calls[-1][1:3] == (False, 0) and calls[-2][1:3] == (False, 0)


def test_controller_args_for_each_history():
    from dronesim_amd.control import INDIControl
    from dronesim_amd.fleet import FleetState
    c = INDIControl.__new__(INDIControl)
    ctx = _fake_ctx()
    c.ctx, c.n, c.env, c._type_id, c._plan, c.control_counter, c._outputs_placed = ctx, N, None, None, None, 0, True
    c.state = FleetState(ctx, N)
    c._targets = Targets(ctx, N)
    c._pos_e, c._yaw_e, c._cmd = torch.zeros(3, c.state.n_pad), torch.zeros(c.state.n_pad), torch.zeros(4, c.state.n_pad)
    calls = ctx.lib.calls
    tpos = frozen(torch.zeros(3, N))
    c.computeControl(1 / 48, None, None, None, None, target_pos=tpos, target_rpy=np.array([0, 0, 0.4]))
    assert calls[-1] == ("control", True, 0xE, [0] * 9 + _bits(0.4))
    c.computeControl(1 / 48, None, None, None, None, target_pos=tpos, target_rpy=np.array([0, 0, 0.4]))
    assert calls[-1] == calls[-2] and c._plan is not None
    c.computeControl(1 / 48, None, None, None, None, target_pos=tpos, target_vel=np.array([0.5, 0, 0]),
                     target_acc=np.array([0, 0, -0.125]), target_rpy=np.array([0, 0, -1.0]))
    assert calls[-1] == ("control", True, 0xE, [0, 0, 0] + _bits([0.5, 0, 0]) + _bits([0, 0, -0.125]) + _bits(-1.0))
    c.computeControl(1 / 48, None, None, None, None, target_pos=tpos, target_vel=torch.ones(3, N), target_rpy=np.array([0, 0, -1.0]))
    assert calls[-1][1:3] == (True, 0xC)
    c.computeControl(1 / 48, None, None, None, None, target_pos=np.zeros(3), target_rpy=np.array([0, 0, -1.0]))
    assert calls[-1][1:3] == (True, 0xF)                     # everything constant: the library reads the view (mask != 0xE)
    c._targets.fields(0, 3)                                  # handed out
    c.computeControl(1 / 48, None, None, None, None, target_pos=tpos, target_rpy=np.array([0, 0, -1.0]))
    assert calls[-1][1:3] == (False, 0)
