"""Which fused launches of an env carry DSIM_OPT_MEM_DERIVED (CPU only: the env on host memory with a recording stand-in for the
library, as tests/test_targets_hint_cpu.py).  The bit says "last_vel / last_rates in the block are what the previous fused step
left": given behind a fused step, withheld for the one launch behind anything that handed the block out."""
import types

import numpy as np
import pytest
import torch

from dronesim_amd import _native as nat
from dronesim_amd.fleet import FleetState, Targets

N = 300


class _Lib:
    def __init__(self):
        self.bits = []

    def dsim_step(self, h, s, n, sview, tview, ref):
        self.bits.append(bool(ref._obj.options & nat.OPT_MEM_DERIVED))
        return 0

    def dsim_materialize(self, *a):
        return 0


def _env(mem_hint=True, chained=False, layout="soa"):
    from dronesim_amd.envs import CtrlAviary
    ctx = types.SimpleNamespace(device=torch.device("cpu"), order=None, n_fields=nat.NF_QUAD, n_act=4, placement=False,
                                lib=_Lib(), handle=None, stream_ptr=lambda: None, read_room=None)
    e = CtrlAviary.__new__(CtrlAviary)
    e.ctx, e.NUM_DRONES, e.state = ctx, N, FleetState(ctx, N, layout)
    e.AGGR_PHY_STEPS, e.TIMESTEP, e._phys_options, e._tuning, e.noise_seed, e._env_steps = 1, 1 / 240, 0, 0, 0, 0
    e._downwash = e._fb_event = e._fb_stream = e._runs = e.order = e._dyn_rates = e._type_id = None
    e._fused_plan = e._fused_plan_dw = e._step_plan = None
    e._chained_enabled, e._chain_live, e._graph_made = chained, False, False
    e._chain_ok, e.n_act, e.step_counter, e._use_last_action = False, 4, 0, False
    e._mem_hint, e._mem_handed_out = mem_hint, True                    # what __init__ sets
    e._action_buf = torch.zeros((4, e.state.n_pad))
    e.state.pre_access, e.state.on_hand_out = e._before_host_access, e._mem_hand_out
    tg = Targets(ctx, N, layout)
    tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
    return e, tg, ctx.lib.bits


def test_three_consecutive_steps():
    e, tg, bits = _env()
    e.step_fused(tg, action=np.full((N, 4), 0.4, np.float32))     # the first iteration of the example loop
    e.step_fused(tg)
    e.step_fused(tg)
    e.step_fused(tg)
    assert bits == [False, True, True, True]
    assert e._fused_plan is not None


def test_defaults_of_an_env_made_without_init():
    """The class itself says "no hint": an object that never ran __init__ (the stubs of the other CPU tests) launches as before."""
    from dronesim_amd.envs import CtrlAviary
    assert CtrlAviary._mem_hint is False and CtrlAviary._mem_handed_out is True


ACCESSES = {
    "raw_fields": lambda e: e.state.raw_fields(0, 3),
    "fields": lambda e: e.state.fields(7, 3),
    "property": lambda e: e.state.vel,
    "set_fields": lambda e: e.state.set_fields(7, torch.ones(3, N)),
    "load_aos": lambda e: e.state.load_aos(np.zeros((N, 13)), np.zeros((N, 11))),
    "rigid_aos": lambda e: e.state.rigid_aos(),
    "data": lambda e: e.state.data,
    "move_state": lambda e: e._move_state(torch.zeros_like(e.state._data)),
}


@pytest.mark.parametrize("how", sorted(ACCESSES))
@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_step_access_step_step(how, layout):
    e, tg, bits = _env(layout=layout)
    e.step_fused(tg)
    e.step_fused(tg)
    assert bits == [False, True]
    ACCESSES[how](e)
    e.step_fused(tg)          # right behind the access: reads the whole memory (a dropped plan or a cleared bit)
    e.step_fused(tg)
    e.step_fused(tg)
    assert bits == [False, True, False, True, True], how


def test_internal_reads_do_not_count():
    e, tg, bits = _env()
    for _ in range(4):
        e.step_fused(tg)
        e.state.view()                                 # what the hot paths themselves read
    assert bits == [False, True, True, True]


def test_other_operations_end_it():
    e, tg, bits = _env()
    e.step_fused(tg)
    e.step_fused(tg)
    e._chain_ok = False                     # what step(), the adaptor envs and a bound controller's computeControl leave
    e.step_fused(tg)
    e.step_fused(tg)
    assert bits == [False, True, False, True]
    e.step_fused(tg, action=np.full((N, 4), 0.4, np.float32))     # an explicit action: the ACT instances read the fields
    e.step_fused(tg)
    assert bits[-2:] == [False, True]


def test_opt_outs(monkeypatch):
    e, tg, bits = _env(mem_hint=False)
    for _ in range(3):
        e.step_fused(tg)
    assert bits == [False] * 3
    e, tg, bits = _env(chained=True)        # chained: its own bit says more, this one is not set beside it
    for _ in range(3):
        e.step_fused(tg)
    assert bits == [False] * 3
    # the constructor's two switches
    import inspect
    from dronesim_amd.envs import CtrlAviary
    assert inspect.signature(CtrlAviary.__init__).parameters["mem_hint"].default is True
    monkeypatch.delenv("DSIM_NO_MEM_HINT", raising=False)
    assert CtrlAviary._mem_hint_wanted(True) is True and CtrlAviary._mem_hint_wanted(False) is False
    monkeypatch.setenv("DSIM_NO_MEM_HINT", "1")
    assert CtrlAviary._mem_hint_wanted(True) is False
    monkeypatch.setenv("DSIM_NO_MEM_HINT", "0")
    assert CtrlAviary._mem_hint_wanted(True) is True
