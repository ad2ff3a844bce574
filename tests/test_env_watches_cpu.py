"""What follows a launch of the env: the counters, then the drone watch, the obstacle watch and the camera, in that order (CPU only:
the env on host memory with a recording stand-in for the library, as tests/test_mem_hint_cpu.py).  The expected records are
written from the rule — one obstacle query behind every launch; a camera capture exactly when a multiple of IMG_CAPTURE_FREQ lies
in (step_counter before, step_counter after] — not from the code."""
import types

import numpy as np
import torch

from dronesim_amd import _native as nat
from dronesim_amd.fleet import FleetState, Targets

N = 300
FREQ = 10          # IMG_CAPTURE_FREQ, in physics steps
AGGR = 5           # physics steps per Env.step

# n_steps of each step_fused call, and what the rule gives behind it
CALLS = [1, 1, 1, 1, 3, 1, 2]
STEP_COUNTER = [5, 10, 15, 20, 35, 40, 50]
ENV_STEPS = [1, 2, 3, 4, 7, 8, 10]
CAPTURE = [False, True, False, True, True, True, True]


class _Lib:
    """Every library call is recorded by name and succeeds."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def call(*a):
            self._log.append(name)
            return 0
        return call


class _Camera:
    drones = False

    def __init__(self, log):
        self._log = log

    def capture(self):
        self._log.append("camera")
        return None, None


class _Clearance:
    def __init__(self, log):
        self._log, self.margins, self.returned = log, [], None

    def clearance(self, margin, pairs_out=None):
        assert pairs_out is None                       # the per-step watch counts in the library, not into an on-demand counter
        self._log.append("clearance")
        self.margins.append(margin)
        self.returned = (torch.zeros(N), torch.zeros(N, dtype=torch.int32))
        return self.returned


def _env(obstacles=False, camera=False, drone_watch=False):
    from dronesim_amd.envs import CtrlAviary
    log = []
    ctx = types.SimpleNamespace(device=torch.device("cpu"), order=None, n_fields=nat.NF_QUAD, n_act=4, placement=False,
                                lib=_Lib(log), handle=None, stream_ptr=lambda: None, read_room=None)
    e = CtrlAviary.__new__(CtrlAviary)
    e.ctx, e.NUM_DRONES, e.state = ctx, N, FleetState(ctx, N, "soa")
    e.AGGR_PHY_STEPS, e.TIMESTEP, e._phys_options, e._tuning, e.noise_seed, e._env_steps = AGGR, 1 / 240, 0, 0, 0, 0
    e._downwash = e._fb_event = e._fb_stream = e._runs = e.order = e._dyn_rates = e._type_id = None
    e._fused_plan = e._fused_plan_dw = e._step_plan = None
    e._chained_enabled, e._chain_live, e._graph_made = False, False, False
    e._chain_ok, e.n_act, e.step_counter, e._use_last_action = False, 4, 0, False
    e._action_buf = torch.zeros((4, e.state.n_pad))
    e.state.pre_access, e.state.on_hand_out = e._before_host_access, e._mem_hand_out
    if obstacles:
        e._obst, e._obst_margin, e._obst_off = types.SimpleNamespace(handle=None), 1.0, None
        e._obst_clr, e._obst_near = torch.zeros(e.state.n_pad), torch.zeros(e.state.n_pad, dtype=torch.int32)
        e._obst_sampled = False
    if camera:
        e._vision, e.IMG_CAPTURE_FREQ, e._vision_seen = _Camera(log), FREQ, 0
    if drone_watch:
        e._drone_watch, e._drone_watch_margin, e._clearance, e.last_clearance = True, 0.75, _Clearance(log), None
    tg = Targets(ctx, N, "soa")
    tg.set(pos=np.zeros((3, N), np.float32), yaw=0.4)
    return e, tg, log


def test_the_table_is_the_rule():
    """The expected records above, re-derived: Env.steps add up, the counter is AGGR times them, and a capture is due exactly
    when some multiple of FREQ lies in (counter before, counter after]."""
    assert ENV_STEPS == list(np.cumsum(CALLS)) and STEP_COUNTER == [AGGR * k for k in ENV_STEPS]
    before = [0] + STEP_COUNTER[:-1]
    assert CAPTURE == [any(c % FREQ == 0 for c in range(b + 1, a + 1)) for b, a in zip(before, STEP_COUNTER)]


def test_obstacle_query_behind_every_launch_and_camera_at_its_cadence():
    e, tg, log = _env(obstacles=True, camera=True)
    assert e.last_obstacle_clearance is None
    plans = []
    for n, counter, steps, capture in zip(CALLS, STEP_COUNTER, ENV_STEPS, CAPTURE):
        del log[:]
        e.step_fused(tg, n_steps=n)
        assert log == ["dsim_step", "dsim_obstacle_clearance"] + ["camera"] * capture, (steps, log)
        assert (e.step_counter, e._env_steps) == (counter, steps)
        assert e.last_obstacle_clearance is not None
        plans.append(e._fused_plan)
    # the fresh path made the plan of call 1; calls 2 to 4 replayed it; another n_steps makes another
    assert plans[0] is not None and plans[0] is plans[1] is plans[2] is plans[3]
    assert plans[4] is not plans[3] and plans[5] is not plans[4]


def test_drone_watch_first_and_last_clearance_is_its_answer():
    e, tg, log = _env(obstacles=True, camera=True, drone_watch=True)
    for n, capture in zip(CALLS, CAPTURE):
        del log[:]
        e.step_fused(tg, n_steps=n)
        assert log == ["dsim_step", "clearance", "dsim_obstacle_clearance"] + ["camera"] * capture
        assert e.last_clearance[0] is e._clearance.returned[0] and e.last_clearance[1] is e._clearance.returned[1]
    assert e._clearance.margins == [0.75] * len(CALLS)
    # the drone watch alone
    e, tg, log = _env(drone_watch=True)
    e.step_fused(tg)
    e.step_fused(tg)
    assert log == ["dsim_step", "clearance"] * 2


def test_nothing_on_nothing_launched():
    e, tg, log = _env()
    plan = None
    for k, n in enumerate(CALLS):
        e.step_fused(tg, n_steps=n)
        if k == 0:
            plan = e._fused_plan
        if k in (1, 2, 3):
            assert e._fused_plan is plan
    assert log == ["dsim_step"] * len(CALLS)
    assert (e.step_counter, e._env_steps) == (STEP_COUNTER[-1], ENV_STEPS[-1])
    assert e.last_obstacle_clearance is None
