"""dsim_step_args.tgt_period: a fleet of replicas that share one task (the targets repeat with a period) steps exactly — torch.equal
on the state block — as an identical fleet whose kernels read every target (its Targets were handed out, so it offers no hint).
An A/B test: it covers the host logic (which period a Targets finds and hands to a prepared launch, when it gives it up) and
bit-identity with the sibling IN GENTLE FLIGHT on the k_step_fast instances that honour the period: noise on / off, streaming
on / off, chained on / off, one and five sub-steps, with DSIM_OPT_TGT_CONST (vel / acc / yaw constant) and without it (vel per
drone, periodic).  A launch through the C ABI with NaN in every target beyond the first period proves that those instances read
the first period only.  Parity of those instances with the ORACLE and the envelope: tests/test_gpu_hinted_vs_oracle.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, REPS = 512, 8             # a task of 512 drones, 8 replicas
N = P * REPS


def _task(n_task=P, seed=30):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-20, 20, n_task), rng.uniform(-20, 20, n_task), rng.uniform(1, 5, n_task)]).astype(np.float32)
    vel = np.stack([rng.uniform(-0.5, 0.5, n_task), rng.uniform(-0.5, 0.5, n_task), np.zeros(n_task)]).astype(np.float32)
    return pos, vel


def _fleet(sub, noise, nt, chained, tc, n=N, layout="soa", p=P):
    """Two identical envs and Targets: [0] offers the period (and, with tc, the constant hint), [1] was handed out."""
    from dronesim_amd import _native as nat
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    rng = np.random.default_rng(21)
    xyz = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(1, 5, n)], 1)   # the states do not repeat
    rpy = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-3, 3, n)], 1)
    pos, vel = _task(p)
    reps = -(-n // p)
    envs, tgts = [], []
    for hinted in (True, False):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, initial_rpys=rpy, aggregate_phy_steps=sub, noise_seed=noise,
                       dict_io=False, chained=chained, layout=layout,
                       options=nat.OPT_STREAM_ON if nt else nat.OPT_STREAM_OFF)
        tg = Targets(e.ctx, n, layout)
        tg.set(pos=np.tile(pos, reps)[:, :n], yaw=0.4)
        if not tc:
            tg.set(vel=np.tile(vel, reps)[:, :n])          # per drone: the kernels read every target field (of one period)
        if not hinted:
            assert tg.data is not None        # handed out: this object offers no hint from now on
        envs.append(e)
        tgts.append(tg)
    return envs, tgts


def _steps(envs, tgts, k, action=None):
    for e, tg in zip(envs, tgts):
        if action is not None:
            e.step_fused(tg, action=action)
        for _ in range(k):
            e.step_fused(tg)


def _same(envs):
    a, b = (e.state.fields(0, 24) for e in envs)         # (materialises a chained fleet)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def _plan(env):
    from dronesim_amd import _native as nat
    p = env._fused_plan
    assert p is not None
    return p.args.tgt_period, p.args.tgt_const_mask if (p.args.options & nat.OPT_TGT_CONST) else None


@pytest.mark.parametrize("sub", [1, 5])
@pytest.mark.parametrize("noise", [0, 11])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("tc", [False, True])
def test_periodic_fused_step_matches_the_plain_one(sub, noise, nt, chained, tc):
    envs, tgts = _fleet(sub, noise, nt, chained, tc)
    _steps(envs, tgts, 10, action=np.full((N, 4), 0.4, dtype=np.float32))
    assert _plan(envs[0]) == (P, 0xE if tc else 0xC)
    assert _plan(envs[1]) == (0, None)
    _same(envs)
    _steps(envs, tgts, 1)                                # (a chained fleet was materialised: its block is prepared again)
    plan = envs[0]._fused_plan
    # new per-drone positions of another task: the prepared block is replayed with the period it finds now
    pos, _ = _task(P // 2, seed=31)
    for tg in tgts:
        tg.set(pos=np.tile(pos, 2 * REPS))
    _steps(envs, tgts, 6)
    assert envs[0]._fused_plan is plan and _plan(envs[0])[0] == (256 if tc else P)     # (without tc: vel repeats with P)
    _same(envs)
    _steps(envs, tgts, 1)
    plan = envs[0]._fused_plan
    # positions that do not repeat: the same block, no period
    pos = np.random.default_rng(5).uniform(-10, 10, (3, N)).astype(np.float32)
    for tg in tgts:
        tg.set(pos=pos)
    _steps(envs, tgts, 6)
    assert envs[0]._fused_plan is plan and _plan(envs[0])[0] == 0
    _same(envs)


@pytest.mark.parametrize("layout", ["tile64", "tile1024"])
def test_tiled_layouts(layout):
    """The headline's layout (blocks of 64) and blocks larger than the task (the period is taken up to a whole block)."""
    envs, tgts = _fleet(1, 11, True, False, True, layout=layout)
    _steps(envs, tgts, 8, action=np.full((N, 4), 0.4, dtype=np.float32))
    assert _plan(envs[0]) == (1024 if layout == "tile1024" else P, 0xE)
    _same(envs)


def _nan_beyond_the_first_period(tg, p):
    nan = float("nan")
    if tg.layout == "soa":
        tg._data[:, p:] = nan
    else:                                  # [n_pad / B, F, B]
        tg._data[p // tg.block:] = nan


def _abi_steps(e, tg, k, period, tc):
    from dronesim_amd import _native as nat
    e.materialize()
    for s in range(k):
        a = e.step_args()
        a.step_index = s
        if tc:
            tg.fill_const_hint(a)
        a.tgt_period = period
        nat.check(e.ctx.lib.dsim_step(e.ctx.handle, e.ctx.stream_ptr(), e.NUM_DRONES, e.state.view(), tg.view(),
                                      ctypes.byref(a)))


@pytest.mark.parametrize("sub", [1, 5])
@pytest.mark.parametrize("noise", [0, 11])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("tc", [False, True])
@pytest.mark.parametrize("layout", ["soa", "tile64"])
def test_abi_reads_the_first_period_only(sub, noise, nt, tc, layout):
    """tgt_period set by hand, every target beyond the first period NaN: the same state as the fully written fleet."""
    envs, tgts = _fleet(sub, noise, nt, False, tc, layout=layout)
    _nan_beyond_the_first_period(tgts[0], P)
    assert torch.isnan(tgts[0]._data).any()
    _abi_steps(envs[0], tgts[0], 8, P, tc)
    _abi_steps(envs[1], tgts[1], 8, 0, tc)
    _same(envs)


@pytest.mark.parametrize("nt", [False, True])
def test_abi_period_of_three_tiles(nt):
    """A period that is no power of two of tiles (768 drones: the modulo form), NaN beyond it."""
    p = 768
    envs, tgts = _fleet(1, 11, nt, False, True, n=4 * p, p=p)
    assert tgts[0].tgt_period() == p
    _nan_beyond_the_first_period(tgts[0], p)
    _abi_steps(envs[0], tgts[0], 6, p, True)
    _abi_steps(envs[1], tgts[1], 6, 0, True)
    _same(envs)


def test_abi_ignores_a_period_it_cannot_honour():
    """Periods that are no multiple of 256, do not divide n_pad or are not below it: ignored, no error."""
    from dronesim_amd import _native as nat
    envs, tgts = _fleet(1, 11, True, False, True)
    for period in (128, 768, N, 2 * N, -P):
        _abi_steps(envs[0], tgts[0], 2, period, True)
        _abi_steps(envs[1], tgts[1], 2, 0, True)
        _same(envs)
    # a ragged fleet: n < n_pad, the targets object knows no period, and the fused steps match
    n = N - 48
    envs, tgts = _fleet(1, 11, True, False, True, n=n)
    assert tgts[0].tgt_period() == 0 and envs[0].state.n_pad > n
    _steps(envs, tgts, 6, action=np.full((n, 4), 0.4, dtype=np.float32))
    assert _plan(envs[0])[0] == 0
    _same(envs)
    assert nat.StepArgs().tgt_period == 0


def test_graph_capture_runs_without_the_period():
    envs, tgts = _fleet(1, 3, True, False, True)
    _steps(envs, tgts, 4, action=np.full((N, 4), 0.4, dtype=np.float32))
    graphs = [e.capture_fused(tg, 4) for e, tg in zip(envs, tgts)]
    assert graphs[0]._args.tgt_period == 0
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    _same(envs)
