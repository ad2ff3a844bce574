"""DSIM_OPT_MEM_DERIVED: a fused step that recomputes last_vel / last_rates from the rigid state it has just loaded, instead of
reading them, leaves the state block bit for bit as the launch that reads them.  Two envs that differ only in ``mem_hint``;
np.array_equal, no tolerance: the recomputed body rates go through the one pinned helper that also produced the stored ones
(dsim_device.h: body_rates).  An A/B test: it covers the host logic (every way the env must withhold the hint for one launch) and
bit-identity with the sibling IN GENTLE FLIGHT, 50 steps from rest, on the instances that honour the bit — k_step_fast with
TGT_CONST: noise on / off x streaming on / off; k_step_hexa: noise x streaming — and on the quad launches without TGT_CONST, which
carry the bit and whose kernels ignore it.  WHICH kernel a launch ran is not visible from here: tools/kernel_coverage.sh lists
the instances this suite launches (profiles/r09_kernels_launched_by_tests.txt).  Parity of those instances with the ORACLE,
bit-identity over the envelope (rates at the +-100 rad/s clamp, tumbling, non-unit quaternions, tiny rates) and a witness launch
that proves the dispatch: tests/test_gpu_hinted_vs_oracle.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 2048
STEPS = 50


def _pair(model, noise, nt, tc=True, layout=None, n=N):
    """(hinted env, its twin with mem_hint=False), each with its Targets, both one explicit-action step in."""
    from dronesim_amd import _native as nat
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    rng = np.random.default_rng(9)
    xyz = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(1, 5, n)], 1)
    rpy = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-3, 3, n)], 1)
    envs, tgts = [], []
    for hint in (True, False):
        e = CtrlAviary([model], n, initial_xyzs=xyz, initial_rpys=rpy, aggregate_phy_steps=1, noise_seed=noise, dict_io=False,
                       layout=layout, options=nat.OPT_STREAM_ON if nt else nat.OPT_STREAM_OFF, mem_hint=hint)
        tg = Targets(e.ctx, n, e.state.layout)
        tg.set(pos=(xyz + 0.3).astype(np.float32).T, yaw=0.4)
        if not tc:
            assert tg.data is not None        # handed out: the object offers no DSIM_OPT_TGT_CONST, the kernels read all ten
        e.step_fused(tg, action=np.full((n, e.n_act), 0.4, dtype=np.float32))
        envs.append(e)
        tgts.append(tg)
    return envs, tgts


def _carried(env):
    """Whether the prepared launch the env would replay next carries the bit (what the last replay was launched with)."""
    from dronesim_amd import _native as nat
    assert env._fused_plan is not None
    return bool(env._fused_plan.args.options & nat.OPT_MEM_DERIVED)


def _blocks_equal(envs):
    a, b = envs
    nf = a.state.n_fields
    fa, fb = a.state.fields(0, nf).cpu().numpy(), b.state.fields(0, nf).cpu().numpy()
    assert np.array_equal(fa, fb), np.abs(fa - fb).max(axis=1)
    assert np.array_equal(a.state.data.cpu().numpy(), b.state.data.cpu().numpy())
    # ... and the memory is what the hint asserts: last_vel == vel, bit for bit
    assert np.array_equal(fa[13:16], fa[7:10])


@pytest.mark.parametrize("tc", [True, False])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("noise", [0, 11])
def test_quad_hint_on_equals_hint_off(noise, nt, tc):
    envs, tgts = _pair("robobee", noise, nt, tc)
    for e, tg in zip(envs, tgts):
        for _ in range(STEPS):
            e.step_fused(tg)
    assert _carried(envs[0]) and not _carried(envs[1])
    from dronesim_amd import _native as nat
    assert bool(envs[0]._fused_plan.args.options & nat.OPT_TGT_CONST) == tc
    _blocks_equal(envs)


@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("noise", [0, 11])
def test_hexa_hint_on_equals_hint_off(noise, nt):
    envs, tgts = _pair("hexa_6DOF", noise, nt)
    assert envs[0].state.n_fields == 26
    for e, tg in zip(envs, tgts):
        for _ in range(STEPS):
            e.step_fused(tg)
    assert _carried(envs[0]) and not _carried(envs[1])
    _blocks_equal(envs)


def test_tiled_layout():
    """The headline's layout and instance (tile64, noise, streaming, TGT_CONST) on a small fleet."""
    envs, tgts = _pair("robobee", 1, True, layout="tile64", n=8192)
    for e, tg in zip(envs, tgts):
        for _ in range(STEPS):
            e.step_fused(tg)
    assert _carried(envs[0])
    _blocks_equal(envs)


@pytest.mark.parametrize("how", ["set_fields", "view_write", "env_step", "reset", "controller"])
def test_host_access_withholds_the_hint_for_one_launch(how):
    """Between two fused steps the caller changes the rigid state (or, "controller", only might have): the launch behind it
    must read the stored memory.  In the first four cases the stored last_vel no longer equals vel, so a launch that wrongly
    took the hint differs from the twin in cmd at once."""
    envs, tgts = _pair("robobee", 5, False, layout="soa")
    ctrls = []
    for e, tg in zip(envs, tgts):
        for _ in range(5):
            e.step_fused(tg)
    assert _carried(envs[0])
    for e, tg in zip(envs, tgts):
        if how == "set_fields":
            e.state.set_fields(7, torch.full((3, N), 0.75))
        elif how == "view_write":
            e.state.vel[:] = 0.75                       # the soa layout hands out a writable view
        elif how == "env_step":
            e.step(np.full((N, 4), 0.45, dtype=np.float32))
        elif how == "reset":
            e.reset()
        else:
            from dronesim_amd.control import INDIControl
            c = INDIControl("robobee", env=e)
            ctrls.append(c)
            c.computeControlFromState(e.TIMESTEP, None, target_pos=np.zeros(3), target_rpy=np.array([0, 0, 0.4]))
        e.step_fused(tg)                                # the cautious launch
    _blocks_equal(envs)
    for e, tg in zip(envs, tgts):
        for _ in range(5):
            e.step_fused(tg)
    assert _carried(envs[0]) and not _carried(envs[1])      # hinted again
    _blocks_equal(envs)


def test_env_var_opt_out(monkeypatch):
    from dronesim_amd.envs import CtrlAviary
    monkeypatch.setenv("DSIM_NO_MEM_HINT", "1")
    e = CtrlAviary(["robobee"], 256, initial_xyzs=np.zeros((256, 3)) + [0, 0, 1.0], noise_seed=0, dict_io=False)
    assert not e._mem_hint
