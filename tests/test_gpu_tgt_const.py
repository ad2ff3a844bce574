"""DSIM_OPT_TGT_CONST: a fleet whose Targets hand vel / acc / yaw to the kernels as constants steps exactly — torch.equal on the
state block — as an identical fleet whose kernels read those fields (its Targets were handed out, so it never offers the hint).
An A/B test: it covers the host logic (when the env offers the hint, re-keys a prepared launch, withdraws it for good) and
bit-identity with the sibling IN GENTLE FLIGHT on the instances that honour the hint — k_step_fast with noise on / off, streaming
on / off, chained on / off, one and five sub-steps, k_control_fast with and without the yaw error, streaming on / off.  Parity of
those instances with the ORACLE, constants that exercise the law, and the envelope: tests/test_gpu_hinted_vs_oracle.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 2048


def _fleet(sub, noise, nt, chained, n=N):
    from dronesim_amd import _native as nat
    from dronesim_amd.envs import CtrlAviary
    from dronesim_amd.fleet import Targets
    rng = np.random.default_rng(20)
    xyz = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(1, 5, n)], 1)
    rpy = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-3, 3, n)], 1)
    envs, tgts = [], []
    for hinted in (True, False):
        e = CtrlAviary(["robobee"], n, initial_xyzs=xyz, initial_rpys=rpy, aggregate_phy_steps=sub, noise_seed=noise,
                       dict_io=False, chained=chained, options=nat.OPT_STREAM_ON if nt else nat.OPT_STREAM_OFF)
        tg = Targets(e.ctx, n)
        tg.set(pos=(xyz + 0.3).astype(np.float32).T, yaw=0.4)
        if not hinted:
            assert tg.data is not None        # handed out: this object offers no hint from now on
        envs.append(e)
        tgts.append(tg)
    return envs, tgts, xyz


def _steps(envs, tgts, k, action=None):
    for e, tg in zip(envs, tgts):
        if action is not None:
            e.step_fused(tg, action=action)
        for _ in range(k):
            e.step_fused(tg)


def _same(envs):
    a, b = (e.state.fields(0, 24) for e in envs)         # (materialises a chained fleet)
    assert torch.equal(a, b)


def _hint(env):
    from dronesim_amd import _native as nat
    p = env._fused_plan
    assert p is not None
    return (p.args.options & nat.OPT_TGT_CONST) != 0, p.args.tgt_const_mask, list(p.args.tgt_const)


@pytest.mark.parametrize("sub", [1, 5])
@pytest.mark.parametrize("noise", [0, 11])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("chained", [False, True])
def test_hinted_fused_step_matches_the_plain_one(sub, noise, nt, chained):
    envs, tgts, xyz = _fleet(sub, noise, nt, chained)
    _steps(envs, tgts, 12, action=np.full((N, 4), 0.4, dtype=np.float32))
    on, mask, c = _hint(envs[0])
    assert on and mask == 0xE and c[9] == np.float32(0.4)
    assert not _hint(envs[1])[0]
    _same(envs)
    # a constant changed between two calls of the cached plan: the plan re-keys on the hint epoch and carries the new value
    for tg in tgts:
        tg.set(yaw=-0.25, vel=[0.5, -0.125, 0.0], acc=[0.1, -0.2, 0.3])
    _steps(envs, tgts, 8)
    on, mask, c = _hint(envs[0])
    assert on and mask == 0xE and c[9] == np.float32(-0.25) and c[3:6] == [0.5, -0.125, 0.0]
    assert c[6:9] == [float(np.float32(x)) for x in (0.1, -0.2, 0.3)]
    _same(envs)
    # a group per drone (no hint: the mask is not pos-only), then constant again
    vel = torch.linspace(-0.5, 0.5, N, device=envs[0].ctx.device).repeat(3, 1)
    for tg in tgts:
        tg.set(vel=vel)
    _steps(envs, tgts, 6)
    assert _hint(envs[0])[1] == 0xC
    _same(envs)
    for tg in tgts:
        tg.set(vel=[0.0, 0.25, 0.0])
    _steps(envs, tgts, 6)
    assert _hint(envs[0])[:2] == (True, 0xE)
    _same(envs)
    # a raw write through the handed-out tensor: the hinted object stops offering the hint for good
    for tg in tgts:
        tg.data[6, :N] = 0.75
    _steps(envs, tgts, 6)
    assert not _hint(envs[0])[0]
    _same(envs)


@pytest.mark.parametrize("sub", [1, 5])
def test_ragged_fleet_with_nonzero_constants(sub):
    """n < n_pad: the padding lanes get the constants instead of the zeros the array holds there (they are no drones, and
    nothing reads them back); the drones themselves step exactly as without the hint."""
    n = N - 48
    envs, tgts, _ = _fleet(sub, 7, True, False, n=n)
    for tg in tgts:
        tg.set(vel=[0.25, 0.0, -0.5], acc=[0.1, -0.2, 0.3], yaw=1.25)
    _steps(envs, tgts, 10, action=np.full((n, 4), 0.4, dtype=np.float32))
    on, mask, c = _hint(envs[0])
    assert on and mask == 0xE and c[6:9] == [float(np.float32(x)) for x in (0.1, -0.2, 0.3)]
    assert envs[0].state.n_pad > n
    _same(envs)


def test_graph_captured_before_a_set_sees_the_new_constant():
    envs, tgts, _ = _fleet(1, 3, True, False)
    _steps(envs, tgts, 4, action=np.full((N, 4), 0.4, dtype=np.float32))
    graphs = [e.capture_fused(tg, 4) for e, tg in zip(envs, tgts)]
    for g in graphs:
        g.replay()
    _same(envs)
    for tg in tgts:
        tg.set(yaw=1.0, acc=[0.0, 0.0, 0.5])
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    _same(envs)
    a = envs[0].state.fields(0, 24).clone()
    # ... and the replayed steps used the new targets: the same as eager steps from the same start
    _steps(envs, tgts, 2)
    _same(envs)
    assert not torch.equal(a, envs[0].state.fields(0, 24))


@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("want_yaw", [False, True])
def test_hinted_control_matches_the_plain_one(nt, want_yaw):
    from dronesim_amd import _native as nat
    envs, tgts, _ = _fleet(1, 0, nt, False)
    _steps(envs, tgts, 3, action=np.full((N, 4), 0.4, dtype=np.float32))
    outs = []
    for e, tg in zip(envs, tgts):
        tg.set(vel=[0.5, -0.125, 0.25], acc=[0.1, -0.2, 0.3], yaw=-0.75)
        a = e.step_args(1.0 / 48)
        tg.fill_const_hint(a)
        pos_e = torch.zeros((3, e.state.n_pad), device=e.ctx.device)
        yaw_e = torch.zeros((e.state.n_pad,), device=e.ctx.device)
        cmd = torch.zeros((4, e.state.n_pad), device=e.ctx.device)
        for _ in range(5):
            nat.check(e.ctx.lib.dsim_control2(e.ctx.handle, e.ctx.stream_ptr(), N, e.state.view(), tg.view(), ctypes.byref(a),
                                              pos_e.data_ptr(), yaw_e.data_ptr() if want_yaw else None, cmd.data_ptr()))
        outs.append((a.options & nat.OPT_TGT_CONST, pos_e, yaw_e, cmd))
    assert outs[0][0] and not outs[1][0]
    for x, y in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(x, y)
    _same(envs)


def test_controller_two_call_loop_matches():
    """INDIControl.computeControlFromState on a bound env (the reference-shaped two-call loop) with the hint and without."""
    from dronesim_amd import _native as nat
    from dronesim_amd.control import INDIControl
    from dronesim_amd.fleet import frozen
    envs, _, xyz = _fleet(1, 5, True, False)
    tpos = frozen(torch.as_tensor((xyz + 0.3).astype(np.float32).T.copy(), device=envs[0].ctx.device))
    ctrls = [INDIControl("robobee", env=e) for e in envs]
    assert ctrls[1]._targets.data is not None        # handed out: no hint
    cmds = [torch.full((N, 4), 0.4, device=e.ctx.device) for e in envs]
    for it in range(10):
        yaw = np.array([0, 0, 0.4 if it < 5 else -0.3])
        for k, (e, c) in enumerate(zip(envs, ctrls)):
            e.step(cmds[k])
            cmds[k], pe, ye = c.computeControlFromState(e.TIMESTEP * e.AGGR_PHY_STEPS, None, target_pos=tpos, target_rpy=yaw)
        assert torch.equal(cmds[0], cmds[1])
    assert ctrls[0]._targets.const_hint()[0] == 0xE and ctrls[1]._targets.const_hint() is None
    _same(envs)
