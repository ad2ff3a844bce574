"""Physics.PYB_GND, PYB_DRAG and PYB_GND_DRAG_DW flown through CtrlAviary: the env's bookkeeping around the drag rule (the
previous Env.step's clipped action on sub-step 0: `_last_action`, zeroed by reset(), kept in storage order on a type-major
fleet, handed to the prepared launch of a repeated step(), carried from launch to launch where an Env.step is split into
one [neighbour query -> one-sub-step physics] pair per sub-step) and the routes of step_fused / capture_fused on these modes.

The model is tests/test_gpu_fuzz.py's Loop, told the physics mode: it holds the env's `last` (zeroed on reset, updated by
every step(action), untouched by fused steps), is re-seated on the device's state in front of every operation and applies
the operation with the fp64 oracle — O.physics(..., options=, last_action=), O.physics_downwash for the mode with the
neighbour term, O.control behind fused steps (which hand the drag the current command: last_action=None).  Fleets of 64-128
drones 0.05-0.5 m above the ground, in couples one above the other, with initial velocities of a few m/s, no rotor noise
but for one test.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_fuzz import Loop  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("PYB_GND", "PYB_DRAG", "PYB_GND_DRAG_DW")
OPT_MEM_DERIVED = 1 << 21


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")


def _mode(name):
    from dronesim_amd.envs import Physics
    return Physics[name]


def _loop(label, mode, models, sub, n=96, tids=None, noise_seed=0, seed=0):
    """Couples: the even drones 0.05-0.1 m up on 10 m x 10 m (at most 64 of them), each odd drone 0.11-0.15 m beside and 0.3-0.4 m above its
    even neighbour and flying with it — under the neighbour term the lower one feels a push of up to 2 % (robobee) or 20 % (tello) of its weight
    step after step (asserted with the oracle: the term is live and nowhere violent; without the term the couples are just a fleet)."""
    from dronesim_amd import params
    from oracle import oracle as orc
    rng = np.random.default_rng(8100 + seed + 13 * sub + sum(map(ord, mode)))
    h = n // 2
    cell = rng.permutation(64)[:h]                     # one couple per cell of an 8 x 8 grid: couples do not meet
    low = np.stack([1.25 * (cell % 8) + rng.uniform(0.3, 0.95, h), 1.25 * (cell // 8) + rng.uniform(0.3, 0.95, h), rng.uniform(0.05, 0.1, h)], 1)
    ang, d = rng.uniform(-np.pi, np.pi, h), rng.uniform(0.11, 0.15, h)
    up = low + np.stack([d * np.cos(ang), d * np.sin(ang), rng.uniform(0.3, 0.4, h)], 1)
    xyz, vels = np.zeros((n, 3)), np.zeros((n, 3))
    xyz[0::2], xyz[1::2] = low, up
    vels[0::2] = vels[1::2] = rng.uniform(-3, 3, (h, 3))
    t = params.builtin_type(models[0])
    r = np.zeros((n, 13)); r[:, 0:3], r[:, 6] = xyz, 1.0
    fz = np.abs(orc.Oracle([t]).downwash(r, xyz))
    assert fz.max() < 0.5 * t.mass * t.gravity and (fz[0::2] > 0.002 * t.mass * t.gravity).sum() >= h // 2, (fz.max(), np.median(fz[0::2]))
    return Loop(label, seed, physics=_mode(mode), fleet=(models, tids, sub, False, False), n=n, xyz=xyz, vels=vels, noise_seed=noise_seed)


def _how(sub):
    # (five sub-steps per action: a fresh action per rotor from 0.3-0.6 would tumble the fleet within a few steps; see Loop.check_step)
    return "random" if sub == 1 else "tight"


@pytest.mark.parametrize("sub", [1, 5])
@pytest.mark.parametrize("model", ["robobee", "tello"])
@pytest.mark.parametrize("mode", MODES)
def test_env_step_in_every_mode(mode, model, sub):
    """Six step(action) calls with a fresh random action each, reset(), two more: state parity and the observation rows (last
    action columns == the model's `last`) after every one.  The first step after construction and the first after reset() run
    against the oracle fed last = 0 (the model's `last` is zero there: asserted).  PYB_GND_DRAG_DW at five sub-steps is the
    per-sub-step launch chain: against O.physics_downwash with ONE last_action, which the oracle replaces after sub-step 0."""
    L = _loop(f"step[{mode} {model} sub={sub}]", mode, [model], sub)
    assert L.env._dw_substepped() == (mode == "PYB_GND_DRAG_DW" and sub > 1)
    assert not L.last.any() and not bool(L.env._last_action.any())
    for _ in range(6):
        L.op_step(_how(sub))
        assert L.last[:, :4].min() > 0.29                       # (from the second step on the drag's first sub-step sees it)
    L.op_observe()
    L.op_reset()
    assert not L.last.any() and not bool(L.env._last_action.any())
    for _ in range(2):
        L.op_step(_how(sub))
    L.run([])


@pytest.mark.parametrize("given", ["view_of_soa", "rows"])
@pytest.mark.parametrize("mode", MODES)
def test_the_same_action_tensor_again(mode, given):
    """step(t) three times with the SAME device tensor object, its contents overwritten in place between the calls.  "view_of_soa":
    t is the transposed view of an [n_act, n_pad] array — the launch reads it where it lies and, without the neighbour term, the
    env keeps the prepared launch (_StepPlan, relaunched with the echo buffer's address); "rows": a plain [n, 4] tensor goes
    through the env's own action buffer and no plan is kept.  Parity on every call either way."""
    L = _loop(f"same tensor[{mode} {given}]", mode, ["robobee"], 2, n=128)
    env = L.env
    if given == "view_of_soa":
        t = torch.zeros((4, env.state.n_pad), device=env.ctx.device)[:, :L.n].T
    else:
        t = torch.zeros((L.n, 4), device=env.ctx.device)
    for k in range(3):
        L.op_step("random", tensor=t)
        planned = given == "view_of_soa" and mode != "PYB_GND_DRAG_DW"
        assert (env._step_plan is not None) == planned, (mode, given, k)
        if planned:
            assert env._step_plan.echo_ptr == env._last_action.data_ptr() and env._step_plan.action is t
    L.run([])


@pytest.mark.parametrize("mode", ["PYB_DRAG", "PYB_GND_DRAG_DW"])
def test_type_major_fleet_in_the_callers_numbering(mode):
    """["robobee", "tello"] * (n / 2): stored type-major behind the caller's numbering, and with these modes the HOST translates
    actions and rows (_caller_io is off) while `_last_action` stays in storage order.  Actions go in, and state, rows and the
    last-action columns come out, in the caller's numbering."""
    L = _loop(f"type-major[{mode}]", mode, ["robobee", "tello"], 2, n=96, tids="per_drone")
    env = L.env
    assert env.order is not None and not env._caller_io and env._phys_options != 0
    for _ in range(4):
        L.op_step("random")
    # the env's own buffer holds the model's `last` in STORAGE order
    np.testing.assert_array_equal(env.order.to_caller(env._last_action[:, :L.n], 1).cpu().numpy().T, L.last[:, :4].astype(np.float32))
    L.op_observe()
    L.op_reset()
    for _ in range(2):
        L.op_step("random")
    L.run([])


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_step_fused_in_every_mode(mode, sub):
    """step_fused on these modes goes to the general kernels: one launch with an explicit first action, three without, three more
    with no host access in between (from the second of those on the prepared launch carries DSIM_OPT_MEM_DERIVED: results
    do not depend on it), then three Env.steps in one launch where the mode has no neighbour term — against
    O.physics[_downwash] + O.control with last_action = None (the fused rule: the current command's rotor speeds).  A step(action) in front and behind: the fused steps leave the env's last action alone."""
    L = _loop(f"fused[{mode} sub={sub}]", mode, ["tello" if mode == "PYB_DRAG" else "robobee"], sub)
    env = L.env
    L.op_step("random")
    last = L.last.copy()
    L.op_step_fused(True, 1)
    for k in range(3):
        L.op_step_fused(False, 1)                               # (the model reads the state in front of each: no hint here)
    L.op_step_fused_run(3)                                      # no host access in between: the hint is handed over
    if mode != "PYB_GND_DRAG_DW":
        assert env._fused_plan is not None and env._fused_plan.args.options & OPT_MEM_DERIVED
        assert env._fused_plan.args.options & 3 == L.opts
        L.op_step_fused(False, 3)
    else:
        with pytest.raises(ValueError):
            env.step_fused(L.tg, n_steps=3)
    L.op_observe()                                              # (the rows echo the controller's command now)
    np.testing.assert_array_equal(L.last, last)
    np.testing.assert_array_equal(env._last_action[:, :L.n].cpu().numpy().T, last[:, :4].astype(np.float32))
    L.op_step("random")                                         # ... and this step's drag starts from `last`, not from the command
    L.op_observe()
    L.run([])


@pytest.mark.parametrize("mode", ["PYB_GND", "PYB_DRAG"])
def test_capture_fused_replays_what_eager_stepping_computes(mode):
    """What the code does today, pinned: capture_fused() captures these modes (the general step kernel under a graph), and the
    replay is bit-equal to the same number of eager step_fused() calls on a twin env — and within the step's bar of the oracle."""
    A = _loop(f"graph[{mode}]", mode, ["robobee"], 2, n=128)
    B = _loop(f"graph twin[{mode}]", mode, ["robobee"], 2, n=128)
    for L in (A, B):
        L.op_step("random")
        L.op_step_fused(True, 1)
    np.testing.assert_array_equal(A.dev_state()[0], B.dev_state()[0])
    A.op_graph(3)
    for _ in range(3):
        B.op_step_fused(False, 1)
    for a, b in zip(A.dev_state(), B.dev_state()):
        np.testing.assert_array_equal(a, b)
    A.op_graph(3)                                               # the same graph again, behind nothing but itself
    for _ in range(3):
        B.op_step_fused(False, 1)
    for a, b in zip(A.dev_state(), B.dev_state()):
        np.testing.assert_array_equal(a, b)
    A.run([]); B.run([])


def test_with_rotor_noise():
    """A non-zero noise seed on the mode with everything in it, the noise fed to the oracle as the fuzz model does (Env.step split
    per sub-step draws the stream of the one-launch step: tests/test_gpu_two_call_loop.py)."""
    L = _loop("noise[PYB_GND_DRAG_DW]", "PYB_GND_DRAG_DW", ["robobee"], 2, n=64, noise_seed=7)
    for _ in range(3):
        L.op_step("random")
    L.op_step_fused(True, 1)
    L.op_step_fused(False, 1)
    L.op_step("random")
    L.op_observe()
    L.run([])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("models", [["hexa_6DOF"], ["robobee", "hexa_6DOF"]])
def test_hexa_fleets_are_refused_at_construction(models, mode):
    """The add-on formulas are written for the four rotor links: the library refuses every step of a table with a six-actuator
    type (tests/test_gpu_aero_edges.py), and the env says so when it is built, as it does for Physics.DYN."""
    from dronesim_amd.envs import CtrlAviary
    with pytest.raises(NotImplementedError, match="four-rotor"):
        CtrlAviary(models, len(models), initial_xyzs=np.ones((len(models), 3)), physics=_mode(mode), noise_seed=0, dict_io=False)
    # (the same fleets under the plain mode are built and fly)
    env = CtrlAviary(models, len(models), initial_xyzs=np.ones((len(models), 3)), noise_seed=0, dict_io=False)
    env.step(np.full((len(models), 6), 0.5, dtype=np.float32))
    env.close()
