"""Drag (P6, DSIM_OPT_DRAG) and ground effect (P7, DSIM_OPT_GROUND) through the C-ABI, at the edges of both formulas: the
ground-effect gate from both sides of each of its thresholds, the per-rotor height clip (at the clip to the ulp, under the
ground, 100 m up, rotors on both sides of it), drag at rest and up to 30 m/s with the previous action far from the current
one — on robobee, tello and an interleaved table of both (tiles partitioned by type), plain SoA and tile64, ragged sizes.

The inputs are tests/util.py's aero_* builders; tests/test_aero_inputs_cpu.py certifies them without a device (both gate
predicates agree with margin at every sub-step of every launch made here; what each comparison would tell of a dropped
term, a wrong previous action or a flipped gate).  No case is excluded from any comparison.  The bar is the step's own:
assert_step_parity with K_ULP x sub-steps x the ground-effect boost at the clip, as
tests/test_gpu_parity.py::test_drag_and_ground_effect_vs_oracle builds it; the drag force and the external force join the
magnitudes of the velocity update (tests/util.py:aero_terms, from the oracle's constants and the state in front of the step).

Padding lanes: the ABI computes and ignores them (include/dronesim_amd.h, "n_pad must be a multiple of 64 (padding lanes
are computed and ignored)"), so their state is not pinned here.  What is: nothing is written outside [0, n_pad) of the state
block and of the echo buffer (guard words on both sides), the echo rows of the padding lanes hold the clipped "action" of
those lanes like everybody else's, and a refused call writes nothing at all.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from dronesim_amd import params  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests.test_gpu_parity import _args  # noqa: E402
from tests.util import (AERO_CLASSES, K_ULP, OPT_GROUND, aero_boost, aero_fleet, aero_fused_starts, aero_gate_margins,  # noqa: E402
                        aero_substep_starts, aero_terms, assert_step_parity, control_rounding_part, f32)

pytestmark = pytest.mark.gpu
DT = float(np.float32(1.0 / 240.0))
SENT = -7.25                     # what guard words and untouched blocks hold
GUARD = 256                      # floats on either side of a guarded buffer
E_UNSUPPORTED = -5               # DSIM_E_UNSUPPORTED (include/dronesim_amd.h)
OPT_MEM_DERIVED = 1 << 21

TABLES = {"robobee": ("robobee",), "tello": ("tello",), "mixed": ("robobee", "tello")}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def _a6(a):
    out = np.zeros((len(a), 6)); out[:, :a.shape[1]] = a
    return out


class Guarded:
    """A flat fp32 device buffer of `numel` floats between two runs of GUARD sentinel words."""

    def __init__(self, numel, device, fill=0.0):
        self.big = torch.full((numel + 2 * GUARD,), SENT, dtype=torch.float32, device=device)
        self.t = self.big[GUARD:GUARD + numel]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.big[:GUARD] == SENT).all()) and bool((self.big[-GUARD:] == SENT).all())


class Rig:
    """One type table, one fleet of aero cases, its state block (guarded, the padding lanes of the SoA form left at the
    sentinel), targets, and the oracle."""

    def __init__(self, gpu, table, layout, n, n_state=1):
        self.nat, fleet = gpu
        self.names = TABLES[table]
        self.types = [params.builtin_type(m) for m in self.names]
        self.ctx = fleet.Context(self.types)
        self.O = orc.Oracle(self.types)
        self.n, self.layout = n, layout
        self.f = aero_fleet(self.types, n)
        self.tid = self.f["tid"]
        self.states, self.blocks = [], []
        for _ in range(n_state):
            st = fleet.FleetState(self.ctx, n, layout)
            g = Guarded(st._data.numel(), self.ctx.device, SENT)
            st._data = g.t.view(st._data.shape)
            self.states.append(st); self.blocks.append(g)
        self.st = self.states[0]
        self.n_pad = self.st.n_pad
        self.tid_dev = None
        if self.tid is not None:
            t = np.zeros(self.n_pad, dtype=np.uint8); t[:n] = self.tid
            self.tid_dev = torch.from_numpy(t).to(self.ctx.device)
        self.tg = fleet.Targets(self.ctx, n, layout)
        self.tg.set_fields(0, torch.from_numpy(np.ascontiguousarray(self.f["tgt"].T)))
        self.boost = lambda opts: aero_boost(self.types, opts)

    def load(self, rigid=None, mem=None):
        for st in self.states:
            st.load_aos(self.f["rigid"] if rigid is None else rigid, self.f["mem"] if mem is None else mem)

    def soa(self, a, rows=None):
        """[n, k] host -> guarded [k, n_pad] device, the padding lanes zero"""
        k = a.shape[1] if rows is None else rows
        g = Guarded(k * self.n_pad, self.ctx.device)
        v = g.t.view(k, self.n_pad)
        v[:a.shape[1], :self.n] = torch.from_numpy(np.ascontiguousarray(a.T)).float().to(self.ctx.device)
        return g, v

    def full_fields(self, st):
        """[F, n_pad] host copy of the whole block, padding lanes included"""
        d = st._data
        if self.layout == "soa":
            return d.cpu().numpy().copy()
        return d.permute(1, 0, 2).reshape(st.n_fields, st.n_pad).cpu().numpy().copy()

    def physics(self, st, sub, opts, act_v, echo_v, ext_v=None):
        a = _args(self.nat, sub, DT, DT, options=opts, action=act_v, type_id=self.tid_dev)
        a.ext_force = ext_v.data_ptr() if ext_v is not None else None
        return self.ctx.lib.dsim_physics(self.ctx.handle, self.ctx.stream_ptr(), self.n, st.view(),
                                         echo_v.data_ptr() if echo_v is not None else None, ctypes.byref(a))

    def step(self, st, sub, opts, n_steps=1):
        a = _args(self.nat, sub, DT, float(np.float32(sub / 240)), options=opts, type_id=self.tid_dev)
        a.n_steps = n_steps
        return self.ctx.lib.dsim_step(self.ctx.handle, self.ctx.stream_ptr(), self.n, st.view(), self.tg.view(), ctypes.byref(a))

    def gate_clear(self, label, starts, opts):
        """In front of a launch: along the oracle's run from the device's own state no drone sits where the fp32 and the fp64
        gate could disagree (tests/test_aero_inputs_cpu.py shows it for the oracle's own states).  Nothing is excluded: a drone
        that fails this is a badly built input and fails the test."""
        if not opts & OPT_GROUND:
            return
        for k, r in enumerate(starts):
            open32, open64, clear, _ = aero_gate_margins(f32(r[:, 3:7]))
            assert clear.all() and np.array_equal(open32, open64), (label, "sub-step", k, np.flatnonzero(~clear))

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("opts", [1, 2, 3])
@pytest.mark.parametrize("n", [200, 333])
@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("table", list(TABLES))
def test_physics_at_the_edges(gpu, table, layout, n, opts):
    """dsim_physics at 1 and 3 sub-steps: (a) explicit action, the echo buffer holding the previous one; (b) the same without
    an echo buffer (drag falls back to the current action); (c) no action (the stored command) with an echo buffer."""
    R = Rig(gpu, table, layout, n)
    f, O, tid, types = R.f, R.O, R.tid, R.types
    before, mem, tgt = f["rigid"], f["mem"], f["tgt"]
    act_g, act_v = R.soa(f["act"])
    for sub in (1, 3):
        for how in ("echo", "no_echo", "stored"):
            R.load()
            echo_g, echo_v = R.soa(f["prev"])
            action = None if how == "stored" else _a6(f["act"])
            last = None if how == "no_echo" else _a6(f["prev"])
            raw = f["mem"][:, 7:11] if how == "stored" else f["act"]
            applied = np.clip(raw, 0.0, 1.0)
            starts, ref = aero_substep_starts(O, tid, before, mem, sub, DT, action=action, options=opts, last_action=last)
            R.gate_clear((table, how, sub), starts, opts)
            pad_cmd = np.clip(R.full_fields(R.st)[20:24, n:], 0.0, 1.0)              # the padding lanes' stored "command"
            R.nat.check(R.physics(R.st, sub, opts, None if how == "stored" else act_v, None if how == "no_echo" else echo_v))
            got = R.st.rigid_aos()
            rpm_cmd = applied if how == "no_echo" else np.maximum(applied, f["prev"])
            assert_step_parity(f"aero physics[{table} {layout} {how} opts={opts}]", types, tid, before, mem, tgt, got, None, ref, None,
                               DT, DT, sub, control=False, k=K_ULP * sub * R.boost(opts), action=applied,
                               extra_terms=aero_terms(types, tid, before, rpm_cmd, DT, sub, opts))
            np.testing.assert_array_equal(R.st.mem_aos(), mem)                       # the controller memory is not the env's
            e = echo_v.cpu().numpy()
            if how == "no_echo":
                np.testing.assert_array_equal(e[:, :n], f["prev"].T.astype(np.float32))        # nobody wrote it
            else:
                np.testing.assert_array_equal(e[:, :n], applied.T.astype(np.float32))          # clip(action, 0, 1), bit for bit
                assert (applied != raw).any() or how == "stored"                             # (the clip was exercised)
                # the padding lanes are computed like everybody else: their rows hold the clip of what stood for their action
                np.testing.assert_array_equal(e[:, n:], pad_cmd if how == "stored" else np.zeros_like(pad_cmd))
            assert R.blocks[0].intact() and echo_g.intact() and act_g.intact()
    R.close()


@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("table", list(TABLES))
def test_drag_at_rest_is_exactly_nothing(gpu, table, layout):
    """A drone at rest: the drag force is R (-c w 0), a signed zero, whatever the rotors did before — one sub-step with two
    very different previous actions gives the same bits, and with the ground effect beside it (options 3) the bits of the step
    without the drag (options 2: the same kernel instance)."""
    n = 333
    R = Rig(gpu, table, layout, n)
    f = R.f
    rest = (f["cls"] == AERO_CLASSES.index("drag")) & (np.linalg.norm(f["rigid"][:, 7:10], axis=1) == 0)
    assert rest.sum() >= 3
    _, act_v = R.soa(f["act"])
    out = {}
    for key, opts, prev in (("a", 1, f["prev"]), ("b", 1, 1.0 - f["prev"]), ("c", 3, f["prev"]), ("d", 2, f["prev"])):
        R.load()
        _, echo_v = R.soa(f32(prev))
        R.nat.check(R.physics(R.st, 1, opts, act_v, echo_v))
        out[key] = R.st.fields(0, 13).T.cpu().numpy()
    assert np.array_equal(out["a"][rest], out["b"][rest]) and np.array_equal(out["c"][rest], out["d"][rest])
    assert not np.array_equal(out["a"][~rest], out["b"][~rest])                      # (for everybody else it matters)
    R.close()


@pytest.mark.parametrize("n", [200, 333])
@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("table", list(TABLES))
def test_physics_with_an_external_force_and_both_terms(gpu, table, layout, n):
    """The kernel path of Physics.PYB_GND_DRAG_DW: F2 = F + ext, then ground effect and drag, in one launch — with body-frame
    forces of the order of the vehicle's weight in every direction."""
    R = Rig(gpu, table, layout, n)
    f, O, tid, types = R.f, R.O, R.tid, R.types
    rng = np.random.default_rng(7400 + n)
    weight = np.array([t.mass * t.gravity for t in types])[np.zeros(n, dtype=int) if tid is None else tid.astype(int)]
    ext = f32(rng.normal(size=(n, 3)) * weight[:, None])
    ext_g, ext_v = R.soa(ext)
    _, act_v = R.soa(f["act"])
    applied = np.clip(f["act"], 0.0, 1.0)
    for sub in (1, 3):
        R.load()
        echo_g, echo_v = R.soa(f["prev"])
        starts, ref = aero_substep_starts(O, tid, f["rigid"], f["mem"], sub, DT, action=_a6(f["act"]), options=3,
                                          last_action=_a6(f["prev"]), ext_force=ext)
        R.gate_clear((table, "ext", sub), starts, 3)
        R.nat.check(R.physics(R.st, sub, 3, act_v, echo_v, ext_v))
        assert_step_parity(f"aero physics ext[{table} {layout}]", types, tid, f["rigid"], f["mem"], f["tgt"], R.st.rigid_aos(), None,
                           ref, None, DT, DT, sub, control=False, k=K_ULP * sub * R.boost(3), action=applied,
                           extra_terms=aero_terms(types, tid, f["rigid"], np.maximum(applied, f["prev"]), DT, sub, 3, ext))
        plain = f["rigid"].copy()
        O.physics(plain, f["mem"], sub, DT, action=_a6(f["act"]), options=3, type_id=tid, last_action=_a6(f["prev"]))
        assert np.abs(plain - ref)[:, 7:10].max(1).min() > 1e-4                      # the force is live on every drone
        assert R.blocks[0].intact() and echo_g.intact() and ext_g.intact()
    R.close()


@pytest.mark.parametrize("opts", [1, 2, 3])
@pytest.mark.parametrize("n", [200, 333])
@pytest.mark.parametrize("layout", ["soa", "tile64"])
@pytest.mark.parametrize("table", list(TABLES))
def test_fused_step_at_the_edges(gpu, table, layout, n, opts):
    """dsim_step (the general kernel; drag with the current command's rotor speeds) at 1 and 2 sub-steps, on a block and its twin:
      1. one Env.step + computeControl from the cases, both blocks alike;
      2. the same again, one block with DSIM_OPT_MEM_DERIVED (valid: a fused step left the block) and its twin without;
      3. three Env.steps in ONE launch (n_steps = 3, with the hint) on one block, three launches of one on the twin.
    After every launch the two blocks hold the same bits, and every launch of ONE Env.step is judged against O.step from the
    device's own previous state, controller memory included (the commands with the oracle's own sensitivity to the rounding of the
    quaternion beside them, tests/util.py:control_rounding_part: the pitch cases hover at the gimbal point).  That is the parity of the n_steps launch with O.step iterated:
    step by step at the single-step bar, through its bit-equal twin.  (Its END state is not compared with three oracle steps
    from its start: the quad law's command is known to k / cos^2(roll) ulps only (tests/util.py:tilt_gain), a million ulps for
    the gate cases at roll = pi/2 -+ delta, and the next Env.step of the same launch turns that into torque.)"""
    R = Rig(gpu, table, layout, n, n_state=2)
    f, O, tid, types = R.f, R.O, R.tid, R.types
    A, B = R.states

    def single(label, sub, dtc, hint_a):
        """one Env.step on both blocks (A with hint_a), bit-equal, against the oracle"""
        r0, m0 = B.rigid_aos(), B.mem_aos()
        starts, _, _, r, m = aero_fused_starts(O, tid, r0, m0, f["tgt"], sub, DT, dtc, opts, 1)
        R.gate_clear((table, "fused", sub, label), starts, opts)
        if hint_a is not None:
            R.nat.check(R.step(A, sub, opts | hint_a, 1))
        R.nat.check(R.step(B, sub, opts, 1))
        assert_step_parity(f"aero fused[{table} {layout} opts={opts}]", types, tid, r0, m0, f["tgt"], B.rigid_aos(), B.mem_aos(), r, m,
                           DT, dtc, sub, k=K_ULP * sub * R.boost(opts), action=m0[:, 7:11],
                           extra_terms=aero_terms(types, tid, r0, m0[:, 7:11], DT, sub, opts),
                           part_mem=control_rounding_part(O, tid, r, m0, f["tgt"], dtc))     # (r: the state the law evaluates)

    def same_bits():
        np.testing.assert_array_equal(R.full_fields(A)[:, :n], R.full_fields(B)[:, :n])

    for sub in (1, 2):
        dtc = float(np.float32(sub / 240))
        R.load()
        single("first", sub, dtc, 0); same_bits()
        single("hinted", sub, dtc, OPT_MEM_DERIVED); same_bits()
        R.nat.check(R.step(A, sub, opts | OPT_MEM_DERIVED, 3))
        for k in range(3):
            single(f"one of three {k}", sub, dtc, None)
        same_bits()
        assert R.blocks[0].intact() and R.blocks[1].intact()
    R.close()


@pytest.mark.parametrize("opts", [1, 2, 3])
@pytest.mark.parametrize("names", [("hexa_6DOF",), ("robobee", "hexa_6DOF")])
def test_six_actuator_tables_are_refused_and_nothing_is_written(gpu, names, opts):
    """The add-on formulas are written for the four rotor links: a table that holds a six-actuator type is refused by
    dsim_physics and dsim_step with DSIM_E_UNSUPPORTED, and the state block and the echo buffer keep every bit."""
    nat, fleet = gpu
    n = 200
    types = [params.builtin_type(m) for m in names]
    ctx = fleet.Context(types)
    st = fleet.FleetState(ctx, n, "soa")
    tg = fleet.Targets(ctx, n, "soa")
    pattern = lambda numel: torch.arange(numel, dtype=torch.float32, device=ctx.device) * 0.5 - 3.0
    st._data.copy_(pattern(st._data.numel()).view(st._data.shape))
    echo = pattern(6 * st.n_pad).view(6, st.n_pad).clone()
    act = torch.full((6, st.n_pad), 0.5, device=ctx.device)
    tid = torch.from_numpy((np.arange(st.n_pad) % len(types)).astype(np.uint8)).to(ctx.device) if len(types) > 1 else None
    block0, echo0 = st._data.clone(), echo.clone()
    for sub in (1, 3):
        a = _args(nat, sub, DT, DT, options=opts, action=act, type_id=tid)
        assert ctx.lib.dsim_physics(ctx.handle, ctx.stream_ptr(), n, st.view(), echo.data_ptr(), ctypes.byref(a)) == E_UNSUPPORTED
        assert ctx.lib.dsim_physics(ctx.handle, ctx.stream_ptr(), n, st.view(), None, ctypes.byref(a)) == E_UNSUPPORTED
        for action in (act, None):
            a = _args(nat, sub, DT, float(np.float32(sub / 240)), options=opts, action=action, type_id=tid)
            a.n_steps = 1
            assert ctx.lib.dsim_step(ctx.handle, ctx.stream_ptr(), n, st.view(), tg.view(), ctypes.byref(a)) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(st._data, block0) and torch.equal(echo, echo0)
    with pytest.raises(nat.DsimError):
        nat.check(E_UNSUPPORTED)
    ctx.close()
