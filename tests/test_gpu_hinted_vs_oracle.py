"""The hinted instances of the fused step against the ORACLE, gentle flight and the whole envelope of row P4: DSIM_OPT_TGT_CONST
(TC: vel / acc / yaw from the kernel arguments), dsim_step_args.tgt_period (the targets of the first period only),
DSIM_OPT_MEM_DERIVED (MD: last_vel / last_rates recomputed on load) and their combinations — k_step_fast<.., TC, MD> with a period is
the instance the benchmark headline times, k_step_hexa<.., MD> the hexa headline.  tests/test_gpu_tgt_const.py, test_gpu_tgt_period.py
and test_gpu_mem_derived.py compare these instances with their siblings bit for bit in gentle flight; here each is launched through the
C-ABI on its own (tests/test_gpu_parity.py:_sweep_case: both cache policies, noise off and on), judged on every drone at the step bar
(tests/util.py:assert_step_parity, unchanged), and a second launch with NaN in every field the hint covers proves WHICH instance ran.

How the MD precondition (last_vel == vel, last_rates == R(q)^T w) is built, per regime:
  every regime but omega_clamp    on the HOST, as _sweep_case builds it for DSIM_OPT_CHAINED: last_rates = f32 of the fp64 body
      rates.  The oracle reads that value while the kernel recomputes its own fp32 one; the two differ by a few ulp32(|w|), which
      the law divides by dt_ctrl.  (non_unit, wreck and wreck_100Hz could not be built otherwise: a step on the device normalises
      the quaternion.)
  omega_clamp (PRIMED)    by a device PRIMING step (_sweep_case(prime=True)): one un-hinted dsim_step from the regime's state, read
      back as (r0, m0), last_vel == vel asserted bit for bit; launch and oracle are judged from (r0, m0), whose rates sit on and
      around the +-100 rad/s clamp.  With the host construction `hexa MD sub1|omega_clamp|0` came out at 1.032 of the bar in cmd5
      of drone 854 (error -1.58e-5 against 1.53e-5; w_y = -93 rad/s, the fp32 body rates up to 6 ulp32(100) from the rounded fp64
      ones): handing the ORACLE the fp32 body rates moves its cmd5 of that drone by -7.7e-6, half of the error — the excess is the
      rounding of the value the oracle read, not the kernel's arithmetic.  Primed, the same label measures 0.474.
  Measured and NOT adopted, for review: primed as well, `hexa MD sub1|pi4_100Hz|0` measures 1.32 (host construction: 0.46) in
      last_thrust of drone 418, error -2.5e-5 against 1.9e-5.  Behind a step at |w| up to 170 rad/s the stored base-link velocity of
      the morphing hexa, v_com + w x (R d), turns by |w|^2 |d| dt = 3 m/s per step, and the law differentiates it: the operand
      |w| |d| / dt_ctrl (190 m/s^2) is not among the terms tests/util.py:step_terms counts for that field (it counts |v| / dt_ctrl:
      114).  It concerns k_step_hexa with and without the hint alike (they are bit-identical there, see the last test but one); the
      bar is left as it is.
test_mem_derived_bits_equal_sibling_over_the_envelope primes in every regime: there the claim is bit-identity with the sibling.

tests/test_hinted_inputs_cpu.py runs the oracle alone on every input constructed here, without a device."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from dronesim_amd import _native as nat_consts  # noqa: E402
from dronesim_amd import params  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests.test_gpu_envelope import REGIMES, _collect  # noqa: E402
from tests.test_gpu_parity import _args, _fill_tgt_const, _poison, _stream, _sweep_case, _sweep_inputs, _wrap_diff  # noqa: E402
from tests.util import assert_control_parity, ulp32  # noqa: E402

pytestmark = pytest.mark.gpu

SPREAD = 2.0      # m: half-width of the fleets whose targets repeat — the replicas' position errors lie on both sides of the clip


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    from dronesim_amd import _native as nat
    from dronesim_amd import fleet
    return nat, fleet


def hinted_families(group=None):
    """name -> keywords of _sweep_case (+ "group", "model"): every instance of dsim_step that honours a traffic hint, and the
    launches that carry DSIM_OPT_MEM_DERIVED to kernels that ignore it.  n = 1024 in whole tiles (tile64, pad 256) unless stated.
    Group "tc": the constant and periodic targets; group "md": everything with DSIM_OPT_MEM_DERIVED."""
    CH = nat_consts.OPT_CHAINED
    fam = {}
    for sub in (1, 5):
        s = f"sub{sub}"
        fam[f"TC {s}"] = dict(group="tc", sub=sub, tgt_const=True, witness=True)
        fam[f"TC CH {s}"] = dict(group="tc", model="tello", sub=sub, options=CH, tgt_const=True, witness=True)
        fam[f"period {s}"] = dict(group="tc", sub=sub, tgt_period=256, witness=True)      # all ten fields read, of one period
        fam[f"TC period {s}"] = dict(group="tc", sub=sub, tgt_const=True, tgt_period=512, witness=True)     # two tiles: the mask form
    fam["TC period mod sub1"] = dict(group="tc", sub=1, n=1536, tgt_const=True, tgt_period=768, witness=True)   # three tiles: the modulo
    fam["TC MD sub1"] = dict(group="md", sub=1, tgt_const=True, mem_derived=True, witness=True)
    fam["headline TC MD period sub1"] = dict(group="md", sub=1, tgt_const=True, mem_derived=True, tgt_period=256, witness=True)
    # ragged fleets.  n = 712: n_pad = 768, three whole tiles — the padding lanes sit INSIDE the last tile of the MD instance.
    # n = 840 with pad 64: n_pad = 896, three tiles to the MD instance and a 128-drone tail to the general kernel, which reads the
    # fields (the witness poisons the whole tiles only); the same oracle judges both parts
    fam["TC MD ragged sub1"] = dict(group="md", sub=1, n=712, tgt_const=True, mem_derived=True, witness=True)
    fam["TC MD ragged + tail sub1"] = dict(group="md", sub=1, n=840, pad=64, tgt_const=True, mem_derived=True, witness=True)
    fam["hexa MD sub1"] = dict(group="md", model="hexa_6DOF", sub=1, mem_derived=True, witness=True)
    # the bit carried to kernels that are documented to ignore it (all ten target fields read; several sub-steps): the
    # precondition is true, so parity with the oracle must hold all the same.  No witness: these launches read the fields
    fam["quad MD without TC sub1"] = dict(group="md", sub=1, mem_derived=True)
    fam["TC MD sub5"] = dict(group="md", sub=5, tgt_const=True, mem_derived=True)
    return {k: v for k, v in fam.items() if group is None or v["group"] == group}


def family_case(kw, fleet_kw):
    """(types, n, keywords of _sweep_case) of one family; fleets with periodic targets are SPREAD wide."""
    kw = dict(kw)
    kw.pop("group")
    types = [params.builtin_type(kw.pop("model", "robobee"))]
    n = kw.pop("n", 1024)
    fleet_kw = dict(fleet_kw)
    if kw.get("tgt_period"):
        fleet_kw["spread"] = SPREAD
    return types, n, dict(kw, fleet_kw=fleet_kw)


PRIMED = ("omega_clamp",)      # regimes whose MD precondition comes from a device priming step (module docstring)


def _run_family(gpu, label, kw, seed, fleet_kw, dt_phys=None, regime=None):
    types, n, kw = family_case(kw, fleet_kw)
    prime = regime in PRIMED and kw.get("mem_derived", False)
    _sweep_case(gpu, label, types, None, n, kw.pop("sub"), seed, kw.pop("options", 0), dt_phys=dt_phys, prime=prime, **kw)


GENTLE = dict(tilt=0.3, rate=1.0)


@pytest.mark.parametrize("group", ["tc", "md"])
@pytest.mark.parametrize("seed", [0, 7])
def test_hinted_instances_vs_oracle(gpu, seed, group):
    """Gentle flight, noise off (seed 0) and on (7): with both cache policies of _sweep_case all 16 plain TC instances of k_step_fast,
    its 4 MD instances and the 4 MD instances of k_step_hexa, each with its witness."""
    failures = []
    for name, kw in hinted_families(group).items():
        _collect(failures, _run_family, gpu, f"hinted[{name}|gentle|{seed}]", kw, seed, GENTLE)
    assert not failures, failures


@pytest.mark.parametrize("group", ["tc", "md"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_hinted_instances_over_the_envelope(gpu, regime, group):
    """Every family through one regime of tests/test_gpu_envelope.py (the velocity and rate clamps, the pi/4 rotation clamp, tiny
    rates, non-unit quaternions, tumbling, all at once).  The MD precondition: a device priming step in the regimes PRIMED, the
    host construction in the others (module docstring)."""
    env, hz = REGIMES[regime]
    failures = []
    for name, kw in hinted_families(group).items():
        for seed in ((0, 7) if regime in ("wreck", "omega_clamp") else (0,)):
            _collect(failures, _run_family, gpu, f"hinted[{name}|{regime}|{seed}]", kw, seed, dict(envelope=env), dt_phys=1.0 / hz,
                     regime=regime)
    assert not failures, failures


MD_KINDS = {"quad TC": ("robobee", True, 0), "quad TC + period": ("robobee", True, 256), "hexa": ("hexa_6DOF", False, 0)}


@pytest.mark.parametrize("kind", list(MD_KINDS))
@pytest.mark.parametrize("regime", list(REGIMES))
def test_mem_derived_bits_equal_sibling_over_the_envelope(gpu, regime, kind):
    """The claim of dsim_step.hip (MD is bit-identical to the sibling that reads the six fields: one pinned body_rates at both ends,
    the recomputation kept apart from the physics), taken over the envelope: one un-hinted priming dsim_step from the regime's
    state — after it the precondition holds bit for bit by construction —, then eight steps on two copies of the block, one with
    DSIM_OPT_MEM_DERIVED and one without; the whole block equal after every step, and last_vel == vel.  Both cache policies, noise
    off and on."""
    nat, fleet = gpu
    model, tc, period = MD_KINDS[kind]
    t = params.builtin_type(model)
    env, hz = REGIMES[regime]
    DT = float(np.float32(1.0 / hz))
    n = 512
    fleet_kw = dict(envelope=env, spread=SPREAD) if period else dict(envelope=env)
    for pol in (nat.OPT_STREAM_ON, nat.OPT_STREAM_OFF):
        for seed in (0, 7):
            rigid, mem, tgt = _sweep_inputs([t], None, n, 1, seed, False, fleet_kw, tgt_const=tc, tgt_period=period)
            ctx = fleet.Context([t])
            sts = [fleet.FleetState(ctx, n, "tile64"), fleet.FleetState(ctx, n, "tile64")]
            tg = fleet.Targets(ctx, n, "tile64")
            assert sts[0].n_pad == n
            sts[0].load_aos(rigid, mem)
            tg.set_fields(0, torch.from_numpy(np.ascontiguousarray(tgt.T)))
            a = _args(nat, 1, DT, DT, options=pol, seed=seed, step_index=3)
            nat.check(ctx.lib.dsim_step(ctx.handle, _stream(ctx), n, sts[0].view(), tg.view(), ctypes.byref(a)))
            sts[1]._data.copy_(sts[0]._data)
            for k in range(9):
                if k:
                    for st, md in zip(sts, (nat.OPT_MEM_DERIVED, 0)):
                        a = _args(nat, 1, DT, DT, options=pol | md, seed=seed, step_index=3 + k)
                        if tc:
                            _fill_tgt_const(nat, a, tgt[0])
                        a.tgt_period = period
                        nat.check(ctx.lib.dsim_step(ctx.handle, _stream(ctx), n, st.view(), tg.view(), ctypes.byref(a)))
                blocks = [st._data.cpu().numpy() for st in sts]
                where = f"{kind}|{regime}|seed {seed}|policy {pol}|step {k}"
                assert np.isfinite(blocks[0]).all(), where
                assert np.array_equal(blocks[0], blocks[1]), (where, np.abs(blocks[0] - blocks[1]).max(axis=(0, 2)))
                assert np.array_equal(blocks[0][:, 13:16, :], blocks[0][:, 7:10, :]), where      # last_vel == vel, bit for bit
            ctx.close()


@pytest.mark.parametrize("fleet_name", ["gentle", "tumbling", "omega_clamp"])
def test_hinted_control_vs_oracle(gpu, fleet_name):
    """dsim_control2 with DSIM_OPT_TGT_CONST (k_control_fast<NT, WANT_YAW, TC>: all four TC instances) against the oracle's
    computeControl: the controller memory at assert_control_parity, the command array equal to the stored command, pos_e and yaw_e
    within the bounds of test_gpu_parity.py::test_control_vs_golden (one fp32 subtraction; one atan2 of angles up to ~4 rad, times
    the conditioning 1 / cos(pitch)).  The constants of _sweep_case's tgt_const; a second launch with NaN in the seven constant
    target fields proves that the TC instance ran."""
    nat, fleet = gpu
    t = params.builtin_type("robobee")
    O = orc.Oracle([t])
    n = 1024
    fleet_kw = GENTLE if fleet_name == "gentle" else dict(envelope=fleet_name)
    for pol in (nat.OPT_STREAM_ON, nat.OPT_STREAM_OFF):
        for want_yaw, seed, sub in ((True, 7, 1), (False, 0, 5)):
            dtc = float(np.float32(sub / 240))
            rigid, mem, tgt = _sweep_inputs([t], None, n, sub, seed, False, fleet_kw, tgt_const=True)
            label = f"hinted control[{fleet_name}|yaw {want_yaw}]"
            m_ref = mem.copy()
            rc, pe_ref, ye_ref = O.control(rigid, m_ref, tgt, dtc)
            assert rc == 0 and np.isfinite(m_ref).all()
            got = None
            for poisoned in (False, True):
                ctx = fleet.Context([t])
                st, tg = fleet.FleetState(ctx, n, "tile64"), fleet.Targets(ctx, n, "tile64")
                st.load_aos(rigid, mem)
                tg.set_fields(0, torch.from_numpy(np.ascontiguousarray(tgt.T)))
                if poisoned:        # breaks the caller's side of the contract on purpose, to pin dispatch (_sweep_case)
                    _poison(tg, 3, 10, 0, n)
                pos_e = torch.zeros((3, st.n_pad), device=ctx.device)
                yaw_e = torch.zeros((st.n_pad,), device=ctx.device)
                cmd = torch.zeros((4, st.n_pad), device=ctx.device)
                a = _args(nat, 0, dtc, dtc, options=pol)
                _fill_tgt_const(nat, a, tgt[0])
                nat.check(ctx.lib.dsim_control2(ctx.handle, _stream(ctx), n, st.view(), tg.view(), ctypes.byref(a), pos_e.data_ptr(),
                                                yaw_e.data_ptr() if want_yaw else None, cmd.data_ptr()))
                res = (st.mem_aos(), pos_e.T.double().cpu().numpy(), yaw_e.double().cpu().numpy(), cmd.T.double().cpu().numpy())
                np.testing.assert_array_equal(st.rigid_aos(), rigid)              # computeControl leaves the rigid state alone
                ctx.close()
                if poisoned:
                    for x, y in zip(res, got):
                        assert np.isfinite(x).all(), label
                        np.testing.assert_array_equal(x, y, err_msg=label + " (witness)")
                else:
                    got = res
            got_m, pe, ye, cm = got
            assert_control_parity(label, [t], None, rigid, mem, tgt, got_m, m_ref, dtc)
            np.testing.assert_array_equal(cm, got_m[:, 7:11])
            assert (np.abs(pe - pe_ref) <= ulp32(np.maximum(np.abs(tgt[:, 0:3]), np.abs(rigid[:, 0:3])))).all(), label
            if want_yaw:
                pitch = np.array([orc.euler_from_quat(q)[1] for q in rigid[:, 3:7]])
                ytol = 8 * ulp32(4.0) / np.maximum(np.abs(np.cos(pitch)), 1e-3)
                assert (_wrap_diff(ye, ye_ref) <= ytol).all(), (label, (_wrap_diff(ye, ye_ref) / ytol).max())
            else:
                assert not ye.any()                                               # not asked for: not written
