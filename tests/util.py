"""Shared helpers for the parity tests (test infrastructure).

Two error metrics live here.

``rel_err`` — |gpu - oracle| / (|oracle| + 1): the round-1 metric.  For a position near +-50 m it
accepts 5 mm per step, about the size of one step's displacement, so on its own it says little
about the position update.  It is kept for quantities of order one and as a drift measure for
closed-loop trajectories.

``increment_ratio`` / ``assert_step_parity`` — the per-step bar applied to the state INCREMENT
of one step, which is what one launch computes:

    |d_gpu - d_oracle| <= 1e-4 |d_oracle| + k ulp32(M),      d = state_after - state_before,

``M`` = the largest magnitude that enters the fp32 update of that field (the field itself before and
after the step and the largest term added to it: ``step_terms``), ``k`` = a small count of fp32
roundings per physics sub-step (``K_ULP``).  The second term is the floor no fp32 kernel can go
below — the oracle computes the same update in fp64 from the same fp32 inputs — and it is per drone
and per field, never a blanket multiple of the bar: at x = 50 m it is k x 3.8e-6 m, not 5e-3 m.
"""
import math

import numpy as np

from oracle import oracle as orc

REL_TOL = 1e-4          # BASELINE.json north_star: per-step state within 1e-4 relative error
K_ULP = 2.0             # fp32 roundings allowed per physics sub-step / control evaluation, in ulps of the largest term
K_ULP_NOISE = 3.0       # ... with the rotor noise on: every rotor force and moment is then a sum of two terms and the lateral force and
                        # moment components exist at all — half again as many roundings in the wrench (assert_step_parity(noise=True))

# natural scale of each quantity: |gpu - oracle| / (|oracle| + scale) (drift metric, see above)
RIGID_SCALE = np.array([1.0] * 3 + [1.0] * 4 + [1.0] * 3 + [1.0] * 3)      # m, -, m/s, rad/s
MEM_SCALE = np.array([1.0] * 3 + [1.0] * 3 + [1.0] + [1.0] * 6)


def rel_err(got, ref, scale):
    return np.abs(got - ref) / (np.abs(ref) + scale[: ref.shape[1]])


def f32(a):
    """Round to fp32-representable values so GPU (fp32) and oracle (fp64) see identical inputs."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ulp32(x):
    """Spacing of fp32 numbers at |x| (element-wise)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return np.spacing(np.maximum(a, np.float32(1e-30))).astype(np.float64)


def step_terms(types, type_id, rigid, mem, tgt, dt_phys, dt_ctrl, substeps, control=True, action=None):
    """Largest magnitude entering the fp32 update of every state field during one fused step, per drone:
    (terms_rigid [n,13], terms_mem [n,13]).  Each entry is a sum of |coefficient| x |operand| over the
    operands of that field's update as the reference writes it (BaseAviary.py:1487-1543 wrench,
    p.stepSimulation, INDIControl.py:278-296, 433-459 / INDIControl_6DOF.py:399-413, 560-628):
      vel      (g + sum_i F_i / m + c (1 + |v|) |v|) dt      gravity and thrust accelerations cancel at hover
      ang vel  (sum_i |r_i| F_i / J_min + gyro |w|^2 + c (1 + |w|) |w|) dt + |w|      the rotor moments cancel pairwise; |w|: R w_b
      quat     1
      thrust   |v| / dt_ctrl + kd (kp |pos_e| + |v*| + |v|) + |a*|     the finite-difference acceleration
      cmd_j    sum_i |alloc_ji| term(nu_i),   nu_{0..2}: krate (katt + |w|) + |w| / dt_ctrl,
               nu_3 (quad): thrust term;  nu_{3..5} (hexa): the acceleration term
    """
    n = rigid.shape[0]
    tr = np.zeros((n, 13))
    tm = np.zeros((n, 13))
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    if tgt.shape[0] == 1 and n != 1:
        tgt = np.broadcast_to(tgt, (n, tgt.shape[1]))
    v = np.abs(rigid[:, 7:10]).max(1)
    w = np.linalg.norm(rigid[:, 10:13], axis=1)
    for k, t in enumerate(types):
        s = np.flatnonzero(tid == k)
        if s.size == 0:
            continue
        na = t.n_act
        cmd = np.clip((mem[s, 7:7 + na] if action is None else np.asarray(action)[s, :na]),   # the action the physics applies
                      np.asarray(t.pwm_min)[:na], np.asarray(t.pwm_max)[:na])
        rpm = np.asarray(t.pwm2rpm_scale)[:na] * cmd + np.asarray(t.pwm2rpm_const)[:na]
        F = t.kf * rpm ** 2                                               # [m, na]
        arm = np.linalg.norm(np.asarray(t.rotor_pos)[:na], axis=1)
        acc = (t.gravity + F.sum(1) / t.mass)
        alpha = ((F * arm).sum(1) + t.km * (rpm ** 2).sum(1)) / min(t.inertia)
        # Bullet's damping m v (c + c |v|), J w (c + c |w|) and the gyroscopic term w x J w (row P4): negligible in gentle
        # flight, the largest terms of the update near the velocity clamps (tests/util.py:random_fleet, envelope=)
        J = np.asarray(t.inertia, dtype=np.float64)
        gyro = max(abs(J[2] - J[1]) / J[0], abs(J[0] - J[2]) / J[1], abs(J[1] - J[0]) / J[2])
        vn = np.linalg.norm(rigid[s, 7:10], axis=1)
        acc = acc + t.lin_damping * (1.0 + vn) * vn
        alpha = alpha + gyro * w[s] ** 2 + t.ang_damping * (1.0 + w[s]) * w[s]
        tr[s, 0:3] = (v[s] + acc * dt_phys * substeps)[:, None] * dt_phys
        tr[s, 3:7] = 1.0
        # (a vehicle flown as a composite about another point than the reported one — the morphing hexa, params.base_offset —
        # reports v_com + w x (R d): operands of magnitude |w| |d|)
        tr[s, 7:10] = (acc * dt_phys + w[s] * float(np.linalg.norm(getattr(t, 'base_offset', (0.0, 0.0, 0.0)))))[:, None]
        # (every kernel turns w between the world and the body frame — the body-frame loop carries R^T w and stores R w_b — so every
        # world coordinate of w is a sum of three products of magnitude up to |w|: at 130 rad/s the rounding of R alone is worth
        # ulp32(130) in a coordinate that happens to be small)
        tr[s, 10:13] = (alpha * dt_phys + w[s])[:, None]
        if not control:
            continue
        v_new = v[s] + acc * dt_phys * substeps                           # bound on |v| after the physics
        w_new = w[s] + alpha * dt_phys * substeps
        pos_e = np.abs(tgt[s, 0:3] - rigid[s, 0:3]).max(1) + v_new * dt_phys * substeps
        # the finite-difference acceleration (v - last_vel) / dt: after a physics step v carries its own fp32 rounding,
        # amplified by 1 / dt; in a control-only call on given inputs the subtraction of two fp32 numbers is exact
        dv = v_new if dt_phys > 0 else np.abs(rigid[s, 7:10] - mem[s, 0:3]).max(1)
        a_term = dv / dt_ctrl + t.kd_pos * (t.kp_pos * pos_e + np.abs(tgt[s, 3:6]).max(1) + v_new) + np.abs(tgt[s, 6:9]).max(1)
        a_term = np.minimum(a_term, 6.0 + dv / dt_ctrl)                   # the clip at +-6 bounds what survives
        rate_term = (np.max(t.rate_gain) * (np.max(t.att_gain) + w_new) + w_new / dt_ctrl)
        tm[s, 0:3] = tr[s, 7:10]
        tm[s, 3:6] = (2.0 * w_new)[:, None] + tr[s, 10:13]
        tm[s, 6] = a_term
        A = np.abs(np.asarray(t.alloc, dtype=np.float64))                 # [n_act][n_out]
        if t.kind != 1:                                                   # the quad law (on four or six actuators)
            nu = np.stack([rate_term] * 3 + [a_term + np.abs(mem[s, 6])], 1)
            tm[s, 7:7 + na] = nu @ A[:na, :4].T
        else:
            A2 = np.abs(np.asarray(t.wls_first_iteration()[1], dtype=np.float64))
            nu = np.stack([rate_term] * 3 + [a_term] * 3, 1)
            tm[s, 7:13] = nu @ A[:6, :6].T + (A2 @ np.ones(6))[None, :]
    return tr, tm


NOISE_MAX_SIGMA = 4.8546       # |n| <= sqrt(2 corr ln 131072) sigma: the fine Box-Muller lattice of the rotor noise (dsim_device.h:box_muller16; the coarse one ends at 3.535)


_ROTOR_NOISE_MAPS = {}


def hexa_noise_maps(t):
    """Six-actuator types draw the noise of the BODY WRENCH (dsim_device.h:noise_normals): W = L z, z six unit normals, L the Cholesky
    factor of M diag(sigma^2) M^T, M the 6 x 12 map from the per-rotor force / moment noise of BaseAviary.py:1429-1457 to the wrench.
    Returns (L [6,6] as the device holds it, P [12,6]): P z = per-rotor noise values (f[6] in N, m[6] in N m) whose wrench under the
    ORACLE's per-rotor map is L z — what the tests hand to the (unchanged) oracle.  L follows dsim_api.hip:to_dev step by step: M
    from the fp32 images of the rotor axes and of r x a, the factor rounded to fp32 over 0.01."""
    key = (np.asarray(t.rotor_pos, dtype=np.float64).tobytes(), np.asarray(t.rotor_axis, dtype=np.float64).tobytes(),
           np.asarray(t.rotor_spin, dtype=np.float64).tobytes())
    if key in _ROTOR_NOISE_MAPS:
        return _ROTOR_NOISE_MAPS[key]
    r = np.asarray(t.rotor_pos, dtype=np.float64)[:6]
    a = np.asarray(t.rotor_axis, dtype=np.float64)[:6]
    sp = np.asarray(t.rotor_spin, dtype=np.float64)[:6]
    sig = np.array([0.01] * 6 + [0.001] * 6)
    a32, rxa32 = f32(a), f32(np.cross(r, a))
    M32 = np.zeros((6, 12))
    M32[0:3, 0:6], M32[3:6, 0:6], M32[3:6, 6:12] = a32.T, rxa32.T, (sp[:, None] * a32).T
    L = np.linalg.cholesky((M32 * sig) @ (M32 * sig).T)
    L = f32(L / 0.01) * 0.01
    M = np.zeros((6, 12))                                       # the oracle's map: fp64 geometry, actual forces and moments
    M[0:3, 0:6], M[3:6, 0:6], M[3:6, 6:12] = a.T, np.cross(r, a).T, (sp[:, None] * a).T
    S = np.diag(sig ** 2)
    P = S @ M.T @ np.linalg.solve(M @ S @ M.T, L)
    _ROTOR_NOISE_MAPS[key] = (L, P)
    return L, P


def rotor_noise(t, u):
    """(f_noise[n_act], m_noise[n_act]), in N and N m, of one sub-step from the unit normals u = Oracle.noise_normals(...) of the
    launch: quads draw them per rotor (BaseAviary.py:1518-1521); six-actuator types draw the six normals of the body wrench, and the
    per-rotor values returned here add up to exactly that wrench under the oracle's map (hexa_noise_maps)."""
    na = t.n_act
    if na == 4:
        return u[0:4] * 0.01, u[4:8] * 0.001
    n = hexa_noise_maps(t)[1] @ np.asarray(u[0:6], dtype=np.float64)
    return n[0:6], n[6:12]


def noise_terms(types, type_id, n, dt_phys, substeps):
    """([n,13], [n,13]) what the rotor noise adds to the magnitudes of step_terms (BaseAviary.py:1518-1525: f_noise ~ N(0, .01)
    per rotor — and on the lateral axes of every rotor link —, m_noise ~ N(0, .001)): at zero command the noise IS the
    largest term of the velocity and rate updates, and an increment that happens to be small (a draw near zero) must not
    shrink the bar below the rounding of the terms that made it."""
    tr, tm = np.zeros((n, 13)), np.zeros((n, 13))
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    for k, t in enumerate(types):
        s = tid == k
        fmax, mmax = NOISE_MAX_SIGMA * 0.01, NOISE_MAX_SIGMA * 0.001
        arm = np.linalg.norm(np.asarray(t.rotor_pos)[: t.n_act], axis=1)
        tr[s, 7:10] = t.n_act * fmax / t.mass * dt_phys
        tr[s, 10:13] = (t.n_act * mmax + 2.0 * (arm * fmax).sum()) / min(t.inertia) * dt_phys
        if t.n_act == 6:            # the wrench W = L z, |z_j| <= NOISE_MAX_SIGMA: row sums of |L|
            w = np.abs(hexa_noise_maps(t)[0]).sum(1) * NOISE_MAX_SIGMA
            tr[s, 7:10] = w[0:3].max() / t.mass * dt_phys
            tr[s, 10:13] = w[3:6].max() / min(t.inertia) * dt_phys
        tr[s, 0:3] = tr[s, 7:10] * dt_phys * substeps
        tm[s, 0:3], tm[s, 3:6] = tr[s, 7:10], tr[s, 10:13]
    return tr, tm


def tilt_gain(types, type_id, rigid):
    """[n,13] factor on the ulp term of the controller-memory fields: the quad law's pitch increment is
    w.a / (T cos^2(roll)) (INDIControl.py:314-339: det G = T^2 cos(roll)), so the fp32 rounding of cos(roll) reaches
    the attitude set-point, and through it the cmd fields, amplified by 1 / cos^2(roll).  1 for the thrust row and
    for the 6-DOF law (its target attitude is forced to zero, INDIControl_6DOF.py:495)."""
    n = rigid.shape[0]
    g = np.ones((n, 13))
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    q = rigid[:, 3:7]
    ra, rb = 2 * (q[:, 1] * q[:, 2] + q[:, 3] * q[:, 0]), q[:, 3] ** 2 - q[:, 0] ** 2 - q[:, 1] ** 2 + q[:, 2] ** 2
    c2 = rb ** 2 / np.maximum(ra ** 2 + rb ** 2, 1e-300)
    for k, t in enumerate(types):
        if t.kind != 1:                        # the quad law, on four or six actuators
            s = tid == k
            g[s, 7:7 + t.n_act] = (1.0 / np.maximum(c2[s], 1e-8))[:, None]
    return g


TINY = 1e-3     # m, m/s, rad/s, PWM: below k ulp32(1e-3) = k x 1.2e-10 a difference is numerical zero (a drone at rest with
                # zero command has rates of 1e-20 on both sides, from cancelling denormal-sized terms)


def increment_ratio(got, ref, prev, terms, k, part=None):
    """|d_got - d_ref| / (REL_TOL (|d_ref| + part) + k ulp32(max(|prev|, |ref|, terms, TINY))): <= 1 passes.
    part: the magnitude of a PART of the increment that is itself only known to REL_TOL — the contribution of an input
    that comes from another fp32 evaluation, e.g. the neighbour-downwash force (hundreds of exp() terms summed in fp32,
    tests/util.py:assert_downwash): where thrust and gravity cancel, |d_ref| says nothing about its size."""
    d_ref = ref - prev
    M = np.maximum(np.maximum(np.maximum(np.abs(prev), np.abs(ref)), terms), TINY)
    return np.abs(got - ref) / (REL_TOL * (np.abs(d_ref) + (0.0 if part is None else part)) + k * ulp32(M))


WORST = {}     # test label -> worst ratio seen (printed by conftest at the end of the session)
WHERE = {}     # test label -> where that worst ratio sits: block, field, the numbers (so that a thin margin can be traced
               # to the term that produces it; written to DSIM_MARGINS_OUT beside the ratios)
RIGID_NAMES = ["x", "y", "z", "qx", "qy", "qz", "qw", "vx", "vy", "vz", "wx", "wy", "wz"]
MEM_NAMES = ["last_vx", "last_vy", "last_vz", "last_p", "last_q", "last_r", "last_thrust", "cmd0", "cmd1", "cmd2", "cmd3", "cmd4", "cmd5"]


PLANE_SWEEPS = 24       # DSIM_PLANE_ITERS / ORC_PLANE_ITERS


def plane_terms(types, type_id, rigid, dt_ctrl, dt_phys=1.0 / 240.0):
    """DSIM_OPT_PLANE: what the contact solve adds to the magnitudes of step_terms, per drone ([n,13], [n,13]); to be
    used with k = K_ULP x sub-steps x (1 + PLANE_SWEEPS) — one more rounding of the contact terms per sweep.
      - a contact point moves at u = v + w x r, |u| <= |v| + |w| R (R: COM to the rim of the collision cylinder); an
        impulse that changes u by du changes v by at most du and w by at most du / (2 rho) (rho = sqrt(J_min / m): the
        maximum of (l / J) / (1 / m + l^2 / J) over the lever arm l);
      - the target velocity of a point is its gap over dt, gap = z + r_z: operands |z| / dt and R / dt, entering once
        per sub-step, not once per sweep (hence the division: k ulp(M) then charges them K_ULP ulps per sub-step);
      - the controller differentiates the new velocity and rates."""
    n = rigid.shape[0]
    tr = np.zeros((n, 13))
    tm = np.zeros((n, 13))
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    for k, t in enumerate(types):
        s = np.flatnonzero(tid == k)
        R = math.hypot(t.collision_radius, t.collision_below)
        u = np.linalg.norm(rigid[s, 7:10], axis=1) + np.linalg.norm(rigid[s, 10:13], axis=1) * R
        u = u + (np.abs(rigid[s, 2]) + R) / dt_phys / (1 + PLANE_SWEEPS)
        rho = math.sqrt(min(t.inertia) / t.mass)
        tr[s, 7:10] = u[:, None]
        tr[s, 10:13] = (u / (2 * rho))[:, None]
        tr[s, 0:3] = tr[s, 7:10] * dt_phys
        tm[s, 0:3] = tr[s, 7:10]
        tm[s, 3:6] = tr[s, 10:13]
        tm[s, 6] = u / dt_ctrl
        A = np.abs(np.asarray(t.alloc, dtype=np.float64))
        na = t.n_act
        rate = np.max(t.rate_gain) * u / (2 * rho) + u / (2 * rho) / dt_ctrl
        n_out = A.shape[1]
        nu = np.stack([rate] * 3 + [u / dt_ctrl] * (n_out - 3), 1)
        tm[s, 7:7 + na] = nu @ A[:na, :n_out].T
    return tr, tm


def assert_step_parity(label, types, type_id, prev_rigid, prev_mem, tgt, got_rigid, got_mem, ref_rigid, ref_mem,
                       dt_phys, dt_ctrl, substeps, control=True, k=None, action=None, extra_terms=None, part_rigid=None, noise=False,
                       part_mem=None):
    """One step of the HIP path against one step of the oracle from the same (fp32-representable) state,
    judged on the increments (module docstring).  got_mem / ref_mem may be None (physics only); action [n, n_act] =
    the explicit action of this step where it is not the stored cmd.  part_mem [n,13]: like part_rigid, for the controller
    memory itself (control_rounding_part)."""
    k = (K_ULP_NOISE if noise else K_ULP) * max(1, substeps) if k is None else k
    tr, tm = step_terms(types, type_id, prev_rigid, prev_mem, tgt, dt_phys, dt_ctrl, max(1, substeps), control, action)
    if extra_terms is not None:
        tr, tm = tr + extra_terms[0], tm + extra_terms[1]
    rr = increment_ratio(got_rigid, ref_rigid, prev_rigid, tr, k, part_rigid)
    worst = float(rr.max())
    i, f = (int(x) for x in np.unravel_index(rr.argmax(), rr.shape))
    where = ("rigid", i, f)
    detail = dict(field=RIGID_NAMES[f], drone=i, err=float(got_rigid[i, f] - ref_rigid[i, f]), increment=float(ref_rigid[i, f] - prev_rigid[i, f]),
                  value=float(ref_rigid[i, f]), largest_term=float(tr[i, f]), k_ulp=float(k))
    if got_mem is not None:
        kk = k * tilt_gain(types, type_id, ref_rigid)
        # (the controller memory copies the new velocity into last_vel: what is only known to REL_TOL in the velocity — the
        # part of its increment that came from the neighbour-downwash force — is only known to REL_TOL there too)
        part_mem_given, part_mem = part_mem, None
        if part_rigid is not None:
            # ... and the law differentiates it: (v - last_vel) / dt_ctrl is the measured acceleration (INDIControl.py:285-291,
            # INDIControl_6DOF.py:399-413), which goes into the thrust state and, through the allocation, into the commands
            part_mem = np.zeros_like(ref_mem)
            part_mem[:, 0:3] = part_rigid[:, 7:10]
            pa = part_rigid[:, 7:10].sum(1) / dt_ctrl
            part_mem[:, 6] = pa
            tid_ = np.zeros(ref_mem.shape[0], dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
            for k_, t_ in enumerate(types):
                s_ = tid_ == k_
                A_ = np.abs(np.asarray(t_.alloc, dtype=np.float64))
                col = A_[: t_.n_act, 3] if t_.kind != 1 else A_[:6, 3:6].sum(1)
                part_mem[np.ix_(s_, 7 + np.arange(t_.n_act))] = pa[s_, None] * col[None, :]
        if part_mem_given is not None:
            part_mem = part_mem_given if part_mem is None else part_mem + part_mem_given
        rm = increment_ratio(got_mem, ref_mem, prev_mem, tm, kk, part_mem)
        if rm.max() > worst:
            worst = float(rm.max())
            i, f = (int(x) for x in np.unravel_index(rm.argmax(), rm.shape))
            where = ("mem", i, f)
            detail = dict(field=MEM_NAMES[f], drone=i, err=float(got_mem[i, f] - ref_mem[i, f]), increment=float(ref_mem[i, f] - prev_mem[i, f]),
                          value=float(ref_mem[i, f]), largest_term=float(tm[i, f]), k_ulp=float(np.broadcast_to(kk, rm.shape)[i, f]))
    if worst >= WORST.get(label, 0.0):
        detail["ulp32_of_M"] = float(ulp32(max(abs(detail["value"]), abs(detail["value"] - detail["increment"]), detail["largest_term"], TINY)))
        WHERE[label] = detail
    WORST[label] = max(WORST.get(label, 0.0), worst)
    assert worst <= 1.0, (label, worst, where)
    return worst


def control_bound(types, type_id, rigid, prev_mem, tgt, ref_mem, dt_ctrl, k=K_ULP):
    """Per-case tolerance [n,13] of one computeControl call on the controller memory (last_vel3 last_rates3
    last_thrust cmd6): REL_TOL |d_ref| + k ulp32(M), M from step_terms with no physics in front."""
    _, tm = step_terms(types, type_id, rigid, prev_mem, tgt, 0.0, dt_ctrl, 1, True)
    M = np.maximum(np.maximum(np.maximum(np.abs(prev_mem), np.abs(ref_mem)), tm), TINY)
    return REL_TOL * np.abs(ref_mem - prev_mem) + k * tilt_gain(types, type_id, rigid) * ulp32(M)


def assert_control_parity(label, types, type_id, rigid, prev_mem, tgt, got_mem, ref_mem, dt_ctrl, k=K_ULP, slack=None):
    """computeControl on the HIP path against the oracle from the same fp32-representable inputs, judged on the
    increments of the controller memory.  slack [n,13] (optional) is added per case — used against the reference's
    fp64-input goldens, where it is |oracle(fp32-rounded inputs) - golden|, the measured effect of input rounding."""
    tol = control_bound(types, type_id, rigid, prev_mem, tgt, ref_mem, dt_ctrl, k)
    if slack is not None:
        tol = tol + slack
    ratio = np.abs(got_mem - ref_mem) / tol
    worst = float(ratio.max())
    WORST[label] = max(WORST.get(label, 0.0), worst)
    assert worst <= 1.0, (label, worst, tuple(int(x) for x in np.unravel_index(ratio.argmax(), ratio.shape)))
    return worst


ENVELOPES = ("omega_clamp", "vel_clamp", "pi4", "tiny_omega", "non_unit", "tumbling", "wreck")


def random_fleet(rng, n, n_act=4, tilt=0.5, speed=2.0, rate=1.5, spread=50.0, envelope=None):
    """Seeded in-flight fleet state: rigid [n,13], mem [n,13], targets [n,10] (fp32-representable).

    envelope: None = gentle flight (the defaults above), or one of ENVELOPES — the corners of Bullet's floating-base
    step (row P4, BaseAviary.py:542-543) that gentle flight never reaches:
      "omega_clamp"  angular-velocity coordinates at 90-130 rad/s, mixed with lanes that have ONE such coordinate and
                     lanes just under 100 rad/s (applyDeltaVeeMultiDof's clamp of every world coordinate to +-100; the
                     body-frame loop's world-frame detour triggers on |w_b| >= 100)
      "vel_clamp"    velocity coordinates at 95-105 m/s (the same clamp on the linear coordinates; damping pulls the
                     ones under 100 away from it, thrust pushes some onto it)
      "pi4"          |w| up to 170 rad/s in random directions: with dt_phys = 1/100 or 1/60 s the rotation per sub-step
                     exceeds pi/4 and Bullet's angular-motion clamp engages (unreachable at 240 Hz)
      "tiny_omega"   |w| < 1e-3 rad/s, some lanes exactly zero (Bullet's Taylor branch of the exponential map)
      "non_unit"     quaternions of length 0.5-1.5 (the helpers do not normalise; Bullet's step does)
      "tumbling"     attitudes over the whole sphere (tilt to pi), both signs of w
      "wreck"        all of it at once: a tumbling lane with clamped rates and velocities and a non-unit quaternion"""
    assert envelope is None or envelope in ENVELOPES, envelope
    rpy = np.stack([rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n), rng.uniform(-math.pi, math.pi, n)], 1)
    quat = np.stack([orc.quat_from_euler(r) for r in rpy]) if n <= 20000 else _quat_from_euler_np(rpy)
    pos = np.concatenate([rng.uniform(-spread, spread, (n, 2)), rng.uniform(0.5, 20.0, (n, 1))], 1)
    vel = rng.uniform(-speed, speed, (n, 3))
    om = rng.uniform(-rate, rate, (n, 3))
    sign = lambda shape: np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)
    if envelope in ("tumbling", "wreck"):
        quat = rng.normal(size=(n, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    if envelope in ("non_unit", "wreck"):
        quat = quat * rng.uniform(0.5, 1.5, (n, 1))
    if envelope in ("omega_clamp", "wreck"):
        big = sign((n, 3)) * rng.uniform(90.0, 130.0, (n, 3))
        kind = rng.integers(0, 4, n)                      # 0, 1: every coordinate; 2: one coordinate; 3: |w| just under 100
        one = np.zeros((n, 3)); one[np.arange(n), rng.integers(0, 3, n)] = 1.0
        om = np.where((kind <= 1)[:, None], big, np.where((kind == 2)[:, None], one * big + (1 - one) * om, om))
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        om = np.where((kind == 3)[:, None], d * rng.uniform(97.0, 101.0, (n, 1)), om)
    if envelope in ("vel_clamp", "wreck"):
        vel = sign((n, 3)) * rng.uniform(95.0, 105.0, (n, 3))
    if envelope == "pi4":
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        om = d * rng.uniform(40.0, 170.0, (n, 1))          # pi / (4 dt) = 78.5 rad/s at 100 Hz, 47.1 at 60 Hz
    if envelope == "tiny_omega":
        om = rng.uniform(-1.0, 1.0, (n, 3)) * (1e-3 / math.sqrt(3.0)) * rng.uniform(0.0, 1.0, (n, 1))
        om[rng.uniform(size=n) < 0.1] = 0.0
    rigid = f32(np.concatenate([pos, quat, vel, om], 1))
    mem = np.zeros((n, 13))
    mem[:, 0:3] = rigid[:, 7:10] + rng.uniform(-0.02, 0.02, (n, 3))
    mem[:, 3:6] = rng.uniform(-rate, rate, (n, 3))
    mem[:, 6] = rng.uniform(0.0, 1.0, n)
    mem[:, 7:7 + n_act] = rng.uniform(0.3, 0.7, (n, n_act))
    mem = f32(mem)
    tgt = np.concatenate([rigid[:, 0:3] + rng.uniform(-1, 1, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3)),
                          rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-4, 4, (n, 1))], 1)
    return rigid, mem, f32(tgt)


def _quat_from_euler_np(rpy):
    h = rpy / 2.0
    s, c = np.sin(h), np.cos(h)
    q = np.stack([
        s[:, 0] * c[:, 1] * c[:, 2] - c[:, 0] * s[:, 1] * s[:, 2],
        c[:, 0] * s[:, 1] * c[:, 2] + s[:, 0] * c[:, 1] * s[:, 2],
        c[:, 0] * c[:, 1] * s[:, 2] - s[:, 0] * s[:, 1] * c[:, 2],
        c[:, 0] * c[:, 1] * c[:, 2] + s[:, 0] * s[:, 1] * s[:, 2]], 1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def attitude_zoo(rng, n_random=2000):
    """Quaternions (xyzw, fp32-representable) that exercise every branch of p.getEulerFromQuaternion
    (BaseAviary.py:729): random attitudes over the whole sphere, both signs of w, both gimbal branches
    (|sarg| >= 0.99999, exactly +-90 deg pitch and just inside the clamp), attitudes just OUTSIDE the clamp
    (|sarg| a few 1e-6 under 0.99999: the ill-conditioned end of asin), and non-unit quaternions (scaled
    0.5 .. 1.5: the helper does not normalise).  Cases within fp32 rounding of the branch threshold are
    excluded by construction — there Bullet's own function is discontinuous (pitch jumps by 4.5e-3 rad)."""
    out = []
    q = rng.normal(size=(n_random, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    out.append(q)                                                     # w of both signs
    rpy = np.stack([rng.uniform(-math.pi, math.pi, 400), np.zeros(400), rng.uniform(-math.pi, math.pi, 400)], 1)
    s_in = np.concatenate([np.full(100, 1.0), 1.0 - rng.uniform(0, 8e-6, 100)])            # inside the clamp
    s_out = 0.99999 - rng.uniform(3e-6, 5e-5, 200)                                         # just outside
    sarg = np.concatenate([s_in, s_out]) * np.where(rng.uniform(size=400) < 0.5, -1.0, 1.0)
    rpy[:, 1] = np.arcsin(sarg)
    out.append(_quat_from_euler_np(rpy))
    q = rng.normal(size=(400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    out.append(q * rng.uniform(0.5, 1.5, (400, 1)))                   # non-unit
    q = f32(np.concatenate(out))
    sarg = -2.0 * (q[:, 0] * q[:, 2] - q[:, 3] * q[:, 1])
    keep = np.abs(np.abs(sarg) - 0.99999) > 1e-6                      # off the discontinuity
    return q[keep]


# ---------------------------------------------------------------------------------------------------------------------
# neighbour downwash (formula P8): tolerance per receiver
# ---------------------------------------------------------------------------------------------------------------------
FLT_MIN = 1.17549435e-38     # smallest normal fp32: v_exp_f32 flushes what lies below it to zero


def p8_terms(types, type_id, recv_pos, world_pos, cutoff=10.0, chunk=256):
    """Per receiver of formula P8 (BaseAviary.py:1736-1763; oracle/dsim_oracle.c:orc_downwash), in fp64 numpy:
    (n_pairs, largest |term|, straddle, flush) — the number of contributing pairs, the largest single term, the summed
    magnitude of the terms of pairs that sit within 2e-5 m of the cut-off circle or of dz = 0, where the fp32 and the
    fp64 evaluation of `dz > 0 and dxy < 10` may legitimately disagree, and sum(alpha) x FLT_MIN: a term is alpha x
    exp(..), and an exponential below the smallest normal fp32 is flushed to zero by the hardware while fp64 keeps it
    (forces of 1e-30 N: "no force" either way)."""
    recv_pos, world_pos = np.asarray(recv_pos, np.float64), np.asarray(world_pos, np.float64)
    n = recv_pos.shape[0]
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    d0 = np.array([t.dw_coeff[0] for t in types])[tid]; d1 = np.array([t.dw_coeff[1] for t in types])[tid]
    d2 = np.array([t.dw_coeff[2] for t in types])[tid]; pr = np.array([t.prop_radius for t in types])[tid]
    n_pairs, t_max, straddle, flush = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n), np.zeros(n)
    chunk = max(1, min(chunk, (1 << 23) // max(1, world_pos.shape[0])))          # <= 8 M pairs (64 MB per temporary) at a time
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        dz = world_pos[None, :, 2] - recv_pos[s:e, None, 2]
        dxy = np.hypot(world_pos[None, :, 0] - recv_pos[s:e, None, 0], world_pos[None, :, 1] - recv_pos[s:e, None, 1])
        near = (dz > -2e-5) & (dxy < cutoff + 2e-5)
        dzs = np.where(dz > 1e-12, dz, 1.0)
        alpha = d0[s:e, None] * (pr[s:e, None] / (4 * dzs)) ** 2
        term = alpha * np.exp(-0.5 * (dxy / (d1[s:e, None] * dzs + d2[s:e, None])) ** 2)
        hit = (dz > 0) & (dxy < cutoff)
        flush[s:e] = np.where(hit, alpha, 0.0).sum(1) * FLT_MIN
        edge = near & ((np.abs(dxy - cutoff) < 2e-5) | (np.abs(dz) < 2e-5))
        n_pairs[s:e] = hit.sum(1)
        t_max[s:e] = np.where(hit, term, 0.0).max(1)
        straddle[s:e] = np.where(edge & (dz > 1e-12), term, 0.0).sum(1)
    return n_pairs, t_max, straddle, flush


def assert_downwash(label, got, ref, types, type_id, recv_pos, world_pos):
    """|got - ref| <= 1e-4 |ref| + n_pairs ulp32(largest term) (+ what straddles the cut-off, + the flushed exponentials),
    per receiver.  The terms of one receiver all have the same sign, so |ref| is the sum of their magnitudes: the bar
    is relative to what was summed, with no absolute floor that would hide the weak far-field terms."""
    n_pairs, t_max, straddle, flush = p8_terms(types, type_id, recv_pos, world_pos)
    tol = REL_TOL * np.abs(ref) + n_pairs * ulp32(np.maximum(t_max, 1e-300)) * (t_max > 0) + straddle + flush + 1e-300
    ratio = np.abs(np.asarray(got, np.float64) - ref) / tol
    worst = float(ratio.max())
    WORST[label] = max(WORST.get(label, 0.0), worst)
    assert worst <= 1.0, (label, worst, int(ratio.argmax()), float(got[ratio.argmax()]), float(ref[ratio.argmax()]))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the service kernels (dsim_reset, dsim_traj_sample, dsim_adjacency, dsim_fleet_bounds): seeded inputs, built once here for
# tests/test_gpu_service_kernels.py (the device) and tests/test_service_inputs_cpu.py (the properties the device tests rely on)
# ---------------------------------------------------------------------------------------------------------------------
PI32, HPI32 = float(np.float32(math.pi)), float(np.float32(math.pi / 2))       # the fp32 images: what a caller can hand over
# rpy rows every reset fleet starts with (a fleet of one takes the first): +-pi roll and yaw, +-pi/2 pitch (the Euler gimbal
# point), 0, and angles of 1e-4 (sin(h) ~ h: the small end of the half-angle products)
RESET_ANGLE_TABLE = np.array([
    [PI32, HPI32, 1e-4], [0, 0, 0], [0, HPI32, 0], [0, -HPI32, 0], [PI32, 0, 0], [-PI32, 0, 0], [0, 0, PI32], [0, 0, -PI32],
    [1e-4, 1e-4, 1e-4], [1e-4, 0, 0], [0, -1e-4, 0], [0, 0, 1e-4], [-PI32, -HPI32, PI32], [HPI32, 0, HPI32], [PI32, HPI32, -PI32]])
EULER_CLAMP = 0.99999       # p.getEulerFromQuaternion's gimbal threshold on |sin(pitch)| (attitude_zoo): discontinuous there


def reset_inputs(n, mixed, seed=4242):
    """What dsim_reset is handed, fp32-representable: pos [n,3], rpy [n,3] (RESET_ANGLE_TABLE, then a seeded spread over
    (-pi, pi]^3), vel [n,3], cmd [n, 4 or 6] and tid [n] uint8 (mixed: even lanes type 0 = quad, odd lanes type 1 = hexa) or None.
    A spread attitude within 1e-4 of the Euler clamp is redrawn: there the helper the controller calls is discontinuous, and
    the step that follows the reset would compare the two branches (tests/util.py:attitude_zoo)."""
    rng = np.random.default_rng(seed + 7 * n + int(mixed))
    pos = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(0.5, 20.0, (n, 1))], 1)
    rpy = -rng.uniform(-math.pi, math.pi, (n, 3))                         # (-pi, pi]
    for _ in range(100):
        bad = np.abs(np.abs(np.sin(f32(rpy[:, 1]))) - EULER_CLAMP) < 1e-4
        if not bad.any():
            break
        rpy[bad, 1] = -rng.uniform(-math.pi, math.pi, int(bad.sum()))
    k = min(n, len(RESET_ANGLE_TABLE))
    rpy[:k] = RESET_ANGLE_TABLE[:k]
    vel = rng.uniform(-2, 2, (n, 3))
    na = 6 if mixed else 4
    cmd = rng.uniform(0.3, 0.7, (n, na))
    tid = None
    if mixed:
        tid = (np.arange(n) % 2).astype(np.uint8)
        cmd[tid == 0, 4:6] = 0.0                                           # a quad's block holds 0 behind its four actuators
    return dict(pos=f32(pos), rpy=f32(rpy), vel=f32(vel), cmd=f32(cmd), tid=tid)


def reset_expected(types, inp, vel_given, cmd_given):
    """The fp64 definition of reset() (BaseAviary.py:640-714, INDIControl.py:109-146) on reset_inputs: rigid [n,13] with the
    quaternion of orc.quat_from_euler, mem [n,13] = Oracle.reset_mem rounded to fp32, or the given command."""
    n = inp["pos"].shape[0]
    rigid = np.zeros((n, 13))
    rigid[:, 0:3] = inp["pos"]
    rigid[:, 3:7] = np.stack([orc.quat_from_euler(r) for r in inp["rpy"]])
    if vel_given:
        rigid[:, 7:10] = inp["vel"]
    mem = f32(orc.Oracle(types).reset_mem(n, inp["tid"]))
    if cmd_given:
        mem[:, 7:7 + inp["cmd"].shape[1]] = inp["cmd"]
    return rigid, mem


TRAJ_N, TRAJ_SAMPLES, TRAJ_DT, TRAJ_WRAPPERS = 600, 20, 1.0 / 96, 24


def traj_service_fleet(coeffs, TS, n=TRAJ_N, seed=99):
    """Per-drone start times, yaw memories and offsets of the sampler test.  t0: every TS[k] exactly and one fp64 ulp either
    side, TS[-1] + 1e-9, TS[-1] + 5 (the clamp t_end - 0.001), 0, then a seeded spread over [0, TS[-1]).  The last TRAJ_WRAPPERS
    drones start mid-flight where the yaw turns, with the heading the sampler would hold there and a yaw memory placed so that the
    yaw passes +-pi half way through the TRAJ_SAMPLES samples (found with the oracle) or, every other one, passes the other end
    at the first sample; everybody else starts as trajGenerator
    does, with zeros.  Returns t0 [n], yaw_state [3, n], offsets [n, 3] (fp32-representable)."""
    TS = np.asarray(TS, dtype=np.float64)
    rng = np.random.default_rng(seed)
    edge = []
    for tk in TS:
        edge += [tk, np.nextafter(tk, -np.inf), np.nextafter(tk, np.inf)]
    edge += [TS[-1] + 1e-9, TS[-1] + 5.0, 0.0]
    t0 = np.concatenate([edge, rng.uniform(0.0, TS[-1], n - len(edge))])
    ys = np.zeros((3, n))
    span = TRAJ_SAMPLES * TRAJ_DT
    for j, i in enumerate(range(n - TRAJ_WRAPPERS, n)):
        # spread over the flight, away from its ends (there the vehicle is at rest and the heading is rounding noise)
        t0[i] = TS[-1] * (0.1 + 0.8 * j / TRAJ_WRAPPERS)
        y = np.zeros(3)
        orc.traj_sample(coeffs, TS, t0[i] - TRAJ_DT, y)                  # the heading one sample earlier
        h = y.copy()
        y[0] = 0.0
        for k in range(TRAJ_SAMPLES // 2):                               # the turn of the first half of the samples ...
            orc.traj_sample(coeffs, TS, t0[i] + k * TRAJ_DT, y)
        turn = y[0]
        orc.traj_sample(coeffs, TS, t0[i] + (TRAJ_SAMPLES // 2) * TRAJ_DT, y)
        turn = 0.5 * (turn + y[0])                                       # ... and half of the next: +-pi falls BETWEEN two samples
        ys[:, i] = [(math.pi if turn > 0 else -math.pi) - turn, h[1], h[2]]
        if j % 2:
            # this trajectory turns one way only: every other drone remembers a heading half a radian to the right of its course,
            # turns left by that much at its first sample and passes the OTHER end, +pi (or -pi on a left-turning trajectory)
            s_ = -0.5 if turn < 0 else 0.5
            ys[:, i] = [(math.pi if turn < 0 else -math.pi) + 0.5 * s_, h[1] * math.cos(s_) - h[2] * math.sin(s_),
                        h[1] * math.sin(s_) + h[2] * math.cos(s_)]
    assert span > 0
    # (offsets that keep |position| below 16 m: one fp32 ulp there is 9.5e-7 m, under the 2e-6 m bar of the position)
    off = f32(np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.uniform(0, 5, (n, 1))], 1))
    return t0, ys, off


def traj_oracle_run(coeffs, TS, t0, ys0, samples=TRAJ_SAMPLES, dt=TRAJ_DT):
    """The oracle's sampler per drone, advanced as the kernel advances it (t += dt after every sample): rows
    [samples, n, 10], t [samples, n] AFTER the advance, yaw_state [samples, 3, n] after each sample."""
    n = len(t0)
    t, ys = np.array(t0, dtype=np.float64), np.array(ys0, dtype=np.float64)
    rows, tt, yy = np.zeros((samples, n, 10)), np.zeros((samples, n)), np.zeros((samples, 3, n))
    for k in range(samples):
        for i in range(n):
            y = ys[:, i].copy()
            rows[k, i] = orc.traj_sample(coeffs, TS, t[i], y)
            ys[:, i] = y
        t = t + dt
        tt[k], yy[k] = t, ys
    return rows, tt, yy


# ---- adjacency: positions on the 1/8 m lattice below 256 m ----------------------------------------------------------------
# Every coordinate is k / 8 with 0 <= k < 2048, so every difference is k / 8 with |k| < 2048, every square k / 64 with
# k < 2^22 and every three-term sum k / 64 with k < 3 x 2^22 < 2^24: exact in fp32 whichever way the compiler rounds (two
# roundings or a fused multiply-add, any order of the sum).  A numpy brute force in fp32 IS the answer, pair by pair.
ADJ_RADIUS = 7.5
ADJ_EXACT_OFFSETS = np.array([[4.5, 6, 0], [6, 4.5, 0], [0, 4.5, 6], [6, 0, 4.5], [7.5, 0, 0], [0, 7.5, 0], [0, 0, 7.5], [2.5, 5, 5]])
ADJ_NEAR_OFFSETS = np.array([[7.375, 0, 0], [7.625, 0, 0], [0, 7.375, 0], [0, 7.625, 0], [0, 0, 7.375], [0, 0, 7.625]])


def _lattice(rng, n, lo, hi, zhi=16.0):
    """n points on the 1/8 m lattice, x and y in [lo, hi), z in [0, zhi)"""
    return np.concatenate([rng.integers(int(lo * 8), int(hi * 8), (n, 2)), rng.integers(0, int(zhi * 8), (n, 1))], 1) / 8.0


def adjacency_case(name):
    """dict(pos [m,3] float32 — the WORLD —, lo, hi: the receivers are pos[lo:hi], radius, cell, xmin, ymin, nx, ny, max_k).
      strict     cell = radius = 7.5: 100 seeds, each with partners at exactly 7.5 m (ADJ_EXACT_OFFSETS) and at 7.5 -+ 1/8 m
      borders    cell 8: a third of the drones with x or y (or both) a whole multiple of the cell, a grid over the whole box
      middle     the same drones, the grid over [16, 240)^2 only: a quarter of them lie outside and are clamped into border cells
      world      1 500 world entries, the receivers are the middle 500 (pos_all + local_offset)
      one_cell_N N = 1, 2, 65, 700 drones inside ONE cell of a 3 x 3 grid, eight of them (from N = 65) on one point
      overflow   300 drones in one cell (well over 20 neighbours each) and 300 spread thin (fewer than 8), lists of max_k = 8"""
    rng = np.random.default_rng(sum(map(ord, "borders" if name == "middle" else name)))
    c = dict(radius=ADJ_RADIUS, cell=8.0, xmin=0.0, ymin=0.0, nx=32, ny=32, max_k=64)
    if name == "strict":
        seeds = _lattice(rng, 100, 16, 232)
        pos = np.concatenate([seeds] + [seeds + o for o in ADJ_EXACT_OFFSETS] + [seeds + o for o in ADJ_NEAR_OFFSETS])
        c.update(cell=7.5, nx=35, ny=35)
    elif name in ("borders", "middle"):
        pos = _lattice(rng, 2000, 0, 256)
        k = np.arange(2000)
        pos[k % 3 == 0, 0] = np.floor(pos[k % 3 == 0, 0] / 8) * 8
        pos[k % 6 == 0, 1] = np.floor(pos[k % 6 == 0, 1] / 8) * 8
        pos[k % 9 == 1, 1] = np.floor(pos[k % 9 == 1, 1] / 8) * 8
        if name == "middle":
            c.update(xmin=16.0, ymin=16.0, nx=28, ny=28)
    elif name == "world":
        pos = _lattice(rng, 1500, 64, 192)
        c.update(lo=500, hi=1000)
    elif name.startswith("one_cell_"):
        n = int(name.rsplit("_", 1)[1])
        pos = _lattice(rng, n, 8, 16, 8.0)
        if n >= 8:
            pos[10:18] = pos[10] if n > 18 else pos[0]
        c.update(nx=3, ny=3)
    elif name == "overflow":
        pos = np.concatenate([_lattice(rng, 300, 40, 48, 8.0), _lattice(rng, 300, 64, 256)])
        c.update(max_k=8)
    else:
        raise ValueError(name)
    assert pos.min() >= 0 and pos.max() < 256 and np.array_equal(pos * 8, np.round(pos * 8))
    c.setdefault("lo", 0)
    c.setdefault("hi", pos.shape[0])
    c["pos"] = pos.astype(np.float32)
    return c


ADJACENCY_CASES = ("strict", "borders", "middle", "world", "one_cell_1", "one_cell_2", "one_cell_65", "one_cell_700", "overflow")


def adjacency_d2(pos, lo, hi, dtype=np.float32):
    """[hi - lo, m] squared distances receiver x world entry, every operation in `dtype`"""
    p = pos.astype(dtype)
    d = p[lo:hi, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def adjacency_brute(c):
    """The exact answer: bool [receivers, m], True where |p_i - p_j| < radius (strictly) and j is not i itself."""
    nb = adjacency_d2(c["pos"], c["lo"], c["hi"]) < np.float32(c["radius"]) ** 2
    nb[np.arange(c["hi"] - c["lo"]), np.arange(c["lo"], c["hi"])] = False
    return nb


def adjacency_cells(c):
    """The cell index cy nx + cx of every world entry as the kernels compute it (dsim_downwash.hip:dw_cell: fp32, clamped)."""
    inv = np.float32(1.0) / np.float32(c["cell"])
    cx = np.clip(np.floor((c["pos"][:, 0] - np.float32(c["xmin"])) * inv).astype(np.int64), 0, c["nx"] - 1)
    cy = np.clip(np.floor((c["pos"][:, 1] - np.float32(c["ymin"])) * inv).astype(np.int64), 0, c["ny"] - 1)
    return cy * c["nx"] + cx


# ---- fleet bounds ---------------------------------------------------------------------------------------------------------
BOUNDS_KINDS = ("negative", "straddle", "zeros", "magnitudes", "nan_x")
BOUNDS_SIZES = (1, 63, 64, 65, 5000)


def bounds_fleet(kind, n, seed=0):
    """rigid [n,13], mem [n,13] (fp32-representable) for dsim_fleet_bounds.
      negative    x, y in [-900, -1): only the ~u branch of the keys runs; every velocity component negative
      straddle    x, y in [-40, 60)
      zeros       x negative but for one -0.0 and (from n = 3 on) one +0.0: the maximum is a zero of either sign; y positive but
                  for the same two zeros: the minimum is
      magnitudes  |x|, |y| = 10^u, u in [-30, 6), both signs; velocities likewise up to 1e2
      nan_x       straddle with one drone's x NaN (from n = 2 on; fminf / fmaxf drop it)"""
    rng = np.random.default_rng(1000 * BOUNDS_KINDS.index(kind) + n + seed)
    rigid, mem, _ = random_fleet(rng, n)
    sign = lambda k: np.where(rng.uniform(size=k) < 0.5, -1.0, 1.0)
    if kind == "negative":
        rigid[:, 0:2] = -rng.uniform(1, 900, (n, 2))
        rigid[:, 7:10] = -rng.uniform(0.01, 3, (n, 3))
    elif kind in ("straddle", "nan_x"):
        rigid[:, 0:2] = rng.uniform(-40, 60, (n, 2))
        if n >= 2:
            rigid[0, 0:2], rigid[1, 0:2] = (-3.0, 2.0), (4.0, -1.0)      # both signs even in a fleet of two
        if kind == "nan_x" and n >= 2:
            rigid[n // 2, 0] = np.nan
    elif kind == "zeros":
        rigid[:, 0] = -rng.uniform(1, 5, n)
        rigid[:, 1] = rng.uniform(1, 5, n)
        rigid[n // 2, 0:2] = -0.0
        if n >= 3:
            rigid[n // 3, 0:2] = 0.0
    elif kind == "magnitudes":
        rigid[:, 0:2] = sign((n, 2)) * 10.0 ** rng.uniform(-30, 6, (n, 2))
        rigid[:, 7:10] = sign((n, 3)) * 10.0 ** rng.uniform(-30, 2, (n, 3))
    return f32(rigid), mem


def bounds_expected(rigid):
    """numpy's fp32 answer: xmin, ymin, xmax, ymax, max |coordinate velocity| (NaN positions dropped, as fminf / fmaxf do)"""
    r = rigid.astype(np.float32)
    with np.errstate(all="ignore"):
        return np.array([np.nanmin(r[:, 0]), np.nanmin(r[:, 1]), np.nanmax(r[:, 0]), np.nanmax(r[:, 1]), np.abs(r[:, 7:10]).max()],
                        dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# drag (P6) and ground effect (P7) at their edges: seeded inputs, built once here for tests/test_gpu_aero_edges.py (the
# device) and tests/test_aero_inputs_cpu.py (the properties the device tests rely on, and their power)
# ---------------------------------------------------------------------------------------------------------------------
AERO_DELTA = 1e-3                                   # rad: how far the gate cases sit from a threshold of the ground-effect gate
AERO_GATE_ULPS = 16.0                               # ... and the least distance, in fp32 ulps of the operands, the CPU file demands
AERO_PITCH_GATE = math.asin(EULER_CLAMP)            # the pitch at which Bullet's Euler helper switches to its gimbal branch
AERO_GATE_RATE = 5.0                                # rad/s: the gate cases turn away from their threshold at this rate
AERO_CLASSES = ("gate", "height", "drag")
OPT_DRAG, OPT_GROUND = 1, 2                         # DSIM_OPT_DRAG, DSIM_OPT_GROUND


def _aero_pack(rng, rpy, pos, vel, om, cmd_lo=0.3, cmd_hi=0.9, equal_rotors=False):
    """dict(rigid [m,13], mem [m,13], tgt [m,10], act [m,4], prev [m,4]), fp32-representable, from attitudes, positions,
    velocities and rates: commands (stored, explicit and previous) in [cmd_lo, cmd_hi] — no rotor at idle —, targets within a
    metre of the drone."""
    m = len(rpy)
    quat = np.stack([orc.quat_from_euler(r) for r in rpy])
    rigid = f32(np.concatenate([pos, quat, vel, om], 1))
    mem = np.zeros((m, 13))
    mem[:, 0:3] = rigid[:, 7:10]
    mem[:, 6] = rng.uniform(0.2, 0.8, m)
    draw = (lambda: np.repeat(rng.uniform(cmd_lo, cmd_hi, (m, 1)), 4, 1)) if equal_rotors else (lambda: rng.uniform(cmd_lo, cmd_hi, (m, 4)))
    mem[:, 7:11] = draw()
    act, prev = f32(draw()), f32(draw())
    tgt = np.concatenate([rigid[:, 0:3] + rng.uniform(-1, 1, (m, 3)), rng.uniform(-0.5, 0.5, (m, 6)), rng.uniform(-3, 3, (m, 1))], 1)
    return dict(rigid=rigid, mem=f32(mem), tgt=f32(tgt), act=act, prev=prev)


def aero_gate_cases(t, seed=7100):
    """States 0.05-0.3 m above the ground on both sides of every threshold of the ground-effect gate (|roll| < pi/2 and
    |pitch| < pi/2, BaseAviary.py:1648-1699), AERO_DELTA away from it:
      roll  = +-(pi/2 -+ delta)               at pitch 0, +0.7, -0.7
      pitch = +-(asin(0.99999) -+ delta)      at roll 0, +0.5, -0.5  (beyond it Bullet's helper reports |pitch| = pi/2: gate shut)
      roll  = 0, +pi, -pi                     plain members
    each at two yaws.  Cases come in PAIRS that differ in the side of the threshold only (`partner`: the index of the other one;
    the plain members: roll 0 is the partner of +-pi, +pi that of 0) and `open` says on which side a case lies.  The gate is
    evaluated again at every later sub-step, on an attitude the step itself has moved: the four rotors of a drone get ONE
    command (no torque but the ground effect's own) and the body turns at AERO_GATE_RATE AWAY from its threshold — the Euler
    angle in question moves 0.02 rad per sub-step, where one that lingers would sooner or later sit within fp32 rounding of
    the threshold (sin(pitch) moves 4e-6 per milliradian there).  Checked, not assumed: aero_gate_margins along
    aero_substep_starts in tests/test_aero_inputs_cpu.py and in front of every device launch."""
    rng = np.random.default_rng(seed + sum(map(ord, t.name)))
    rpy, is_open, partner, away = [], [], [], []
    for yaw_k in range(2):
        for s in (1.0, -1.0):
            for pitch in (0.0, 0.7, -0.7):
                yaw = rng.uniform(-math.pi, math.pi)
                for d in (-AERO_DELTA, AERO_DELTA):
                    rpy.append([s * (math.pi / 2 + d), pitch, yaw]); is_open.append(d < 0); away.append([s * np.sign(d), 0.0, 0.0])
                partner += [len(rpy) - 1, len(rpy) - 2]
            for roll in (0.0, 0.5, -0.5):
                yaw = rng.uniform(-math.pi, math.pi)
                for d in (-AERO_DELTA, AERO_DELTA):
                    rpy.append([roll, s * (AERO_PITCH_GATE + d), yaw]); is_open.append(d < 0); away.append([0.0, s * np.sign(d), 0.0])
                partner += [len(rpy) - 1, len(rpy) - 2]
        yaw, k = rng.uniform(-math.pi, math.pi), len(rpy)
        rpy += [[0.0, 0.1, yaw], [math.pi, 0.1, yaw], [-math.pi, 0.1, yaw]]; is_open += [True, False, False]
        partner += [k + 1, k, k]
        away += [[0.0] * 3] * 3
    rpy, partner, away = np.array(rpy), np.array(partner), np.array(away)
    m = len(rpy)
    state = rng.uniform(size=(m, 6))
    state = state[np.minimum(np.arange(m), partner)]                   # a pair shares everything but the side
    pos = np.stack([-5 + 10 * state[:, 0], -5 + 10 * state[:, 1], 0.05 + 0.25 * state[:, 2]], 1)
    vel = -1 + 2 * state[:, 3:6]
    # the world-frame angular velocity that moves the Euler angles at `away` x AERO_GATE_RATE: w = 2 (dq / dt) q^-1, by a
    # central difference of the half-angle product (Bullet integrates q <- dq(w dt) q: the increment acts from the left)
    om, h = np.zeros((m, 3)), 1e-6
    for i in range(m):
        q, dq = orc.quat_from_euler(rpy[i]), (orc.quat_from_euler(rpy[i] + h * away[i]) - orc.quat_from_euler(rpy[i] - h * away[i])) / (2 * h)
        qi = np.array([-q[0], -q[1], -q[2], q[3]])
        om[i] = 2 * AERO_GATE_RATE * np.array([dq[3] * qi[0] + dq[0] * qi[3] + dq[1] * qi[2] - dq[2] * qi[1],
                                               dq[3] * qi[1] + dq[1] * qi[3] + dq[2] * qi[0] - dq[0] * qi[2],
                                               dq[3] * qi[2] + dq[2] * qi[3] + dq[0] * qi[1] - dq[1] * qi[0]])
    c = _aero_pack(rng, rpy, pos, vel, om, equal_rotors=True)
    for key in ("mem", "tgt", "act", "prev"):
        c[key] = c[key][np.minimum(np.arange(m), partner)]
    c.update(open=np.array(is_open), partner=partner, rpy=rpy)
    return c


def aero_gate_margins(quat):
    """For quaternions [n,4] as the state block holds them (fp32-representable): (open32, open64, clear, strict).
      open64  the oracle's gate: orc_euler_from_quat, then |roll| < pi/2 and |pitch| < pi/2 (oracle/dsim_oracle.c:orc_ground_effect)
      open32  the kernel's gate restated in fp32 numpy: sarg = -2 (x z - w y), rb = w w - x x - y y + z z,
              |sarg| < 0.99999f and rb > 0 (dsim_device.h:ground_effect_quad)
      strict  | |sarg| - 0.99999 | and |rb| are both at least AERO_GATE_ULPS fp32 ulps of their operands away from zero.  The
              operands are products of two components and their sums, bounded by |q|^2: whichever way the compiler contracts
              or orders the four products (two roundings or fused multiply-adds), the result moves by a few of those ulps.
      clear   the predicate's VALUE cannot flip: strict, or one of the two comparisons is false by that margin (a shut roll
              gate hides the pitch threshold and the reverse) — what a state reached DURING a run is asked for."""
    q64 = np.asarray(quat, dtype=np.float64)
    rpy = np.stack([orc.euler_from_quat(q) for q in q64])
    open64 = (np.abs(rpy[:, 0]) < math.pi / 2) & (np.abs(rpy[:, 1]) < math.pi / 2)
    x, y, z, w = (q64[:, k].astype(np.float32) for k in range(4))
    sarg = np.float32(-2.0) * (x * z - w * y)
    rb = w * w - x * x - y * y + z * z
    open32 = (np.abs(sarg) < np.float32(EULER_CLAMP)) & (rb > np.float32(0.0))
    u = ulp32(np.maximum((q64 ** 2).sum(1), 1.0))
    far_s = np.abs(np.abs(sarg.astype(np.float64)) - EULER_CLAMP) >= AERO_GATE_ULPS * u
    far_r = np.abs(rb.astype(np.float64)) >= AERO_GATE_ULPS * u
    shut_s = far_s & (np.abs(sarg) >= np.float32(EULER_CLAMP))
    shut_r = far_r & (rb <= 0)
    return open32, open64, (far_s & far_r) | shut_s | shut_r, far_s & far_r


def aero_height_cases(t, seed=7200):
    """The per-rotor height clip h_i = max(z + (R r_i)_z, gnd_eff_h_clip) at its edges.  `group`:
      0  z = the clip exactly (its fp32 image)      1  one fp32 ulp above      2  one fp32 ulp below
      3  z = -0.2 (every rotor under the clip)      4  z = 100 (the term is 1e-7 of the thrust: the far end of 1 / h^2)
      5  tilted 0.5-1.2 rad about a random horizontal axis, z placed so that the clip lies between the lowest and the
         highest rotor: some rotors clipped, some not
    Groups 0-4 fly level (any yaw): R's third row is (0, 0, 1) exactly and h_i = z + r_i,z."""
    rng = np.random.default_rng(seed + sum(map(ord, t.name)))
    clip32 = np.float32(t.gnd_eff_h_clip)
    zs = [clip32, np.nextafter(clip32, np.float32(np.inf)), np.nextafter(clip32, np.float32(-np.inf)), np.float32(-0.2), np.float32(100.0)]
    counts = [4, 4, 4, 6, 3]
    group = np.concatenate([np.full(c, g) for g, c in enumerate(counts)] + [np.full(36, 5)])
    m = len(group)
    rpy = np.zeros((m, 3))
    rpy[:, 2] = rng.uniform(-math.pi, math.pi, m)
    tilted = np.flatnonzero(group == 5)
    ang, axis = rng.uniform(0.5, 1.2, len(tilted)), rng.uniform(-math.pi, math.pi, len(tilted))
    rpy[tilted, 0], rpy[tilted, 1] = ang * np.cos(axis) * 0.95, ang * np.sin(axis) * 0.95
    z = np.zeros(m)
    for g, zg in enumerate(zs):
        z[group == g] = float(zg)
    rel = aero_rotor_rel_heights(t, np.stack([f32(orc.quat_from_euler(r)) for r in rpy]))
    lo, hi = rel[tilted].min(1), rel[tilted].max(1)
    z[tilted] = t.gnd_eff_h_clip - (0.5 * (lo + hi) + rng.uniform(-0.25, 0.25, len(tilted)) * (hi - lo))
    pos = np.stack([rng.uniform(-5, 5, m), rng.uniform(-5, 5, m), z], 1)
    c = _aero_pack(rng, rpy, pos, rng.uniform(-1, 1, (m, 3)), rng.uniform(-0.3, 0.3, (m, 3)))
    # the drones 100 m up also carry the out-of-range actions of the set (the echo is clip(action, 0, 1), CtrlAviary.py:258-263)
    c["act"][group == 4, 0], c["act"][group == 4, 2] = np.float32(-0.25), np.float32(1.5)
    c.update(group=group)
    return c


def aero_rotor_rel_heights(t, quat):
    """[n, 4] the height of every rotor above the drone's own z, (R r_i)_z, in fp64 from the given quaternions."""
    out = np.zeros((len(quat), 4))
    r = np.asarray(t.rotor_pos, dtype=np.float64)[:4]
    for i, q in enumerate(np.asarray(quat, dtype=np.float64)):
        out[i] = r @ orc.matrix_from_quat(q)[2]
    return out


AERO_DRAG_SPEEDS = (0.0, 0.5, 5.0, 30.0)


def aero_drag_cases(t, seed=7300):
    """Drag = R (-c sum(2 pi rpm / 60) v) with the PREVIOUS action's rotor speeds on sub-step 0 (BaseAviary.py:531-532, 1705-1732).
    `speed` [m]: |v| = 0 exactly (3 drones), 0.5 (4), 5 (24), 30 m/s (40), in random directions, the body tilted up to 0.8 rad
    at any yaw, 1-5 m up.  `far` [m]: the previous action is a world away from this step's — every rotor at 0.28-0.32 now and
    at 0.9-0.95 before, or, for every third drone at 30 m/s, the other way round (`act_high`); every fifth drone has
    prev == act bit for bit (`far` False): the control group of the previous-action rule.
    (Why not more drones with a LOW previous action, and none of them at 5 m/s: the drag of the 0.75 kg type at 5 m/s with its
    rotors at 0.3 is 4e-5 m/s per sub-step, a few times the 1e-4-relative bar on the thrust's own 0.14 m/s — such a drone
    tells little, whatever the kernel does; tests/test_aero_inputs_cpu.py measures what each drone tells.)"""
    rng = np.random.default_rng(seed + sum(map(ord, t.name)))
    speed = np.concatenate([np.full(c, s) for s, c in zip(AERO_DRAG_SPEEDS, (3, 4, 24, 40))])
    m = len(speed)
    d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rpy = np.stack([rng.uniform(-0.8, 0.8, m), rng.uniform(-0.8, 0.8, m), rng.uniform(-math.pi, math.pi, m)], 1)
    pos = np.stack([rng.uniform(-5, 5, m), rng.uniform(-5, 5, m), rng.uniform(1, 5, m)], 1)
    c = _aero_pack(rng, rpy, pos, d * speed[:, None], rng.uniform(-0.3, 0.3, (m, 3)))
    lo, hi = f32(rng.uniform(0.28, 0.32, (m, 4))), f32(rng.uniform(0.9, 0.95, (m, 4)))
    act_high = (speed == 30.0) & (np.arange(m) % 3 == 0)
    c["act"], c["prev"] = np.where(act_high[:, None], hi, lo), np.where(act_high[:, None], lo, hi)
    c["mem"][:, 7:11] = c["act"]                                  # (the stored command: the action of a call without one)
    far = np.arange(m) % 5 != 4
    c["prev"][~far] = c["act"][~far]
    c.update(speed=speed, far=far, act_high=act_high)
    return c


_AERO_SETS = {}


def aero_sets(t):
    """{class: cases} of one type, built once per session and never modified (callers copy what they change)."""
    if t.name not in _AERO_SETS:
        _AERO_SETS[t.name] = dict(gate=aero_gate_cases(t), height=aero_height_cases(t), drag=aero_drag_cases(t))
    return _AERO_SETS[t.name]


def aero_fleet(types, n):
    """The fleet the device tests fly: dict(rigid, mem, tgt, act, prev [n, .], tid [n] uint8 or None, cls [n] index into
    AERO_CLASSES, case [n] index into that class's set).  One type: the concatenation of its three sets, cycled to n.  Two
    types: interleaved (even drones type 0, odd drones type 1, the caller's order: every tile holds both), and the j-th drone
    of a type takes case (3 j + type) mod m of its type's concatenation — a third of the list, spread over all three sets, so
    that the hundred drones a type has in the smallest fleet still reach every class."""
    cat = []
    for t in types:
        s = aero_sets(t)
        c = {k: np.concatenate([s[cl][k] for cl in AERO_CLASSES]) for k in ("rigid", "mem", "tgt", "act", "prev")}
        c["cls"] = np.concatenate([np.full(len(s[cl]["rigid"]), i) for i, cl in enumerate(AERO_CLASSES)])
        c["case"] = np.concatenate([np.arange(len(s[cl]["rigid"])) for cl in AERO_CLASSES])
        cat.append(c)
    tid = None if len(types) == 1 else (np.arange(n) % len(types)).astype(np.uint8)
    out = {k: np.zeros((n,) + cat[0][k].shape[1:], dtype=cat[0][k].dtype) for k in cat[0]}
    for k_, c in enumerate(cat):
        sel = np.arange(n) if tid is None else np.flatnonzero(tid == k_)
        j = np.arange(len(sel))
        idx = (j if tid is None else 3 * j + k_) % len(c["cls"])
        for key in out:
            out[key][sel] = c[key][idx]
    out["tid"] = tid
    return out


def aero_boost(types, options):
    """The factor the ground effect puts on a rotor's thrust at the height clip, 1 + coeff (r / 4 h_clip)^2 (4 / 15 above one for
    the built-in quads): charged to the roundings of the wrench, K_ULP x sub-steps x boost, as
    tests/test_gpu_parity.py::test_drag_and_ground_effect_vs_oracle does."""
    if not options & OPT_GROUND:
        return 1.0
    return max(1.0 + t.gnd_eff_coeff * (t.prop_radius / (4 * t.gnd_eff_h_clip)) ** 2 for t in types)


def aero_terms(types, type_id, rigid, rpm_cmd, dt_phys, substeps, options, ext_force=None):
    """([n,13], [n,13]) what the add-on forces put among the operands of the velocity update, for step_terms' magnitudes
    (extra_terms of assert_step_parity; nothing here comes from a device result):
      drag        |F| <= max(c) sum_i(2 pi rpm_i / 60) |v|, from the type's constants, the state in front of the step and
                  rpm_cmd [n,4], the LARGER of the previous and the current command per rotor; over the mass, times dt
      ext_force   |F| / m dt of the given body-frame force [n,3]
    Both are single products like the thrusts step_terms sums: they join M, the magnitude whose fp32 ulp the bar counts."""
    n = rigid.shape[0]
    tr, tm = np.zeros((n, 13)), np.zeros((n, 13))
    tid = np.zeros(n, dtype=np.int64) if type_id is None else np.asarray(type_id).astype(np.int64)
    vn = np.linalg.norm(rigid[:, 7:10], axis=1)
    for k, t in enumerate(types):
        s = tid == k
        acc = np.zeros(int(s.sum()))
        if options & OPT_DRAG:
            rpm = np.asarray(t.pwm2rpm_scale)[:4] * np.asarray(rpm_cmd)[s, :4] + np.asarray(t.pwm2rpm_const)[:4]
            acc = acc + max(t.drag_coeff) * (2 * math.pi * rpm / 60).sum(1) * vn[s] / t.mass
        if ext_force is not None:
            acc = acc + np.linalg.norm(ext_force[s], axis=1) / t.mass
        tr[s, 7:10] = (acc * dt_phys)[:, None]
        tr[s, 0:3] = (acc * dt_phys * substeps * dt_phys)[:, None]
        tm[s, 0:3] = tr[s, 7:10]
    return tr, tm


def aero_substep_starts(O, type_id, rigid, mem, substeps, dt, action=None, options=0, last_action=None, ext_force=None):
    """The oracle's Env.step taken one sub-step at a time: (states [substeps, n, 13] at the START of every sub-step, the
    state after the last).  Bit-equal to O.physics(rigid, ..., substeps): that call runs this very loop (orc_physics_batch:
    sub-step 0 with the previous action, the later ones with the current one)."""
    r = rigid.copy()
    starts = []
    last = None if last_action is None else last_action.copy()
    for s_ in range(substeps):
        starts.append(r.copy())
        O.physics(r, mem, 1, dt, action=action, options=options, type_id=type_id, last_action=last if s_ == 0 else None,
                  ext_force=ext_force)
    return np.array(starts), r


def aero_fused_starts(O, type_id, rigid, mem, tgt, substeps, dt, dt_ctrl, options, n_steps, action=None):
    """The oracle's fused loop body (Env.step with the current command's rotor speeds in the drag, then computeControl), n_steps
    times, one sub-step at a time: (states at the start of every sub-step [n_steps x substeps, n, 13], rigid and mem in front of
    the LAST Env.step, rigid and mem after it).  action [n,6]: the explicit action of the first Env.step."""
    r, m = rigid.copy(), mem.copy()
    starts, rp, mp = [], r, m
    for k in range(n_steps):
        rp, mp = r.copy(), m.copy()
        s_, r = aero_substep_starts(O, type_id, r, m, substeps, dt, action=action if k == 0 else None, options=options)
        starts.append(s_)
        assert O.control(r, m, tgt, dt_ctrl, type_id=type_id)[0] == 0
    return np.concatenate(starts), rp, mp, r, m


def aero_power(types, type_id, before, mem, tgt, ref, alt, dt, substeps, options, applied, rpm_cmd, ext_force=None):
    """[n] how many times the bar of the device tests (assert_step_parity with K_ULP x sub-steps x aero_boost and aero_terms)
    a result `alt` lies from the oracle's `ref`, in its worst rigid field: the POWER of that comparison against the fault
    that turns ref into alt."""
    tr, _ = step_terms(types, type_id, before, mem, tgt, dt, dt, substeps, False, applied)
    tr = tr + aero_terms(types, type_id, before, rpm_cmd, dt, substeps, options, ext_force)[0]
    return increment_ratio(alt, ref, before, tr, K_ULP * substeps * aero_boost(types, options)).max(1)


def control_rounding_part(O, type_id, rigid, mem, tgt, dt_ctrl):
    """[n,13] (part_mem of assert_step_parity): how far the oracle's OWN command and thrust state move when one component of the
    quaternion it is given moves by two fp32 ulps, up or down (the largest of the eight moves), over REL_TOL — the construction
    of the neighbour term's sensitivity in tests/test_gpu_two_call_loop.py:_downwash_part.  The quad law reads roll, pitch and yaw
    off the quaternion (INDIControl.py:301: pitch = asin(sarg), roll and yaw = atan2 of terms that vanish with cos(pitch)) and
    builds its attitude target on them: beside the gimbal point a rounding of sarg — the device forms it from four fp32 products —
    is a rounding of the ANGLE 1 / sqrt(1 - sarg^2) times as large (60-130 times for a drone that hovers at sarg = -0.9999, as the
    gate cases of aero_gate_cases do), where the step's bar counts ulps of the terms themselves and tilt_gain knows of
    cos(roll) only.  In gentle flight the eight moves change the command by an ulp or two and the term adds nothing.
    rigid: the state the law evaluates (behind the physics); mem: the controller memory in front of it."""
    base = mem.copy()
    assert O.control(rigid, base, tgt, dt_ctrl, type_id=type_id)[0] == 0
    sens = np.zeros_like(base)
    step = 2.0 * ulp32(np.linalg.norm(rigid[:, 3:7], axis=1))
    for k in range(4):
        for sign in (1.0, -1.0):
            rr, mm = rigid.copy(), mem.copy()
            rr[:, 3 + k] += sign * step
            O.control(rr, mm, tgt, dt_ctrl, type_id=type_id)
            sens = np.maximum(sens, np.abs(mm - base))
    sens[:, 0:6] = 0.0                   # (last_vel is a copy; last_rates = R^T w is charged to its own terms)
    return sens / REL_TOL
