"""Times dsim_trajgen: a bank of --copies copies of the 16 courses of tests/golden/trajgen_courses.npz (65 536 courses by default),
one launch per mode, between device events, behind a warm-up.  Each copy keeps its course's own (max_vel, gamma) only in GIVEN; TMIN
and OPTIMIZE run the whole bank at --max-vel / --gamma, as one launch must.  Prints one JSON line: per mode the median and the
spread of --reps launches in microseconds, and the evaluations of J an OPTIMIZE launch spent.

    python tools/bench_trajgen.py [--lib other/libdronesim_amd.so] [--copies 4096] [--reps 7] [--warmup 2]

--lib: another build of the same ABI (the parent commit's, to compare: run the tool once per library).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--copies", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-vel", type=float, default=2.0)
    ap.add_argument("--gamma", type=float, default=1e3)
    a = ap.parse_args()
    import torch
    from dronesim_amd import _native as nat
    nat.load(a.lib)
    from dronesim_amd import fleet, params
    from tests import trajgen_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajgen needs a HIP device")
    ctx = fleet.Context([params.builtin_type("robobee")])
    courses = R.load_courses(os.path.join(ROOT, "tests", "golden"))
    wps = [c["waypoints"] for c in courses] * a.copies
    given = [c["TS"] for c in courses] * a.copies
    out = {"lib": a.lib or "built", "courses": len(wps), "max_vel": a.max_vel, "gamma": a.gamma}
    for mode, times in (("given", given), ("tmin", "tmin"), ("optimize", "optimize")):
        bank = fleet.TrajectoryBank(ctx, wps, max_vel=a.max_vel, gamma=a.gamma, times=times)      # built once, relaunched below
        need = int(ctx.lib.dsim_trajgen_workspace(bank.K_pad, bank.L_max))
        ws = torch.empty((max(need, 1),), dtype=torch.float64, device=ctx.device)
        ts0 = bank.ts.clone()
        args = nat.TrajGenArgs(wp=bank.wp.data_ptr(), n_wp=bank.n_wp.data_ptr(), max_vel=a.max_vel, gamma=a.gamma, mode=bank.mode,
                               max_evals=2000, cost=bank._cost.data_ptr(), evals=bank._evals.data_ptr(), status=bank._status.data_ptr(),
                               seg_times=bank.seg_times.data_ptr(), workspace=ws.data_ptr(), workspace_len=need)
        us = []
        for rep in range(a.warmup + a.reps):
            bank.ts.copy_(ts0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.check(ctx.lib.dsim_trajgen(ctx.handle, ctx.stream_ptr(), ctypes.byref(bank.c), ctypes.byref(args)))
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                us.append(e0.elapsed_time(e1) * 1e3)
        assert (bank.status == 0).all()
        out[mode + "_us_median"] = round(float(np.median(us)), 1)
        out[mode + "_us_min_max"] = [round(min(us), 1), round(max(us), 1)]
        if mode == "optimize":
            out["optimize_evals_total"] = int(bank.evals.astype(np.int64).sum())
        del bank, ws
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
