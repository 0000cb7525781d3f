"""The fleet stage on config 2's 4096 table queries taken as fleets of 8 and of 16 (profiles/fleet.txt): conflicts of the
uncoordinated plans, SCHEDULED / BLOCKED / NO_PLAN counts with and without parking keep-outs, delays and makespans for
delay_stride 5, 10, 20, and the three stage times beside the solve and the gusto_interpolate of the same batch (two warm-up
calls, then REPS timed ones: median, min, max).

    python tools/fleet_rate.py [B]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gusto_jl_amd as g  # noqa: E402

WARM, REPS = 2, 10


def spread(v):
    v = np.asarray(v)
    return f"median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f}"


def timed(call, read):
    for _ in range(WARM):
        call()
    out = []
    for _ in range(REPS):
        call()
        out.append(read())
    return np.array(out)


def study(s, R, tag):
    B = s.B
    st = s.status()
    ok = st["converged"] & st["successful"]
    rep0 = s.fleet_separation(R, delay_steps=np.where(ok, 0, -1).astype(np.int32))
    print(f"[{tag} R={R}] plans ok {int(ok.sum())}/{B}; uncoordinated: fleets with a conflict {int((rep0['n_conflicts'] > 0).sum())}/{B // R}, "
          f"conflicting pairs {int(rep0['n_conflicts'].sum())} of {B // R * R * (R - 1) // 2}, smallest separation {rep0['fleet_min_sep'].min():.4f}")
    for stride in (5, 10, 20):
        r = s.fleet_schedule(R, delay_stride=stride)
        n = [int((r["status"] == k).sum()) for k in (1, 2, 0)]
        d = r["delay"][r["status"] == 1]
        print(f"[{tag} R={R} stride={stride}] SCHEDULED {n[0]} BLOCKED {n[1]} NO_PLAN {n[2]}; conflicts after {int(r['n_conflicts'].sum())}; "
              f"delay [s] median {np.median(d):.1f} p90 {np.percentile(d, 90):.1f} max {d.max():.1f}; "
              f"makespan [steps] median {np.median(r['makespan_steps']):.0f} max {r['makespan_steps'].max()}")
    ms = timed(lambda: s.fleet_schedule(R), lambda: np.append(s.fleet_info()["stage_ms"], s.last_fleet_ms()))
    for i, k in enumerate(("track", "schedule", "separation", "whole call")):
        print(f"[{tag} R={R}] {k} ms: {spread(ms[:, i])}")


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    P = g.problems
    x0, lo, hi, tf = P.freeflyer_batch(B)
    boxes = P.freeflyer_env()
    sp, mp = g.default_params(0)
    s = g.BatchSolver(0, 50, B, hist_cap=136, boxes=boxes, scp_params=sp, model_params=mp)

    def solve():
        s.set_problems(x0, lo, hi, tf)
        s.solve(30)

    print(f"solve ms: {spread(timed(solve, s.last_solve_ms))}")
    print(f"interpolate ms: {spread(timed(lambda: s.L.gusto_interpolate(s.h, None, None, None, None), s.last_verify_ms))}")
    for R in (8, 16):
        study(s, R, "shared table")
    off = np.array([list(mp.comp_off[c]) for c in range(mp.n_robot_comp)])
    for R in (8, 16):
        park, skipped = g.host.fleet_park_spheres(x0[:, :2], lo[:, :2], R, mp.radius, mp.clearance, off, [len(boxes)] * B)
        s.set_env_batch([boxes] * B, park)
        solve()
        s.L.gusto_interpolate(s.h, None, None, None, None)
        print(f"[parking R={R}] spheres per robot {np.mean([len(p) for p in park]):.1f}, skipped {len(skipped)} (own start or goal inside)")
        study(s, R, "parking")
    s.close()


if __name__ == "__main__":
    main()
