"""The figures behind the tolerances of tests/test_gpu_shoot.py (profiles/shoot_tests.txt), one block per case family.

  python tools/shoot_errors.py [--device]

Without a GPU, over exactly the cases of tests/shoot_cases.py: the largest difference between the float64 and the np.longdouble
run of the numpy restatement (tests/np_shoot.py) on the extremals, relative to max(1, |value|); the largest difference between
the float64 restatement and the oracle's go_shoot on p0 and X; the tolerances derived from them (100 x, rounded up to a power of
ten); what the oracle does with every member of the straggler batches.  With --device: the device's errors beside them -- X, U and
resid against the longdouble extremal from the device's own p0, p0 after one Newton step against the restatement and the oracle --
and the stragglers the device itself counts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import shoot_cases as SC  # noqa: E402
import test_shoot_cpu as TC  # noqa: E402


def main():
    device = "--device" in sys.argv
    if device:
        import test_gpu_shoot as TG
    print("roll-out (max_newton = 0, ftol = 1e300): float64 against longdouble, the oracle against longdouble" + (", the device against longdouble" if device else ""))
    for case in SC.ROLLOUT:
        inp = SC.rollout(case)
        fin = np.flatnonzero(np.isfinite(inp.p0).all(axis=1))
        Xld, Uld = SC.extremal(inp, inp.p0, np.longdouble)
        ora = SC.oracle_shoot(inp)
        eo = max(max(SC.rel_err(ora[b]["X"], Xld[b]), SC.rel_err(ora[b]["U"], Uld[b])) for b in fin)
        line = f"  {SC.case_id(case):28s} {TC.rollout_figure(case):.2e}  {eo:.2e}"
        if device:
            line += f"  {TG.certify(inp, TG.rollout_on_device(case)):.2e}"
        print(line, flush=True)
    print("one Newton step (max_newton = 1, ftol = 1e-3, B = 8): conditioned problems; float64 against longdouble on the :Optimal extremals;"
          " float64 restatement against the oracle, p0 and X" + ("; device: p0 against restatement and oracle, certificate" if device else ""))
    for case in SC.ONE_STEP:
        inp, ora, r64, rld, cond = TC.cpu_sides("one_step", case)
        fx, fp, fX, _ = TC.newton_figures("one_step", case)
        line = f"  {SC.case_id(case):28s} {int(cond.sum())} of 8  {fx:.2e}  {fp:.2e}  {fX:.2e}"
        if device:
            s = TG.solver(inp)
            r = TG.shoot(s, inp)
            s.close()
            ep = max(SC.rel_inf(r["p0"][b], ref[b]["p0"]) for b in np.flatnonzero(cond) for ref in (ora, r64))
            line += f"  {ep:.2e}  {TG.certify(inp, r):.2e}"
        print(line, flush=True)
    for model in (SC.DUB, SC.MAN):
        S = SC.STRAGGLERS[model]
        inp, ora, r64, rld, cond = TC.cpu_sides("stragglers", model)
        early, late_ok, late_no = TC.classes(model)
        fx, fp, fX, left = TC.newton_figures("stragglers", model)
        print(f"stragglers {SC.NAME[model]}: N = {S['N']}, substeps = {S['substeps']}, ftol = {S['ftol']:g}, B = {len(ora)}; oracle: "
              f"{len(late_ok) + len(late_no)} with more than 8 steps, {len(late_ok)} of them converge; left out of the newton_iters comparison: {left}")
        for b, (pb, sc) in enumerate(S["members"]):
            o = ora[b]
            print(f"  problem {pb:2d} x {sc:4g}: status {o['status']} newton_iters {o['newton_iters']:3d} resid {o['resid']:.3e}"
                  f"   float64 {r64[b]['newton_iters']:3d}  longdouble {rld[b]['newton_iters']:3d}")
        print(f"  float64 against longdouble on the :Optimal extremals {fx:.2e}; float64 restatement against the oracle: p0 {fp:.2e}, X {fX:.2e}")
        if device:
            two, one = TG.stragglers_on_device(model)
            late = two["newton_iters"] > SC.SHOOT_CAP
            print(f"  device: {int(late.sum())} with more than 8 steps, {int((two['status'][late] == 1).sum())} of them converge; newton_iters "
                  f"{two['newton_iters'].tolist()}; certificate {TG.certify(inp, two):.2e}", flush=True)
    for model in (SC.DUB, SC.MAN):
        fx, fp = TC.model_figures(model)
        print(f"{SC.NAME[model]}: float64 against longdouble {fx:.3e} -> TOL_X {SC.tol_from(fx):.0e}; restatement against oracle, p0 after one step "
              f"{fp:.3e} -> TOL_P0 {SC.tol_from(fp):.0e}")


if __name__ == "__main__":
    main()
