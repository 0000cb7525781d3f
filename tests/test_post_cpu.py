"""The Nstep rule that gusto_verify, gusto_interpolate and gusto_tvlqr share (csrc/post.hpp), without a GPU: the pure resolver is
compiled into a host program (tests/c/nstep_rule.cpp) and held against ceil(tf / (N - 1) / dt_min) computed here."""
import json
import math
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _expect(N, dt_min, nstep, cap, tf):
    """(accepted, nstep_max or the index of the first problem refused), by the rule of include/gusto_hip.h: never clamped"""
    if nstep > 0:
        return nstep <= cap, nstep
    worst = 0
    for b, t in enumerate(tf):
        q = t / (N - 1) / dt_min
        if not (math.isfinite(q) and 1 <= math.ceil(q) <= cap):
            return False, b
        worst = max(worst, math.ceil(q))
    return True, worst


def test_nstep_rule_of_the_post_solve_stages(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "nstep_rule")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip",
                           os.path.join(ROOT, "tests", "c", "nstep_rule.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    nan, tiny = float("nan"), 1e-320   # (tf / 2 / 1e-320 overflows: q = inf)
    # (N, dt_min, nstep, nstep_cap, tf): N = 3 and dt_min = 0.25 make q = 2 tf exactly
    cases = [
        (3, 0.25, 8, 8, [1.0, 50.0]),            # fixed nstep at the cap (tf plays no part)
        (3, 0.25, 9, 8, [1.0]),                  # ... one above it
        (3, 0.25, 0, 8, [1.0, 4.0, 2.0]),        # a problem exactly at nstep_cap
        (3, 0.25, 0, 8, [1.0, 4.0, 4.1, 9.0]),   # q = 9 = nstep_cap + 1 at problem 2 (problem 3 is worse, and later)
        (3, 0.25, 0, 8, [1.0, 0.0]),             # tf = 0: q = 0
        (3, 0.25, 0, 8, [nan, 1.0]),             # tf = NaN
        (3, tiny, 0, 64, [1.0, 1.0, 1.0]),       # q = inf
        (50, 0.1, 0, 64, [97.0, 200.0, 10.0, 150.0]),   # a mixed batch: 20, 41, 3, 31 substeps
        (50, 0.1, 0, 64, [0.3]),                 # q = 1, the smallest count there is
        (3, 0.25, 0, 8, [-1.0]),                 # tf < 0: q = -2
    ]
    bad_opts = [(3, d, 0, 8, [1.0]) for d in (0.0, -0.1, nan)] + [(3, 0.25, -1, 8, [1.0]), (3, 0.25, 0, 0, [1.0]), (3, 0.25, 2, 0, [1.0])]
    args = [",".join(repr(float(v)) if isinstance(v, float) else str(v) for v in (N, d, ns, cap, *tf)) for N, d, ns, cap, tf in cases + bad_opts]
    out = json.loads(subprocess.check_output([exe] + args).decode())
    assert len(out) == len(cases) + len(bad_opts)
    seen = []
    for (N, d, ns, cap, tf), r in zip(cases, out):
        ok, v = _expect(N, d, ns, cap, tf)
        seen.append(ok)
        assert r["opts_ok"], (N, d, ns, cap)
        if ok:
            assert (r["rc"], r["nstep_max"], r["err"]) == (0, v, ""), (tf, r)
        elif ns > 0:
            assert r["rc"] == ERR_ARG and r["err"] == "who: nstep above nstep_cap", r
        else:   # the refusal names the first problem outside 1 .. nstep_cap
            assert r["rc"] == ERR_ARG and r["err"].startswith("who: problem %d needs " % v) and "substeps" in r["err"], (tf, r)
    assert seen == [True, False, True, False, False, False, False, True, True, False]   # (the cases are what their comments say)
    assert out[2]["nstep_max"] == 8 and out[7]["nstep_max"] == 41
    # nstep = 0 without a positive dt_min, a negative nstep, no room under the cap: the caller's "bad options", before the rule
    for c, r in zip(bad_opts, out[len(cases):]):
        assert r == {"opts_ok": False}, (c, r)
    # a fixed nstep does not need dt_min
    assert json.loads(subprocess.check_output([exe, "3,0.0,2,8,1.0"]).decode()) == [{"opts_ok": True, "rc": 0, "nstep_max": 2, "err": ""}]
