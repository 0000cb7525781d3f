"""The arguments that gusto_set_problems_multistart, gusto_set_problems_trajlib, gusto_set_problems_roadmap and
gusto_tfsearch_begin share (csrc/seed.hpp: query_args_host), without a GPU: the pure check is compiled into a host program
(tests/c/seed_args.cpp) and held against the rule of include/gusto_hip.h -- K in 1 .. the entry's limit, Bq >= 1 with
Bq K <= batch_cap, no null array, refused in that order."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
K_TEXT = "who: K outside 1 .. LIMIT"
BQ_TEXT = "who: need Bq >= 1 and Bq K <= batch_cap"
NULL_TEXT = "who: a null array"
INT_MAX = 2 ** 31 - 1


def test_query_arguments_of_the_seeding_stages(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "seed_args")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip",
                           os.path.join(ROOT, "tests", "c", "seed_args.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    ok = (0, "")
    # (Bq, K, k_max, batch_cap, null_mask) -> (code, text)
    cases = [
        ((2, 0, 8, 64, 0), (ERR_ARG, K_TEXT)),             # K at 0
        ((2, 1, 8, 64, 0), ok),                            # ... at 1
        ((2, 8, 8, 64, 0), ok),                            # ... at the limit
        ((2, 9, 8, 64, 0), (ERR_ARG, K_TEXT)),             # ... one above it
        ((2, -1, 8, 64, 0), (ERR_ARG, K_TEXT)),
        ((0, 4, 8, 64, 0), (ERR_ARG, BQ_TEXT)),            # Bq at 0
        ((-3, 4, 8, 64, 0), (ERR_ARG, BQ_TEXT)),
        ((16, 4, 8, 64, 0), ok),                           # Bq K at batch_cap
        ((13, 5, 8, 64, 0), (ERR_ARG, BQ_TEXT)),           # ... at batch_cap + 1
        ((1, 1, 1, 1, 0), ok),                             # the smallest call there is
        ((INT_MAX, 64, 64, INT_MAX, 0), (ERR_ARG, BQ_TEXT)),      # Bq K overflows an int (2^37): not wrapped into range
        ((2 ** 30, 4, 64, INT_MAX, 0), (ERR_ARG, BQ_TEXT)),       # Bq K = 2^32 wraps to 0 in an int
        ((2 ** 29, 4, 64, INT_MAX, 0), (ERR_ARG, BQ_TEXT)),       # Bq K = 2^31 wraps to INT_MIN
        ((INT_MAX, 1, 64, INT_MAX, 0), ok),                # the largest product an int holds
    ]
    cases += [((2, 4, 8, 64, 1 << i), (ERR_ARG, NULL_TEXT)) for i in range(4)]    # each array null in turn
    cases += [
        ((2, 4, 8, 64, 15), (ERR_ARG, NULL_TEXT)),
        # which refusal comes first when two apply: K, then Bq, then the arrays
        ((0, 0, 8, 64, 15), (ERR_ARG, K_TEXT)),
        ((0, 9, 8, 64, 0), (ERR_ARG, K_TEXT)),
        ((100, 9, 8, 64, 1), (ERR_ARG, K_TEXT)),
        ((0, 4, 8, 64, 15), (ERR_ARG, BQ_TEXT)),
        ((17, 4, 8, 64, 2), (ERR_ARG, BQ_TEXT)),
    ]
    args = [",".join(str(v) for v in c) for c, _ in cases]
    out = json.loads(subprocess.check_output([exe] + args).decode())
    assert len(out) == len(cases)
    for (c, (rc, text)), r in zip(cases, out):
        assert (r["rc"], r["err"]) == (rc, text), (c, r)
