"""Child process of tests/test_convs2_shapes_gpu.py::test_gather_kernels_with_the_fast_paths_disabled and (argument `plan`) of
tests/test_convs2_cases_cpu.py::test_plan_agrees_with_route_under_the_switches -- its own process: the library reads DC_STEM_PATCH,
DC_CONV_TRIP and DC_STEM_X3 once.

Without an argument (GPU): DC_STEM_PATCH=0 DC_CONV_TRIP=0 must be set.  The triple-gather and stem rows of tests/convs2_cases.py then
go through the general gather kernels -- cg_fwd_kernel<.,.,3> with Kp == K and cg_wgrad_kernel<2,2,7> at Co = 64 among them, which
no launch reaches otherwise -- forward, weight gradient and data gradient against the fp64 statement at the same 1e-5.  It first
checks through dc_convs2_plan_query that the library read the switches.  Prints one `convs2_gather <row> ...` line per row and
`convs2_gather_done <n>`; exits non-zero at the first failure and launches nothing after it.

`plan` (no GPU, starts none): under whatever switches the environment sets, plan and workspaces of every row, split mode and entry
against route(row, mode, env).  Prints one `convs2_plan <row> ...` line per row and `convs2_plan_done <n>`."""
import os
import sys
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "self-supervised-depth-estimation_amd"), os.path.join(REPO, "tests")]

SWITCHES = ("DC_STEM_PATCH", "DC_CONV_TRIP", "DC_STEM_X3")


def plan_main():
    import convs2_cases as S
    env = {k: os.environ[k] for k in SWITCHES if k in os.environ}
    for c in S.CASES:
        stem = S.route(c, 1, env)["stem"]
        for mode in (0, 1, 3):
            for raw in (0,) + (S.raw_modes(c) if stem else ()):
                bad = S.plan_mismatches(c, mode, env, raw)
                if bad:
                    print("convs2_plan_failed %s mode %d raw %d: (field, library, route) %s" % (S.case_id(c), mode, raw, bad))
                    return 1
        if c.Ci in (3, 6) and c.Co == 64 and c.k == 7 and not stem and S.plan_query(c, raw=1)[0] != S.EINVAL:
            print("convs2_plan_failed %s: dc_stem_* would run with the patch-staged stem switched off" % S.case_id(c))
            return 1
        with S.split_mode(1):
            got = S.plan_query(c)[1]
        print("convs2_plan %s %s%s" % (S.case_id(c), " ".join("%s=%d" % kv for kv in got.items()),
                                       " differs" if got != S.plan_of(S.route(c)) else ""))
    print("convs2_plan_done %d" % len(S.CASES))
    return 0


def main():
    if len(sys.argv) > 1:
        return plan_main() if sys.argv[1:] == ["plan"] else 2
    if any(os.environ.get(k) != "0" for k in ("DC_STEM_PATCH", "DC_CONV_TRIP")):
        print("convs2_gather_child: DC_STEM_PATCH=0 DC_CONV_TRIP=0 is not set")
        return 2
    import convs2_cases as S
    cases = S.gather_child_cases()
    for c in cases:
        r = S.route(c, 1, S.GATHER_ENV)
        try:
            # the library's own view of the switches
            assert S.plan_mismatches(c, 1, S.GATHER_ENV) == [] and S.plan_query(c)[1] != S.plan_of(S.route(c)), \
                "the library did not read DC_STEM_PATCH=0 DC_CONV_TRIP=0"
            assert r["fwd"] == "gather" and r["dw"] == "gather"
            inp, r64, r32 = S.reference(c)
            with S.split_mode(1):
                res = S.launch(c, inp, S.outputs(c))
            errs = S.gate(c, res, r64, r32, tag="convs2_gather_parity")
            print("convs2_gather %s %s | %s" % (S.case_id(c), " ".join("%s %.2e" % kv for kv in errs.items()), S.describe(r)))
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            print("convs2_gather_failed %s" % S.case_id(c))
            return 1
        sys.stdout.flush()
    print("convs2_gather_done %d" % len(cases))
    return 0


if __name__ == "__main__":
    sys.exit(main())
