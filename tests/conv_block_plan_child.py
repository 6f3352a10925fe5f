"""Child process of tests/test_conv_block_cases_cpu.py::test_plan_agrees_with_route_with_winograd_disabled (its own process: the
library reads DC_CONV_WINO once).  With DC_CONV_WINO=0 the plan the launches follow (dc_conv3x3_plan_query) must name, field by
field, what route(case, False) names for every case of conv_block_cases.direct_child_cases(): the direct implicit GEMMs
everywhere, conv_gemm_v2_kernel<MR, false> among them.  Needs no GPU and starts none.  Prints one `conv_block_plan <case> ...`
line per case and `conv_block_plan_done <n>`; exits non-zero at the first disagreement."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "self-supervised-depth-estimation_amd"), os.path.join(REPO, "tests")]


def main():
    if os.environ.get("DC_CONV_WINO") != "0":
        print("conv_block_plan_child: DC_CONV_WINO=0 is not set")
        return 2
    import conv_block_cases as CC
    cases = CC.direct_child_cases()
    for c in cases:
        bad = CC.plan_mismatches(c, wino_enabled=False)
        rc, got = CC.plan_query(c)
        print("conv_block_plan %-58s %s" % (CC.case_id(c), " ".join("%s=%d" % kv for kv in got.items())))
        if bad or rc != 0:
            print("conv_block_plan_failed %s: (field, library, route) %s" % (CC.case_id(c), bad))
            return 1
        if got["fwd"] != CC.FWD_DIRECT or got["dx"] != CC.DX_DIRECT_FOLD or got["dw"] != CC.DW_DIRECT:
            print("conv_block_plan_failed %s: the library did not read DC_CONV_WINO=0" % CC.case_id(c))
            return 1
    print("conv_block_plan_done %d" % len(cases))
    return 0


if __name__ == "__main__":
    sys.exit(main())
