"""Child process of tests/test_conv_block_shapes_gpu.py::test_direct_kernels_with_winograd_disabled (its own process: the library
reads DC_CONV_WINO once).  With DC_CONV_WINO=0 neither the Winograd launches nor the head kernels run: every table case of
tests/conv_block_cases.py whose route changes goes through the direct implicit GEMMs -- conv_gemm_v2_kernel<MR, false> among
them, which no launch below 2 GiB reaches otherwise -- the forward and the all-gradients backward, against the fp64 statement at
the direct kernels' 1e-5.  Prints one `conv_block_direct <case> ...` line per case and `conv_block_direct_done <n>`; exits non-zero
at the first failure and launches nothing after it."""
import os
import sys
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "self-supervised-depth-estimation_amd"), os.path.join(REPO, "tests")]


def main():
    if os.environ.get("DC_CONV_WINO") != "0":
        print("conv_block_direct_child: DC_CONV_WINO=0 is not set")
        return 2
    import conv_block_cases as CC
    L = CC.host_lib()
    cases = CC.direct_child_cases()
    differs = 0
    for c in cases:
        r = CC.route(c, False)
        try:
            # the library's own view of the switch: its workspace queries are those of the Winograd-free layout
            fw, bw = L.dc_conv3x3_fwd_workspace(c.C0, c.C1, c.B, c.Co, c.H, c.W), L.dc_conv3x3_bwd_workspace(c.C0, c.C1, c.B, c.Co, c.H, c.W)
            assert (fw, bw) == (CC.fwd_workspace(c, False), CC.bwd_workspace(c, False)), "the library did not read DC_CONV_WINO=0"
            differs += bw != CC.bwd_workspace(c, True)
            assert all(CC.tol(r[k]) == CC.DIRECT_TOL for k in ("fwd", "dx", "dw"))
            inp, r64, r32 = CC.reference(c)
            CC.gate(c, CC.launch(c, inp), r64, r32, wino_enabled=False, tag="conv_block_direct")
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            print("conv_block_direct_failed %s" % CC.case_id(c))
            return 1
        sys.stdout.flush()
    if not differs:
        print("conv_block_direct_child: no case tells the Winograd-free workspace layout from the default one")
        return 1
    print("conv_block_direct_done %d" % len(cases))
    return 0


if __name__ == "__main__":
    sys.exit(main())
