"""Child process of tests/test_wino_split_shapes_gpu.py::test_forced_plans (its own process, so that no other test ever sees a
forced plan).  DC_WINO_FORCE = "mr,nr,ks" is read per launch: every case of wino_split_cases.FORCED sets its own and goes through
the launch and the gates of the parent's tests -- the 9-chunk reduction over 4 slabs, whose empty slab begins exactly at nchunks,
and the splits on the 32 x 64 tile variant, which the cost model picks for no shape.  Prints the `wino_split_forced <case> ...`
lines and `wino_split_forced_done <n>`; exits non-zero at the first failure and launches nothing after it."""
import os
import sys
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "self-supervised-depth-estimation_amd"), os.path.join(REPO, "tests")]


def main():
    if not os.environ.get("DC_WINO_FORCE"):
        print("wino_split_forced_child: DC_WINO_FORCE is not set")
        return 2
    import wino_split_cases as WS
    for c in WS.FORCED:
        os.environ["DC_WINO_FORCE"] = c.force
        try:
            # the library's own view of the variable: the forced split takes the epilogue away
            assert WS.mech(c)["ksplit"] > 1 and WS.parts_query(c) == 0, "the library did not read DC_WINO_FORCE=%s" % c.force
            inp = WS.reference(c)[0]
            out, ws = WS.launch(c, inp)
            WS.gate(c, inp, out, ws, tag="wino_split_forced")
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            print("wino_split_forced_failed %s" % WS.case_id(c))
            return 1
        sys.stdout.flush()
    print("wino_split_forced_done %d" % len(WS.FORCED))
    return 0


if __name__ == "__main__":
    sys.exit(main())
