"""The bf16 matrix-core 3x3 convolutions (csrc/conv_bf16.hip) through the C ABI under dc_set_matrix_precision(DC_PREC_BF16), at the
edges of their staging and of their tiles, against the rounded-operand fp64 statement of tests/conv_bf16_cases.py: the fused block
(one dc_conv3x3_fwd + one dc_conv3x3_bwd_add per row), the trunk entries (dc_wino3x3_fwd / _dgrad / _dgrad_add / _wgrad) and the
stride-2 entries (dc_convs2_fwd / _wgrad / _dgrad).  The fitness of the rows and route()'s agreement with the library's plans are the
subject of tests/test_conv_bf16_cases_cpu.py; the tables with their reasons, the predicates, the gates and the measured shares are in
DESIGN.md, "The bf16 convolutions at their staging and tile edges".  Every test prints its figures (`conv_bf16_parity ...`) before
it asserts.

Gates (conv_bf16_cases.gate; the project's own for this contract, tests/test_conv_bf16_gpu.py)
    y                 rel-L2 against the rounded-operand fp64 statement < 2e-6
    dx0, dx1, dx, dw  ... < 5e-6; a DW_DIRECT dw (Co < 16) max|hip - fp64| <= 1e-5 max|fp64| against the unrounded statement
    db                within (n + 2) 2^-24 sum|g'| of the sum of the unrounded fp32 g' per channel, n = B H W
Every output and every workspace -- exactly the bytes its query returns -- sits between sentinel guards that must come back intact,
and starts as NaN: every output element must be finite afterwards.  A separate addend must come back bitwise unchanged."""
import pytest
import torch

import conv_block_cases as CC
import conv_bf16_cases as BF

pytestmark = pytest.mark.gpu


def _run(case):
    inp, rnd, unr = BF.reference(case)
    res = BF.launch(case, inp)
    BF.gate(case, res, rnd, unr)
    return res


@pytest.mark.parametrize("case", BF.params(BF.BLOCK))
def test_block(case):
    _run(case)


@pytest.mark.parametrize("case", BF.params(BF.TRUNK))
def test_trunk(case):
    _run(case)


@pytest.mark.parametrize("case", BF.params(BF.S2))
def test_stride2(case):
    _run(case)


@pytest.mark.parametrize("case", BF.params(BF.HEAD_FIRST))
def test_heads_keep_their_fp32_kernels_under_the_policy(case):
    """The head-first rule: fp32 plain-FMA kernels, so the fp32 statement and the fp32 gates of conv_block_cases apply, and the
    results are bitwise those of the same launches under DC_PREC_F32."""
    inp, r64, r32 = CC.reference(case)
    res = BF.launch(case, inp)
    CC.gate(case, res, r64, r32, tag="conv_bf16_parity")
    plain = CC.launch(case, inp)
    for k, v in res.items():
        assert v is None or torch.equal(BF.bits(v), BF.bits(plain[k])), k


@pytest.mark.parametrize("family", sorted(BF.NULL_FAMILIES))
def test_null_patterns_leave_the_other_outputs_alone(family):
    """Each output of a partial-gradient launch against the same output of the all-gradients launch: bitwise equal where route()
    names the same kernels for that output in both launches, within the gate (which _run has applied) either way."""
    base = BF.NULL_FAMILIES[family]
    full, kb = _run(base), BF.output_kernels(base)
    nulls = [c for c in BF.BLOCK_NULLS if c[:10] == base[:10]]
    assert len(nulls) == (6 if base.C1 else 4)
    for c in nulls:
        part, kc = _run(c), BF.output_kernels(c)
        assert torch.equal(BF.bits(part["y"]), BF.bits(full["y"]))
        for g, k in CC.OUTPUTS.items():
            assert (part[k] is not None) == (g in c.grads), (k, c.grads)
            if part[k] is None:
                continue
            same = kc[k] == kb[k]
            equal = torch.equal(BF.bits(part[k]), BF.bits(full[k]))
            print("conv_bf16_nulls %s grads=%s %s: %s, %s" % (family, "".join(c.grads), k, "same kernels" if same else "%s instead of %s" % (kc[k], kb[k]),
                                                             "bitwise equal" if equal else "differs"))
            assert equal or not same, (family, c.grads, k)


@pytest.mark.parametrize("name", sorted(BF.WALK))
def test_two_launches_of_a_walk_are_bitwise_equal(name):
    case = BF.WALK[name]
    inp = BF.reference(case)[0]
    a, b = BF.launch(case, inp), BF.launch(case, inp)
    for k, v in a.items():
        assert v is None or torch.equal(BF.bits(v), BF.bits(b[k])), k


def test_the_policy_is_restored_and_is_what_routes_the_launch():
    from depthcore import _lib
    L = _lib.lib()
    assert L.dc_get_matrix_precision() == BF.PREC_F32
    case = BF.BLOCK[8]
    inp, rnd, unr = BF.reference(case)
    res = BF.launch(case, inp)
    assert L.dc_get_matrix_precision() == BF.PREC_F32
    with pytest.raises(AssertionError):           # a launch that fails inside the policy leaves it restored too
        with BF.bf16_policy():
            assert L.dc_get_matrix_precision() == BF.PREC_BF16
            raise AssertionError
    assert L.dc_get_matrix_precision() == BF.PREC_F32
    plain = CC.launch(case, inp)                  # the same launches outside the policy: the fp32 kernels, unrounded operands
    assert BF.distance(plain["y"], unr["y"], "l2") < BF.Y_GATE < BF.distance(plain["y"], rnd["y"], "l2")
    assert BF.distance(res["y"], rnd["y"], "l2") < BF.Y_GATE < BF.distance(res["y"], unr["y"], "l2")
