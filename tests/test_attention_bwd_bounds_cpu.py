"""CPU self-check of the attention backward parity references (tests/attention_bwd_ref.py) on the reduced list, one case per group: well-posed inputs, the fp32
emulation inside half of the fp32 part of every bound and inside the slope threshold, every mutant caught.  The whole list: python tools/attention_bwd_bounds.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import attention_bwd_bounds as T   # noqa: E402
import attention_bwd_ref as A      # noqa: E402


def test_case_counts_and_reduced_list():
    assert {g: len(A.ids_of(g)) for g in A.N_CASES} == A.N_CASES == {"packed": 7, "uniform": 12, "hd": 57, "hdq1": 24, "image": 10}
    assert len(A.all_cases()) == 110
    assert sorted(A.case(i).group for i in A.REDUCED) == sorted(A.N_CASES)          # one case per group
    assert {A.case(i).form for i in A.REDUCED} == {"true", "stored"}
    assert A.PACKED_KLENS.count(1) == 2          # two utterances with one valid key, under dropout in the p > 0 packed cases
    for c in A.all_cases():
        assert c.B <= 8 and c.H in (2, 3, 12) and all(0 <= k <= r for k, r in zip(c.klens, c.rows))


def test_reduced_list_emulation_inside_half_bounds_and_every_mutant_caught():
    failures, margins = T.run(list(A.REDUCED), quiet=True)
    assert not failures, failures
    assert set(margins) == set(A.MUTANTS + A.SLOPE_MUTANTS + A.IMAGE_MUTANTS)
    for mut in A.SLOPE_MUTANTS:
        assert margins[mut][1] > 1.0, (mut, margins[mut])
    for mut in A.MUTANTS + A.IMAGE_MUTANTS:
        assert margins[mut][0] > 1.0, (mut, margins[mut])


def test_single_kept_key_bound_holds_only_the_fp32_terms():
    n = 0
    for cid in ("hd96-L65-p0.1", "hd64-L1-p0.1", "hdq1-hd128-Tk65-p0.1"):
        c = A.case(cid)
        n += A.single_key_check(c, A.case_reference(c))
    assert n >= 3
