"""The cases of tests/poison_cases.py against their own conditions, from the reference alone (no GPU).

For every case the reference runs in float64 and in fp32 on every poisoned input the GPU test launches.  Asserted:

  * dep = ~isfinite(reference) is the set the graph gives (`dep_graph`: the rows with an edge from the poisoned rows, the pairs
    and scores that name them): the reference itself is local, in both precisions;
  * at least four dependent rows (pairs, scores; elements in the row-local families) - except in the "nobody" variants, where
    dep is empty or the poisoned row's own output;
  * clean covers at least half of the output;
  * where a case has rows of neighbours: one clean row is empty and one is shorter than the padding unit of four;
  * the fp32 reference passes `check` against its own zeroed run: clean elements bit for bit, the non-finite set, NaN for NaN.
"""
import pytest
import torch

import poison_cases as pc


def conditions(case, dep, what):
    assert torch.equal(dep, case.dep_graph), "{}: the reference's non-finite set is not the graph's ({} against {} elements)".format(
        what, int(dep.sum()), int(case.dep_graph.sum()))
    units = dep if case.unit != "row" else dep.any(dim=-1)
    if case.unit == "row":
        assert torch.equal(dep, units[..., None].expand_as(dep)), what + ": a dependent row has finite columns"
    count = int(units.sum())
    if case.nobody:
        assert count <= len(case.rows), "{}: {} dependent {}s where nobody names the row".format(what, count, case.unit)
    else:
        assert count >= 4, "{}: only {} dependent {}s".format(what, count, case.unit)
    assert 2 * int(dep.sum()) <= dep.numel(), "{}: {} of {} elements are dependent".format(what, int(dep.sum()), dep.numel())
    if case.lengths is not None:
        clean_rows = ~dep.any(dim=-1)
        assert clean_rows.shape == case.lengths.shape, what
        assert bool((clean_rows & (case.lengths == 0)).any()), what + ": no clean row is empty"
        assert bool((clean_rows & (case.lengths > 0) & (case.lengths < pc.PAD_UNIT)).any()), what + ": no clean row is shorter than the padding unit"


@pytest.mark.parametrize("family", list(pc.FAMILIES))
def test_reference_meets_the_contract_and_the_case_conditions(family):
    cases = pc.FAMILIES[family]()
    assert cases
    for case in cases:
        zeroed = {}
        for poison, flags in case.variants:
            what = "{} [{}{}]".format(case.name, poison, "".join(" " + k for k in flags))
            tensors = pc.poisoned(case, poison)
            ref64 = case.ref(tensors, torch.float64, **flags)
            conditions(case, ~torch.isfinite(ref64), what)
            key = tuple(sorted(flags))
            if key not in zeroed:
                zeroed[key] = case.ref(pc.poisoned(case, 0.0), torch.float32, **flags)
                assert bool(torch.isfinite(zeroed[key]).all()), what + ": the zeroed run is not finite"
            ref32 = case.ref(tensors, torch.float32, **flags)
            assert torch.equal(~torch.isfinite(ref32), case.dep_graph), what + ": fp32 reference"
            pc.check(ref32, zeroed[key], ref64, what + " (fp32 reference)", nan=poison in pc.NAN_POISONS)


def test_low_half_nan_is_a_nan_with_an_empty_high_half():
    case = pc.gather_case("bf16_wave", "row0")
    row = pc.overwrite(case, "low nan")["x"][0]
    assert bool(torch.isnan(row).all()) and bool((row.view(torch.int32) == 0x7F800001).all())
    assert bool((row.view(torch.int32) >> 16 == 0x7F80).all())                    # (truncated to bf16 it would read +Inf)
    assert torch.equal(case.tensors["x"], pc.gather_case("bf16_wave", "row0").tensors["x"]) and bool(torch.isfinite(case.tensors["x"]).all())


def test_check_rejects_the_failures_it_is_there_for():
    ref = torch.tensor([[1.0, 2.0], [float("nan"), float("nan")], [3.0, 4.0]], dtype=torch.float64)
    out_0 = torch.tensor([[1.0, 2.0], [0.0, 0.0], [3.0, 4.0]])
    good = ref.float()
    pc.check(good, out_0, ref, "good")
    for bad, word in ((torch.tensor([[1.0, 2.0], [0.0, 0.0], [3.0, 4.0]]), "dependent elements are finite"),            # a ReLU that drops NaN
                      (torch.tensor([[1.0, 2.0], [float("nan")] * 2, [float("nan"), 4.0]]), "clean elements are not finite"),   # 0 * NaN in a padded slot
                      (torch.tensor([[1.0, 2.5], [float("nan")] * 2, [3.0, 4.0]]), "differ from the zeroed launch"),
                      (torch.tensor([[1.0, 2.0], [float("inf")] * 2, [3.0, 4.0]]), "are infinite")):
        with pytest.raises(AssertionError, match=word):
            pc.check(bad, out_0, ref, "bad")
