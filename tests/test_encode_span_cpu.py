"""The span form of the two-stage encode on the CPU (quantv2x_amd/encode_two_stage.py: ``span_classes``, ``span_rule``): a listed cell of
class (first, last) -- the first and the last level stage 1 could not decide -- goes through the fp32 chain from ``first`` to ``last`` only;
if the chain reproduces the candidates there it keeps the STORED codes behind ``last``, else it runs on to the end.  The rule must give the
oracle's indices (``Oracle.encode_rows``, the reference-order fp32 chain) on EVERY row: on the reference's golden rows, on the codebook with
duplicated and nearly duplicated codewords, and on every hostile family of tests/_encode_families.py -- rows where the candidate differs
from the oracle at an undecided level included (they must continue).  The HIP kernels are held to the same rule in
tests/test_hip_encode_span.py."""
import numpy as np
import pytest

from test_codebook_full_golden import _state, golden_rows
from test_encode_two_stage_cpu import _families, _family, _levels_kc, adversarial_state


def check_rule(state, tabs, rows_u8, in_delta, in_zx, name):
    """the rule on ``rows_u8``: equal to the oracle everywhere.  Returns (first, last, cls, exited, work, work_before, cand, want)."""
    import _encode_families as F
    from oracle.spec import Oracle
    from quantv2x_amd.encode_two_stage import SPAN_CLASSES, candidate_emulate, span_classes, span_rule
    cand, flagged, flags, _ = candidate_emulate(rows_u8, tabs, float(in_delta), int(in_zx))
    want = Oracle(state).encode_rows(F.dequantized(rows_u8, float(in_delta), int(in_zx)))
    first, last, cls = span_classes(flags)
    assert np.array_equal(first >= 0, flagged) and np.array_equal(cls >= 0, flagged) and (last >= first).all()
    got, exited, work, before = span_rule(cand, flags, want)
    bad = int((got != want).sum())
    hist = {f"{f}-{e}": int((cls == k).sum()) for k, (f, e) in enumerate(SPAN_CLASSES)}
    moved = flagged & (cand != want).any(0)
    print(f"span rule [{name}]: {len(flagged)} rows, listed {int(flagged.sum())}, classes (first-last) {hist}, continued "
          f"{int((flagged & ~exited).sum())}, candidate != oracle on {int(moved.sum())} listed rows, work {work:.1f} of {before:.1f} units"
          + (f" = {work / before:.3f}" if before else ""))
    assert bad == 0, f"[{name}] the span rule leaves {bad} indices that are not the oracle's"
    return first, last, cls, exited, work, before, cand, want


def test_golden_rows_the_rule_is_the_oracle_and_saves_a_quarter(golden):
    from quantv2x_amd.encode_two_stage import candidate_tables
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    state = _state()
    levels, _ = _levels_kc(state)
    tabs = candidate_tables(state, levels, float(g["in_delta"]), int(g["in_zp"]))
    first, last, cls, exited, work, before, cand, want = check_rule(state, tabs, codes_u8, g["in_delta"], g["in_zp"], "reference golden rows")
    # the sample holds cells whose candidate is NOT the fp32 chain's index at an undecided level: they continue, and still end as the oracle
    span_differs = np.array([(cand[first[r]:last[r] + 1, r] != want[first[r]:last[r] + 1, r]).any() for r in np.flatnonzero(first >= 0)])
    assert span_differs.sum() >= 1 and not exited[np.flatnonzero(first >= 0)[span_differs]].any()
    ratio = work / before
    print(f"span rule: executed products on the golden rows {ratio:.3f} of the first pair's")
    assert ratio <= 0.80                                                # (measured 0.738: most cells are undecided at ONE level)


def test_duplicated_and_nearly_duplicated_codewords(golden):
    from quantv2x_amd.encode_two_stage import candidate_tables
    g = golden["codebook_full"]
    codes_u8, _ = golden_rows(g)
    st = adversarial_state(_state())
    tabs = candidate_tables(st, 3, float(g["in_delta"]), int(g["in_zp"]))
    first, last, cls, exited, *_ , cand, want = check_rule(st, tabs, codes_u8[::4], g["in_delta"], g["in_zp"], "duplicated / nearly duplicated codewords")
    listed = first >= 0
    print("cells that continue:", int((listed & ~exited).sum()))
    assert (listed & ~exited).sum() >= 1                               # the eps 1e-5 duplicates: candidates the chain does not reproduce


@pytest.mark.parametrize("name", _families())
def test_every_family(golden, name):
    import _encode_families as F
    fam, tabs = _family(name, golden)
    codes_u8, _ = golden_rows(golden["codebook_full"])
    rows, _ = F.hostile_rows(codes_u8, tabs, fam.in_zx)
    check_rule(fam.state, tabs, rows, fam.in_delta, fam.in_zx, fam.name)


def test_classes_and_cost_are_the_kernels():
    """the list order (dearest class first) and the class of every (first, last): what csrc/codebook_encode.h states"""
    from quantv2x_amd.encode_two_stage import SPAN_CLASSES, span_classes, span_cost
    cost = [span_cost(f, e) for f, e in SPAN_CLASSES]
    assert cost == [9.5, 8.0, 6.5, 6.0, 4.5, 2.5] and cost == sorted(cost, reverse=True)
    flags = np.array([[1, 0, 0, 1, 0, 1, 0], [0, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 1, 1, 0]], bool)      # columns: 0-0 1-1 2-2 0-2 1-2 0-2 none
    first, last, cls = span_classes(flags)
    assert first.tolist() == [0, 1, 2, 0, 1, 0, -1] and last.tolist() == [0, 1, 2, 2, 2, 2, -1] and cls.tolist() == [5, 4, 2, 0, 1, 0, -1]
    two = np.array([[1, 0], [0, 0], [0, 1], [0, 0]], bool)               # two segments: a level is undecided if any of its segments is
    first, last, cls = span_classes(two, segs=2)
    assert (first.tolist(), last.tolist(), cls.tolist()) == ([0, 1], [0, 1], [5, 4])
