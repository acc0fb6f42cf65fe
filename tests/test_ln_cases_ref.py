"""The input conditions of tests/test_gpu_ln_reference.py, checked on the reference alone (no
GPU).  Figures found (67 rows, the mistakes counted over the first 64):

* every case: ln_restated() without a mistake gives the reference's bytes;
* a (ill-conditioned rows): the mean summed left to right changes a byte in 15 .. 57 of 64 rows at
  every width from 8 up (below 8 columns NumPy's sum is itself sequential: nothing to see, no
  condition); no byte is clipped; 128 .. 230 distinct values (217 and more from 768 columns up);
* b, bm (one-ulp-resolving rows): exactly half the bytes at -128, none at 127, 199 .. 211 distinct
  values; rows changed by the mistakes mean_seq 8 .. 21, var_seq 22 .. 60, inv_ulp 50 .. 64,
  inv_f64 8 .. 35, fma 33 .. 64, regroup 24 .. 64;
* c (exact ties, 192 / 384 / 768 columns): every row's mean is 0; with eps = 1e-12 21 .. 24 % of the
  elements are ties with an even floor and 20 .. 24 % with an odd one, 3.7 .. 9.2 % of the outputs at
  either clip bound (at 96 columns one bound would pass 10 %: the kind runs at the tree widths).  With
  eps = 1e-5 var + eps != var, y is inexact and only 3 .. 4 % + 3 .. 4 % ties remain at the small zero
  points (held to "some of each"); at |zp| >= 2^20 beta ~ 2^16 swallows the inexactness (y is
  rounded to multiples of 2^-7) and 18 .. 25 % of each remain;
* d (parameter edges, widths from 96 up): at most 17 % on either bound and all 2^bw values at bit
  widths 2 .. 4, 196 and more at 8.  One bit has only the two bounds (16 % | 84 %: both must occur);
  below 96 columns a row has too few values for the counts (1 column: y = beta) and the case is
  held to the reference alone."""
import numpy as np
import pytest

import _ln_cases as C


def _all(kinds):
    """The cases of `kinds` that the GPU tests run: every kind at the tree widths, all but c at the others."""
    cases = [c for cols in C.TREE_COLS for c in C.cases_for(cols, kinds)]
    cases += [c for cols in C.GENERIC_COLS for c in C.cases_for(cols, kinds.replace("c", ""))]
    return [pytest.param(c, id=C.case_id(c)) for c in cases]


@pytest.mark.parametrize("case", _all("abcde"))
def test_restatement_equals_the_reference(case):
    d = C.ln_case(case)
    assert C.rows_changed(d, None, first=case.rows) == 0


@pytest.mark.parametrize("case", _all("a"))
def test_ill_conditioned_rows_show_the_means_tree(case):
    d = C.ln_case(case)
    st = C.stats(d)
    n = C.rows_changed(d, "mean_seq")
    print(case, st, "mean_seq", n)
    assert st["at_lo"] == 0 and st["at_hi"] == 0
    if case.cols >= 8:   # (n < 8: NumPy's pairwise sum is the sequential one)
        assert n >= 4
    if case.cols >= 768:   # the rows span +-3.5 / 0.031 = +-113 steps: most of 227 values occur
        assert st["distinct"] >= 215


@pytest.mark.parametrize("case", _all("b"))
def test_one_ulp_rows_show_every_mistake(case):
    d = C.ln_case(case)
    st = C.stats(d)
    n = {m: C.rows_changed(d, m) for m in C.MISTAKES}
    print(case, st, n)
    assert st["at_lo"] == 0.5 and st["at_hi"] == 0 and st["distinct"] >= 128
    assert min(n.values()) >= 4, n


@pytest.mark.parametrize("case", _all("c"))
def test_tie_rows_are_ties(case):
    d = C.ln_case(case)
    st = C.stats(d)
    even, odd = C.tie_shares(d)
    print(case, st, even, odd)
    assert (d["x"].mean(axis=-1) == 0).all()
    if case.eps == 1e-12 or abs(d["zp"]) >= C.P20:
        assert even >= 0.05 and odd >= 0.05
    else:   # var + eps != var: y is inexact and few ties remain (see the docstring)
        assert even > 0 and odd > 0
    assert 0 < st["at_lo"] < 0.1 and 0 < st["at_hi"] < 0.1


@pytest.mark.parametrize("case", _all("d"))
def test_parameter_edges_are_not_all_clipped(case):
    d = C.ln_case(case)
    st = C.stats(d)
    print(case, C.D_PARAMS[case.var], st)
    if case.cols < 96:
        return   # too few values per row for the counts below: held to the reference alone
    if d["bw"] == 1:   # both values are clip bounds
        assert st["at_lo"] >= 0.1 and st["at_hi"] >= 0.1
        return
    assert st["at_lo"] <= 0.2 and st["at_hi"] <= 0.2
    if d["bw"] >= 3:
        assert st["distinct"] >= 2 ** (d["bw"] - 1)


def test_degenerate_and_non_finite_cases():
    d = C.ln_case(C.L("e", 768, C.E_ROWS, 1e-12))
    x = d["x"]
    assert (x[0] == 0).all() and np.signbit(x[1]).all() and (x[5] == 0).all()
    assert np.abs(x[4]).min() >= 5e17 and np.abs(x[6]).max() <= 1.5e-18   # one wave: rows 4 .. 7
    ref = d["ref"].astype(np.int64)
    for r in (0, 1, 2, 3, 5):   # var = 0: y = beta
        np.testing.assert_array_equal(ref[r], C.O.quantize(d["beta"], 8, d["scale"], np.int64(d["zp"])))
    assert (ref[10] != ref[0]).any()   # the row that 1 / sqrt(eps) = 1e6 scales
    f = C.ln_case(C.L("f", 768, 67, 1e-12))
    assert f["finite"].sum() == 63 and not f["finite"][[1, 2, 6, 9]].any()
