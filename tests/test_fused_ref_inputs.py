"""The input conditions of tests/test_gpu_fused_reference.py, checked on the reference alone (no
GPU): the builders of tests/_fused_cases.py assert them, this test runs the builders and states
the figures found.

* accumulator extremes: max |acc - col zpa| over the extreme rows EQUALS the bound of the
  f32-exactness proof (16 515 072 / 16 773 120 just below 2^24; 16 809 984, 26 345 472,
  16 902 144 above), odd and even values within 5 % of it, and 0 .. 34 % of the extreme rows'
  outputs equal lo or hi;
* exact ties: 0.78 % (K = 192) and 0.69 % (K = 768) of the QKV elements, 0.75 % of the PV elements
  are unclipped exact ties, with even and odd floors;
* fused LayerNorm: under 28 % of the outputs clipped at every bit width and zero point;
* fused LayerNorm on residual rows of tests/_ln_cases.py (131 x 192): the conditions of
  tests/test_ln_cases_ref.py hold at this shape (kind a: the sequential mean changes at least 4 of
  64 rows, nothing clipped; b, bm: half at -128, none at 127, every mistake changes at least 4 rows;
  c: mean 0, ties with even and odd floors, both clip bounds reached by under 10 %);
* attention: flat rows (all arguments 0), peaked rows (the runner-up 216.75 behind), and at
  T >= 197 rows with 2 x T arguments within 2 above and 3 x T within 2 below -86.5;
* the int32 algebra of the long attention at the zero-point limits (attn_exact_case): one context
  step is 2^15 int32 units at 577 tokens (0.4 % | 1.2 % of the random heads' context clipped, 145 | 143
  distinct values for "lim+" | "lim-") and 2^16 at 1618 tokens (0.4 %, 126 | 130 distinct values),
  with |acc - z| up to 595 721 919 and 1 670 499 246 < 2^31;
* the softmax denominator's last bit (attn_sum_case): s_p 28 196 | 28 197 f32 steps below or 55 108
  above 1 / 255; the denominator's neighbour changes one P in each row of head 3 and 4112 .. 12 300
  context elements."""
import pytest

import _fused_cases as F


@pytest.mark.parametrize("case", [c for c, _ in F.EXTREME_CASES], ids=lambda c: "-".join(map(str, c)))
def test_extreme_rows_reach_the_bound(case):
    st = F.gemm_case(case)["stats"]
    print(case, st)
    assert st["vmax"] == st["bound"] and st["parities"] == [0, 1]
    assert st["below"] == (case.zpa in (40, 2))
    assert (st["bound"] < 1 << 24) == st["below"]
    assert case.epi == "resid" or st["clipped"] < 0.5


@pytest.mark.parametrize("case", [c for c, _ in F.TIES_CASES], ids=lambda c: "-".join(map(str, c)))
def test_ties_occur(case):
    st = F.gemm_case(case)["stats"]
    print(case, st)
    assert st["tie_share"] >= 0.005 and st["even"] > 0 and st["odd"] > 0
    st = F.pv_ties_case()["stats"]
    print("pv", st)
    assert st["tie_share"] >= 0.005 and st["even"] > 0 and st["odd"] > 0


@pytest.mark.parametrize("case", [c for c, _ in F.LN_CASES], ids=lambda c: "-".join(map(str, c)))
def test_layernorm_outputs_not_all_clipped(case):
    st = F.gemm_case(case)["stats"]
    print(case, st)
    assert st["clipped"] < 0.5


@pytest.mark.parametrize("case", [c for c, _ in F.LN_ROW_CASES], ids=lambda c: "-".join(map(str, c)))
def test_layernorm_row_cases_show_the_last_bits(case):
    """The residual-row cases of the fused LayerNorm (131 rows of 192 columns, the mistakes of
    _ln_cases.ln_restated counted over the first 64): the f32 row equals the residual row (asserted
    by the builder) and the conditions of tests/test_ln_cases_ref.py hold at this shape too."""
    import _ln_cases as L
    d = F.gemm_case(case)["ln_case"]
    st = L.stats(d)
    kind = case.kind[len("rows_"):].rstrip("5")
    if kind == "a":
        n = L.rows_changed(d, "mean_seq")
        print(case, st, n)
        assert st["at_lo"] == 0 and st["at_hi"] == 0 and n >= 4
    elif kind in ("b", "bm"):
        n = {m: L.rows_changed(d, m) for m in L.MISTAKES}
        print(case, st, n)
        assert st["at_lo"] == 0.5 and st["at_hi"] == 0 and st["distinct"] >= 128 and min(n.values()) >= 4
    else:
        even, odd = L.tie_shares(d)
        print(case, st, even, odd)
        assert (d["x"].mean(axis=-1) == 0).all() and 0 < st["at_lo"] < 0.1 and 0 < st["at_hi"] < 0.1
        if not case.kind.endswith("5"):
            assert even >= 0.05 and odd >= 0.05
        else:   # var + eps != var: few ties remain
            assert even > 0 and odd > 0


@pytest.mark.parametrize("case", F.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_softmax_rows_have_the_stated_kinds(case):
    st = F.attn_case(case)["stats"]
    print(case, st)
    if case.T >= 16 and case.bw == 8:
        assert st["peak_gap"] > 104
    if case.T >= 197:
        assert st["straddle"][0] > 0 and st["straddle"][1] > 0


@pytest.mark.parametrize("zset", ["lim+", "lim-"])
@pytest.mark.parametrize("T", F.EXACT_T)
def test_exact_cases_resolve_the_int32_algebra(T, zset):
    st = F.attn_exact_case(T, zset)["stats"]
    print(T, zset, st)
    assert st["clip_share"] < 0.02 and st["distinct"] >= 64
    assert st["e"] == {577: 15, 1618: 16}[T]    # the smallest such step: one less clips 2 % or more
    assert st["acc_absmax"] < 1 << 31
    assert st["peak_gap"] > 104 and st["straddle"][0] > 0 and st["straddle"][1] > 0


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("T", F.SUM_T)
def test_sum_cases_show_the_denominators_last_bit(T, sign):
    st = F.attn_sum_case(T, sign)["stats"]
    print(T, sign, st)
    assert st["p_changed"] >= T and st["ctx_changed"] >= T and abs(st["s_p_steps"]) <= 200000
