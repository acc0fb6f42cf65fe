"""Host restatements of streamed calibration (numpy_quant/calibration.py): keys, bins, edges
and the range rule against the sort-based reference of _calib_ref.py, bit for bit.  No GPU."""
import os
import re

import numpy as np
import pytest

import _calib_ref as R
from conftest import ROOT
from numpy_quant import calibration as C
from numpy_quant import kernels as K

PERCENTILES = [100, 99.99, 99.9, 99, 90, 50.5]


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "nqk.h")).read()
    defs = dict(re.findall(r"#define (NQK_HIST_[A-Z_]+) (\d+)\b", text))
    assert int(defs["NQK_HIST_SHIFT"]) == C.HIST_SHIFT == K.HIST_SHIFT == 18
    assert int(defs["NQK_HIST_BINS"]) == C.HIST_BINS == K.HIST_BINS == 16384
    assert int(defs["NQK_HIST_DIRECT_MAX"]) == K.HIST_DIRECT_MAX
    assert re.search(r"#define NQK_HIST_MAX_N \(\(int64_t\)1 << 40\)", text) and K.HIST_MAX_N == 1 << 40


def test_float_key_is_strictly_increasing_over_the_ladder():
    assert np.all(np.diff(R.LADDER.astype(np.float64)[[0, 1, 2, 3, 5, 6, 7, 8, 9, 10]]) > 0)  # the ladder is sorted
    k = C.float_key(R.LADDER)
    assert k.dtype == np.uint32
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    np.testing.assert_array_equal(k, R.key(R.LADDER))
    assert int(C.float_key(np.float32(-0.0))) + 1 == int(C.float_key(np.float32(0.0)))


def test_quoted_bins_and_edges():
    b = lambda v: int(C.float_key(np.float32(v))) >> C.HIST_SHIFT  # noqa: E731
    assert b(1.0) == 12256
    lo, hi = C.bin_edges(12256)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert lo == np.float32(1.0) and hi == np.nextafter(np.float32(1.03125), np.float32(0))
    assert R.bits(hi) == R.bits(np.float32(1.0)) + 0x3FFFF
    assert (b(-0.0), b(0.0)) == (8191, 8192)
    assert (b(-np.inf), b(np.inf)) == (31, 16352)


def test_float_key_round_trips_through_bin_edges():
    rng = np.random.default_rng(0)
    x = np.concatenate([R.LADDER, (rng.standard_normal(4000) * 10.0 ** rng.integers(-30, 30, 4000)).astype(np.float32)])
    k = C.float_key(x)
    bins = (k >> np.uint32(C.HIST_SHIFT)).astype(np.int64)
    lo, hi = C.bin_edges(bins)
    klo, khi = C.float_key(lo), C.float_key(hi)
    np.testing.assert_array_equal(klo, (bins << C.HIST_SHIFT).astype(np.uint32))
    np.testing.assert_array_equal(khi, ((bins << C.HIST_SHIFT) | 0x3FFFF).astype(np.uint32))
    assert np.all((klo <= k) & (k <= khi))
    np.testing.assert_array_equal(C.key_float(k).view(np.uint32), x.view(np.uint32))
    # all bins: the edges tile the key space in order
    lo, hi = C.bin_edges(np.arange(C.HIST_BINS))
    np.testing.assert_array_equal(C.float_key(hi).astype(np.int64) + 1, np.append(C.float_key(lo)[1:].astype(np.int64), 1 << 32))
    with pytest.raises(ValueError):
        C.bin_edges(C.HIST_BINS)


def _arrays():
    rng = np.random.default_rng(2026)
    sizes = [1, 2, 3, 5, 17, 100, 101, 999, 1000, 2500, 5000]
    out = []
    for i in range(66):
        n = sizes[i % len(sizes)] if i < 22 else int(rng.integers(1, 5001))
        scale = 10.0 ** rng.uniform(-3, 3)
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        kind = i % 3
        if kind == 1:
            x[rng.integers(0, n)] = np.float32(1e6)
        elif kind == 2:
            x = np.abs(x)
        out.append(x)
    out.append(np.zeros(300, np.float32))
    out.append(np.array([-0.0, 0.0] * 50, np.float32))
    out.append(np.full(77, -2.5, np.float32))
    return out


def test_host_state_is_bincount():
    for x in _arrays()[:12]:
        np.testing.assert_array_equal(C.host_state(x), R.state(x))
        np.testing.assert_array_equal(C.host_state(x, counts=False), R.state(x, counts=False))


@pytest.mark.parametrize("percentile", PERCENTILES)
def test_ranges_from_state_equals_the_sort_reference(percentile):
    for i, x in enumerate(_arrays()):
        vmin, vmax = C.ranges_from_state(R.state(x), percentile)
        wmin, wmax = R.sort_ranges(x, percentile)
        assert isinstance(vmin, np.float32) and isinstance(vmax, np.float32)
        assert (R.bits(vmin), R.bits(vmax)) == (R.bits(wmin), R.bits(wmax)), (i, x.size, percentile)
        assert vmin <= vmax
        if percentile == 100:
            assert (R.bits(vmin), R.bits(vmax)) == (R.bits(R.unkey(R.key(x).min())), R.bits(R.unkey(R.key(x).max())))
            assert vmin == x.min() and vmax == x.max()
            # the range entries alone are enough
            got = C.ranges_from_state(R.state(x, counts=False), 100)
            assert (R.bits(got[0]), R.bits(got[1])) == (R.bits(vmin), R.bits(vmax))


def test_clipping_drops_the_outlier():
    x = np.random.default_rng(1).standard_normal(2000).astype(np.float32)
    x[5] = 1e6
    assert C.ranges_from_state(R.state(x), 100)[1] == np.float32(1e6)
    vmin, vmax = C.ranges_from_state(R.state(x), 99)
    assert vmax < 4 and vmin > -4


@pytest.mark.parametrize("nan", [np.float32(np.nan), -np.float32(np.nan)])
@pytest.mark.parametrize("percentile", [100, 99])
def test_nan_gives_nan(nan, percentile):
    x = np.random.default_rng(3).standard_normal(500).astype(np.float32)
    x[123] = nan
    vmin, vmax = C.ranges_from_state(R.state(x), percentile)
    assert np.isnan(vmin) and np.isnan(vmax)
    x[123] = np.inf  # an infinity is a number
    x[7] = -np.inf
    assert C.ranges_from_state(R.state(x), 100) == (-np.inf, np.inf)


def test_empty_state_raises():
    fresh = R.state(np.zeros(0, np.float32))
    np.testing.assert_array_equal(fresh, C.fresh_state())
    for p in (100, 99):
        with pytest.raises(ValueError, match="fc1.weight"):
            C.ranges_from_state(fresh, p, name="fc1.weight")
    # a range without counts cannot be clipped
    with pytest.raises(ValueError):
        C.ranges_from_state(R.state(np.ones(4, np.float32), counts=False), 99)


@pytest.mark.parametrize("bad", [50, 100.1, "99", 0, -1, float("nan"), None, True])
def test_bad_percentile_raises(bad):
    state = R.state(np.ones(4, np.float32))
    with pytest.raises(ValueError):
        C.ranges_from_state(state, bad)
    with pytest.raises(ValueError):
        C.Calibrator(percentile=bad)
    from numpy_quant.model import Model
    model = Model([], [], [], [])

    def batches():
        raise AssertionError("the iterable is not touched before the arguments are checked")
        yield

    with pytest.raises(ValueError):
        model.calibrate_stream(batches(), percentile=bad)
    with pytest.raises(ValueError):
        model.quantize_stream(batches(), percentile=bad)
