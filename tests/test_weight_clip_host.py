"""The weight clipping search without a GPU: the restatement (tests/_clip_ref.py) against a
brute-force float64 loop, and the arguments the host side refuses before it touches the device."""
import numpy as np
import pytest

import _clip_ref as R


def test_restatement_equals_a_brute_force_loop():
    """5 x 3, 4 bits: with five rows the stated order of the sum is ((r0 + r4) + r2) + (r1 + r3)."""
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 3)).astype(np.float32)
    s0 = (2 * np.maximum(w.max(axis=0), 0) / np.float32(15)).astype(np.float32)
    ratio = R.ratios(8)
    assert ratio.dtype == np.float32 and ratio[0] == 1 and np.array_equal(ratio, np.float32(1) - np.arange(8) / np.float32(16))
    scale, index, err = R.search_cols(w, s0, ratio, 4)
    for n in range(3):
        want = []
        for g in range(8):
            s = np.float32(s0[n] * ratio[g])
            sq = []
            for k in range(5):
                q = float(np.rint(min(max(np.float32(w[k, n] / s), np.float32(-8)), np.float32(7))))
                d = float(w[k, n]) - float(np.float32(q * float(s)))
                sq.append(d * d)
            want.append(((sq[0] + sq[4]) + sq[2]) + (sq[1] + sq[3]))
        assert err[:, n].tolist() == want
        assert index[n] == int(np.argmin(want)) and scale[n] == np.float32(s0[n] * ratio[index[n]])
    assert (err[index, np.arange(3)] <= err[0]).all()
    g = R.search_tensor(w, s0.max(), ratio, 4)[1]
    total = R.search_cols(w, np.full(3, s0.max(), np.float32), ratio, 4)[2].sum(axis=1)
    assert g == int(np.argmin(total))


def test_arguments_refused_on_the_host():
    from numpy_quant import kernels as K
    from numpy_quant.model import clip_candidates
    assert clip_candidates(None, 64, 32) is None
    assert np.array_equal(clip_candidates("mse", 64, 4).view(np.uint32), R.ratios(64).view(np.uint32))
    assert np.array_equal(K.clip_ratios(5).view(np.uint32), R.ratios(5).view(np.uint32))
    for clip, steps, bits in (("MSE", 64, 8), (True, 64, 8), ("mse", 0, 8), ("mse", 65, 8), ("mse", 8.0, 8),
                              ("mse", True, 8), ("mse", 64, 9)):
        with pytest.raises(ValueError):
            clip_candidates(clip, steps, bits)
    with pytest.raises(ValueError):
        K.clip_search_cols(np.zeros((4, 4), np.float32), np.ones(4, np.float32), R.ratios(4), 4)  # not on the device
