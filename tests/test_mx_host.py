"""The MX restatement (tests/_mx_ref.py) against itself and against torch's float8_e4m3fn conversion, and
the argument checks of the mx_format keywords.  No GPU."""
import numpy as np
import pytest

import _mx_ref as R


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_grid_values_survive_a_round_trip(fmt):
    """Every code point at both signs, under block exponents from -127 to 100: x on the grid comes back."""
    g = R.grid(fmt)
    vals = np.resize(np.concatenate([g, -g]), (8, 256))
    vals[:, ::32] = g[-1]  # the block's amax is the format's largest value, so X is the planted power of two
    for e in (-127, -20, 0, 100):
        x = (vals * 2.0 ** e).astype(np.float32)
        assert np.array_equal(x.astype(np.float64), vals * 2.0 ** e)  # representable
        codes, scales = R.mx_quantize(x, fmt)
        assert np.all(scales == e + 127)
        assert np.array_equal(R.mx_dequantize(codes, scales, fmt), x.astype(np.float64))
        assert np.array_equal(R.unpack(R.pack(codes, fmt), fmt), codes)


def test_e4m3_rounding_equals_torch():
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    rng = np.random.default_rng(0)
    g = R.grid("mxfp8")
    mid = (g[:-1] + g[1:]) / 2
    t = np.concatenate([g, mid, np.nextafter(mid, 0), np.nextafter(mid, 1000), rng.uniform(0, 448, 4000),
                        np.exp2(rng.uniform(-14, 0, 4000))]).astype(np.float32)
    t = np.concatenate([t, -t])
    t = t[np.abs(t) <= 448]
    want = torch.from_numpy(t).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(R.round_to_format(t.astype(np.float64), "mxfp8"), want)


@pytest.mark.parametrize("kw,match", [
    (dict(mx_format="fp8"), "mx_format"), (dict(mx_format="mxfp8", mx_weight_format="int4"), "mx_weight_format"),
    (dict(mx_format="mxfp4", mx_weight_format="mxfp8"), "pair"), (dict(mx_weight_format="mxfp4"), "needs mx_format"),
    (dict(mx_format="mxfp8", per_token=True), "per_token"), (dict(mx_format="mxfp8", group_size=64), "group_size"),
    (dict(mx_format="mxfp8", weight_clip="mse"), "weight_clip"), (dict(mx_format="mxfp8", weight_bit_width=4), "weight_bit_width"),
    (dict(mx_format="mxfp8", bit_width=16), "bit_width")])
def test_check_mx_args_refuses(kw, match):
    from numpy_quant.model import check_mx_args
    args = dict(mx_format=None, mx_weight_format=None, bit_width=8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        check_mx_args(**args)
    assert check_mx_args(None, None, 8) == (None, None) and check_mx_args("mxfp8", "mxfp4", 4) == ("mxfp8", "mxfp4")
    assert check_mx_args("mxfp4", None, 8) == ("mxfp4", "mxfp4")
