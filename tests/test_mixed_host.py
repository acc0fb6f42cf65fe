"""The separate weight bit width's restatement (tests/_mixed_ref.py) against the oracle and its own
rule; the bounds k_pg's nibble path rests on, per element; the accuracy the feature is for.  No GPU."""
import os

import numpy as np
import pytest

from conftest import ROOT

import _mixed_ref as R
import _perchannel_ref as P
from oracle import nq_oracle as O

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


@pytest.fixture(scope="module")
def layer():
    """The spread encoder-layer fixture (batch 1 here), its float output, and the restatement's
    results per (bit width, weight bit width, per_channel), each computed once."""
    proto, graph, x = R.encoder_layer_fixture(MODELS, batch=1)
    with np.errstate(all="ignore"):
        ref = O.outputs_of(graph, O.float_forward(graph, [x]))[0]
    cache = {}

    def run(bw, wbw, pc=False):
        if (bw, wbw, pc) not in cache:
            qp, qc, axes = R.calibrate(graph, [x], bw, wbw, per_channel=pc)
            vals = R.quantized_forward(graph, qp, qc, [x], bw, weights=axes)
            cache[(bw, wbw, pc)] = (qp, qc, axes, vals, R.outputs_of(graph, vals)[0])
        return cache[(bw, wbw, pc)]

    return graph, x, ref, run


def test_equal_widths_are_the_oracles_node_loop(layer, bw=8):
    graph, x, _, run = layer
    for wbw in (None, bw):
        qp, qc, axes = R.calibrate(graph, [x], bw, wbw)
        with np.errstate(all="ignore"):
            oqp, oqc = O.calibrate(graph, [x], bw)
        assert set(qp) == set(oqp) and set(qc) == set(oqc)
        for name, t in oqc.items():
            assert qc[name][2] == t[2] and np.array_equal(qc[name][1], t[1]), name
            assert np.array_equal(np.asarray(qc[name][3], np.float32).view(np.uint32),
                                  np.asarray(t[3], np.float32).view(np.uint32)), name
    vals = run(bw, bw)[3]
    with np.errstate(all="ignore"):
        ovals = O.quantized_forward(graph, oqp, oqc, [x], bw)
    assert set(vals) == set(ovals)
    for name, t in ovals.items():
        assert vals[name][0] == t[0], name
        if t[0] == "Q":
            assert vals[name][2] == t[2] and np.array_equal(vals[name][1], t[1]), name
        else:
            got, want = np.ascontiguousarray(vals[name][1]), np.ascontiguousarray(t[1])
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
    assert np.array_equal(run(bw, bw)[4].view(np.uint32), O.outputs_of(graph, ovals)[0].view(np.uint32))


def test_the_eligible_set_is_the_six_matmul_weights(layer):
    graph, x, _, run = layer
    axes = R.eligible(graph)
    matmul_weights = {ins[1] for _, op, _, ins, _ in graph.nodes if op == "MatMul" and ins[1] in graph.constants}
    assert len(axes) == 6 and set(axes) == matmul_weights and set(axes.values()) == {1}
    qp, qc, _, vals, _ = run(8, 4)
    for name, t in qc.items():  # the weights at 4 bits; LayerNorm parameters at 8, biases at 32
        assert (t[2] == 4) if name in axes else (t[2] in (8, 32)), name
        if name in axes:
            assert t[1].min() >= -8 and t[1].max() <= 7 and len(np.unique(t[1])) > 8
            s, _ = O.quant_parameters(*R.weight_range(graph.constants[name]), 4, False)
            assert np.array_equal(np.asarray(t[3]), np.asarray(s)) and t[4] is None
    widths = sorted({t[2] for t in qc.values()})
    assert widths == [4, 8, 32]
    for _, op, _, ins, outs in graph.nodes:  # every product has width 4 * 8, whatever the weight's
        if op == "MatMul":
            assert vals[outs[0]][2] == 32, outs
    with pytest.raises(ValueError):
        R.calibrate(graph, [x], 4, 8)
    for bad in (0, -1, 9, 4.0, True, "4"):
        with pytest.raises(ValueError):
            R.weight_width(8, bad)


@pytest.mark.parametrize("pc", [False, True])
def test_a_gemm_bias_keeps_four_times_the_activation_width(pc):
    from numpy_quant import onnx_proto
    graph = O.Graph(onnx_proto.load(os.path.join(MODELS, "mlp.onnx")))
    x = np.random.default_rng(0).uniform(-1.2, 1.2, size=(64, 2)).astype(np.float32)
    qp, qc, axes = R.calibrate(graph, [x], 8, 4, per_channel=pc)
    assert axes and set(axes.values()) == {0}  # transB: the columns on axis 0
    gemms = [(ins, outs) for _, op, _, ins, outs in graph.nodes if op == "Gemm"]
    assert gemms
    for ins, _ in gemms:
        w, b = qc[ins[1]], qc[ins[2]]
        assert w[2] == 4 and w[1].min() >= -8 and w[1].max() <= 7
        assert b[2] == 32
        s_x, s_w = qp[ins[0]].scale, qp[ins[1]].scale
        want = (np.float32(s_x) * np.asarray(s_w, np.float32)).astype(np.float32)
        assert np.array_equal(np.asarray(b[3], np.float32), want)
        if not pc:
            assert np.array_equal(b[1], O.quantize(graph.constants[ins[2]], 32, s_x * s_w, None))
    vals = R.quantized_forward(graph, qp, qc, [x], 8, weights=axes)
    for _, outs in gemms:
        assert vals[outs[0]][2] == 8  # requantized at the activation width
    out = R.outputs_of(graph, vals)[0]
    assert out.dtype == np.float32 and np.all(np.isfinite(out))


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("zpa", [-128, 0, 127])
def test_k_pg_bounds_hold_per_element_at_the_extremes(K, zpa):
    """16 (128 col_l1max + col_absmax |zpa|) < 2^31 bounds every partial sum of the nibble MFMA
    accumulator, and 128 col_l1max + col_absmax |zpa| < 2^24 every value the f32 epilogue converts:
    checked element by element, partial sum by partial sum, on operands built to reach them."""
    rng = np.random.default_rng(K + zpa)
    M, N = 6, 8
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    bt = rng.integers(-8, 8, size=(N, K)).astype(np.int8)
    R.extreme_columns(bt, a)
    assert a.min() == -128 and a.max() == 127 and bt.min() == -8 and bt.max() == 7
    b32, b24 = R.pg_bounds(bt, zpa)
    assert b24 == 128 * 8 * K + 8 * K * abs(zpa)  # column 0: l1 = |sum| = 8 K
    assert b32 == 16 * b24 and b32 < 2 ** 31 and b24 < 2 ** 24
    worst, final = R.pg_partial_sums(a, bt, zpa)
    assert worst.max() <= b32 and final.max() <= b24
    # reached: row 0 (-128) on column 0 (-8), or row 1 (127) on it, runs to 16 * 8 K (128 or 127 + |zpa|)
    assert worst.max() >= 16 * 8 * K * (127 + abs(zpa)) and final.max() >= 8 * K * (127 + abs(zpa))
    if zpa >= 0:
        assert worst[0, 0] == b32 and final[0, 0] == b24
    # the alternating column nearly cancels in its sum (-K / 2), not in its L1 norm (15 K / 2): the
    # column's own bound, below column 0's
    assert int(bt[2].astype(np.int64).sum()) == -K // 2
    assert worst[:, 2].max() <= 16 * (128 * (15 * K // 2) + (K // 2) * abs(zpa)) < b32
    # and the products themselves are what q_matmul gives
    acc = P.int_matmul(a, bt.T)
    assert np.array_equal(np.abs(acc - bt.astype(np.int64).sum(axis=1)[None, :] * zpa), final)


def test_w4a8_has_a_lower_output_error_than_w4a4(layer):
    graph, x, ref, run = layer
    err = {}
    for bw, wbw in ((8, 8), (8, 4), (4, 4)):
        for pc in (False, True):
            out = run(bw, wbw, pc)[4]
            err[(bw, wbw, pc)] = R.mse(ref, out)
            print(f"encoder layer ({bw},{wbw}) per_channel={pc}: output MSE {err[(bw, wbw, pc)]:.6g}, "
                  f"SQNR {R.sqnr_db(ref, out):.3f} dB")
    for pc in (False, True):
        assert err[(8, 4, pc)] < err[(4, 4, pc)]
