"""ONNX graph IR, float and quantized executors — the drop-in for
numpy_quant/model.py (Model.from_onnx / Model.quantize / Model.__call__ /
QModel.__call__), running every tensor op in libnqk.so on the MI355X.

The node loop is the reference's (model.py:294-326, 486-565): per node, QTensor
inputs of float ops are dequantized, float inputs of MatMul / Gemm are quantized
with the calibrated parameters, Gemm outputs are requantized.  All intermediate
values stay in HBM; `value.data.data` copies one to the host on request.
`QModel.__call__` runs through a fused device plan (plan.py, compiled on first
use) with bit-identical results for the hot MatMul chains; `qmodel.keep_values = True`
(or `profile=True`) keeps the reference's node-by-node loop, which materialises every
intermediate `value.data`.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from time import time
from typing import Any, List, Union

import numpy as np

from . import _lib
from . import onnx_proto
from .device import DeviceArray, permute, sync
from .images import QuantLut, UploadSlot
from .numpy_quantization import quant_parameters
from .tensor import (FTensor, ITensor, QTensor, Tensor, concat, fconv2d, qconv2d, quantize_tensor, where)
from . import kernels as K


class Constant:
    def __init__(self, name: str, outputs: List["Node"], data: Tensor = None):
        self.name = name
        self.outputs = outputs
        self.data = data

    def __repr__(self):
        return f"Constant({self.name})"


class Variable:
    def __init__(self, name: str, inputs: List["Node"], outputs: List["Node"], data: Tensor = None):
        self.name = name
        self.inputs = inputs
        self.outputs = outputs
        self.data = data

    def __repr__(self):
        return f"Variable({self.name})"


Value = Union[Constant, Variable]


class Node:
    def __init__(self, name: str, op: str, attrs: dict[str, Any], inputs: List[Value], outputs: List[Value]):
        self.name = name
        self.op = op
        self.attrs = attrs
        self.inputs = inputs
        self.outputs = outputs

    def __repr__(self):
        return f"Node({self.name})"


class QuantizationParams:
    def __init__(self, scale: np.float32, zero_point: Union[np.int64, None]):
        self.scale = scale
        self.zero_point = zero_point

    def __repr__(self):
        return f"QuantizationParams(scale={self.scale}, zero_point={self.zero_point})"


def _is_image_list(array, pre) -> bool:
    """Whether an input goes through `pre.resize` (images.ResizeCrop): a list or tuple of
    images (ValueError when no resize is configured) or a uint8 array when one is."""
    resize = getattr(pre, "resize", None)
    if isinstance(array, (list, tuple)):
        if resize is None:
            raise ValueError("A list of images is not supported without image_preprocess.resize (images.ResizeCrop)")
        return True
    return resize is not None and isinstance(array, np.ndarray) and array.dtype == np.uint8


def _topk_output(tensor, k: int):
    """(indices [B, k], probabilities [B, k]) device tensors of a model output [..., classes],
    leading axes flattened into B.  A QTensor is read as it is: no float logits are made."""
    if not isinstance(tensor, (FTensor, QTensor)) or tensor.dev.ndim < 2:
        shape = tuple(tensor.dev.shape) if hasattr(tensor, "dev") else np.shape(getattr(tensor, "data", None))
        raise ValueError(f"classify: the model's first output must be [batch, classes] (got {type(tensor).__name__} "
                         f"of shape {shape})")
    idx, prob = tensor.topk(k)
    flat = ITensor(np.array([-1, k], dtype=np.int64))
    return idx.reshape(flat), prob.reshape(flat)


def _listing(kind: str, fields) -> str:
    """Readable multi-line dump of an IR object: one line per element of each list or
    dict field (the reference prints its models this way, model.py:223-234, 464-484)."""
    out = [f"{kind}("]
    for name, val in fields:
        if isinstance(val, dict):
            out.append(f"  {name}={{")
            out.extend(f"    {k}: {v}," for k, v in val.items())
            out.append("  },")
        elif isinstance(val, list):
            out.append(f"  {name}=[")
            out.extend(f"    {e}" for e in val)
            out.append("  ],")
        else:
            out.append(f"  {name}={val},")
    out.append(")")
    return "\n".join(out) + "\n"


# ----------------------------------------------------------------------------- operators
def _gemm(inputs, attrs):
    x, w, b = inputs
    if attrs.get("transA"):
        x = x.T
    if attrs.get("transB"):
        if (isinstance(x, FTensor) and isinstance(w, FTensor) and x.dev.ndim == 2 and w.dev.ndim == 2
                and x.dev.shape[0] == 1):
            # x[1, K] @ w.T: NumPy's matmul takes OpenBLAS GEMV-T for this layout (the
            # w.T view has its columns contiguous), or sdot for one column, whose summation
            # orders differ from GEMM's
            n, k = w.dev.shape
            if K.small_one_row(n, k):
                return [FTensor(K.sgemv_small(x.dev, w.dev)) + b]
            if K.gemv_t_applies(1, n, k):
                return [FTensor(K.sgemv_t(x.dev, w.dev)) + b]
        if (isinstance(x, FTensor) and isinstance(w, FTensor) and x.dev.ndim == 2 and w.dev.ndim == 2
                and not x.tview and not w.tview and w.dev.shape[0] >= 2
                and K.gemm_small_regime(x.dev.shape[0], w.dev.shape[0], w.dev.shape[1], True)):
            # the small-matrix kernels of the transposed form read w[N, K] as it lies
            m, (n, k) = x.dev.shape[0], w.dev.shape
            if x.dev.shape[1] != k:
                raise ValueError(f"matmul: mismatch in core dimension ({x.dev.shape[1]} vs {k})")
            return [FTensor(K.sgemm(x.dev, k, 1, w.dev, 1, k, m, n, k, transb=True)) + b]
        w = w.T  # .tview: the matmul below takes the transposed form's order
    return [x.matmul(w) + b]


def _layernorm(inputs, attrs):
    x, g, b = inputs
    return [FTensor(K.layernorm(x.dev, g.dev, b.dev, attrs.get("axis", -1), attrs.get("epsilon", 1e-5)))]


def _slice(inputs, attrs):
    x = inputs[0]
    starts, ends, axes = inputs[1].data, inputs[2].data, inputs[3].data
    slices = [slice(None, None, None)] * x.shape.size
    for s, e, a in zip(starts, ends, axes):
        slices[a] = slice(s, e)
    return [x.__getitem__(tuple(slices))]


def _constant(inputs, attrs):
    v = attrs["value"]
    if v.dtype == np.float32:
        return [FTensor(v)]
    if v.dtype == np.int64:
        return [ITensor(v)]
    cls = v.dtype.__class__
    raise ValueError(f"Constant value type {cls.__module__}.{cls.__qualname__} not supported.")


def _constant_of_shape(inputs, attrs):
    v = attrs["value"]
    arr = np.full(tuple(inputs[0].data), fill_value=v, dtype=v.dtype)
    if v.dtype == np.float32:
        return [FTensor(arr)]
    if v.dtype == np.int64:
        return [ITensor(arr)]
    cls = v.dtype.__class__
    raise ValueError(f"Constant value type {cls.__module__}.{cls.__qualname__} not supported.")


_OPS = {
    "Add": lambda i, a: [i[0] + i[1]],
    "Concat": lambda i, a: [concat(list(i), axis=a["axis"])],
    "Constant": _constant,
    "ConstantOfShape": _constant_of_shape,
    "Conv": lambda i, a: [fconv2d(i[0], i[1], i[2], tuple(a["pads"]), tuple(a["strides"]))],
    "Div": lambda i, a: [i[0].div(i[1])],
    "Equal": lambda i, a: [i[0] == i[1]],
    "Erf": lambda i, a: [i[0].erf()],
    "Expand": lambda i, a: [i[0].expand(i[1])],
    "Gather": lambda i, a: [i[0].take(i[1], axis=a["axis"])],
    "Gemm": _gemm,
    "Identity": lambda i, a: [i[0].copy()],
    "LayerNormalization": _layernorm,
    "MatMul": lambda i, a: [i[0].matmul(i[1])],
    "Mul": lambda i, a: [i[0] * i[1]],
    "ReduceMean": lambda i, a: [i[0].mean(a["axis"], keepdims=a["keepdims"])],
    "Relu": lambda i, a: [i[0].relu()],
    "Reshape": lambda i, a: [i[0].reshape(i[1])],
    "Sigmoid": lambda i, a: [i[0].sigmoid()],
    "Shape": lambda i, a: [i[0].shape],
    "Slice": _slice,
    "Softmax": lambda i, a: [i[0].softmax(axis=a["axis"])],
    "Tanh": lambda i, a: [i[0].tanh()],
    "Transpose": lambda i, a: [i[0].transpose(a["perm"])],
    # model.py:203-206 returns the tensor itself instead of a 1-list; the executor
    # then unpacks it element-wise: the output is row 0 (kept bug-compatible)
    "Unsqueeze": lambda i, a: i[0].expand_dims(axis=i[1]),
    "Where": lambda i, a: [where(i[0], i[1], i[2])],
}


def onnx_operator_implementation(op: str, inputs: list[Tensor], attrs: dict[str, object]) -> list[Tensor]:
    """Device implementation of model.py:65-213 (same op set, same results)."""
    fn = _OPS.get(op)
    if fn is None:
        raise ValueError(f"ONNX operand {op} not supported.")
    return fn(inputs, attrs)


def integer_conv_eligible(node) -> bool:
    """Whether a Conv node takes the integer path when QModel.integer_conv is set: a quantized
    input with a scalar zero point or none, a quantized constant weight, a bias, dilation 1 and
    group 1.  Every other Conv keeps the float path."""
    if node.op != "Conv" or len(node.inputs) != 3:
        return False
    x, w, b = (i.data for i in node.inputs)
    if not isinstance(x, QTensor) or not isinstance(w, QTensor) or not isinstance(node.inputs[1], Constant):
        return False
    if not isinstance(b, (QTensor, FTensor)):
        return False
    for t in (x, w):
        if t._bias is not None or isinstance(t._zero_point, K.ZpTerm) or t.dev.ndim != 4:
            return False
    a = node.attrs
    if any(int(d) != 1 for d in a.get("dilations", [1, 1])) or int(a.get("group", 1)) != 1:
        return False
    return "pads" in a and "strides" in a


def per_channel_axis(value):
    """The axis of a constant's output columns when it may take one scale per column
    (QModel.per_channel), else None.  Eligible: a 2-D float constant every consumer of which is a
    MatMul that takes it as input 1 (columns on the last axis) or a Gemm that takes it as its
    weight, input 1 (the last axis, axis 0 with transB), all naming the same axis."""
    if not isinstance(value, Constant) or not isinstance(value.data, FTensor) or value.data.dev.ndim != 2:
        return None
    if not value.outputs or value.data.dev.size == 0:
        return None
    axes = set()
    for node in value.outputs:
        if node.op not in ("MatMul", "Gemm") or len(node.inputs) < 2 or node.inputs[1] is not value:
            return None
        if any(i is value for k, i in enumerate(node.inputs) if k != 1):
            return None
        axes.add(0 if node.op == "Gemm" and node.attrs.get("transB") else 1)
    return axes.pop() if len(axes) == 1 else None


def column_scales(tensor: FTensor, axis: int, bit_width: int) -> np.ndarray:
    """float32 [N]: quant_parameters (numpy_quantization.py:7-21, symmetric) of every output
    column's own range clamped to include 0 (tensor.py:304-308 applied to one column); the
    columns lie on `axis` of the 2-D `tensor`.  The minima and maxima come from one kernel."""
    dev = tensor.dev if axis % 2 == 1 else permute(tensor.dev, [1, 0])
    mn, mx = K.minmax_cols(dev)
    zero = np.array(0.0).astype(np.float32)
    lo, hi = np.minimum(mn, zero), np.maximum(mx, zero)
    return np.array([quant_parameters(lo[n], hi[n], bit_width, False)[0] for n in range(lo.shape[0])],
                    dtype=np.float32)


def weight_width(bit_width, weight_bit_width) -> int:
    """The width of the eligible weights (per_channel_axis) of a model quantized at `bit_width`:
    `weight_bit_width`, an int with 1 <= weight_bit_width <= bit_width, or bit_width for None.
    Anything else raises ValueError."""
    if weight_bit_width is None:
        return bit_width
    if (isinstance(weight_bit_width, bool) or not isinstance(weight_bit_width, (int, np.integer))
            or not 1 <= weight_bit_width <= bit_width):
        raise ValueError(f"weight_bit_width must be an integer in 1..bit_width ({bit_width}), or None "
                         f"(got {weight_bit_width!r})")
    return int(weight_bit_width)


# ----------------------------------------------------------------------------- models
class Model:
    def __init__(self, nodes: list[Node], values: list[Value], inputs: List[Variable], outputs: List[Variable]):
        self.nodes = nodes
        self.values = values
        self.inputs = inputs
        self.outputs = outputs
        # an images.ImagePreprocess: uint8 image batches are then accepted as inputs
        # (normalized and moved to NCHW on the device); None: uint8 is refused
        self.image_preprocess = None
        # an equalize.Equalization on the result of Model.equalize (its sites and their vectors)
        self.equalization = None

    def __repr__(self):
        return f"Model({len(self.nodes)} nodes, {len(self.values)} values, inputs={self.inputs}, outputs={self.outputs})"

    def __str__(self):
        return _listing("Model", [("nodes", self.nodes), ("values", self.values), ("inputs", self.inputs),
                                  ("outputs", self.outputs)])

    def __del__(self):
        # break node <-> value cycles so device buffers are released promptly (model.py:236-247)
        for node in getattr(self, "nodes", []):
            node.inputs = []
            node.outputs = []
        for value in getattr(self, "values", []):
            if isinstance(value, Variable):
                value.inputs = []
            value.outputs = []

    @classmethod
    def from_onnx(cls, onnx_model):
        """model.py:249-292.  Accepts a decoded onnx_proto.ModelProto (or anything
        duck-typed like onnx.ModelProto), a file path or raw bytes."""
        if isinstance(onnx_model, (str, os.PathLike, bytes, bytearray)):
            onnx_model = onnx_proto.load(onnx_model)
        graph = onnx_model.graph
        value_dict: dict[str, Value] = {}
        for t in graph.initializer:
            arr = np.array(t.to_array() if hasattr(t, "to_array") else onnx_proto.to_array(t))
            value_dict[t.name] = Constant(t.name, outputs=[], data=FTensor(arr))
        inputs: List[Value] = []
        for vi in graph.input:
            var = Variable(vi.name, inputs=[], outputs=[])
            value_dict[vi.name] = var
            inputs.append(var)
        nodes: dict[str, Node] = {}
        for n in graph.node:
            node = Node(name=n.name, op=n.op_type,
                        attrs={a.name: onnx_proto.attribute_value(a) for a in n.attribute},
                        inputs=[value_dict[i] for i in n.input], outputs=[])
            for i in n.input:
                value_dict[i].outputs.append(node)
            for o in n.output:
                if o in value_dict:
                    value_dict[o].inputs.append(node)
                else:
                    value_dict[o] = Variable(name=o, inputs=[node], outputs=[])
            node.outputs = [value_dict[o] for o in n.output]
            nodes[n.name] = node
        outputs = [value_dict[vi.name] for vi in graph.output]
        return cls(list(nodes.values()), list(value_dict.values()), inputs, outputs)

    def rebatch(self, batch: int) -> int:
        """Rewrite the batch-1 int64 shape constants of a torch export in place
        (onnx_proto.rebatch).  The batch-1 original is kept in
        the node's attribute dict, which a QModel built from this model shares, so
        either one may be rebatched any number of times."""
        count = 0
        for node in self.nodes:
            if node.op != "Constant":
                continue
            v = node.attrs.setdefault("__batch1_value__", node.attrs.get("value"))
            if isinstance(v, np.ndarray) and v.dtype == np.int64 and v.ndim == 1 and v.shape[0] in (3, 4) and v[0] == 1:
                v = v.copy()
                v[0] = batch
                node.attrs["value"] = v
                count += 1
        return count

    def _set_inputs(self, inputs):
        for array, variable in zip(inputs, self.inputs):
            if _is_image_list(array, self.image_preprocess):
                variable.data = self.image_preprocess.to_device(array)
            elif array.dtype == np.float32:
                variable.data = FTensor(np.ascontiguousarray(array))
            elif array.dtype == np.int64:
                variable.data = ITensor(array.copy())
            elif array.dtype == np.uint8 and self.image_preprocess is not None:
                variable.data = self.image_preprocess.to_device(array)
            else:
                raise ValueError(f"Array dtype {array.dtype} not supported")

    def _forward(self, inputs, profile=False) -> dict:
        """The node loop of the float executor; the outputs stay on the device."""
        times = {op: 0.0 for op in {n.op for n in self.nodes}}
        self._set_inputs(inputs)
        for node in self.nodes:
            args = [i.data for i in node.inputs]
            t0 = time()
            outs = onnx_operator_implementation(node.op, args, node.attrs)
            if profile:
                sync()
            times[node.op] += time() - t0
            for o, tensor in zip(node.outputs, outs):
                o.data = tensor
        return times

    def __call__(self, inputs: List[np.ndarray], profile=False):
        """Float executor (model.py:294-326), on device."""
        times = self._forward(inputs, profile)
        result = [out.data.data for out in self.outputs]
        return (result, times) if profile else result

    def classify(self, inputs: List[np.ndarray], k: int = 5):
        """`(indices int64 [B, k], probabilities float32 [B, k])` of the model's first output
        [B, classes]: per row np.argsort(-logits, kind="stable")[:k] and the Softmax of the
        logits gathered there, computed on the device (one kernel); only the [B, k] results
        are downloaded.  Inputs as `__call__` takes them."""
        self._forward(inputs)
        idx, prob = _topk_output(self.outputs[0].data, k)
        return idx.data, prob.data

    def calibrate(self, calibration_inputs: list[np.ndarray]) -> tuple[dict, dict]:
        """Float forward + per-value global min / max (model.py:329-336), min/max on device."""
        self(calibration_inputs)
        vmin, vmax = {}, {}
        for val in self.values:
            t = val.data
            if isinstance(t, FTensor):
                mn, mx = K.minmax(t.dev)
                vmin[val.name], vmax[val.name] = np.mean(mn), np.mean(mx)
            else:
                d = t.data
                flat = d.reshape((d.shape[0], -1) if d.shape else (-1,))
                vmin[val.name], vmax[val.name] = np.mean(flat.min()), np.mean(flat.max())
        return vmin, vmax

    def equalize(self, batches, alpha=0.5, emax=8, pow2=True) -> "Model":
        """Channel equalization (equalize.py; not the reference's behaviour): a new float Model over
        the same graph in which every LayerNorm that feeds only MatMul weights has its gamma and beta
        divided by a per-channel vector s[k] and row k of those weights multiplied by s[k], so that
        the LN output the quantizer sees is flat.  s comes from the channel maxima of the LN outputs
        over `batches` (an iterable of input lists, one float forward each, accumulated on the
        device) and of the weights' rows: s[k] = 2^e[k], e[k] = clip(rint(r[k] - median(r)), -emax,
        emax), r[k] = alpha log2 a[k] - (1 - alpha) log2 w[k]; `pow2=False` keeps the exponent
        unrounded.  With pow2 the result computes the source's float outputs bit for bit.  `self` is
        not changed and shares every other constant with the result, whose `equalization` lists
        the sites and their vectors.  Quantize the result as any other Model."""
        from .equalize import equalize
        if isinstance(self, QModel):
            raise ValueError("equalize: call it on the float Model, before it is quantized")
        return equalize(self, batches, alpha, emax, pow2)

    def quantize(self, calibration_inputs: list[np.ndarray], bit_width=8, integer_conv=False, per_channel=False,
                 weight_bit_width=None):
        """Calibration + graph rewrite (model.py:328-442).  `integer_conv=True` (not the
        reference's behaviour): eligible Conv nodes multiply their quantized operands in integers
        (QModel.integer_conv).  `per_channel=True` (not the reference's behaviour either): every
        MatMul / Gemm weight gets one scale per output column (QModel.per_channel).
        `weight_bit_width=w` (not the reference's behaviour either, 1 <= w <= bit_width): the same
        weights are quantized at w bits, everything else at bit_width (QModel.weight_bit_width)."""
        weight_width(bit_width, weight_bit_width)  # refused before the calibration forward
        vmin, vmax = self.calibrate(calibration_inputs)

        def params(value: Value, asym: bool, bw=bit_width):
            s, z = quant_parameters(vmin[value.name], vmax[value.name], bit_width=bw, asymmetric=asym)
            return QuantizationParams(s, z)

        return self._rewrite(bit_width, params, integer_conv=integer_conv, per_channel=per_channel,
                             weight_bit_width=weight_bit_width)

    def calibrate_stream(self, batches, percentile=100.0, clip_weights=False) -> tuple[dict, dict]:
        """`calibrate` over any number of batches (calibration.py): per batch one float forward
        whose values are accumulated on the device into per-value histograms of float bit
        patterns; nothing is downloaded until the end, and only one batch's values are alive at
        a time.  `batches`: an iterable (a generator will do: one pass) of input lists as
        `__call__` takes them.  `percentile` in (50, 100] clips every variable's range at that
        percentile of all its observed elements, to 2^-5 relative; 100 is the exact min / max,
        `calibrate`'s answer.  `clip_weights`: clip the constants too."""
        from .calibration import Calibrator
        cal = Calibrator(percentile, clip_weights)
        seen = False
        for inputs in batches:
            self._forward(inputs)
            cal.observe(self)
            seen = True
        if not seen:
            raise ValueError("calibrate_stream: no calibration batch")
        return cal.ranges()

    def quantize_stream(self, batches, bit_width=8, percentile=100.0, clip_weights=False, integer_conv=False,
                        per_channel=False, weight_bit_width=None):
        """`quantize` with the ranges of `calibrate_stream(batches, percentile, clip_weights)`.
        `per_channel` with `clip_weights` is refused: the per-column ranges are the exact minima
        and maxima of the constants."""
        weight_width(bit_width, weight_bit_width)
        if per_channel and clip_weights:
            raise ValueError("quantize_stream: per_channel takes the exact per-column ranges of the weights; "
                             "clip_weights does not combine with it")
        vmin, vmax = self.calibrate_stream(batches, percentile, clip_weights)

        def params(value: Value, asym: bool, bw=bit_width):
            s, z = quant_parameters(vmin[value.name], vmax[value.name], bit_width=bw, asymmetric=asym)
            return QuantizationParams(s, z)

        return self._rewrite(bit_width, params, integer_conv=integer_conv, per_channel=per_channel,
                             weight_bit_width=weight_bit_width)

    def compare(self, qmodel, batches, k=5, labels=None, values=True):
        """What `qmodel` lost against this float model over an evaluation set: a
        `compare.Report` with the error statistics of every value and the agreement of the two
        models' top-k classes (compare.py defines the metrics).  Everything is accumulated on
        the device (one kernel per value and batch); per batch only the two [B, k] index
        arrays are downloaded, and the statistics once at the end.

        `batches`: an iterable (a generator will do: one pass) of input lists as `__call__`
        takes them.  `labels`: an iterable of integer arrays [B], one per batch, adds the
        top-1 and top-k accuracy of both models.
        `values=True` runs the float forward and the QModel's node loop, so that every value of
        both models exists, and compares every value name the two share (constants once).  Both
        models' values of one batch are alive at the same time, and the node loop is far
        slower than the fused plan: size the evaluation batches accordingly.
        `values=False` runs the QModel as `qmodel(inputs)` does, through the fused plan, and
        compares the model outputs only: accuracy over a large evaluation set at full speed."""
        from .compare import Agreement, Comparator, Report
        if isinstance(self, QModel) or not isinstance(qmodel, QModel):
            raise ValueError("compare: call it on the float Model with its QModel as the argument")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"compare: k must be a positive integer (got {k!r})")
        if [v.name for v in self.outputs] != [v.name for v in qmodel.outputs]:
            raise ValueError("compare: the two models have different outputs")
        k = int(k)
        cmp = Comparator()
        agree = Agreement(labels is not None)
        label_it = iter(labels) if labels is not None else None
        eager = bool(values) or qmodel.keep_values
        for inputs in batches:
            lab = None
            if label_it is not None:
                try:
                    lab = next(label_it)
                except StopIteration:
                    raise ValueError("compare: fewer label arrays than batches") from None
            self._forward(inputs)
            kept = {v.name: v.data for v in self.inputs if isinstance(v.data, FTensor)}
            if not eager and qmodel._plan is None and qmodel.fuse:
                qmodel.compile()
            qmodel.set_inputs(inputs)
            qmodel.run(eager=eager)
            if values:
                cmp.observe(self, qmodel, ref_inputs=kept)
            else:
                for ref, got in zip(self.outputs, qmodel.outputs):
                    cmp.observe_pair(ref.name, ref.data, got.data, "variable",
                                     ref.inputs[0].op if ref.inputs else "Input")
            fidx, _ = _topk_output(self.outputs[0].data, k)
            qidx, _ = _topk_output(qmodel.outputs[0].data, k)
            agree.add(fidx.data, qidx.data, lab)
        if agree.rows == 0:
            raise ValueError("compare: no evaluation batch")
        states = cmp.states()
        return Report(cmp.report(states), k, agree, qmodel.bit_width, states)

    def quantize_with(self, quant_params: dict, bit_width=8, integer_conv=False, per_channel=False,
                      weight_bit_width=None):
        """The graph rewrite of Model.quantize with given per-value quantization
        parameters (e.g. calibrated on a smaller batch, or the reference's own),
        skipping the calibration forward.  With `per_channel` the entry of an eligible weight
        (per_channel_axis) may hold a float32 scale vector, one entry per output column; every
        entry is taken as it is given.  With `weight_bit_width` the entry of an eligible weight is
        the scale of that width: the weight is quantized with it at weight_bit_width."""
        return self._rewrite(bit_width, lambda value, asym, bw=None: quant_params[value.name],
                             integer_conv=integer_conv, per_channel=per_channel, given=True,
                             weight_bit_width=weight_bit_width)

    def load_quantized(self, path):
        """The QModel saved by `QModel.save(path)` (blob.py) on this model's graph:
        no calibration forward and no constant re-quantization."""
        from . import blob
        return blob.load(self, path)

    def _rewrite(self, bit_width, params, constants=None, integer_conv=False, per_channel=False, given=False,
                 weight_bit_width=None):
        """model.py:338-442.  `constants`: name -> ready quantized QTensor (blob.py);
        those constants are taken as they are instead of being quantized here.
        `per_channel`: eligible weights (per_channel_axis) get a scale per output column, computed
        here from the weight's columns, or taken from `params` when `given`.
        `weight_bit_width`: the width of the same eligible weights (range, scale and integers, per
        tensor or per column); every other constant, every activation and every bias (4 * bit_width)
        keeps `bit_width`.  `params(value, asym, bw)` then gives an eligible weight's parameters at
        that width."""
        wbw = weight_width(bit_width, weight_bit_width)
        constants = constants or {}
        wanted = {}
        if constants:
            # a blob must carry exactly this graph's constants, each with this graph's shape:
            # never quietly re-quantize a missing one from local weights, never attach a
            # blob of another model whose initializer names happen to match
            graph_consts = {v.name: v for v in self.values if isinstance(v, Constant)}
            missing = sorted(set(graph_consts) - set(constants))
            extra = sorted(set(constants) - set(graph_consts))
            if missing or extra:
                raise ValueError(f"blob constants differ from the graph's: missing {missing[:5]}, "
                                 f"unknown {extra[:5]}")
            for name, t in constants.items():
                d = graph_consts[name].data
                want = None if d is None else tuple(d.dev.shape if hasattr(d, "dev") else np.shape(d.data))
                if want is not None and tuple(t.dev.shape) != want:
                    raise ValueError(f"blob constant {name}: shape {tuple(t.dev.shape)}, graph {want}")

        def qconst(value, bw, scale, zp, axis=-1):
            t = constants.get(value.name)
            if t is None:
                return quantize_tensor(value.data, bw, scale, zp, scale_axis=axis)
            wanted[value.name] = bw  # a bias is quantized at bw, then again at 4*bw: last wins
            return t

        node_dict = {node.name: node for node in self.nodes}
        value_dict = {value.name: value for value in self.values}

        qnodes: OrderedDict[str, Node] = OrderedDict()
        qvalues: dict[str, Value] = {}
        qp: dict[str, QuantizationParams] = {}
        for value in self.inputs:
            qvalues[value.name] = value
            qp[value.name] = params(value, isinstance(value, Variable))
        for value in self.values:
            if isinstance(value, Constant):
                # the constant's width: the weights' for a MatMul / Gemm weight, else the model's
                cbw = wbw if wbw != bit_width and per_channel_axis(value) is not None else bit_width
                p = params(value, False) if cbw == bit_width else params(value, False, cbw)
                axis = per_channel_axis(value) if per_channel else None
                if axis is not None and not given:
                    p = QuantizationParams(column_scales(value.data, axis, cbw), None)
                if K.is_cols(p.scale):
                    if not per_channel:
                        raise ValueError(f"{value.name}: a scale vector is given, but per_channel is not set")
                    if p.zero_point is not None:
                        raise ValueError(f"{value.name}: a per-column scale has no zero point")
                    if axis is None and not any(n.op == "Gemm" and len(n.inputs) > 2 and n.inputs[2] is value
                                                for n in value.outputs):
                        raise ValueError(f"{value.name}: a scale vector is given, but the constant is neither a "
                                         "MatMul / Gemm weight nor a Gemm bias")
                if K.is_cols(p.scale) and axis is None:
                    # a Gemm bias with the vector a per_channel QModel's quant_params hold for it: the
                    # Gemm branch below quantizes it at 4 * bit_width with s_x * s_w[n]; nothing to do here
                    qvalues[value.name] = Constant(value.name, [], None)
                    qp[value.name] = p
                    continue
                qt = qconst(value, cbw, p.scale, p.zero_point, -1 if axis is None else axis)
                qt._is_weight = True
                qvalues[value.name] = Constant(value.name, [], qt)
                qp[value.name] = p
        for node in self.nodes:
            out_val = node.outputs[0]
            if node.op == "MatMul":
                qnodes[node.name] = Node(node.name, "MatMul", node.attrs, [], [])
                qp[out_val.name] = params(out_val, True)
                qvalues[out_val.name] = Variable(out_val.name, [], [], None)
            if node.op == "Gemm":
                for iv in node.inputs[:2]:
                    if isinstance(iv, Variable):
                        qvalues[iv.name] = Variable(iv.name, [], [], None)
                        qp[iv.name] = params(iv, True)
                bias = node.inputs[2]
                s_x, s_w = qp[node.inputs[0].name].scale, qp[node.inputs[1].name].scale
                if K.is_cols(s_w):  # bscale[n] = s_x * s_w[n], float32 element by element
                    bscale = (np.float32(s_x) * np.asarray(s_w, dtype=np.float32)).astype(np.float32)
                else:
                    bscale = s_x * s_w
                qp[bias.name] = QuantizationParams(bscale, None)
                qvalues[bias.name] = Constant(bias.name, [], qconst(bias, 4 * bit_width, bscale, None))
                qnodes[node.name] = Node(node.name, "Gemm", node.attrs, [], [])
                qp[out_val.name] = params(out_val, True)
                qvalues[out_val.name] = Variable(out_val.name, [], [], None)
            if node.op == "Add" and (isinstance(node.inputs[0], Constant) or isinstance(node.inputs[1], Constant)):
                bi, xi = (0, 1) if isinstance(node.inputs[0], Constant) else (1, 0)
                bname = node.inputs[bi].name
                bscale = qp[node.inputs[xi].name].scale
                qvalues[bname] = Constant(bname, [], qconst(node.inputs[bi], 4 * bit_width, bscale, None))
                qp[bname] = QuantizationParams(bscale, None)
                qnodes[node.name] = Node(node.name, "Add", node.attrs, [], [])
                qp[out_val.name] = params(out_val, True)
                qvalues[out_val.name] = Variable(out_val.name, [], [], None)
            elif node.op in ("Identity", "Relu"):
                qvalues[out_val.name] = Variable(out_val.name, [], [], None)
                qp[out_val.name] = qp[node.inputs[0].name]
                qnodes[node.name] = Node(node.name, node.op, node.attrs, [], [])
            else:
                qvalues[out_val.name] = Variable(out_val.name, [], [], None)
                qp[out_val.name] = params(out_val, True)
                qnodes[node.name] = Node(node.name, node.op, node.attrs, [], [])
        for name, qnode in qnodes.items():
            qnode.inputs = [qvalues[i.name] for i in node_dict[name].inputs]
            qnode.outputs = [qvalues[o.name] for o in node_dict[name].outputs]
        for name, qvalue in qvalues.items():
            if isinstance(qvalue, Variable):
                qvalue.inputs = [qnodes[i.name] for i in value_dict[name].inputs]
            qvalue.outputs = [qnodes[o.name] for o in value_dict[name].outputs]
        for name, bw in wanted.items():
            if qvalues[name].data.bit_width != bw:
                raise ValueError(f"blob constant {name}: bit width {qvalues[name].data.bit_width}, the graph needs {bw}")
        qoutputs = [qvalues[o.name] for o in self.outputs]
        qinputs = [qvalues[i.name] for i in self.inputs]
        qmodel = QModel(list(qnodes.values()), list(qvalues.values()), qinputs, qoutputs, bit_width, qp)
        qmodel.image_preprocess = self.image_preprocess
        qmodel.integer_conv = bool(integer_conv)
        qmodel.per_channel = bool(per_channel)
        qmodel.weight_bit_width = wbw
        return qmodel


class QModel(Model):
    def __init__(self, nodes, values, inputs, outputs, bit_width: int, quant_params: dict[str, QuantizationParams]):
        super().__init__(nodes, values, inputs, outputs)
        self.bit_width = bit_width
        self.quant_params = quant_params
        self._deq_cache: dict[str, FTensor] = {}
        self._image_luts: dict[str, QuantLut] = {}  # per uint8 input (image_preprocess)
        self._plan = None
        # QModel.__call__ compiles the fused plan on first use (NQK_FUSE=0: never);
        # keep_values = True runs the reference's node loop instead, so every
        # intermediate value.data is populated (reference test/test_mlp.py:159-168)
        self.fuse = os.environ.get("NQK_FUSE", "1") != "0"
        self.keep_values = False
        # opt-in, not the reference's behaviour: a Conv whose input and weight are quantized
        # multiplies them in integers (tensor.qconv2d: q_matmul on the im2col of the quantized
        # input) instead of dequantizing both for the float Conv.  Set it before the first call:
        # the fused plan reads it when it is compiled.
        self.integer_conv = False
        # opt-in, not the reference's behaviour: every MatMul / Gemm weight was quantized with one
        # scale per output column (per_channel_axis; tensor.QTensor carries the vector).  The
        # integer products are unchanged; dequantize and requantize take the column's scale.  Set
        # by Model.quantize(per_channel=True); the fused plan hands such a model's GEMMs the product
        # vectors (nqk_epilogue.s_col): k_pg's per-column variant, or the small-tile GEMM kernel.
        self.per_channel = False
        # opt-in, not the reference's behaviour: the width of every MatMul / Gemm weight (the
        # constants per_channel_axis names), 1 <= weight_bit_width <= bit_width; activations, every
        # other constant and the biases (4 * bit_width) keep bit_width.  Equal to bit_width unless
        # Model.quantize(weight_bit_width=...) set it.  The integer products are q_matmul's; at
        # weight_bit_width <= 4 the fused plan packs the weights as nibbles under activations of any
        # width up to 8 (nqk_epilogue.w_bits).
        self.weight_bit_width = bit_width

    def __repr__(self):
        return (f"QModel({len(self.nodes)} nodes, {len(self.values)} values, bit_width={self.bit_width}, "
                f"inputs={self.inputs}, outputs={self.outputs})")

    def __str__(self):
        return _listing("QModel", [("nodes", self.nodes), ("values", self.values), ("inputs", self.inputs),
                                   ("outputs", self.outputs), ("bit_width", self.bit_width),
                                   ("quant_params", self.quant_params)])

    def _dequant_input(self, value: Value) -> FTensor:
        if isinstance(value, Constant):
            hit = self._deq_cache.get(value.name)
            if hit is None:
                hit = value.data.dequantize()
                self._deq_cache[value.name] = hit
            return hit
        return value.data.dequantize()

    def set_inputs(self, inputs: List[np.ndarray]):
        for array, variable in zip(inputs, self.inputs):
            qp = self.quant_params[variable.name]
            if _is_image_list(array, self.image_preprocess):
                pre = self.image_preprocess
                variable.data = QTensor(pre.resize_lookup_host(array, self._image_lut(variable)), self.bit_width,
                                        scale=qp.scale, zero_point=qp.zero_point)
            elif isinstance(array, FTensor):
                variable.data = quantize_tensor(array, self.bit_width, qp.scale, qp.zero_point)
            elif array.dtype == np.float32:
                variable.data = quantize_tensor(FTensor(np.ascontiguousarray(array)), self.bit_width, qp.scale,
                                                qp.zero_point)
            elif array.dtype == np.int64:
                variable.data = ITensor(array)
            elif array.dtype == np.uint8 and self.image_preprocess is not None:
                self.image_preprocess.check(array)
                self._set_images(variable, DeviceArray.from_host(array), array.shape)
            else:
                raise ValueError(f"Array dtype {array.dtype} not supported")

    def _image_lut(self, variable) -> DeviceArray:
        """The quantized table of this input (images.QuantLut)"""
        qp = self.quant_params[variable.name]
        return self._image_luts.setdefault(variable.name, QuantLut()).get(self.image_preprocess, self.bit_width,
                                                                          qp.scale, qp.zero_point)

    def _set_images(self, variable, images_dev, shape):
        """The input QTensor of a uint8 batch on the device: one table lookup writes what
        quantize_tensor(FTensor(image_preprocess.reference(images))) would."""
        pre = self.image_preprocess
        qp = self.quant_params[variable.name]
        variable.data = QTensor(pre.lookup(images_dev, shape, self._image_lut(variable)), self.bit_width,
                                scale=qp.scale, zero_point=qp.zero_point)

    def _set_slot(self, variable, slot):
        """_set_images of classify_stream's staged batch (a RaggedBatch goes through the resize
        kernel, which checks its descriptors in the slot's pinned copy)."""
        if slot.batch is None:
            return self._set_images(variable, slot.images(), slot.shape)
        pre = self.image_preprocess
        qp = self.quant_params[variable.name]
        out = pre.lookup_resized(slot.images(), slot.batch, slot.host.ptr, self._image_lut(variable))
        variable.data = QTensor(out, self.bit_width, scale=qp.scale, zero_point=qp.zero_point)

    def classify_stream(self, batches, topk=None):
        """Iterator of the model's first output for an iterable of uint8 image batches (with
        `image_preprocess.resize`: of lists of HWC images, packed with their descriptors and
        taps into the one pinned buffer), in order, equal to `qmodel([batch])[0]` of each.
        Batch k + 1 is copied into one of two pinned host buffers and uploaded on the library's copy stream while batch k computes;
        the lookup kernel waits for its batch's copy, and a copy into a staging buffer waits
        for the kernel that last read it.  A batch the model refuses raises what
        `qmodel([batch])` raises, after the results of the batches before it were handed
        out; the library is back on stream 0 then.
        With `topk=k` it yields `(indices [B, k], probabilities [B, k])` per batch instead, equal
        to `classify([batch], k)`: the top-k kernel is issued on the forward's stream right
        behind it, and only its results are downloaded."""
        pre = self.image_preprocess
        if pre is None:
            raise ValueError("classify_stream: set qmodel.image_preprocess first")
        if len(self.inputs) != 1:
            raise ValueError("classify_stream: a model with one (image) input")
        if not self.keep_values and self._plan is None and self.fuse:
            self.compile()
        variable = self.inputs[0]
        slots = [UploadSlot(), UploadSlot()]

        def stage(k, batch):
            if pre.resize is not None:
                batch = pre.pack(batch)  # checks it
            else:
                pre.check(batch)
            slots[k % 2].upload(batch)

        try:
            it = iter(batches)
            k = 0
            try:
                stage(0, next(it))
            except StopIteration:
                return
            while True:
                slot = slots[k % 2]
                self._set_slot(variable, slot)
                slot.consumed()
                self.run(eager=self.keep_values)
                top = None if topk is None else _topk_output(self.outputs[0].data, topk)
                # batch k is issued: stage batch k + 1 beside it; an error of that batch is
                # raised after batch k's result went out
                more, failure = True, None
                try:
                    stage(k + 1, next(it))
                except StopIteration:
                    more = False
                except Exception as e:  # noqa: BLE001
                    failure = e
                if top is None:
                    yield self.outputs_device()[0].data
                else:
                    yield top[0].data, top[1].data
                if failure is not None:
                    raise failure
                if not more:
                    return
                k += 1
        finally:
            _lib.call("nqk_set_stream", 0)
            sync()  # no upload in flight when the pinned buffers go
            for slot in slots:
                slot.close()

    def compile(self):
        """Build the fused device plan (plan.py): matched transformer layers run as
        fused launches with bit-identical results; everything else stays eager.
        Values inside fused layers are not materialised (their `.data` is None)."""
        from .plan import compile_plan
        self._plan = compile_plan(self)
        return self._plan

    def save(self, path) -> int:
        """Write the packed quantized constants + every QuantizationParams (blob.py);
        `Model.load_quantized(path)` rebuilds this QModel on the same graph."""
        from . import blob
        return blob.save(self, path)

    def graph(self, example_inputs, topk=None):
        """Capture one forward on inputs of this shape as a hipGraph (graph.py); the
        returned DeviceGraph replays it with one launch and the same results.  With
        `topk=k` the top-k kernel is captured behind the forward and the graph returns
        `[indices, probabilities]` as `classify(inputs, k)` does."""
        from .graph import DeviceGraph
        return DeviceGraph(self, example_inputs, topk=topk)

    def _run_node(self, node, times, profile=False):
        """One iteration of the node loop of QModel.__call__ (model.py:502-550)."""
        args = []
        if self.integer_conv and node.op == "Conv" and integer_conv_eligible(node):
            return self._run_qconv(node, times, profile)
        if node.op in ("MatMul", "Gemm"):
            for i in node.inputs:
                if isinstance(i.data, FTensor):
                    qp = self.quant_params[i.name]
                    t0 = time()
                    args.append(quantize_tensor(i.data, self.bit_width, qp.scale, qp.zero_point))
                    if profile:
                        sync()
                    if times is not None:
                        times["TinyqQuant"] += time() - t0
                else:
                    args.append(i.data)
        else:
            for i in node.inputs:
                if isinstance(i.data, QTensor):
                    t0 = time()
                    args.append(self._dequant_input(i))
                    if profile:
                        sync()
                    if times is not None:
                        times["TinyqDequant"] += time() - t0
                else:
                    args.append(i.data)
        t0 = time()
        outs = onnx_operator_implementation(node.op, args, node.attrs)
        if node.op == "Gemm":
            qp = self.quant_params[node.outputs[0].name]
            outs = [t.requantize(self.bit_width, qp.scale, qp.zero_point) for t in outs]
        if profile:
            sync()
        if times is not None:
            times[node.op] += time() - t0
        for o, tensor in zip(node.outputs, outs):
            o.data = tensor

    def _run_qconv(self, node, times, profile=False):
        """An eligible Conv with integer_conv set: input and weight stay quantized (qconv2d), the
        bias is the dequantized float constant of the float path; timed under "Conv"."""
        x, w, b = node.inputs
        t0 = time()
        bias = self._dequant_input(b) if isinstance(b.data, QTensor) else b.data
        if profile:
            sync()
        if times is not None:
            times["TinyqDequant"] += time() - t0
        t0 = time()
        out = qconv2d(x.data, w.data, bias, tuple(node.attrs["pads"]), tuple(node.attrs["strides"]))
        if profile:
            sync()
        if times is not None:
            times["Conv"] += time() - t0
        node.outputs[0].data = out

    def run(self, profile=False, eager=False):
        """The node loop of QModel.__call__ (model.py:497-550) on device tensors,
        through the fused plan when one was compiled (and not `eager`)."""
        times = {op: 0.0 for op in {n.op for n in self.nodes}}
        times["TinyqQuant"] = 0.0
        times["TinyqDequant"] = 0.0
        if self._plan is not None and not eager:
            self._plan.run(self, times, profile)
        else:
            for node in self.nodes:
                self._run_node(node, times, profile)
        return times

    def outputs_device(self) -> list[FTensor]:
        res = []
        for out_var in self.outputs:
            d = out_var.data
            if isinstance(d, FTensor):
                res.append(d)
            elif isinstance(d, QTensor):
                res.append(d.dequantize())
            else:
                raise ValueError
        return res

    def __call__(self, inputs: List[np.ndarray], profile=False):
        """QModel.__call__ (model.py:486-565).  The fused plan (bit-identical) unless
        keep_values is set or a per-op profile is asked for (profile=True returns the
        reference's {op_type: seconds} dict, which needs the node loop)."""
        eager = self.keep_values or profile
        if not eager and self._plan is None and self.fuse:
            self.compile()
        self.set_inputs(inputs)
        times = self.run(profile=profile, eager=eager)
        outs = [t.data for t in self.outputs_device()]
        return (outs, times) if profile else outs

    def classify(self, inputs: List[np.ndarray], k: int = 5):
        """`(indices int64 [B, k], probabilities float32 [B, k])` of the model's first output
        [B, classes]: what np.argsort(-logits, kind="stable")[:, :k] and the Softmax of
        `qmodel(inputs)[0]` gathered there give, bit for bit, computed on the device.  A
        quantized output (the requantized classifier Gemm) is read in its integer storage by the
        one top-k kernel: no float logits are made, and only the [B, k] results are downloaded.
        Inputs, `image_preprocess` and the choice of the fused plan as in `__call__`."""
        eager = self.keep_values
        if not eager and self._plan is None and self.fuse:
            self.compile()
        self.set_inputs(inputs)
        self.run(eager=eager)
        idx, prob = _topk_output(self.outputs[0].data, k)
        return idx.data, prob.data
