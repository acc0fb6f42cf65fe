"""NumPy restatement of channel equalization (Model.equalize): the specification.

Not the reference's behaviour: the reference quantizes every activation with one scale.  Here the
LayerNorm that feeds a group of MatMuls is rewritten so that its wide output channels move into
the weights: gamma and beta are divided by a vector s[k], row k of every consuming weight is
multiplied by s[k].  The float model computes the same function.  Nothing here imports numpy_quant
but its ONNX reader.

Site     a LayerNormalization node over the last axis (axis == -1) whose scale gamma and bias beta
         are 1-D constants of one length K consumed by that node alone, whose output is no graph
         output, and every consumer of whose output is a MatMul taking it as input 0 with a 2-D
         constant weight W_i [K, N_i] on input 1 that this MatMul alone consumes.
a[k]     max over all rows of all batches of |Y[r, k]|, Y the LN's float32 output as [rows, K]
w[k]     max over the site's weights i and n of |W_i[k, n]|
         both as integer maxima of key(v) = bits(v) & 0x7FFFFFFF, every NaN -> 0x7FC00000
r[k]     alpha * log2(f64(a[k])) - (1 - alpha) * log2(f64(w[k])), float64
x[k]     clip(r[k] - median(r over the usable k), -emax, emax); a channel is usable when a[k] and
         w[k] are finite and above zero; x[k] = 0 on every other channel
e[k]     rint(x[k]) as an integer
s[k]     pow2: f32(2^e[k]);  else: f32(2^x[k])
gamma'   gamma / s, beta' = beta / s, W_i'[k, n] = W_i[k, n] * s[k]: float32, one rounding each
"""
import copy
from collections import OrderedDict

import numpy as np

from oracle import nq_oracle as O

NAN_KEY = np.uint32(0x7FC00000)


class Site:
    def __init__(self, node, out, gamma, beta, weights, K):
        self.node, self.out, self.gamma, self.beta, self.weights, self.K = node, out, gamma, beta, list(weights), K

    def __repr__(self):
        return f"Site({self.node}: {self.gamma}, {self.beta} -> {self.weights}, K={self.K})"


def check_parameters(alpha, emax):
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0 <= alpha <= 1:
        raise ValueError(f"alpha {alpha!r} is not in 0..1")
    if isinstance(emax, bool) or not isinstance(emax, (int, np.integer)) or not 1 <= emax <= 16:
        raise ValueError(f"emax {emax!r} is not an integer in 1..16")
    return float(alpha), int(emax)


def find_sites(graph):
    uses = {}
    for name, op, _, ins, _ in graph.nodes:
        for k, v in enumerate(ins):
            uses.setdefault(v, []).append((name, op, k, ins))
    sites = []
    for name, op, attrs, ins, outs in graph.nodes:
        if op != "LayerNormalization" or len(ins) != 3 or attrs.get("axis", -1) != -1:
            continue
        g, b = ins[1], ins[2]
        if g == b or any(c not in graph.constants or len(uses[c]) != 1 for c in (g, b)):
            continue
        K = graph.constants[g].shape
        if len(K) != 1 or graph.constants[b].shape != K or K[0] == 0:
            continue
        out = outs[0]
        if out in graph.outputs or not uses.get(out):
            continue
        weights = []
        for _, cop, k, cins in uses[out]:
            w = cins[1] if cop == "MatMul" and k == 0 and len(cins) == 2 else None
            arr = graph.constants.get(w)
            if arr is None or arr.ndim != 2 or arr.shape[0] != K[0] or arr.shape[1] == 0 or len(uses[w]) != 1:
                weights = None
                break
            weights.append(w)
        if weights:
            sites.append(Site(name, out, g, b, weights, K[0]))
    return sites


def abs_key(arr):
    """uint32 keys of float32 values, monotone in the magnitude; every NaN is NAN_KEY."""
    k = np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.where(k > np.uint32(0x7F800000), NAN_KEY, k).astype(np.uint32)


def absmax(arr, axis):
    """np.abs(arr).max(axis) of a 2-D float32 array through the keys (the kernel's statement)."""
    return abs_key(arr).max(axis=axis).view(np.float32)


def activation_maxima(graph, batches, sites=None):
    """{LN output name: a float32 [K]} over every batch (a list of input lists)."""
    sites = find_sites(graph) if sites is None else sites
    keys = {s.out: np.zeros(s.K, np.uint32) for s in sites}
    for inputs in batches:
        with np.errstate(all="ignore"):
            vals = O.float_forward(graph, inputs)
        for s in sites:
            y = vals[s.out][1]
            keys[s.out] = np.maximum(keys[s.out], abs_key(y.reshape(-1, s.K)).max(axis=0))
    return {name: k.view(np.float32) for name, k in keys.items()}


def weight_maxima(graph, site):
    k = np.zeros(site.K, np.uint32)
    for w in site.weights:
        k = np.maximum(k, abs_key(graph.constants[w]).max(axis=1))
    return k.view(np.float32)


def exponent_vector(a, w, alpha=0.5, emax=8):
    """x [K] float64 of the rule above from the two float32 maxima."""
    alpha, emax = check_parameters(alpha, emax)
    a64, w64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    ok = np.isfinite(a64) & np.isfinite(w64) & (a64 > 0) & (w64 > 0)
    x = np.zeros(a64.shape, np.float64)
    if ok.any():
        r = alpha * np.log2(a64[ok]) - (1.0 - alpha) * np.log2(w64[ok])
        x[ok] = np.clip(r - np.median(r), -emax, emax)
    return x


def scales(x, pow2=True):
    """(what `exponents` reports, s float32 [K])."""
    if pow2:
        e = np.rint(x).astype(np.int64)
        return e, np.exp2(e.astype(np.float64)).astype(np.float32)
    return x, np.exp2(x).astype(np.float32)


def exponents(graph, batches, alpha=0.5, emax=8, pow2=True):
    """{LN output name: int64 e [K]}, or the float64 x [K] without pow2."""
    sites = find_sites(graph)
    a = activation_maxima(graph, batches, sites)
    return {s.out: scales(exponent_vector(a[s.out], weight_maxima(graph, s), alpha, emax), pow2)[0] for s in sites}


def apply(graph, vectors, pow2=True):
    """A graph with the sites' constants rewritten; `vectors` as `exponents` returns them."""
    new = copy.copy(graph)
    new.constants = OrderedDict(graph.constants)
    for s in find_sites(graph):
        v = np.asarray(vectors[s.out])
        sk = np.exp2(v.astype(np.float64)).astype(np.float32)
        assert sk.shape == (s.K,) and (not pow2 or v.dtype.kind == "i")
        new.constants[s.gamma] = np.true_divide(graph.constants[s.gamma], sk)
        new.constants[s.beta] = np.true_divide(graph.constants[s.beta], sk)
        for w in s.weights:
            new.constants[w] = graph.constants[w] * sk[:, None]
        assert all(new.constants[n].dtype == np.float32 for n in (s.gamma, s.beta, *s.weights))
    return new


def equalize(graph, batches, alpha=0.5, emax=8, pow2=True):
    """Model.equalize: (the rewritten graph, {LN output name: vector})."""
    if not batches:
        raise ValueError("equalize: no calibration batch")
    vec = exponents(graph, batches, alpha, emax, pow2)
    return apply(graph, vec, pow2), vec


# ----------------------------------------------------------------------------- fixture
OUTLIERS, FACTOR = 6, np.float32(32)


def own_parameters(proto):
    """Give every value that is an Identity of an initializer an initializer of its own, in place.
    The ONNX exporter shares equal tensors that way: the encoder-layer graph's layernorm_after
    parameters are Identities of layernorm_before's, so as shipped neither LayerNorm is a site (a
    shared gamma cannot take two vectors).  Returns the number of Identity nodes replaced."""
    from numpy_quant.onnx_proto import TensorProto  # the ONNX reader only
    g = proto.graph
    inits = {t.name: t for t in g.initializer}
    count = 0
    for node in list(g.node):
        if node.op_type == "Identity" and node.input[0] in inits:
            t = TensorProto()
            t.name = node.output[0]
            t.set_array(np.array(inits[node.input[0]].to_array()))
            g.initializer.append(t)
            g.node.remove(node)
            count += 1
    return count


def boost_gamma(proto, graph, seed, count=OUTLIERS, factor=FACTOR):
    """Multiply `count` seeded entries of every site's gamma by `factor` in `proto`, in place.
    Returns {LN output name: the sorted channel indices}."""
    rng = np.random.default_rng(seed)
    tensors = {t.name: t for t in proto.graph.initializer}
    picked = {}
    for s in find_sites(graph):
        idx = np.sort(rng.choice(s.K, size=count, replace=False))
        g = graph.constants[s.gamma].copy()
        g[idx] = g[idx] * factor
        tensors[s.gamma].set_array(g)
        picked[s.out] = idx
    return picked


SEED = 7
LAYER = "vit_image_classifier_encoder_layer_no_weights.onnx"


def outlier_fixture(models_dir, batch=2, outliers=True, seed=SEED):
    """(proto, graph, x, {LN output name: outlier channels}): the encoder-layer graph with seeded
    stand-in weights and one seeded input batch [batch, 197, 768] (as tests/_perchannel_ref.py's
    encoder_layer_fixture, without its column spread: that spread reaches LayerNorm 2's input
    through the out-projection, whose channels then differ by themselves), each LayerNorm with
    parameters of its own and OUTLIERS entries of its gamma multiplied by FACTOR."""
    import os
    from numpy_quant import onnx_proto  # the ONNX reader only
    proto = onnx_proto.load(os.path.join(models_dir, LAYER), synthetic_weights=True, seed=seed)
    if batch != 1:
        onnx_proto.rebatch(proto, batch)
    assert find_sites(O.Graph(proto)) == [] and own_parameters(proto) == 2
    picked = boost_gamma(proto, O.Graph(proto), seed) if outliers else {}
    x = np.random.default_rng(seed).standard_normal((batch, 197, 768)).astype(np.float32)
    return proto, O.Graph(proto), x, picked


def mse(ref, got):
    d = np.asarray(ref, np.float64) - np.asarray(got, np.float64)
    return float(np.mean(d * d))
