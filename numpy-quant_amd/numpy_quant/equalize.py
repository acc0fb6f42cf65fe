"""Channel equalization: move the wide output channels of a LayerNorm into the weights it feeds.

Not the reference's behaviour (opt-in: `Model.equalize`).  Every activation is quantized with one
scale, and in a transformer the LayerNorm output that feeds QKV and FFN-up has a few channels with
a large gamma whose range sets the step of all the others.  Dividing gamma and beta by a vector
s[k] and multiplying row k of every consuming weight by s[k] leaves the float function as it was
(SmoothQuant's identity) and hands the quantizer a flat activation.

Site     a LayerNormalization node over the last axis (axis == -1) whose scale gamma and bias beta
         are 1-D constants of one length K consumed by that node alone, whose output is no model
         output, and every consumer of whose output is a MatMul taking it as input 0 with a 2-D
         constant weight W_i [K, N_i] on input 1 that this MatMul alone consumes.
a[k]     max over all rows of all calibration batches of |Y[r, k]|, Y the LN's output as [rows, K]
w[k]     max over the site's weights i and n of |W_i[k, n]|
         (both on the device: nqk_absmax_f32, an integer maximum of float bit patterns)
r[k]     alpha * log2(f64(a[k])) - (1 - alpha) * log2(f64(w[k])), float64, on the host
x[k]     clip(r[k] - median(r over the usable k), -emax, emax); a channel is usable when a[k] and
         w[k] are finite and above zero, x[k] = 0 on every other one.  The median is subtracted
         because a per-tensor quantizer does not see a factor common to all channels.
e[k]     rint(x[k]), an integer
s[k]     pow2 (the default): f32(2^e[k]);  pow2=False: f32(2^x[k])
gamma'   gamma / s, beta' = beta / s, W_i'[k, n] = W_i[k, n] * s[k]: float32, one rounding each
         (nqk_binary_f32 with the vector broadcast)

With pow2 every one of those roundings is exact, and so is every step of the float forward that
sees them: RN(RN(n gamma 2^-e) + beta 2^-e) = RN(RN(n gamma) + beta) 2^-e, and each product
(y 2^-e)(w 2^e) of the MatMul is the float it was.  The equalized float model is bit-identical to
the source in every value but the LN outputs (unless a scaled value leaves the normal range).
"""
from __future__ import annotations

import numbers

import numpy as np

from . import _lib
from . import kernels as K
from .device import DeviceArray
from .tensor import FTensor


class Site:
    """One LayerNorm and the MatMul weights its output feeds."""

    def __init__(self, node, out, gamma, beta, weights):
        self.node = node                              # the LayerNormalization Node
        self.out = out.name                           # its output's name
        self.gamma, self.beta = gamma.name, beta.name
        self.weights = [w.name for w in weights]
        self.K = int(gamma.data.dev.shape[0])
        self.vector = None                            # Equalizer.exponents()'s entry, once applied
        self.scale = None                             # s float32 [K], once applied

    def __repr__(self):
        return f"Site({self.node.name}: {self.gamma}, {self.beta} -> {self.weights}, K={self.K})"


class Equalization:
    """What `Model.equalize` did: `result.equalization`."""

    def __init__(self, sites, alpha, emax, pow2):
        self.sites, self.alpha, self.emax, self.pow2 = sites, alpha, emax, pow2

    def __repr__(self):
        return f"Equalization({len(self.sites)} sites, alpha={self.alpha}, emax={self.emax}, pow2={self.pow2})"


def check_parameters(alpha, emax) -> tuple:
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0 <= alpha <= 1:
        raise ValueError(f"equalize: alpha must be a real number in 0..1 (got {alpha!r})")
    if isinstance(emax, bool) or not isinstance(emax, (int, np.integer)) or not 1 <= emax <= 16:
        raise ValueError(f"equalize: emax must be an integer in 1..16 (got {emax!r})")
    return float(alpha), int(emax)


def _vector_constant(value, consumer) -> bool:
    from .model import Constant
    return (isinstance(value, Constant) and isinstance(value.data, FTensor) and value.data.dev.ndim == 1
            and value.data.dev.size > 0 and len(value.outputs) == 1 and value.outputs[0] is consumer)


def find_sites(model) -> list:
    """The sites of `model` (the rule at the top of this module), in node order."""
    from .model import Constant
    sites = []
    for node in model.nodes:
        if node.op != "LayerNormalization" or len(node.inputs) != 3 or node.attrs.get("axis", -1) != -1:
            continue
        _, g, b = node.inputs
        if g is b or not _vector_constant(g, node) or not _vector_constant(b, node):
            continue
        k = g.data.dev.shape[0]
        if b.data.dev.shape[0] != k:
            continue
        out = node.outputs[0]
        if not out.outputs or any(out is o for o in model.outputs):
            continue
        weights = []
        for c in out.outputs:
            w = c.inputs[1] if c.op == "MatMul" and len(c.inputs) == 2 and c.inputs[0] is out else None
            if (not isinstance(w, Constant) or not isinstance(w.data, FTensor) or w.data.dev.ndim != 2
                    or w.data.dev.shape[0] != k or w.data.dev.shape[1] == 0 or len(w.outputs) != 1):
                weights = None
                break
            weights.append(w)
        if weights:
            sites.append(Site(node, out, g, b, weights))
    return sites


def exponent_vector(a, w, alpha: float, emax: int) -> np.ndarray:
    """x float64 [K] of the rule above from the two float32 maxima (host NumPy)."""
    a64, w64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    usable = np.isfinite(a64) & np.isfinite(w64) & (a64 > 0) & (w64 > 0)
    x = np.zeros(a64.shape, np.float64)
    if usable.any():
        r = alpha * np.log2(a64[usable]) - (1.0 - alpha) * np.log2(w64[usable])
        x[usable] = np.clip(r - np.median(r), -emax, emax)
    return x


class Equalizer:
    """Accumulates every site's channel maxima on the device and rewrites the constants.

    One uint32 arena holds a[k] and w[k] of all sites; `observe()` is one launch per site without
    a synchronisation or a download, `exponents()` downloads the arena once."""

    def __init__(self, model, alpha=0.5, emax=8, pow2=True):
        self.alpha, self.emax = check_parameters(alpha, emax)
        self.pow2 = bool(pow2)
        self.model = model
        self.sites = find_sites(model)
        self._values = {v.name: v for v in model.values}
        self._at = {}
        total = 0
        for s in self.sites:
            self._at[s.out] = total
            total += s.K
        self._total = total
        self._arena = DeviceArray((2, max(1, total)), np.uint32).fill_zero()
        self._weights_done = False
        self._vectors = None

    def _state(self, site, which: int) -> DeviceArray:
        return self._arena.offset_view(which * max(1, self._total) + self._at[site.out], (site.K,))

    def observe(self) -> None:
        """After a float forward of the model: every site's LN output into its a[k]."""
        for s in self.sites:
            t = self._values[s.out].data
            if not isinstance(t, FTensor) or t.dev.ndim < 1 or t.dev.shape[-1] != s.K:
                raise ValueError(f"{s.out}: observe() needs the float forward's LayerNorm output [..., {s.K}]")
            K.absmax(t.dev, self._state(s, 0), 0, rows=t.dev.size // s.K, cols=s.K, ld=s.K)
        self._vectors = None

    def _observe_weights(self) -> None:
        if self._weights_done:
            return
        for s in self.sites:
            for name in s.weights:
                K.absmax(self._values[name].data.dev, self._state(s, 1), 1)
        self._weights_done = True

    def maxima(self) -> dict:
        """{LN output name: (a float32 [K], w float32 [K])}: the one download."""
        self._observe_weights()
        host = self._arena.to_host().view(np.float32)
        return {s.out: (host[0, self._at[s.out]:self._at[s.out] + s.K], host[1, self._at[s.out]:self._at[s.out] + s.K])
                for s in self.sites}

    def exponents(self) -> dict:
        """{LN output name: int64 e [K]}, or the float64 x [K] when pow2 is off."""
        if self._vectors is None:
            out = {}
            for name, (a, w) in self.maxima().items():
                x = exponent_vector(a, w, self.alpha, self.emax)
                out[name] = np.rint(x).astype(np.int64) if self.pow2 else x
            self._vectors = out
        return self._vectors

    def apply(self):
        """The equalized Model: a new Model over the same graph with its own nodes and values.
        The sites' gamma, beta and weights are new constants; every other constant shares its
        device tensor with the source model, which is left as it was."""
        from .model import Constant, Model, Node, Variable
        vectors = self.exponents()
        src = self.model
        replaced = {}
        sites = []
        for s in self.sites:
            v = vectors[s.out]
            sk = np.exp2(v.astype(np.float64)).astype(np.float32)
            sdev = DeviceArray.from_host(sk)
            col = sdev.reshape((s.K, 1))
            for name in (s.gamma, s.beta):
                replaced[name] = FTensor(K.binary(_lib.DIV, self._values[name].data.dev, sdev))
            for name in s.weights:
                replaced[name] = FTensor(K.binary(_lib.MUL, self._values[name].data.dev, col))
            done = Site.__new__(Site)
            done.__dict__.update(s.__dict__)
            done.vector, done.scale = v, sk
            sites.append(done)
        values = {}
        for value in src.values:
            if isinstance(value, Constant):
                values[value.name] = Constant(value.name, [], replaced.get(value.name, value.data))
            else:
                values[value.name] = Variable(value.name, [], [], None)
        nodes = {}
        for node in src.nodes:
            nodes[node.name] = Node(node.name, node.op, node.attrs, [values[i.name] for i in node.inputs],
                                    [values[o.name] for o in node.outputs])
        for value in src.values:
            new = values[value.name]
            if isinstance(value, Variable):
                new.inputs = [nodes[n.name] for n in value.inputs]
            new.outputs = [nodes[n.name] for n in value.outputs]
        for done in sites:
            done.node = nodes[done.node.name]
        result = Model(list(nodes.values()), list(values.values()), [values[i.name] for i in src.inputs],
                       [values[o.name] for o in src.outputs])
        result.image_preprocess = src.image_preprocess
        result.equalization = Equalization(sites, self.alpha, self.emax, self.pow2)
        return result


def equalize(model, batches, alpha=0.5, emax=8, pow2=True):
    """Model.equalize."""
    eq = Equalizer(model, alpha, emax, pow2)
    seen = False
    for inputs in batches:
        model._forward(inputs)
        eq.observe()
        seen = True
    if not seen:
        raise ValueError("equalize: no calibration batch")
    return eq.apply()
