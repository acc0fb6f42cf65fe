"""What a quantization costs, value by value: the float model against the quantized model.

After a forward of both models every value sits in HBM under the same name (`Model._rewrite`
keeps the names).  Every compared value owns one row of a device arena, 8 words of state, into
which `nqk_compare_stats` (nqk_compare.hip) accumulates batch after batch; the arena is
downloaded once, at the end, and every metric is derived from it on the host in float64.

Pair   x is the float model's element (float32), y the quantized model's: float32, or the
       integer storage of a QTensor read as np.float32(np.float64(q - zp) * np.float64(scale))
       (`dequantize`, never materialised).  A pair is skipped when x or the float32 y is NaN or
       +-inf.  Otherwise d = np.float64(x) - np.float64(y).
State  int64 [8]: [0] pairs compared, [1] pairs skipped, then as float64 bit patterns [2] sum |d|,
       [3] sum d * d, [4] sum np.float64(x) ** 2, [5] max |d|; [6] and [7] stay 0.  A fresh state is
       all zero bytes.  Every call accumulates into it.
Sums   float64 additions in one fixed order, so a state is a function of the data and the
       order of the calls, never of the grid or of which workgroup ran first:
       chunk c is elements [4096 c, 4096 (c + 1)); lane t of 256 adds the terms of elements
       4096 c + 1024 j + 4 t + k, j = 0..3 outer, k = 0..3 inner, to +0.0 (absent and skipped
       elements add +0.0: nothing, every term being >= +0); the 256 lane sums fold by adjacent
       pairs, v = v[0::2] + v[1::2] until one is left: the chunk's partial.  Then lane t of 256
       adds the partials of chunks t, t + 256, .. in increasing order to +0.0, those lane sums
       fold the same way, and the total is added to the state word.  `host_state` is that in
       NumPy.  Within (n - 1) * 2^-53 relative of the exact sum of the float64 terms.
Metric mean_abs = sum |d| / count (the reference's compare_all_nodes), mse = sum d^2 / count,
       rms_ref = sqrt(sum x^2 / count), sqnr_db = 10 log10(sum x^2 / sum d^2): inf when sum d^2
       is 0, nan when both are; max_abs.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

import numpy as np

from . import kernels as K
from .device import DeviceArray, copy_strided
from .kernels import CMP_CHUNK, CMP_STATE
from .tensor import FTensor, ITensor, QTensor


def _fold(v: np.ndarray) -> np.ndarray:
    """adjacent pairs along the last axis until one is left"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _ordered_sum(terms: np.ndarray) -> np.float64:
    """The kernel's sum of one call's float64 terms (>= +0, zero where a pair is skipped)."""
    n = terms.size
    chunks = (n + CMP_CHUNK - 1) // CMP_CHUNK
    padded = np.zeros(chunks * CMP_CHUNK, dtype=np.float64)
    padded[:n] = terms
    t = padded.reshape(chunks, 4, 256, 4)  # [c, j, lane, k]
    lane = np.zeros((chunks, 256), dtype=np.float64)
    for j in range(4):
        for k in range(4):
            lane = lane + t[:, j, :, k]
    partial = _fold(lane)
    rounds = (chunks + 255) // 256
    padded = np.zeros(rounds * 256, dtype=np.float64)
    padded[:chunks] = partial
    lane = np.zeros(256, dtype=np.float64)
    for row in padded.reshape(rounds, 256):
        lane = lane + row
    return _fold(lane)


def host_state(x, y, state=None) -> np.ndarray:
    """The state nqk_compare_stats leaves after one call on float32 `x` and `y` (a quantized y
    dequantized first), from `state` or a fresh one, in NumPy."""
    x = np.asarray(x, dtype=np.float32).ravel()
    y = np.asarray(y, dtype=np.float32).ravel()
    if x.shape != y.shape:
        raise ValueError(f"shapes differ ({x.shape} against {y.shape})")
    out = np.zeros(CMP_STATE, dtype=np.int64) if state is None else np.array(state, dtype=np.int64)
    if out.shape != (CMP_STATE,):
        raise ValueError(f"state must be int64 [{CMP_STATE}]")
    if x.size == 0:
        return out
    ok = np.isfinite(x) & np.isfinite(y)
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xd - y.astype(np.float64)
        ad = np.where(ok, np.abs(d), 0.0)
        terms = (ad, np.where(ok, d * d, 0.0), np.where(ok, xd * xd, 0.0))
    f = out.view(np.float64)
    out[0] += int(ok.sum())
    out[1] += int(x.size - ok.sum())
    for w, t in enumerate(terms):
        f[2 + w] = f[2 + w] + _ordered_sum(t)
    f[5] = max(f[5], ad.max())
    return out


@dataclass(frozen=True)
class ValueStats:
    """The metrics of one value (the module docstring defines them)."""
    count: int
    nonfinite: int
    mean_abs: float
    mse: float
    rms_ref: float
    sqnr_db: float
    max_abs: float
    kind: str   # "variable" or "constant"
    op: str     # the producing node's op; "Input" for a graph input, "Initializer" for a constant


def stats_from_state(state, kind: str = "variable", op: str = "") -> ValueStats:
    """ValueStats of one int64 [8] state, in float64 on the host."""
    if not isinstance(state, np.ndarray) or state.shape != (CMP_STATE,) or state.dtype != np.int64:
        raise ValueError(f"state must be int64 [{CMP_STATE}]")
    count, skipped = int(state[0]), int(state[1])
    sa, sd, sx, mx = (float(v) for v in state.view(np.float64)[2:6])
    nan = float("nan")
    if sd == 0.0:
        sqnr = math.inf if sx > 0.0 else nan
    elif sx == 0.0:
        sqnr = -math.inf
    else:
        sqnr = 10.0 * math.log10(sx / sd)
    return ValueStats(count, skipped, sa / count if count else nan, sd / count if count else nan,
                      math.sqrt(sx / count) if count else nan, sqnr, mx, kind, op)


def _producer(value) -> tuple:
    from .model import Constant
    if isinstance(value, Constant):
        return "constant", "Initializer"
    nodes = getattr(value, "inputs", None) or []
    return "variable", (nodes[0].op if nodes else "Input")


class Comparator:
    """Accumulates the comparison state of every named value on the device.  The arena is
    int64 [rows, 8], zero-filled; it grows by doubling."""

    def __init__(self):
        self._rows: dict[str, int] = {}
        self._meta: dict[str, tuple] = {}
        self._arena: DeviceArray | None = None

    def reserve(self, rows: int) -> None:
        have = 0 if self._arena is None else self._arena.shape[0]
        if rows <= have:
            return
        arena = DeviceArray((max(rows, 2 * have), CMP_STATE), np.int64).fill_zero()
        if have:
            copy_strided(self._arena, arena, (have * CMP_STATE,), (1,), (1,))
        self._arena = arena

    def _row(self, name: str) -> DeviceArray:
        row = self._rows.get(name)
        if row is None:
            row = len(self._rows)
            self.reserve(row + 1)
            self._rows[name] = row
        return self._arena.offset_view(row * CMP_STATE, (CMP_STATE,))

    def observe_pair(self, name: str, ref, got, kind: str = "variable", op: str = "") -> None:
        """Accumulate `got` (the quantized model's FTensor or QTensor) against `ref` (the float
        model's FTensor) under `name`: one call of the kernel, no synchronisation, no download.
        A QTensor is read in its integer storage when its zero point is a scalar or None; one
        with a q_matmul zero-point term or a per-column scale goes through `dequantize()` first, and one with a
        pending bias raises what `dequantize()` raises."""
        if not isinstance(ref, FTensor):
            raise ValueError(f"{name}: the reference side must be an FTensor (got {type(ref).__name__})")
        if not isinstance(got, (FTensor, QTensor)):
            raise ValueError(f"{name}: the compared side must be an FTensor or a QTensor (got {type(got).__name__})")
        if tuple(ref.dev.shape) != tuple(got.dev.shape):
            raise ValueError(f"{name}: shapes differ (float model {tuple(ref.dev.shape)}, quantized model "
                             f"{tuple(got.dev.shape)})")
        scale = zp = None
        if isinstance(got, QTensor):
            if got._bias is not None or isinstance(got._zero_point, K.ZpTerm) or got.per_column:
                y = got.dequantize().dev  # nqk_compare_stats takes one scalar scale
            else:
                y, scale, zp = got.dev, got.scale, got._zero_point
        else:
            y = got.dev
        self._meta.setdefault(name, (kind, op))
        K.compare_stats(ref.dev, y, self._row(name), scale=scale, zp=zp)

    def observe(self, model, qmodel, ref_inputs=None) -> None:
        """Every value name present in both models, after a forward of each that left every
        value in place (the QModel's node loop): variables each time, constants the first time
        only (the weight error; the biases at 4 x the bit width).  Values the float model holds
        on the host (ITensor) are skipped; a shape mismatch is a ValueError.
        `ref_inputs`: {name: FTensor} of the float model's inputs.  A QModel shares the input
        Variables that feed no Gemm with its float model, so its `set_inputs` replaces their
        float tensors; a caller that kept them hands them in here."""
        from .model import Constant
        theirs = {v.name: v for v in qmodel.values}
        kept = ref_inputs or {}
        pairs = []
        for val in model.values:
            q = theirs.get(val.name)
            ref = kept.get(val.name, val.data)
            if q is None or not isinstance(ref, FTensor):
                continue
            if isinstance(val, Constant) and val.name in self._rows:
                continue
            if q.data is None or isinstance(q.data, ITensor):
                raise ValueError(f"{val.name}: the quantized model holds no tensor for it (run its node loop: "
                                 "set_inputs, then run(eager=True))")
            pairs.append((val, ref, q.data))
        self.reserve(len(self._rows) + sum(1 for val, _, _ in pairs if val.name not in self._rows))
        for val, ref, got in pairs:
            kind, op = _producer(val)
            self.observe_pair(val.name, ref, got, kind, op)

    def state(self, name: str) -> np.ndarray:
        """int64 [8] of one value, on the host."""
        if name not in self._rows:
            raise KeyError(name)
        return self._row(name).to_host()

    def states(self) -> dict:
        """{name: int64 [8]} in the order of first observation, from one download of the arena."""
        n = len(self._rows)
        if not n:
            return {}
        states = self._arena.offset_view(0, (n, CMP_STATE)).to_host()
        return {name: states[row] for name, row in self._rows.items()}

    def report(self, states=None) -> dict:
        """{name: ValueStats} of `states()` (one download of the arena when none are given)."""
        states = self.states() if states is None else states
        return {name: stats_from_state(state, *self._meta[name]) for name, state in states.items()}


class Agreement:
    """Running top-k agreement and accuracy counts over batches of [B, k] index arrays."""

    def __init__(self, labelled: bool):
        self.rows = self.top1 = self.topk = 0
        self.correct = None if not labelled else {"float": [0, 0], "quantized": [0, 0]}

    def add(self, fidx: np.ndarray, qidx: np.ndarray, labels=None) -> None:
        self.rows += fidx.shape[0]
        self.top1 += int(np.sum(fidx[:, 0] == qidx[:, 0]))
        self.topk += int(np.sum(np.any(qidx == fidx[:, :1], axis=1)))
        if self.correct is not None:
            lab = np.asarray(labels)
            if lab.dtype.kind not in "iu" or lab.shape != (fidx.shape[0],):
                raise ValueError(f"compare: labels of a batch must be {fidx.shape[0]} integers (got {lab.dtype} "
                                 f"{lab.shape})")
            for tag, idx in (("float", fidx), ("quantized", qidx)):
                self.correct[tag][0] += int(np.sum(idx[:, 0] == lab))
                self.correct[tag][1] += int(np.sum(np.any(idx == lab[:, None], axis=1)))


class Report:
    """The result of `Model.compare`.

    values           {name: ValueStats}, in graph order
    states           {name: int64 [8]}: the raw state every ValueStats was derived from
    k, rows          the k of the top-k figures and the number of classified rows
    top1_agreement   share of rows whose top-1 class is the same in both models
    topk_agreement   share of rows whose float top-1 class lies in the quantized top-k
    top1_accuracy, topk_accuracy   {"float": .., "quantized": ..} when labels were given, else None
    """

    def __init__(self, values: dict, k: int, agreement: Agreement, bit_width=None, states=None):
        self.values = values
        self.states = states
        self.k = k
        self.bit_width = bit_width
        self.rows = agreement.rows
        self.top1_agreement = agreement.top1 / agreement.rows
        self.topk_agreement = agreement.topk / agreement.rows
        self.top1_accuracy = self.topk_accuracy = None
        if agreement.correct is not None:
            self.top1_accuracy = {t: c[0] / agreement.rows for t, c in agreement.correct.items()}
            self.topk_accuracy = {t: c[1] / agreement.rows for t, c in agreement.correct.items()}

    def worst(self, n: int = 10) -> list:
        """[(name, ValueStats)] of the n values of lowest SQNR, lowest first (nan last)."""
        def key(item):
            s = item[1].sqnr_db
            return (math.isnan(s), s)
        return sorted(self.values.items(), key=key)[:n]

    def to_dict(self) -> dict:
        """Plain Python numbers, strings, dicts: ready for json.dumps."""
        return {"bit_width": self.bit_width, "k": self.k, "rows": self.rows, "top1_agreement": self.top1_agreement,
                "topk_agreement": self.topk_agreement, "top1_accuracy": self.top1_accuracy,
                "topk_accuracy": self.topk_accuracy, "values": {n: asdict(s) for n, s in self.values.items()}}

    def __str__(self):
        head = f"{'value':<40} {'kind':<8} {'op':<18} {'count':>12} {'nonfin':>6} {'mean|d|':>10} {'max|d|':>10} " \
               f"{'rms ref':>10} {'SQNR dB':>8}"
        lines = [head, "-" * len(head)]
        for name, s in self.values.items():
            lines.append(f"{name:<40} {s.kind:<8} {s.op:<18} {s.count:>12d} {s.nonfinite:>6d} {s.mean_abs:>10.4g} "
                         f"{s.max_abs:>10.4g} {s.rms_ref:>10.4g} {s.sqnr_db:>8.2f}")
        bw = "" if self.bit_width is None else f"bit width {self.bit_width}: "
        lines.append(f"{bw}{self.rows} rows, top-1 agreement {self.top1_agreement:.4f}, float top-1 in quantized "
                     f"top-{self.k} {self.topk_agreement:.4f}")
        if self.top1_accuracy is not None:
            for tag in ("float", "quantized"):
                lines.append(f"{tag:>9} model: top-1 accuracy {self.top1_accuracy[tag]:.4f}, top-{self.k} "
                             f"{self.topk_accuracy[tag]:.4f}")
        return "\n".join(lines) + "\n"


def _reiterable(batches, what: str):
    if iter(batches) is batches:
        raise ValueError(f"sweep: {what} is a one-pass iterator; pass a list (it is read once per bit width)")


def sweep(model, calibration_batches, eval_batches, bit_widths=(8, 6, 4), percentile=100.0, weight_bit_widths=None,
          **compare_kw) -> dict:
    """{bit_width: Report}: per bit width `model.quantize_stream(calibration_batches, bit_width,
    percentile)` followed by `model.compare(qmodel, eval_batches, **compare_kw)`.  Both batch
    arguments are read once per bit width, so they must be re-iterable (a list, not a
    generator); `labels` among compare_kw likewise.
    With `weight_bit_widths` (a sequence) the sweep runs over the pairs (activation width a of
    `bit_widths`, weight width w of `weight_bit_widths`) that Model.quantize defines, w <= a, in
    that order, and returns {(a, w): Report}; no such pair at all is an error."""
    _reiterable(calibration_batches, "calibration_batches")
    _reiterable(eval_batches, "eval_batches")
    if compare_kw.get("labels") is not None:
        _reiterable(compare_kw["labels"], "labels")
    widths = list(bit_widths)
    if not widths:
        raise ValueError("sweep: no bit width")
    wwidths = None if weight_bit_widths is None else list(weight_bit_widths)
    for bw in widths + (wwidths or []):
        if isinstance(bw, bool) or not isinstance(bw, (int, np.integer)) or not 1 <= int(bw) <= 16:
            raise ValueError(f"sweep: bit widths are integers in 1..16 (got {bw!r})")
    out = {}
    if wwidths is not None:
        pairs = [(int(a), int(w)) for a in widths for w in wwidths if int(w) <= int(a)]
        if not pairs:
            raise ValueError("sweep: no (bit width, weight bit width) pair with weight bit width <= bit width")
        for a, w in pairs:
            qmodel = model.quantize_stream(calibration_batches, bit_width=a, percentile=percentile, weight_bit_width=w)
            out[(a, w)] = model.compare(qmodel, eval_batches, **compare_kw)
        return out
    for bw in widths:
        qmodel = model.quantize_stream(calibration_batches, bit_width=int(bw), percentile=percentile)
        out[int(bw)] = model.compare(qmodel, eval_batches, **compare_kw)
    return out
