"""Calibration streamed over any number of batches, with optional percentile clipping.

`Model.calibrate` keeps one batch's values in HBM and downloads a min and a max per value.
Here every value owns one row of a device arena, a histogram of float bit patterns plus the
exact key range, into which `nqk_hist_f32` (nqk_hist.hip) accumulates batch after batch; the
arena is downloaded once, at the end.  Everything is integer arithmetic on bit patterns, so
the device result equals the NumPy statement below bit for bit.

Key    key(x) = ~bits if the sign bit is set, else bits | 0x80000000 (uint32): monotone in x
       over all floats, -0.0 just before +0.0.
Bin    bin(x) = key(x) >> HIST_SHIFT: HIST_BINS = 16384 bins of a sign, an exponent and 5
       mantissa bits, 2^-5 wide relative to their values, so no range is needed in advance.
       Low edge: the float of key bin << 18; high edge: the float of key (bin << 18) | 0x3FFFF.
State  int64 [HIST_BINS + 2]: the counts, the smallest key seen (fresh: 0xFFFFFFFF), the
       largest (fresh: 0).
Range  N = total count, tail = int(N * (100.0 - percentile) / 100.0) for percentile in
       (50, 100].  bu / bl = the bins of the elements of ascending rank N - 1 - tail / tail.
       vmax = the exact maximum if bu is the maximum's bin, else bu's high edge; vmin = the
       exact minimum if bl is the minimum's bin, else bl's low edge.  percentile = 100 is the
       exact (min, max) and needs the range entries only.  A NaN among the elements (largest
       key > 0xFF800000 or smallest < 0x007FFFFF) makes both NaN, as nqk_minmax_f32 does.

The histogram is of the union of everything observed under a name: the clip is a percentile
of all batches together, not a mean of per-batch percentiles.
"""
from __future__ import annotations

import numbers

import numpy as np

from . import kernels as K
from .device import DeviceArray, copy_strided
from .kernels import HIST_BINS, HIST_SHIFT
from .tensor import FTensor

STATE_LEN = HIST_BINS + 2
FRESH_MIN_KEY = 0xFFFFFFFF
_EDGE_MASK = (1 << HIST_SHIFT) - 1


def check_percentile(percentile) -> float:
    if isinstance(percentile, bool) or not isinstance(percentile, numbers.Real):
        raise ValueError(f"percentile must be a real number in (50, 100] (got {percentile!r})")
    p = float(percentile)
    if not (50.0 < p <= 100.0):
        raise ValueError(f"percentile must lie in (50, 100] (got {percentile!r})")
    return p


def float_key(arr) -> np.ndarray:
    """uint32 keys of float32 values, in the order of the values."""
    b = np.asarray(arr, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_float(key) -> np.ndarray:
    """The inverse of float_key."""
    k = np.asarray(key, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _key_f32(key: int) -> np.float32:
    """key_float of one Python int (ranges_from_state runs once per value of a model)"""
    return np.uint32(key & 0x7FFFFFFF if key & 0x80000000 else ~key & 0xFFFFFFFF).view(np.float32)


def bin_edges(bin) -> tuple:
    """(lowest, highest) float32 of a bin (arrays for an array of bins)."""
    b = np.asarray(bin, dtype=np.int64)
    if np.any((b < 0) | (b >= HIST_BINS)):
        raise ValueError(f"bin outside 0..{HIST_BINS - 1}")
    lo = (b << HIST_SHIFT).astype(np.uint32)
    lo_f, hi_f = key_float(lo), key_float(lo | np.uint32(_EDGE_MASK))
    return (lo_f[()], hi_f[()]) if lo_f.ndim == 0 else (lo_f, hi_f)


def fresh_state() -> np.ndarray:
    state = np.zeros(STATE_LEN, dtype=np.int64)
    state[HIST_BINS] = FRESH_MIN_KEY
    return state


def host_state(arr, counts: bool = True) -> np.ndarray:
    """The state nqk_hist_f32 leaves after one call on `arr` from a fresh state, in NumPy."""
    keys = float_key(np.asarray(arr, dtype=np.float32).ravel())
    state = fresh_state()
    if keys.size:
        if counts:
            state[:HIST_BINS] = np.bincount(keys >> np.uint32(HIST_SHIFT), minlength=HIST_BINS)
        state[HIST_BINS], state[HIST_BINS + 1] = int(keys.min()), int(keys.max())
    return state


def ranges_from_state(state, percentile=100.0, name: str = "value") -> tuple:
    """(vmin, vmax) as np.float32 from one state (the rule at the top of this module)."""
    p = check_percentile(percentile)
    if not isinstance(state, np.ndarray) or state.shape != (STATE_LEN,) or state.dtype != np.int64:
        raise ValueError(f"state must be int64 [{STATE_LEN}]")
    return _ranges(state, int(state[HIST_BINS]), int(state[HIST_BINS + 1]), p, name)


def _ranges(state, kmin: int, kmax: int, p: float, name: str) -> tuple:
    """ranges_from_state on checked arguments; `state` is not read when p == 100"""
    if kmin > kmax:
        raise ValueError(f"{name}: no element was observed")
    if p < 100.0:
        # the bins in use: a few hundred of the 16384, all between the bins of the two range keys
        first = kmin >> HIST_SHIFT
        used = first + np.flatnonzero(state[first:(kmax >> HIST_SHIFT) + 1])
        if used.size == 0:
            raise ValueError(f"{name}: observed without counts, which percentile {p} needs")
        cum = np.cumsum(state[used])
        total = int(cum[-1])
    if kmax > 0xFF800000 or kmin < 0x007FFFFF:
        return np.float32(np.nan), np.float32(np.nan)
    if p == 100.0:
        return _key_f32(kmin), _key_f32(kmax)
    tail = int(total * (100.0 - p) / 100.0)
    bu = int(used[np.searchsorted(cum, total - 1 - tail, side="right")])
    bl = int(used[np.searchsorted(cum, tail, side="right")])
    if bu != kmax >> HIST_SHIFT:
        kmax = (bu << HIST_SHIFT) | _EDGE_MASK  # the bin's high edge
    if bl != kmin >> HIST_SHIFT:
        kmin = bl << HIST_SHIFT                 # the bin's low edge
    return _key_f32(kmin), _key_f32(kmax)


class Calibrator:
    """Accumulates the state of every named value on the device.

    percentile     in (50, 100]; 100 (the default) is the exact min / max `Model.calibrate` gives
                   and observes without counts.
    clip_weights   False: `percentile` applies to variables only, constants get their exact
                   range; True: constants are clipped too.
    The arena is int64 [rows, HIST_BINS + 2], 128 KiB per value; it grows by doubling.
    """

    def __init__(self, percentile=100.0, clip_weights: bool = False):
        self.percentile = check_percentile(percentile)
        self.clip_weights = bool(clip_weights)
        self._rows: dict[str, int] = {}
        self._exact: set[str] = set()       # names whose range is the exact one (no counts kept)
        self._host: dict[str, list] = {}    # host values: running [min, max]
        self._arena: DeviceArray | None = None

    # ------------------------------------------------------------------ the arena
    @staticmethod
    def _fresh(rows: int) -> DeviceArray:
        arena = DeviceArray((rows, STATE_LEN), np.int64).fill_zero()
        seed = DeviceArray.from_host(np.array([FRESH_MIN_KEY], dtype=np.int64))
        copy_strided(seed, arena, (rows,), (0,), (STATE_LEN,), 0, HIST_BINS)
        return arena

    def reserve(self, rows: int) -> None:
        """Room for `rows` values (observe() calls this with the model's value count)."""
        have = 0 if self._arena is None else self._arena.shape[0]
        if rows <= have:
            return
        arena = self._fresh(max(rows, 2 * have))
        if have:
            copy_strided(self._arena, arena, (have * STATE_LEN,), (1,), (1,))
        self._arena = arena

    def _row(self, name: str) -> DeviceArray:
        row = self._rows.get(name)
        if row is None:
            row = len(self._rows)
            self.reserve(row + 1)
            self._rows[name] = row
        return self._arena.offset_view(row * STATE_LEN, (STATE_LEN,))

    # ------------------------------------------------------------------ observing
    def observe_tensor(self, name: str, tensor, exact: bool = False) -> None:
        """Accumulate a float32 FTensor or DeviceArray under `name`: one kernel, no
        synchronisation, no download.  `exact`: this name takes its exact range whatever the
        percentile (every observation of one name must say the same)."""
        dev = tensor.dev if isinstance(tensor, FTensor) else tensor
        if not isinstance(dev, DeviceArray) or dev.dtype != np.float32:
            raise ValueError(f"{name}: observe_tensor takes an FTensor or a float32 DeviceArray")
        exact = bool(exact) or self.percentile == 100.0
        if name in self._rows and (name in self._exact) != exact:
            raise ValueError(f"{name}: observed both with and without counts")
        if exact:
            self._exact.add(name)
        K.histogram(dev, self._row(name), counts=not exact)

    def observe(self, model) -> None:
        """Every value of `model` after a float forward: FTensors through observe_tensor
        (a Constant only the first time), host values (ITensor) as a running minimum and
        maximum of what Model.calibrate computes for them."""
        from .model import Constant
        self.reserve(len(self._rows) + sum(1 for v in model.values
                                           if isinstance(v.data, FTensor) and v.name not in self._rows))
        for val in model.values:
            t = val.data
            const = isinstance(val, Constant)
            if isinstance(t, FTensor):
                if const and val.name in self._rows:
                    continue
                self.observe_tensor(val.name, t, exact=const and not self.clip_weights)
            else:
                if const and val.name in self._host:
                    continue
                d = t.data
                flat = d.reshape((d.shape[0], -1) if d.shape else (-1,))
                mn, mx = np.mean(flat.min()), np.mean(flat.max())
                seen = self._host.get(val.name)
                self._host[val.name] = [mn, mx] if seen is None else [min(seen[0], mn), max(seen[1], mx)]

    # ------------------------------------------------------------------ results
    def state(self, name: str) -> np.ndarray:
        """int64 [HIST_BINS + 2] of one value, on the host."""
        if name not in self._rows:
            raise KeyError(name)
        return self._row(name).to_host()

    def histogram(self, name: str) -> np.ndarray:
        """int64 [HIST_BINS] counts of one value, on the host (zeros for a name observed
        without counts: percentile 100, or a constant without clip_weights)."""
        return self.state(name)[:HIST_BINS]

    def ranges(self) -> tuple:
        """(vmin, vmax) dicts by value name, shaped like Model.calibrate's, from one download:
        of the whole arena, or of its two range columns when no name keeps counts."""
        vmin, vmax = {}, {}
        n = len(self._rows)
        if n:
            if len(self._exact) == n:
                dev = DeviceArray((n, 2), np.int64)
                copy_strided(self._arena, dev, (n, 2), (STATE_LEN, 1), (2, 1), HIST_BINS, 0)
                keys = dev.to_host()
                states = None
            else:
                states = self._arena.offset_view(0, (n, STATE_LEN)).to_host()
        for name, row in self._rows.items():
            if states is None:
                vmin[name], vmax[name] = _ranges(None, int(keys[row, 0]), int(keys[row, 1]), 100.0, name)
            else:
                state = states[row]
                p = 100.0 if name in self._exact else self.percentile
                vmin[name], vmax[name] = _ranges(state, int(state[HIST_BINS]), int(state[HIST_BINS + 1]), p, name)
        for name, (mn, mx) in self._host.items():
            vmin[name], vmax[name] = mn, mx
        return vmin, vmax
