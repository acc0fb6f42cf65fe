"""nqk_ln_quant on every kernel form against the oracle's LayerNormalization + quantize, byte for
byte, on inputs whose int8 bytes see the last bit of the mean, the variance, 1 / sqrt and the
last multiply-add (tests/_ln_cases.py; their conditions are asserted on the reference without a
GPU by tests/test_ln_cases_ref.py).  There is no tolerance.

The forms are reached through the launcher's own conditions (nqk_fused.hip nqk_ln_quant; no call
reports which one ran, the ids follow those conditions):
* k_ln_quant_lds<8, true, 4> / <4, true, 1> / <2, true, 1>: 768 / 384 / 192 columns, aligned
  operands, |zp| <= 2^20 ("lds");
* the same three with the f64 quantize chain (MQ = false): NQK_LN_F64Q=1 ("lds_f64q"), and in
  "lds" the cases whose zero point is +-(2^20 + 1);
* k_ln_quant_reg<8 | 4 | 2>: NQK_LN_REG=1 ("reg"), and 2^31 bytes of x and more;
* the generic k_ln_quant: every other width; 768 columns when x, gamma or beta is 4 bytes or out
  1 byte off its alignment, and (inside "lds") when the scale is 2^-101 or 2^101.

Every output buffer is prefilled with a sentinel byte and is one row and 64 bytes longer than the
rows the call may write: what lies outside them must keep the sentinel."""
import ctypes

import numpy as np
import pytest

import _ln_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
FORMS = {"lds": {}, "lds_f64q": {"NQK_LN_F64Q": "1"}, "reg": {"NQK_LN_REG": "1"}}


def _set_env(monkeypatch, env):
    for k in ("NQK_LN_REG", "NQK_LN_F64Q"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _upload(host, byte_offset):
    """A device copy of `host` that starts byte_offset bytes past a 256-byte-aligned address."""
    from numpy_quant.device import DeviceArray
    raw = np.zeros(host.nbytes + byte_offset, np.uint8)
    raw[byte_offset:] = np.ascontiguousarray(host).view(np.uint8).ravel()
    dev = DeviceArray.from_host(raw)
    assert dev.ptr % 256 == 0
    return dev, ctypes.c_void_p(dev.ptr + byte_offset)


def _run(d, rows, off=None):
    """nqk_ln_quant on the first `rows` rows of case d; off: byte offsets of x, gamma, beta, out."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    off = dict(dict(x=0, gamma=0, beta=0, out=0), **(off or {}))
    cols = d["x"].shape[1]
    keep = [_upload(d["x"][:rows], off["x"]), _upload(d["gamma"], off["gamma"]), _upload(d["beta"], off["beta"])]
    n = rows * cols
    out = DeviceArray.from_host(np.full(off["out"] + n + cols + 64, SENTINEL, np.int8))
    _lib.call("nqk_ln_quant", keep[0][1], keep[1][1], keep[2][1], ctypes.c_void_p(out.ptr + off["out"]), rows, cols,
              d["eps"], float(d["scale"]), d["zp"], d["bw"])
    got = out.to_host()
    o = off["out"]
    assert (got[:o] == SENTINEL).all() and (got[o + n:] == SENTINEL).all(), "bytes outside the rows were written"
    return got[o:o + n].reshape(rows, cols)


def _check(d, rows, off=None):
    got, ref = _run(d, rows, off), d["ref"][:rows]
    if d["finite"] is not None:   # kind f: rows with an inf or a NaN are out of contract
        got, ref = got[d["finite"][:rows]], ref[d["finite"][:rows]]
    bad = got != ref
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} bytes differ, in rows "
                           f"{np.flatnonzero(bad.any(axis=1))[:8].tolist()}")


def _params(cases):
    return [pytest.param(c, id=C.case_id(c)) for c in cases]


@pytest.mark.parametrize("case", _params([c for cols in C.TREE_COLS for c in C.cases_for(cols)]))
@pytest.mark.parametrize("form", list(FORMS))
def test_tree_forms_equal_the_reference(form, case, monkeypatch):
    """768, 384 and 192 columns on the LDS form with the magic-number quantize, with the f64
    quantize, and on the register form: every case of tests/_ln_cases.py."""
    _set_env(monkeypatch, FORMS[form])
    d = C.ln_case(case)
    _check(d, case.rows)


def _row_counts(cols):
    rw = 32 * 96 // cols                     # rows per wave: 4, 8, 16
    wg = rw * (4 if cols == 768 else 1)      # rows per workgroup of the LDS form
    return sorted({1, rw - 1, rw, rw + 1, wg + 1, 67})


@pytest.mark.parametrize("cols,rows", [(cols, rows) for cols in C.TREE_COLS for rows in _row_counts(cols)])
@pytest.mark.parametrize("form", list(FORMS))
def test_tree_forms_at_every_row_count(form, cols, rows, monkeypatch):
    """One row, one less than a wave's rows, a wave's, one more, one more than a workgroup's, and
    67: every row of kinds a and b differs from every other, so a swapped row shows."""
    _set_env(monkeypatch, FORMS[form])
    for kind in ("a", "b"):
        _check(C.ln_case(C.L(kind, cols, 67, 1e-12)), rows)


@pytest.mark.parametrize("case", _params([c for cols in C.GENERIC_COLS for c in C.cases_for(cols, "abdef")]))
def test_generic_kernel_equals_the_reference(case, monkeypatch):
    """k_ln_quant at the pairwise plan's edges (below and at 8 columns, one leaf of up to 128, the
    first split at 129, leaves with a tail), ViT-L's and ViT-H's 1024 and 1280, and 8192, the
    longest row the plan holds (140 352 bytes of dynamic LDS)."""
    _set_env(monkeypatch, {})
    _check(C.ln_case(case), case.rows)


@pytest.mark.parametrize("case", _params([C.L("a", 768), C.L("b", 768), C.L("bm", 768, 67, 1e-5), C.L("c", 768),
                                          C.L("c", 768, 67, 1e-5, 1), C.L("e", 768, C.E_ROWS), C.L("f", 768)]))
@pytest.mark.parametrize("operand,nbytes", [("x", 4), ("gamma", 4), ("beta", 4), ("out", 1)])
def test_generic_kernel_takes_unaligned_operands_at_768_columns(operand, nbytes, case, monkeypatch):
    """x, gamma or beta 4 bytes off 16-byte alignment, or out 1 byte off 4-byte alignment: the
    tree forms' vector accesses are not possible and the generic kernel runs ViT-Base's width."""
    _set_env(monkeypatch, {})
    _check(C.ln_case(case), case.rows, {operand: nbytes})


def test_generic_kernel_with_more_rows_than_its_grid(monkeypatch):
    """4 * 262144 + 5 rows of 8 columns: the grid holds 262144 workgroups of four rows, so every wave
    walks a second row and five rows a third."""
    _set_env(monkeypatch, {})
    case = C.L("a", 8, 4 * 262144 + 5)
    _check(C.ln_case(case), case.rows)


def test_the_2_31_byte_switch_from_the_lds_form_to_the_register_form(monkeypatch):
    """The LDS form addresses x by 32-bit buffer offsets; from rows * cols * 4 = 2^31 on the launcher
    takes the register form.  699 050 rows of 768 columns are 2^31 - 2048 bytes, the most the LDS
    form takes; 699 051 are 2^31 + 1024.  x is a 4099-row block of kind a repeated on the device (2.1 GB
    of x, 0.5 GB of out; nothing large is uploaded)."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray, copy_strided
    _set_env(monkeypatch, {})
    block, cols, total = 4099, 768, 699051
    assert (total - 1) * cols * 4 == 2 ** 31 - 2048 and total * cols * 4 == 2 ** 31 + 1024
    d = C.ln_case(C.L("a", cols, block))
    src, g, b = (DeviceArray.from_host(d[k]) for k in ("x", "gamma", "beta"))
    x = DeviceArray((total, cols), np.float32)
    whole, rest = divmod(total, block)
    copy_strided(src, x, (whole, block * cols), (0, 1), (block * cols, 1))
    copy_strided(src, x, (rest, cols), (cols, 1), (cols, 1), dst_offset=whole * block * cols)
    out = DeviceArray((total * cols + cols + 64,), np.int8)
    for rows in (total - 1, total):
        _lib.call("nqk_memset", out.vp, SENTINEL, out.nbytes)
        _lib.call("nqk_ln_quant", x.vp, g.vp, b.vp, out.vp, rows, cols, d["eps"], float(d["scale"]), d["zp"], d["bw"])
        got = out.to_host()
        assert (got[rows * cols:] == SENTINEL).all(), rows
        tiles = got[:whole * block * cols].reshape(whole, block, cols)
        bad = (tiles != d["ref"][None]).any(axis=(1, 2))
        assert not bad.any(), (rows, np.flatnonzero(bad)[:8].tolist())
        tail = got[whole * block * cols:rows * cols].reshape(-1, cols)
        np.testing.assert_array_equal(tail, d["ref"][:len(tail)], err_msg=str(rows))


# ------------------------------------------------------------------------------- argument checks
def _ln_args(d, rows=3, cols=None, bw=8, null=None):
    from numpy_quant.device import DeviceArray
    keep = [DeviceArray.from_host(d[k]) for k in ("x", "gamma", "beta")] + [DeviceArray(d["x"].shape, np.int8)]
    ptrs = [None if k == null else a.vp for k, a in zip(("x", "gamma", "beta", "out"), keep)]
    cols = d["x"].shape[1] if cols is None else cols
    return keep, ptrs + [rows, cols, d["eps"], float(d["scale"]), d["zp"], bw]


@pytest.mark.parametrize("kw,message", [
    (dict(cols=8193), "row length not supported by the pairwise-sum plan"),
    (dict(cols=0), "nqk_ln_quant: cols <= 0"),
    (dict(cols=-768), "nqk_ln_quant: cols <= 0"),
    (dict(bw=0), "nqk_ln_quant: bit_width outside 1..8"),
    (dict(bw=9), "nqk_ln_quant: bit_width outside 1..8"),
    (dict(bw=16), "nqk_ln_quant: bit_width outside 1..8"),
    (dict(null="x"), "nqk_ln_quant: null"),
    (dict(null="gamma"), "nqk_ln_quant: null"),
    (dict(null="beta"), "nqk_ln_quant: null"),
    (dict(null="out"), "nqk_ln_quant: null"),
])
def test_ln_quant_refuses_bad_arguments(kw, message):
    from numpy_quant import _lib
    lib = _lib.load()
    _lib.ensure_init()
    d = C.ln_case(C.L("a", 8192, 67))   # (8193 columns of it would still lie inside the buffers)
    keep, args = _ln_args(d, **kw)
    assert lib.nqk_ln_quant(*args) != 0
    assert message in lib.nqk_last_error().decode(), lib.nqk_last_error()
    for rows in (0, -1):   # nothing to do: no error, whatever the other arguments are
        keep, args = _ln_args(d, rows=rows, **kw)
        assert lib.nqk_ln_quant(*args) == 0


@pytest.mark.parametrize("kw,message", [
    (dict(cols=8193), "row length not supported by the pairwise-sum plan"),
    (dict(cols=0), "nqk_softmax_quant: cols <= 0"),
    (dict(bw=0), "nqk_softmax_quant: bit_width outside 1..8"),
    (dict(bw=9), "nqk_softmax_quant: bit_width outside 1..8"),
    (dict(null="x"), "nqk_softmax_quant: null"),
    (dict(null="out"), "nqk_softmax_quant: null"),
    (dict(ldo=7), "nqk_softmax_quant: ldo < cols"),
])
def test_softmax_quant_refuses_bad_arguments(kw, message):
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    lib = _lib.load()
    _lib.ensure_init()
    x = DeviceArray.from_host(np.zeros((3, 8193), np.float32))
    out = DeviceArray((3, 8208), np.int8)

    def args(rows):
        cols = kw.get("cols", 8)
        return [None if kw.get("null") == "x" else x.vp, None if kw.get("null") == "out" else out.vp, None, rows, cols,
                kw.get("ldo", max(cols, 1)), 1.0 / 255, -128, kw.get("bw", 8)]
    assert lib.nqk_softmax_quant(*args(3)) != 0
    assert message in lib.nqk_last_error().decode(), lib.nqk_last_error()
    assert lib.nqk_softmax_quant(*args(0)) == 0
