"""Every fused kernel of the forward's hot path against a plain NumPy reference built from the
pinned oracle (tests/_fused_ref.py, itself pinned to the oracle's node loop by
tests/test_fused_ref.py): nqk_qgemm_fused on each of its kernel routes (forced with the
environment switches and asserted with nqk_qgemm_last_kernel) for the QKV / RESID / RESID + LN /
GELU / SCORES / PV epilogues, nqk_softmax_quant, nqk_transpose_pad_i8 and nqk_attention_fused.
Every output is compared bit for bit (f32 as int32 views); there is no tolerance.

The inputs (tests/_fused_cases.py; their conditions are asserted on the reference there and
run without a GPU by tests/test_fused_ref_inputs.py) sit where random data never gets:
accumulators AT the f32-exactness bound 2^14 K + cmax |zpa| (or 128 L1 + cmax |zpa|) just below
and just above 2^24, exact rounding ties, output zero points at +-2^20 and one beyond, zpa up
to 2^20 (the non-int32 zero-point algebra), bit widths 2 and 3, small output scales, and for
attention the zero-point limits of include/nqk.h with flat, peaked and -86.5-straddling rows.
Shapes are the smallest that reach each route's mechanisms (3-, 12-, 48-step k loops, ragged
tiles against 128 / 256 rows, an image boundary inside a tile), not the workload's."""
import ctypes

import numpy as np
import pytest

import _fused_cases as F
from _fused_gpu import attn_params, check_three_launch_pieces, head_mismatches, pv_gemm

pytestmark = pytest.mark.gpu

_SWITCHES = ("NQK_NO_PROJ", "NQK_NO_F32X", "NQK_NO_PG", "NQK_PG_NORESID", "NQK_PROJ_RESID", "NQK_PROJ_GELU", "NQK_PG_WM",
             "NQK_NO_GELU_FILTER", "NQK_NO_GLUT", "NQK_GLUT_NO1", "NQK_GLUT_NOWIDE", "NQK_NO_L1",
             "NQK_PROJ_CUS", "NQK_LN_F64Q", "NQK_NO_BPACK", "NQK_NO_B4", "NQK_XCDS",
             "NQK_PG_NOS8")
_PG = {"NQK_NO_PROJ": "1", "NQK_PG_WM": "1"}
_PROJ = {"NQK_PROJ_RESID": "1", "NQK_PROJ_GELU": "1"}
# route: (nqk_qgemm_last_kernel id, environment, weight operand, k_pg image, GELU table)
ROUTES = {
    "epi": (0, {}, "plain", None, False),                    # no precomputed column sums: k_qgemm_epi
    "big": (1, {"NQK_NO_PROJ": "1"}, "plain", None, False),
    "big_pack": (1, {"NQK_NO_PROJ": "1"}, "pack", None, False),
    "big_pack4": (1, {"NQK_NO_PROJ": "1"}, "pack4", None, False),
    "proj": (3, _PROJ, "pack", None, False),
    "proj8": (3, dict(_PROJ, NQK_PROJ_CUS="8"), "pack", None, False),
    "proj_fb": (1, _PROJ, "pack", None, False),              # offered to k_proj, which must decline
    "pg": (4, _PG, "pack", "pg", False),
    "pg_fb": (1, _PG, "pack", "pg", False),                  # offered to k_pg, which must decline
    "pg4": (4, _PG, "pack4", "pg4", False),
    "pg_wm2": (5, {"NQK_NO_PROJ": "1", "NQK_PG_WM": "2"}, "pack", "pg", False),
    "glut": (6, _PG, "pack", "pg", True),
    "glut_wm2": (7, {"NQK_NO_PROJ": "1", "NQK_PG_WM": "2"}, "pack", "pg", True),
    "nolut": (4, _PG, "pack", "pg", True),                   # nqk_gelu_lut_build returns n = 0: the filtered chain
}


def _params(cases):
    return [pytest.param(c, r, id="-".join(map(str, c)) + "-" + r) for c, routes in cases for r in routes]


def _run_gemm(c, route, monkeypatch, extra_env=None):
    """Runs case c on `route` (setup: tests/_fused_gpu.py); returns (kernel id, expected id, outputs)."""
    from _fused_gpu import build_gelu_lut, fused_gemm
    want, env, wkind, pgkind, table = ROUTES[route]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env, **(extra_env or {})).items():
        monkeypatch.setenv(k, v)
    d = F.gemm_case(c)
    if np.abs(d["col"] * c.zpa).max() >= 2 ** 31:  # no int32 column term: the persistent kernels cannot run
        assert wkind in ("plain", "pack") and pgkind is None
    lut = ln = None
    if table:
        lut = build_gelu_lut(d["s_out"][0], d["zp_out"][0], c.bw)
        if route == "nolut":
            assert lut[2] == 0, lut[2]
            lut = None
        else:
            assert lut[2] > 0, lut[2]
            if lut[2] > 512:  # only the 256 x 256-tile form holds such a table
                assert c.M >= 256, "test design: a table of more than 512 entries needs M >= 256"
                want = 7
    if c.epi == "resid_ln":
        ln = dict(gamma=d["gamma"], beta=d["beta"], eps=d["ln_eps"], scale=d["ln_scale"], zp=d["ln_zp"])
    got, outs, _ = fused_gemm("resid" if c.epi == "resid_ln" else c.epi, d["a"], d["bt"], zpa=c.zpa, bias_h=d["bias"],
                              resid_h=d["resid"], s_acc=d["s_acc"], s_out=d["s_out"], zp_out=d["zp_out"], bw=c.bw,
                              weights=wkind, pg=pgkind, use_col=route != "epi", col_l1max=d["col_l1max"], tokens=F.T_TOK,
                              ln=ln, lut=lut)
    return got, want, outs


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _check_gemm(c, route, monkeypatch, extra_env=None):
    got, want, outs = _run_gemm(c, route, monkeypatch, extra_env)
    assert got == want, f"route {route}: kernel {got}, expected {want}"
    ref = F.gemm_case(c)["ref"]
    bad = [int((_bits(o) != _bits(np.asarray(r, o.dtype).reshape(o.shape))).sum()) for o, r in zip(outs, ref)]
    assert bad == [0] * len(ref), (bad, [o.size for o in outs])
    return outs


@pytest.mark.parametrize("case,route", _params(F.ROUTE_CASES))
def test_every_route_equals_the_reference(case, route, monkeypatch):
    """Random operands with small output scales (many values next to rounding boundaries: the
    rounding filters' and the GELU filter's exact fallbacks, the GELU table), every epilogue on
    every kernel route that takes it; bit widths 2, 3 (4 with the nibble-packed weight images);
    output zero points 0, +-2^20 and +-(2^20 + 1) (the last pair leaves the f32 path: the
    persistent kernels must decline, *_fb); zpa in {0, -128, 127, 2^20} (2^20: the non-int32
    zero-point algebra; no int32 column term exists, so only routes 0 - 2)."""
    _check_gemm(case, route, monkeypatch)


@pytest.mark.parametrize("case,route", _params(F.EXTREME_CASES))
def test_accumulators_at_the_f32_exactness_bound(case, route, monkeypatch):
    """Rows whose |acc - col zpa| EQUALS abound + cmax |zpa|, the quantity the dispatch compares
    with 2^24 to take the f32 epilogue arithmetic: 16 515 072 (K = 768, zpa = 40) and 16 773 120
    (K = 3072 through col_l1max, zpa = 2) are below it, zpa = 43 / 140 / 3 above (odd values there
    are not f32 numbers: a kernel that took the f32 path anyway would round them)."""
    _check_gemm(case, route, monkeypatch)


@pytest.mark.parametrize("case,route", _params(F.TIES_CASES))
def test_exact_ties_round_half_even(case, route, monkeypatch):
    """Power-of-two scales (2^-13, 2^-6) and biases that are multiples of s_acc: zp + y / s_out is
    exact, and a half-integer for 0.7 - 0.8 % of the elements, with even and odd floors."""
    _check_gemm(case, route, monkeypatch)


@pytest.mark.parametrize("case,route", _params(F.LN_CASES))
@pytest.mark.parametrize("f64q", [False, True])
def test_fused_layernorm_equals_the_reference(case, route, f64q, monkeypatch):
    """k_qgemm_big<RESID, LN> at N = 192: the f32 rows and the int8 LayerNorm output against the
    oracle's LayerNormalization + quantize; bit widths 2, 3, 8; ln_zp at +-2^20 (the magic-number
    quantize's limit) and one beyond (the f64 quantize), and the f64 quantize forced."""
    _check_gemm(case, route, monkeypatch, {"NQK_LN_F64Q": "1"} if f64q else None)


@pytest.mark.parametrize("case,route", _params(F.LN_ROW_CASES))
@pytest.mark.parametrize("f64q", [False, True])
def test_fused_layernorm_on_rows_that_show_its_last_bits(case, route, f64q, monkeypatch):
    """The same kernel with a = 0, zpa = 0 and no bias, so that its f32 row IS the residual row:
    the ill-conditioned, one-ulp-resolving and exact-tie rows of tests/_ln_cases.py at 192 columns
    (random residual rows do not see the order of the epilogue's sums, its 1 / sqrt or a fused
    last step: tests/test_ln_cases_ref.py)."""
    _check_gemm(case, route, monkeypatch, {"NQK_LN_F64Q": "1"} if f64q else None)


@pytest.mark.parametrize("case,route", _params(F.PERSIST_CASES))
def test_persistent_routes_walk_three_tiles(case, route, monkeypatch):
    """Some workgroup walks at least three tiles and the last row tile is ragged, at the narrowest
    N each route takes (one column tile: N = 64 for k_pg's GELU, 256 for k_proj).  A grid of G
    workgroups over nt tiles gives some workgroup three as soon as nt >= 2 G + 1:
    * k_pg, 128-row tiles: G = 2 workgroups per CU = 512 on the MI355X's 256 CUs (pg_launch:
      slots), so nt = 1025 row tiles: M = 1024 * 128 + 77;
    * k_pg, 256-row tiles (NQK_PG_WM=2): G = 256, nt = 513: M = 512 * 256 + 77;
    * k_proj: G = min(nt, CUs), or NQK_PROJ_CUS of them (launch_proj): with NQK_PROJ_CUS=8,
      nt = 17: M = 16 * 256 + 77 (its residual form needs M % 256 == 0, so the GELU form).
      The launcher reads the switch on every call, so earlier k_proj launches of the process do not
      matter: 8 workgroups over 17 tiles in 8 bands, the last band's workgroup walks tiles 14, 15 and
      the ragged 16.
    On a device with fewer CUs the workgroups walk more tiles, never fewer."""
    _check_gemm(case, route, monkeypatch)


# ------------------------------------------------------------------------------- XCD tile order
@pytest.mark.parametrize("xcds", ["1", "3", "4", "6"])
@pytest.mark.parametrize("route", ["pg", "big"])
def test_gemm_tile_order_for_any_xcd_count(route, xcds, monkeypatch):
    """k_pg's band walk and k_qgemm_big's remap (nqk_xcd.h) with the XCD count overridden
    (NQK_XCDS): 15 tiles (5 row panels x 3 column tiles), every one computed exactly once."""
    _check_gemm(F.GemmCase("qkv", 197 * 3, 576, 192, "small"), route, monkeypatch, {"NQK_XCDS": xcds})


@pytest.mark.parametrize("xcds", ["1", "3", "4", "6"])
@pytest.mark.parametrize("mfma", ["32", "16"])
def test_embed_q_tile_order_for_any_xcd_count(mfma, xcds, monkeypatch):
    """nqk_embed_q (both MFMA forms, 3 images, N = 192: 5 x 3 tiles) with NQK_XCDS in {1, 3, 4, 6}
    equals its NQK_EMBED_NOXCD=1 output and the im2col chain nqk_patchify_dequant +
    nqk_sgemm_embed (pinned to the reference's fconv2d by test_gpu_kernels).  Before nqk_xcd.h,
    k_embed_q placed a block in its band by b / 8 whatever the XCD count: with 4 XCDs some tiles
    were computed twice and others never."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray, permute
    from numpy_quant.plan import embed_weight_image
    monkeypatch.setenv("NQK_EMBED_MFMA", mfma)
    n, h, w, N, zp = 3, 224, 224, 192, -5
    rng = np.random.default_rng(1000 + N)
    q = rng.integers(-128, 128, size=(n, 3, h, w), dtype=np.int8)
    s = np.float32(0.0173)
    W = (0.05 * rng.standard_normal((N, 3, 16, 16))).astype(np.float32)
    hw = (h // 16) * (w // 16)
    bias = DeviceArray.from_host((0.1 * rng.standard_normal(N)).astype(np.float32))
    cls = DeviceArray.from_host(rng.standard_normal(N).astype(np.float32))
    pos = DeviceArray.from_host(rng.standard_normal((hw + 1, N)).astype(np.float32))
    Wd, qd = DeviceArray.from_host(W), DeviceArray.from_host(q)
    wm = permute(Wd, [2, 3, 1, 0]).reshape((768, N))
    cols = DeviceArray((n * hw, 768), np.float32)
    _lib.call("nqk_patchify_dequant", qd.vp, cols.vp, n, 3, h, w, 16, 16, float(s), zp)
    ref = DeviceArray((n, hw + 1, N), np.float32)
    _lib.call("nqk_sgemm_embed", cols.vp, wm.vp, bias.vp, cls.vp, pos.vp, ref.vp, n, hw, N, 768)
    wt = embed_weight_image(Wd, N, 768)
    outs = []
    for env in ({"NQK_EMBED_NOXCD": "1"}, {"NQK_XCDS": xcds}):
        monkeypatch.delenv("NQK_EMBED_NOXCD", raising=False)
        monkeypatch.delenv("NQK_XCDS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = DeviceArray((n, hw + 1, N), np.float32)
        out.fill_zero()
        _lib.call("nqk_embed_q", qd.vp, float(s), zp, wt.vp, bias.vp, cls.vp, pos.vp, out.vp, n, 3, h, w, 16, 16, N)
        outs.append(out.to_host().view(np.int32))
    r = ref.to_host().view(np.int32)
    assert int((outs[0] != r).sum()) == 0, "grid order vs the im2col chain"
    assert int((outs[1] != r).sum()) == 0, f"NQK_XCDS={xcds} vs the im2col chain"
    np.testing.assert_array_equal(outs[1], outs[0])


# ------------------------------------------------------------------------------- attention
_KERNELS = {"k_attention": ("0", "4"), "k_attn16": ("1", "4"), "k_attn16_nw5": ("1", "5")}


def _attn_ids():
    out = []
    # k_attn16 takes T = 197 on the f32-exact (FAST) path only: other T, and zero points beyond
    # 64 (2^14 + 128 (|zq| + |zk|) + |zq zk|) < 2^24 (every "lim" set), run k_attention whatever the
    # switches say, so those cases carry one id.  "fast": the largest zero points k_attn16 itself takes.
    for c in F.ATTN_CASES:
        for kern in (_KERNELS if c.T == 197 and c.zset in ("std", "fast") and c.bw == 8 else ["k_attention"]):
            out.append(pytest.param(c, kern, id="-".join(map(str, c)) + "-" + kern))
    return out


@pytest.mark.parametrize("case,kern", _attn_ids())
def test_attention_fused_equals_the_reference(case, kern, monkeypatch):
    """nqk_attention_fused (k_attention, k_attn16 with four and five waves) against the
    composition SCORES -> softmax_quant -> PV of the NumPy reference, B.H = 6: per head random,
    flat, peaked, -86.5-straddling, all -128 and all 127 rows; zero points at the limits of
    include/nqk.h (|zq|, |zk| = 4096, |zp_p|, |zv| = 1024: k_attention's exact form, the only
    kernel that takes them) and at the edge of the FAST path's own bound (|zq|, |zk| = 380,
    zv = 180: 16 516 096 / 16 382 520 of 2^24, all three kernels); s_p = 1 / 255 and 8e-5 with
    zp_p = -142.  (No call reports which attention kernel ran; the ids follow the launcher's
    conditions in nqk_attn.hip.)"""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    monkeypatch.setenv("NQK_ATTN16", _KERNELS[kern][0])
    monkeypatch.setenv("NQK_ATTN16_NW", _KERNELS[kern][1])
    d = F.attn_case(case)
    T, BH = case.T, F.B_ATT * F.H_ATT
    dq, dk, dv = (DeviceArray.from_host(d[x].reshape(BH * T, F.DH)) for x in "qkv")
    ctx = DeviceArray((F.B_ATT, T, F.H_ATT * F.DH), np.int8)
    ctx.fill_zero()
    a = attn_params(d, F.H_ATT, T, case.bw)
    _lib.call("nqk_attention_fused", dq.vp, dk.vp, dv.vp, ctx.vp, BH, ctypes.byref(a))
    got = ctx.to_host()
    assert int((got != d["ctx"]).sum()) == 0, head_mismatches(got, d["ctx"], T)


@pytest.mark.parametrize("case", F.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_three_launch_pieces_equal_the_reference(case):
    """The SCORES and PV epilogues (k_qgemm_epi, batched, row / column / K-constant zero-point
    terms), nqk_softmax_quant and nqk_transpose_pad_i8 with their int64 sums, each fed with the
    reference's own input of that stage."""
    check_three_launch_pieces(case)


def test_pv_exact_ties():
    """EPI_PV with power-of-two scales: 0.75 % of the elements are exact ties (even and odd floors)."""
    d = F.pv_ties_case()
    np.testing.assert_array_equal(pv_gemm(d, d["p"], d["vt"], F.T_TOK, 208, 8), d["ctx"])


@pytest.mark.parametrize("field,value", [("zq", 4097), ("zq", -4097), ("zk", 4097), ("zk", -4097), ("zp_p", 1025),
                                         ("zp_p", -1025), ("zv", 1025), ("zv", -1025)])
def test_attention_rejects_zero_points_beyond_the_limits(field, value):
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    d = F.attn_case(F.AttnCase(17, "std", "unit"))
    T, BH = 17, F.B_ATT * F.H_ATT
    dq, dk, dv = (DeviceArray.from_host(d[x].reshape(BH * T, F.DH)) for x in "qkv")
    ctx = DeviceArray((F.B_ATT, T, F.H_ATT * F.DH), np.int8)
    a = attn_params(d, F.H_ATT, T, 8)
    setattr(a, field, value)
    with pytest.raises(_lib.NQKError):
        _lib.call("nqk_attention_fused", dq.vp, dk.vp, dv.vp, ctx.vp, BH, ctypes.byref(a))
