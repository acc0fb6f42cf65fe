"""tests/_sgemm_ref.py (the exact restatement of np.matmul for float32 matrices that the GPU tests
compare nqk_sgemm with) against np.matmul itself, bit for bit, on a host whose OpenBLAS runs the
SkylakeX kernels (scipy-openblas 0.3.29, the reference's): every regime, both level-3 drivers,
every K-block edge, every column and row class of the small-matrix kernels, the transposed form,
edge values.  No GPU."""
import numpy as np
import pytest

import _sgemm_ref as R
from numpy_quant import kernels as KM
from oracle import openblas_order as OB


def _skylakex():
    threadpoolctl = pytest.importorskip("threadpoolctl")
    info = [i for i in threadpoolctl.threadpool_info() if i.get("internal_api") == "openblas"]
    if not info or info[0].get("architecture") != "SkylakeX":
        pytest.skip("OpenBLAS does not run its SkylakeX kernels on this host")
    return threadpoolctl


def _rows():
    """(M, N, K, transb, threads, edge values)"""
    t = []
    # K-block edges under the threaded driver (8 threads, 50 x 50) and the single-thread one
    for K in (447, 448, 449, 450, 895, 896, 897, 898, 1343, 1345):
        t.append((50, 50, K, False, 8, K in (450, 897)))
        t.append((50, 50, K, False, 1, False))
    t += [(130, 70, 500, False, 8, False), (300, 7, 769, False, 8, True), (7, 300, 769, False, 16, False),
          (40, 64, 1000, False, 16, False), (64, 64, 898, False, 16, True), (20, 20, 2501, False, 8, False)]
    # several threads, yet the single-thread driver: m below 32 and n below 17, or too few products per thread
    t += [(16, 16, 3907, False, 8, False), (10, 10, 10001, False, 8, False), (16, 31, 4101, False, 16, False),
          (17, 8, 8201, False, 8, False), (8, 32, 4101, False, 8, False),
          (8, 40, 3201, False, 2, False), (8, 40, 3201, False, 3, False)]
    # the regime boundary from both sides
    t += [(25, 40, 1000, False, 8, False), (25, 40, 1001, False, 8, False), (10, 10, 10000, False, 8, False),
          (100, 100, 100, False, 8, True), (101, 100, 100, False, 8, False), (101, 99, 100, False, 16, False)]
    # small regime: every N % 16 (a row tail of 2 and of 1), K on both sides of 32, no K blocking
    for N in range(16, 32):
        t.append((6, N, 40, False, 8, False))
    for N in range(2, 16):
        t.append((5, N, 77, False, 1, False))
    t += [(6, 7, 77, False, 8, True), (7, 24, 40, False, 8, True), (6, 17, 31, False, 8, False), (6, 24, 32, False, 8, False), (7, 9, 897, False, 8, False),
          (16, 16, 1000, False, 8, False), (5, 1000, 64, False, 16, False), (64, 2, 64, False, 8, False),
          (20, 100, 77, False, 8, True), (33, 33, 100, False, 8, False), (2, 2, 449, False, 8, False)]
    # row counts 1 .. 17 against a 2-column and a 4 + 2 + 1-column tail
    for M in range(1, 18):
        t.append((M, 18, 33, False, 8, False))
        t.append((M, 7, 48, False, 16, False))
    # B a transposed view: the small kernels (M N <= 1200, K >= 32), their refusals, the level-3 regime
    t += [(16, 16, 1000, True, 8, False), (6, 7, 64, True, 8, True), (30, 40, 100, True, 16, False),
          (7, 7, 333, True, 1, False), (6, 6, 32, True, 8, False), (13, 3, 50, True, 8, False),
          (3, 13, 50, True, 8, False), (2, 600, 64, True, 8, False), (8, 11, 40, True, 8, False),
          (30, 41, 100, True, 8, False), (20, 20, 31, True, 8, False), (100, 100, 100, True, 8, False),
          (2, 601, 64, True, 8, False), (50, 50, 449, True, 8, False), (64, 64, 897, True, 16, True),
          (16, 16, 3907, True, 8, False)]
    return t


TABLE = _rows()


def _operands(M, N, K, transb, threads, edge):
    blocks = R.k_blocks(K, R.gemm_driver(M, N, K, threads)) if R.gemm_regime(M, N, K, transb) == "level3" else [K]
    if edge:
        return R.edge_operands(M, N, K, M * 1000 + N * 10 + K, blocks)
    rng = np.random.default_rng(M * 1000 + N * 10 + K)
    return rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)


def _reference(a, b, transb, threads):
    M, N = a.shape[0], b.shape[1]
    if M >= 2 and N >= 2:
        return R.sgemm_ref(a, b, transb, threads)
    assert M == 1 and N >= 2 and not transb  # a one-row product: GEMV-N (pinned by tests/test_host.py)
    return OB.sgemv_n(b, a[0], threads)[None, :]


def test_table_reaches_every_regime_and_driver():
    seen = set()
    for M, N, K, transb, threads, _ in TABLE:
        if M < 2:
            continue
        reg = R.gemm_regime(M, N, K, transb, threads)
        seen.add((reg, transb, R.gemm_driver(M, N, K, threads) if reg == "level3" else None))
    for transb in (False, True):
        assert ("small", transb, None) in seen
        for drv in R.DRIVERS:
            assert ("level3", transb, drv) in seen, (transb, drv)
    assert {r[4] for r in TABLE} >= {1, 8, 16}
    small = [r for r in TABLE if r[0] >= 2 and R.gemm_regime(*r[:4]) == "small"]
    assert {r[1] % 16 for r in small if not r[3]} == set(range(16))
    assert {r[0] for r in TABLE} >= set(range(1, 18))
    # what kernels.gemm_restated declines: at most a quarter of the small rows, none of the level-3 ones
    declined = [r for r in TABLE if r[0] >= 2 and not KM.gemm_restated(*r[:4])]
    assert all(R.gemm_regime(*r[:4]) == "small" for r in declined)
    assert 4 * len(declined) <= len(small)


@pytest.mark.parametrize("M,N,K,transb,threads,edge", TABLE)
def test_sgemm_ref_equals_numpy_matmul(M, N, K, transb, threads, edge):
    threadpoolctl = _skylakex()
    a, b = _operands(M, N, K, transb, threads, edge)
    w = np.ascontiguousarray(b.T)
    with threadpoolctl.threadpool_limits(limits=threads, user_api="blas"), np.errstate(all="ignore"):
        want = np.matmul(a, w.T) if transb else np.matmul(a, b)
    got = _reference(a, b, transb, threads)
    same = R.same_bits(got, want)
    restated = KM.gemm_restated(M, N, K, transb) if M >= 2 else KM.one_row_restated(N, K)
    assert restated == bool(same.all()), f"{int((~same).sum())} of {same.size} differ; first at {np.argwhere(~same)[:4].tolist()}"
    if edge:
        assert np.isnan(want).any() and np.isinf(want).any()
        sub = np.abs(want[np.isfinite(want)])
        assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any()


def test_fma32_is_correctly_rounded():
    """fma32 against exact rational arithmetic on the cases a double rounding gets wrong (a sum that
    lies a hair off an f32 midpoint), subnormal results, overflow and the invalid operations."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(np.float32)
    # c = an f32 midpoint's neighbourhood: 1 + 2^-24 is a midpoint of f32; the product adds 2^-60
    a[:4] = np.float32(2.0 ** -30)
    b[:4] = np.float32([2.0 ** -30, -2.0 ** -30, 2.0 ** -40, -2.0 ** -40])
    c[:4] = np.float32(1.0)
    a[4:8] = np.float32(1.0 + 2.0 ** -12)
    b[4:8] = np.float32(1.0 + 2.0 ** -12)      # product 1 + 2^-11 + 2^-24: a midpoint plus c's hair
    c[4:8] = np.float32([2.0 ** -60, -2.0 ** -60, 2.0 ** -149, -2.0 ** -149])
    a[8:12] = np.float32(2.0 ** -75)
    b[8:12] = np.float32([2.0 ** -74, 1.5 * 2.0 ** -75, -2.0 ** -75, 3 * 2.0 ** -76])  # subnormal / underflow
    c[8:12] = np.float32([0.0, 2.0 ** -149, 2.0 ** -149, -2.0 ** -149])
    got = OB.fma32(a, b, c)

    def rn32(q):  # exact RN-even of a rational to f32
        if q == 0:
            return np.float32(0.0)
        s, q = (-1 if q < 0 else 1), abs(q)
        e = max(-126, int(np.floor(np.log2(float(q)))) if float(q) > 0 else -126)
        while Fraction(2) ** e > q and e > -126:
            e -= 1
        while Fraction(2) ** (e + 1) <= q:
            e += 1
        ulp = Fraction(2) ** (e - 23)
        n, r = divmod(q, ulp)
        if r * 2 > ulp or (r * 2 == ulp and n % 2):
            n += 1
        return np.float32(s * float(n * ulp))

    for i in range(a.size):
        want = rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)
    big, inf, nan = np.float32(3e38), np.float32(np.inf), np.float32(np.nan)
    sp = OB.fma32(np.float32([big, inf, 0, nan, big, -0.0, 1]), np.float32([big, 1, inf, 1, 2, 5, 1]),
                  np.float32([0, -inf, 1, 1, -big, -0.0, -1]))
    assert sp[0] == inf and np.isnan(sp[1]) and np.isnan(sp[2]) and np.isnan(sp[3]) and sp[4] == big
    assert sp[5] == 0 and np.signbit(sp[5]) and sp[6] == 0 and not np.signbit(sp[6])


def test_vit_shapes_unaffected():
    """The ViT's float GEMMs keep their kernels and K blocks: K = 768 and 3072 (and ViT-tiny's 192)
    block alike under both drivers, every block end a multiple of 16, and none of their shapes is
    in the small regime."""
    for drv in R.DRIVERS:
        assert R.k_blocks(768, drv) == [384, 384]
        assert R.k_blocks(3072, drv) == [448] * 5 + [416, 416]
        assert R.k_blocks(1536, drv) == [448, 448, 320, 320]
        assert R.k_blocks(192, drv) == [192] and R.k_blocks(64, drv) == [64]
    for batch in (1, 4, 256):
        for M, N, K in ((197 * batch, 768, 768), (197 * batch, 3072, 768), (197 * batch, 768, 3072),
                        (196 * batch, 768, 768), (197, 197, 64), (197, 64, 197), (197 * batch, 192, 192),
                        (196 * batch, 192, 768)):
            assert R.gemm_regime(M, N, K, False) == "level3" and R.gemm_regime(M, N, K, True) == "level3"
            assert not KM.gemm_small_regime(M, N, K, False) and not KM.gemm_small_regime(M, N, K, True)


def test_device_predicates_follow_the_reference_map():
    """kernels.gemm_small_regime (and so nqk_gemm.hip's rule, which the GPU tests pin) is
    _sgemm_ref.gemm_regime on every row of the table and around the boundary."""
    shapes = [r[:4] for r in TABLE if r[0] >= 2] + [(M, N, K, tb) for M in (2, 30, 100, 125) for N in (2, 40, 41, 80, 100)
                                                  for K in (31, 32, 100, 101, 1000) for tb in (False, True)]
    for M, N, K, tb in shapes:
        assert KM.gemm_small_regime(M, N, K, tb) == (R.gemm_regime(M, N, K, tb) == "small"), (M, N, K, tb)
