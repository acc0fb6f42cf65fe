"""np.matmul of float32 matrices restated exactly, independent of the host it runs on: the order
of NumPy 2.2.6 on scipy-openblas 0.3.29 with its SkylakeX kernels, which nqk_sgemm reproduces.
Pinned to np.matmul by tests/test_sgemm_ref_host.py on a host that runs those kernels; the GPU
tests compare the device with sgemm_ref, never with the GPU host's own BLAS.

The map, for a row-major A[M, K] @ B[K, N] with M, N >= 2 (BLAS sees m = N, n = M):
  * regime: at most 100^3 multiply-adds take the small-matrix kernels (with B a transposed view
    only when M N <= 1200 and K >= 32); everything else a level-3 driver;
  * driver: interface/gemm.c allows min(threads, M N K / 262144) threads; one thread is the
    single-thread driver; otherwise level3_thread.c splits m over nthreads_m (the thread count
    halved until m >= 16 nthreads_m; 1 below m = 32) and n over ceil(n / (16 nthreads_m)) (1 below
    n = 16 nthreads_m), and one part is the single-thread driver again;
  * K blocks: GEMM_Q = 448; a remainder of 2 Q or more takes Q; one between Q and 2 Q is split: the
    single-thread driver takes half rounded up to a multiple of 16, the threaded driver the ceiling
    half; every block a k-ordered fma chain from +0 per output, block sums added to +0 in order."""
import numpy as np

from oracle.openblas_order import fma32, fma_chain, sgemm_small  # noqa: F401  (fma32 re-exported)

GEMM_Q = 448
DRIVERS = ("threaded", "single")
REGIMES = ("small", "level3")


def k_blocks(K: int, driver: str) -> list:
    if driver not in DRIVERS:
        raise ValueError(driver)
    out, ls = [], 0
    while ls < K:
        m = K - ls
        if m >= 2 * GEMM_Q:
            m = GEMM_Q
        elif m > GEMM_Q:
            m = (m + 1) // 2 if driver == "threaded" else ((m // 2 + 15) // 16) * 16
        out.append(m)
        ls += m
    return out


def gemm_driver(M: int, N: int, K: int, threads: int) -> str:
    nth = min(int(threads), max(1, int(float(M) * float(N) * float(K) / 262144.0)))
    if nth <= 1:
        return "single"
    m, n, ratio = N, M, 16
    nm = nn = 1
    if m >= 2 * ratio:
        nm = nth
        while m < nm * ratio:
            nm //= 2
    if n >= ratio * nm:
        nn = (n + ratio * nm - 1) // (ratio * nm)
        if nm * nn > nth:
            nn = nth // nm
    return "threaded" if nm * nn > 1 else "single"


def gemm_regime(M: int, N: int, K: int, transb: bool = False, threads: int = 1) -> str:
    """(The thread count does not enter: the small-matrix check comes before threading.)"""
    if float(M) * float(N) * float(K) > 1e6:
        return "level3"
    return "small" if (not transb or (M * N <= 1200 and K >= 32)) else "level3"


def blocked_chain(a: np.ndarray, b: np.ndarray, blocks) -> np.ndarray:
    """A level-3 driver's result: per K block a k-ordered fma chain from +0, the block sums added
    to C = +0 in order."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert sum(blocks) == a.shape[1]
    tot = np.zeros((a.shape[0], b.shape[1]), np.float32)
    ls = 0
    with np.errstate(all="ignore"):
        for m in blocks:
            tot = tot + fma_chain(a, b, ls, ls + m)
            ls += m
    return tot


def sgemm_ref(a: np.ndarray, b: np.ndarray, transb: bool = False, threads: int = 16) -> np.ndarray:
    """np.matmul(a, b) for float32 a[M, K], b[K, N] (M, N >= 2, K >= 1), bit for bit; `transb` says
    that NumPy holds b as the transposed view of a row-major [N, K] matrix; `threads` is OpenBLAS's
    thread count."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    (M, K), N = a.shape, b.shape[1]
    if M < 2 or N < 2 or K < 1 or b.shape[0] != K:
        raise ValueError("sgemm_ref: M, N >= 2 and K >= 1 expected (level-2 products: oracle/openblas_order.py)")
    if gemm_regime(M, N, K, transb, threads) == "small":
        return sgemm_small(a, b, transb)
    return blocked_chain(a, b, k_blocks(K, gemm_driver(M, N, K, threads)))


def blas_blocks(K: int, driver: str = "threaded") -> list:
    return k_blocks(K, driver)


def _fma_chain_blocks(a, w, K, driver: str = "threaded") -> np.ndarray:
    """Per output element: a k-ordered f32 fma chain from 0 in every BLAS block, block results
    added in order (correctly rounded fma32)."""
    return blocked_chain(np.asarray(a, np.float32), np.asarray(w, np.float32), k_blocks(K, driver))


def same_bits(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Elementwise: equal as int32 views, any NaN equal to any NaN."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return (x.view(np.int32) == y.view(np.int32)) | (np.isnan(x) & np.isnan(y))


def edge_operands(M: int, N: int, K: int, seed: int, blocks=None):
    """Operands whose last row and column (a ragged tile's) and whose k on both sides of every
    block boundary carry the edge values: subnormal products and sums, a chain that overflows to
    +inf and then meets -inf (NaN), 0 * inf, a NaN operand, rows of -0.0, magnitudes near 2^127."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    ends = [0]
    for m in (blocks or [K]):
        ends.append(ends[-1] + m)
    ks = sorted({k for e in ends for k in (e - 1, e) if 0 <= k < K})
    big, tiny = np.float32(2.0 ** 126.5), np.float32(2.0 ** -75)
    r, c = M - 1, N - 1
    if M >= 6 and N >= 6:
        # row r: subnormal products (2^-75 * 2^-70 ~ 2^-145) in the last row; sums stay subnormal
        a[r, :] = tiny * rng.uniform(1, 2, K).astype(np.float32)
        b[:, c] = np.float32(2.0 ** -70) * rng.uniform(-2, 2, K).astype(np.float32)
        # row r - 1: -0.0 throughout
        a[r - 1, :] = np.float32(-0.0)
        # row r - 2: near 2^127 on both sides of the boundaries, against column c - 1 -> overflow to +inf
        a[r - 2, :] = np.float32(1.0)
        b[:, c - 1] = np.float32(0.5)
        for k in ks:
            a[r - 2, k] = big
            b[k, c - 1] = big
        # column c - 2: +inf overflow, then -inf from the operand: inf - inf = NaN
        b[:, c - 2] = b[:, c - 1]
        if len(ks) >= 2:
            b[ks[-1], c - 2] = -np.inf
        # row r - 3: a zero against an inf in column c - 3: 0 * inf
        a[r - 3, ks[0]] = np.float32(0.0)
        b[ks[0], c - 3] = np.inf
        # row r - 4: a NaN operand at a block boundary
        a[r - 4, ks[-1]] = np.nan
    return a, b
