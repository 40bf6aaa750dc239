"""Inputs and case lists of the value-domain tests: the same rows and queries for the GPU file
(tests/test_gpu_value_domain.py: the HIP paths against the oracle) and for the host file
(tests/test_value_domain_host.py: the premises those cases rest on, checked on the oracle alone).

Base data: unit-norm synthetic rows and queries (``O.synth_rows``).  Groups:
  A  rows times 2^a, queries times 2^b (f32 / bf16 rows);
  B  L2 with mismatched scales (every dtype);
  C  f16 rows small and large (across the f16 subnormal boundary 2^-14);
  D  row i times 2^((7 i) % 41 - 20) (f32 / bf16) or 2^((7 i) % 25 - 12) (f16), unit queries;
  E  every 97th row and every 5th query with one element times 1024 (the int8 row / query scale).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O

# path -> the smallest shape that reaches its kernel (shapes of the existing GPU tests)
PATHS = {
    # name: (family, screen, (nq, k, N, d), expected kind)
    "gemv": ("flat", "native", (3, 5, 5000, 96), "gemv"),
    "mfma16_tiled": ("flat", "native", (40, 10, 9000, 128), "mfma"),
    # d = 256: 8 K-steps of 32 elements per tile, a multiple of 4 and at least 8 (d16_direct_ok)
    "mfma16_direct": ("flat", "native", (20, 50, 3000, 256), "mfma"),
    "mfma_f32": ("flat", "native", (64, 10, 9000, 128), "mfma"),
    "i8_tiled": ("flat", "int8", (40, 10, 9000, 128), "mfma_i8"),
    "i8_direct": ("flat", "int8", (40, 10, 9000, 512), "mfma_i8"),
    "i8_gemv": ("flat", "int8", (3, 37, 5000, 96), "gemv_i8"),
    "small_scan": ("plain", "native", (2, 33, 4099, 96), "full_scan"),
    "sel_scan": ("sel", "scan", (2, 10, 3000, 100), "scan"),
    "sel_overfetch": ("sel", "overfetch", (9, 10, 9000, 128), "overfetch"),
    "ivf_gemv": ("ivf", "gemv", (5, 10, 20000, 64), "gemv"),
    "ivf_mfma": ("ivf", "mfma", (40, 10, 20000, 256), "mfma"),
}
IVF_LISTS = {"ivf_gemv": (64, 8), "ivf_mfma": (2, 2)}  # path -> (nlist, nprobe)
IVF_CENTROID_SEED = 5

PAIRS_A = [(-40, -40), (-40, 40), (40, -40), (40, 40), (-20, 3)]
PAIRS_A_MIN = [(-40, -40), (40, 40)]
PAIRS_B = [(12, 0), (0, 12)]
PAIRS_C = [(-20, 0), (-12, 0), (-12, 12), (-6, 0), (14, 0)]
METRICS = ["ip", "l2"]


def _cases_a():
    out = []
    full = {"gemv": ("f32", "bf16"), "mfma16_tiled": ("bf16",), "mfma16_direct": ("bf16",), "mfma_f32": ("f32",),
            "i8_tiled": ("bf16",), "i8_direct": ("bf16",), "i8_gemv": ("bf16",)}
    for path, dts in full.items():
        out += [(path, dt, m, a, b) for dt in dts for m in METRICS for a, b in PAIRS_A]
    few = {"small_scan": ("f32", "bf16"), "sel_scan": ("f32", "bf16"), "sel_overfetch": ("f32", "bf16"),
           "ivf_gemv": ("f32", "bf16"), "ivf_mfma": ("bf16",), "i8_tiled": ("f32",)}
    for path, dts in few.items():
        out += [(path, dt, m, a, b) for dt in dts for m in METRICS for a, b in PAIRS_A_MIN]
    return out


def _cases_b():
    dts = {"gemv": ("f32", "bf16", "f16"), "i8_gemv": ("f32", "bf16", "f16"), "mfma16_tiled": ("bf16", "f16"),
           "mfma16_direct": ("bf16", "f16"), "mfma_f32": ("f32",), "i8_tiled": ("f32", "bf16", "f16"),
           "i8_direct": ("f32", "bf16", "f16")}
    return [(path, dt, "l2", a, b) for path, d in dts.items() for dt in d for a, b in PAIRS_B]


def _cases_c():
    out = []
    for path in ("gemv", "mfma16_tiled", "mfma16_direct", "i8_tiled", "i8_direct", "i8_gemv"):
        out += [(path, "f16", m, a, b) for m in METRICS for a, b in PAIRS_C]
    for path in ("small_scan", "sel_scan", "sel_overfetch", "ivf_gemv", "ivf_mfma"):
        out += [(path, "f16", m, -12, 0) for m in METRICS]
    return out


def _cases_d():
    dts = {"gemv": ("f32", "bf16", "f16"), "mfma16_tiled": ("bf16", "f16"), "mfma16_direct": ("bf16", "f16"),
           "mfma_f32": ("f32",), "i8_tiled": ("bf16", "f16"), "i8_direct": ("bf16", "f16"), "i8_gemv": ("bf16", "f16"),
           "small_scan": ("f32", "f16"), "sel_scan": ("bf16", "f16"), "sel_overfetch": ("bf16", "f16"),
           "ivf_gemv": ("f32", "f16"), "ivf_mfma": ("bf16", "f16")}
    return [(path, dt, m) for path, d in dts.items() for dt in d for m in METRICS]


CASES_A, CASES_B, CASES_C, CASES_D = _cases_a(), _cases_b(), _cases_c(), _cases_d()
CASES_E = [(path, "bf16", m) for path in ("i8_tiled", "i8_direct", "i8_gemv") for m in METRICS]
# F: one shard holding the whole global top-k of a two-phase search over `world` shards
F_SHAPE, F_WORLD = (40, 25, 20011, 64), 8
CASES_F = [(m, s) for m in METRICS for s in (0, 40)]


def shape_of(path):
    return PATHS[path][2]


@functools.lru_cache(maxsize=None)
def _base(N, d, nq):
    x = O.synth_rows(O.SEED_CORPUS, 0, N, d, True, "f32")
    q = O.synth_rows(O.SEED_QUERIES, 0, nq, d, True, "f32")
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def base(shape):
    """The unit-norm rows and queries of a (nq, k, N, d) shape (cached, read-only)."""
    nq, _, N, d = shape
    return _base(N, d, nq)


def pow2(e) -> np.float32:
    return np.ldexp(np.float32(1.0), int(e))


def scaled(shape, a, b):
    """Groups A, B, C: rows times 2^a, queries times 2^b (exact in fp32)."""
    x, q = base(shape)
    return x * pow2(a), q * pow2(b)


def spread(shape, dtype):
    """Group D: one corpus whose row norms span 2^-20 .. 2^20 (f16: 2^-12 .. 2^12); unit queries."""
    x, q = base(shape)
    i = np.arange(x.shape[0])
    e = (7 * i) % 25 - 12 if dtype == "f16" else (7 * i) % 41 - 20
    return x * np.ldexp(np.float32(1.0), e.astype(np.int32))[:, None].astype(np.float32), q.copy()


def outliers(shape):
    """Group E: every 97th row i has its element (13 i) % d times 1024, and so has every 5th query."""
    x, q = base(shape)
    x, q = x.copy(), q.copy()
    d = x.shape[1]
    for i in range(0, x.shape[0], 97):
        x[i, (13 * i) % d] *= np.float32(1024.0)
    for i in range(0, q.shape[0], 5):
        q[i, (13 * i) % d] *= np.float32(1024.0)
    return x, q


def sel_mask(path):
    """The allowed rows of the selector paths: 500 of N for the scan, half of them for the overfetch."""
    N = shape_of(path)[2]
    m = 500 if path == "sel_scan" else N // 2
    mask = np.zeros(N, dtype=bool)
    mask[np.random.default_rng(97).permutation(N)[:m]] = True
    return mask


def covariant(metric, a, b) -> bool:
    """Whether the scaled problem is the unit-scale problem times a power of two (same ranking, scores
    times 2^(a+b)): inner product always, L2 only when rows and queries share the scale."""
    return metric == "ip" or a == b


def factor(metric, a, b) -> float:
    return 2.0 ** (a + b) if metric == "ip" else 2.0 ** (2 * a)
