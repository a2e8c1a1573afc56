"""Host reference of the dropout mask (gist_amd/csrc/dropout.h), for tests that compare a kernel's mask bit for bit:
one splitmix64 of (index >> 1) + seed * golden ratio per element pair, an even index takes the low 32-bit word, an odd
index the high word, keep = (word >> 8) * 2^-24 >= p, kept elements are multiplied by the fp32 1 / (1 - p).

Two restatements stay on their own on purpose: tests/test_kernels_gpu._dropout_mask_ref and
tests/test_rowops_kernels_gpu.mask_ref are each other's cross-check (test_rowops_dispatch_coverage.py)."""
import numpy as np


def keep(idx, p, seed):
    """The keep decision (bool array) of mask indices idx (uint64 numpy array of any shape)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (idx >> np.uint64(1)) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    w = np.where(idx & np.uint64(1), z >> np.uint64(32), z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) >= np.float32(p)


def keep_mask(n, d, p, seed, offset, ld=None):
    """bool [n, d]: the keep decision of element (r, c) = index offset + r * ld + c (ld = d: a dense tensor)."""
    ld = d if ld is None else ld
    idx = (np.uint64(offset) + np.arange(n, dtype=np.uint64)[:, None] * np.uint64(ld)
           + np.arange(d, dtype=np.uint64)[None, :])
    return keep(idx, p, seed)


def scale(p):
    """The factor of a kept element, in float32 like the kernels'."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def factors(n, d, p, seed, offset, ld=None):
    """float32 [n, d]: what the kernels multiply element (r, c) by -- scale(p) or 0."""
    return np.where(keep_mask(n, d, p, seed, offset, ld), scale(p), np.float32(0.0)).astype(np.float32)
