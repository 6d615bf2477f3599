"""The generating role's exp (rbf_of_sqdist_lean, csrc/common.h) against the device library's.

The tile mat-vec's generating role evaluates exp(-0.5 s) by the library's own arithmetic
sequence without its two range selects.  Every generated entry must be the
stored bit pattern, so the two are compared on the device, as raw bits, over the whole domain
the role can see: s >= 0 or s = +inf.  (The host's exp is a different implementation and
proves nothing here.)
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))


def neighbours(x, ulps=(-2, -1, 0, 1, 2)):
    """x and its +-1, +-2 ulp neighbours (x > 0)."""
    x = np.asarray(x, dtype=np.float64)
    bits = x.view(np.int64)
    return np.concatenate([(bits + u).view(np.float64) for u in ulps])


def inputs():
    rng = np.random.default_rng(2024)
    n = 1 << 21
    k = np.arange(1552, dtype=np.float64)
    parts = [
        # log-uniform over [1e-320, 1e4]: denormal and tiny s up to far past the underflow
        10.0 ** rng.uniform(-320.0, 4.0, n),
        # uniform over [0, 2200]: the whole range of results, denormal results included
        rng.uniform(0.0, 2200.0, n),
        # x log2e = -0.5 s log2e is a tie of the rounding to n at s = (2k + 1) ln 2 and an
        # integer at s = 2k ln 2
        neighbours((2.0 * k + 1.0) * LN2),
        neighbours(2.0 * k[1:] * LN2),
        np.array([0.0, 5e-324, 1e300, np.inf]),
        neighbours([1490.0]),  # the result goes denormal
        neighbours([2150.0]),  # x = -1075: the clamp, where the library's select sets in
    ]
    s = np.ascontiguousarray(np.concatenate(parts))
    assert np.all(s >= 0.0) and not np.any(np.isnan(s))
    return s


def test_lean_exp_is_the_library_exp_bit_for_bit():
    import sgdml_amd
    from sgdml_amd import _native as nat

    s = inputs()
    assert abs(s.size - (1 << 22)) < (1 << 15)
    lib_out = np.empty_like(s)
    lean_out = np.empty_like(s)
    solver = sgdml_amd.KernelSolver(64, device=0)
    try:
        solver._call("mlff_test_rbf_exp", nat.dptr(s), ctypes.c_int64(s.size), nat.dptr(lib_out),
                     nat.dptr(lean_out))
    finally:
        solver.close()
    a, b = lib_out.view(np.uint64), lean_out.view(np.uint64)
    bad = np.flatnonzero(a != b)
    print(f"{s.size} inputs, {bad.size} differ"
          + (f"; first s = {s[bad[0]]!r}: {lib_out[bad[0]]!r} / {lean_out[bad[0]]!r}" if bad.size else ""))
    assert np.array_equal(a, b)
    # the probe ran and means what it says: the end points of the domain and one interior value
    assert lib_out[s == 0.0][0] == 1.0
    assert lib_out[np.isinf(s)][0] == 0.0 and not np.signbit(lib_out[np.isinf(s)][0])
    assert abs(lib_out[0] - np.exp(-0.5 * s[0])) <= 4 * np.spacing(np.exp(-0.5 * s[0]))
    # results on both sides of the underflow are in the set
    assert np.any((lib_out > 0.0) & (lib_out < 2.3e-308)) and np.any((lib_out == 0.0) & (s < 2200.0))
