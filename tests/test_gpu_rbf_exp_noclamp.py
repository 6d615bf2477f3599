"""The generating role's exp without its clamp (rbf_of_sqdist_lean<false>, csrc/common.h)
against the device library's.

Where the points of an operator keep every squared distance below 2150 (mlff_sym_gen_info), the
plain tiles of the tile mat-vec's generating role evaluate exp(-0.5 s) without the min(s, 2150)
that stands in for the library's underflow select.  On 0 <= s <= 2150 that form
must still give the library's bits: the inputs are those of tests/test_gpu_rbf_exp_lean.py inside
that domain, with its upper end and the two values below it, compared on the device as raw bits.
"""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_rbf_exp_lean import inputs

pytestmark = pytest.mark.gpu

S_MAX = 2150.0


def noclamp_inputs():
    s = inputs()
    s = s[s <= S_MAX]
    top = np.array([S_MAX]).view(np.int64)
    s = np.concatenate([s, (top - np.arange(3)).view(np.float64)])
    return np.ascontiguousarray(s)


def test_noclamp_exp_is_the_library_exp_bit_for_bit():
    import sgdml_amd
    from sgdml_amd import _native as nat

    s = noclamp_inputs()
    assert s.size > (1 << 21) and np.all(s >= 0.0) and np.all(s <= S_MAX)
    assert s[-1] < s[-2] < s[-3] == S_MAX
    lib_out = np.empty_like(s)
    lean_out = np.empty_like(s)
    solver = sgdml_amd.KernelSolver(64, device=0)
    try:
        solver._call("mlff_test_rbf_exp_noclamp", nat.dptr(s), ctypes.c_int64(s.size),
                     nat.dptr(lib_out), nat.dptr(lean_out))
        # outside the form's domain the hook refuses instead of answering
        o1, o2 = np.empty(1), np.empty(1)
        for bad in (np.nextafter(S_MAX, np.inf), np.inf, -1.0, np.nan):
            one = np.array([bad])
            with pytest.raises(ValueError):
                solver._call("mlff_test_rbf_exp_noclamp", nat.dptr(one), ctypes.c_int64(1),
                             nat.dptr(o1), nat.dptr(o2))
    finally:
        solver.close()
    a, b = lib_out.view(np.uint64), lean_out.view(np.uint64)
    bad = np.flatnonzero(a != b)
    print(f"{s.size} inputs, {bad.size} differ"
          + (f"; first s = {s[bad[0]]!r}: {lib_out[bad[0]]!r} / {lean_out[bad[0]]!r}" if bad.size else ""))
    assert np.array_equal(a, b)
    # s = 0 and denormal results are in the set, and results on the far side of the underflow
    assert np.any(s == 0.0) and np.all(lean_out[s == 0.0] == 1.0)
    assert np.any((lean_out > 0.0) & (lean_out < 2.3e-308))
    assert np.any(lean_out == 0.0) and not np.any(np.signbit(lean_out))
    assert abs(lean_out[0] - np.exp(-0.5 * s[0])) <= 4 * np.spacing(np.exp(-0.5 * s[0]))
