"""The counts of the timed segments that bench.py and the iterative solver report (gemv_count,
iter_count, precon_count, comm_count of KernelSolver.timing_read), read from the iteration's code
(csrc/pcg.hip): J = 8 iterations at tol = 0, maxiter = 8 -- one chunk, no launch gated -- on the
host SPD system N = 65 of tests/pcg_shapes.py with and without its k = 9 panel.

One rank brackets the operator once per sampled iteration and the low-rank apply once; it has no
collective.  Several ranks bracket three collectives per iteration: the gather of z, then either
the p.q and the rr all-reduce (no preconditioner, dense rows) or the tiles' reduce-scatter and
the merged rr | T r all-reduce (two-pass apply; the T r all-reduce of iteration 1, before the
first merged one exists, is not bracketed).
"""
import math

import pytest

from tests import pcg_shapes as pc
from tests.test_gpu_pcg_shapes import Form, _cut, _on_ranks, sg  # noqa: F401

pytestmark = pytest.mark.gpu

N, K, J = 65, 9, 8
NAMES = ("gemv", "iter", "precon", "comm")
# form, timing(on), expected counts (None: not asserted)
CASES = [
    (Form("dense"), 1, dict(gemv=8, iter=8, precon=0, comm=0)),
    (Form("sym", "0"), 1, dict(gemv=8, iter=8, precon=8, comm=0)),
    (Form("sym", "1"), 1, dict(gemv=8, iter=8, precon=8, comm=0)),
    (Form("dense"), 2, dict(gemv=4, iter=8, precon=0, comm=0)),
    (Form("dense", world=3), 1, dict(comm=24)),
    (Form("sym", "0", world=3), 1, dict(precon=8, comm=24)),
]


@pytest.mark.parametrize("form,every,want", CASES, ids=[f"{f.id}-timing{e}" for f, e, _ in CASES])
def test_timing_counts(sg, monkeypatch, form, every, want):  # noqa: F811
    s = pc.system(("spd", N), K if form.lr is not None else 0, pc.HOST_LAM)
    form.setenv(monkeypatch)

    def fn(c, r0, r1):
        c.timing(every)
        c.timing_reset()
        res = c.pcg(_cut(s.b, r0, r1), tol=0.0, maxiter=J)
        got = c.timing_read()
        c.timing_reset()
        return {"iters": res.iters, "got": got, "reset": c.timing_read()}

    for rank, out in enumerate(_on_ranks(sg, s, form, fn)):
        got = out["got"]
        print(f"timing-counts {form.id} timing({every}) rank {rank}: {got}")
        assert out["iters"] == J
        for name, count in want.items():
            assert got[f"{name}_count"] == count, (rank, name)
        for name in NAMES:
            ms, count = got[f"{name}_ms"], got[f"{name}_count"]
            assert math.isfinite(ms) and (ms > 0.0 if count > 0 else ms == 0.0), (rank, name)
        assert all(v == 0 for v in out["reset"].values()), out["reset"]
