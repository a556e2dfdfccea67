#!/usr/bin/env python3
"""CPU calibration of the AMG-PCG iteration bounds of tests/test_amg.py (BOUNDS): the NumPy restatement of the hierarchy (aggregation,
eigenvalue estimate, V-cycle, PCG; tests/test_amg.py:_np_count) on the oracle's assembled matrices, clamped at x = 0 the way
fh_apply_dirichlet_csr_dev clamps (rows and columns zero, the diagonal |A_00|), right-hand side 1 with the clamped rows 0.  No GPU.

    python scripts/calibrate_amg_bounds.py
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fenris_amd as fa  # noqa: E402
from oracle import oracle  # noqa: E402
import test_amg as T  # noqa: E402

CASES = [("hex8", 12, "elastic"), ("hex8", 24, "elastic"), ("hex8", 16, "laplace"), ("hex8", 32, "laplace"),
         ("tet4", 12, "elastic"), ("tet4", 24, "elastic"), ("tet4", 16, "laplace"), ("tet4", 32, "laplace")]


def clamped_matrix(m, op):
    w, pts = T.RULES[m.elem_kind]()
    kind = {fa.HEX8: oracle.HEX8, fa.TET4: oracle.TET4}[m.elem_kind]
    params = None if op == "laplace" else fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3)).as_pair()
    a = oracle.ElementAssembler(kind, oracle.LAPLACE if op == "laplace" else oracle.LINEAR_ELASTIC, m.vertices, m.connectivity, w, pts,
                                params=params)
    st, _, ro, ci, v = oracle.assemble(a)
    assert st == 0
    A = sp.csr_matrix((v, ci.astype(np.int64), ro.astype(np.int64)))
    s = 1 if op == "laplace" else 3
    clamp = np.where(np.isclose(m.vertices[:, 0], 0.0))[0]
    dofs = (s * clamp[:, None] + np.arange(s)).ravel()
    keep = np.ones(A.shape[0])
    keep[dofs] = 0.0
    scale = abs(A[0, 0])
    A = (sp.diags(keep) @ A @ sp.diags(keep) + sp.diags(scale * (1.0 - keep))).tocsr()
    return A, s, clamp


if __name__ == "__main__":
    for name, k, op in CASES:
        m = T._mesh(name, k)
        A, s, clamp = clamped_matrix(m, op)
        print(f"({name!r}, {k}, {op!r}): {T._np_count(A, m, s, 'constant' if op == 'laplace' else 'rigid_body', clamp)}", flush=True)
