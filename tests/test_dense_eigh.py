"""fh_dense_generalized_eigh, the host side of the eigensolver's Rayleigh-Ritz step (Cholesky of B, cyclic Jacobi on L^-1 A L^-T): no GPU.

The yardstick is numpy on the same input by the same reduction (Cholesky, eigh of L^-1 A L^-T, back substitution): both routes are
backward stable with different constants, so the residual of each pair and the departure of C^T B C from the identity may be at most 8
times what numpy's own pairs leave."""
import os
import re

import numpy as np
import pytest

from fenris_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fh_block_gram_dev", "fh_block_combine_dev", "fh_dense_generalized_eigh", "fh_eigs_lowest", "fh_eigs_lowest_dev")
FH_BAD_ARGUMENT, FH_EIG_MAX_ITERATIONS, FH_EIG_BREAKDOWN = 2, 13, 14


def _problem(p, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((p, p))
    a = 0.5 * (a + a.T)
    q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    d = np.logspace(0, -6, p) if p > 1 else np.ones(1)     # cond(B) = 1e6
    b = (q * d) @ q.T
    return a, 0.5 * (b + b.T)


def _numpy_pairs(a, b):
    low = np.linalg.cholesky(b)
    h = np.linalg.solve(low, np.linalg.solve(low, a).T).T
    w, v = np.linalg.eigh(0.5 * (h + h.T))
    return w, np.linalg.solve(low.T, v)


def _residuals(a, b, w, c):
    return np.linalg.norm(a @ c - (b @ c) * w, axis=0)


@pytest.mark.parametrize("p", [1, 2, 7, 48, 96])
def test_pairs_are_as_good_as_numpys(p):
    a, b = _problem(p, 100 + p)
    rc, w, c = _ffi.dense_generalized_eigh(a, b)
    assert rc == 0
    assert np.all(np.diff(w) >= 0.0)
    w_ref, c_ref = _numpy_pairs(a, b)
    eps = np.finfo(float).eps
    # numpy's own residuals, never below one rounding of the terms (a pair can come out exact by chance, p = 1 above all)
    floor = eps * (np.abs(a) @ np.abs(c_ref) + (np.abs(b) @ np.abs(c_ref)) * np.abs(w_ref)).max(axis=0)
    r_ref = np.maximum(_residuals(a, b, w_ref, c_ref), floor)
    r = _residuals(a, b, w, c)
    o_ref = max(np.abs(c_ref.T @ b @ c_ref - np.eye(p)).max(), eps)
    o = np.abs(c.T @ b @ c - np.eye(p)).max()
    print(f"p={p}: residual ratio {np.max(r / r_ref):.3f}, orthonormality ratio {o / o_ref:.3f}")
    assert np.all(r <= 8.0 * r_ref), (r / r_ref).max()
    assert o <= 8.0 * o_ref, (o, o_ref)


def test_indefinite_b_breaks_down():
    a, b = _problem(7, 3)
    b[3, 3] = -1.0
    rc, _, _ = _ffi.dense_generalized_eigh(a, b)
    assert rc == FH_EIG_BREAKDOWN
    rc, _, _ = _ffi.dense_generalized_eigh(a, np.zeros((7, 7)))
    assert rc == FH_EIG_BREAKDOWN


def test_bad_arguments():
    lib = _ffi.lib()
    a = np.eye(2)
    w, c = np.zeros(2), np.zeros((2, 2))
    assert lib.fh_dense_generalized_eigh(0, _ffi.fp(a), _ffi.fp(a), _ffi.fp(w), _ffi.fp(c)) == FH_BAD_ARGUMENT
    assert lib.fh_dense_generalized_eigh(97, _ffi.fp(a), _ffi.fp(a), _ffi.fp(w), _ffi.fp(c)) == FH_BAD_ARGUMENT
    assert lib.fh_dense_generalized_eigh(2, None, _ffi.fp(a), _ffi.fp(w), _ffi.fp(c)) == FH_BAD_ARGUMENT


def test_eigensolver_entry_points_are_declared():
    """the new entry points are in the header, exported, in the ctypes table and in the Rust bindings; the status codes follow the old ones"""
    header = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    lib = _ffi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.exported_symbols()
        assert getattr(lib, name) is not None
        assert "pub fn %s(" % name in rs, name
    assert re.search(r"FH_EIG_MAX_ITERATIONS\s*=\s*13", header) and re.search(r"FH_EIG_BREAKDOWN\s*=\s*14", header)
    assert re.search(r"FH_EIG_MAX_BLOCK\s*=\s*32", header)
    assert (_ffi.FH_EIG_MAX_ITERATIONS, _ffi.FH_EIG_BREAKDOWN, _ffi.EIG_MAX_BLOCK) == (13, 14, 32)
