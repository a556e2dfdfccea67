"""The block-vector kernels of the eigensolver on their own (fh_block_gram_dev, fh_block_combine_dev) against numpy, at shapes the solver
never produces: one row, sizes around the 256-row workgroup and the 32-row chunk, more than one workgroup, one to 96 columns, a leading
dimension above n with NaN in the padding rows.

Bounds: an inner product of n terms summed in any order with fused multiply-adds is within n u sum |s_i t_i| / (1 - n u) of the exact one
(Higham, Accuracy and Stability, sec. 3.1), u = eps / 2, so n eps sum |s_i t_i| holds it against a reference in extended precision; a
row of Y = S C is an inner product of p terms.  Accumulating, the kernel starts its sums from Y: p roundings of partial sums that are at
most |Y| + |S||C|, so with |Y| <= |S||C| entrywise (which the test arranges) the same bound p eps |S||C| holds."""
import numpy as np
import pytest

import fenris_amd as fa

EPS = np.finfo(float).eps
NS = [1, 63, 255, 256, 257, 5000]
PQ = [(1, 1), (3, 5), (16, 16), (17, 31), (96, 96), (96, 1)]
FH_BAD_ARGUMENT = 2


@pytest.fixture(scope="module")
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


_blocks = {}


def _exact(a, b):
    """a @ b in extended precision"""
    return np.asarray(a, dtype=np.longdouble) @ np.asarray(b, dtype=np.longdouble)


def _block(n, cols, pad, seed):
    """(host n x cols, device tensor cols x (n + pad) whose rows are the columns, NaN in the padding); made once per shape"""
    import torch

    key = (n, cols, pad, seed)
    if key not in _blocks:
        rng = np.random.default_rng(1000 * seed + 7 * n + cols)
        h = rng.standard_normal((n, cols)) * np.exp(rng.uniform(-3, 3, (1, cols)))
        full = np.full((cols, n + pad), np.nan)
        full[:, :n] = h.T
        _blocks[key] = (h, torch.from_numpy(full).cuda())
    return _blocks[key]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("n", NS)
def test_gram_against_numpy(engine, n, pad):
    for p, q in PQ:
        s, s_t = _block(n, p, pad, 1)
        t, t_t = _block(n, q, pad, 2)
        g = engine.block_gram(n, p, s_t, n + pad, q, t_t, n + pad)
        ref = _exact(s.T, t)
        bound = n * EPS * (np.abs(s).T @ np.abs(t))
        assert np.all(np.isfinite(g)), (n, p, q)
        assert np.all(np.abs(g - ref) <= bound), (n, p, q, (np.abs(g - ref) / bound).max())
        g2 = engine.block_gram(n, p, s_t, n + pad, q, t_t, n + pad)
        assert np.array_equal(g, g2), (n, p, q)
        if pad:   # the same bits as without the padding rows
            assert np.array_equal(g, engine.block_gram(n, p, _block(n, p, 0, 1)[1], n, q, _block(n, q, 0, 2)[1], n))


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("n", NS)
def test_combine_against_numpy(engine, n, pad):
    import torch

    rng = np.random.default_rng(n + pad)
    for p, q in PQ:
        s, s_t = _block(n, p, pad, 1)
        c = rng.standard_normal((p, q))
        bound = p * EPS * (np.abs(s) @ np.abs(c))
        y0 = rng.uniform(-1, 1, (n, q)) * (np.abs(s) @ np.abs(c))
        for accumulate in (False, True):
            full = np.full((q, n + pad), -777.0)
            full[:, :n] = y0.T
            y_t = torch.from_numpy(full).cuda()
            engine.block_combine(n, p, s_t, n + pad, c, y_t, n + pad, accumulate)
            y = y_t.cpu().numpy()
            ref = _exact(s, c) + (y0 if accumulate else 0.0)
            assert np.all(np.abs(y[:, :n].T - ref) <= bound), (n, p, q, accumulate)
            assert np.all(y[:, n:] == -777.0), (n, p, q, accumulate)   # rows >= n untouched


@pytest.mark.gpu
def test_block_argument_errors(engine):
    import ctypes as C

    import torch

    from fenris_amd import _ffi

    lib, h = engine._lib, engine._h
    x = torch.ones(4 * 10, dtype=torch.float64, device="cuda")
    y = torch.ones(4 * 10, dtype=torch.float64, device="cuda")
    g = np.full((96, 96), 5.0)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.fh_block_gram_dev(h, 10, 0, px, 10, 2, py, 10, _ffi.fp(g)) == FH_BAD_ARGUMENT
    assert lib.fh_block_gram_dev(h, 10, 2, px, 10, 97, py, 10, _ffi.fp(g)) == FH_BAD_ARGUMENT
    assert lib.fh_block_gram_dev(h, 10, 2, px, 9, 2, py, 10, _ffi.fp(g)) == FH_BAD_ARGUMENT
    assert lib.fh_block_gram_dev(h, 10, 2, None, 10, 2, py, 10, _ffi.fp(g)) == FH_BAD_ARGUMENT
    assert lib.fh_block_gram_dev(h, 10, 2, px, 10, 2, py, 10, None) == FH_BAD_ARGUMENT
    assert lib.fh_block_gram_dev(h, 0, 2, px, 10, 3, py, 10, _ffi.fp(g)) == 0 and np.all(g.ravel()[:6] == 0.0)
    c = np.ones((2, 2))
    assert lib.fh_block_combine_dev(h, 10, 2, px, 10, 0, _ffi.fp(c), py, 10, 0) == FH_BAD_ARGUMENT
    assert lib.fh_block_combine_dev(h, 10, 97, px, 10, 2, _ffi.fp(c), py, 10, 0) == FH_BAD_ARGUMENT
    assert lib.fh_block_combine_dev(h, 10, 2, px, 10, 2, _ffi.fp(c), py, 9, 0) == FH_BAD_ARGUMENT
    assert lib.fh_block_combine_dev(h, 10, 2, px, 10, 2, None, py, 10, 0) == FH_BAD_ARGUMENT
    assert lib.fh_block_combine_dev(h, 10, 2, px, 10, 2, _ffi.fp(c), C.c_void_p(x.data_ptr() + 80), 10, 0) == FH_BAD_ARGUMENT   # Y inside S
    assert lib.fh_block_combine_dev(h, 0, 2, px, 10, 2, _ffi.fp(c), py, 10, 0) == 0
    assert torch.all(y == 1.0)
