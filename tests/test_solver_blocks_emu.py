"""CPU tier: the dense solver blocks (solver_blocks.h: ldl_solve / ldl_block / ldl_block0_dual, gj_inverse6 / gj_solve6), each called
on one wave of the emulator, in both forms of the sources: the default one (one lane predicate per pivot, the back-substitution sum
without a lane mask) and -DJACO_SOLVER_MASKS=1 (solver_blocks_masks.h: one compare per role, the masked sum: what the kernel did
before).  Every case runs in the three layouts (default, 12-hinge, 30-dof: the last two run the read-lane forms of ldl_block and
ldl_block0_dual with blocks that cross a 16-lane row); a routine whose block is empty in a layout (the 12-hinge one has no third
block) is skipped there.

Every case: what each of the 64 lanes holds afterwards -- x, the dual's damped x, the matrix rows -- is equal bit for bit between the
two forms; x is 0 outside the block; the rows of the lanes outside the block are the ones handed in.  On the well-conditioned cases
x is within 1e-5 (max |x - ref| / max |ref|) of numpy's fp64 solve of the block.  fp32 on a matrix of condition number <= 4 gives a
few 1e-7 there, so the bound is never close.

Inputs: a dense SPD matrix over all dofs (each block routine sees the other blocks' rows, and their coupling columns, non-zero in the
registers it shares with them); a block-diagonal one (ldl_solve<false>); one pivot of the block near zero (bits only: the answer is
ill-conditioned by construction); inf in lanes outside the block, in the block's columns and in the right-hand side."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu_solver")
FORMS = ("libjaco_emu_solver%s.so", "libjaco_emu_solver_masks%s.so")
LAYOUTS = ("", "_d12", "_d30")
F32P = ctypes.POINTER(ctypes.c_float)
_libs = {}
_layout = [""]


def per_layout(name, values):
    """Every value in every layout; the default layout's cases keep the ids they had."""
    return pytest.mark.parametrize("layout," + name, [pytest.param(l, v, id=(l[1:] + "-" if l else "") + str(v)) for l in LAYOUTS for v in values])


def libs():
    """The two forms' libraries of the layout the running test chose."""
    layout = _layout[0]
    if layout not in _libs:
        names = [f % layout for f in FORMS]
        subprocess.check_call(["make", "-s", "-C", EMU_DIR] + names)
        pair = []
        for k, name in enumerate(names):
            L = ctypes.CDLL(os.path.join(EMU_DIR, name))
            d = (ctypes.c_int * 5)()
            L.emu_solver_dims(d)
            assert d[4] == k, "%s holds the wrong form" % name
            L.dims = tuple(d[:4])
            pair.append(L)
        assert pair[0].dims == pair[1].dims
        _libs[layout] = pair
    return _libs[layout]


def block(layout, which):
    """Chooses the layout for this test; the routine's [lo, hi), or a skip where the layout gives it no dofs."""
    _layout[0] = layout
    lo, hi = ranges()[which]
    if lo == hi:
        pytest.skip("routine %d: the block [%d, %d) is empty in this layout" % (which, lo, hi))
    return lo, hi


def _p(a):
    return a.ctypes.data_as(F32P)


def ldl(L, which, H, b, hd):
    H, b, hd = (np.ascontiguousarray(a, np.float32) for a in (H, b, hd))
    x, xd, Ho = np.full(64, 7.0, np.float32), np.full(64, 7.0, np.float32), np.full(H.shape, 7.0, np.float32)
    assert L.emu_ldl(which, _p(H), _p(b), _p(hd), _p(x), _p(xd), _p(Ho)) == 0
    return x, xd, Ho


def gj(L, which, A, B):
    A, B = np.array(A, np.float32, order="C"), np.array(B, np.float32, order="C")
    det = np.full(64, 7.0, np.float32)
    assert L.emu_gj(which, _p(A), _p(B), _p(det)) == 0
    return A, B, det


def both_ldl(which, H, b, hd):
    """The routine in both forms: equal bit for bit in every lane.  Returns the default form's (x, xd, rows)."""
    new, old = (ldl(L, which, H, b, hd) for L in libs())
    for a, c, what in zip(new, old, ("x", "xd", "rows")):
        assert a.tobytes() == c.tobytes(), "routine %d: %s differs between the two forms" % (which, what)
    return new


def spd(rng, n):
    """Symmetric, eigenvalues in [2, 4 + ...]: condition number below 4."""
    G = rng.uniform(-1, 1, (n, n))
    A = G @ G.T
    return 2.0 * np.eye(n) + 2.0 * A / np.linalg.eigvalsh(A).max()


def ranges():
    nv, b0, b1, nsh = libs()[0].dims
    return {0: (0, b0), 1: (b0, b1), 2: (b1, nv), 3: (b0, nv), 4: (0, b0), 5: (0, nv), 6: (0, nv)}


def registers(A, rhs):
    """Lane l < JNV: row l and its right-hand side; the lanes above: identity rows (zero in the columns below JNV), rhs 0."""
    nv = libs()[0].dims[0]
    H, b = np.zeros((64, nv), np.float32), np.zeros(64, np.float32)
    H[:nv] = A
    b[:nv] = rhs
    return H, b


def rel(x, ref):
    return float(np.abs(x.astype(np.float64) - ref).max() / np.abs(ref).max())


def check_block(which, H, b, hd, x, xd, Ho, reference=True):
    lo, hi = ranges()[which]
    nv, b0, b1, nsh = libs()[0].dims
    out = np.r_[0:lo, hi:64]
    assert not x[out].any() and not xd[out].any(), "x outside the block"
    assert Ho[out].tobytes() == H[out].tobytes(), "rows of lanes outside the block changed"
    assert np.isfinite(x[lo:hi]).all() and np.isfinite(xd[lo:hi]).all()
    if not reference:
        return
    A64 = H[lo:hi, lo:hi].astype(np.float64)
    if which == 6:   # block diagonal by contract: the coupling entries are not read
        for a, c in ((0, b0), (b0, b1), (b1, nv)):
            if a < c:   # (a layout may leave a sub-block empty)
                assert rel(x[a:c], np.linalg.solve(A64[a:c, a:c], b[a:c].astype(np.float64))) < 1e-5
    else:
        assert rel(x[lo:hi], np.linalg.solve(A64, b[lo:hi].astype(np.float64))) < 1e-5
    if which == 4:
        assert rel(xd[lo:hi], np.linalg.solve(A64 + np.diag(hd[lo:hi].astype(np.float64)), b[lo:hi].astype(np.float64))) < 1e-5
    else:
        assert not xd.any()


def damping(rng):
    nv, b0, b1, nsh = libs()[0].dims
    hd = np.zeros(64, np.float32)
    hd[nsh:b0] = rng.uniform(0.05, 0.5, b0 - nsh)   # the finger joints' h * damping
    return hd


@per_layout("which", range(7))
def test_random_spd_with_the_other_blocks_rows_in_the_registers(layout, which):
    """A dense SPD matrix over all dofs: a block routine solves its diagonal block and leaves the rest alone."""
    block(layout, which)
    nv = libs()[0].dims[0]
    for seed in range(4):
        rng = np.random.default_rng([which, seed])
        A = spd(rng, nv)
        if which == 6:   # ldl_solve<false>: block diagonal by contract
            nv_, b0, b1, _ = libs()[0].dims
            M = np.zeros_like(A)
            for a, c in ((0, b0), (b0, b1), (b1, nv)):
                M[a:c, a:c] = A[a:c, a:c]
            A = M
        H, b = registers(A, rng.uniform(-1, 1, nv))
        hd = damping(rng)
        x, xd, Ho = both_ldl(which, H, b, hd)
        check_block(which, H, b, hd, x, xd, Ho)


@per_layout("which", range(7))
def test_near_singular_pivot_same_bits(layout, which):
    """The block's third pivot comes out 1e-7 of its neighbours: the two forms still agree in every bit, and nothing leaves the block."""
    lo, hi = block(layout, which)
    nv = libs()[0].dims[0]
    rng = np.random.default_rng([which, 99])
    A = spd(rng, nv)
    k = lo + 2
    A[k, :] = 0; A[:, k] = 0   # decouple row k, then give it an almost dependent copy of row lo
    A[k, lo:hi] = A[lo, lo:hi]; A[lo:hi, k] = A[lo:hi, lo]; A[k, k] = A[lo, lo] * (1 + 1e-7)
    H, b = registers(A, rng.uniform(-1, 1, nv))
    hd = damping(rng)
    x, xd, Ho = both_ldl(which, H, b, hd)
    out = np.r_[0:lo, hi:64]
    assert not x[out].any() and not xd[out].any() and Ho[out].tobytes() == H[out].tobytes()


@per_layout("which", range(7))
def test_inf_in_lanes_outside_the_block(layout, which):
    """inf where the routine must not look: in the block's columns of the rows outside it and in their right-hand sides (for the two
    ldl_solve forms, whose block is all dofs, that is the lanes above JNV).  The block's answer is the clean one."""
    lo, hi = block(layout, which)
    nv = libs()[0].dims[0]
    rng = np.random.default_rng([which, 7])
    A = spd(rng, nv)
    if which == 6:
        M = np.zeros_like(A)
        for a, c in ((0, libs()[0].dims[1]), (libs()[0].dims[1], libs()[0].dims[2]), (libs()[0].dims[2], nv)):
            M[a:c, a:c] = A[a:c, a:c]
        A = M
    H, b = registers(A, rng.uniform(-1, 1, nv))
    hd = damping(rng)
    clean = both_ldl(which, H, b, hd)
    Hi, bi = H.copy(), b.copy()
    out = np.r_[0:lo, hi:64]
    Hi[np.ix_(out, np.arange(lo, hi))] = np.inf
    Hi[out[::2], lo] = -np.inf
    bi[out] = np.inf
    x, xd, Ho = both_ldl(which, Hi, bi, hd)
    assert x[lo:hi].tobytes() == clean[0][lo:hi].tobytes() and xd[lo:hi].tobytes() == clean[1][lo:hi].tobytes()
    assert Ho[lo:hi].tobytes() == clean[2][lo:hi].tobytes()
    assert not x[out].any() and not xd[out].any()
    if which < 5:   # (the block routines leave the other rows alone; ldl_solve eliminates in every lane, identity rows included)
        assert Ho[out].tobytes() == Hi[out].tobytes()
    check_block(which, H, b, hd, *clean)


def both_gj(which, A, B):
    new, old = (gj(L, which, A, B) for L in libs())
    for a, c, what in zip(new, old, ("A", "B", "det")):
        assert a.tobytes() == c.tobytes(), "gj routine %d: %s differs between the two forms" % (which, what)
    return new


def gj_inputs(rng, junk):
    A, B = np.zeros((64, 6), np.float32), np.zeros((64, 6), np.float32)
    A[:6] = spd(rng, 6)
    B[:6] = np.eye(6)
    if junk == "random":
        A[6:], B[6:] = rng.uniform(-1, 1, (58, 6)), rng.uniform(-1, 1, (58, 6))
    elif junk == "inf":
        A[6:], B[6:] = np.inf, -np.inf
    return A, B


@per_layout("junk", ["zero", "random", "inf"])
def test_gj_inverse6_and_gj_solve6(layout, junk):
    _layout[0] = layout
    for seed in range(4):
        rng = np.random.default_rng([seed, 6])
        A, B = gj_inputs(rng, junk)
        A64 = A[:6].astype(np.float64)
        Ao, Bo, det = both_gj(0, A, B)
        assert rel(Bo[:6], np.linalg.inv(A64)) < 1e-5
        assert rel(Ao[:6], np.eye(6)) < 1e-5
        assert abs(det[0] / np.linalg.det(A64) - 1) < 1e-5 and (det == det[0]).all()
        rhs = B.copy()
        rhs[:6, 0] = rng.uniform(-1, 1, 6)
        Ao, Bo, det = both_gj(1, A, rhs)
        assert rel(Bo[:6, 0], np.linalg.solve(A64, rhs[:6, 0].astype(np.float64))) < 1e-5
        assert Bo[:, 1:].tobytes() == rhs[:, 1:].tobytes()
        assert abs(det[0] / np.linalg.det(A64) - 1) < 1e-5


def test_gj_near_singular_pivot_same_bits():
    rng = np.random.default_rng(5)
    A, B = gj_inputs(rng, "random")
    A[2, :6] = A[0, :6]; A[:6, 2] = A[:6, 0]; A[2, 2] = A[0, 0] * (1 + 1e-7)
    for layout in LAYOUTS:   # (no parameter: the test keeps its id)
        _layout[0] = layout
        both_gj(0, A, B)
        both_gj(1, A, B)
