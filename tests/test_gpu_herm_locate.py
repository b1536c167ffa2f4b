"""GPU tests (-m gpu) of the Hermite order of the point locator (csrc/locate.hip order 3 through helmholtz/locate.py) against
tests/_hermlocref.py (pinned by tests/test_herm_locate_ref.py): the weight rows, the gather kernel, cubics end to end, the transfer onto
another mesh, observers, and the error contract of wae_hermite_locator_set.

Meshes, query sets and the selection of located points are those of tests/test_gpu_locate.py; the Hermite numbering always comes from
the device (`herm_connectivity` with the mesh's boundary triangles)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _hermlocref as HL
import _hermref as H
import _locref as R
import _octoref as O
import test_gpu_locate as G
from wae_amd import _lib
from wae_amd.helmholtz import Locator
from wae_amd.helmholtz.assemble import herm_connectivity, herm_dofs

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
INVALID = _lib.WAE_ERR_INVALID
LD = np.longdouble
N_DIR = HL.N_DIR
# the weight bound: see test_weight_rows
C_MEASURED = 4.02
C_WEIGHTS = 8 * C_MEASURED
KINDS = ((0, "p"), (1, "n_grad_p"))


@functools.lru_cache(maxsize=None)
def setup(name):
    """(locator, points, tets, tris, faces, tets20, ndof) with the numbering of the device"""
    pts, tets, tris = O.mesh(name)
    faces, t20, _, ndof = herm_connectivity(pts, tets, tris)
    return Locator(pts, tets), pts, tets, tris, faces, t20, ndof


def row_tolerance(pts, tets, t, kind, w, u):
    """the bound of a sampled value: sum_a (C_WEIGHTS row_bound_a + 17 eps |w_a|) |u_a| -- the row's own bound, the 16 eps of the gather kernel's
    sum (test_sample_is_the_row_sum_in_order) and eps / 2 for a vector u that is the exact one rounded to float64"""
    return np.sum((C_WEIGHTS * HL.row_bound(pts, tets, t, kind, N_DIR) + 17 * EPS * np.abs(w)) * np.abs(u), axis=1)


@pytest.mark.parametrize("name", ["two", "sheared", "cube", "rijke"])
def test_weight_rows(name):
    """idx == tets20[t] exactly and |val_dev - val_ref| <= c eps kappa_inf(J) s per weight against the longdouble rows of _hermlocref (the
    dual basis on the physical element, not the table): s = 1 for the value and face weights, ||J||_inf for the weights of the gradient
    unknowns, for kind "n_grad_p" times ||J^-1||_inf ||n||.  c: the float64 transliteration of the device formula in _hermlocref.py reaches
    at most C_MEASURED times that unit against longdouble on these same inputs (measured_herm_ratio: 1.68, 3.08, 2.44, 4.01 on the four
    meshes, on the CPU, never against the device; tests/test_herm_locate_ref.py keeps the constant above the measurement); c = C_WEIGHTS =
    32.16 is 8 times that, which covers another equally stable operation order."""
    loc, pts, tets, tris, faces, t20, ndof = setup(name)
    assert np.array_equal(t20, H.connectivity(len(pts), tets, tris)[1]) and ndof == int(t20.max()) + 1
    X, t = G.located_points(name)
    for kind, kname in KINDS:
        n = N_DIR if kind else None
        idx, val = loc.weights(X, "herm", kname, n=n, tets20=t20)
        idx2, val2 = loc.weights(X, "herm", kname, n=n, tet=t)                 # the table is on the handle by now
        assert np.array_equal(idx, idx2) and np.array_equal(val.view(np.int64), val2.view(np.int64))
        assert idx.dtype == np.int32 and idx.shape == (len(X), 20) and np.array_equal(idx, t20[t])
        ref = HL.weight_rows_herm(pts, tets, X, t, kind, N_DIR)
        err = np.abs(val.astype(LD) - ref).astype(np.float64)
        unit = HL.row_bound(pts, tets, t, kind, N_DIR)
        host = np.abs(HL.device_rows_herm(pts, tets, X, t, kind, N_DIR).astype(LD) - ref).astype(np.float64)
        print(f"{name} herm {kname}: max err / (eps kappa s) = {np.max(err / unit):.2f}, host float64 {np.max(host / unit):.2f}, "
              f"rows equal to the transliteration bit for bit: {np.mean(np.all(val == HL.device_rows_herm(pts, tets, X, t, kind, N_DIR), axis=1)):.3f}")
        assert np.all(err <= C_WEIGHTS * unit)
    Xo = np.concatenate([X[:3], G.queries(name)["outside"][:2]])
    idx, val = loc.weights(Xo, "herm", outside="nan")
    assert idx.shape == (5, 20) and np.all(idx[3:] == 0) and np.all(val[3:] == 0) and np.array_equal(idx[:3], t20[t[:3]])
    with pytest.raises(ValueError, match="point 3"):
        loc.weights(Xo, "herm")


@pytest.mark.parametrize("ncols", [1, 3, 8])
@pytest.mark.parametrize("name", ["two", "sheared", "rijke"])
def test_sample_is_the_row_sum_in_order(name, ncols):
    """out[q, c] against sum_i val[q, i] V[idx[q, i], c] accumulated in float64 in the order of i, val the float64 transliteration rows of
    _hermlocref (the device's formula operation for operation), within 16 eps sum_i |val_i| |V_i| per entry"""
    loc, pts, tets, tris, faces, t20, ndof = setup(name)
    X, t = G.located_points(name, 300)
    Xo = np.concatenate([X, G.queries(name)["outside"][:5]])
    rng = np.random.default_rng(ncols)
    V = rng.standard_normal((ndof, ncols)) + 1j * rng.standard_normal((ndof, ncols))
    for kind, kname in KINDS:
        n = N_DIR if kind else None
        val = HL.device_rows_herm(pts, tets, X, t, kind, N_DIR)
        want = np.zeros((len(X), ncols), dtype=np.complex128)
        mag = np.zeros((len(X), ncols))
        for i in range(20):
            want = want + val[:, i, None] * V[t20[t, i]]
            mag += np.abs(val[:, i, None]) * np.abs(V[t20[t, i]])
        got = loc.sample(V, Xo, "herm", kname, n=n, tets20=t20, outside="nan")
        assert got.shape == (len(Xo), ncols) and got.dtype == np.complex128
        assert np.all(np.isnan(got[len(X):].real)) and np.all(np.isnan(got[len(X):].imag))
        print(f"{name} {ncols} {kname}: max |got - want| / (eps mag) = {np.max(np.abs(got[:len(X)] - want) / (EPS * mag)):.2f}")
        assert np.all(np.abs(got[:len(X)] - want) <= 16 * EPS * mag)
        with pytest.raises(ValueError):
            loc.sample(V, Xo, "herm", kname, n=n)
    v1 = loc.sample(V[:, 0], X, "herm")
    assert v1.shape == (len(X),) and np.array_equal(v1, loc.sample(V[:, :1], X, "herm")[:, 0])


def rounded_dofs(pts, faces, tris, f, grad):
    """the unknowns of a cubic in the order of herm_dofs, evaluated in longdouble and rounded once to float64"""
    return H.dofs(pts.astype(LD), faces, tris, f, grad).astype(np.float64)


@pytest.mark.parametrize("name", ["cube", "rijke"])
def test_cubics_are_reproduced_end_to_end(name):
    """u = herm_dofs(cubic) with the faces of the device; sample(u, X, "herm") is the cubic and its n-gradient n . grad p at every located
    point, no tetrahedra passed in: find, numbering and rows together.  Bound: row_tolerance."""
    loc, pts, tets, tris, faces, t20, ndof = setup(name)
    X, t = G.located_points(name)
    assert np.array_equal(loc.find(X), t)
    for k in range(3):
        f, grad = HL.mesh_cubic(pts, k)
        u = rounded_dofs(pts, faces, tris, f, grad)
        assert u.shape == (ndof,)
        assert np.max(np.abs(u - herm_dofs(pts, faces, tris, f, grad))) <= 64 * EPS * np.max(np.abs(u))     # the product's helper, same numbering
        for kind, kname in KINDS:
            n = N_DIR if kind else None
            got = loc.sample(u, X, "herm", kname, n=n, tets20=t20)
            want = f(X.astype(LD)) if kind == 0 else grad(X.astype(LD)) @ N_DIR.astype(LD)
            w = HL.device_rows_herm(pts, tets, X, t, kind, N_DIR)
            tol = row_tolerance(pts, tets, t, kind, w, u[t20[t]])
            err = np.abs(got.real.astype(LD) - want).astype(np.float64)
            print(f"{name} cubic {k} {kname}: max err / tol = {np.max(err / tol):.3f}, max err {np.max(err):.2e}")
            assert np.all(got.imag == 0) and np.all(err <= tol)


def test_herm_transfer_onto_a_mesh_that_is_not_nested():
    """a cubic's unknowns on kuhn_cube(2) arrive on kuhn_cube(3) as herm_dofs(cubic) of that mesh: values, gradients and face values, every
    fine point and centroid located at tol = 1e-10 (checked on the host with _locref.first_containing_tol as well).  Bound: row_tolerance in
    the coarse tetrahedron the device chose."""
    p1, t1, top1 = H.kuhn_cube(2)
    p2, t2, top2 = H.kuhn_cube(3)
    faces1, t20, _, ndof1 = herm_connectivity(p1, t1, top1)
    faces2, _, _, ndof2 = herm_connectivity(p2, t2, top2)
    cen = p2[np.concatenate([top2, faces2])].mean(axis=1)
    assert np.all(R.first_containing_tol(p1, t1, p2, 1e-10)[0] >= 0) and np.all(R.first_containing_tol(p1, t1, cen, 1e-10)[0] >= 0)
    loc = Locator(p1, t1)
    try:
        tp, tc = loc.find(p2, tol=1e-10), loc.find(cen, tol=1e-10)
        assert np.all(tp >= 0) and np.all(tc >= 0)
        f, grad = HL.mesh_cubic(p1, 1)
        u1 = rounded_dofs(p1, faces1, top1, f, grad)
        got = loc.herm_transfer(u1, p2, t2, top2, tets20=t20)
        assert got.shape == (ndof2,) and np.all(got.imag == 0)
        want = H.dofs(p2.astype(LD), faces2, top2, f, grad)
        tol = [row_tolerance(p1, t1, tp, 0, HL.device_rows_herm(p1, t1, p2, tp, 0), u1[t20[tp]])]
        for e in np.eye(3):
            w = HL.device_rows_herm(p1, t1, p2, tp, 1, e)
            tol.append(np.sum((C_WEIGHTS * HL.row_bound(p1, t1, tp, 1, e) + 17 * EPS * np.abs(w)) * np.abs(u1[t20[tp]]), axis=1))
        tol.append(row_tolerance(p1, t1, tc, 0, HL.device_rows_herm(p1, t1, cen, tc, 0), u1[t20[tc]]))
        tol = np.concatenate(tol)
        err = np.abs(got.real.astype(LD) - want).astype(np.float64)
        print(f"herm_transfer: max err / tol = {np.max(err / tol):.3f}, max err {np.max(err):.2e}")
        assert np.all(err <= tol)
        two = loc.herm_transfer(np.stack([u1, 2 * u1], axis=1), p2, t2, top2)
        assert two.shape == (ndof2, 2) and np.array_equal(two[:, 0], got) and np.array_equal(two[:, 1], 2 * got)
    finally:
        loc.close()


def test_observers_go_through_the_packing_of_forced_response():
    from wae_amd.nlevp.forcing import pack_sparse_vectors
    loc, pts, tets, tris, faces, t20, ndof = setup("rijke")
    mics = G.located_points("rijke", 12)[0][:8]
    obs = loc.observers(mics, "herm", tets20=t20) + loc.observers(mics[:2], "herm", "n_grad_p", N_DIR, None, None, 0.0, t20)
    assert len(obs) == 10 and all(i.shape == (20,) and v.shape == (20,) for i, v in obs)
    ptr, idx, val = pack_sparse_vectors(obs, ndof, "observer")
    assert np.array_equal(ptr, 20 * np.arange(11)) and np.array_equal(idx, np.concatenate([i for i, _ in obs]))
    assert np.array_equal(val, np.concatenate([v for _, v in obs]).astype(np.complex128))
    rng = np.random.default_rng(5)
    v = rng.standard_normal(ndof) + 1j * rng.standard_normal(ndof)
    host = np.array([np.sum(val[ptr[k]:ptr[k + 1]] * v[idx[ptr[k]:ptr[k + 1]]]) for k in range(10)])
    dev = np.concatenate([loc.sample(v, mics, "herm"), loc.sample(v, mics[:2], "herm", "n_grad_p", n=N_DIR)])
    mag = np.array([np.sum(np.abs(val[ptr[k]:ptr[k + 1]]) * np.abs(v[idx[ptr[k]:ptr[k + 1]]])) for k in range(10)])
    assert np.all(np.abs(host - dev) <= 16 * EPS * mag)
    I = loc.interpolation(mics, order="herm")
    assert I.shape == (8, ndof) and np.all(np.abs(I @ v - dev[:8]) <= 32 * EPS * mag[:8])


def test_error_contract_of_the_hermite_table():
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pts, tets, tris = O.mesh("one")
    pts, tets = np.ascontiguousarray(pts), np.ascontiguousarray(tets, dtype=np.int32)
    np_, nt = len(pts), len(tets)
    _, t20, _, ndof = H.connectivity(np_, tets, tris)
    t20 = np.ascontiguousarray(t20, dtype=np.int32)
    D, I = (lambda a: a.ctypes.data_as(dp)), (lambda a: a.ctypes.data_as(ip))

    def refused(code):
        msg = L.wae_last_error().decode()
        assert code == INVALID and msg, (code, msg)
        return msg

    h = C.c_void_p()
    assert L.wae_locator_create(0, np_, D(pts), nt, I(tets), 0, C.byref(h)) == 0 and h.value
    try:
        X = np.ascontiguousarray(pts[tets].mean(axis=1))
        nq = len(X)
        t = np.zeros(nq, dtype=np.int32)
        idx, val = np.zeros((nq, 20), dtype=np.int32), np.zeros((nq, 20))
        V = np.zeros((ndof, 2), dtype=np.complex128, order="F")
        out = np.zeros((nq, 2), dtype=np.complex128, order="F")

        def order3():
            return L.wae_locator_weights(h, 3, 0, nq, D(X), I(t), None, I(idx), D(val))

        assert refused(L.wae_hermite_locator_set(None, ndof, I(t20))) == "null handle"
        refused(order3())                                                      # order 3 before any table
        swapped, shifted, low, high = t20.copy(), t20.copy(), t20.copy(), t20.copy()
        swapped[0, [0, 1]] = swapped[0, [1, 0]]                                # a value entry that is not the tetrahedron's point
        shifted[0, 9] += 1                                                      # a gradient entry of the wrong point
        low[0, 17], high[0, 19] = 4 * np_ - 1, ndof
        for code in (L.wae_hermite_locator_set(h, ndof, None), L.wae_hermite_locator_set(h, 4 * np_ - 1, I(t20)),
                     L.wae_hermite_locator_set(h, -1, I(t20)), L.wae_hermite_locator_set(h, 2 ** 31, I(t20)),
                     L.wae_hermite_locator_set(h, ndof, I(swapped)), L.wae_hermite_locator_set(h, ndof, I(shifted)),
                     L.wae_hermite_locator_set(h, ndof, I(low)), L.wae_hermite_locator_set(h, ndof, I(high))):
            refused(code)
            refused(order3())                                                  # nothing was kept
        assert L.wae_hermite_locator_set(h, ndof, I(t20)) == 0
        assert order3() == 0 and np.array_equal(idx, t20[t]) and abs(val[0, :4].sum() + val[0, 16:].sum() - 1) <= 64 * EPS
        keep = val.copy()
        refused(L.wae_hermite_locator_set(h, ndof, I(high)))                   # a refused table leaves the good one in place
        assert order3() == 0 and np.array_equal(val, keep)
        refused(L.wae_locator_sample(h, 3, 0, nq, D(X), I(t), None, ndof + 1, 2, D(V), D(out)))        # d != ndof
        refused(L.wae_locator_sample(h, 3, 0, nq, D(X), I(t), None, np_, 2, D(V), D(out)))
        refused(L.wae_locator_weights(h, 4, 0, nq, D(X), I(t), None, I(idx), D(val)))
        refused(L.wae_locator_weights(h, 3, 1, nq, D(X), I(t), None, I(idx), D(val)))                  # kind 1 without n
        assert L.wae_locator_sample(h, 3, 0, nq, D(X), I(t), None, ndof, 2, D(V), D(out)) == 0 and np.all(out == 0)
        t[0] = -1
        assert order3() == 0 and np.all(idx == 0) and np.all(val == 0)
        assert L.wae_locator_sample(h, 3, 0, nq, D(X), I(t), None, ndof, 2, D(V), D(out)) == 0 and np.all(np.isnan(out.real))
        tet = np.full(nq, -7, dtype=np.int32)
        assert L.wae_locator_find(h, nq, D(X), 0.0, I(tet), None) == 0 and np.array_equal(tet, np.arange(nt))
    finally:
        L.wae_locator_free(h)
