"""Forced response: the reference's ``L(ω) \\ Array(rhs(ω))`` (forcing tutorial; ``rhs`` from ``discretize(...; source=true)``) over a list of
excitation frequencies, as one device call (wae_forced_response, include/waehip.h).  The right-hand sides are built in HBM from the sparse
source vectors, the frequencies are solved in lock-step batches, and only what was asked for comes back: the values of sparse observation
functionals (``helmholtz.probe``) and the solutions of the frequencies listed in ``keep``."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


class ForcedResponse:
    """H (nobs x nfreq): H[q, j] = observer q applied to x_j;  X (d x nkeep): the kept solutions;  omegas;  info (wae_solve_info as a dict)"""

    def __init__(self, H, X, omegas, info):
        self.H, self.X, self.omegas, self.info = H, X, omegas, info


def pack_sparse_vectors(vectors, d, what):
    """[(idx, val), ...] -> (ptr int64, idx int32, val complex128) in compressed form, checked: equal lengths, indices in 0..d-1, finite values"""
    ptr, idxs, vals = [0], [], []
    for k, v in enumerate(vectors):
        try:
            idx, val = v
        except (TypeError, ValueError):
            raise ValueError(f"{what} {k}: expected a pair (idx, val)") from None
        idx = np.asarray(idx)
        val = np.asarray(val, dtype=np.complex128)
        if idx.ndim != 1 or val.shape != idx.shape:
            raise ValueError(f"{what} {k}: idx has shape {idx.shape}, val has shape {val.shape}")
        if len(idx) and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"{what} {k}: idx must hold integers")
        if len(idx) and (idx.min() < 0 or idx.max() >= d):
            raise ValueError(f"{what} {k}: an index lies outside 0..{d - 1}")
        if not np.all(np.isfinite(val)):
            raise ValueError(f"{what} {k}: a value is not finite")
        idxs.append(idx.astype(np.int32))
        vals.append(val)
        ptr.append(ptr[-1] + len(idx))
    cat = (lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros(0, dtype=dt))
    return np.asarray(ptr, dtype=np.int64), cat(idxs, np.int32), cat(vals, np.complex128)


def _coefficient_table(fam, omegas):
    """fam.coefficients(ω_j) for every frequency (mode "all", the eigenvalue parameter active, the aux term skipped: its coefficient is 0);
    params / active / mode are restored, as ensure_solver does"""
    saved = dict(fam.params), list(fam.active), fam.mode
    fam.active, fam.mode = [fam.eigval], "all"
    try:
        return np.ascontiguousarray([fam.coefficients(w) for w in omegas], dtype=np.complex128).reshape(len(omegas), len(fam.terms))
    finally:
        fam.params, fam.active, fam.mode = saved


def forced_response(L, rhs, omegas, observers=(), keep=(), tol=None, maxit=None):
    """x_j = L(ω_j) \\ rhs(ω_j) for every ω_j in ``omegas``.  ``rhs``: a family of d x 1 sparse column terms (``helmholtz.speaker_source``);
    ``observers``: sparse functionals (idx, val), e.g. from ``helmholtz.probe``; ``keep``: ascending indices into ``omegas`` of the solutions
    to return in full.  Returns a ``ForcedResponse``; an inner solve that misses the tolerance raises an ``UnconvergedWarning`` by the rule of
    ``DeviceFamily.solve``."""
    omegas = np.atleast_1d(np.asarray(omegas, dtype=np.complex128))
    if omegas.ndim != 1:
        raise ValueError(f"omegas must be a list of frequencies, got shape {omegas.shape}")
    d = L.size()
    sources = []
    for k, term in enumerate(rhs.terms):
        m = sp.coo_matrix(term.coeff)
        if m.shape != (d, 1):
            raise ValueError(f"term {k} of rhs has shape {m.shape}, the operator family has {d} rows: expected ({d}, 1)")
        m.sum_duplicates()
        sources.append((m.row, m.data))
    src = pack_sparse_vectors(sources, d, "source vector")
    obs = pack_sparse_vectors(observers, d, "observer")
    keep = np.asarray(keep, dtype=np.int64).reshape(-1) if np.size(keep) else np.zeros(0, dtype=np.int64)
    if len(keep) and (keep.min() < 0 or keep.max() >= len(omegas)):
        raise ValueError(f"keep: an index lies outside 0..{len(omegas) - 1}")
    if np.any(np.diff(keep) <= 0):
        raise ValueError("keep must be strictly ascending")
    if len(omegas) and len(obs[0]) == 1 and not len(keep):
        raise ValueError("nothing was asked for: give observers, keep, or both")
    ct = _coefficient_table(L, omegas)
    sc = _coefficient_table(rhs, omegas)
    fam = L.ensure_solver()
    H, X, info = fam.forced_response(ct, src, sc, obs, keep, tol=L.solver_tol if tol is None else tol, maxit=L.solver_maxit if maxit is None else maxit)
    return ForcedResponse(H, X, omegas, info)
