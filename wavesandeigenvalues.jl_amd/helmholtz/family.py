"""Assemble a device-backed LinearOperatorFamily from Helmholtz term matrices -- the family
``Helmholtz.discretize`` returns in the reference (src/Helmholtz.jl:507-522,571-574):

    L(ω) = ω²·M + K + ω·Y·C + n·exp(-iωτ)·Q      and the auxiliary term  -λ·M  ("__aux__") last.
"""
from __future__ import annotations

import numpy as np

from ..nlevp.algebra import exp_delay, pow1, pow2
from ..nlevp.linopfam import LinearOperatorFamily, Term
from . import annulus


def helmholtz_family(terms, Y=1e15, n=1.0, tau=1e-3, device=0, flame=True):
    """terms: dict with scipy matrices M, K, C, Q (as produced by discretize / the fixtures)."""
    L = LinearOperatorFamily(["ω", "λ"], [0.0, complex(np.inf, 0)], device=device)
    # M, K, C are symmetric by construction (element matrices of src/FEM/FEM.jl:435-441,704-710,1745-1766) but, summed in floating
    # point, only to rounding: tell the library so, and `A'*y` / `A'\\b` stay on the fast path (include/waehip.h, opts[0])
    L.symmetry_tol = 1e-14
    L.push(Term(terms["M"], (pow2,), (("ω",),), "ω^2", "M"))
    L.push(Term(terms["K"], (), (), "", "K"))
    L.params["Y"] = complex(Y)
    L.push(Term(terms["C"], (pow1, pow1), (("ω",), ("Y",)), "ω*Y", "C"))
    if flame:
        L.params["n"] = complex(n)
        L.params["τ"] = complex(tau)
        L.push(Term(terms["Q"], (pow1, exp_delay), (("n",), ("ω", "τ")), "n*exp(-iωτ)", "Q"))
    L.push(Term(-terms["M"], (pow1,), (("λ",),), "-λ", "__aux__"))
    return L


def herm_hierarchy(Lp, points, tets, tris=None, device=None):
    """Give a Hermite family (terms from ``assemble_herm*`` on this mesh, ``tris`` as there) the set-up that makes its inner solves
    converge: the p-hierarchy full space -> point unknowns -> P1 as ``solver_prolongators`` (``assemble.herm_prolongators``, built on the
    device) and ``solver_level_weights = "spectral"``, the Jacobi weights of every level scaled by its own spectral estimate.  Without
    it the default set-up stagnates on cubic elements.  A solver set-up that exists already is dropped.  Returns Lp."""
    from .assemble import herm_prolongators
    Ps = herm_prolongators(points, tets, tris, device=Lp.device_id if device is None else device)
    if Ps[0].shape[0] != Lp.size():
        raise ValueError(f"the Hermite space of this mesh has {Ps[0].shape[0]} unknowns, the family {Lp.size()}")
    Lp.solver_prolongators = Ps
    Lp.solver_level_weights = "spectral"
    if Lp._fam is not None:
        Lp._fam.solver_ready = False
    return Lp


def speaker_source(m, Y=1e15, A=1.0, device=0):
    """The ``rhs`` family that ``discretize(mesh, dscrp, c, source=true)`` returns for a :speaker boundary (src/Helmholtz.jl:79,251-258,
    501-505,519-522): rhs(ω) = ω·Y·A·m with m = -i·s the column of ``assemble_p1_source`` / ``assemble_p2_source``; the response to an
    excitation at ω is L(ω) \\ rhs(ω) (``nlevp.forced_response``), L carrying the ω·Y·C term of the same triangles."""
    rhs = LinearOperatorFamily(["ω"], [0.0], device=device)
    rhs.params["Y"] = complex(Y)
    rhs.params["A"] = complex(A)
    rhs.push(Term(m, (pow1, pow1, pow1), (("ω",), ("Y",), ("A",)), "speaker", "m"))
    return rhs


def annulus_family(preset="C2", device=0, **kw):
    """The synthetic annular combustor as a device-backed family; returns (L, problem dict)."""
    pb = annulus.build(preset, **{k: v for k, v in kw.items() if k in ("Y", "n", "tau", "grid")})
    p = pb["params"]
    L = helmholtz_family(pb["terms"], Y=p["Y"], n=p["n"], tau=p["τ"], device=device)
    return L, pb
