#!/usr/bin/env python3
"""Writes wavesandeigenvalues.jl_amd/csrc/herm_tables.h: the reference-element tables of the Hermite (cubic) tetrahedron and of its trace
on a face, derived in exact rational arithmetic from the definition of the element alone.

Reference tetrahedron: xi in R^3, corners v0 = e0, v1 = e1, v2 = e2, v3 = 0 (x = p3 + J xi with J[:, j] = p_j - p_3).  The space is P3, its
basis psi_0..psi_19 is dual to the functionals
    0..3    u(v_k)
    4..15   d u / d xi_j (v_k)      at position 4 (1 + j) + k
    16..19  u at the centroid of the face opposite v_k.
Reference triangle: eta in R^2, corners w0 = (1, 0), w1 = (0, 1), w2 = 0; P3 with the 10 functionals u(w_k) (0..2), d u / d eta_j (w_k) at
3 (1 + j) + k (3..8), u at the centroid (9).

The basis is the inverse of the functional-by-monomial matrix; every integral is the monomial formula
    int xi^alpha = prod(alpha_i!) / (|alpha| + n)!        (n = 3 or 2, unit simplex).
Tables: mass[a][b] = int psi_a psi_b; stiff[a][b][s] = int d_i psi_a d_j psi_b (+ the transposed pair for i != j) with
s = (i, j) in (00, 01, 02, 11, 12, 22), to be contracted with the symmetric J^-1 J^-T; src[a] = int psi_a; tri[a][b] = int psi_a psi_b on the
triangle; coef[a][m] the coefficient of monomial m (exponents exp[m]) in psi_a.

Run it from anywhere: it rewrites the header in place, byte for byte the same (tests/test_herm_args.py runs main(out=...) into a
temporary file and compares)."""
import os
from fractions import Fraction
from itertools import product
from math import factorial

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "wavesandeigenvalues.jl_amd", "csrc", "herm_tables.h")


def monomials(nvar, degree=3):
    return [e for e in product(range(degree + 1), repeat=nvar) if sum(e) <= degree]


def mono_value(e, x):
    v = Fraction(1)
    for k, xk in zip(e, x):
        v *= Fraction(xk) ** k
    return v


def mono_diff(e, j):
    """(factor, exponents) of d/dx_j of the monomial"""
    if e[j] == 0:
        return Fraction(0), e
    f = list(e)
    f[j] -= 1
    return Fraction(e[j]), tuple(f)


def functionals(nvar):
    """every functional as a function monomial -> Fraction, in local order"""
    corners = [tuple(Fraction(int(i == k)) for i in range(nvar)) for k in range(nvar)] + [tuple(Fraction(0) for _ in range(nvar))]
    fs = [lambda e, v=v: mono_value(e, v) for v in corners]
    for j in range(nvar):
        for v in corners:
            def d(e, v=v, j=j):
                c, f = mono_diff(e, j)
                return c * mono_value(f, v)
            fs.append(d)
    if nvar == 3:
        for k in range(4):
            cen = tuple(sum(corners[m][i] for m in range(4) if m != k) / 3 for i in range(3))
            fs.append(lambda e, c=cen: mono_value(e, c))
    else:
        cen = tuple(sum(corners[m][i] for m in range(3)) / 3 for i in range(2))
        fs.append(lambda e, c=cen: mono_value(e, c))
    return fs


def invert(A):
    n = len(A)
    M = [list(row) + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        M[c] = [x / piv for x in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [x - f * y for x, y in zip(M[r], M[c])]
    return [row[n:] for row in M]


def basis(nvar):
    """coef[a][m]: psi_a = sum_m coef[a][m] mono_m, with functional_f(psi_a) = delta_fa"""
    mons = monomials(nvar)
    fs = functionals(nvar)
    assert len(fs) == len(mons)
    A = [[f(e) for e in mons] for f in fs]
    Ai = invert(A)                                    # A coef^T = I
    coef = [[Ai[m][a] for m in range(len(mons))] for a in range(len(fs))]
    for f_i, f in enumerate(fs):                      # the duality, checked
        for a in range(len(fs)):
            assert sum(coef[a][m] * f(e) for m, e in enumerate(mons)) == int(f_i == a)
    return mons, coef


def integral(e):
    num = 1
    for k in e:
        num *= factorial(k)
    return Fraction(num, factorial(sum(e) + len(e)))


def poly(coefs, mons):
    return {e: c for e, c in zip(mons, coefs) if c != 0}


def pmul(p, q):
    out = {}
    for ea, ca in p.items():
        for eb, cb in q.items():
            e = tuple(x + y for x, y in zip(ea, eb))
            out[e] = out.get(e, Fraction(0)) + ca * cb
    return out


def pdiff(p, j):
    out = {}
    for e, c in p.items():
        f, g = mono_diff(e, j)
        if f != 0:
            out[g] = out.get(g, Fraction(0)) + c * f
    return out


def pint(p):
    return sum((c * integral(e) for e, c in p.items()), Fraction(0))


def fmt(x):
    return repr(float(x))                             # Fraction -> float is correctly rounded, repr round-trips


def main(out=OUT):
    mons, coef = basis(3)
    fs = [poly(c, mons) for c in coef]
    mass = [[pint(pmul(a, b)) for b in fs] for a in fs]
    d = [[pdiff(f, j) for j in range(3)] for f in fs]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    stiff = [[[pint(pmul(d[a][i], d[b][j])) + (pint(pmul(d[a][j], d[b][i])) if i != j else 0) for i, j in pairs] for b in range(20)]
             for a in range(20)]
    src = [pint(f) for f in fs]
    assert sum(src[:4]) + sum(src[16:]) == Fraction(1, 6) and all(mass[a][b] == mass[b][a] for a in range(20) for b in range(20))
    tmons, tcoef = basis(2)
    tf = [poly(c, tmons) for c in tcoef]
    tri = [[pint(pmul(a, b)) for b in tf] for a in tf]
    L = ["// Reference-element tables of the Hermite (cubic) tetrahedron and of its trace on a face.",
         "// Generated by dev/gen_herm_tables.py from the dual-basis definition in exact rational arithmetic: edit the generator, not this file.",
         "#pragma once",
         "",
         "struct HermTables {",
         "    double mass[20][20];        // int psi_a psi_b over the unit tetrahedron",
         "    double stiff[20][20][6];    // int d_i psi_a d_j psi_b (+ the pair (j, i) if i != j), (i, j) = 00, 01, 02, 11, 12, 22",
         "    double src[20];             // int psi_a",
         "    double tri[10][10];         // int psi_a psi_b over the unit triangle, the 10 functions of the trace",
         "};",
         "",
         "constexpr HermTables kHermTables = {",
         "    {"]
    for a in range(20):
        L.append("        {" + ", ".join(fmt(x) for x in mass[a]) + "},")
    L.append("    },")
    L.append("    {")
    for a in range(20):
        L.append("        {")
        for b in range(20):
            L.append("            {" + ", ".join(fmt(x) for x in stiff[a][b]) + "},")
        L.append("        },")
    L.append("    },")
    L.append("    {" + ", ".join(fmt(x) for x in src) + "},")
    L.append("    {")
    for a in range(10):
        L.append("        {" + ", ".join(fmt(x) for x in tri[a]) + "},")
    L.append("    },")
    L.append("};")
    L.append("")
    L.append("// psi_a = sum_m kHermCoef[a][m] xi^kHermExp[m]")
    L.append("constexpr int kHermExp[20][3] = {" + ", ".join("{%d, %d, %d}" % e for e in mons) + "};")
    L.append("constexpr double kHermCoef[20][20] = {")
    for a in range(20):
        L.append("    {" + ", ".join(fmt(x) for x in coef[a]) + "},")
    L.append("};")
    text = "\n".join(L) + "\n"
    with open(out, "w", newline="\n") as f:
        f.write(text)
    print("wrote", os.path.normpath(out), len(text), "bytes; src =", [str(x) for x in src])


if __name__ == "__main__":
    main()
