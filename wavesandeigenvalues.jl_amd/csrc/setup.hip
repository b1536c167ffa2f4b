// libwaehip.so -- construction: the family handle from the caller's term matrices (wae_family_create_opts) and the multigrid
// hierarchy with its work spaces (wae_solver_setup, and wae_solver_setup_nested from prolongators the caller supplies).  Host code and
// uploads only, but for the Galerkin products of the supplied levels (galerkin.hip); the solvers that use what is built here: solver.h.
#include <atomic>
#include <cmath>
#include <exception>
#include <limits>
#include <map>
#include <memory>
#include <tuple>

#include "family.h"

// ----------------------------------------------------------------------------------------------------
// level operators on device
// ----------------------------------------------------------------------------------------------------
OpDev LevelOp::dev(int op) const {
    OpDev o;
    memset(&o, 0, sizeof(o));
    o.ngroups = (int)groups.size();
    o.nplanes_total = nplanes;
    o.n = n;
    o.diag = diag.p;
    o.conj_diag = (op == WAE_OP_C) ? 1 : 0;
    o.tiles = !tiles.ready ? nullptr : (op == WAE_OP_N || tiles.all_symmetric) ? &tiles.dev : (tiles.ready_t ? &tiles.dev_t : nullptr);
    {
        const LongRows &LR = (op == WAE_OP_N) ? long_n : long_t;
        o.nlong = LR.n;
        o.long_rows = LR.rows.p; o.long_ptr = LR.ptr.p; o.long_col = LR.col.p; o.long_slot = LR.slot.p;
        o.long_val = LR.val.p; o.long_acc = LR.acc.p; o.long_part = LR.part.p;
        o.long_conj = (op == WAE_OP_C) ? 1 : 0;
    }
    for (size_t g = 0; g < groups.size(); ++g) {
        const GroupHost &G = groups[g];
        GroupDev &D = o.g[g];
        const bool tr = (op != WAE_OP_N) && !G.symmetric;
        D.rowptr = tr ? G.rowptr_t.p : G.rowptr.p;
        D.col = tr ? G.col_t.p : G.col.p;
        D.vals = tr ? (const void *)G.vals_t.p : (const void *)G.vals.p;
        D.nplanes = G.nplanes;
        D.is_real = G.is_real ? 1 : 0;
        D.plane0 = G.plane0;
        D.conj_vals = (op == WAE_OP_C && !G.is_real) ? 1 : 0;
    }
    return o;
}
static OpDev transfer_dev(const DevBuf<int> &ptr, const DevBuf<int> &col, const DevBuf<double> &val, int64_t n) {
    OpDev o;
    memset(&o, 0, sizeof(o));
    o.ngroups = 1;
    o.nplanes_total = 1;
    o.n = n;
    o.g[0].rowptr = ptr.p;
    o.g[0].col = col.p;
    o.g[0].vals = val.p;
    o.g[0].nplanes = 1;
    o.g[0].is_real = 1;
    return o;
}
OpDev Transfer::devP() const { return transfer_dev(p_ptr, p_col, p_val, nf); }
OpDev Transfer::devR() const {
    OpDev o = transfer_dev(r_ptr, r_col, r_val, nc);
    o.tiles = r_tiles.ready ? &r_tiles.dev : nullptr;
    return o;
}

// ----------------------------------------------------------------------------------------------------
// switches and debug lines of create / set-up
// ----------------------------------------------------------------------------------------------------
// Read once per call of wae_family_create_opts / wae_solver_setup, not once per process: the tests change them between handles.
struct SetupEnv {
    bool debug = getenv("WAE_SETUP_DEBUG") != nullptr;          // the [create] / [setup] / [tiles] lines on stderr
    bool reorder = env_int("WAE_REORDER", 1) != 0;              // 0: keep the caller's row numbering, no tiles (A/B measurements)
    // fine level: two window buffers of 608 rows x 128 B.  WAE_TILE_NBUF=3: three of 400 (two windows in flight while a third is
    // read) -- measured slower, 966 vs 733 us at 1M unknowns and 64 columns: a chunk costs a wavefront the same ~10 k cycles
    // whether its tile has 174 rows or 256 (lane = row), the gather was not what it waited for.
    int nbuf = env_int("WAE_TILE_NBUF", 2);
    int wcap = env_int("WAE_TILE_WCAP", nbuf == 3 ? 400 : 608);
    bool tile_level1 = env_int("WAE_TILE_LEVEL1", 1) != 0;      // 0: level 1 keeps its numbering, no tiles there
    bool tile_restrict = env_int("WAE_TILE_RESTRICT", 1) != 0;  // 0: the restriction of level 0 stays a CSR product
    bool xfer_tiles = xfer_tiles_on();
    int long_row = getenv("WAE_LONG_ROW") ? std::max(1, env_int("WAE_LONG_ROW", 0)) : WAE_LONG_ROW;   // (tests lower it)
};
constexpr int TILE_THICK = 6;           // plan_tiles: strips per shell
constexpr int TILE_WCAP_COARSE = 608;   // window rows of the tiles of level 1 and of the restriction (two window buffers)

// "<prefix> <what, padded to width> <seconds since the previous line>"; sync (optional): the stream whose work the lap includes
struct Lap {
    bool on;
    const char *prefix;
    int width;
    hipStream_t sync = nullptr;
    double t = now_s();
    void operator()(const char *what) {
        if (!on) return;
        if (sync) HIP_CHECK(hipStreamSynchronize(sync));
        const double t1 = now_s();
        fprintf(stderr, "%s %-*s %.3f s\n", prefix, width, what, t1 - t);
        t = t1;
    }
};

static bool plane_is_real(const CsrZ &A) {
    for (const zc &v : A.val)
        if (v.imag() != 0.0) return false;
    return true;
}

// ----------------------------------------------------------------------------------------------------
// level operator: pattern groups, transposed copies, long rows, upload
// ----------------------------------------------------------------------------------------------------
struct PlaneGroup { std::vector<int> members; bool real; };     // planes of one sparsity pattern, all real or all complex
static std::vector<PlaneGroup> group_planes(const std::vector<CsrZ> &planes) {
    std::vector<PlaneGroup> grps;
    for (int q = 0; q < (int)planes.size(); ++q) {
        const bool re = plane_is_real(planes[q]);
        bool placed = false;
        for (auto &g : grps)
            if (g.real == re && csr_same_pattern(planes[g.members[0]], planes[q])) { g.members.push_back(q); placed = true; break; }
        if (!placed) grps.push_back(PlaneGroup{{q}, re});
    }
    if ((int)grps.size() > WAE_MAXG) throw WaeError(WAE_ERR_INVALID, "too many distinct sparsity patterns (max 24)");
    if ((int)planes.size() > WAE_MAXP) throw WaeError(WAE_ERR_INVALID, "too many distinct term matrices (max 64)");
    return grps;
}

// body(lo, hi, t) over nth contiguous ranges of [0, n), one host thread each; an exception of any range is rethrown here
template <class F> static void host_ranges(int64_t n, int nth, F &&body) {
    if (nth <= 1) { body((int64_t)0, n, 0); return; }
    std::vector<std::future<void>> jobs;
    for (int t = 0; t < nth; ++t) {
        const int64_t lo = n * t / nth, hi = n * (t + 1) / nth;
        jobs.push_back(std::async(std::launch::async, [&body, lo, hi, t]() { body(lo, hi, t); }));
    }
    std::exception_ptr first;
    for (auto &j : jobs) {
        try { j.get(); } catch (...) { if (!first) first = std::current_exception(); }
    }
    if (first) std::rethrow_exception(first);
}
static int row_threads(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 8192)); }

// Symmetry test: same pattern and mirror entries that agree exactly (sym_tol = 0) or to within sym_tol of the smaller of the two
// rows' off-diagonal scales.  Why a tolerance exists at all: a finite-element matrix assembled in floating point is symmetric only
// up to the order of its element sums (K and M of the 200k..1M-DoF annulus: mirror entries differ by 1e-16 of the row scale in half
// of the positions), and the exact test sends every adjoint product of such a family through a second, transposed copy of the
// operator and past the tile kernel.  A plane accepted with sym_tol > 0 is applied in its stored orientation for op = T / C: the
// product then differs from the exact transposed one by that assembly rounding.  The caller asks for it
// (wae_family_create_opts); the hierarchy's own coarse levels use 1e-14.
static std::vector<double> row_scales(const CsrZ &P) {          // largest off-diagonal magnitude per row
    std::vector<double> sc((size_t)P.n, 0.0);
    host_ranges(P.n, row_threads(P.n), [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) {
            double m = 0.0;
            for (int p = P.ptr[i]; p < P.ptr[i + 1]; ++p)
                if (P.col[p] != (int)i) m = std::max(m, std::norm(P.val[p]));
            sc[(size_t)i] = std::sqrt(m);
        }
    });
    return sc;
}
// The mirror entry a_ji is looked up in row j (sorted columns) on the host threads.  1 symmetric, 0 not, -1 unsorted rows (undecided)
static int mirror_test(const CsrZ &P, double sym_tol) {
    if (P.n != P.m) return 0;
    std::vector<double> sc;
    if (sym_tol > 0.0) sc = row_scales(P);
    const int nth = row_threads(P.n);
    std::vector<int> verdict(nth, 1);
    host_ranges(P.n, nth, [&](int64_t lo, int64_t hi, int t) {
        int vd = 1;                                // (thread-local: the per-thread slots share cache lines)
        for (int64_t i = lo; i < hi && vd == 1; ++i)
            for (int p = P.ptr[i]; p < P.ptr[i + 1]; ++p) {
                if (p > P.ptr[i] && P.col[p - 1] >= P.col[p]) { vd = -1; break; }
                const int j = P.col[p];
                if (j == i) continue;
                const int *b = P.col.data() + P.ptr[j], *e = P.col.data() + P.ptr[j + 1];
                const int *f = std::lower_bound(b, e, (int)i);
                if (f == e || *f != (int)i) { vd = 0; break; }
                const zc m = P.val[(size_t)(f - P.col.data())];
                if (m == P.val[p]) continue;
                if (!(sym_tol > 0.0 && std::abs(P.val[p] - m) <= sym_tol * std::min(sc[(size_t)i], sc[(size_t)j]))) { vd = 0; break; }
            }
        verdict[t] = vd;
    });
    int v = 1;
    for (int t = 0; t < nth; ++t) { if (verdict[t] == -1) v = -1; else if (verdict[t] == 0 && v == 1) v = 0; }
    return v;
}
// Is every plane of the group symmetric?  The transposed copies (tr) are built only for a group that fails the mirror test -- it
// needs them -- or whose rows are not sorted: then the transpose decides, as it used to.
static bool group_symmetric(const std::vector<CsrZ> &planes, const std::vector<int> &members, double sym_tol, std::vector<CsrZ> &tr) {
    const CsrZ &A0 = planes[members[0]];
    bool sym = (A0.n == A0.m);
    bool undecided = false;
    for (size_t k = 0; k < members.size() && sym; ++k) {
        const int v = mirror_test(planes[members[k]], sym_tol);
        if (v == 0) sym = false;
        if (v < 0) { undecided = true; break; }
    }
    if (sym && !undecided) return true;
    std::vector<std::future<CsrZ>> tj;
    for (int q : members) tj.push_back(std::async(std::launch::async, [&planes, q]() { return csr_transpose(planes[q]); }));
    for (size_t k = 0; k < tj.size(); ++k) {
        tr.push_back(tj[k].get());
        if (!sym) continue;
        const CsrZ &P0 = planes[members[k]], &P1 = tr.back();
        if (!(P1.ptr == P0.ptr && P1.col == P0.col)) { sym = false; continue; }
        std::vector<double> sc;
        if (sym_tol > 0.0) sc = row_scales(P0);
        for (int64_t i = 0; i < P0.n && sym; ++i)          // (same pattern: entry e of P1 is the mirror of entry e of P0)
            for (int e = P0.ptr[i]; e < P0.ptr[i + 1]; ++e) {
                if (P0.val[e] == P1.val[e]) continue;
                const int j = P0.col[e];
                if (!(sym_tol > 0.0 && j != i && std::abs(P0.val[e] - P1.val[e]) <= sym_tol * std::min(sc[(size_t)i], sc[(size_t)j]))) { sym = false; break; }
            }
    }
    return sym;
}

// long rows go to the level's long-row store (OpDev) and leave the group's CSR arrays
struct LongEntries {
    std::map<int, std::vector<std::tuple<int, int, zc>>> rows;      // row -> (column, slot, value)
    void add(int r, int c, int slot, zc v) { rows[r].emplace_back(c, slot, v); }
};
static bool strip_long_rows(const std::vector<const CsrZ *> &src, int plane0, int limit, std::vector<CsrZ> &kept, LongEntries &LE) {
    std::vector<char> is_long(src[0]->n, 0);
    bool any = false;
    for (int64_t i = 0; i < src[0]->n; ++i)
        if (src[0]->ptr[i + 1] - src[0]->ptr[i] > limit) { is_long[i] = 1; any = true; }
    if (!any) return false;
    for (size_t k = 0; k < src.size(); ++k) {
        const CsrZ &A = *src[k];
        CsrZ B;
        B.n = A.n; B.m = A.m;
        B.ptr.assign(A.n + 1, 0);
        for (int64_t i = 0; i < A.n; ++i) {
            if (is_long[i]) {
                for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p) LE.add((int)i, A.col[p], plane0 + (int)k, A.val[p]);
            } else {
                B.col.insert(B.col.end(), A.col.begin() + A.ptr[i], A.col.begin() + A.ptr[i + 1]);
                B.val.insert(B.val.end(), A.val.begin() + A.ptr[i], A.val.begin() + A.ptr[i + 1]);
            }
            B.ptr[i + 1] = (int)B.col.size();
        }
        kept.push_back(std::move(B));
    }
    return true;
}
static void upload_long(const LongEntries &LE, LongRows &LR, hipStream_t st) {
    LR = LongRows();
    LR.n = (int)LE.rows.size();
    if (!LR.n) return;
    std::vector<int> rows, ptr(1, 0), col, slot;
    std::vector<cplx> val;
    for (const auto &kv : LE.rows) {
        rows.push_back(kv.first);
        for (const auto &e : kv.second) { col.push_back(std::get<0>(e)); slot.push_back(std::get<1>(e)); val.push_back(cplx{std::get<2>(e).real(), std::get<2>(e).imag()}); }
        ptr.push_back((int)col.size());
    }
    LR.rows.upload(rows.data(), rows.size(), st); LR.ptr.upload(ptr.data(), ptr.size(), st);
    LR.col.upload(col.data(), col.size(), st); LR.slot.upload(slot.data(), slot.size(), st);
    LR.val.upload(val.data(), val.size(), st);
    LR.acc.alloc((size_t)LR.n * 256);                     // batch widths up to 256 columns
    LR.part.alloc((size_t)LR.n * WAE_LONG_SPLIT * 256);
    HIP_CHECK(hipStreamSynchronize(st));
}

// One orientation of a group on its way to the device: long rows out (into LE), the planes' values interleaved [entry][plane]
// (doubles, or re / im pairs).  The copies are asynchronous: the object must live until the stream has been synchronised.
struct GroupUpload {
    std::vector<CsrZ> kept;                 // the planes without their long rows (empty: there were none)
    std::vector<double> packed;
    bool stripped = false;
    GroupUpload(const std::vector<const CsrZ *> &src, int plane0, bool real, int limit, LongEntries &LE, DevBuf<int> &rowptr, DevBuf<int> &col,
                DevBuf<double> &vals, hipStream_t st) {
        stripped = strip_long_rows(src, plane0, limit, kept, LE);
        std::vector<const CsrZ *> mats = src;
        if (stripped) for (size_t k = 0; k < kept.size(); ++k) mats[k] = &kept[k];
        const int np = (int)mats.size(), w = real ? 1 : 2;
        const int64_t nnz = mats[0]->nnz();
        packed.resize((size_t)nnz * np * w);
        // (host threads: entries in contiguous ranges)
        host_ranges(nnz, (int)std::max<int64_t>(1, std::min<int64_t>(8, nnz / 262144)), [&](int64_t lo, int64_t hi, int) {
            for (int64_t p = lo; p < hi; ++p)
                for (int k = 0; k < np; ++k) {
                    const zc v = mats[k]->val[p];
                    if (real) packed[(size_t)p * np + k] = v.real();
                    else { packed[((size_t)p * np + k) * 2] = v.real(); packed[((size_t)p * np + k) * 2 + 1] = v.imag(); }
                }
        });
        rowptr.upload(mats[0]->ptr.data(), mats[0]->ptr.size(), st);
        col.upload(mats[0]->col.data(), mats[0]->col.size(), st);
        vals.upload(packed.data(), packed.size(), st);
    }
};

// Build the device representation of sum_q pc[q] plane_q from host planes; returns slot -> plane map.
// sym_tol: when is a plane "symmetric", i.e. applied in its stored orientation for op = T / C?  0: only if mirror entries are equal
// bit for bit (A' is exactly A').  > 0: if  |a_ij - a_ji| <= sym_tol * min(s_i, s_j),  s_i = the largest OFF-DIAGONAL magnitude of
// row i -- the rounding scale of a row's assembled sums that a penalty / Dirichlet diagonal entry cannot inflate.
static std::vector<int> build_levelop(LevelOp &L, const std::vector<CsrZ> &planes, hipStream_t st, double sym_tol, const SetupEnv &env) {
    L.n = planes.empty() ? 0 : planes[0].n;
    L.nplanes = (int)planes.size();
    const std::vector<PlaneGroup> grps = group_planes(planes);
    std::vector<int> slot_plane;
    L.groups.clear();
    L.groups.resize(grps.size());
    LongEntries long_n, long_t;
    for (size_t gi = 0; gi < grps.size(); ++gi) {
        const PlaneGroup &g = grps[gi];
        GroupHost &G = L.groups[gi];
        G.nplanes = (int)g.members.size();
        G.is_real = g.real;
        G.nnz = planes[g.members[0]].nnz();
        G.plane0 = (int)slot_plane.size();
        std::vector<const CsrZ *> own, trp;
        for (int q : g.members) { slot_plane.push_back(q); own.push_back(&planes[q]); }
        std::vector<CsrZ> tr;
        G.symmetric = group_symmetric(planes, g.members, sym_tol, tr);
        const GroupUpload un(own, G.plane0, g.real, env.long_row, long_n, G.rowptr, G.col, G.vals, st);
        if (un.stripped && G.symmetric) {                    // the T orientation aliases these arrays: same rows, same entries
            std::vector<CsrZ> dummy;
            strip_long_rows(own, G.plane0, env.long_row, dummy, long_t);
        }
        std::unique_ptr<GroupUpload> ut;
        if (!G.symmetric) {
            for (const CsrZ &t : tr) trp.push_back(&t);
            ut.reset(new GroupUpload(trp, G.plane0, g.real, env.long_row, long_t, G.rowptr_t, G.col_t, G.vals_t, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));   // host staging buffers die at scope end
    }
    upload_long(long_n, L.long_n, st);
    upload_long(long_t, L.long_t, st);
    // diagonals [n][nplanes] in slot order
    std::vector<cplx> dg((size_t)L.n * L.nplanes, cplx{0.0, 0.0});
    for (int s = 0; s < L.nplanes; ++s) {
        const CsrZ &A = planes[slot_plane[s]];
        for (int64_t i = 0; i < A.n; ++i)
            for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p)
                if (A.col[p] == i) dg[(size_t)i * L.nplanes + s] = cplx{A.val[p].real(), A.val[p].imag()};
    }
    L.diag.upload(dg.data(), dg.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));
    return slot_plane;
}

// tile-local storage of an operator whose rows have been cut into tiles (tiles.h): windows and the bulk group (two real planes on
// one pattern).  U: pattern that defines the windows (every column any plane of the operator touches).
static bool build_tiles_core(TileStore &T, const std::vector<const CsrZ *> &bulk, const Pattern &U, const std::vector<int> &row_ptr, int lpr,
                             hipStream_t st, const char *what, bool debug, int nbuf = 2, int nwaves = 8) {
    T = TileStore();
    if (row_ptr.size() < 2) return false;
    const TileWindows W = build_windows(U, row_ptr);
    const int nt = (int)row_ptr.size() - 1;
    int wmax = 0;
    for (int t = 0; t < nt; ++t) wmax = std::max(wmax, W.win_ptr[t + 1] - W.win_ptr[t]);
    if (wmax > 65535) return false;
    nbuf = (nbuf == 3 && lpr == 2 && wmax <= 400) ? 3 : 2;
    T.row_ptr.upload(row_ptr.data(), row_ptr.size(), st);
    T.win_ptr.upload(W.win_ptr.data(), W.win_ptr.size(), st);
    T.win_cols.upload(W.win_cols.data(), W.win_cols.size(), st);
    memset(&T.dev, 0, sizeof(T.dev));
    {
        const TileGroupHost H = build_tile_group(bulk, true, row_ptr, W, lpr, nwaves);
        T.sptr.upload(H.sptr.data(), H.sptr.size(), st);
        T.sidx.upload(H.sidx.data(), H.sidx.size(), st);
        T.svals.upload(H.svals.data(), H.svals.size(), st);
        T.dslot.upload(H.dslot.data(), H.dslot.size(), st);
        HIP_CHECK(hipStreamSynchronize(st));                 // H dies at the end of this scope
        T.dev.g0 = TileGroupDev{T.sptr.p, T.sidx.p, T.svals.p, T.dslot.p};
        if (debug) {
            int over = 0, full = 0;                          // slices longer than the register-resident entries per lane
            for (size_t i = 0; i + 1 < H.sptr.size(); ++i) over += (H.sptr[i + 1] - H.sptr[i]) / 64 > (nwaves == 16 ? 4 : (lpr == 2 ? 8 : 12));
            for (int t = 0; t < nt; ++t) full += row_ptr[t + 1] - row_ptr[t] == 64 * nwaves / lpr;
            fprintf(stderr, "[tiles] %s: %d tiles (%d lanes per row, %d window buffers), %.1f rows and %.1f window rows per tile on average, %d full tiles, largest window %d\n",
                    what, nt, lpr, nbuf, (double)row_ptr[nt] / nt, (double)W.win_ptr[nt] / nt, full, wmax);
            fprintf(stderr, "[tiles] %s: %lld nonzeros in %lld slots (%.3f filled), %d of %zu slices stream entries\n", what,
                    (long long)bulk[0]->ptr.back(), (long long)H.sptr.back(), (double)bulk[0]->ptr.back() / (double)std::max(1, H.sptr.back()),
                    over, H.sptr.size() - 1);
        }
    }
    const std::vector<unsigned> zero(16, 0u);
    T.counters.upload(zero.data(), zero.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));
    T.dev.ntiles = nt;
    T.dev.wmax = wmax;
    T.dev.lpr = lpr;
    T.dev.nwaves = nwaves;
    T.dev.nbuf = nbuf;
    T.dev.row_ptr = T.row_ptr.p;
    T.dev.win_ptr = T.win_ptr.p;
    T.dev.win_cols = T.win_cols.p;
    T.dev.counters = T.counters.p;
    return true;
}

// Side rows of a tiled level operator: every entry of the groups other than the bulk group, row by row (level numbering), plane
// slot and complex value per entry.  transposed: the entries of the groups' transposes (symmetric groups as they are); rows longer
// than the long-row limit keep an empty CSR row and go to the long list (ls_*) instead
struct SideHost {
    std::vector<int> of_row, ptr, col, slot, ls_ptr, ls_col, ls_slot, ls_side;
    std::vector<cplx> val, ls_val;
    int nside = 0;
};
static SideHost build_side_rows(const LevelOp &L, const std::vector<CsrZ> &planes, const std::vector<int> &slot_plane, bool transposed, int limit) {
    SideHost S;
    const int64_t n = L.n;
    const size_t ng = L.groups.size();
    std::vector<CsrZ> trs;                                 // transposes of the non-symmetric planes, in (group, plane) order
    std::vector<const CsrZ *> src;                         // per (group >= 1, plane): the matrix to take rows from
    std::vector<int> src_slot;
    for (size_t g = 1; g < ng; ++g)
        for (int q = 0; q < L.groups[g].nplanes; ++q) {
            const CsrZ &A = planes[slot_plane[L.groups[g].plane0 + q]];
            src_slot.push_back(L.groups[g].plane0 + q);
            if (transposed && !L.groups[g].symmetric) trs.push_back(csr_transpose(A));
        }
    size_t it = 0;
    for (size_t g = 1; g < ng; ++g)
        for (int q = 0; q < L.groups[g].nplanes; ++q)
            src.push_back(transposed && !L.groups[g].symmetric ? &trs[it++] : &planes[slot_plane[L.groups[g].plane0 + q]]);
    std::vector<int> count((size_t)n, 0);
    for (const CsrZ *A : src)
        for (int64_t i = 0; i < n; ++i) count[(size_t)i] += A->ptr[i + 1] - A->ptr[i];
    S.of_row.assign((size_t)n, -1);
    S.ptr.assign(1, 0);
    S.ls_ptr.assign(1, 0);
    std::vector<char> is_long((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i)
        if (count[(size_t)i]) {
            S.of_row[(size_t)i] = (int)S.ptr.size() - 1;
            is_long[(size_t)i] = transposed && count[(size_t)i] > limit;
            S.ptr.push_back(S.ptr.back() + (is_long[(size_t)i] ? 0 : count[(size_t)i]));
        }
    S.nside = (int)S.ptr.size() - 1;
    S.col.resize((size_t)S.ptr.back()); S.slot.resize((size_t)S.ptr.back()); S.val.resize((size_t)S.ptr.back());
    std::vector<int> fill(S.ptr.begin(), S.ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) {                      // (long rows: one list per row, entries in (plane, column) order)
        if (!is_long[(size_t)i]) continue;
        for (size_t k = 0; k < src.size(); ++k)
            for (int p = src[k]->ptr[i]; p < src[k]->ptr[i + 1]; ++p) {
                S.ls_col.push_back(src[k]->col[p]); S.ls_slot.push_back(src_slot[k]);
                S.ls_val.push_back(cplx{src[k]->val[p].real(), src[k]->val[p].imag()});
            }
        S.ls_ptr.push_back((int)S.ls_col.size());
        S.ls_side.push_back(S.of_row[(size_t)i]);
    }
    for (size_t k = 0; k < src.size(); ++k) {
        const CsrZ &A = *src[k];
        for (int64_t i = 0; i < n; ++i) {
            if (is_long[(size_t)i]) continue;
            for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p) {
                const int e = fill[(size_t)S.of_row[(size_t)i]]++;
                S.col[(size_t)e] = A.col[p]; S.slot[(size_t)e] = src_slot[k]; S.val[(size_t)e] = cplx{A.val[p].real(), A.val[p].imag()};
            }
        }
    }
    return S;
}
// the side rows' CSR arrays on their way to the device (the caller synchronises before S dies) and their place in D
static void upload_side_rows(const SideHost &S, DevBuf<int> &of_row, DevBuf<int> &ptr, DevBuf<int> &col, DevBuf<int> &slot, DevBuf<cplx> &val,
                             DevBuf<cplx> &acc, TileDev &D, hipStream_t st) {
    of_row.upload(S.of_row.data(), S.of_row.size(), st);
    ptr.upload(S.ptr.data(), S.ptr.size(), st);
    if (S.nside) {
        col.upload(S.col.data(), S.col.size(), st);
        slot.upload(S.slot.data(), S.slot.size(), st);
        val.upload(S.val.data(), S.val.size(), st);
        acc.alloc((size_t)S.nside * 256);                    // batch widths up to 256 columns
    }
    D.nside = S.nside;
    D.side_of_row = of_row.p;
    D.side_ptr = ptr.p; D.side_col = col.p; D.side_slot = slot.p;
    D.side_val = val.p; D.side_acc = acc.p;
}

// ... of a level operator; planes in the level's numbering
static void build_level_tiles(LevelOp &L, const std::vector<CsrZ> &planes, const std::vector<int> &slot_plane, const std::vector<int> &row_ptr,
                              hipStream_t st, const SetupEnv &env, int lpr = 2, int nbuf = 2, int nwaves = 8) {
    TileStore &T = L.tiles;
    T = TileStore();
    if (L.groups.empty() || !L.groups[0].is_real || L.groups[0].nplanes != 2) return;   // the tile kernel's bulk group: two real planes
    const size_t ng = L.groups.size();
    {
        const GroupHost &G = L.groups[0];
        std::vector<const CsrZ *> mats;
        for (int q = 0; q < G.nplanes; ++q) mats.push_back(&planes[slot_plane[G.plane0 + q]]);
        if (!build_tiles_core(T, mats, union_pattern(planes), row_ptr, lpr, st, "operator", env.debug, nbuf, nwaves)) return;
    }
    T.all_symmetric = true;
    for (size_t g = 0; g < ng; ++g) T.all_symmetric = T.all_symmetric && L.groups[g].symmetric;
    {
        const SideHost S = build_side_rows(L, planes, slot_plane, false, env.long_row);
        upload_side_rows(S, T.side_of_row, T.side_ptr, T.side_col, T.side_slot, T.side_val, T.side_acc, T.dev, st);
        HIP_CHECK(hipStreamSynchronize(st));
        T.dev.nlong_side = 0;
        if (env.debug) fprintf(stderr, "[tiles] %d side rows with %d entries of the other %zu groups\n", S.nside, S.ptr.back(), ng - 1);
    }
    // The transposed orientation (op = T / C on a family with a non-symmetric term -- the flame term of the adjoint solves): the bulk
    // group must be symmetric (the tile storage itself is shared), the side rows are those of the other groups' transposes.
    if (!T.all_symmetric && L.groups[0].symmetric) {
        const SideHost S = build_side_rows(L, planes, slot_plane, true, env.long_row);
        T.dev_t = T.dev;
        upload_side_rows(S, T.t_side_of_row, T.t_side_ptr, T.t_side_col, T.t_side_slot, T.t_side_val, T.t_side_acc, T.dev_t, st);
        const int nls = (int)S.ls_side.size();
        if (nls) {
            T.t_ls_ptr.upload(S.ls_ptr.data(), S.ls_ptr.size(), st);
            T.t_ls_col.upload(S.ls_col.data(), S.ls_col.size(), st);
            T.t_ls_slot.upload(S.ls_slot.data(), S.ls_slot.size(), st);
            T.t_ls_val.upload(S.ls_val.data(), S.ls_val.size(), st);
            T.t_ls_side.upload(S.ls_side.data(), S.ls_side.size(), st);
            T.t_ls_part.alloc((size_t)nls * WAE_LONG_SPLIT * 256);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        T.dev_t.nlong_side = nls;
        T.dev_t.ls_ptr = T.t_ls_ptr.p; T.dev_t.ls_col = T.t_ls_col.p; T.dev_t.ls_slot = T.t_ls_slot.p; T.dev_t.ls_val = T.t_ls_val.p;
        T.dev_t.ls_side = T.t_ls_side.p;
        T.dev_t.ls_part = T.t_ls_part.p;
        T.ready_t = true;
        if (env.debug)
            fprintf(stderr, "[tiles] transposed orientation: %d side rows with %d entries, %d long rows with %d entries\n", S.nside, S.ptr.back(), nls,
                    S.ls_ptr.back());
    }
    T.ready = true;
}

// ----------------------------------------------------------------------------------------------------
// input conversion
// ----------------------------------------------------------------------------------------------------
static CsrZ term_to_csr(int64_t d, int index_bytes, int base, int orientation, const void *ptr, const void *idx, const double *val) {
    auto getp = [&](int64_t i) -> int64_t { return index_bytes == 4 ? (int64_t)((const uint32_t *)ptr)[i] : ((const int64_t *)ptr)[i]; };
    auto geti = [&](int64_t i) -> int64_t { return index_bytes == 4 ? (int64_t)((const uint32_t *)idx)[i] : ((const int64_t *)idx)[i]; };
    CsrZ A;
    A.n = A.m = d;
    const int64_t nnz = getp(d) - base;
    WAE_REQUIRE(nnz >= 0 && nnz < (int64_t)2147483647, "term nnz out of range");
    A.ptr.resize(d + 1);
    A.col.resize(nnz);
    A.val.resize(nnz);
    // (four threads per term, the terms themselves side by side in wae_family_create_opts: copying and checking 30 M entries of a
    // 1M-unknown family on one thread was 1.0 s of the 1.7 s a family takes to create)
    auto nth = [](int64_t n) { return (int)std::min<int64_t>(4, n / 65536 + 1); };
    host_ranges(d + 1, nth(d + 1), [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t p = getp(i) - base;
            WAE_REQUIRE(p >= 0 && p <= nnz, "pointer array out of range");
            A.ptr[i] = (int)p;
        }
    });
    host_ranges(nnz, nth(nnz), [&](int64_t lo, int64_t hi, int) {
        for (int64_t p = lo; p < hi; ++p) {
            const int64_t j = geti(p) - base;
            WAE_REQUIRE(j >= 0 && j < d, "index out of range");
            A.col[p] = (int)j;
            A.val[p] = zc(val[2 * p], val[2 * p + 1]);
        }
    });
    // rows already sorted without duplicates (what scipy and SparseArrays hand over): taken as they are
    std::atomic<bool> canonical{true};
    host_ranges(d, nth(d), [&](int64_t lo, int64_t hi, int) {
        bool ok = true;
        for (int64_t i = lo; i < hi; ++i) {
            WAE_REQUIRE(A.ptr[i] <= A.ptr[i + 1], "pointer array not monotone");
            for (int p = A.ptr[i] + 1; p < A.ptr[i + 1]; ++p) ok = ok && A.col[p - 1] < A.col[p];
        }
        if (!ok) canonical = false;
    });
    if (canonical) return orientation == WAE_CSC ? csr_transpose(A) : A;
    // sort + merge duplicates per row
    CsrZ S;
    S.n = S.m = d;
    S.ptr.assign(d + 1, 0);
    std::vector<std::pair<int, zc>> row;
    for (int64_t i = 0; i < d; ++i) {
        row.clear();
        for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p) row.emplace_back(A.col[p], A.val[p]);
        std::stable_sort(row.begin(), row.end(), [](const std::pair<int, zc> &a, const std::pair<int, zc> &b) { return a.first < b.first; });
        for (size_t k = 0; k < row.size(); ++k) {
            if (!S.col.empty() && (int)S.col.size() > S.ptr[i] && S.col.back() == row[k].first) S.val.back() += row[k].second;
            else { S.col.push_back(row[k].first); S.val.push_back(row[k].second); }
        }
        S.ptr[i + 1] = (int)S.col.size();
    }
    if (orientation == WAE_CSC) return csr_transpose(S);
    return S;
}

// term k == s * plane q exactly?
static bool proportional(const CsrZ &A, const CsrZ &P, zc &s) {
    if (!csr_same_pattern(A, P) || A.nnz() == 0) return false;
    int64_t p0 = -1;
    for (int64_t p = 0; p < P.nnz(); ++p)
        if (P.val[p] != zc(0)) { p0 = p; break; }
    if (p0 < 0) return false;
    s = A.val[p0] / P.val[p0];
    for (int64_t p = 0; p < P.nnz(); ++p)
        if (A.val[p] != s * P.val[p]) return false;
    return true;
}

// ... of the restriction R (rows: the coarse level's tile numbering, columns: the fine level's): consecutive rows are cut into tiles
// whose fine-level window fits LDS
static void build_restriction_tiles(Transfer &X, const CsrD &R, int wcap, hipStream_t st, bool debug) {
    X.r_tiles = TileStore();
    CsrZ Rz, Zz;                                             // plane 0 = R, plane 1 = 0 (the kernel's bulk group has two planes)
    Rz.n = R.n; Rz.m = R.m; Rz.ptr = R.ptr; Rz.col = R.col;
    Rz.val.resize(R.val.size());
    for (size_t i = 0; i < R.val.size(); ++i) Rz.val[i] = zc(R.val[i], 0.0);
    Zz.n = R.n; Zz.m = R.m; Zz.ptr = R.ptr; Zz.col = R.col;
    Zz.val.assign(R.val.size(), zc(0.0, 0.0));
    Pattern U;
    U.n = R.n; U.ptr = R.ptr; U.col = R.col;
    std::vector<int> row_ptr(1, 0), stamp((size_t)R.m, -1);
    int rows = 0, win = 0;
    for (int64_t i = 0; i < R.n; ++i) {
        if (R.ptr[i + 1] - R.ptr[i] > wcap) return;          // (a row that does not fit a window)
        int fresh = 0;
        const int t = (int)row_ptr.size() - 1;
        for (int p = R.ptr[i]; p < R.ptr[i + 1]; ++p) fresh += stamp[(size_t)R.col[p]] != t;
        if (rows == 128 || win + fresh > wcap) {
            row_ptr.push_back((int)i);
            rows = 0; win = 0;
        }
        const int t2 = (int)row_ptr.size() - 1;
        for (int p = R.ptr[i]; p < R.ptr[i + 1]; ++p)
            if (stamp[(size_t)R.col[p]] != t2) { stamp[(size_t)R.col[p]] = t2; ++win; }
        ++rows;
    }
    row_ptr.push_back((int)R.n);
    if (!build_tiles_core(X.r_tiles, {&Rz, &Zz}, U, row_ptr, 4, st, "restriction", debug)) return;
    X.r_tiles.dev.unit = 1;
    X.r_tiles.ready = true;
}

// The prolongation by fine tile (wae_internal.h XferTiles): P (fine x coarse, rows in the fine level's tile order), row_ptr = the fine tiles.
static void build_transfer_tiles(Transfer &X, const CsrD &P, const std::vector<int> &row_ptr, hipStream_t st) {
    XferTiles &F = X.ft;
    F.ready = false;
    const int nt = (int)row_ptr.size() - 1;
    if (nt <= 0 || row_ptr.back() != P.n) return;
    std::vector<int> tptr(nt + 1, 0), clist, stamp((size_t)P.m, -1), slot((size_t)P.m, 0);
    std::vector<unsigned short> ploc(P.col.size());
    int maxslots = 0, maxent = 0;
    std::vector<int> cols;
    for (int t = 0; t < nt; ++t) {
        const int a = row_ptr[t], b = row_ptr[t + 1];
        if (b - a > 256) return;                             // (the kernel walks at most 256 fine rows per workgroup)
        cols.clear();
        for (int p = P.ptr[a]; p < P.ptr[b]; ++p)
            if (stamp[(size_t)P.col[p]] != t) { stamp[(size_t)P.col[p]] = t; cols.push_back(P.col[p]); }
        std::sort(cols.begin(), cols.end());
        const int ns = (int)cols.size();
        maxslots = std::max(maxslots, ns);
        maxent = std::max(maxent, P.ptr[b] - P.ptr[a]);
        for (int k = 0; k < ns; ++k) slot[(size_t)cols[k]] = k;
        clist.insert(clist.end(), cols.begin(), cols.end());
        tptr[t + 1] = (int)clist.size();
        for (int p = P.ptr[a]; p < P.ptr[b]; ++p) ploc[p] = (unsigned short)slot[(size_t)P.col[p]];
    }
    maxent = (maxent + 3) & ~3;
    if ((size_t)maxslots * 128 + (size_t)maxent * 10 + 1100 > 60 * 1024) return;       // (LDS of the kernel)
    F.row_ptr.upload(row_ptr.data(), row_ptr.size(), st);
    F.tptr.upload(tptr.data(), tptr.size(), st);
    F.clist.upload(clist.data(), clist.size(), st);
    F.pptr.upload(P.ptr.data(), P.ptr.size(), st);
    F.ploc.upload(ploc.data(), ploc.size(), st);
    F.pval.upload(P.val.data(), P.val.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));                     // (the host vectors die at scope end)
    XferTilesDev &D = F.dev;
    D.ntiles = nt; D.maxslots = maxslots; D.maxent = maxent; D.nslots = (int64_t)clist.size(); D.nf = P.n; D.nc = P.m;
    D.row_ptr = F.row_ptr.p; D.tptr = F.tptr.p; D.clist = F.clist.p; D.pptr = F.pptr.p; D.ploc = F.ploc.p; D.pval = F.pval.p;
    F.ready = true;
}

// ----------------------------------------------------------------------------------------------------
// wae_family_create_opts: conversion / plane detection / tile plan / operator
// ----------------------------------------------------------------------------------------------------
// the terms' conversions side by side, a thread each
static std::vector<CsrZ> convert_terms(int64_t d, int T, int index_bytes, int base, int orientation, const void *const *ptr, const void *const *idx,
                                       const double *const *val) {
    std::vector<CsrZ> out(T);
    host_ranges(T, T, [&](int64_t k, int64_t, int) { out[k] = term_to_csr(d, index_bytes, base, orientation, ptr[k], idx[k], val[k]); });
    return out;
}
// distinct planes: a term that is an exact multiple of an earlier plane shares it
static void detect_planes(wae_family *h, std::vector<CsrZ> &terms) {
    for (int k = 0; k < h->T; ++k) {
        CsrZ A = std::move(terms[k]);
        h->term_nnz[k] = A.nnz();
        bool found = false;
        for (int q = 0; q < (int)h->planes0.size() && !found; ++q) {
            zc s;
            if (proportional(A, h->planes0[q], s)) { h->term_plane[k] = q; h->term_scale[k] = s; found = true; }
        }
        if (!found) {
            h->term_plane[k] = (int)h->planes0.size();
            h->term_scale[k] = 1.0;
            h->planes0.push_back(std::move(A));
        }
    }
    h->nplanes = (int)h->planes0.size();
}
// renumber the rows into compact tiles (tiles.h)
static void renumber_fine_level(wae_family *h, const SetupEnv &env) {
    const double tq0 = now_s();
    TilePlan plan = plan_tiles(union_pattern(h->planes0), 256, env.wcap, TILE_THICK);
    const double tq1 = now_s();
    if (!plan.perm.empty()) {
        host_ranges(h->nplanes, h->nplanes, [&](int64_t q, int64_t, int) { h->planes0[q] = permute_symmetric(h->planes0[q], plan.perm, plan.iperm); });
        h->perm_h = plan.perm;
        h->perm_dev.upload(h->perm_h.data(), h->perm_h.size(), h->stream);
        h->tile_row_ptr = plan.row_ptr;
    }
    if (env.debug)
        fprintf(stderr, "[create] tile plan %.3f s (%zu tiles, largest window %d), permutation of the planes %.3f s\n", tq1 - tq0,
                plan.row_ptr.empty() ? (size_t)0 : plan.row_ptr.size() - 1, plan.wmax, now_s() - tq1);
}

extern "C" int wae_family_create(wae_family **out, int64_t d, int32_t T, int32_t index_bytes, int32_t base, int32_t orientation,
                                 const void *const *ptr, const void *const *idx, const double *const *val, int32_t device) {
    return wae_family_create_opts(out, d, T, index_bytes, base, orientation, ptr, idx, val, device, nullptr, 0);
}

extern "C" int wae_family_create_opts(wae_family **out, int64_t d, int32_t T, int32_t index_bytes, int32_t base, int32_t orientation,
                                      const void *const *ptr, const void *const *idx, const double *const *val, int32_t device,
                                      const double *opts, int32_t nopts) {
    return guarded([&]() {
        WAE_REQUIRE(out && d > 0 && T > 0 && T <= 64, "bad d/T");
        WAE_REQUIRE(nopts >= 0 && (nopts == 0 || opts), "bad opts");
        const double sym_tol = nopts > 0 ? opts[0] : 0.0;
        WAE_REQUIRE(sym_tol >= 0.0 && sym_tol <= 1e-8, "opts[0] (symmetry tolerance) must lie in [0, 1e-8]");
        WAE_REQUIRE(index_bytes == 4 || index_bytes == 8, "index_bytes must be 4 or 8");
        WAE_REQUIRE(base == 0 || base == 1, "base must be 0 or 1");
        WAE_REQUIRE(d < 2147483647, "d too large for 32-bit indices");
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        WAE_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<wae_family> h(new wae_family);
        h->device = device;
        h->d = d;
        h->T = T;
        HIP_CHECK(hipStreamCreate(&h->stream));
        h->term_plane.resize(T);
        h->term_scale.resize(T);
        h->term_nnz.resize(T);
        const SetupEnv env;
        Lap lap{env.debug, "[create]", 34};
        std::vector<CsrZ> terms = convert_terms(d, T, index_bytes, base, orientation, ptr, idx, val);
        detect_planes(h.get(), terms);
        lap("terms to CSR, distinct planes");
        if (env.reorder) renumber_fine_level(h.get(), env);
        h->ops.resize(1);
        h->slot_plane.resize(1);
        lap.t = now_s();
        h->slot_plane[0] = build_levelop(h->ops[0], h->planes0, h->stream, sym_tol, env);
        lap("operator groups (CSR, both orientations)");
        if (!h->tile_row_ptr.empty()) {
            build_level_tiles(h->ops[0], h->planes0, h->slot_plane[0], h->tile_row_ptr, h->stream, env, 2, env.nbuf);
            lap("tile storage");
        }
        cplx one = {1.0, 0.0};
        h->one_dev.upload(&one, 1, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
        return WAE_OK;
    });
}

// ----------------------------------------------------------------------------------------------------
// wae_solver_setup
// ----------------------------------------------------------------------------------------------------
static void upload_transfer(Transfer &X, const AmgLevel &L, hipStream_t st) {
    X.nf = L.P.n; X.nc = L.P.m;
    X.p_ptr.upload(L.P.ptr.data(), L.P.ptr.size(), st);
    X.p_col.upload(L.P.col.data(), L.P.col.size(), st);
    X.p_val.upload(L.P.val.data(), L.P.val.size(), st);
    X.r_ptr.upload(L.R.ptr.data(), L.R.ptr.size(), st);
    X.r_col.upload(L.R.col.data(), L.R.col.size(), st);
    X.r_val.upload(L.R.val.data(), L.R.val.size(), st);
    HIP_CHECK(hipStreamSynchronize(st));
}
struct OwnStream {                              // a stream of the current device for the life of a helper thread's job
    hipStream_t s = nullptr;
    OwnStream() { HIP_CHECK(hipStreamCreate(&s)); }
    ~OwnStream() { (void)hipStreamDestroy(s); }
};

// Everything of level 1 -- tile plan, renumbering, operator groups, tile storage, the transfer operators of level 0 and the tile
// storage of the restriction -- needs only that level's planes and the first prolongator: run() works on a helper thread, with a
// stream of its own, while the host builds the deeper levels (round 3, second half: 0.7 s of work of which 0.15 s used to be
// hidden).  The level's operator is built into this object and moved into the handle once the number of levels is known.
struct Level1Work {
    std::vector<int> row_ptr, perm, iperm;      // tile plan of level 1 (empty: no tiles)
    int wmax = 0;
    std::vector<CsrZ> planes;                    // the level's planes in the new numbering (amg_setup still reads the old ones)
    LevelOp op;                                  // level-1 operator (groups + tiles)
    std::vector<int> slot_plane;
    Transfer xfer0;                              // P / R of level 0 (+ restriction tiles)
    bool built = false;
    double seconds = 0.0;

    // Level 1 renumbered into tiles as well (the numbering of a coarse level is nobody's business but the hierarchy's): P of level 0
    // changes its columns, R its rows; the transfer to level 2 the other way round (SolverSetup::adopt_level1, when it exists).
    void renumber(AmgLevel &L0, const TilePlan &plan) {
        perm = plan.perm; iperm = plan.iperm; row_ptr = plan.row_ptr;
        std::vector<std::future<void>> pj;
        planes.resize(L0.coarse_planes.size());
        for (size_t q = 0; q < L0.coarse_planes.size(); ++q)
            pj.push_back(std::async(std::launch::async, [this, &L0, q]() { planes[q] = permute_symmetric(L0.coarse_planes[q], perm, iperm); }));
        auto j1 = std::async(std::launch::async, [&]() { rename_cols(L0.P, iperm); });
        permute_rows(L0.R, perm);
        j1.get();
        for (auto &j : pj) j.get();
    }
    // L0: level 0 of the hierarchy under construction; it stays where it is (amg_setup reserves its levels) and nothing else touches
    // it until the thread has been joined
    void run(const wae_family *h, AmgLevel &L0, const SetupEnv &env) {
        const double tq0 = now_s();
        HIP_CHECK(hipSetDevice(h->device));
        const OwnStream s3;
        Lap lap{env.debug, "[setup]   (level-1 thread)", 22};
        const TilePlan plan = plan_tiles(union_pattern(L0.coarse_planes), 128, TILE_WCAP_COARSE, TILE_THICK);
        wmax = plan.wmax;
        lap("tile plan");
        if (!plan.perm.empty()) renumber(L0, plan);
        lap("permutation");
        // the transfer operators and the restriction's tile storage beside the operator (a thread and a stream of their own)
        const bool with_tiles = !row_ptr.empty();
        auto xj = std::async(std::launch::async, [&, h, with_tiles]() {
            HIP_CHECK(hipSetDevice(h->device));
            const OwnStream s2;
            upload_transfer(xfer0, L0, s2.s);
            if (with_tiles && env.tile_restrict) build_restriction_tiles(xfer0, L0.R, TILE_WCAP_COARSE, s2.s, env.debug);
            if (!h->tile_row_ptr.empty() && env.xfer_tiles) build_transfer_tiles(xfer0, L0.P, h->tile_row_ptr, s2.s);
        });
        const std::vector<CsrZ> &pl1 = planes.empty() ? L0.coarse_planes : planes;
        slot_plane = build_levelop(op, pl1, s3.s, WAE_LEVEL_SYM_TOL, env);
        lap("operator groups");
        if (with_tiles) build_level_tiles(op, pl1, slot_plane, row_ptr, s3.s, env, 4);
        HIP_CHECK(hipStreamSynchronize(s3.s));
        lap("tile storage");
        xj.get();
        lap("wait for the transfer");
        built = true;
        seconds = now_s() - tq0;
    }
};

// rows `rows` of A; an entry of column c goes to column col_of(c), or is dropped where that is negative
template <class ColMap> static CsrZ extract_rows(const CsrZ &A, const std::vector<int> &rows, int64_t m, ColMap &&col_of) {
    CsrZ B;
    B.n = (int64_t)rows.size();
    B.m = m;
    B.ptr.assign(rows.size() + 1, 0);
    for (size_t i = 0; i < rows.size(); ++i) {
        for (int pp = A.ptr[rows[i]]; pp < A.ptr[rows[i] + 1]; ++pp)
            if (col_of(A.col[pp]) >= 0) { B.col.push_back(col_of(A.col[pp])); B.val.push_back(A.val[pp]); }
        B.ptr[i + 1] = (int)B.col.size();
    }
    return B;
}

// ----------------------------------------------------------------------------------------------------
// wae_solver_setup_nested: the caller's prolongators
// ----------------------------------------------------------------------------------------------------
// checked copies of the caller's CSR prolongators (finest first); every complaint is a WaeError(WAE_ERR_INVALID) and nothing of the
// handle has been touched when it is raised
static std::vector<CsrD> read_prolongators(int64_t d, int32_t nlev, const int64_t *rows, const int64_t *cols, const int32_t *const *ptr,
                                           const int32_t *const *col, const double *const *val) {
    WAE_REQUIRE(nlev >= 1, "nested set-up: nlev must be at least 1");
    WAE_REQUIRE(rows && cols && ptr && col && val, "nested set-up: a null array");
    std::vector<CsrD> Ps((size_t)nlev);
    for (int32_t k = 0; k < nlev; ++k) {
        const std::string at = " (prolongator " + std::to_string(k) + ")";
        WAE_REQUIRE(ptr[k] && col[k] && val[k], "nested set-up: a null array" + at);
        if (k == 0) WAE_REQUIRE(rows[0] == d, "nested set-up: prolongator 0 has " + std::to_string(rows[0]) + " rows, the family has " + std::to_string(d) + " unknowns");
        else WAE_REQUIRE(rows[k] == cols[k - 1], "nested set-up: the dimensions do not chain: " + std::to_string(rows[k]) + " rows after " + std::to_string(cols[k - 1]) + " columns" + at);
        WAE_REQUIRE(cols[k] >= 1 && cols[k] < 2147483647 && rows[k] >= 1, "nested set-up: bad dimensions" + at);
        CsrD &P = Ps[(size_t)k];
        P.n = rows[k]; P.m = cols[k];
        const int32_t *pp = ptr[k];
        WAE_REQUIRE(pp[0] == 0, "nested set-up: the row pointer does not start at 0" + at);
        for (int64_t i = 0; i < P.n; ++i) WAE_REQUIRE(pp[i] <= pp[i + 1], "nested set-up: the row pointer is not monotone" + at);
        const int64_t nnz = pp[P.n];
        P.ptr.assign(pp, pp + P.n + 1);
        P.col.assign(col[k], col[k] + nnz);
        P.val.assign(val[k], val[k] + nnz);
        for (int64_t i = 0; i < P.n; ++i)
            for (int e = P.ptr[i]; e < P.ptr[i + 1]; ++e) {
                WAE_REQUIRE(P.col[e] >= 0 && P.col[e] < P.m, "nested set-up: a column out of range" + at);
                WAE_REQUIRE(e == P.ptr[i] || P.col[e - 1] < P.col[e], "nested set-up: unsorted or duplicate columns in a row" + at);
                WAE_REQUIRE(std::isfinite(P.val[e]), "nested set-up: a value that is not finite" + at);
            }
    }
    return Ps;
}
// row i of the result is row src[i] of P (empty where src[i] < 0); the columns no row uses are dropped and the others renumbered in
// their order: kept[c'] = the old number of column c'
static CsrD take_rows_drop_columns(const CsrD &P, const std::vector<int> &src, std::vector<int> &kept) {
    CsrD B;
    B.n = (int64_t)src.size();
    B.ptr.assign(src.size() + 1, 0);
    std::vector<int> newcol((size_t)P.m, -1);
    for (size_t i = 0; i < src.size(); ++i) {
        if (src[i] >= 0)
            for (int e = P.ptr[src[i]]; e < P.ptr[src[i] + 1]; ++e) { B.col.push_back(P.col[e]); B.val.push_back(P.val[e]); newcol[(size_t)P.col[e]] = 0; }
        B.ptr[i + 1] = (int)B.col.size();
    }
    kept.clear();
    for (int64_t c = 0; c < P.m; ++c)
        if (newcol[(size_t)c] == 0) { newcol[(size_t)c] = (int)kept.size(); kept.push_back((int)c); }
    B.m = (int64_t)kept.size();
    for (int &c : B.col) c = newcol[(size_t)c];             // (monotone: the rows stay sorted)
    return B;
}

// A helper thread that is waited for when this goes out of scope, also on an exception
struct Joined {
    std::future<void> f;
    void get() { if (f.valid()) f.get(); }      // (rethrows what the thread threw)
    ~Joined() { if (f.valid()) f.wait(); }
};

// ----------------------------------------------------------------------------------------------------
// opts[12] = 1: the spectral estimate behind a level's weight scale (include/waehip.h)
// ----------------------------------------------------------------------------------------------------
// The diagonal scaling of the power iteration on B = S Re(A) S, S = |D|^-1/2, D = Re(sum_q pc[q] diag[:, q]) (0 where D is 0).  The
// operator product needs x = S v and gives y = A x; v is real, so Re(y) = Re(A) x.
//     y == nullptr:  v_i = the start vector, ((i * 2654435761 mod 2^32) >> 16) / 32768 - 1  (in [-1, 1), exact in binary, the same on every call)
//     otherwise:     v_i = c s_i Re(y_i)           (c: the reciprocal of the previous norm, keeps the iterates of size one)
// and in both cases x_i = s_i v_i, imaginary parts 0.  One thread per row.
__global__ __launch_bounds__(256) void weight_scale_kernel(const cplx *__restrict__ diag, const cplx *__restrict__ pc, int nplanes, int64_t n,
                                                           const cplx *__restrict__ y, double c, cplx *__restrict__ v, cplx *__restrict__ x) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int q = 0; q < nplanes; ++q) {
        const cplx a = diag[(size_t)i * nplanes + q], w = pc[q];
        d += a.x * w.x - a.y * w.y;
    }
    const double s = d != 0.0 ? 1.0 / sqrt(fabs(d)) : 0.0;
    const double vi = y ? c * (s * y[i].x) : (double)(((unsigned)i * 2654435761u) >> 16) / 32768.0 - 1.0;
    v[i] = cplx{vi, 0.0};
    x[i] = cplx{s * vi, 0.0};
}

// One call of wae_solver_setup: what its stages share, one member function per stage (run() is the table of contents).
// The two helper threads work on members of this object and of the handle: basis_job and l1_job are the LAST members, so they are
// destroyed -- joined -- first, before anything their threads use.
struct SolverSetup {
    wae_family *h;
    const double *coeffs_ref, *opts;
    int nopts;
    const SetupEnv env;
    AmgOptions ao;
    bool spectral = false;          // opts[12]: scale the Jacobi weights of every level by its own spectral estimate
    uint64_t excl = 0;              // opts[7]: bit k set = term k stays out of the shape matrix (strength graph, aggregation, prolongator smoothing)
    std::vector<zc> pc, pc_shape;   // plane coefficients of the reference operator / of the shape matrix (excl != 0)
    std::vector<AmgLevel> lv;
    std::vector<char> pen;          // penalty rows of the fine level
    Level1Work l1;
    std::vector<CsrD> supplied;     // wae_solver_setup_nested: the caller's prolongators, finest first (empty: smoothed aggregation)
    Lap lap{env.debug, "[setup]", 34, h->stream};
    double t_amg0 = 0.0, t_amg1 = 0.0;
    Joined basis_job, l1_job;

    double opt(int i, double dflt) const { return (opts && i < nopts && opts[i] > 0) ? opts[i] : dflt; }

    void read_options() {
        ao.theta = opt(0, 0.02);
        ao.max_coarse = (int64_t)opt(1, 128);
        h->jac_w = opt(2, 0.8);
        // Post-smoothing and light-cycle weights (round 4; measured at 1M unknowns, pass in seconds, pre / post / light): 0.8 / 0.8 / 0.8
        // 2.02; 0.8 / 0.9 / 0.8 1.93; 0.9 / 1.0 / 0.8 2.07 (better snapshot solves, worse projected ones); 0.8 / 0.9 / 0.65 1.88;
        // 0.8 / 0.9 / 0.5 1.84; 0.8 / 0.9 / 0.3 1.80.  The light cycle's ONE sweep wants a small weight: its job is only to keep the
        // coarse correction honest on the components the coarse level cannot see.  0.5 is the default (eigenpair residuals and rank
        // gap of the benchmark unchanged: 6.6e-9, 1.3e9).
        h->jac_w_post = opt(10, 0.9);
        h->jac_w_light = opt(11, 0.5);
        const double lw = (opts && nopts > 12) ? opts[12] : 0.0;
        WAE_REQUIRE(lw == 0.0 || lw == 1.0, "opts[12] (per-level weight scaling) must be 0 or 1");
        spectral = lw == 1.0;
        h->nsweeps = (int)opt(3, 1);
        h->restart = (int)opt(4, 30);
        ao.penalty_ratio = opt(5, 1e8);
        h->NB = (int)opt(6, 64);
        WAE_REQUIRE(h->NB >= 1 && h->NB <= 256, "batch width must be in 1..256");
        WAE_REQUIRE(h->restart >= 2 && h->restart <= 200, "restart must be in 2..200");
        excl = (uint64_t)opt(7, 0.0);
        plane_coeffs(h, coeffs_ref, WAE_OP_N, pc);
        if (excl) {
            std::vector<double> cs(coeffs_ref, coeffs_ref + (size_t)2 * h->T);
            for (int k = 0; k < h->T && k < 52; ++k)
                if (excl >> k & 1) cs[2 * k] = cs[2 * k + 1] = 0.0;
            plane_coeffs(h, cs.data(), WAE_OP_N, pc_shape);
        }
    }

    void drop_hierarchy() {                     // (every device buffer of a level frees itself)
        h->ops.resize(1);
        h->slot_plane.resize(1);
        h->xfer.clear();
    }

    // The Krylov basis -- (restart + 1) vectors of d x NB complex numbers, 42 GB at 1M unknowns -- takes the driver about a
    // second to map: it is requested now, on a helper thread, and is there when the host part of the set-up is done.
    // opts[8], opts[9] (hints): probe columns and snapshot capacity of the contour integrals to come -- their snapshot store
    // (5 GB at 1M unknowns x 8 columns x 40 snapshots) and the resident term products (20 GB) are then mapped here as well,
    // behind the host work, instead of in the first pass (0.4 s of its snapshot phase).
    void reserve_device_memory() {
        const size_t vec = (size_t)h->d * h->NB, need = vec * (size_t)(h->restart + 1);
        const size_t hint_l = (size_t)opt(8, 0.0), hint_s = (size_t)opt(9, 0.0);
        const size_t need_q = hint_l > 0 && hint_s > 0 && hint_l <= (size_t)h->NB ? (size_t)h->d * hint_l * hint_s : 0;
        const size_t need_w = need_q * (size_t)h->nplanes;
        h->rb.wait_w();
        if (h->V.n == need && h->rbQ.n >= need_q && h->rb.W.n >= need_w) return;
        basis_job.f = std::async(std::launch::async, [this, need, need_q, need_w]() {
            HIP_CHECK(hipSetDevice(h->device));
            if (h->V.n != need) h->V.alloc(need);
            // (the snapshot stores are written once here as well: the first kernels that touch freshly mapped device memory
            // ran slower -- 0.14 s over the first pass's snapshot phase on some boxes; behind the host work it costs nothing)
            const bool new_q = h->rbQ.n < need_q, new_w = h->rb.W.n < need_w;
            if (new_q) h->rbQ.alloc(need_q);
            if (new_w) h->rb.W.alloc(need_w);
            if (new_q && need_q) HIP_CHECK(hipMemset(h->rbQ.p, 0, need_q * sizeof(cplx)));
            if (new_w && need_w) HIP_CHECK(hipMemset(h->rb.W.p, 0, need_w * sizeof(cplx)));
            HIP_CHECK(hipDeviceSynchronize());
        });
    }

    // the host part: amg_setup, which hands level 1 to the helper thread as soon as that level's planes exist
    void coarsen() {
        // fine-level aggregation in the caller's node order (iperm[o] = internal index of the caller's node o)
        std::vector<int> visit0;
        if (!h->perm_h.empty()) { visit0.resize(h->perm_h.size()); for (size_t i = 0; i < h->perm_h.size(); ++i) visit0[h->perm_h[i]] = (int)i; }
        const bool want_plan = env.tile_level1 && !h->tile_row_ptr.empty();
        amg_setup(h->planes0, pc, ao, lv, &pen, excl ? &pc_shape : nullptr, visit0.empty() ? nullptr : &visit0, [&](const AmgLevel &L) {
            if (!want_plan || l1_job.f.valid() || &L != &lv[0]) return;
            l1_job.f = std::async(std::launch::async, [this]() { l1.run(h, lv[0], env); });
        });
        t_amg1 = now_s();
        if (!env.debug) return;
        fprintf(stderr, "[setup] amg_setup (host) %.3f s\n", t_amg1 - t_amg0);
        fprintf(stderr, "[setup] level 0: n=%lld nnz/plane:", (long long)h->planes0[0].n);
        for (const CsrZ &A : h->planes0) fprintf(stderr, " %lld", (long long)A.nnz());
        fprintf(stderr, "\n");
        for (size_t l = 0; l < lv.size(); ++l) {
            fprintf(stderr, "[setup] level %zu: n=%lld P nnz=%lld nnz/plane:", l + 1, (long long)lv[l].P.m, (long long)lv[l].P.col.size());
            for (const CsrZ &A : lv[l].coarse_planes) fprintf(stderr, " %lld", (long long)A.nnz());
            fprintf(stderr, "\n");
        }
    }

    // wae_solver_setup_nested: the same lv and pen from the caller's prolongators.  Penalty rows by amg_setup's rule (the diagonal of the
    // reference operator summed in plane order, as its shape-matrix pass sums it); their rows of the first prolongator are emptied, a
    // column nobody uses any more leaves its level and the rows of the next prolongator.  The coarse planes are formed on the device
    // (galerkin.hip), a level's result feeding the next product there; level 1 goes to the helper thread as in coarsen().
    void find_penalty_rows() {
        const int64_t n0 = h->d;
        std::vector<double> dabs((size_t)n0);
        host_ranges(n0, row_threads(n0), [&](int64_t lo, int64_t hi, int) {
            for (int64_t i = lo; i < hi; ++i) {
                zc dg = 0;
                for (size_t k = 0; k < h->planes0.size(); ++k) {
                    const CsrZ &A = h->planes0[k];
                    const int *b = A.col.data() + A.ptr[i], *e = A.col.data() + A.ptr[i + 1];
                    const int *f = std::lower_bound(b, e, (int)i);
                    if (f != e && *f == (int)i) dg += pc[k] * A.val[(size_t)(f - A.col.data())];
                }
                dabs[(size_t)i] = std::abs(dg);
            }
        });
        std::vector<double> tmp(dabs);
        std::nth_element(tmp.begin(), tmp.begin() + n0 / 2, tmp.end());
        const double med = tmp[(size_t)(n0 / 2)];
        pen.assign((size_t)n0, 0);
        for (int64_t i = 0; i < n0; ++i) pen[(size_t)i] = dabs[(size_t)i] > ao.penalty_ratio * med;
    }
    void coarsen_nested() {
        const size_t nlev = supplied.size();
        find_penalty_rows();
        lv.clear();
        lv.reserve(nlev + (size_t)ao.max_levels + 1);          // (the helper thread keeps a reference to lv[0])
        const bool want_plan = env.tile_level1 && !h->tile_row_ptr.empty();
        // rows of the first prolongator: the library's numbering of the fine level, penalty rows empty
        std::vector<int> src((size_t)h->d), kept;
        for (int64_t i = 0; i < h->d; ++i) src[(size_t)i] = pen[(size_t)i] ? -1 : (h->perm_h.empty() ? (int)i : h->perm_h[(size_t)i]);
        std::vector<DevPlane> cur, next;
        for (size_t l = 0; l < nlev; ++l) {
            AmgLevel L;
            L.P = take_rows_drop_columns(supplied[l], src, kept);
            supplied[l] = CsrD();                                 // (the caller's copy is not needed again)
            WAE_REQUIRE(L.P.m >= 1, "nested set-up: a supplied level is left without unknowns");
            src = kept;                                        // the next prolongator keeps the rows of the columns that are left
            L.R = csr_transpose(L.P);
            DevProlongator Pd;
            upload_prolongator(L.P, Pd);
            L.coarse_planes.resize((size_t)h->nplanes);
            next.clear();
            next.resize((size_t)h->nplanes);
            int64_t triplets = 0;
            for (int q = 0; q < h->nplanes; ++q) {
                if (l == 0) {                                  // a fine plane is in HBM only for its own product
                    DevPlane A;
                    upload_plane(h->planes0[(size_t)q], A);
                    triplets += galerkin_device(A, Pd, next[(size_t)q], L.coarse_planes[(size_t)q]);
                } else {
                    triplets += galerkin_device(cur[(size_t)q], Pd, next[(size_t)q], L.coarse_planes[(size_t)q]);
                    cur[(size_t)q] = DevPlane();
                }
            }
            cur.swap(next);
            if (env.debug) fprintf(stderr, "[setup] supplied level %zu: %lld -> %lld unknowns, %lld triplets\n", l + 1, (long long)L.P.n, (long long)L.P.m, (long long)triplets);
            lv.push_back(std::move(L));
            if (l == 0 && want_plan) l1_job.f = std::async(std::launch::async, [this]() { l1.run(h, lv[0], env); });
        }
        cur.clear();
        if (lv.back().P.m > ao.max_coarse) {                   // smoothed aggregation goes on from the last supplied level (no penalty rows there)
            AmgOptions ac = ao;
            ac.penalty_ratio = std::numeric_limits<double>::infinity();
            std::vector<AmgLevel> more;
            amg_setup(lv.back().coarse_planes, pc, ac, more, nullptr, excl ? &pc_shape : nullptr);
            for (AmgLevel &L : more) lv.push_back(std::move(L));
        }
        t_amg1 = now_s();
        if (!env.debug) return;
        fprintf(stderr, "[setup] nested levels (device products + continuation) %.3f s\n", t_amg1 - t_amg0);
        for (size_t l = 0; l < lv.size(); ++l) {
            fprintf(stderr, "[setup] level %zu%s: n=%lld P nnz=%lld nnz/plane:", l + 1, l < nlev ? " (supplied)" : "", (long long)lv[l].P.m, (long long)lv[l].P.col.size());
            for (const CsrZ &A : lv[l].coarse_planes) fprintf(stderr, " %lld", (long long)A.nnz());
            fprintf(stderr, "\n");
        }
    }

    void adopt_level1() {
        l1_job.get();
        if (!l1.planes.empty()) lv[0].coarse_planes = std::move(l1.planes);
        if (l1.built && !l1.perm.empty() && lv.size() >= 2) {              // the transfer to level 2 in the new numbering of level 1
            auto j3 = std::async(std::launch::async, [&]() { permute_rows(lv[1].P, l1.perm); });
            rename_cols(lv[1].R, l1.iperm);
            j3.get();
        }
        if (env.debug && l1.built)
            fprintf(stderr, "[setup] level 1 on the helper thread: plan + permutation + operator + tiles + transfer %.3f s (%zu tiles, largest window %d)\n",
                    l1.seconds, l1.row_ptr.empty() ? (size_t)0 : l1.row_ptr.size() - 1, l1.wmax);
    }

    // the penalty rows' own sub-block, plane by plane (compact numbering), and the same rows with ALL their columns (global numbering)
    void build_penalty_ops() {
        hipStream_t st = h->stream;
        std::vector<int> rows, loc(pen.size(), -1);
        for (size_t i = 0; i < pen.size(); ++i)
            if (pen[i]) { loc[i] = (int)rows.size(); rows.push_back((int)i); }
        h->n_penalty = (int64_t)rows.size();
        if (rows.empty()) return;
        std::vector<CsrZ> block, full;
        for (const CsrZ &A : h->planes0) {
            block.push_back(extract_rows(A, rows, (int64_t)rows.size(), [&](int c) { return loc[c]; }));
            full.push_back(extract_rows(A, rows, A.m, [](int c) { return c; }));
        }
        h->pen_slot = build_levelop(h->pen_op, block, st, WAE_LEVEL_SYM_TOL, env);
        h->pen_row_slot = build_levelop(h->pen_row_op, full, st, WAE_LEVEL_SYM_TOL, env);
        h->pen_rows.upload(rows.data(), rows.size(), st);
        const size_t cnt = rows.size() * (size_t)h->NB;
        h->pen_b.alloc(cnt); h->pen_x.alloc(cnt); h->pen_t.alloc(cnt);
        HIP_CHECK(hipStreamSynchronize(st));
    }

    void upload_levels() {
        hipStream_t st = h->stream;
        h->ops.resize(lv.size() + 1);
        h->slot_plane.resize(lv.size() + 1);
        h->xfer.resize(lv.size());
        for (size_t l = 0; l < lv.size(); ++l) {
            if (l == 0 && l1.built) {
                h->slot_plane[1] = l1.slot_plane;
                // (a two-level hierarchy: level 1 is the dense one, its tiles are not used; not reached in practice: a tiled fine level
                // has a large level 1)
                if (lv.size() < 2) l1.op.tiles = TileStore();
                h->ops[1] = std::move(l1.op);
                h->xfer[0] = std::move(l1.xfer0);
                continue;
            }
            h->slot_plane[l + 1] = build_levelop(h->ops[l + 1], lv[l].coarse_planes, st, WAE_LEVEL_SYM_TOL, env);
            upload_transfer(h->xfer[l], lv[l], st);
            if (l == 0 && !h->tile_row_ptr.empty() && env.xfer_tiles) build_transfer_tiles(h->xfer[0], lv[0].P, h->tile_row_ptr, st);
        }
    }

    // dense planes of the coarsest level (plane order, row-major)
    void dense_coarsest() {
        const std::vector<CsrZ> &last = lv.empty() ? h->planes0 : lv.back().coarse_planes;
        h->nc = last[0].n;
        WAE_REQUIRE(h->nc <= 2048, "coarsest level too large for the dense solver (increase levels / lower max_coarse)");
        const size_t nn = (size_t)h->nc * h->nc;
        std::vector<cplx> dp(nn * h->nplanes, cplx{0.0, 0.0});
        const std::vector<int> &sp = h->slot_plane.back();
        for (int s = 0; s < h->nplanes; ++s) {
            const CsrZ &A = last[sp[s]];
            for (int64_t i = 0; i < A.n; ++i)
                for (int p = A.ptr[i]; p < A.ptr[i + 1]; ++p) dp[(size_t)s * nn + (size_t)i * h->nc + A.col[p]] = cplx{A.val[p].real(), A.val[p].imag()};
        }
        h->dense_planes.upload(dp.data(), dp.size(), h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->Ainv.alloc(nn * h->NB);
        h->dstatus.alloc(1);
    }

    void alloc_workspaces() {
        hipStream_t st = h->stream;
        const int NB = h->NB, m = h->restart;
        const int nl = (int)h->ops.size();
        h->lx.resize(nl); h->lb.resize(nl); h->lt.resize(nl);
        for (int l = 0; l < nl; ++l) {
            const size_t cnt = (size_t)h->ops[l].n * NB;
            h->lx[l].alloc(cnt); h->lb[l].alloc(cnt); h->lt[l].alloc(cnt);
        }
        const size_t vec = (size_t)h->d * NB;
        lap("level workspaces");
        basis_job.get();                                             // (rethrows an allocation failure)
        lap("wait for the Krylov basis");
        if (h->V.n != vec * (m + 1)) h->V.alloc(vec * (m + 1));
        h->W.alloc(vec); h->Xs.alloc(vec); h->Bs.alloc(vec); h->U.alloc(vec);
        // masked (converged) columns keep stale data: make sure "stale" is never an uninitialised NaN pattern
        HIP_CHECK(hipMemsetAsync(h->V.p, 0, vec * (m + 1) * sizeof(cplx), st));
        HIP_CHECK(hipMemsetAsync(h->W.p, 0, vec * sizeof(cplx), st));
        HIP_CHECK(hipMemsetAsync(h->U.p, 0, vec * sizeof(cplx), st));
        for (int l = 0; l < nl; ++l) {
            const size_t cnt = (size_t)h->ops[l].n * NB;
            HIP_CHECK(hipMemsetAsync(h->lx[l].p, 0, cnt * sizeof(cplx), st));
            HIP_CHECK(hipMemsetAsync(h->lb[l].p, 0, cnt * sizeof(cplx), st));
            HIP_CHECK(hipMemsetAsync(h->lt[l].p, 0, cnt * sizeof(cplx), st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        h->partial.alloc((size_t)1024 * 32 * NB);   // DOT_BLOCKS x 32 vectors x NB columns
        h->hdev.alloc((size_t)2 * (m + 3) * NB);     // second half: scratch for the re-orthogonalisation pass
        h->vsq.alloc((size_t)(m + 3) * NB);
        h->ydev.alloc((size_t)(m + 1) * NB);
        if (h->h_pinned) { (void)hipHostFree(h->h_pinned); h->h_pinned = nullptr; }
        HIP_CHECK(hipHostMalloc((void **)&h->h_pinned, (size_t)(m + 2) * NB * sizeof(cplx)));
    }

    // lambda_l and s_l of every level above the dense one (opts[12] = 1; otherwise 0 and exactly 1.0).  Runs on the level work spaces,
    // one column wide, and leaves them zero as alloc_workspaces left them.
    // Every step copies one norm back and waits for the stream: 40 round trips per level, which a normalisation on the device would
    // save.  Left so on purpose: it is set-up time (0.13 s for the whole set-up of the Hermite Rijke family), off by default, and the
    // host scalar keeps the kernel to one form.
    void level_weights() {
        const int nl = (int)h->ops.size();
        h->lvl_lambda.assign((size_t)nl, 0.0);
        h->lvl_scale.assign((size_t)nl, 1.0);
        if (!spectral) return;
        hipStream_t st = h->stream;
        DevBuf<cplx> pcd, nrm;
        nrm.alloc(1);
        std::vector<cplx> pcl((size_t)h->nplanes);
        auto norm_of = [&](const cplx *v, int64_t n) {
            launch_norms(v, n, 1, h->partial.p, nrm.p, st);
            cplx r{0.0, 0.0};
            HIP_CHECK(hipMemcpyAsync(&r, nrm.p, sizeof(cplx), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            return r.x;
        };
        for (int l = 0; l + 1 < nl; ++l) {
            const int64_t n = h->ops[l].n;
            if (n <= 0) continue;
            slot_coeffs(h, h->slot_plane[l], pc, pcl.data());
            pcd.upload(pcl.data(), pcl.size(), st);
            HIP_CHECK(hipStreamSynchronize(st));
            const OpDev A = h->ops[l].dev(WAE_OP_N);
            cplx *v = h->lt[l].p, *x = h->lx[l].p, *y = h->lb[l].p;
            const dim3 grid((unsigned)((n + 255) / 256));
            hipLaunchKernelGGL(weight_scale_kernel, grid, dim3(256), 0, st, h->ops[l].diag.p, pcd.p, h->nplanes, n, (const cplx *)nullptr, 1.0, v, x);
            HIP_CHECK(hipGetLastError());
            double prev = norm_of(v, n), lam = 0.0;
            for (int k = 0; k < WAE_WEIGHT_POWER_STEPS && prev > 0.0; ++k) {
                launch_spmv(A, pcd.p, 1, x, y, nullptr, 0.0, 1, MODE_AX, st);
                hipLaunchKernelGGL(weight_scale_kernel, grid, dim3(256), 0, st, h->ops[l].diag.p, pcd.p, h->nplanes, n, (const cplx *)y, 1.0 / prev, v, x);
                HIP_CHECK(hipGetLastError());
                lam = prev = norm_of(v, n);
            }
            WAE_REQUIRE(std::isfinite(lam) && lam > 0.0, "level weights: the spectral estimate of a level is not a positive number");
            h->lvl_lambda[(size_t)l] = lam;
            h->lvl_scale[(size_t)l] = std::min(1.0, 5.0 / (3.0 * 1.1 * lam));
            const size_t bytes = (size_t)n * sizeof(cplx);
            HIP_CHECK(hipMemsetAsync(v, 0, bytes, st));
            HIP_CHECK(hipMemsetAsync(x, 0, bytes, st));
            HIP_CHECK(hipMemsetAsync(y, 0, bytes, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        if (env.debug)
            for (int l = 0; l + 1 < nl; ++l) fprintf(stderr, "[setup] level %d: lambda %.6g, weight scale %.6g\n", l, h->lvl_lambda[(size_t)l], h->lvl_scale[(size_t)l]);
    }

    void run() {
        read_options();
        drop_hierarchy();
        t_amg0 = now_s();
        reserve_device_memory();
        if (supplied.empty()) coarsen();
        else {
            h->solver_ready = false;                           // (until the new hierarchy stands)
            coarsen_nested();
        }
        lap.t = now_s();
        adopt_level1();
        lap("wait for level 1 (helper thread)");
        build_penalty_ops();
        lap("penalty operators");
        upload_levels();
        lap("levels >= 2");
        dense_coarsest();
        lap("dense coarsest level");
        alloc_workspaces();
        level_weights();
        h->solver_ready = true;
        lap("other workspaces + memsets");
        if (env.debug) fprintf(stderr, "[setup] uploads + workspaces %.3f s\n", now_s() - t_amg1);
    }
};

extern "C" int wae_solver_setup(wae_family *h, const double *coeffs_ref, const double *opts, int32_t nopts) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs_ref, "bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        SolverSetup s{h, coeffs_ref, opts, nopts};
        s.run();
        return WAE_OK;
    });
}

extern "C" int wae_solver_setup_nested(wae_family *h, const double *coeffs_ref, const double *opts, int32_t nopts, int32_t nlev, const int64_t *rows,
                                       const int64_t *cols, const int32_t *const *ptr, const int32_t *const *col, const double *const *val) {
    return guarded([&]() {
        WAE_REQUIRE(h && coeffs_ref, "bad argument");
        std::vector<CsrD> Ps = read_prolongators(h->d, nlev, rows, cols, ptr, col, val);       // (before anything of the handle changes)
        HIP_CHECK(hipSetDevice(h->device));
        SolverSetup s{h, coeffs_ref, opts, nopts};
        s.supplied = std::move(Ps);
        s.run();
        return WAE_OK;
    });
}

extern "C" int wae_solver_level_weights(const wae_family *h, int32_t cap, double *lambda, double *scale, int32_t *nlev) {
    return guarded([&]() {
        WAE_REQUIRE(h && cap >= 0, "bad argument");
        require_solver(h);
        const int32_t nl = (int32_t)h->ops.size() - 1;
        if (nlev) *nlev = nl;
        for (int32_t l = 0; l < std::min(cap, nl); ++l) {
            if (lambda) lambda[l] = h->lvl_lambda[(size_t)l];
            if (scale) scale[l] = h->lvl_scale[(size_t)l];
        }
        return WAE_OK;
    });
}
