// lm_batch.hpp -- interface of lm_batch.hip: Levenberg-Marquardt for a batch of small independent bundle-adjustment
// components, one workgroup per component, the whole solve of a component on the device (rdis_hip_lm_batch).
//
// The host part is in this header and is pure: lm_batch_prepare turns the caller's component lists (already checked for
// independence by plan_index_build) into the per-component tables the kernel follows -- active camera / point blocks,
// the factors' local block indices, the factor lists per block, the camera pairs that share a point -- decides every
// component's class and lays out its workspace slice.  No HIP call, no context: everything that can be refused is
// refused here, before anything is launched or written.
//
// Components of 17 to 64 active camera blocks are the *wide* class (3), taken only where the caller opts in (RDIS_HIP_LM_WIDE
// in residual_model): their reduced system does not fit the LDS and lies in the component's workspace slice, in 16 x 16 tiles
// (LmWideTiles below: the one description host and device read).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LMB_HD __host__ __device__
#else
#define LMB_HD
#endif

namespace rdis_hip {

constexpr int LM_BATCH_MAX_CAMERAS = 16;   // include/rdis_hip.h: RDIS_HIP_LM_BATCH_MAX_CAMERAS
constexpr int LM_BATCH_WIDE_MAX_CAMERAS = 64;   // include/rdis_hip.h: RDIS_HIP_LM_WIDE_MAX_CAMERAS (with the option RDIS_HIP_LM_WIDE)
constexpr int LM_BATCH_EINVAL = -1, LM_BATCH_ERANGE = -5;   // include/rdis_hip.h's codes (lm_api.hip asserts them equal)

// ---- component classes: the workgroup and its dynamic LDS are a function of the component alone ---------------------------
// class 0: no active camera block (points only: no reduced system);  1: up to 6 camera blocks;  2: up to 16;
// 3 (wide, by option): 17 up to 64, the reduced system in the workspace slice.
constexpr int LM_BATCH_CLASSES = 4;
LMB_HD constexpr int lm_batch_class(int nca) { return nca == 0 ? 0 : nca <= 6 ? 1 : nca <= LM_BATCH_MAX_CAMERAS ? 2 : 3; }
LMB_HD constexpr int lm_batch_class_cameras(int cls) { return cls == 0 ? 0 : cls == 1 ? 6 : cls == 2 ? LM_BATCH_MAX_CAMERAS : LM_BATCH_WIDE_MAX_CAMERAS; }
LMB_HD constexpr int lm_batch_class_threads(int cls) { return cls == 0 ? 64 : cls == 1 ? 256 : 512; }
// LDS of a class, in doubles: reduction scratch [64] | U [81 C] | bc [9 C] | dc [9 C] | the reduced system's
// lower triangle, packed by rows, with the right-hand side as row M = 9 C: (M + 1)(M + 2) / 2
constexpr int LM_BATCH_LDS_HEAD = 64;
LMB_HD constexpr size_t lm_batch_lds_doubles(int maxc) {
    return maxc == 0 ? (size_t)LM_BATCH_LDS_HEAD
                     : (size_t)LM_BATCH_LDS_HEAD + 81 * (size_t)maxc + 18 * (size_t)maxc + (size_t)(9 * maxc + 1) * (size_t)(9 * maxc + 2) / 2;
}


// ---- the wide class's reduced system: S with the right-hand side as row M = 9 C, as the lower triangle of 16 x 16 tiles ----
// Tile (ti, tj), tj <= ti, is the ti (ti + 1) / 2 + tj-th run of 256 doubles, row-major inside.  nt = ceil((M + 1) / 16) tile
// rows hold rows 0 .. M; np = ceil(M / 16) column panels hold the columns that are factorised (0 .. M - 1).  Rows and
// columns beyond M inside the last tiles are padding: written as zero, never read into a result.  At 64 cameras: 37 tile
// rows, 703 tiles, 1 439 744 bytes.
constexpr int LM_WIDE_TILE = 16;
struct LmWideTiles {
    int M, nt, np;
    LMB_HD constexpr explicit LmWideTiles(int nca) : M(9 * nca), nt((9 * nca + 1 + LM_WIDE_TILE - 1) / LM_WIDE_TILE), np((9 * nca + LM_WIDE_TILE - 1) / LM_WIDE_TILE) {}
    LMB_HD constexpr long long doubles() const { return (long long)nt * (nt + 1) / 2 * (LM_WIDE_TILE * LM_WIDE_TILE); }
    LMB_HD constexpr long long tile(int ti, int tj) const { return ((long long)ti * (ti + 1) / 2 + tj) * (LM_WIDE_TILE * LM_WIDE_TILE); }   // tj <= ti
    LMB_HD constexpr long long at(int row, int col) const {   // col / 16 <= row / 16
        return tile(row / LM_WIDE_TILE, col / LM_WIDE_TILE) + (row % LM_WIDE_TILE) * LM_WIDE_TILE + col % LM_WIDE_TILE;
    }
};
// LDS of the wide class, in doubles: reduction scratch [64] | U [81 C] | bc [9 C] | dc [9 C] | one panel of 16 columns: the
// 16 nt rows of the tile rows (those above the panel's own tile row are not loaded), a row every LM_WIDE_PANEL_STRIDE doubles
// (17: lanes that read one column of sixteen rows hit sixteen different pairs of banks)
constexpr int LM_WIDE_PANEL_STRIDE = 17;
LMB_HD constexpr size_t lm_batch_wide_lds_doubles(int maxc) {
    return (size_t)LM_BATCH_LDS_HEAD + 81 * (size_t)maxc + 18 * (size_t)maxc + (size_t)LmWideTiles(maxc).nt * LM_WIDE_TILE * LM_WIDE_PANEL_STRIDE;
}
LMB_HD constexpr size_t lm_batch_class_lds_doubles(int cls) {
    return cls == 3 ? lm_batch_wide_lds_doubles(lm_batch_class_cameras(3)) : lm_batch_lds_doubles(lm_batch_class_cameras(cls));
}
static_assert(lm_batch_class_lds_doubles(3) * sizeof(double) <= 160 * 1024 && lm_batch_class_lds_doubles(2) * sizeof(double) <= 160 * 1024,
              "a class's LDS fits the 160 KiB of a compute unit");

// ---- a component's workspace slice in HBM (doubles; offsets from the slice's start) -------------------------------------------
// (S: the wide class's tiles, LmWideTiles(nca).doubles() of them, appended behind what every class has; total includes it)
struct LmBatchSlice { long long Jc, Jp, e, T, Zc, V, bp, Lp, yp, dp, psave, total, S; };
// nf listed factors with R residual rows each, nca / npa active camera / point blocks, nfree free variables
LMB_HD inline LmBatchSlice lm_batch_slice(long long nf, long long nca, long long npa, long long nfree, long long R) {
    LmBatchSlice s{};
    long long o = 0;
    auto take = [&o](long long n) { const long long at = o; o += (n + 1) / 2 * 2; return at; };   // (16-byte granules)
    s.Jc = take(nf * R * 9); s.Jp = take(nf * R * 3); s.e = take(nf * R); s.T = take(nf * R * 3);
    s.Zc = take(nca > 0 && npa > 0 ? nf * 27 : 0);
    s.V = take(npa * 6); s.bp = take(npa * 3); s.Lp = take(npa * 6); s.yp = take(npa * 3); s.dp = take(npa * 3);
    s.psave = take(nfree);
    s.S = o;
    if (lm_batch_class((int)nca) == 3) (void)take(LmWideTiles((int)nca).doubles());
    s.total = o;
    return s;
}

// what the kernel knows of a component: counts, where its int tables start (offsets from `ints0` into the batch's int
// block), where its workspace slice and its part of the free list start, and which output row is its
struct LmBatchComp {
    int nf, nca, npa, nfree, npair, cls;
    int o_lf, o_fci, o_fpi;             // [nf] listed factor id; local camera / point block of the factor (-1: constant)
    int o_cptr, o_clist;                // CSR: the listed factors of every active camera block, in listed order
    int o_pptr, o_plist;                // ... and of every active point block
    int o_fslot;                        // [nfree] the unknown a free variable is: >= 0 camera unknown 9 c + k; <= -2 point unknown -(s + 2) = 3 p + k; -1 none (no block: step 0)
    int o_pab, o_pairptr, o_pja, o_pjb; // camera pairs (a >= b) that share a point: [2 npair], CSR [npair + 1], (factor of a, factor of b) per entry in point order
    long long ints0, ws0, free0, comp;
};

struct LmBatchTables {
    std::vector<LmBatchComp> comps;          // in the caller's order
    std::vector<int> ints;                   // every component's int tables, one after the other
    std::vector<int> free32;                 // the free list as int32
    std::vector<unsigned char> freem;        // [N] free in some component
    std::vector<int> order[LM_BATCH_CLASSES];   // per class: its components, heaviest (most listed factors) first
    long long ws_doubles = 0;
};

// a problem's blocks: the camera / point block a variable belongs to as its factors define it (-1: no factor reads it);
// where the variables are laid out as ncams camera blocks of 9 followed by point blocks of 3 (what rdis_hip_lm_optimize
// requires), a variable no factor reads belongs to the layout's block, like there
struct LmBatchBlocks {
    int64_t N, F;
    const int *h_cam, *h_pt, *block_of, *ptblock_of;
    bool layout;
    int ncams;
};

// the key of a camera pair (a, b), b <= a: ordered as (a, b) whatever the class
constexpr int LM_BATCH_PAIR_STRIDE = LM_BATCH_WIDE_MAX_CAMERAS + 1;

// 0, or a code with *msg.  The lists have passed plan_index_build: ids in range, components independent.
// wide: components of 17 to LM_BATCH_WIDE_MAX_CAMERAS active camera blocks are taken (class 3) instead of refused.
inline int lm_batch_prepare(const LmBatchBlocks& B, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid,
                            const int64_t* fac_ptr, const int64_t* fac_id, int R, LmBatchTables& T, std::string* msg, bool wide = false) {
    auto refuse = [&](int code, std::string m) { *msg = std::move(m); return code; };
    const int64_t nfree_all = free_ptr[ncomp];
    T.comps.assign((size_t)ncomp, LmBatchComp{});
    T.ints.clear();
    T.free32.resize((size_t)nfree_all);
    T.freem.assign((size_t)std::max<int64_t>(B.N, 1), 0);
    for (auto& o : T.order) o.clear();
    T.ws_doubles = 0;
    for (int64_t i = 0; i < nfree_all; ++i) { T.free32[(size_t)i] = (int)free_vid[i]; T.freem[(size_t)free_vid[i]] = 1; }
    std::vector<int> loc((size_t)std::max<int64_t>(B.N, 1), -1);   // local index of the block that starts at a variable (this component's)
    // the block of a variable: (start, 9 or 3), or (-1, 0)
    auto block = [&](int v, int& len) {
        if (B.block_of[(size_t)v] >= 0) { len = 9; return B.block_of[(size_t)v]; }
        if (B.ptblock_of[(size_t)v] >= 0) { len = 3; return B.ptblock_of[(size_t)v]; }
        if (B.layout) {
            if (v < 9 * B.ncams) { len = 9; return v / 9 * 9; }
            const int q = 9 * B.ncams + (v - 9 * B.ncams) / 3 * 3;
            if ((int64_t)q + 3 <= B.N) { len = 3; return q; }
        }
        len = 0;
        return -1;
    };
    std::vector<int> cams, pts, lf, fci, fpi, cptr, clist, pptr, plist, fslot, pab, pairptr, pja, pjb, seen;
    struct PairEntry { int key, ja, jb; };
    std::vector<PairEntry> ents;
    for (int64_t cc = 0; cc < ncomp; ++cc) {
        const int64_t f0 = free_ptr[cc], nfr = free_ptr[cc + 1] - f0, j0 = fac_ptr[cc], nf = fac_ptr[cc + 1] - j0;
        cams.clear(); pts.clear();
        for (int64_t i = 0; i < nfr; ++i) {
            int len;
            const int b = block((int)free_vid[f0 + i], len);
            if (b >= 0 && loc[(size_t)b] == -1) { loc[(size_t)b] = -2; (len == 9 ? cams : pts).push_back(b); }
        }
        // active blocks in ascending id order, like rdis_hip_lm_optimize
        std::sort(cams.begin(), cams.end());
        std::sort(pts.begin(), pts.end());
        const int nca = (int)cams.size(), npa = (int)pts.size();
        auto unmark = [&]() { for (int b : cams) loc[(size_t)b] = -1; for (int b : pts) loc[(size_t)b] = -1; };
        if (nca > (wide ? LM_BATCH_WIDE_MAX_CAMERAS : LM_BATCH_MAX_CAMERAS)) {
            unmark();
            return refuse(LM_BATCH_ERANGE, "lm_batch: component " + std::to_string(cc) + " has " + std::to_string(nca) +
                                               " active camera blocks, the limit is " + std::to_string(wide ? LM_BATCH_WIDE_MAX_CAMERAS : LM_BATCH_MAX_CAMERAS) +
                                               (wide ? " (RDIS_HIP_LM_WIDE_MAX_CAMERAS, with RDIS_HIP_LM_WIDE)" : " (RDIS_HIP_LM_BATCH_MAX_CAMERAS)") +
                                               ": solve it with rdis_hip_lm_optimize");
        }
        for (int c = 0; c < nca; ++c) loc[(size_t)cams[(size_t)c]] = c;
        for (int p = 0; p < npa; ++p) loc[(size_t)pts[(size_t)p]] = p;
        fslot.assign((size_t)nfr, -1);
        for (int64_t i = 0; i < nfr; ++i) {
            int len;
            const int v = (int)free_vid[f0 + i], b = block(v, len);
            if (b >= 0) fslot[(size_t)i] = len == 9 ? 9 * loc[(size_t)b] + (v - b) : -(3 * loc[(size_t)b] + (v - b)) - 2;
        }
        lf.resize((size_t)nf); fci.assign((size_t)nf, -1); fpi.assign((size_t)nf, -1);
        cptr.assign((size_t)nca + 1, 0); pptr.assign((size_t)npa + 1, 0);
        for (int64_t j = 0; j < nf; ++j) {
            const int f = (int)fac_id[j0 + j];
            lf[(size_t)j] = f;
            // (a camera block start is no point block start: loc of a factor's camera is a camera index or -1)
            fci[(size_t)j] = loc[(size_t)B.h_cam[(size_t)f]];
            fpi[(size_t)j] = loc[(size_t)B.h_pt[(size_t)f]];
            if (fci[(size_t)j] >= 0) ++cptr[(size_t)fci[(size_t)j] + 1];
            if (fpi[(size_t)j] >= 0) ++pptr[(size_t)fpi[(size_t)j] + 1];
        }
        unmark();
        for (int c = 0; c < nca; ++c) cptr[(size_t)c + 1] += cptr[(size_t)c];
        for (int p = 0; p < npa; ++p) pptr[(size_t)p + 1] += pptr[(size_t)p];
        clist.resize((size_t)cptr[(size_t)nca]); plist.resize((size_t)pptr[(size_t)npa]);
        {
            std::vector<int> ccur(cptr.begin(), cptr.end() - 1), pcur(pptr.begin(), pptr.end() - 1);
            for (int64_t j = 0; j < nf; ++j) {   // listed order = summation order
                if (fci[(size_t)j] >= 0) clist[(size_t)ccur[(size_t)fci[(size_t)j]]++] = (int)j;
                if (fpi[(size_t)j] >= 0) plist[(size_t)pcur[(size_t)fpi[(size_t)j]]++] = (int)j;
            }
        }
        // two factors joining the same camera and point would need their Z blocks added: refused, like rdis_hip_lm_optimize
        seen.assign((size_t)std::max(nca, 1), -1);
        for (int p = 0; p < npa; ++p)
            for (int t = pptr[(size_t)p]; t < pptr[(size_t)p + 1]; ++t) {
                const int ci = fci[(size_t)plist[(size_t)t]];
                if (ci < 0) continue;
                if (seen[(size_t)ci] == p)
                    return refuse(LM_BATCH_EINVAL, "lm_batch: two listed factors of component " + std::to_string(cc) + " join the same camera and point");
                seen[(size_t)ci] = p;
            }
        // the camera pairs (a >= b) that share a point with their (factor of a, factor of b) entries; within a pair the
        // entries keep their point order: the order of the sums
        pab.clear(); pja.clear(); pjb.clear(); pairptr.assign(1, 0); ents.clear();
        for (int p = 0; p < npa && nca > 0; ++p) {
            const int t0 = pptr[(size_t)p], t1 = pptr[(size_t)p + 1];
            for (int t = t0; t < t1; ++t) {
                const int ja = plist[(size_t)t], a = fci[(size_t)ja];
                if (a < 0) continue;
                for (int u = t0; u < t1; ++u) {
                    const int jb = plist[(size_t)u], b = fci[(size_t)jb];
                    if (b < 0 || b > a) continue;
                    ents.push_back({a * LM_BATCH_PAIR_STRIDE + b, ja, jb});
                }
            }
        }
        std::stable_sort(ents.begin(), ents.end(), [](const PairEntry& x, const PairEntry& y) { return x.key < y.key; });
        for (size_t i = 0; i < ents.size(); ++i) {
            if (i == 0 || ents[i].key != ents[i - 1].key) {
                if (i > 0) pairptr.push_back((int)i);
                pab.push_back(ents[i].key / LM_BATCH_PAIR_STRIDE); pab.push_back(ents[i].key % LM_BATCH_PAIR_STRIDE);
            }
            pja.push_back(ents[i].ja); pjb.push_back(ents[i].jb);
        }
        if (!ents.empty()) pairptr.push_back((int)ents.size());

        LmBatchComp& D = T.comps[(size_t)cc];
        D.nf = (int)nf; D.nca = nca; D.npa = npa; D.nfree = (int)nfr; D.npair = (int)pairptr.size() - 1; D.cls = lm_batch_class(nca);
        D.ints0 = (long long)T.ints.size(); D.free0 = f0; D.comp = cc;
        auto put = [&](const std::vector<int>& v) { const int off = (int)((long long)T.ints.size() - D.ints0); T.ints.insert(T.ints.end(), v.begin(), v.end()); return off; };
        D.o_lf = put(lf); D.o_fci = put(fci); D.o_fpi = put(fpi); D.o_cptr = put(cptr); D.o_clist = put(clist);
        D.o_pptr = put(pptr); D.o_plist = put(plist); D.o_fslot = put(fslot);
        D.o_pab = put(pab); D.o_pairptr = put(pairptr); D.o_pja = put(pja); D.o_pjb = put(pjb);
        D.ws0 = T.ws_doubles;
        T.ws_doubles += lm_batch_slice(nf, nca, npa, nfr, R).total;
        T.order[D.cls].push_back((int)cc);
    }
    for (auto& o : T.order)
        std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return T.comps[(size_t)a].nf > T.comps[(size_t)b].nf; });
    return 0;
}

// where the tables lie in one device block, uploaded in one copy: comps | ints | free32 | order (class 0, 1, 2, 3) | freem,
// each part on a 256-byte boundary; `bytes` is the block's size.  Nothing in it depends on x.
struct LmBatchTableLayout { size_t comps, ints, free32, order, freem, bytes; };
inline LmBatchTableLayout lm_batch_table_layout(const LmBatchTables& T) {
    size_t norder = 0;
    for (const auto& o : T.order) norder += o.size();
    LmBatchTableLayout L{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t off = at; at += (std::max<size_t>(bytes, 8) + 255) / 256 * 256; return off; };
    L.comps = take(T.comps.size() * sizeof(LmBatchComp)); L.ints = take(T.ints.size() * 4); L.free32 = take(T.free32.size() * 4);
    L.order = take(norder * 4); L.freem = take(T.freem.size());
    L.bytes = at;
    return L;
}
// the block's host image: stage[L.bytes], zero where no table lies
inline void lm_batch_stage_tables(const LmBatchTables& T, const LmBatchTableLayout& L, char* stage) {
    std::fill(stage, stage + L.bytes, (char)0);
    auto put = [stage](size_t off, const void* src, size_t bytes) { if (bytes) std::copy_n(static_cast<const char*>(src), bytes, stage + off); };
    put(L.comps, T.comps.data(), T.comps.size() * sizeof(LmBatchComp));
    put(L.ints, T.ints.data(), T.ints.size() * 4);
    put(L.free32, T.free32.data(), T.free32.size() * 4);
    size_t at = L.order;
    for (const auto& o : T.order) { put(at, o.data(), o.size() * 4); at += o.size() * 4; }
    put(L.freem, T.freem.data(), T.freem.size());
}

// a component's row of results: fret, finit, iterations, stop code, residual evaluations, Jacobian evaluations, linear solves,
// final mu, active camera blocks, active point blocks, history records (also those beyond the caller's capacity), unused
constexpr int LM_BATCH_RES = 12;
constexpr int LM_BATCH_RES_NHIST = 10;   // where in the row the history's record count stands

#if defined(__HIPCC__)
struct LmBatchProblem {     // device arrays of an uploaded bundle-adjustment problem
    double* x;
    const double *lo, *hi;
    const int *cam, *pt;    // first variable id of each factor's camera / point block
    const double2* obs;
};
struct LmBatchOptions {
    int maxiters, model;                // SSmaxit; residual rows per factor (1 or 2)
    double tau, eps1, eps2, eps3;       // levmar opts[0..3] (reference: 1e-3, 1e-15, 1e-15, SSftol)
};
// the batch's device block, kept by the caller between calls (grown on demand)
struct LmBatchWorkspace {
    void* dev = nullptr;
    size_t dev_bytes = 0;
    LmBatchWorkspace() = default;
    LmBatchWorkspace(const LmBatchWorkspace&) = delete;
    LmBatchWorkspace& operator=(const LmBatchWorkspace&) = delete;
    ~LmBatchWorkspace();
};
// The members of one launch (the member is the grid's second dimension): member m solves every component from, and into,
// P.x + m x_stride, in the workspace replica ws + m ws_stride, and leaves its rows at res + m res_stride ([ncomp][LM_BATCH_RES])
// and hist + m hist_stride ([ncomp][hist_cap][4]; unused when hist_cap is 0).  Strides in doubles.  lo, hi, the factor
// arrays and the tables are shared.  A member's bits depend neither on `count` nor on its place among the members.
// xout + m xout_stride ([nfree], the free list's order) receives the member's clamped results beside x itself: a plan keeps
// them for its fetch.  xout null: rdis_hip_lm_batch's launch -- one member (count 1), the strides unused, and the kernel's
// instantiation without member terms; the bits are the same.
struct LmBatchMembers {
    long long x_stride;
    double* res; long long res_stride;
    double* hist; long long hist_stride;
    double* ws; long long ws_stride;
    double* xout; long long xout_stride;
    int count;
};
// Enqueues the solve of every component of an uploaded table block (lm_batch_table_layout; n: the components of each class)
// for M.count members: one launch per class that occurs (at most four), heaviest class first.  No copy, no wait, no allocation.
// Returns 0 or a hipError_t.
int lm_batch_launch(hipStream_t stream, const LmBatchProblem& P, const void* tables, const LmBatchTableLayout& lay, const int (&n)[LM_BATCH_CLASSES],
                    const LmBatchOptions& opt, int64_t hist_cap, const LmBatchMembers& M);
// Solves every component of T (lm_batch_prepare) from the currently assigned x, which is updated in place: the free
// variables end at the clamped results.  res: [ncomp][LM_BATCH_RES]; hist: [ncomp][hist_cap][4] (hist_cap 0: none).
// One upload, one launch per class that occurs, the downloads, one wait.  Returns 0 or a hipError_t.
int device_lm_batch(hipStream_t stream, const LmBatchProblem& P, const LmBatchTables& T, const LmBatchOptions& opt,
                    int64_t hist_cap, LmBatchWorkspace* ws, std::vector<double>* res, std::vector<double>* hist);
#endif

}  // namespace rdis_hip
