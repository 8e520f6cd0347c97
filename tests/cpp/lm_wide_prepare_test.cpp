// The host half of the wide class (rdis_amd/csrc/lm_batch.hpp, class 3: 17 to 64 active camera blocks, by option) without a
// device: the class's limits, the tiles of the reduced system appended to the workspace slice, the LDS bound, the tables and
// order of a 17- and a 64-camera component written out by hand, the refusals, and that the option changes nothing for a
// component of at most 16 cameras.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rdis_amd/csrc/lm_batch.hpp"

using namespace rdis_hip;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } \
    } while (0)

struct Problem {   // cameras first (ncams blocks of 9), then points; factors (camera index, point index)
    int ncams, npts;
    std::vector<int> cam, pt, block_of, ptblock_of;
    Problem(int nc, int np, const std::vector<std::pair<int, int>>& fac) : ncams(nc), npts(np) {
        const int N = 9 * nc + 3 * np;
        block_of.assign((size_t)N, -1); ptblock_of.assign((size_t)N, -1);
        for (const auto& f : fac) {
            cam.push_back(9 * f.first); pt.push_back(9 * nc + 3 * f.second);
            for (int k = 0; k < 9; ++k) block_of[(size_t)(9 * f.first + k)] = 9 * f.first;
            for (int k = 0; k < 3; ++k) ptblock_of[(size_t)(9 * nc + 3 * f.second + k)] = 9 * nc + 3 * f.second;
        }
    }
    LmBatchBlocks blocks() const {
        return LmBatchBlocks{9 * ncams + 3 * npts, (int64_t)cam.size(), cam.data(), pt.data(), block_of.data(), ptblock_of.data(), true, ncams};
    }
};

struct Lists {
    std::vector<int64_t> free_ptr{0}, free_vid, fac_ptr{0}, fac_id;
    void add(const std::vector<int64_t>& fr, const std::vector<int64_t>& fc) {
        free_vid.insert(free_vid.end(), fr.begin(), fr.end()); fac_id.insert(fac_id.end(), fc.begin(), fc.end());
        free_ptr.push_back((int64_t)free_vid.size()); fac_ptr.push_back((int64_t)fac_id.size());
    }
    int prepare(const LmBatchBlocks& B, int R, LmBatchTables& T, std::string* msg, bool wide) const {
        return lm_batch_prepare(B, (int64_t)free_ptr.size() - 1, free_ptr.data(), free_vid.data(), fac_ptr.data(), fac_id.data(), R, T, msg, wide);
    }
    int prepare9(const LmBatchBlocks& B, int R, LmBatchTables& T, std::string* msg) const {   // the call as it was before the option
        return lm_batch_prepare(B, (int64_t)free_ptr.size() - 1, free_ptr.data(), free_vid.data(), fac_ptr.data(), fac_id.data(), R, T, msg);
    }
};

static std::vector<int64_t> range(int64_t a, int64_t b) { std::vector<int64_t> v; for (int64_t i = a; i < b; ++i) v.push_back(i); return v; }
static std::vector<int> table(const LmBatchTables& T, const LmBatchComp& C, int off, int n) {
    return std::vector<int>(T.ints.begin() + C.ints0 + off, T.ints.begin() + C.ints0 + off + n);
}

// a chain: camera c sees points c and c + 1 (factors 2 c, 2 c + 1): neighbours share a point, no others do
static Problem chain(int nc) {
    std::vector<std::pair<int, int>> fac;
    for (int c = 0; c < nc; ++c) { fac.push_back({c, c}); fac.push_back({c, c + 1}); }
    return Problem(nc, nc + 1, fac);
}

int main() {
    // ---- the class: 17 .. 64 cameras, 512 lanes; classes 0 - 2 where they were ----
    CHECK(LM_BATCH_CLASSES == 4 && LM_BATCH_MAX_CAMERAS == 16 && LM_BATCH_WIDE_MAX_CAMERAS == 64);
    CHECK(lm_batch_class(0) == 0 && lm_batch_class(6) == 1 && lm_batch_class(7) == 2 && lm_batch_class(16) == 2);
    CHECK(lm_batch_class(17) == 3 && lm_batch_class(64) == 3);
    CHECK(lm_batch_class_cameras(2) == 16 && lm_batch_class_cameras(3) == 64 && lm_batch_class_threads(3) == 512);
    for (int nca = 0; nca <= LM_BATCH_WIDE_MAX_CAMERAS; ++nca) CHECK(nca <= lm_batch_class_cameras(lm_batch_class(nca)));
    // ---- the tiles: rows 0 .. M in nt tile rows, columns 0 .. M - 1 in np panels ----
    {
        const LmWideTiles a(17), b(64), c(49);
        CHECK(a.M == 153 && a.nt == 10 && a.np == 10);                // the rhs row shares the partial last tile row
        CHECK(b.M == 576 && b.nt == 37 && b.np == 36);                // ... opens a tile row of its own
        CHECK(c.M == 441 && c.nt == 28 && c.np == 28);
        CHECK(a.doubles() == 55 * 256 && b.doubles() == 703 * 256 && b.doubles() * 8 <= 1500 * 1024);
        // every entry of the lower triangle and of row M has a place of its own inside the tiles
        for (const LmWideTiles& g : {a, b}) {
            std::vector<char> used((size_t)g.doubles(), 0);
            for (int row = 0; row <= g.M; ++row)
                for (int col = 0; col <= row && col < g.M; ++col) {
                    const long long at = g.at(row, col);
                    CHECK(at >= 0 && at < g.doubles() && !used[(size_t)at]);
                    used[(size_t)at] = 1;
                }
            CHECK(g.at(0, 0) == 0 && g.at(16, 0) == 256 && g.at(16, 16) == 512 && g.at(17, 18) == 512 + 16 + 2);
            CHECK(g.tile(g.nt - 1, g.nt - 1) + 256 == g.doubles());
        }
    }
    // ---- the LDS: classes 0 - 2 as they were; the wide class: head, U, bc, dc and one panel, inside 160 KiB ----
    CHECK(lm_batch_class_lds_doubles(0) == lm_batch_lds_doubles(0) && lm_batch_class_lds_doubles(1) == lm_batch_lds_doubles(6));
    CHECK(lm_batch_class_lds_doubles(2) == lm_batch_lds_doubles(16) && lm_batch_lds_doubles(16) == 64 + 1296 + 288 + 145 * 146 / 2);
    CHECK(lm_batch_wide_lds_doubles(64) == 64 + 5184 + 1152 + 37 * 16 * LM_WIDE_PANEL_STRIDE && lm_batch_class_lds_doubles(3) == lm_batch_wide_lds_doubles(64));
    CHECK(LM_WIDE_PANEL_STRIDE >= LM_WIDE_TILE && lm_batch_class_lds_doubles(3) * 8 <= 160 * 1024);
    {   // ---- the slice: classes 0 - 2 end where they ended; the wide class appends S behind, aligned, overlapping nothing ----
        for (int nca : {0, 2, 16}) {
            const LmBatchSlice s = lm_batch_slice(7, nca, 3, 27, 2);
            CHECK(s.S == s.total && s.total == s.psave + 28);
        }
        CHECK(lm_batch_slice(7, 2, 3, 27, 2).total == 126 + 42 + 14 + 42 + 190 + 18 + 10 + 18 + 10 + 10 + 28);
        const LmBatchSlice n = lm_batch_slice(40, 16, 20, 204, 2), w = lm_batch_slice(40, 17, 20, 204, 2);
        CHECK(w.Jc == n.Jc && w.Zc == n.Zc && w.psave == n.psave && w.S == n.total && w.S >= w.psave + 204 && w.S % 2 == 0);
        CHECK(w.total == w.S + LmWideTiles(17).doubles());
        CHECK(lm_batch_slice(40, 64, 20, 636, 1).total - lm_batch_slice(40, 64, 20, 636, 1).S == 703 * 256);
    }
    std::string msg;
    {   // ---- 17 cameras in a chain: class 3 with the option, its tables and pair order; refused without, by today's text ----
        const Problem A = chain(17);
        Lists L; L.add(range(0, 9 * 17 + 3 * 18), range(0, 34));
        LmBatchTables T;
        CHECK(L.prepare(A.blocks(), 2, T, &msg, true) == 0);
        const LmBatchComp& C = T.comps[0];
        CHECK(C.nf == 34 && C.nca == 17 && C.npa == 18 && C.nfree == 207 && C.cls == 3 && C.npair == 17 + 16);
        CHECK(T.order[3] == std::vector<int>{0} && T.order[0].empty() && T.order[1].empty() && T.order[2].empty());
        CHECK(T.ws_doubles == lm_batch_slice(34, 17, 18, 207, 2).total && T.ws_doubles >= 55 * 256);
        const std::vector<int> pab = table(T, C, C.o_pab, 2 * C.npair), pp = table(T, C, C.o_pairptr, C.npair + 1);
        const std::vector<int> pja = table(T, C, C.o_pja, pp.back()), pjb = table(T, C, C.o_pjb, pp.back());
        // pairs in (a, b) order: (0,0) (1,0) (1,1) (2,1) (2,2) ...; a camera with itself over its two points, neighbours over one
        CHECK(pab[0] == 0 && pab[1] == 0 && pp[1] == 2 && pja[0] == 0 && pja[1] == 1);
        for (int a = 1; a < 17; ++a) {
            const int q = 2 * a - 1;
            CHECK(pab[2 * q] == a && pab[2 * q + 1] == a - 1 && pp[q + 1] - pp[q] == 1);
            CHECK(pja[pp[q]] == 2 * a && pjb[pp[q]] == 2 * (a - 1) + 1);            // they share point a
            CHECK(pab[2 * q + 2] == a && pab[2 * q + 3] == a && pp[q + 2] - pp[q + 1] == 2);
            CHECK(pja[pp[q + 1]] == 2 * a && pja[pp[q + 1] + 1] == 2 * a + 1 && pjb[pp[q + 1]] == 2 * a);
        }
        const std::vector<int> fs = table(T, C, C.o_fslot, 207);
        CHECK(fs[0] == 0 && fs[152] == 152 && fs[153] == -2 && fs[206] == -(3 * 17 + 2) - 2);
        CHECK(L.prepare9(A.blocks(), 2, T, &msg) == LM_BATCH_ERANGE);
        CHECK(msg == "lm_batch: component 0 has 17 active camera blocks, the limit is 16 (RDIS_HIP_LM_BATCH_MAX_CAMERAS): solve it with rdis_hip_lm_optimize");
        CHECK(L.prepare(A.blocks(), 2, T, &msg, false) == LM_BATCH_ERANGE && msg.find("limit is 16") != std::string::npos);
    }
    {   // ---- 64 cameras pass with the option, heaviest first within the class; 65 are refused before anything, by name ----
        const Problem B = chain(65);
        Lists L; L.add(range(0, 9 * 20), range(0, 40)); L.add(range(9 * 20, 9 * 64), range(40, 128)); L.add(range(9 * 65, 9 * 65 + 3), {});
        LmBatchTables T;
        CHECK(L.prepare(B.blocks(), 1, T, &msg, true) == 0);
        CHECK(T.comps[0].cls == 3 && T.comps[0].nca == 20 && T.comps[1].cls == 3 && T.comps[1].nca == 44 && T.comps[2].cls == 0);
        CHECK(T.order[3] == (std::vector<int>{1, 0}) && T.order[0] == std::vector<int>{2});
        CHECK(T.comps[1].ws0 == lm_batch_slice(40, 20, 0, 180, 1).total && T.comps[2].ws0 == T.comps[1].ws0 + lm_batch_slice(88, 44, 0, 396, 1).total);
        Lists W; W.add(range(0, 9 * 64), range(0, 128));
        CHECK(W.prepare(B.blocks(), 1, T, &msg, true) == 0 && T.comps[0].nca == 64 && T.comps[0].cls == 3 && T.comps[0].npa == 0 && T.comps[0].npair == 0);
        const std::vector<int> pabw = table(T, T.comps[0], T.comps[0].o_pab, 0);
        CHECK(pabw.empty());                                           // (no active point: no pair)
        Lists Q; Q.add(range(9 * 65, 9 * 65 + 3 * 66), range(0, 130)); // every point, the cameras constant: class 0
        CHECK(Q.prepare(B.blocks(), 1, T, &msg, true) == 0 && T.comps[0].cls == 0 && T.comps[0].npa == 66);
        Lists X; X.add(range(9 * 65, 9 * 65 + 3), {}); X.add(range(0, 9 * 65), range(0, 130));
        CHECK(X.prepare(B.blocks(), 1, T, &msg, true) == LM_BATCH_ERANGE);
        CHECK(msg.find("component 1") != std::string::npos && msg.find("65 active camera blocks") != std::string::npos && msg.find("limit is 64") != std::string::npos);
        CHECK(msg.find("RDIS_HIP_LM_WIDE_MAX_CAMERAS") != std::string::npos);
        // the highest pair of a 64-camera component with points: (63, 62) and (63, 63) come last, in that order
        Lists F; { std::vector<int64_t> fr = range(0, 9 * 64); for (int64_t v = 9 * 65; v < 9 * 65 + 3 * 66; ++v) fr.push_back(v); F.add(fr, range(0, 128)); }
        CHECK(F.prepare(B.blocks(), 2, T, &msg, true) == 0 && T.comps[0].nca == 64 && T.comps[0].npa == 66 && T.comps[0].npair == 64 + 63);
        const std::vector<int> pab = table(T, T.comps[0], T.comps[0].o_pab, 2 * 127);
        CHECK(pab[2 * 125] == 63 && pab[2 * 125 + 1] == 62 && pab[2 * 126] == 63 && pab[2 * 126 + 1] == 63);
        for (int q = 1; q < 127; ++q) CHECK(pab[2 * q] > pab[2 * q - 2] || (pab[2 * q] == pab[2 * q - 2] && pab[2 * q + 1] > pab[2 * q - 1]));
    }
    {   // ---- 16 cameras: the option changes no table, no order, no size ----
        const Problem Cq = chain(16);
        Lists L; L.add(range(0, 9 * 16 + 3 * 17), range(0, 32));
        LmBatchTables T0, T1;
        CHECK(L.prepare9(Cq.blocks(), 2, T0, &msg) == 0 && L.prepare(Cq.blocks(), 2, T1, &msg, true) == 0);
        CHECK(T0.comps[0].cls == 2 && T1.comps[0].cls == 2 && T0.comps[0].npair == 31 && T0.ints == T1.ints && T0.free32 == T1.free32);
        CHECK(T0.ws_doubles == T1.ws_doubles && T0.order[2] == T1.order[2] && T1.order[3].empty());
        const LmBatchComp& C = T0.comps[0];
        const std::vector<int> pab = table(T0, C, C.o_pab, 62);
        for (int a = 1; a < 16; ++a) CHECK(pab[2 * (2 * a - 1)] == a && pab[2 * (2 * a - 1) + 1] == a - 1 && pab[4 * a] == a && pab[4 * a + 1] == a);
    }
    std::printf("ok\n");
    return 0;
}
