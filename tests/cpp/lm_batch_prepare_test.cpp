// The host half of rdis_hip_lm_batch without a device (rdis_amd/csrc/lm_batch.hpp: no HIP in it when compiled by a host
// compiler): component classes, the LDS of a class, the workspace slice, and lm_batch_prepare's tables, refusals and order
// on small problems written out by hand.  Prints "ok".
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
    LmBatchBlocks blocks(bool layout) const {
        return LmBatchBlocks{9 * ncams + 3 * npts, (int64_t)cam.size(), cam.data(), pt.data(), block_of.data(), ptblock_of.data(), layout, ncams};
    }
};

struct Lists {
    std::vector<int64_t> free_ptr{0}, free_vid, fac_ptr{0}, fac_id;
    void add(const std::vector<int64_t>& fr, const std::vector<int64_t>& fc) {
        free_vid.insert(free_vid.end(), fr.begin(), fr.end()); fac_id.insert(fac_id.end(), fc.begin(), fc.end());
        free_ptr.push_back((int64_t)free_vid.size()); fac_ptr.push_back((int64_t)fac_id.size());
    }
    int prepare(const LmBatchBlocks& B, int R, LmBatchTables& T, std::string* msg) const {
        return lm_batch_prepare(B, (int64_t)free_ptr.size() - 1, free_ptr.data(), free_vid.data(), fac_ptr.data(), fac_id.data(), R, T, msg);
    }
};

static std::vector<int64_t> range(int64_t a, int64_t b) { std::vector<int64_t> v; for (int64_t i = a; i < b; ++i) v.push_back(i); return v; }
static std::vector<int> table(const LmBatchTables& T, const LmBatchComp& C, int off, int n) {
    return std::vector<int>(T.ints.begin() + C.ints0 + off, T.ints.begin() + C.ints0 + off + n);
}

int main() {
    // ---- classes: a function of the camera count alone; the LDS of the largest fits one workgroup's 160 KiB ----
    CHECK(lm_batch_class(0) == 0 && lm_batch_class(1) == 1 && lm_batch_class(6) == 1 && lm_batch_class(7) == 2 && lm_batch_class(16) == 2);
    for (int nca = 0; nca <= LM_BATCH_MAX_CAMERAS; ++nca) CHECK(nca <= lm_batch_class_cameras(lm_batch_class(nca)));
    CHECK(lm_batch_class_threads(0) == 64 && lm_batch_class_threads(1) == 256 && lm_batch_class_threads(2) == 512);
    CHECK(lm_batch_lds_doubles(0) * 8 == 512);
    CHECK(lm_batch_lds_doubles(6) == 64 + 486 + 108 + 55 * 56 / 2 && lm_batch_lds_doubles(6) * 8 < 20 * 1024);
    CHECK(lm_batch_lds_doubles(16) == 64 + 1296 + 288 + 145 * 146 / 2 && lm_batch_lds_doubles(16) * 8 <= 160 * 1024);
    {   // ---- the slice: consecutive, 16-byte granules, no Z blocks without cameras or without points ----
        const LmBatchSlice s = lm_batch_slice(7, 2, 3, 27, 2);
        const long long o[] = {s.Jc, s.Jp, s.e, s.T, s.Zc, s.V, s.bp, s.Lp, s.yp, s.dp, s.psave, s.total};
        const long long n[] = {126, 42, 14, 42, 189, 18, 9, 18, 9, 9, 27};
        CHECK(o[0] == 0);
        for (int i = 0; i < 11; ++i) CHECK(o[i] % 2 == 0 && o[i + 1] >= o[i] + n[i] && o[i + 1] <= o[i] + n[i] + 1);
        CHECK(lm_batch_slice(7, 0, 3, 9, 1).V == lm_batch_slice(7, 0, 3, 9, 1).Zc && lm_batch_slice(7, 2, 0, 18, 1).V == lm_batch_slice(7, 2, 0, 18, 1).Zc);
    }
    std::string msg;
    // ---- one component: 2 cameras x 3 points, factors 0:(c0,p0) 1:(c1,p0) 2:(c0,p1) 3:(c1,p2) 4:(c1,p1) ----
    const Problem A(2, 3, {{0, 0}, {1, 0}, {0, 1}, {1, 2}, {1, 1}});
    {
        Lists L; L.add(range(0, 27), range(0, 5));
        LmBatchTables T;
        CHECK(L.prepare(A.blocks(true), 1, T, &msg) == 0);
        const LmBatchComp& C = T.comps[0];
        CHECK(C.nf == 5 && C.nca == 2 && C.npa == 3 && C.nfree == 27 && C.cls == 1 && C.npair == 3 && C.ws0 == 0 && C.free0 == 0 && C.comp == 0);
        CHECK(table(T, C, C.o_fci, 5) == (std::vector<int>{0, 1, 0, 1, 1}) && table(T, C, C.o_fpi, 5) == (std::vector<int>{0, 0, 1, 2, 1}));
        CHECK(table(T, C, C.o_cptr, 3) == (std::vector<int>{0, 2, 5}) && table(T, C, C.o_clist, 5) == (std::vector<int>{0, 2, 1, 3, 4}));
        CHECK(table(T, C, C.o_pptr, 4) == (std::vector<int>{0, 2, 4, 5}) && table(T, C, C.o_plist, 5) == (std::vector<int>{0, 1, 2, 4, 3}));
        // pairs (0,0) (1,0) (1,1), entries in point order
        CHECK(table(T, C, C.o_pab, 6) == (std::vector<int>{0, 0, 1, 0, 1, 1}) && table(T, C, C.o_pairptr, 4) == (std::vector<int>{0, 2, 4, 7}));
        CHECK(table(T, C, C.o_pja, 7) == (std::vector<int>{0, 2, 1, 4, 1, 4, 3}) && table(T, C, C.o_pjb, 7) == (std::vector<int>{0, 2, 0, 2, 1, 4, 3}));
        const std::vector<int> fs = table(T, C, C.o_fslot, 27);
        for (int i = 0; i < 18; ++i) CHECK(fs[(size_t)i] == i);
        for (int i = 0; i < 9; ++i) CHECK(fs[(size_t)(18 + i)] == -i - 2);
        CHECK(T.ws_doubles == lm_batch_slice(5, 2, 3, 27, 1).total && T.order[1] == std::vector<int>{0} && T.order[0].empty() && T.order[2].empty());
        for (int v = 0; v < 27; ++v) CHECK(T.freem[(size_t)v] == 1);
    }
    {   // ---- the points alone (cameras constant), listed p2, p0, p1; and camera 1's translation alone over its factors ----
        Lists L; L.add(range(24, 27), {3}); L.add(range(18, 21), {0, 1}); L.add(range(21, 24), {2, 4}); L.add(range(12, 15), {});
        LmBatchTables T;
        CHECK(L.prepare(A.blocks(false), 2, T, &msg) == 0);
        CHECK(T.comps[0].cls == 0 && T.comps[0].nca == 0 && T.comps[0].npa == 1 && T.comps[0].npair == 0);
        CHECK(table(T, T.comps[1], T.comps[1].o_fci, 2) == (std::vector<int>{-1, -1}) && table(T, T.comps[1], T.comps[1].o_fpi, 2) == (std::vector<int>{0, 0}));
        CHECK(T.order[0] == (std::vector<int>{1, 2, 0}));             // heaviest first, equal weights in the caller's order
        CHECK(T.comps[3].cls == 1 && T.comps[3].nca == 1 && T.comps[3].nf == 0 && T.order[1] == std::vector<int>{3});
        CHECK(table(T, T.comps[3], T.comps[3].o_fslot, 3) == (std::vector<int>{3, 4, 5}));   // a block with constant variables keeps its numbering
        CHECK(T.comps[1].ws0 == lm_batch_slice(1, 0, 1, 3, 2).total && T.comps[2].free0 == 6);
        CHECK(T.freem[12] == 1 && T.freem[9] == 0 && T.freem[0] == 0);
    }
    {   // ---- a variable no factor reads: the layout's block where the layout holds, no block otherwise ----
        const Problem Bq(3, 1, {{0, 0}, {1, 0}});   // camera 2 (18 .. 26) is read by nothing
        Lists L; L.add(range(18, 27), {});
        LmBatchTables T;
        CHECK(L.prepare(Bq.blocks(true), 1, T, &msg) == 0 && T.comps[0].nca == 1 && table(T, T.comps[0], T.comps[0].o_fslot, 9)[8] == 8);
        CHECK(L.prepare(Bq.blocks(false), 1, T, &msg) == 0 && T.comps[0].nca == 0 && T.comps[0].cls == 0 && table(T, T.comps[0], T.comps[0].o_fslot, 9)[8] == -1);
    }
    {   // ---- 16 cameras pass, 17 are refused by name, also behind a valid component ----
        std::vector<std::pair<int, int>> fac;
        for (int c = 0; c < 17; ++c) fac.push_back({c, 0});
        const Problem Cq(17, 2, fac);
        Lists ok; ok.add(range(0, 9 * 16), range(0, 16));
        LmBatchTables T;
        CHECK(ok.prepare(Cq.blocks(true), 1, T, &msg) == 0 && T.comps[0].nca == 16 && T.comps[0].cls == 2);
        Lists bad; bad.add(range(9 * 17, 9 * 17 + 3), {}); bad.add(range(0, 9 * 17), range(0, 17));
        CHECK(bad.prepare(Cq.blocks(true), 1, T, &msg) == LM_BATCH_ERANGE);
        CHECK(msg.find("component 1") != std::string::npos && msg.find("17 active camera blocks") != std::string::npos && msg.find("limit is 16") != std::string::npos);
    }
    {   // ---- two listed factors joining the same camera and point; fine where the camera is constant ----
        const Problem D(1, 1, {{0, 0}, {0, 0}});
        Lists L; L.add(range(0, 12), {0, 1});
        LmBatchTables T;
        CHECK(L.prepare(D.blocks(true), 1, T, &msg) == LM_BATCH_EINVAL && msg.find("same camera and point") != std::string::npos);
        Lists P; P.add(range(9, 12), {0, 1});
        CHECK(P.prepare(D.blocks(true), 1, T, &msg) == 0 && T.comps[0].npa == 1 && T.comps[0].nf == 2);
    }
    std::printf("ok\n");
    return 0;
}
