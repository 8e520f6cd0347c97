// plan_index_test.cpp -- rdis_amd/csrc/plan_index.hpp without a device (tests/test_plan_index_cpu.py).  Reads commands from
// standard input, whitespace-separated integers after the command's name:
//   problem ba  N F cam[F] pt[F] ncam_blocks block_of[N]     a problem's host arrays and fresh scratch (marks, stamps)
//   problem nlp N F rowptr[F + 1] nvid vid[nvid]
//   call ncomp free_ptr[ncomp + 1] n free_vid[n] fac_ptr[ncomp + 1] m fac_id[m]
//        plan_index_check, then plan_index_build with the next stamp on the problem's scratch (n or m = -1: a null pointer;
//        n and m say how many ids FOLLOW, the pointer arrays' last entries may claim more)
// and answers each call with "rc <code> <message>" and, where the code is 0, the tables as lines "<name> <entries ...>" up to
// a line "end".  Its own check: the kept lists are the caller's ids.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../rdis_amd/csrc/plan_index.hpp"

using namespace rdis_hip;

template <class V> static void print(const char* name, const V& v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

static std::vector<int64_t> read64(size_t n) {
    std::vector<int64_t> v(n);
    for (auto& x : v) if (!(std::cin >> x)) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}
static std::vector<int> read32(size_t n) {
    std::vector<int> v(n);
    for (auto& x : v) if (!(std::cin >> x)) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}

int main() {
    std::string cmd, kind;
    int64_t N = 0, F = 0, ncam_blocks = 0;
    bool ba = true;
    std::vector<int> cam, pt, rowptr, vid, block_of, fac_stamp;
    std::vector<VarMark> mark;
    int stamp = 0;
    while (std::cin >> cmd) {
        if (cmd == "problem") {
            std::cin >> kind >> N >> F;
            ba = kind == "ba";
            cam.clear(); pt.clear(); rowptr.clear(); vid.clear(); block_of.clear();
            if (ba) {
                cam = read32((size_t)F); pt = read32((size_t)F);
                std::cin >> ncam_blocks;
                block_of = read32((size_t)N);
            } else {
                rowptr = read32((size_t)F + 1);
                int64_t nvid = 0;
                std::cin >> nvid;
                vid = read32((size_t)nvid);
                ncam_blocks = 0;
            }
            mark.assign((size_t)N, VarMark{0, -1, -1, 0});   // (as rdis_hip.hip's ensure_problem_scratch leaves them)
            fac_stamp.assign((size_t)F, 0);
            stamp = 0;
        } else if (cmd == "call") {
            int64_t ncomp = 0, n = 0, m = 0;
            std::cin >> ncomp;
            const std::vector<int64_t> free_ptr = read64((size_t)ncomp + 1);
            std::cin >> n;
            const std::vector<int64_t> free_vid = read64((size_t)std::max<int64_t>(n, 0));
            const std::vector<int64_t> fac_ptr = read64((size_t)ncomp + 1);
            std::cin >> m;
            const std::vector<int64_t> fac_id = read64((size_t)std::max<int64_t>(m, 0));
            static const int64_t none = 0;   // (an empty list is still a pointer)
            const int64_t* fv = n < 0 ? nullptr : n == 0 ? &none : free_vid.data();
            const int64_t* fi = m < 0 ? nullptr : m == 0 ? &none : fac_id.data();
            std::string message;
            PlanIndex X;
            int rc = plan_index_check(ncomp, free_ptr.data(), fv, fac_ptr.data(), fi, &message);
            if (!rc) {
                const IndexArrays P{ba ? PLAN_INDEX_KIND_BA : 1, N, F, cam.data(), pt.data(), rowptr.data(), vid.data(), block_of.data(),
                                    ncam_blocks, mark.data(), fac_stamp.data(), ++stamp};
                rc = plan_index_build(P, ncomp, free_ptr.data(), fv, fac_ptr.data(), fi, X, &message);
            }
            std::printf("rc %d %s\n", rc, message.c_str());
            if (rc) continue;
            if (!message.empty()) { std::fprintf(stderr, "a message on the accepting path\n"); return 1; }
            for (size_t i = 0; i < X.h_free_vid.size(); ++i) if (X.h_free_vid[i] != free_vid[i]) { std::fprintf(stderr, "free_vid %zu\n", i); return 1; }
            for (size_t i = 0; i < X.h_fac_id.size(); ++i) if (X.h_fac_id[i] != fac_id[i]) { std::fprintf(stderr, "fac_id %zu\n", i); return 1; }
            print("free_ptr", X.h_free_ptr); print("free_vid", X.h_free_vid); print("fac_ptr", X.h_fac_ptr); print("fac_id", X.h_fac_id);
            print("v2s_ptr", X.h_v2s_ptr); print("slot_li", X.h_slot_li); print("order", X.h_order);
            print("counts", std::vector<int64_t>{X.nslots, X.ngfac});
            print("offsets", std::vector<size_t>{X.off_order, X.off_free_ptr, X.off_free_vid, X.off_fac_ptr, X.off_fac_id, X.off_v2s_ptr, X.off_slot_base,
                                                 X.off_slot_pos, X.off_cb_ptr, X.off_cb, X.off_cb_li});
            print("blk", X.h_blk);
            std::printf("end\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
