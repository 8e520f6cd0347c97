// grad_tables_test.cpp -- rdis_amd/csrc/grad_tables.hpp without a device (tests/test_grad_tables_cpu.py).  Reads cases from
// standard input, whitespace-separated integers:
//   case N ncb GW tile_chunks cam_soft F cam[F] pt[F] cam_ord[N] nf m fac[m]        (m = -1: fac is null; else m = nf)
// and prints each case's tables as lines "<name> <entries ...>" up to a line "end": the scalars, the int32 block's offsets, the
// block, the 16-bit block.  Its own checks: every offset is even and inside the block, the blocks have the sizes the scalars say.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../rdis_amd/csrc/grad_tables.hpp"

using namespace rdis_hip;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

template <class V> static void print(const char* name, const V& v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

template <class T> static std::vector<T> read(size_t n) {
    std::vector<T> v(n);
    for (auto& x : v) { long long t; if (!(std::cin >> t)) { std::fprintf(stderr, "short input\n"); std::exit(2); } x = (T)t; }
    return v;
}

int main() {
    static_assert(sizeof(IntPair) == 2 * sizeof(int), "a pair is two ints");
    std::string cmd;
    while (std::cin >> cmd) {
        CHECK(cmd == "case", "unknown command %s", cmd.c_str());
        long long N, ncb, GW, tile_chunks, cam_soft, F, nf, m;
        std::cin >> N >> ncb >> GW >> tile_chunks >> cam_soft >> F;
        const std::vector<int> cam = read<int>((size_t)F), pt = read<int>((size_t)F), cam_ord = read<int>((size_t)N);
        std::cin >> nf >> m;
        CHECK(m == -1 || m == nf, "m = %lld", m);
        const std::vector<int64_t> fac = read<int64_t>((size_t)(m < 0 ? 0 : m));
        GradIndex T;
        grad_tables_build((size_t)N, (size_t)ncb, cam.data(), pt.data(), cam_ord.data(), (int)nf, m < 0 ? nullptr : fac.data(), (int)GW,
                          (int)tile_chunks, (int)cam_soft, T);
        const std::vector<size_t> off{T.o_ptv, T.o_tc0, T.o_tm0, T.o_tcam, T.o_cs0, T.o_cseg, T.o_ps0, T.o_pseg, T.o_csv, T.o_csp, T.o_psv, T.o_psp, T.o_z};
        for (size_t i = 0; i < off.size(); ++i) {
            CHECK(off[i] % 2 == 0 && off[i] <= T.blk.size(), "offset %zu = %zu of %zu", i, off[i], T.blk.size());
            CHECK(i == 0 || off[i] >= off[i - 1], "offset %zu below its predecessor", i);
        }
        CHECK(T.npad == (size_t)T.nchunks * (size_t)GW && T.sh.size() == 3 * T.npad, "16-bit block: %zu entries, npad %zu", T.sh.size(), T.npad);
        CHECK(T.nchunks == (nf + GW - 1) / GW, "nchunks %d", T.nchunks);
        print("scalars", std::vector<long long>{T.nchunks, T.ntiles, T.ncam_cap, T.ncs, T.nps, T.nz, T.cstage_slots, T.pstage_slots, (long long)T.npad});
        print("offsets", off);
        print("blk", T.blk);
        print("sh", T.sh);
        std::printf("end\n");
    }
    std::printf("ok\n");
    return 0;
}
