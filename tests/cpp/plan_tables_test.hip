// plan_tables_test.hip -- rdis_amd/csrc/plan_tables.hpp on the host, no device: small bundle-adjustment components from a fixed
// integer recurrence through the table builders in the order rdis_hip.hip's prepare_partition calls them.  Prints the tables
// that tests/test_plan_tables.py compares with oracle/oracle.py's restatements, and checks their structure itself
// (exit status 1 and a line on stderr where a check fails).
//   plan_tables_test order <cameras> <points> <obs lo> <obs hi> <spread|wide|local> <compute units>
//   plan_tables_test owners
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../rdis_amd/csrc/plan_tables.hpp"
#include "../../rdis_amd/csrc/grid_sync.hpp"   // (COOP_LONG_LIST)

using namespace rdis_hip;

static const size_t LDS_LIMIT = 160 * 1024 - 4096;   // what a launch may ask for on the MI355X (solver_lds.hpp: LDS_MAX_BYTES)

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static unsigned long long lcg_state = 12345;
static unsigned lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(lcg_state >> 33); }

template <class V> static void print(const char* name, const V& v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

// a problem of ncam + 1 cameras and npt + 1 points: component 1 is the one under test, component 0 (the last camera and point,
// seven factors, listed first) only moves every plan-wide offset off zero
struct Problem {
    int ncam, npt, N;
    ivec cam, pt, block_of, ptblock_of, blk_stamp, blk_idx, owner_stamp, local;
    ivec fac_id, free_vid;    // plan-wide lists: component 0's, then component 1's
    int c0 = 0, f0 = 0;       // where component 1's start
    int cam_block(int c) const { return 9 * c; }
    int pt_block(int p) const { return 9 * (ncam + 1) + 3 * p; }
    void add(int c, int p) { cam.push_back(cam_block(c)); pt.push_back(pt_block(p)); }
    void finish(int first_free_cam) {
        N = 9 * (ncam + 1) + 3 * (npt + 1);
        block_of.assign((size_t)N, -1); ptblock_of.assign((size_t)N, -1);
        for (int c = 0; c <= ncam; ++c) for (int k = 0; k < 9; ++k) block_of[(size_t)(9 * c + k)] = 9 * c;
        for (int p = 0; p <= npt; ++p) for (int k = 0; k < 3; ++k) ptblock_of[(size_t)(pt_block(p) + k)] = pt_block(p);
        blk_stamp.assign((size_t)N, 0); blk_idx.assign((size_t)N, 0); owner_stamp.assign((size_t)N, 0); local.assign((size_t)N, -1);
        const int m = (int)cam.size();
        for (int j = 0; j < 7; ++j) { add(ncam, npt); fac_id.push_back(m + j); }
        c0 = 7;
        // component 1's factors in a scrambled listed order (a stride coprime to their number)
        int stride = m / 2 + 1;
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        while (gcd(stride, m) != 1) ++stride;
        for (int j = 0; j < m; ++j) fac_id.push_back((int)(((long long)j * stride) % m));
        for (int k = 0; k < 3; ++k) free_vid.push_back(pt_block(npt) + k);
        f0 = 3;
        for (int c = first_free_cam; c < ncam; ++c) for (int k = 0; k < 9; ++k) free_vid.push_back(9 * c + k);
    }
    BlockArrays arrays() { return BlockArrays{cam.data(), pt.data(), block_of.data(), ptblock_of.data(), blk_stamp.data(), blk_idx.data(), owner_stamp.data(), local.data()}; }
};

// every workgroup's segment rows cover the blocks of its chunks exactly once; its round tables count what each round stages
static void check_work_tables(const PtmStreamTables& T, int cc, int threads, int K) {
    const int nw = threads / 64, ncb_all = T.ls_ncb[cc], npb = (T.ls_ptr[cc + 1] - T.ls_ptr[cc] - PTM_CS * ncb_all) / 3, npc = (npb + 63) / 64;
    const bool local = T.local_comp == cc;
    const int* cp = T.cptr + T.pm_ch0[cc];
    ivec rows, nr;
    std::vector<long long> off, roff;
    ptm_segment_rows(T, threads, K, rows, off);
    for (int rk = 0; rk < K; ++rk) {
        ivec mine;   // the workgroup's chunks
        if (local) for (int ch = T.local->wg_chunk0[(size_t)rk]; ch < T.local->wg_chunk0[(size_t)rk + 1]; ++ch) mine.push_back(ch);
        else for (int ch = rk; ch < npc; ch += K) mine.push_back(ch);
        const int* r = rows.data() + off[(size_t)cc * K + rk];
        const int R = r[0];
        CHECK(R % nw == 0 && R >= 3 * nw, "rows %d of %d waves", R, nw);
        ivec covered((size_t)npc, 0);   // entries of a chunk covered so far: the shares must come in order, without gaps
        for (int w = 0; w < nw; ++w)
            for (int k = 0; k < R / nw; ++k) {
                const int ch = r[4 + k * nw + w], e0 = r[4 + R + k * nw + w], e1 = r[4 + 2 * R + k * nw + w];
                if (e1 == e0) continue;
                CHECK(ch >= 0 && ch < npc && e0 == cp[ch] + covered[(size_t)ch] && e1 > e0 && e1 <= cp[ch + 1], "threads %d K %d rank %d wave %d row %d", threads, K, rk, w, k);
                CHECK((e0 - cp[ch]) % (64 * PTM_BLK) == 0, "a share starts inside a block of slots");
                covered[(size_t)ch] = e1 - cp[ch];
            }
        for (int ch : mine) { CHECK(covered[(size_t)ch] == cp[ch + 1] - cp[ch], "chunk %d of rank %d covered %d of %d", ch, rk, covered[(size_t)ch], cp[ch + 1] - cp[ch]); covered[(size_t)ch] = 0; }
        for (int ch = 0; ch < npc; ++ch) CHECK(covered[(size_t)ch] == 0, "rank %d covers chunk %d of another workgroup", rk, ch);
    }
    for (int rs = 1; rs <= 2; ++rs) {
        std::vector<unsigned short> tab, grow;
        ptm_round_tables(T, threads, K, rs, tab, grow, roff, nr);
        for (int rk = 0; rk < K; ++rk) {
            const int ncb = local ? T.local->lc[(size_t)T.local->lc_off[(size_t)rk]] : ncb_all;
            const int stride = ptm_round_stride(ncb);
            std::vector<ivec> staged;   // per round: the entries it stages
            for (int w = 0; w < nw; ++w) {
                size_t rr = 0;
                const int ch0 = local ? T.local->wg_chunk0[(size_t)rk] + w : rk + K * w, chend = local ? T.local->wg_chunk0[(size_t)rk + 1] : npc, chstep = local ? nw : K * nw;
                for (int ch = ch0; ch < chend; ch += chstep)
                    for (int e = cp[ch]; e < cp[ch + 1]; e += 64 * rs, ++rr) {
                        if (staged.size() <= rr) staged.resize(rr + 1);
                        for (int l = 0; l < std::min(64 * rs, cp[ch + 1] - e); ++l) if (T.jg[e + l] >= 0) staged[rr].push_back(e + l);
                    }
            }
            CHECK((size_t)nr[(size_t)cc * K + rk] == staged.size(), "rounds of rank %d: %d against %zu", rk, nr[(size_t)cc * K + rk], staged.size());
            for (size_t rr = 0; rr < staged.size(); ++rr) {
                const unsigned short* rec = tab.data() + roff[(size_t)cc * K + rk] + rr * (size_t)stride;
                CHECK(rec[ncb] == staged[rr].size(), "round %zu of rank %d: last entry %d, %zu factors staged", rr, rk, (int)rec[ncb], staged[rr].size());
                cvec seen(staged[rr].size(), 0);
                for (int e : staged[rr]) {
                    const int g = grow[(size_t)e], cam = local ? (int)T.local->pm_lcam[(size_t)e] : (T.ls_fidx[T.jg[e]] & 0xFFF);
                    CHECK(g < (int)seen.size() && !seen[(size_t)g], "round %zu: row %d taken twice or out of range", rr, g);
                    CHECK(g >= rec[cam] && g < rec[cam + 1], "round %zu: row %d outside the segment of camera %d", rr, g, cam);
                    seen[(size_t)g] = 1;
                }
            }
        }
    }
}

static int run_order(int ncam, int npt, int lo, int hi, const std::string& how, int cus) {
    Problem P;
    P.ncam = ncam; P.npt = npt;
    for (int p = 0; p < npt; ++p) {   // lo .. hi observations of distinct cameras per point
        const int k = lo + (int)(lcg() % (unsigned)(hi - lo + 1));
        int seen[8];
        for (int t = 0; t < k; ++t) {
            int c;
            bool again;
            do { c = (int)(lcg() % (unsigned)ncam); again = false; for (int s = 0; s < t; ++s) again = again || seen[s] == c; } while (again);
            seen[t] = c;
            P.add(c, p);
        }
    }
    P.finish(1);   // (camera 0 is a constant of the component: it has slots, no free index)
    for (int p = 0; p < npt; ++p) for (int k = 0; k < 3; ++k) P.free_vid.push_back(P.pt_block(p) + k);
    const int m = (int)P.fac_id.size() - P.c0, n = (int)P.free_vid.size() - P.f0, c0 = P.c0;
    const BlockArrays B = P.arrays();
    const CompLists C{P.fac_id.data() + c0, m, P.free_vid.data() + P.f0, n, nullptr};
    ivec cams, pts, deg, gp;
    bool free_cam = false;
    CHECK(block_census(B, C, 1, cams, &pts, &free_cam) && free_cam, "census");
    ivec only_cams;
    CHECK(block_census(B, C, 2, only_cams, nullptr) && only_cams == cams, "the census without points finds other cameras");
    std::sort(cams.begin(), cams.end());
    number_blocks(B, cams);
    const int ncb = (int)cams.size(), npb = (int)pts.size();
    gradient_pass_order(B, C, ncb, free_cam, gp);
    {   // every listed factor once, a wave-chunk of 64 has one camera
        cvec seen((size_t)m, 0);
        CHECK(gp.size() % 64 == 0, "gp is not whole waves");
        for (size_t i = 0; i < gp.size(); ++i) {
            if (gp[i] < 0) continue;
            CHECK(!seen[(size_t)gp[i]], "gp lists factor %d twice", gp[i]); seen[(size_t)gp[i]] = 1;
            const int first = gp[i / 64 * 64];
            CHECK(first >= 0 && P.cam[(size_t)C.fac_id[gp[i]]] == P.cam[(size_t)C.fac_id[first]], "a chunk of gp mixes cameras");
        }
        for (int j = 0; j < m; ++j) CHECK(seen[(size_t)j], "gp misses factor %d", j);
    }
    PtmLocalTables loc;
    std::vector<ivec> local_cams;
    PtmLocalReport rep;
    const PtmDeal deal = how == "local" ? PtmDeal::LOCAL : how == "wide" ? PtmDeal::WIDE : PtmDeal::SPREAD;
    const bool fits = ptm_point_order(B, C, ncb, deal, cus, LDS_LIMIT, pts, deg, loc.wg_chunk0, local_cams, rep);
    ivec fcam, fpt;
    for (int j = 0; j < m; ++j) { fcam.push_back(P.cam[(size_t)C.fac_id[j]]); fpt.push_back(P.pt[(size_t)C.fac_id[j]]); }
    print("factor_cam", fcam); print("factor_pt", fpt);
    std::printf("fits %d\n", fits ? 1 : 0);
    if (!fits) { std::printf("ok\n"); return 0; }
    print("cams", cams); print("pts", pts); print("wg_chunk0", loc.wg_chunk0);
    // the slot table and the factor stream, as the plan's int32 block holds them (two components, the first without tables)
    ivec sv, sf, fidx((size_t)(c0 + m), 0), pidx((size_t)(c0 + m), 0), pptr, pm_jg, cptr, cbase;
    slot_table(B, C, 1, cams, pts, true, sv, sf, fidx.data() + c0, pidx.data() + c0, pptr);
    CHECK((int)sv.size() == PTM_CS * ncb + 3 * npb && sf.size() == sv.size(), "slots");
    for (size_t s = 0; s < sv.size(); ++s) {   // a free slot names its variable's place in the free list
        if (sf[s] >= 0) CHECK(C.free_vid[sf[s]] == sv[s], "slot %zu", s);
        else CHECK(s < (size_t)PTM_CS * ncb && (sv[s] < 9 || (int)(s % PTM_CS) == PTM_CS - 1), "slot %zu is no constant", s);
    }
    pm_jg.assign(5, -1);   // (another component's entries in front)
    const int e0 = (int)pm_jg.size();
    cptr.push_back(0);
    ptm_factor_stream(c0, m, pidx.data() + c0, pptr, pm_jg, cptr, cbase);
    {   // every factor of the component once and -1 elsewhere; entry cptr[ch] + 64 t + lane is the t-th listed factor of the lane's block
        ivec count((size_t)(c0 + m), 0);
        for (size_t e = 0; e < pm_jg.size(); ++e) if (pm_jg[e] >= 0) { CHECK((int)e >= e0 && pm_jg[e] >= c0 && pm_jg[e] < c0 + m, "entry %zu", e); ++count[(size_t)pm_jg[e]]; }
        for (int j = 0; j < c0 + m; ++j) CHECK(count[(size_t)j] == (j >= c0 ? 1 : 0), "factor %d is listed %d times", j, count[(size_t)j]);
        std::vector<ivec> of((size_t)npb);
        for (int j = 0; j < m; ++j) of[(size_t)B.blk_idx[(size_t)P.pt[(size_t)C.fac_id[j]]]].push_back(c0 + j);
        const int npc = (npb + 63) / 64;
        CHECK((int)cptr.size() == npc + 2, "cptr");
        for (int ch = 0; ch < npc; ++ch) {
            const int slots = (cptr[(size_t)ch + 2] - cptr[(size_t)ch + 1]) / 64;
            CHECK(slots == (int)of[(size_t)(64 * ch)].size(), "chunk %d: %d slots", ch, slots);
            for (int t = 0; t < slots; ++t)
                for (int lane = 0; lane < 64; ++lane) {
                    const int b = 64 * ch + lane, want = b < npb && t < (int)of[(size_t)b].size() ? of[(size_t)b][(size_t)t] : -1;
                    CHECK(pm_jg[(size_t)(cptr[(size_t)ch + 1] + 64 * t + lane)] == want, "chunk %d slot %d lane %d", ch, t, lane);
                }
        }
    }
    if (deal == PtmDeal::LOCAL) {
        ptm_local_tables(ncb, local_cams, cbase, e0, pm_jg, fidx.data(), loc);
        std::printf("local_K %d\n", rep.K);
        CHECK((int)loc.cr_ptr.size() == ncb + 1 && rep.worst <= rep.cam_cap, "local tables");
        for (size_t e = 0; e + e0 < pm_jg.size(); ++e)   // a workgroup's number for a camera leads back to the camera
            if (pm_jg[e + e0] >= 0) {
                int rk = 0;
                while (cbase[(size_t)loc.wg_chunk0[(size_t)rk + 1]] <= (int)e) ++rk;
                CHECK(local_cams[(size_t)rk][(size_t)loc.pm_lcam[e]] == (fidx[(size_t)pm_jg[e + e0]] & 0xFFF), "entry %zu", e);
            }
    }
    ivec ls_ptr{0, 0, (int)sv.size()}, ls_ncb{0, ncb}, pm_ch0{0, 1}, comps{1};
    // (the work tables address entries from the component's chunk table on: the local group's tables count from its first entry)
    ivec jg_comp(pm_jg.begin() + e0, pm_jg.end()), cptr_comp{0};
    for (size_t k = 1; k < cptr.size(); ++k) cptr_comp.push_back(cptr[k] - e0);
    PtmStreamTables T;
    T.ncomp = 2; T.pm_entries = (int64_t)jg_comp.size(); T.comps = comps.data(); T.ncomps = 1;
    T.ls_ptr = ls_ptr.data(); T.ls_ncb = ls_ncb.data(); T.ls_fidx = fidx.data(); T.pm_ch0 = pm_ch0.data(); T.cptr = cptr_comp.data(); T.jg = jg_comp.data();
    T.local_comp = deal == PtmDeal::LOCAL ? 1 : -1; T.local = &loc;
    check_work_tables(T, 1, 256, 1); check_work_tables(T, 1, 512, 4); check_work_tables(T, 1, 768, 1);
    if (deal == PtmDeal::LOCAL) check_work_tables(T, 1, PTM_WIDE_THREADS, rep.K);
    std::printf("ok\n");
    return 0;
}

// one free camera with 200 factors, one free point with one of them: nine variables on long lists, three on short ones
static int run_owners() {
    Problem P;
    P.ncam = 1; P.npt = 200;
    for (int p = 0; p < 200; ++p) P.add(0, p);
    P.finish(0);
    for (int k = 0; k < 3; ++k) P.free_vid.push_back(P.pt_block(17) + k);
    const int m = 200, n = 12;
    ivec v2s{0};
    for (int i = 0; i < n; ++i) v2s.push_back(v2s.back() + (i < 9 ? 200 : 1));
    const CompLists C{P.fac_id.data() + P.c0, m, P.free_vid.data() + P.f0, n, v2s.data()};
    ivec fcam, fpt, fv(C.free_vid, C.free_vid + n), sl, lane_var, wave_var;
    for (int j = 0; j < m; ++j) { fcam.push_back(P.cam[(size_t)C.fac_id[j]]); fpt.push_back(P.pt[(size_t)C.fac_id[j]]); }
    coop_slot_li(P.arrays(), C, 1, sl);
    std::printf("long_list %d\n", COOP_LONG_LIST);
    print("factor_cam", fcam); print("factor_pt", fpt); print("free_vid", fv); print("slot_li", sl);
    for (int lanes : {128, 640}) {   // fewer waves than long lists; the group the dispatcher forms (five workgroups of 128 factor lanes)
        coop_owner_tables(C, lanes, COOP_LONG_LIST, lane_var, wave_var);
        CHECK((int)lane_var.size() == lanes && (int)wave_var.size() == lanes / 64, "sizes");
        print(lanes == 128 ? "wave_var_128" : "wave_var_640", wave_var);
        print(lanes == 128 ? "lane_var_128" : "lane_var_640", lane_var);
    }
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "owners")) return run_owners();
    if (argc == 8 && !std::strcmp(argv[1], "order"))
        return run_order(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), argv[6], std::atoi(argv[7]));
    std::fprintf(stderr, "usage: plan_tables_test order <cameras> <points> <obs lo> <obs hi> <spread|wide|local> <compute units> | owners\n");
    return 2;
}
