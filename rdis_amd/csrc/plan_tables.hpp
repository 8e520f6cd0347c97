// plan_tables.hpp -- the index tables a plan's solvers read, built on the host from plain arrays: the owner tables of a
// cooperative group, a component's camera / point blocks, the LDS-resident solver's slot table, the point-major order,
// factor stream and local-group tables of the streaming solver, and its gradient's segment rows and round tables.  The
// order in which every gradient is summed follows these tables.  Pure integer work: no HIP call, no plan, no problem,
// no environment (rdis_hip.hip decides which solver takes a component, allocates and uploads); tests/cpp/plan_tables_test.hip
// runs it without a device against oracle/oracle.py's restatements.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "host_blocks.hpp"
#include "ptm_api.hpp"   // (layout constants and ptm_bytes_for)

namespace rdis_hip {

// a bundle-adjustment problem's host arrays; a block is named by the id of its first variable
struct BlockArrays {
    const int* cam;          // [F] a factor's camera block
    const int* pt;           // [F] ... and point block
    const int* block_of;     // [N] the camera block a variable belongs to, -1 = none
    const int* ptblock_of;   // [N] ... the point block, -1 = none
    int* blk_stamp;          // [N] scratch, valid for one stamp: block seen
    int* blk_idx;            // [N] scratch: a block's number within the component at hand
    int* owner_stamp;        // [N] scratch, valid for one stamp: variable free in the component at hand ...
    int* local;              // [N] ... and its index in the component's free list
};
// one component's lists
struct CompLists {
    const int* fac_id; int m;     // its listed factors
    const int* free_vid; int n;   // its free variables
    const int* v2s_ptr;           // [n + 1] CSR of the partials that feed each free variable
};

// ---------------------------------------------------------------------------------------------------------------------
// cooperative groups

// local free index of each factor slot (for a plan that did not keep plan_create's table), formed from the per-problem
// marks, valid for one stamp
inline void coop_slot_li(const BlockArrays& B, const CompLists& C, int stamp, ivec& sl) {
    for (int i = 0; i < C.n; ++i) { B.local[(size_t)C.free_vid[i]] = i; B.owner_stamp[(size_t)C.free_vid[i]] = stamp; }
    sl.resize((size_t)12 * (size_t)C.m);
    for (int j = 0; j < C.m; ++j) {
        const int f = C.fac_id[j];
        for (int k = 0; k < 12; ++k) {
            const int v = k < 9 ? B.cam[f] + k : B.pt[f] + (k - 9);
            sl[(size_t)(12 * (size_t)j + k)] = B.owner_stamp[(size_t)v] == stamp ? B.local[(size_t)v] : -1;
        }
    }
}
// owners of the CG recurrence: a lane per variable, a whole wave for variables fed by
// many partials (more than long_list: grid_sync.hpp's COOP_LONG_LIST; longest first), see solver_coop.hpp
inline void coop_owner_tables(const CompLists& C, int lanes, int long_list, ivec& lane_var, ivec& wave_var) {
    const int waves = lanes / 64;
    lane_var.assign((size_t)lanes, -1);
    wave_var.assign((size_t)waves, -1);
    ivec longv;
    for (int i = 0; i < C.n; ++i)
        if (C.v2s_ptr[i + 1] - C.v2s_ptr[i] > long_list) longv.push_back(i);
    std::stable_sort(longv.begin(), longv.end(), [&](int a, int b) {
        return (C.v2s_ptr[a + 1] - C.v2s_ptr[a]) > (C.v2s_ptr[b + 1] - C.v2s_ptr[b]);
    });
    cvec wave_owned((size_t)C.n, 0);
    for (size_t k = 0; k < longv.size() && (int)k < waves; ++k) { wave_var[k] = longv[k]; wave_owned[(size_t)longv[k]] = 1; }
    for (int i = 0; i < C.n; ++i) if (!wave_owned[(size_t)i]) lane_var[(size_t)i] = i;
}

// ---------------------------------------------------------------------------------------------------------------------
// a component's blocks

// The camera blocks (and, with pts, the point blocks) that a component's factors read or its free variables belong to, in the
// order met; free_cam: a camera variable is free.  false: a variable no factor of the problem reads -- no block to put it in.
inline bool block_census(const BlockArrays& B, const CompLists& C, int stamp, ivec& cams, ivec* pts, bool* free_cam = nullptr) {
    cams.clear();
    if (pts) pts->clear();
    if (free_cam) *free_cam = false;
    auto note = [&](int b, ivec& list) {
        if (B.blk_stamp[(size_t)b] != stamp) { B.blk_stamp[(size_t)b] = stamp; list.push_back(b); }
    };
    for (int j = 0; j < C.m; ++j) { const int f = C.fac_id[j]; note(B.cam[(size_t)f], cams); if (pts) note(B.pt[(size_t)f], *pts); }
    for (int i = 0; i < C.n; ++i) {
        const int v = C.free_vid[i];
        if (B.block_of[(size_t)v] >= 0) { note(B.block_of[(size_t)v], cams); if (free_cam) *free_cam = true; }
        else if (B.ptblock_of[(size_t)v] >= 0) { if (pts) note(B.ptblock_of[(size_t)v], *pts); }
        else return false;
    }
    return true;
}
// a block's number within the component: its place in the list
inline void number_blocks(const BlockArrays& B, const ivec& blocks) {
    for (size_t k = 0; k < blocks.size(); ++k) B.blk_idx[(size_t)blocks[k]] = (int)k;
}

// the order of the gradient pass: camera by camera (listed order within a camera), whole waves per camera --
// where a camera variable is free; otherwise nothing is summed per camera and the listed order serves
// (the camera blocks numbered: number_blocks)
inline void gradient_pass_order(const BlockArrays& B, const CompLists& C, int ncb, bool free_cam, ivec& gp) {
    const int m = C.m;
    if (free_cam) {
        ivec start((size_t)ncb + 1, 0);
        for (int j = 0; j < m; ++j) ++start[(size_t)B.blk_idx[(size_t)B.cam[(size_t)C.fac_id[j]]] + 1];
        for (int k = 0; k < ncb; ++k) start[(size_t)k + 1] = start[(size_t)k] + (start[(size_t)k + 1] + 63) / 64 * 64;
        gp.assign((size_t)start[(size_t)ncb], -1);
        for (int j = 0; j < m; ++j) gp[(size_t)start[(size_t)B.blk_idx[(size_t)B.cam[(size_t)C.fac_id[j]]]]++] = j;
    } else {
        gp.assign((size_t)((m + 63) / 64 * 64), -1);
        std::iota(gp.begin(), gp.begin() + m, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the streaming solver's point-major order

enum class PtmDeal { SPREAD, WIDE, LOCAL };   // how a component's wave-chunks are dealt out: a launch of many components or small groups, a wide group, a wide group with local cameras
struct PtmLocalReport {    // what the deal of a local group found (RDIS_HIP_LOCAL_STATS prints it)
    bool dealt = false;    // the component had the chunks for a local group: the figures below are set
    int K = 0, chunks = 0;
    size_t worst = 0, cam_cap = 0;   // most cameras in a workgroup; what the LDS holds
};

// The component's point blocks `pts` (any order on entry) in the streaming solver's order; the camera blocks numbered
// (number_blocks).  `deg` is scratch.  LOCAL: also the workgroups' chunk ranges and camera lists (component numbers,
// ascending); false -- and only then -- when local numbering does not fit (too few chunks, a workgroup's cameras beyond the LDS).
inline bool ptm_point_order(const BlockArrays& B, const CompLists& C, int ncb, PtmDeal deal, int num_cus, size_t lds_limit, ivec& pts, ivec& deg,
                            ivec& wg_chunk0, std::vector<ivec>& local_cams, PtmLocalReport& rep) {
    const int npb = (int)pts.size(), m = C.m;
    // By number of factors, descending: the lanes of a wave run loops of equal length.  Among blocks of equal
    // count by their cameras, in listed order, lexicographically: neighbours in a wave-chunk then read the SAME
    // camera slots at the same time -- one LDS access serves them all, and the few distinct cameras of a chunk
    // are neighbours too, which keeps them on different banks (random cameras: 54 % of the LDS cycles were bank
    // conflicts, profiles/r03_a_pmc_lds_synthL.txt).  Ties: ascending id.
    std::sort(pts.begin(), pts.end());
    number_blocks(B, pts);
    deg.assign((size_t)npb + 1, 0);
    for (int j = 0; j < m; ++j) ++deg[(size_t)B.blk_idx[(size_t)B.pt[(size_t)C.fac_id[j]]] + 1];
    for (int k = 0; k < npb; ++k) deg[(size_t)k + 1] += deg[(size_t)k];   // (now a CSR over the blocks in id order)
    ivec pcam((size_t)m), fill(deg.begin(), deg.end() - 1);
    for (int j = 0; j < m; ++j) {
        const int f = C.fac_id[j];
        // (camera numbers within the component: blk_idx of the camera blocks was set by the caller and is still valid for them)
        pcam[(size_t)fill[(size_t)B.blk_idx[(size_t)B.pt[(size_t)f]]]++] = B.blk_idx[(size_t)B.cam[(size_t)f]];
    }
    ivec ord((size_t)npb);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int a, int b) {
        const int da = deg[(size_t)a + 1] - deg[(size_t)a], db = deg[(size_t)b + 1] - deg[(size_t)b];
        if (da != db) return da > db;
        const int* pa = pcam.data() + deg[(size_t)a];
        const int* pb = pcam.data() + deg[(size_t)b];
        for (int t = 0; t < da; ++t) if (pa[t] != pb[t]) return pa[t] < pb[t];
        return a < b;
    });
    // Whole wave-chunks of equal slot count are then dealt out over PTM_SPREAD runs of the sorted order: the chunks
    // that the waves of a workgroup evaluate at the same time come from different runs and meet different cameras
    // (the gradient's round sums, solver_ptm.hpp, are as long as a round's longest camera segment).
    const int nfull = npb / 64, npc_all = (npb + 63) / 64;
    auto slots_of = [&](int a) { return deg[(size_t)ord[(size_t)(64 * a)] + 1] - deg[(size_t)ord[(size_t)(64 * a)]]; };
    auto for_each_run = [&](auto&& body) {   // body(a0, a1): the full chunks [a0, a1) have equal slot count
        for (int a0 = 0; a0 < nfull;) {
            const int T = slots_of(a0);
            int a1 = a0;
            while (a1 < nfull && slots_of(a1) == T) ++a1;
            body(a0, a1);
            a0 = a1;
        }
    };
    ivec chunk_of((size_t)nfull);   // position in the order -> chunk of the sorted order
    bool fits = true;
    if (deal == PtmDeal::LOCAL) {
        // LOCAL: workgroup r owns a CONTIGUOUS slice of every run of chunks of equal slot count (the runs stand in
        // camera order: a slice meets few cameras; a slice of every run: equal work), its positions in the chunk order
        // are consecutive ([wg_chunk0[r], wg_chunk0[r + 1])), and inside them wave w (position - first mod 8) takes a
        // contiguous eighth of the workgroup's chunks: the waves of a workgroup meet different cameras at a time
        const int Kl = (int)std::min<int64_t>(std::min<int64_t>(num_cus, PTM_WIDE_MAX_GROUP), std::max<int64_t>(1, npc_all / 24));
        if (Kl <= PTM_MAX_GROUP) return false;
        std::vector<ivec> wl((size_t)Kl);
        for_each_run([&](int a0, int a1) {
            const long long mm = a1 - a0;
            for (int rk = 0; rk < Kl; ++rk)
                for (long long a = a0 + rk * mm / Kl; a < a0 + (rk + 1) * mm / Kl; ++a) wl[(size_t)rk].push_back((int)a);
        });
        wg_chunk0.assign((size_t)Kl + 1, 0);
        int pos = 0;
        for (int rk = 0; rk < Kl; ++rk) {
            const ivec& li = wl[(size_t)rk];
            const int nr = (int)li.size(), nwv = PTM_WIDE_THREADS / 64;
            wg_chunk0[(size_t)rk] = pos;
            int taken = 0;
            for (int w = 0; w < nwv; ++w) {   // wave w's positions: first + w, first + w + 8, ... -- the next (nr - w + 7) / 8 chunks of the list
                const int cnt = nr > w ? (nr - w + nwv - 1) / nwv : 0;
                for (int j = 0; j < cnt; ++j) chunk_of[(size_t)(pos + w + nwv * j)] = li[(size_t)(taken + j)];
                taken += cnt;
            }
            pos += nr;
        }
        wg_chunk0[(size_t)Kl] = npc_all;   // (the last workgroup also takes the chunk of the npb % 64 blocks left over)
    } else {
        int pos = 0;
        for_each_run([&](int a0, int a1) {
            const int mm = a1 - a0, q = (mm + PTM_SPREAD - 1) / PTM_SPREAD;
            if (deal == PtmDeal::SPREAD) {
                for (int rr = 0; rr < q; ++rr)
                    for (int gg = 0; gg < PTM_SPREAD; ++gg) { const int idx = gg * q + rr; if (idx < mm) chunk_of[(size_t)pos++] = a0 + idx; }
            } else {
                // A wide group deals chunk c to workgroup c mod K, wave (c / K) mod waves -- with K a multiple of
                // PTM_SPREAD the round robin above would hand all the waves of a workgroup neighbours of ONE run, i.e.
                // one camera: a gradient round's sums (one lane per camera entry, solver_ptm.hpp) 512 rows long, 22 000
                // of a round's 26 000 cycles at 8e6 factors.  Here position c takes the next chunk of run h(c), h a
                // weighted sum of c's hexadecimal digits mod 16: the positions c, c + K, c + 2 K, ... of a workgroup's
                // waves meet different runs for every K that occurs (searched over K = 1 .. 16, 32 .. 512).
                int used[PTM_SPREAD] = {};
                for (int t = 0; t < mm; ++t) {
                    int gg = ((pos & 15) + 15 * ((pos >> 4) & 15) + ((pos >> 8) & 15) + 15 * ((pos >> 12) & 15) + ((pos >> 16) & 15) + ((pos >> 20) & 15)) % PTM_SPREAD;
                    for (int tries = 0; tries < PTM_SPREAD && gg * q + used[gg] >= std::min(mm, (gg + 1) * q); ++tries) gg = (gg + 1) % PTM_SPREAD;
                    chunk_of[(size_t)pos++] = a0 + gg * q + used[gg]++;
                }
            }
        });
    }
    {
        ivec ord2(ord);
        for (int a = 0; a < nfull; ++a)
            for (int l = 0; l < 64; ++l) ord2[(size_t)(64 * a + l)] = ord[(size_t)(64 * chunk_of[(size_t)a] + l)];
        ord.swap(ord2);
    }
    if (deal == PtmDeal::LOCAL) {   // every workgroup's cameras
        const int Kl = (int)wg_chunk0.size() - 1;
        local_cams.assign((size_t)Kl, ivec());
        const size_t cam_cap = [&] { size_t k = 1; while (k < 255 && ptm_bytes_for((int)k + 1, PTM_WIDE_THREADS) <= lds_limit) ++k; return k; }();
        ivec mark((size_t)ncb, -1);
        size_t worst = 0;
        for (int rk = 0; rk < Kl && fits; ++rk) {
            ivec& lc = local_cams[(size_t)rk];
            for (int k = 64 * wg_chunk0[(size_t)rk]; k < std::min(npb, 64 * wg_chunk0[(size_t)rk + 1]); ++k) {
                const int a = ord[(size_t)k];
                for (int t = deg[(size_t)a]; t < deg[(size_t)a + 1]; ++t)
                    if (mark[(size_t)pcam[(size_t)t]] != rk) { mark[(size_t)pcam[(size_t)t]] = rk; lc.push_back(pcam[(size_t)t]); }
            }
            std::sort(lc.begin(), lc.end());
            if (lc.empty()) lc.push_back(0);   // (a workgroup without chunks still has its LDS laid out for one camera)
            worst = std::max(worst, lc.size());
            if (lc.size() > cam_cap) fits = false;
        }
        rep.dealt = true; rep.K = Kl; rep.chunks = npc_all; rep.worst = worst; rep.cam_cap = cam_cap;
        if (!fits) return false;
    }
    ivec pts2((size_t)npb);
    for (int k = 0; k < npb; ++k) pts2[(size_t)k] = pts[(size_t)ord[(size_t)k]];
    pts.swap(pts2);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// slot tables

// A component's slot table: camera blocks (`cams`, ascending), then point blocks (`pts`, in slot order).  sv / sf: a slot's
// variable id and local free index (-1: a constant); fidx / pidx [m]: a listed factor's slot word (camera | point << 12)
// and its point block's number, all 31 bits of it.  ptm (the streaming solver): ten slots per camera block, and
// pptr: the point's factors, in listed order (a CSR over the point blocks in their slot order).
inline void slot_table(const BlockArrays& B, const CompLists& C, int stamp, const ivec& cams, const ivec& pts, bool ptm,
                       ivec& sv, ivec& sf, int* fidx, int* pidx, ivec& pptr) {
    const int ncb = (int)cams.size(), npb = (int)pts.size(), ns = 9 * ncb + 3 * npb;
    number_blocks(B, pts);
    // local free index of the component's variables (the per-problem arrays are valid for one stamp)
    for (int i = 0; i < C.n; ++i) { const int v = C.free_vid[i]; B.owner_stamp[(size_t)v] = stamp; B.local[(size_t)v] = i; }
    sv.reserve((size_t)ns); sf.reserve((size_t)ns);
    auto slot = [&](int v) { sv.push_back(v); sf.push_back(B.owner_stamp[(size_t)v] == stamp ? B.local[(size_t)v] : -1); };
    if (!ptm) { for (int b : cams) for (int k = 0; k < 9; ++k) slot(b + k); }
    else {   // the streaming solver's camera slots: ten per block, [t f k1 k2 | r | pad] (ptm_api.hpp)
        for (int b : cams)
            for (int q = 0; q < PTM_CS; ++q) {
                const int k = ptm_var_of(q);
                if (k >= 0) slot(b + k); else { sv.push_back(b); sf.push_back(-1); }
            }
    }
    for (int b : pts) for (int k = 0; k < 3; ++k) slot(b + k);
    for (int j = 0; j < C.m; ++j) {
        const int f = C.fac_id[j];
        fidx[j] = (int)((unsigned)B.blk_idx[(size_t)B.cam[(size_t)f]] | ((unsigned)B.blk_idx[(size_t)B.pt[(size_t)f]] << 12));
        pidx[j] = B.blk_idx[(size_t)B.pt[(size_t)f]];
    }
    if (ptm) {
        pptr.assign((size_t)npb + 1, 0);
        for (int j = 0; j < C.m; ++j) ++pptr[(size_t)pidx[j] + 1];
        for (int k = 0; k < npb; ++k) pptr[(size_t)k + 1] += pptr[(size_t)k];
    }
}

// Point-major factor order of one streaming component, appended to pm_jg and cptr.  A component's point blocks stand in
// slot order (by number of factors, descending) and are taken 64 at a time -- a wave-chunk, a lane per block.  The
// factors of a chunk's blocks are laid out slot-major: entry cptr[chunk] + 64 t + lane is the t-th listed
// factor of the lane's block (or no factor: -1), so a wave's loads of a slot are 64 neighbours and their
// addresses depend on nothing the wave has loaded before.  entry -> listed factor (plan-wide index: c0 + place in the list).
// cbase [chunks + 1]: the chunks' first entries within the component.
inline void ptm_factor_stream(int c0, int m, const int* pidx, const ivec& pptr, ivec& pm_jg, ivec& cptr, ivec& cbase) {
    const int npb = (int)pptr.size() - 1, npc = (npb + 63) / 64;
    const int e0 = (int)pm_jg.size();
    cbase.assign((size_t)npc + 1, 0);
    for (int ch = 0; ch < npc; ++ch)   // (descending: a chunk's first block has the most factors)
        cbase[(size_t)ch + 1] = cbase[(size_t)ch] + 64 * (pptr[(size_t)(64 * ch) + 1] - pptr[(size_t)(64 * ch)]);
    pm_jg.resize((size_t)e0 + (size_t)cbase[(size_t)npc], -1);
    ivec fill((size_t)npb, 0);
    for (int j = 0; j < m; ++j) {
        const int pi = pidx[j];
        const int e = e0 + cbase[(size_t)(pi / 64)] + 64 * fill[(size_t)pi]++ + (pi % 64);
        pm_jg[(size_t)e] = c0 + j;
    }
    for (int k = 0; k <= npc; ++k) cptr.push_back(e0 + cbase[(size_t)k]);
}

// the tables of the local group (ptm_api.hpp: PtmGroupArgs)
struct PtmLocalTables {
    ivec lc, cr_ptr, cr, wg_chunk0;     // PtmGroupArgs' tables; the workgroups' chunk ranges
    std::vector<long long> lc_off;
    std::vector<short> pm_lcam;         // entry of the point-major order -> its camera's number in the owning workgroup
    void clear() { lc.clear(); cr_ptr.clear(); cr.clear(); wg_chunk0.clear(); lc_off.clear(); pm_lcam.clear(); }
};
// ... per workgroup its cameras and chunk range, per entry of the factor stream the camera's number in the workgroup that owns
// the chunk, per component camera who holds it.  e0: the component's first entry of pm_jg; fidx: plan-wide; T.wg_chunk0 is set.
inline void ptm_local_tables(int ncbg, const std::vector<ivec>& local_cams, const ivec& cbase, int e0, const ivec& pm_jg, const int* fidx, PtmLocalTables& T) {
    const int Kl = (int)local_cams.size(), npc = (int)cbase.size() - 1;
    T.pm_lcam.assign((size_t)cbase[(size_t)npc] + 64 * PTM_BLK, (short)-1);
    T.lc_off.assign((size_t)Kl, 0);
    std::vector<ivec> holders((size_t)ncbg);
    ivec g2l((size_t)ncbg, -1);
    for (int rk = 0; rk < Kl; ++rk) {
        const ivec& lc = local_cams[(size_t)rk];
        for (size_t k = 0; k < lc.size(); ++k) g2l[(size_t)lc[k]] = (int)k;
        T.lc_off[(size_t)rk] = (long long)T.lc.size();
        T.lc.push_back((int)lc.size()); T.lc.push_back(T.wg_chunk0[(size_t)rk]); T.lc.push_back(T.wg_chunk0[(size_t)rk + 1]); T.lc.push_back(0);
        T.lc.insert(T.lc.end(), lc.begin(), lc.end());
        for (size_t k = 0; k < lc.size(); ++k) {   // (the first workgroup that holds a camera speaks for it)
            T.lc.push_back(holders[(size_t)lc[k]].empty() ? 1 : 0);
            holders[(size_t)lc[k]].push_back((rk << 8) | (int)k);
        }
        for (int e = cbase[(size_t)T.wg_chunk0[(size_t)rk]]; e < cbase[(size_t)T.wg_chunk0[(size_t)rk + 1]]; ++e) {
            const int j = pm_jg[(size_t)(e0 + e)];
            if (j >= 0) T.pm_lcam[(size_t)e] = (short)g2l[(size_t)(((unsigned)fidx[(size_t)j]) & 0xFFFu)];
        }
    }
    T.cr_ptr.assign(1, 0);
    for (int g = 0; g < ncbg; ++g) {
        T.cr.insert(T.cr.end(), holders[(size_t)g].begin(), holders[(size_t)g].end());
        T.cr_ptr.push_back((int)T.cr.size());
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the streaming solver's work tables, for workgroups of `threads` lanes, K to a component

// the plan's point-major host tables as the two builders below read them
struct PtmStreamTables {
    int64_t ncomp = 0, pm_entries = 0;
    const int* comps = nullptr; size_t ncomps = 0;   // the streaming components, in launch order
    const int *ls_ptr = nullptr, *ls_ncb = nullptr, *ls_fidx = nullptr, *pm_ch0 = nullptr, *cptr = nullptr, *jg = nullptr;
    int local_comp = -1;                 // the component of the local group, -1 = none
    const PtmLocalTables* local = nullptr;
};

// A trial's work by wave (solver_ptm.hpp: eval_line): the workgroup's wave-chunks cut into blocks of
// PTM_BLK slots, the blocks in chunk order dealt out in equal CONTIGUOUS shares -- a wave's share is a run of whole chunks
// with at most a partial one at either end (a chunk's 64 point blocks times some of their slots).  By whole chunks 41 of them
// over 12 waves are four for some and three for the rest, and a trial waits for the slowest.
// rows: per workgroup its number of rows R, 0, 0, 0, then three planes of R ints; off [ncomp K]: where a workgroup's start.
inline void ptm_segment_rows(const PtmStreamTables& T, int threads, int K, ivec& rows, std::vector<long long>& off) {
    const int nw = threads / 64;
    off.assign((size_t)T.ncomp * (size_t)K, 0);
    rows.clear();
    std::vector<ivec> share((size_t)nw);
    for (size_t ri = 0; ri < T.ncomps; ++ri) {
        const int cc = T.comps[ri];
        const int ncb = T.ls_ncb[cc], ns = T.ls_ptr[cc + 1] - T.ls_ptr[cc], npb = (ns - PTM_CS * ncb) / 3, npc = (npb + 63) / 64;
        const int* cp = T.cptr + T.pm_ch0[cc];
        const bool local = T.local_comp == cc;   // (a workgroup's chunks: consecutive ones instead of every K-th)
        for (int rk = 0; rk < K; ++rk) {
            const int ch0 = local ? T.local->wg_chunk0[(size_t)rk] : rk, chend = local ? T.local->wg_chunk0[(size_t)rk + 1] : npc, chstep = local ? 1 : K;
            long long units = 0;
            for (int ch = ch0; ch < chend; ch += chstep) units += ((cp[ch + 1] - cp[ch]) / 64 + PTM_BLK - 1) / PTM_BLK;
            size_t depth = 0;
            long long u = 0;   // blocks dealt out so far
            int ch = ch0, done = 0;   // the chunk at hand and its blocks already dealt out
            for (int w = 0; w < nw; ++w) {
                ivec& sh = share[(size_t)w];
                sh.clear();
                const long long end = units * (w + 1) / nw;
                while (u < end) {
                    const int nb = ((cp[ch + 1] - cp[ch]) / 64 + PTM_BLK - 1) / PTM_BLK;
                    if (done >= nb) { ch += chstep; done = 0; continue; }
                    const int take = (int)std::min<long long>(nb - done, end - u);
                    const int e0 = cp[ch] + 64 * PTM_BLK * done, e1 = std::min(cp[ch + 1], e0 + 64 * PTM_BLK * take);
                    sh.push_back(ch); sh.push_back(e0); sh.push_back(e1); sh.push_back(0);
                    done += take; u += take;
                }
                depth = std::max(depth, sh.size() / 4);
            }
            // (two rows of nothing behind every wave's last: the loop asks for its rows two ahead)
            // (and at least one row of work: a rank with no chunks still has the three rows a wave reads up front)
            const size_t base = rows.size(), R = (std::max<size_t>(depth, 1) + 2) * (size_t)nw;
            off[(size_t)cc * K + rk] = (long long)base;
            rows.resize(base + 4 + 3 * R, 0);
            rows[base] = (int)R;
            for (int w = 0; w < nw; ++w)
                for (size_t k = 0; k < share[(size_t)w].size() / 4; ++k)
                    for (size_t q = 0; q < 3; ++q) rows[base + 4 + q * R + k * (size_t)nw + (size_t)w] = share[(size_t)w][4 * k + q];
        }
    }
}

// The gradient's rounds (solver_ptm.hpp: gradient_to_xi), rs slots staged a round.  Workgroup (component, rank r) takes the
// point chunks c = r (mod K), its wave w those with (c / K) mod waves = w, slot by slot: that is the wave's sequence of steps,
// and round rr of the workgroup is every wave's rr-th step.  Within a round the factors are ranked by camera block (within a
// camera by wave and lane): a factor's rank is the staging row of its camera partials (grow, two bytes per factor), and a
// round's table names per camera the first row of its segment [ncb + 1] -- the order of the sums.
// tab: the round tables, ptm_round_stride(ncb) words each; off / nr [ncomp K]: a workgroup's first table and its rounds.
inline void ptm_round_tables(const PtmStreamTables& T, int threads, int K, int rs, std::vector<unsigned short>& tab, std::vector<unsigned short>& grow,
                             std::vector<long long>& off, ivec& nr) {
    const int nw = threads / 64;
    const unsigned* fidx = reinterpret_cast<const unsigned*>(T.ls_fidx);
    const int* jg = T.jg;
    const size_t nwg = (size_t)T.ncomp * (size_t)K;
    off.assign(nwg, 0);
    nr.assign(nwg, 0);
    tab.clear();
    grow.assign((size_t)T.pm_entries + 64 * PTM_BLK, 0);
    std::vector<ivec> steps((size_t)nw), step_slots((size_t)nw);
    ivec seg, pos;
    for (size_t ri = 0; ri < T.ncomps; ++ri) {
        const int cc = T.comps[ri];
        const int ncb_all = T.ls_ncb[cc], ns = T.ls_ptr[cc + 1] - T.ls_ptr[cc], npb = (ns - PTM_CS * ncb_all) / 3, npc = (npb + 63) / 64;
        const int* cp = T.cptr + T.pm_ch0[cc];
        const bool local = T.local_comp == cc;
        for (int rk = 0; rk < K; ++rk) {
            // (a local group: the workgroup's own cameras, under its own numbers; its chunks consecutive, wave w every eighth from the w-th on)
            const int ncb = local ? T.local->lc[(size_t)T.local->lc_off[(size_t)rk]] : ncb_all;
            const size_t stride = (size_t)ptm_round_stride(ncb);
            auto cam_of = [&](int e, int j) { return local ? (int)T.local->pm_lcam[(size_t)e] : (int)(fidx[j] & 0xFFFu); };   // (an entry's camera as the stream names it)
            size_t nrounds = 0;
            for (int w = 0; w < nw; ++w) {
                ivec& st = steps[(size_t)w];
                ivec& sn = step_slots[(size_t)w];
                st.clear(); sn.clear();
                const int ch0 = local ? T.local->wg_chunk0[(size_t)rk] + w : rk + K * w, chend = local ? T.local->wg_chunk0[(size_t)rk + 1] : npc, chstep = local ? nw : K * nw;
                // (a step: one slot of a chunk, or -- two slots a round -- a block of up to two of ONE chunk)
                for (int ch = ch0; ch < chend; ch += chstep)
                    for (int e = cp[ch]; e < cp[ch + 1]; e += 64 * rs) { st.push_back(e); sn.push_back(std::min(rs, (cp[ch + 1] - e) / 64)); }
                nrounds = std::max(nrounds, st.size());
            }
            const size_t base = tab.size();
            off[(size_t)cc * K + rk] = (long long)base;
            nr[(size_t)cc * K + rk] = (int)nrounds;
            tab.resize(base + nrounds * stride, 0);
            for (size_t rr = 0; rr < nrounds; ++rr) {
                unsigned short* rec = tab.data() + base + rr * stride;
                seg.assign((size_t)ncb + 1, 0);
                for (int w = 0; w < nw; ++w) {
                    if (rr >= steps[(size_t)w].size()) continue;
                    const int e = steps[(size_t)w][rr];
                    for (int l = 0; l < 64 * step_slots[(size_t)w][rr]; ++l) { const int j = jg[e + l]; if (j >= 0) ++seg[(size_t)cam_of(e + l, j) + 1]; }
                }
                for (int k = 0; k < ncb; ++k) seg[(size_t)k + 1] += seg[(size_t)k];
                for (int k = 0; k <= ncb; ++k) rec[k] = (unsigned short)seg[(size_t)k];
                pos.assign(seg.begin(), seg.end() - 1);
                // (within a camera: the round's first slots by wave and lane, then its second slots -- with every chunk an even number of
                // slots long that is the order of one slot a round)
                for (int sl = 0; sl < rs; ++sl)
                    for (int w = 0; w < nw; ++w) {
                        if (rr >= steps[(size_t)w].size() || sl >= step_slots[(size_t)w][rr]) continue;
                        const int e = steps[(size_t)w][rr] + 64 * sl;
                        for (int l = 0; l < 64; ++l) {
                            const int j = jg[e + l];
                            if (j >= 0) grow[(size_t)(e + l)] = (unsigned short)pos[(size_t)cam_of(e + l, j)]++;
                        }
                    }
            }
        }
    }
}

}  // namespace rdis_hip
