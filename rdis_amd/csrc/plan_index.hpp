// plan_index.hpp -- the index a plan is created from: the caller's component lists (two CSRs of int64 ids) checked for
// independence and turned into the plan's int32 tables -- free and factor lists, the variable-major positions of every listed
// factor slot's partial (v2s_ptr, slot_base, slot_pos), the slots' component-local indices (h_slot_li), the heaviest-first order
// and the per-component camera-block tables (cb_ptr, cb, cb_li) -- packed into the one int32 block a plan uploads.  Every
// address a solver reads follows these tables.  Pure integer work over plain arrays: no HIP call, no plan, no context, no
// environment (rdis_hip.hip's plan_create_impl calls it, allocates and uploads); tests/cpp/plan_index_test.cpp runs it without a
// device against tests/test_plan_index_cpu.py's restatement.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>
#include "host_blocks.hpp"

namespace rdis_hip {

// include/rdis_hip.h's codes and device_views.hpp's kind, restated (rdis_hip.hip asserts each equal to its original)
constexpr int PLAN_INDEX_EINVAL = -1, PLAN_INDEX_EOVERLAP = -4, PLAN_INDEX_ERANGE = -5;
constexpr int PLAN_INDEX_KIND_BA = 0;

// plan_index_build's view of a variable: free in which component, where in the free list (valid for one stamp)
struct VarMark { int stamp, owner, gidx, pad; };

// what plan_index_build needs of a problem: its host arrays, and scratch that is valid for one stamp
struct IndexArrays {
    int kind;                // PLAN_INDEX_KIND_BA: twelve slots a factor (cam, pt); else rowptr / vid
    int64_t N, F;            // variables, factors
    const int* cam;          // [F] a factor's camera block (the id of its first variable)
    const int* pt;           // [F] ... and point block
    const int* rowptr;       // [F + 1] CSR of a nonlinear-product factor's variables
    const int* vid;
    const int* block_of;     // [N] the camera block a variable belongs to, -1 = none
    int64_t ncam_blocks;     // 0: no camera-block tables
    VarMark* mark;           // [N] scratch
    int* fac_stamp;          // [F] scratch: factor listed
    int stamp;               // a value no earlier call on this scratch used

    int arity(int f) const { return kind == PLAN_INDEX_KIND_BA ? 12 : rowptr[f + 1] - rowptr[f]; }
    int var_of(int f, int k) const { return vid[rowptr[f] + k]; }   // (nonlinear products)
};

// what plan_index_build produces and a plan keeps
struct PlanIndex {
    int64_t nslots = 0, ngfac = 0;
    // one device block of int32, `ints` (order | free_ptr | free_vid | fac_ptr | fac_id | v2s_ptr | slot_base | slot_pos |
    // cb_ptr | cb | cb_li)
    size_t off_order = 0, off_free_ptr = 0, off_free_vid = 0, off_fac_ptr = 0, off_fac_id = 0, off_v2s_ptr = 0,
           off_slot_base = 0, off_slot_pos = 0;
    size_t off_cb_ptr = 0, off_cb = 0, off_cb_li = 0;
    ivec h_blk;   // host image of `ints` (kept alive: its upload is asynchronous)
    ivec h_order, h_fac_ptr, h_free_ptr, h_free_vid, h_fac_id, h_v2s_ptr;
    ivec h_slot_li;           // [nslots] per listed factor slot: index of its variable within its component, -1 = constant (may be dropped: plan_index_build)
};

// What can be refused before anything else is touched: 0, or a code with *msg.  free_ptr and fac_ptr are not null.
inline int plan_index_check(int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid, const int64_t* fac_ptr,
                            const int64_t* fac_id, std::string* msg) {
    const int64_t nfree = free_ptr[ncomp], nfac = fac_ptr[ncomp];
    if (free_ptr[0] != 0 || fac_ptr[0] != 0 || nfree < 0 || nfac < 0 || (nfree && !free_vid) || (nfac && !fac_id)) {
        *msg = "plan_create: bad CSR";
        return PLAN_INDEX_EINVAL;
    }
    if (nfree >= (1ll << 31) / 5 || nfac >= ((1ll << 31) - 16) / 12) { *msg = "plan_create: too large"; return PLAN_INDEX_ERANGE; }
    return 0;
}

// The tables of lists that passed plan_index_check, written into X: 0, or a code with *msg (X is then half written).
inline int plan_index_build(const IndexArrays& P, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid,
                            const int64_t* fac_ptr, const int64_t* fac_id, PlanIndex& X, std::string* msg) {
    const int64_t nfree = free_ptr[ncomp], nfac = fac_ptr[ncomp];
    auto refuse = [&](int code, std::string m) { *msg = std::move(m); return code; };   // (called on a refusing path only)

    // --- validate independence (free sets disjoint, factors owned once, no factor of one
    // component reading a free variable of another); the marks are a persistent per-problem
    // array validated by a stamp, so a call costs O(its own size), not O(N)
    const int stamp = P.stamp;
    VarMark* const mark = P.mark;
    X.h_free_ptr.resize((size_t)ncomp + 1); X.h_fac_ptr.resize((size_t)ncomp + 1);
    X.h_free_vid.resize((size_t)nfree); X.h_fac_id.resize((size_t)nfac);
    for (int64_t cc = 0; cc <= ncomp; ++cc) {
        if (cc && (free_ptr[cc] < free_ptr[cc - 1] || fac_ptr[cc] < fac_ptr[cc - 1]))
            return refuse(PLAN_INDEX_EINVAL, "plan_create: ptr not monotone");
        X.h_free_ptr[(size_t)cc] = (int)free_ptr[cc];
        X.h_fac_ptr[(size_t)cc] = (int)fac_ptr[cc];
    }
    for (int64_t cc = 0; cc < ncomp; ++cc)
        for (int64_t i = free_ptr[cc]; i < free_ptr[cc + 1]; ++i) {
            const int64_t v = free_vid[i];
            if (v < 0 || v >= P.N) return refuse(PLAN_INDEX_EINVAL, "plan_create: free variable id out of range");
            VarMark& mk = mark[(size_t)v];
            if (mk.stamp == stamp) return refuse(PLAN_INDEX_EOVERLAP, "plan_create: variable " + std::to_string(v) + " is free in two components (or listed twice)");
            mk.stamp = stamp; mk.owner = (int)cc; mk.gidx = (int)i;
            X.h_free_vid[(size_t)i] = (int)v;
        }
    // One pass over the listed factors' slots leaves, per slot, the position of its variable in the
    // plan's free list (-1: a constant for this solve) and counts the slots per variable; a second,
    // sequential one turns that into the variable-major position of the slot's partial (slot_pos) and
    // the variable's index within its component (h_slot_li: what the cooperative layouts address by).
    ivec& v2s_ptr = X.h_v2s_ptr;
    v2s_ptr.assign((size_t)nfree + 1, 0);
    ivec slot_base((size_t)nfac + 1);
    slot_base[0] = 0;
    int* const fid32 = X.h_fac_id.data();
    int* const cnt = v2s_ptr.data() + 1;
    const bool ba = P.kind == PLAN_INDEX_KIND_BA;
    if (ba) X.nslots = 12 * nfac;
    else {
        int64_t ns = 0;
        for (int64_t j = 0; j < nfac; ++j) {
            const int64_t f = fac_id[j];
            if (f < 0 || f >= P.F) return refuse(PLAN_INDEX_EINVAL, "plan_create: factor id out of range");
            ns += P.arity((int)f);
        }
        if (ns >= (1ll << 31) - 16) return refuse(PLAN_INDEX_ERANGE, "plan_create: too large");
        X.nslots = ns;
    }
    ivec& sli = X.h_slot_li;
    sli.resize((size_t)X.nslots);
    int* const gi = sli.data();
    auto other_owner = [&](int64_t f, int64_t cc, int o) {
        return refuse(PLAN_INDEX_EOVERLAP, "plan_create: factor " + std::to_string(f) + " of component " + std::to_string(cc) + " reads a free variable of component " + std::to_string(o));
    };
    for (int64_t cc = 0; cc < ncomp; ++cc) {
        const int icc = (int)cc;
        for (int64_t j = fac_ptr[cc]; j < fac_ptr[cc + 1]; ++j) {
            const int64_t f = fac_id[j];
            if (f < 0 || f >= P.F) return refuse(PLAN_INDEX_EINVAL, "plan_create: factor id out of range");
            if (P.fac_stamp[(size_t)f] == stamp) return refuse(PLAN_INDEX_EOVERLAP, "plan_create: factor " + std::to_string(f) + " listed twice");
            P.fac_stamp[(size_t)f] = stamp;
            fid32[j] = (int)f;
            if (ba) {
                slot_base[(size_t)j + 1] = 12 * (int)(j + 1);
                int* g = gi + 12 * j;
                const VarMark* mc = mark + P.cam[(size_t)f];
                const VarMark* mp = mark + P.pt[(size_t)f];
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const VarMark& mk = k < 9 ? mc[k] : mp[k - 9];
                    int pos = -1;
                    if (mk.stamp == stamp) {
                        if (mk.owner != icc) return other_owner(f, cc, mk.owner);
                        pos = mk.gidx;
                        ++cnt[pos];
                    }
                    g[k] = pos;
                }
            } else {
                const int a = P.arity((int)f), sb = slot_base[(size_t)j];
                slot_base[(size_t)j + 1] = sb + a;
                for (int k = 0; k < a; ++k) {
                    const VarMark& mk = mark[(size_t)P.var_of((int)f, k)];
                    int pos = -1;
                    if (mk.stamp == stamp) {
                        if (mk.owner != icc) return other_owner(f, cc, mk.owner);
                        pos = mk.gidx;
                        ++cnt[pos];
                    }
                    gi[sb + k] = pos;
                }
            }
        }
    }
    for (int64_t i = 0; i < nfree; ++i) v2s_ptr[(size_t)i + 1] += v2s_ptr[(size_t)i];
    X.ngfac = v2s_ptr[(size_t)nfree];
    // heaviest components first (longest-processing-time order for the launch)
    X.h_order.resize((size_t)ncomp);
    std::iota(X.h_order.begin(), X.h_order.end(), 0);
    std::stable_sort(X.h_order.begin(), X.h_order.end(), [&](int a, int b) {
        return (fac_ptr[a + 1] - fac_ptr[a]) > (fac_ptr[b + 1] - fac_ptr[b]);
    });

    // --- one int32 block, one H2D copy
    ivec& blk = X.h_blk;
    blk.reserve((size_t)(4 * ncomp + 3 * nfree + 2 * nfac + X.nslots) + 64);
    auto put = [&](const ivec& v) { const size_t off = blk.size(); blk.insert(blk.end(), v.begin(), v.end()); return off; };
    X.off_order = put(X.h_order);
    X.off_free_ptr = put(X.h_free_ptr); X.off_free_vid = put(X.h_free_vid);
    X.off_fac_ptr = put(X.h_fac_ptr); X.off_fac_id = put(X.h_fac_id);
    X.off_v2s_ptr = put(v2s_ptr); X.off_slot_base = put(slot_base);
    {   // gfac is variable-major: slot_pos[s] = where listed factor slot s lands in it (-1: not free here),
        // the slots of a variable in listed order; the positions above become component-local indices
        X.off_slot_pos = blk.size();
        blk.resize(blk.size() + (size_t)X.nslots);
        int* const slot_pos = blk.data() + X.off_slot_pos;
        ivec fill(v2s_ptr.begin(), v2s_ptr.end() - 1);
        int* const fl = fill.data();
        for (int64_t cc = 0; cc < ncomp; ++cc) {
            const int f0 = (int)free_ptr[cc];
            const int64_t s0 = slot_base[(size_t)fac_ptr[cc]], s1 = slot_base[(size_t)fac_ptr[cc + 1]];
            for (int64_t s = s0; s < s1; ++s) {
                const int g = gi[s];
                slot_pos[s] = g >= 0 ? fl[g]++ : -1;
                gi[s] = g >= 0 ? g - f0 : -1;
            }
        }
    }
    // (the per-slot local indices serve prepare_partition's cooperative groups, bundle adjustment only; a plan
    // too large for them to matter does not keep them: prepare_partition then forms a group's indices itself)
    if (!ba || X.nslots > (64ll << 20)) { ivec().swap(X.h_slot_li); }
    {   // per component: the camera blocks with a free rotation variable (their records follow the trial
        // point) and where in the component's vectors their three rotation variables are (-1: constant)
        ivec cb_ptr((size_t)ncomp + 1, 0), cb, cb_li;
        if (P.kind == PLAN_INDEX_KIND_BA && P.ncam_blocks > 0) {
            std::vector<std::array<int, 3>> ent;   // (block, which of the three, local index)
            for (int64_t cc = 0; cc < ncomp; ++cc) {
                ent.clear();
                for (int64_t i = free_ptr[cc]; i < free_ptr[cc + 1]; ++i) {
                    const int v = X.h_free_vid[(size_t)i], b = P.block_of[(size_t)v];
                    if (b >= 0 && v - b < 3) ent.push_back({b, v - b, (int)(i - free_ptr[cc])});
                }
                std::sort(ent.begin(), ent.end());
                for (const auto& e : ent) {
                    if (cb.size() == (size_t)cb_ptr[(size_t)cc] || cb.back() != e[0]) {
                        cb.push_back(e[0]);
                        cb_li.insert(cb_li.end(), {-1, -1, -1});
                    }
                    cb_li[cb_li.size() - 3 + (size_t)e[1]] = e[2];
                }
                cb_ptr[(size_t)cc + 1] = (int)cb.size();
            }
        }
        for (int64_t cc = 0; cc < ncomp; ++cc) cb_ptr[(size_t)cc + 1] = std::max(cb_ptr[(size_t)cc + 1], cb_ptr[(size_t)cc]);
        X.off_cb_ptr = put(cb_ptr); X.off_cb = put(cb); X.off_cb_li = put(cb_li);
    }
    return 0;
}

}  // namespace rdis_hip
