// replica_layout.hpp -- the replicas of a many-member launch, described once: the five host entries that run a kernel with the
// member as the grid's second dimension (rdis_hip_plan_solve_starts, rdis_hip_plan_solve_population[_range],
// rdis_hip_population_eval and both forms of rdis_hip_population_eval_grad) give every member of a launch a replica of some
// per-solve arrays, in one buffer laid out [R][part 0] [R][part 1] ...  A ReplicaLayout names the parts and their bytes per
// member; the buffer's size, the members a budget allows and every pointer and stride the kernels are handed come from it.
// The Levenberg-Marquardt plan's solves (rdis_hip_lm_plan_solve, rdis_hip_lm_plan_solve_population) describe their two buffers the
// same way (lm_plan_layout) and split their members by the same rule; its multi-start solves (rdis_hip_lm_plan_solve_starts,
// rdis_hip_lm_plan_solve_starts_population) add a winners' row, best[ncomp] and a scratch row of x a start (lm_starts_layout).
// rdis_hip_plan_solve_population_cooperative adds a buffer for its cooperative launches (population_coop_layout) and bounds the
// members of a launch by the resident workgroups as well (coop_members_per_launch).
// Pure host functions: no HIP call, no plan, no population (tests/cpp/replica_layout_test.cpp runs them without a device).
#pragma once
#include <algorithm>
#include <cstdint>

namespace rdis_hip {

// An ordered list of parts, each with its bytes per member (a part of zero bytes is legal and takes no room; a negative count is
// taken as zero).  For R members part i lies at R * (the bytes of the parts before it): [R][part 0] [R][part 1] ...
struct ReplicaLayout {
    static constexpr int MAX_PARTS = 4;
    int nparts = 0;
    int64_t bytes[MAX_PARTS] = {0, 0, 0, 0};   // per member
    ReplicaLayout() = default;
    ReplicaLayout(int n, int64_t b0, int64_t b1 = 0, int64_t b2 = 0, int64_t b3 = 0) : nparts(n) {
        const int64_t b[MAX_PARTS] = {b0, b1, b2, b3};
        for (int i = 0; i < MAX_PARTS; ++i) bytes[i] = i < n ? std::max<int64_t>(b[i], 0) : 0;
    }
    int64_t member_bytes() const { return bytes[0] + bytes[1] + bytes[2] + bytes[3]; }
    int64_t total_bytes(int64_t R) const { return R * member_bytes(); }
    int64_t offset(int part, int64_t R) const {   // bytes from the buffer's base to part `part` of a launch of R members
        int64_t before = 0;
        for (int i = 0; i < part; ++i) before += bytes[i];
        return R * before;
    }
    long long doubles(int part) const { return bytes[part] / 8; }   // a member's stride in a part of doubles
    template <class T>
    T* at(void* base, int part, int64_t R) const { return reinterpret_cast<T*>(static_cast<char*>(base) + offset(part, R)); }
};

constexpr int64_t REPLICA_PT_REC = 6;     // ptm_api.hpp: PT_REC   (rdis_hip.hip asserts both equal)
constexpr int64_t GRAD_MEMBER_REC = 14;   // grad_fused.hpp: GRAD_REC

// ---- rdis_hip_plan_solve_starts ----
// ms_work: ws[5 nfree], gfac[ngfac] and, for the plain solver only, x[nvars]
enum { STARTS_WS = 0, STARTS_GFAC = 1, STARTS_X = 2 };
inline ReplicaLayout starts_work_layout(int64_t nfree, int64_t ngfac, bool plain, int64_t nvars) {
    return ReplicaLayout(3, 8 * 5 * nfree, 8 * ngfac, plain ? 8 * nvars : 0);
}
// ms_dir, a buffer of its own (zero between launches), of both solve entries: the plain solver's dir[nvars]
inline ReplicaLayout solve_dir_layout(bool plain, int64_t nvars) { return ReplicaLayout(1, plain ? 8 * nvars : 0); }

// ---- rdis_hip_plan_solve_population ----
// ms_work: ws and gfac where the LDS-resident or the plain solver has listed components (`listed`), the cameras' rotation
// records [nvars] where the tiny-component launch reads records (`tiny_records`)
enum { POPULATION_WS = 0, POPULATION_GFAC = 1, POPULATION_ROT = 2 };
inline ReplicaLayout population_work_layout(bool listed, int64_t nfree, int64_t ngfac, bool tiny_records, int64_t nvars) {
    return ReplicaLayout(3, listed ? 8 * 5 * nfree : 0, listed ? 8 * ngfac : 0, tiny_records ? 8 * nvars : 0);
}
// ms_ptm: the point-major solver's pm_rec, pm_gh and pm_bex -- six doubles a point block each -- and, behind the three planes of
// doubles, pm_cbox, eight floats per entry of pm_cptr.  A plan without point blocks has no such part.
enum { PTM_REPLICA_REC = 0, PTM_REPLICA_GH = 1, PTM_REPLICA_BEX = 2, PTM_REPLICA_CBOX = 3 };
inline ReplicaLayout population_ptm_layout(int64_t pm_blocks, int64_t pm_cptr_len) {
    const int64_t plane = 8 * REPLICA_PT_REC * pm_blocks;
    return pm_blocks > 0 ? ReplicaLayout(4, plane, plane, plane, 4 * 8 * pm_cptr_len) : ReplicaLayout(4, 0);
}

// ms_coop, a buffer of its own, of rdis_hip_plan_solve_population_cooperative (solver_coop_population.hpp): the cooperative
// solver's gfac[ngfac], the groups' published directions (xi_doubles: the free variables of the plan's cooperative components,
// each group at its offset in the plan's xi_glob) and one exchange state (state_bytes: sizeof CoopState) for each of `groups`
// groups -- the most a launch of the plan has.  The two parts of doubles are padded to whole 32 bytes a member (a member's
// stride is doubles(part), not the count), so that every state lies on the 32 bytes its granule pairs ask for whatever R is
// (state_bytes is a multiple of 32).  A plan without cooperative components has no such part.
enum { COOP_REPLICA_GFAC = 0, COOP_REPLICA_XI = 1, COOP_REPLICA_STATE = 2 };
inline ReplicaLayout population_coop_layout(int64_t ngfac, int64_t xi_doubles, int64_t groups, int64_t state_bytes) {
    const auto pad = [](int64_t doubles) { return (8 * std::max<int64_t>(doubles, 0) + 31) / 32 * 32; };
    return groups > 0 ? ReplicaLayout(3, pad(ngfac), pad(xi_doubles), groups * state_bytes) : ReplicaLayout(3, 0);
}

// ---- rdis_hip_population_eval ----
// two buffers of one part each, charged to the budget together: eval_partial, a member's chunk or block sums (a count of zero
// allocates one), and eval_xr, its rotation records [nvars] where the launch reads records
inline ReplicaLayout population_eval_partial_layout(int64_t partials_per_member) { return ReplicaLayout(1, 8 * std::max<int64_t>(partials_per_member, 1)); }
inline ReplicaLayout population_eval_xr_layout(bool records, int64_t nvars) { return ReplicaLayout(1, records ? 8 * nvars : 0); }

// ---- rdis_hip_population_eval_grad ----
// grad_ws on the fused branch: the member's camera records (GRAD_MEMBER_REC doubles a camera block), the list's camera and point
// staging arrays (9 and 3 doubles a slot) and its chunk sums -- a count of zero allocates one, as the list's own arrays do
enum { GRAD_FUSED_CAMREC = 0, GRAD_FUSED_CSTAGE = 1, GRAD_FUSED_PSTAGE = 2, GRAD_FUSED_PARTIAL = 3 };
inline ReplicaLayout population_grad_fused_layout(int64_t ncam_blocks, int64_t cstage_slots, int64_t pstage_slots, int64_t nchunks) {
    const auto one = [](int64_t v) { return std::max<int64_t>(v, 1); };
    return ReplicaLayout(4, 8 * GRAD_MEMBER_REC * ncam_blocks, 8 * 9 * one(cstage_slots), 8 * 3 * one(pstage_slots), 8 * one(nchunks));
}
// grad_ws on the short and the two-pass branch: the per-factor partials gfac[nslots] and the value partials (short: the one
// chunk's sum, partials = 1; two-pass: the blocks' sums)
enum { GRAD_LIST_GFAC = 0, GRAD_LIST_PARTIAL = 1 };
inline ReplicaLayout population_grad_list_layout(int64_t nslots, int64_t partials) {
    return ReplicaLayout(2, 8 * nslots, 8 * std::max<int64_t>(partials, 1));
}

// ---- rdis_hip_lm_plan_solve, rdis_hip_lm_plan_solve_population ----
// two buffers.  `out`, for every member of the solve (kept until fetched): a result row of res_doubles doubles a component,
// hist_cap history records of four doubles a component, and the member's clamped results x[nfree] in free-list order.  `work`,
// for the members of one launch only -- the one the budget (the plan option workspace_bytes) is charged with: the components'
// workspace slices, ws_doubles doubles in all.
enum { LM_PLAN_RES = 0, LM_PLAN_HIST = 1, LM_PLAN_X = 2 };
enum { LM_PLAN_WS = 0 };
struct LmPlanLayout { ReplicaLayout out, work; };
inline LmPlanLayout lm_plan_layout(int64_t ncomp, int64_t res_doubles, int64_t hist_cap, int64_t nfree, int64_t ws_doubles) {
    return LmPlanLayout{ReplicaLayout(3, 8 * res_doubles * ncomp, 8 * 4 * hist_cap * ncomp, 8 * nfree), ReplicaLayout(1, 8 * ws_doubles)};
}

// ---- rdis_hip_lm_plan_solve_starts, rdis_hip_lm_plan_solve_starts_population ----
// The same two buffers for a solve of nstarts starts.  `out` has nstarts + 1 rows of lm_plan_layout's three fields: row s < nstarts
// is start s's, row nstarts the winners' (per component the row of its best start: the plan's ordinary outputs after such a
// solve); behind the rows best[ncomp] (int32, padded to 8 bytes).  `work` charges a start of a launch its workspace slices and its
// scratch row of x (N doubles: the free variables from the start, everything else the problem's x).
enum { LM_STARTS_WS = 0, LM_STARTS_ROWS = 1 };
struct LmStartsLayout {
    ReplicaLayout out, work;
    int64_t ncomp = 0;
    int64_t out_rows(int64_t nstarts) const { return nstarts + 1; }
    int64_t winners_row(int64_t nstarts) const { return nstarts; }
    int64_t best_offset(int64_t nstarts) const { return out.total_bytes(out_rows(nstarts)); }   // bytes from out's base to best[ncomp]
    int64_t best_bytes() const { return (4 * std::max<int64_t>(ncomp, 0) + 7) / 8 * 8; }
    int64_t out_bytes(int64_t nstarts) const { return best_offset(nstarts) + best_bytes(); }
};
inline LmStartsLayout lm_starts_layout(int64_t ncomp, int64_t res_doubles, int64_t hist_cap, int64_t nfree, int64_t ws_doubles, int64_t nvars) {
    return LmStartsLayout{lm_plan_layout(ncomp, res_doubles, hist_cap, nfree, ws_doubles).out, ReplicaLayout(2, 8 * ws_doubles, 8 * nvars), ncomp};
}

// Members of one launch: the member is the grid's second dimension (at most 65535) and every member of a launch has
// `member_bytes` of replicas within `budget_bytes` -- at least one member a launch, whatever the budget; a replica of nothing
// bounds nothing.  No bit of a result depends on it.  The one rule of the five entries and of the Levenberg-Marquardt plan's two
// solve entries.  What its callers can pass:
//   count         >= 1: every entry refuses or returns before it asks (nstarts < 1, count < 1; a population has a member);
//   budget_bytes  >= 0: the plan option starts_workspace_bytes, the population options eval_workspace_bytes and
//                 grad_workspace_bytes and the Levenberg-Marquardt plan's option workspace_bytes are refused below zero by their
//                 option rules (a negative budget would give 1, as zero does);
//   member_bytes  >= 0, and 0 only from the two solve entries (a launch that runs nothing but the tiny-component solver on
//                 per-factor rotations) and from a Levenberg-Marquardt plan whose components are all empty (no free variable,
//                 no factor: ws_doubles 0; a plan of no component returns before it asks): the evaluation has at least one partial, 8 bytes, and the gradient's branches at least
//                 8 (9 + 3 + 1) and 8 (0 + 1) -- its "no factor" branch, the only one without scratch, does not ask.
inline int64_t members_per_launch(int64_t count, int64_t budget_bytes, int64_t member_bytes) {
    const int64_t fit = member_bytes > 0 ? std::max<int64_t>(1, budget_bytes / member_bytes) : count;
    return std::min(std::min(fit, count), (int64_t)65535);
}

// ... of a call whose launches include cooperative ones (rdis_hip_plan_solve_population_cooperative): every workgroup of a
// cooperative launch must be resident, so a launch of R members with `launch_workgroups` workgroups a member (the largest
// total_wg among the plan's cooperative launches) has R launch_workgroups <= cap_workgroups, the resident workgroups of the
// population kernel -- at least one member a launch (a launch too large for the device is rejected by the runtime, not hung).
// launch_workgroups <= 0: the plan has no cooperative launch, and the cap bounds nothing.
inline int64_t coop_members_per_launch(int64_t count, int64_t budget_bytes, int64_t member_bytes, int64_t cap_workgroups, int64_t launch_workgroups) {
    const int64_t R = members_per_launch(count, budget_bytes, member_bytes);
    if (launch_workgroups <= 0) return R;
    return std::max<int64_t>(1, std::min(R, cap_workgroups / launch_workgroups));
}

}  // namespace rdis_hip
