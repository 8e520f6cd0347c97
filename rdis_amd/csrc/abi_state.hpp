// abi_state.hpp -- what the translation units of the C ABI (include/rdis_hip.h) share: the handles' structs, the small helpers
// every entry point uses (errors, the current device, device memory) and the two functions of rdis_hip.hip another unit calls
// (prepare_partition, problem_scratch).  Internal to librdis_hip.so.
// No kernel and no header with a kernel is seen from here: rdis_hip.hip is the one translation unit of the ABI with device
// code, the others (comm.hip, plan_query.hip, lm_api.hip) are host code.
#pragma once
#include "../../include/rdis_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_blocks.hpp"
#include "plan_tables.hpp"
#include "plan_options.hpp"
#include "plan_index.hpp"
#include "components.hpp"
#include "lm_solver.hpp"
#include "lm_batch.hpp"
#include "grad_fused.hpp"
#include "starts_api.hpp"

using namespace rdis_hip;   // (the ABI's translation units are written inside it)

namespace rdis_hip {
// Constants of headers that define kernels, restated for the translation units that must not see those; rdis_hip.hip, which
// sees both, asserts each equal to its original.
constexpr int ABI_LDS_MAX_BYTES = 160 * 1024 - 4096;   // solver_lds.hpp: LDS_MAX_BYTES
constexpr int ABI_PIPE_TM = 48;                        // solver_pipe.hpp: PIPE_TM
// the caller's starts of a multi-start solve go through pinned memory up to this size (rdis_hip_plan_solve_starts,
// rdis_hip_lm_plan_solve_starts)
constexpr size_t STARTS_STAGE_MAX_BYTES = 64u << 20;
}  // namespace rdis_hip

struct rdis_hip_ctx {
    int device = 0;                   // the device as the caller names it
    int phys = 0;                     // ... and the GPU behind it (the same, except under RDIS_HIP_VIRTUAL_DEVICES: tests)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 0;
    std::string err;
    // second stream for the batched launch of a plan that also has cooperative launches (they overlap)
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // resident-workgroup caps of the cooperative layouts on THIS device (occupancy queries, asked once per context)
    int cap_pipe = -1, cap_coop[3] = {-1, -1, -1};
    int cap_pipe_rr = -1, cap_coop_rr[3] = {-1, -1, -1};   // ... of the reference-rounding instantiations (refround_api.hpp)
    int cap_coop_pop[3] = {-1, -1, -1}, cap_coop_pop_rr[3] = {-1, -1, -1};   // ... of the cooperative population kernel (solver_coop_population.hpp), over all members of a launch
    // dynamic LDS a launch may ask for on THIS device: what a compute unit has, less the solvers' static share (at most
    // solver_lds.hpp's LDS_MAX_BYTES, which is gfx950's); components that do not fit go to the solvers that need none
    size_t lds_limit = ABI_LDS_MAX_BYTES;
};

namespace rdis_hip {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool owned = true;  // false: a slice of the problem's arena
    bool host = false;  // pinned host memory (hipHostMalloc), mapped into the device's address space
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned), host(o.host) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf() { release(); }
    void release() { if (p && owned) (void)(host ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; owned = true; host = false; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

inline int fail(rdis_hip_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
// Several contexts from one thread (OptimizableFunction::setDevices): every entry point must make its context's device current
// before it allocates or launches.  A box with ONE GPU cannot show a forgotten one -- so RDIS_HIP_VIRTUAL_DEVICES=n (tests) makes
// the library offer n devices that all stand on GPU 0, remember which of them the calling thread made current last
// (make_current), and refuse every HIP call issued for a context while another context's device is the current one.
inline int virtual_devices() {
    static const int n = [] { const char* e = std::getenv("RDIS_HIP_VIRTUAL_DEVICES"); return e ? std::max(0, std::atoi(e)) : 0; }();
    return n;
}
inline int& current_logical_device() { static thread_local int d = -1; return d; }
inline hipError_t make_current(const rdis_hip_ctx* c) { current_logical_device() = c->device; return hipSetDevice(c->phys); }
#define HIPCHK(ctx, expr)                                                                    \
    do {                                                                                     \
        if (virtual_devices() > 0 && (ctx) != nullptr && current_logical_device() != (ctx)->device)  \
            return fail((ctx), RDIS_HIP_EDEVICE, std::string(#expr) + ": issued while device " + std::to_string(current_logical_device()) + \
                        " is current, for a context of device " + std::to_string((ctx)->device) + " (an entry point that did not make its device current)"); \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail((ctx), e__ == hipErrorOutOfMemory ? RDIS_HIP_ENOMEM : RDIS_HIP_EDEVICE, \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                 \
    } while (0)

// Every entry point makes its context's device the calling thread's current one first: a host that drives several
// contexts from one thread (rdis::OptimizableFunction::setDevices) would otherwise allocate, create events and launch
// on whichever device its previous call left current.
#define USE_DEVICE(ctx)                                        \
    do {                                                       \
        hipError_t d__ = make_current(ctx);                    \
        HIPCHK((ctx), d__);                                    \
    } while (0)

inline int dalloc(rdis_hip_ctx* c, DevBuf& b, size_t bytes) {
    b.release();
    if (bytes == 0) bytes = 8;
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    b.owned = true;
    return 0;
}
// pinned host memory, mapped into the device's address space (the same pointer on both sides)
inline int halloc(rdis_hip_ctx* c, DevBuf& b, size_t bytes) {
    b.release();
    if (bytes == 0) bytes = 8;
    HIPCHK(c, hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
    b.bytes = bytes;
    b.owned = true;
    b.host = true;
    return 0;
}
template <class T>
int upload(rdis_hip_ctx* c, DevBuf& b, const T* src, size_t n) {
    int rc = dalloc(c, b, n * sizeof(T));
    if (rc) return rc;
    if (n) HIPCHK(c, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}
template <class T>
int upload(rdis_hip_ctx* c, DevBuf& b, const std::vector<T>& v) { return upload(c, b, v.data(), v.size()); }
inline int upload(rdis_hip_ctx* c, DevBuf& b, const ivec& v) { return upload(c, b, v.data(), v.size()); }
inline int ensure(rdis_hip_ctx* c, DevBuf& b, size_t bytes) { return b.bytes >= bytes ? 0 : dalloc(c, b, bytes); }

inline int grid_for(const rdis_hip_ctx* c, long long work, int threads) {
    long long blocks = (work + threads - 1) / threads;
    const long long cap = (long long)std::max(1, c->num_cus) * 8;  // grid-stride beyond 8 blocks/CU
    return (int)std::max(1ll, std::min(blocks, cap));
}

}  // namespace rdis_hip

// the fused gradient pass's tables for one factor list (grad_fused.hpp), kept by the problem
struct GradPlan {
    unsigned long long key0 = 0, key1 = 0, used = 0;   // two hashes of the id list (0, 0: all factors); last use
    int64_t nf = 0;
    DevBuf ints, shorts, fac;      // one int32 block, one 16-bit block, the list as int32 (explicit lists)
    DevBuf cstage, pstage, partial;
    int cstage_slots = 0, pstage_slots = 0;   // slots of the staging arrays (a population's gradient sizes its replicas by them)
    std::vector<int64_t> ids;      // the list itself (explicit lists): compared on a hash hit -- two lists with the same hashes must not share tables
    size_t device_bytes() const { return ints.bytes + shorts.bytes + fac.bytes + cstage.bytes + pstage.bytes + partial.bytes; }
    rdis_hip::GradTables T{};
};

struct rdis_hip_problem {
    rdis_hip_ctx* ctx = nullptr;
    int kind = KIND_BA;
    int64_t N = 0, F = 0, nnz = 0;
    int each_rounding = 0;             // rdis_hip_set_factor_rounding: how eval_each / grad_each_ba round (1: like the reference's build)
    DevBuf x, lo, hi, cam, pt, obs, coeff, rowptr, vid, expo, cons, sine;
    DevBuf useexp;                     // per factor: value = coeff * exp(-product) (rdis_hip_nlp_set_exponential)
    std::vector<uint8_t> h_useexp;     // empty: no factor has it
    DevBuf cam_blocks, xrot;                        // distinct camera blocks; their rotation records (shadow of x)
    int64_t ncam_blocks = 0;
    ivec h_block_of;                    // [N] first variable id of the camera block a variable belongs to, -1 = none
    ivec h_ptblock_of;                  // [N] ... of the point block, -1 = none (valid when ncam_blocks > 0)
    ivec h_blk_stamp, h_blk_idx;        // [N] scratch of the slot tables (solver_lds.hpp), valid by stamp
    ivec h_cam, h_pt, h_rowptr, h_vid;  // host copies for plan building
    // scratch for the eval entry points
    DevBuf gfac, partial, scalar, tmp_idx, tmp_val, tmp_out, g_all;
    DevBuf all_v2s_ptr, all_v2s_idx;  // gather lists for "all factors"
    bool have_all_v2s = false;
    // fused value + gradient (bundle adjustment with disjoint blocks): per-call camera records, the lists' tables
    DevBuf camrec;
    ivec h_cam_ord;                   // [N] ordinal of the camera block that starts at a variable id, -1 = none
    std::vector<std::unique_ptr<GradPlan>> grad_plans;
    unsigned long long grad_tick = 0;
    // shared by the plans of this problem (solves on a context are serialised)
    DevBuf dir, coop_state, coop_timing;   // search direction by variable id (kept zero between solves), ...
    int coop_state_gen = 0;                // bumped whenever coop_state moves: plans re-derive the pointers they baked in
    DevBuf arena;                          // memory of the transient plan of rdis_hip_cgd_batch
    DevBuf stage_x;                        // pinned staging of a resident plan's start point (rdis_hip_plan_set_start)
    hipEvent_t stage_ev = nullptr;         // ... recorded behind its copy: the next use waits for it
    bool stage_busy = false;
    size_t arena_used = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct rdis_hip_plan* last_timed_plan = nullptr;
    ivec h_local, h_owner_stamp, h_fac_stamp;  // validity by stamp: no O(N) clears per call
    std::vector<VarMark> h_mark;           // [N] plan_create's view of a variable: free in which component, where in the free list
    LmWorkspace lm_ws;                     // scratch of rdis_hip_lm_optimize, kept between calls
    LmBatchWorkspace lm_batch_ws;          // ... and of rdis_hip_lm_batch
    CcWorkspace cc_ws;                     // ... and of rdis_hip_components
    ComponentLists comps;                  // result of the last rdis_hip_components call
    DevBuf assigned;
    int stamp = 0;
    ~rdis_hip_problem() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); if (stage_ev) (void)hipEventDestroy(stage_ev); }

    ProblemView view() const {
        ProblemView v{};
        v.kind = kind; v.N = (int)N; v.F = (int)F;
        v.x = x.as<double>(); v.lo = lo.as<double>(); v.hi = hi.as<double>();
        v.cam = cam.as<int>(); v.pt = pt.as<int>(); v.obs = obs.as<double2>();
        v.xrot = nullptr; v.rot_mode = ROT_PER_FACTOR;
        v.coeff = coeff.as<double>(); v.rowptr = rowptr.as<int>(); v.vid = vid.as<int>();
        v.expo = expo.as<double>(); v.cons = cons.as<double>(); v.sine = sine.as<uint8_t>();
        v.useexp = h_useexp.empty() ? nullptr : useexp.as<uint8_t>();
        return v;
    }
    int64_t nslots() const { return kind == KIND_BA ? 12 * F : nnz; }
    int arity(int f) const { return kind == KIND_BA ? 12 : h_rowptr[f + 1] - h_rowptr[f]; }
    int var_of(int f, int k) const {
        if (kind == KIND_BA) return k < 9 ? h_cam[f] + k : h_pt[f] + (k - 9);
        return h_vid[h_rowptr[f] + k];
    }
    int slot_of(int f, int k) const { return kind == KIND_BA ? 12 * f + k : h_rowptr[f] + k; }
};


struct CoopItem {
    int comp = 0, nwg = 0;
    size_t xi_off = 0;  // where its published search direction starts in the plan's xi_glob
    // offsets into the plan's coop_ints block (one upload for all cooperative components)
    size_t slot_li = 0;   // [12 * m] local free index of each factor slot, -1 = constant
    size_t lane_var = 0;  // [nwg * threads] free variable owned by a lane, -1 = none
    size_t wave_var = 0;  // [nwg * threads / 64] free variable owned by a whole wave, -1 = none
};

struct CoopLaunch {      // cooperative groups that run side by side in one launch
    int first = 0, count = 0, total_wg = 0;   // items [first, first + count) of the plan's list
    DevBuf groups, wg_group;
};

struct StreamItem {
    int comp = 0, nwg = 0, nlong = 0;
    DevBuf long_vars;  // local indices of the variables fed by many partials
};

// The options (plan_options.hpp: what rdis_hip_plan_set_option writes) and the index plan_create lays out (plan_index.hpp: the
// host lists, the int32 block `ints` with its offsets) are the bases; below them what prepare_partition decides, the device
// buffers, and what the last solve and the last many-solve call left.
struct rdis_hip_plan : PlanOptions, PlanIndex {
    rdis_hip_problem* prob = nullptr;
    bool transient = false;  // lives in the problem's arena (rdis_hip_cgd_batch): one at a time
    size_t dev_bytes = 0;    // device memory of its own (plan_alloc; rdis_hip_plan_device_bytes)

    // ---- the lists (plan_create) ----
    int64_t ncomp = 0, nfree = 0, nfac = 0;
    // one device block of int32, `ints` (PlanIndex), and one of results, `outbuf`
    // results block: xout[nfree] fret[nc] delta[nc] (f64) | nfeval[nc] ngeval[nc] (i64) | iters[nc] status[nc] trace_n[nc] (i32)
    size_t out_bytes = 0;
    cvec h_out;
    // a resident plan's host image of the results block is pinned (plan_create): the D2H copy of rdis_hip_plan_fetch then lands
    // without the runtime's staging of a pageable destination.  It starts at byte h_pin_base of the block (a long x never passes
    // through it: DIRECT_X_BYTES).  Empty -- a transient plan, a block over the bound, no pinned memory to be had -- : h_out.
    DevBuf h_pin;
    size_t h_pin_base = 0;
    bool have_start = false;

    // ---- what prepare_partition decides: which components go where (rebuilt when an option changes) ----
    bool partition_dirty = true;
    int coop_state_gen = -1;          // generation of the problem's exchange-state buffer this partition points into
    std::vector<CoopItem> coop;
    std::vector<CoopLaunch> coop_launches;
    ivec h_coop_ints;   // host image of coop_ints (kept: the upload is asynchronous)
    std::vector<std::vector<CoopGroup>> h_coop_groups;
    std::vector<ivec> h_coop_wg;
    bool use_pipe = false;            // the plan's groups fit the pipelined layout (fewer factor lanes per workgroup)
    bool pipelined() const { return use_pipe; }
    bool objective_in_solver = false; // the plan's one launch is the single-group pipelined solver, which stores the objective itself (CoopArgs::objective)
    int coop_lanes() const;           // factor lanes per workgroup of a cooperative group
    std::vector<StreamItem> stream;
    ivec h_rest;                      // the batch list: tiny components, then the plain solver's, the point-major ones, the LDS-resident ones
    int rest_tiny = 0;                // the first rest_tiny entries of the batch list run on the quad / wave solver
    int rest_lds = 0;                 // the LAST rest_lds entries run on the LDS-resident solver (solver_lds.hpp)
    int rest_ptm = 0;                 // the rest_ptm entries before them on the point-major streaming solver (solver_ptm.hpp)
    int tiny_group = 4;               // ... with this many lanes per tiny component (4 or 16)
    int group_blocks4 = 0, group_blocks16 = 0;   // resident blocks of the tiny-component kernels
    int rest_rot_mode = ROT_PER_FACTOR; // how the factors of the batch list get their camera rotations (device_views.hpp)
    // the LDS-resident solver's slot tables (one int32 block, lds_ints) and caps
    int lds_ns_cap = 0, lds_ncb_cap = 0, lds_chunk_cap = 0, lds_rot_mode = ROT_PER_FACTOR;
    int64_t lds_max_factors = 0;
    ivec h_lds_ints;
    size_t off_ls_ptr = 0, off_ls_vid = 0, off_ls_free = 0, off_ls_ncb = 0, off_ls_fidx = 0, off_ls_gperm = 0, off_ls_gptr = 0;
    int64_t ls_total_chunks = 0;      // gradient chunks of all slot tables
    // the dynamic LDS of the LDS-resident launch, and whether its trials run in matrix form (the records must fit behind the other arrays)
    bool lds_matrix_on(const rdis_hip_ctx* c) const;
    size_t lds_dyn_bytes(const rdis_hip_ctx* c) const;
    // the point-major streaming solver's tables
    int ptm_ncb_cap = 0, ptm_rot_mode = ROT_PER_FACTOR;
    int64_t pm_blocks = 0, pm_entries = 0;
    ivec h_pm_jg;
    int64_t pm_cptr_len = 0;          // entries of pm_cptr (a component's wave-chunks + 1)
    int64_t ptm_min_points = 0;       // the smallest streaming component's point blocks
    size_t off_pm_pt0 = 0, off_pm_ch0 = 0, off_pm_cptr = 0, off_pm_jg = 0;
    // the gradient's round lists (solver_ptm.hpp), built for one workgroup size and group size at a time (ptm_build_rounds)
    int rounds_threads = 0, rounds_K = 0, rounds_slots = 1;   // (slots a round stages: ptm_round_slots_for)
    bool ptm_wide_wanted = false;     // a large component joined the batch list for a wide point-major group
    // a wide group with LOCAL camera numbering (solver_ptm.hpp: a component with more cameras than the LDS holds; one such component a plan)
    bool ptm_local = false, ptm_local_off = false;   // the plan has such a component; it was tried and did not fit (then never again)
    int ptm_local_K = 0, ptm_local_comp = -1;
    PtmLocalTables loc;                              // its host tables (plan_tables.hpp)
    bool coop_reference_rounding() const { return factor_rounding != 0; }
    bool batch_reference_rounding() const { return factor_rounding == 1; }

    // ---- device buffers ----
    DevBuf ints, ws, gfac, xstart, outbuf, objective, trace, vdump;
    DevBuf coop_ints;
    DevBuf rest_order, xi_glob, queue;
    DevBuf lds_ints, lds_obs;
    DevBuf pm_rec, pm_gh, pm_cbox, pm_bex, pm_cam, pm_obs;
    DevBuf pm_rounds, pm_rd_off, pm_rd_n, pm_grow, pm_segs, pm_sg_off;
    // ... shared by several workgroups each (cgd_ptmg_kernel) when a launch has fewer components than compute units
    DevBuf ptm_xch, ptm_state;
    DevBuf lc_dev, lc_off_dev, cr_ptr_dev, cr_dev, ptm_tot;   // the local group's tables
    DevBuf st_ev, st_val;             // the stale-cache emulation's, allocated at the first solve that needs them
    DevBuf seq_val, seq_ab;           // the parity option's buffers (PlanView::seq_val, seq_ab), likewise
    // multi-start and population solves (rdis_hip_plan_solve_starts, rdis_hip_plan_solve_population): inputs and outputs of every
    // start of the last call, kept until fetched; the replicas of the per-solve workspace one launch needs, bounded by the option
    // "starts_workspace_bytes" (ms_work: ws, gfac and, for the plain solver, x; ms_dir: that solver's dir, zero between launches)
    DevBuf ms_in, ms_out, ms_work, ms_dir, ms_best, ms_stage;   // (ms_stage: pinned host memory the caller's starts are uploaded through)
    DevBuf ms_queue;                  // the tiny-component population launch: a queue counter for each of its members
    DevBuf ms_coop;                   // the cooperative population launch (rdis_hip_plan_solve_population_cooperative): a replica of gfac and of the groups' xi_glob and an exchange state a group for each of its members (within "starts_workspace_bytes" too)
    DevBuf ms_ptm;                    // the point-major population launch: a replica of pm_rec, pm_gh, pm_bex and pm_cbox for each of its members (within "starts_workspace_bytes" too)

    // ---- the last solve ----
    int last_launches = 0;
    bool timed = false;
    int ptm_last_group = 1;           // the point-major launch's workgroups a component (rdis_hip_plan_debug_counters has no slot for it: get_info)
    int ptm_last_threads = 0;         // ... and their lanes
    bool ptm_wide_last = false;       // ... and whether it ran as wide groups

    // ---- the last many-solve call ----
    hipEvent_t ms_stage_ev = nullptr;
    bool ms_stage_busy = false;
    int64_t ms_n = 0;                 // starts of the last multi-start solve (0: none to fetch)
    bool ms_population = false;       // ... which was a population solve (rdis_hip_plan_solve_population: the members are the starts; no ms_best)
    int64_t ms_per_launch = 0, ms_launches = 0;
    int ms_tiny_blocks = 0;           // blocks a member of the tiny-component launch in the last population solve (plan_get_info "population_tiny_blocks")
    int ms_coop_wg = 0, ms_coop_cap = 0;   // the cooperative launches of the last population solve: the most workgroups a member, and the resident workgroups a launch may have over all its members (0, 0: it had none; plan_get_info "population_cooperative_workgroups", "population_cooperative_cap")
    int ms_ptm_threads = 0;           // the lanes of the point-major kernel in the last population solve, 0 = it had none (plan_get_info "population_point_major_threads")

    ~rdis_hip_plan() { if (ms_stage_ev) (void)hipEventDestroy(ms_stage_ev); }
    // the outputs' block for n starts: xout[n][nfree] fret[n][nc] delta[n][nc] (f64) | nfeval[n][nc] ngeval[n][nc] (i64) | iters[n][nc] status[n][nc] (i32)
    size_t ms_out_bytes(int64_t n) const { return (size_t)n * ((size_t)nfree * 8 + (size_t)ncomp * 40); }
    StartsView starts_view(int64_t n) const {
        StartsView s{};
        const size_t sn = (size_t)n * (size_t)nfree, sc = (size_t)n * (size_t)ncomp;
        s.xstart = ms_in.as<double>();
        s.xout = ms_out.as<double>();
        s.fret = s.xout + sn; s.delta = s.fret + sc;
        s.nfeval = reinterpret_cast<long long*>(s.delta + sc); s.ngeval = s.nfeval + sc;
        s.iters = reinterpret_cast<int*>(s.ngeval + sc); s.status = s.iters + sc;
        s.ws = ms_work.as<double>(); s.gfac = nullptr;   // (gfac, x: behind the launch's replicas of ws -- the solve knows their number)
        s.x = nullptr; s.dir = nullptr;
        s.nfree = nfree; s.ngfac = ngfac; s.N = prob->N; s.first = 0;
        return s;
    }

    const int* ip(size_t off) const { return ints.as<int>() + off; }
    double* out_f64(size_t idx) const { return outbuf.as<double>() + idx; }
    PlanView view() const {
        PlanView v{};
        const size_t nc = (size_t)ncomp;
        v.ncomp = (int)ncomp;
        v.order = rest_order.as<int>();
        v.free_ptr = ip(off_free_ptr); v.free_vid = ip(off_free_vid);
        v.fac_ptr = ip(off_fac_ptr); v.fac_id = ip(off_fac_id);
        v.v2s_ptr = ip(off_v2s_ptr); v.slot_base = ip(off_slot_base); v.slot_pos = ip(off_slot_pos);
        v.cb_ptr = ip(off_cb_ptr); v.cb = ip(off_cb); v.cb_li = ip(off_cb_li);
        const int* li = lds_ints.as<int>();
        v.ls_ptr = li + off_ls_ptr; v.ls_vid = li + off_ls_vid; v.ls_free = li + off_ls_free; v.ls_ncb = li + off_ls_ncb;
        v.ls_fidx = reinterpret_cast<const unsigned*>(li + off_ls_fidx);
        v.ls_obs = lds_obs.as<double2>();
        v.ls_gperm = li + off_ls_gperm; v.ls_gptr = li + off_ls_gptr;
        v.ls_cam_gfac = lds_camera_sums ? 0 : 1;
        v.ls_matrix = lds_matrix_on(prob->ctx) ? 1 : 0;
        v.st_ev = emulate_stale ? st_ev.as<int>() : nullptr; v.st_val = emulate_stale ? st_val.as<double>() : nullptr;
        v.pm_pt0 = li + off_pm_pt0; v.pm_ch0 = li + off_pm_ch0; v.pm_cptr = li + off_pm_cptr;
        v.pm_rec = pm_rec.as<double>(); v.pm_gh = pm_gh.as<double>(); v.pm_cbox = pm_cbox.as<float>(); v.pm_bex = pm_bex.as<double>(); v.pm_cam = pm_cam.as<short>(); v.pm_obs = pm_obs.as<double2>();
        v.pm_grow = pm_grow.as<unsigned short>(); v.pm_rounds = pm_rounds.as<unsigned short>(); v.pm_rd_off = pm_rd_off.as<long long>(); v.pm_rd_n = pm_rd_n.as<int>(); v.pm_round_slots = rounds_slots;
        v.pm_segs = pm_segs.as<int>(); v.pm_sg_off = pm_sg_off.as<long long>();
        v.seq_val = seq_val.as<double>(); v.seq_ab = seq_ab.as<double>(); v.seq_n = (int)nfree;
        v.timing = prob->coop_timing.as<long long>();
        v.ws = ws.as<double>(); v.dir = prob->dir.as<double>(); v.gfac = gfac.as<double>();
        v.xstart = xstart.as<double>();
        v.xout = out_f64(0);
        v.fret = out_f64((size_t)nfree); v.delta = out_f64((size_t)nfree + nc);
        long long* i64 = reinterpret_cast<long long*>(out_f64((size_t)nfree + 2 * nc));
        v.nfeval = i64; v.ngeval = i64 + nc;
        int* i32 = reinterpret_cast<int*>(i64 + 2 * nc);
        v.iters = i32; v.status = i32 + nc; v.trace_n = i32 + 2 * nc;
        v.trace = trace_records > 0 ? trace.as<double>() : nullptr;
        v.trace_cap = trace_records;
        v.vdump = dump_iters > 0 ? vdump.as<double>() : nullptr;
        v.dump_iters = dump_iters;
        return v;
    }
};

// rdis_hip.hip: decide which solver takes each component and build what it needs (plan_query.hip asks before it answers)
namespace rdis_hip {
int prepare_partition(rdis_hip_plan* L);
int problem_scratch(rdis_hip_problem* p);   // rdis_hip.hip's ensure_problem_scratch (the problem's shared scratch, at first use) for lm_api.hip
}
