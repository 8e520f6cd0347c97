// lm_api.hip -- the C ABI's Levenberg-Marquardt entries (include/rdis_hip.h): rdis_hip_lm_optimize, rdis_hip_lm_batch and the
// plans (rdis_hip_lm_plan_*).  Host code only: every launch goes through a function of lm_solver.hip, lm_batch.hip or
// lm_starts.hip, and no header with a kernel is seen from here.  The rules the entries share are lm_rules.hpp's.
#include "abi_state.hpp"

#include <new>

#include "lm_rules.hpp"
#include "lm_starts.hpp"
#include "population_state.hpp"
#include "replica_layout.hpp"

extern "C" int rdis_hip_lm_optimize(rdis_hip_problem* p, int64_t nfree, const int64_t* free_vid, int64_t nf, const int64_t* fac_id,
                                    double* x_inout, int32_t maxiters, double ftol, int32_t model, double* fret, double* delta, double* info8,
                                    double* hist4, int64_t hist_cap, int64_t* nhist) {
    if (!p) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (p->kind != KIND_BA) return fail(c, RDIS_HIP_EINVAL, "lm_optimize: bundle adjustment problems only");
    if (nfree <= 0 || nf <= 0 || !free_vid || !fac_id || maxiters < 1) return fail(c, RDIS_HIP_EINVAL, "lm_optimize: bad arguments");
    USE_DEVICE(c);
    const LmBlockLayout B = lm_block_layout(p->N, p->F, p->h_cam.data(), p->h_pt.data());
    if (!B.factors_fit)
        return fail(c, RDIS_HIP_EINVAL, "lm_optimize: variables are not laid out as camera blocks of 9 followed by point blocks of 3");
    if (x_inout) {
        int rc = rdis_hip_set_x(p, nfree, free_vid, x_inout);
        if (rc) return rc;
    }
    LmProblem P{(int)p->N, (int)p->F, B.ncams, p->x.as<double>(), p->lo.as<double>(), p->hi.as<double>(),
                p->cam.as<int>(), p->pt.as<int>(), p->h_cam.data(), p->h_pt.data(), p->obs.as<double2>()};
    LmOptions o{maxiters, LM_TAU, LM_EPS1, LM_EPS2, ftol, model & 15, (model >> 4) & 3};
    LmResult r;
    std::string err;
    const int e = device_lm_ba(c->stream, P, nfree, free_vid, nf, fac_id, o, &p->lm_ws, &r, &err);
    if (e < 0) return fail(c, RDIS_HIP_EINVAL, err);
    if (e > 0) return fail(c, RDIS_HIP_EDEVICE, std::string("lm_optimize: ") + hipGetErrorString((hipError_t)e));
    if (x_inout) {
        int rc = rdis_hip_get_x(p, nfree, free_vid, x_inout);
        if (rc) return rc;
    }
    const double row[LM_BATCH_RES] = {r.fret, r.finit, (double)r.iters, (double)r.stop, (double)r.nfev, (double)r.njev, (double)r.nsolve, r.mu,
                                      (double)r.ncam_blocks, (double)r.npt_blocks, (double)r.history.size()};
    lm_result_rows(1, row, nullptr, 0, fret, delta, info8, nhist, nullptr);
    if (hist4)
        for (size_t i = 0; i < r.history.size() && (int64_t)i < hist_cap; ++i) {
            hist4[4 * i] = r.history[i].mu; hist4[4 * i + 1] = r.history[i].dp_l2;
            hist4[4 * i + 2] = r.history[i].f_trial; hist4[4 * i + 3] = r.history[i].accepted;
        }
    return 0;
}

// Levenberg-Marquardt for a batch of small components, one workgroup each (lm_batch.hip).  Everything that can be refused
// is refused on the host, before x is touched or anything is launched: the lists by the plan index's checks, the
// components' sizes and factor pairs by lm_batch_prepare.
static_assert(LM_BATCH_EINVAL == RDIS_HIP_EINVAL && LM_BATCH_ERANGE == RDIS_HIP_ERANGE && LM_BATCH_MAX_CAMERAS == RDIS_HIP_LM_BATCH_MAX_CAMERAS &&
                  LM_BATCH_WIDE_MAX_CAMERAS == RDIS_HIP_LM_WIDE_MAX_CAMERAS && (RDIS_HIP_LM_WIDE & 255) == 0,
              "lm_batch.hpp restates include/rdis_hip.h");
namespace {
// What rdis_hip_lm_batch and rdis_hip_lm_plan_create check and build before x is touched (`who` names the entry in the
// messages): the problem, the model, the lists, the components' independence, then lm_batch_prepare's tables.
int lm_batch_tables(rdis_hip_problem* p, const std::string& who, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid,
                    const int64_t* fac_ptr, const int64_t* fac_id, int R, bool wide, LmBatchTables& T) {
    rdis_hip_ctx* c = p->ctx;
    if (R != 1 && R != 2) return fail(c, RDIS_HIP_EINVAL, who + ": residual model must be 1 or 2");
    if (p->ncam_blocks <= 0 && p->F > 0) return fail(c, RDIS_HIP_EINVAL, who + ": the factors' camera and point blocks overlap");
    auto relabel = [&who](std::string m) {
        for (const char* from : {"plan_create", "lm_batch"})
            if (m.rfind(from, 0) == 0) return who + m.substr(std::strlen(from));
        return m;
    };
    std::string why;
    if (int rc = plan_index_check(ncomp, free_ptr, free_vid, fac_ptr, fac_id, &why)) return fail(c, rc, relabel(why));
    USE_DEVICE(c);
    int rc = problem_scratch(p);
    if (rc) return rc;
    {   // independence, by the plan index's check (its tables are not kept)
        PlanIndex X;
        const IndexArrays A{p->kind, p->N, p->F, p->h_cam.data(), p->h_pt.data(), p->h_rowptr.data(), p->h_vid.data(),
                            p->h_block_of.data(), p->ncam_blocks, p->h_mark.data(), p->h_fac_stamp.data(), ++p->stamp};
        if ((rc = plan_index_build(A, ncomp, free_ptr, free_vid, fac_ptr, fac_id, X, &why))) return fail(c, rc, relabel(why));
    }
    // what rdis_hip_lm_optimize requires; where it holds and the points' ids are whole blocks, a variable no factor reads belongs
    // to the layout's block, like there
    const LmBlockLayout B = lm_block_layout(p->N, p->F, p->h_cam.data(), p->h_pt.data());
    const bool layout = p->F > 0 && B.whole_points && B.factors_fit;
    const LmBatchBlocks blocks{p->N, p->F, p->h_cam.data(), p->h_pt.data(), p->h_block_of.data(), p->h_ptblock_of.data(), layout, B.ncams};
    if ((rc = lm_batch_prepare(blocks, ncomp, free_ptr, free_vid, fac_ptr, fac_id, R, T, &why, wide))) return fail(c, rc, relabel(why));
    return 0;
}
}  // namespace

extern "C" int rdis_hip_lm_batch(rdis_hip_problem* p, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid,
                                 const int64_t* fac_ptr, const int64_t* fac_id, double* x_inout, int32_t maxiters, double ftol,
                                 int32_t model, double* fret, double* delta, double* info8, double* hist4, int64_t hist_cap,
                                 int64_t* nhist) {
    if (!p) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (p->kind != KIND_BA) return fail(c, RDIS_HIP_EINVAL, "lm_batch: bundle adjustment problems only");
    if (ncomp < 0 || !free_ptr || !fac_ptr || maxiters < 1 || hist_cap < 0) return fail(c, RDIS_HIP_EINVAL, "lm_batch: bad arguments");
    const int R = model & 15;   // (the Schur bits of rdis_hip_lm_optimize are ignored)
    const bool wide = (model & RDIS_HIP_LM_WIDE) != 0;
    LmBatchTables T;
    int rc = lm_batch_tables(p, "lm_batch", ncomp, free_ptr, free_vid, fac_ptr, fac_id, R, wide, T);
    if (rc) return rc;
    const int64_t nfree = free_ptr[ncomp];
    if (x_inout && nfree > 0 && (rc = rdis_hip_set_x(p, nfree, free_vid, x_inout))) return rc;
    const LmBatchProblem P{p->x.as<double>(), p->lo.as<double>(), p->hi.as<double>(), p->cam.as<int>(), p->pt.as<int>(), p->obs.as<double2>()};
    std::vector<double> res, hist;
    const int64_t cap = hist4 ? hist_cap : 0;
    const int e = device_lm_batch(c->stream, P, T, lm_batch_options(maxiters, R, ftol), cap, &p->lm_batch_ws, &res, &hist);
    if (e != 0) return fail(c, RDIS_HIP_EDEVICE, std::string("lm_batch: ") + hipGetErrorString((hipError_t)e));
    if (x_inout && nfree > 0 && (rc = rdis_hip_get_x(p, nfree, free_vid, x_inout))) return rc;
    lm_result_rows(ncomp, res.data(), hist.data(), cap, fret, delta, info8, nhist, hist4);
    return 0;
}

// =====================================================================================
// Levenberg-Marquardt plans: lm_batch's tables built and uploaded once, solves that stay on the stream, on the problem's x
// or on the members of a population (the member is the grid's second dimension of lm_batch.hip's kernel)
// =====================================================================================
struct rdis_hip_lm_plan {
    rdis_hip_problem* prob = nullptr;
    int64_t ncomp = 0, nfree = 0, hist_cap = 0;
    int R = 1;
    LmBatchTableLayout lay{};
    int ncls[LM_BATCH_CLASSES] = {};
    LmPlanLayout layout;                    // replica_layout.hpp: the outputs of a solve's members, the workspace of a launch's
    LmStartsLayout starts;                  // ... and of a multi-start solve: a row more (the winners'), best, a scratch row of x a start
    DevBuf tables, out, work;
    int64_t workspace_bytes = (int64_t)1 << 30;   // option "workspace_bytes": bounds `work`
    // the last solve: 0 none, 1 rdis_hip_lm_plan_solve, 2 rdis_hip_lm_plan_solve_population (of last_count members), 3 a multi-start
    // solve (of last_count starts).  Nothing of the population is kept: a fetch reads the plan's own `out` block, which holds
    // last_rows rows of each field; the plan's ordinary outputs -- what rdis_hip_lm_plan_fetch returns and
    // rdis_hip_lm_plan_objective_device sums -- are row last_rows - 1 (kind 1: the one row; kind 3: the winners')
    int last_kind = 0;
    int64_t last_count = 0, last_rows = 0, last_per_launch = 0, last_launches = 0;
    std::vector<double> h_res, h_hist;      // fetch's staging
    // multi-start solves.  The lists are kept from create (host memory only); everything else appears at the first such solve:
    // the tables pos[N] | comp_of[nfree] (lm_starts.hpp) in a buffer of their own, the uploaded starts [nstarts][nfree] with their
    // pinned staging, and the one double of rdis_hip_lm_plan_objective_device
    std::vector<int64_t> h_free_ptr, h_free_vid;
    std::vector<int32_t> h_starts_tables;
    DevBuf starts_tables, starts_in, starts_stage, objective;
    // rdis_hip_lm_plan_summary: the 16 doubles on the device; rdis_hip_lm_plan_summary_population: [count][16], grown on demand.
    // Each with a pinned host image of its size that appears at the first read (lm_read_back; *_pin_failed: no pinned memory
    // was to be had, the copies go to the caller's array directly)
    DevBuf summary, summary_pin, member_summary, member_summary_pin;
    bool summary_pin_failed = false, member_summary_pin_failed = false;
    hipEvent_t starts_stage_ev = nullptr;
    bool starts_stage_busy = false;
    ~rdis_hip_lm_plan() { if (starts_stage_ev) (void)hipEventDestroy(starts_stage_ev); }
    // row `row` of a field of `out` laid out for `rows` rows
    double* res_dev(int64_t rows, int64_t row = 0) const { return layout.out.at<double>(out.p, LM_PLAN_RES, rows) + row * layout.out.doubles(LM_PLAN_RES); }
    double* hist_dev(int64_t rows, int64_t row = 0) const { return layout.out.at<double>(out.p, LM_PLAN_HIST, rows) + row * layout.out.doubles(LM_PLAN_HIST); }
    double* x_dev(int64_t rows, int64_t row = 0) const { return layout.out.at<double>(out.p, LM_PLAN_X, rows) + row * layout.out.doubles(LM_PLAN_X); }
};

namespace {
// What a solve's launches share, whichever layout describes its buffers (lm_plan_layout or lm_starts_layout: the same three
// fields of `out`, the workspace slices as part 0 of `work`).  First the sizes: `out` for the whole solve, `work` for the *per
// members of one launch that workspace_bytes allows.
static_assert(LM_PLAN_WS == 0 && LM_STARTS_WS == 0, "the workspace slices are part 0 of `work` in both layouts");
int lm_plan_size(rdis_hip_lm_plan* L, int64_t count, int64_t out_bytes, const ReplicaLayout& work, int64_t* per) {
    rdis_hip_ctx* c = L->prob->ctx;
    *per = members_per_launch(count, L->workspace_bytes, work.member_bytes());
    const int rc = ensure(c, L->out, (size_t)out_bytes);
    return rc ? rc : ensure(c, L->work, (size_t)work.total_bytes(*per));
}
// ... then the class launches for `n` members: member m from, and into, x + m x_stride, its outputs to row row0 + m of `out`
// laid out for `rows` rows (`who` names the entry where a launch fails)
int lm_plan_launch(rdis_hip_lm_plan* L, const char* who, const LmBatchOptions& o, const ReplicaLayout& work, int64_t per, double* x, long long x_stride,
                   int64_t rows, int64_t row0, int64_t n) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    const ReplicaLayout& out = L->layout.out;
    const LmBatchProblem P{x, p->lo.as<double>(), p->hi.as<double>(), p->cam.as<int>(), p->pt.as<int>(), p->obs.as<double2>()};
    const LmBatchMembers M{x_stride, L->res_dev(rows, row0), out.doubles(LM_PLAN_RES), L->hist_dev(rows, row0), out.doubles(LM_PLAN_HIST),
                           work.at<double>(L->work.p, 0, per), work.doubles(0), L->x_dev(rows, row0), out.doubles(LM_PLAN_X), (int)n};
    const int e = lm_batch_launch(c->stream, P, L->tables.p, L->lay, L->ncls, o, L->hist_cap, M);
    if (e != 0) return fail(c, RDIS_HIP_EDEVICE, std::string(who) + ": " + hipGetErrorString((hipError_t)e));
    L->last_launches += (L->ncls[0] > 0) + (L->ncls[1] > 0) + (L->ncls[2] > 0) + (L->ncls[3] > 0);
    return 0;
}

// `count` members from x0, a member's stride x_stride: outputs for all of them, workspace replicas for the members of one
// launch, the launches.  After the first call of a kind and size: no allocation; never an upload, a download or a wait.
int lm_plan_enqueue(rdis_hip_lm_plan* L, double* x0, long long x_stride, int64_t count, int32_t maxiters, double ftol) {
    L->last_per_launch = 0; L->last_launches = 0;
    if (L->ncomp == 0) return 0;
    int64_t per;
    int rc = lm_plan_size(L, count, L->layout.out.total_bytes(count), L->layout.work, &per);
    if (rc) return rc;
    const LmBatchOptions o = lm_batch_options(maxiters, L->R, ftol);
    for (int64_t m0 = 0; m0 < count; m0 += per)
        if ((rc = lm_plan_launch(L, "lm_plan_solve", o, L->layout.work, per, x0 + m0 * x_stride, x_stride, count, m0, std::min(per, count - m0)))) return rc;
    L->last_per_launch = per;
    return 0;
}

// `count` rows of the last solve's outputs from row `row0` on (the block holds L->last_rows): one download each of the rows' x, the
// result rows and the history, one wait
int lm_plan_download(rdis_hip_lm_plan* L, int64_t row0, int64_t count, double* x_out, double* fret, double* delta, double* info8, double* hist4, int64_t* nhist) {
    rdis_hip_ctx* c = L->prob->ctx;
    const int64_t held = L->last_rows;
    const size_t rows = (size_t)count * (size_t)L->ncomp;
    if (rows == 0) return 0;
    const bool want_x = x_out && L->nfree > 0;
    if (!(want_x || fret || delta || info8 || hist4 || nhist)) return 0;
    const bool want_hist = hist4 && L->hist_cap > 0;
    if (want_x) HIPCHK(c, hipMemcpyAsync(x_out, L->x_dev(held, row0), (size_t)count * (size_t)L->nfree * 8, hipMemcpyDeviceToHost, c->stream));
    L->h_res.resize(rows * LM_BATCH_RES);
    HIPCHK(c, hipMemcpyAsync(L->h_res.data(), L->res_dev(held, row0), rows * LM_BATCH_RES * 8, hipMemcpyDeviceToHost, c->stream));
    if (want_hist) {
        L->h_hist.resize(rows * (size_t)L->hist_cap * 4);
        HIPCHK(c, hipMemcpyAsync(L->h_hist.data(), L->hist_dev(held, row0), rows * (size_t)L->hist_cap * 32, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (row-major in both: entry cc is component cc % ncomp of row row0 + cc / ncomp)
    lm_result_rows((int64_t)rows, L->h_res.data(), L->h_hist.data(), L->hist_cap, fret, delta, info8, nhist, hist4);
    return 0;
}

// `bytes` from the device to the caller's array and a wait: through the pinned image `pin`, grown on demand, where pinned memory
// is to be had; where it is not (`failed` remembers), straight into the caller's array, and no error is left behind
int lm_read_back(rdis_hip_ctx* c, DevBuf& pin, bool& failed, const void* dev, size_t bytes, void* out) {
    if (pin.bytes < bytes && !failed) {
        const std::string err = c->err;
        if (halloc(c, pin, bytes) != 0) { (void)hipGetLastError(); c->err = err; failed = true; }
    }
    void* const img = pin.bytes >= bytes ? pin.p : out;
    HIPCHK(c, hipMemcpyAsync(img, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (img != out) std::memcpy(out, img, bytes);
    return 0;
}
}  // namespace

extern "C" int rdis_hip_lm_plan_create(rdis_hip_problem* p, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid,
                                       const int64_t* fac_ptr, const int64_t* fac_id, int32_t model, int64_t hist_cap, rdis_hip_lm_plan** out) {
    if (!p || !out) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (p->kind != KIND_BA) return fail(c, RDIS_HIP_EINVAL, "lm_plan_create: bundle adjustment problems only");
    if (ncomp < 0 || !free_ptr || !fac_ptr || hist_cap < 0) return fail(c, RDIS_HIP_EINVAL, "lm_plan_create: bad arguments");
    const int R = model & 15;
    const bool wide = (model & RDIS_HIP_LM_WIDE) != 0;
    LmBatchTables T;
    int rc = lm_batch_tables(p, "lm_plan_create", ncomp, free_ptr, free_vid, fac_ptr, fac_id, R, wide, T);
    if (rc) return rc;
    if ((double)ncomp * (double)std::max<int64_t>(hist_cap, 1) >= 1.0e15) return fail(c, RDIS_HIP_ERANGE, "lm_plan_create: history too large");
    std::unique_ptr<rdis_hip_lm_plan> L(new (std::nothrow) rdis_hip_lm_plan);
    if (!L) return fail(c, RDIS_HIP_ENOMEM, "lm_plan_create: host allocation");
    L->prob = p; L->ncomp = ncomp; L->nfree = free_ptr[ncomp]; L->hist_cap = hist_cap; L->R = R;
    for (int k = 0; k < LM_BATCH_CLASSES; ++k) L->ncls[k] = (int)T.order[k].size();
    L->lay = lm_batch_table_layout(T);
    L->layout = lm_plan_layout(ncomp, LM_BATCH_RES, hist_cap, L->nfree, T.ws_doubles);
    L->starts = lm_starts_layout(ncomp, LM_BATCH_RES, hist_cap, L->nfree, T.ws_doubles, p->N);
    L->h_free_ptr.assign(free_ptr, free_ptr + ncomp + 1);   // (for lm_starts_tables, at the first multi-start solve)
    if (L->nfree > 0) L->h_free_vid.assign(free_vid, free_vid + L->nfree);
    // the one upload of the plan's life: nothing in the tables depends on x
    std::vector<char> stage(L->lay.bytes);
    lm_batch_stage_tables(T, L->lay, stage.data());
    if ((rc = upload(c, L->tables, stage.data(), stage.size()))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the staging vector ends here)
    *out = L.release();
    return 0;
}

extern "C" void rdis_hip_lm_plan_destroy(rdis_hip_lm_plan* L) {
    if (!L) return;
    if (L->prob) { (void)make_current(L->prob->ctx); (void)hipStreamSynchronize(L->prob->ctx->stream); }
    delete L;
}

extern "C" int rdis_hip_lm_plan_solve(rdis_hip_lm_plan* L, int32_t maxiters, double ftol) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    if (maxiters < 1) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve: maxiters must be positive");
    USE_DEVICE(c);
    const int rc = lm_plan_enqueue(L, p->x.as<double>(), 0, 1, maxiters, ftol);
    if (rc) return rc;
    L->last_kind = 1; L->last_count = 1; L->last_rows = 1;
    return 0;
}

extern "C" int rdis_hip_lm_plan_fetch(rdis_hip_lm_plan* L, double* x_out, double* fret, double* delta, double* info8, double* hist4, int64_t* nhist) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_FETCH, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    return lm_plan_download(L, L->last_rows - 1, 1, x_out, fret, delta, info8, hist4, nhist);   // (after a multi-start solve: the winners' row)
}

extern "C" int rdis_hip_lm_plan_solve_population(rdis_hip_lm_plan* L, rdis_hip_population* pop, int64_t first, int64_t count, int32_t maxiters, double ftol) {
    if (!L || !pop) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    if (maxiters < 1) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve_population: maxiters must be positive");
    const std::string why = lm_member_range_refusal("lm_plan_solve_population", pop->prob == p, first, count, pop->nmembers);
    if (!why.empty()) return fail(c, RDIS_HIP_EINVAL, why);
    if ((double)count * (double)std::max<int64_t>(L->ncomp * std::max<int64_t>(L->hist_cap, 1), 1) >= 1.0e15)
        return fail(c, RDIS_HIP_ERANGE, "lm_plan_solve_population: too many members");
    USE_DEVICE(c);
    pop->eval_valid = false; pop->best_current = false;   // X is written: the values of the last evaluation are stale
    const int rc = lm_plan_enqueue(L, pop->row(first), (long long)p->N, count, maxiters, ftol);
    if (rc) return rc;
    L->last_kind = 2; L->last_count = count; L->last_rows = count;
    return 0;
}

extern "C" int rdis_hip_lm_plan_fetch_population(rdis_hip_lm_plan* L, double* x_out, double* fret, double* delta, double* info8, double* hist4,
                                                 int64_t* nhist) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_FETCH_POPULATION, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    return lm_plan_download(L, 0, L->last_count, x_out, fret, delta, info8, hist4, nhist);
}

// ---- multi-start solves: every component from each of S rows of start values, the problem left at the best start per component ----
namespace {
// What both entries do once their starts are on the device: `src` holds start s's values at src + (first + s) * src_stride, in
// free-list order (by_pos) or by variable id.  Rounds of fill + the class launches on scratch rows, then select and gather.
// After the first call of a size: no allocation; never a wait.
int lm_plan_enqueue_starts(rdis_hip_lm_plan* L, const char* who, int64_t nstarts, const double* src, long long src_stride, bool by_pos, int64_t first,
                           int32_t maxiters, double ftol) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    const LmStartsLayout& Y = L->starts;
    const int64_t rows = Y.out_rows(nstarts);
    int64_t per;
    int rc = lm_plan_size(L, nstarts, Y.out_bytes(nstarts), Y.work, &per);
    if (rc) return rc;
    const int* const pos = L->starts_tables.as<int>();
    const int* const comp_of = pos + p->N;
    double* const xrows = Y.work.at<double>(L->work.p, LM_STARTS_ROWS, per);
    const LmBatchOptions o = lm_batch_options(maxiters, L->R, ftol);
    L->last_kind = 0;   // (what an earlier solve left in `out` is overwritten from here on)
    L->last_per_launch = 0; L->last_launches = 0;
    for (int64_t m0 = 0; m0 < nstarts; m0 += per) {
        const int64_t n = std::min(per, nstarts - m0);
        HIPCHK(c, lm_starts_fill_launch(c->stream, grid_for(c, p->N, 256), xrows, p->N, p->x.as<double>(), pos, src, src_stride, by_pos, first + m0, (int)n));
        if ((rc = lm_plan_launch(L, who, o, Y.work, per, xrows, (long long)p->N, rows, m0, n))) return rc;
    }
    const LmStartsOut O{L->res_dev(rows), L->hist_dev(rows), L->x_dev(rows), Y.out.doubles(LM_PLAN_RES), Y.out.doubles(LM_PLAN_HIST), Y.out.doubles(LM_PLAN_X),
                        (long long)L->hist_cap, LM_BATCH_RES, LM_BATCH_RES_NHIST, reinterpret_cast<int*>(static_cast<char*>(L->out.p) + Y.best_offset(nstarts))};
    HIPCHK(c, lm_starts_select_launch(c->stream, O, nstarts, L->ncomp));
    HIPCHK(c, lm_starts_gather_launch(c->stream, O, nstarts, L->nfree, reinterpret_cast<const int*>(static_cast<const char*>(L->tables.p) + L->lay.free32),
                                      comp_of, p->x.as<double>()));
    L->last_per_launch = per;
    L->last_kind = 3; L->last_count = nstarts; L->last_rows = rows;
    return 0;
}

// pos[N] | comp_of[nfree], built and uploaded at the first multi-start solve (the host image is kept: the upload is asynchronous)
int lm_plan_starts_tables(rdis_hip_lm_plan* L) {
    if (L->starts_tables.p) return 0;
    rdis_hip_problem* p = L->prob;
    std::vector<int32_t> pos, comp_of;
    lm_starts_tables(p->N, L->ncomp, L->h_free_ptr.data(), L->h_free_vid.data(), pos, comp_of);
    L->h_starts_tables = std::move(pos);
    L->h_starts_tables.insert(L->h_starts_tables.end(), comp_of.begin(), comp_of.end());
    return upload(p->ctx, L->starts_tables, L->h_starts_tables);
}

// a start count the outputs can be sized for: rows of int32 ids, byte counts far inside int64
bool lm_plan_starts_sizable(const rdis_hip_lm_plan* L, int64_t nstarts) {
    const double row = (double)std::max<int64_t>(std::max<int64_t>(L->ncomp * (LM_BATCH_RES + 4 * std::max<int64_t>(L->hist_cap, 1)), L->nfree), 1);
    return nstarts < (1ll << 31) - 1 && ((double)nstarts + 1.0) * row < 1.0e15;
}
}  // namespace

extern "C" int rdis_hip_lm_plan_solve_starts(rdis_hip_lm_plan* L, int64_t nstarts, const double* x_starts, int32_t maxiters, double ftol) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    if (maxiters < 1) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve_starts: maxiters must be positive");
    if (nstarts < 1) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve_starts: nstarts must be at least 1");
    if (!x_starts) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve_starts: x_starts is NULL (a row of start values per start)");
    if (!lm_plan_starts_sizable(L, nstarts)) return fail(c, RDIS_HIP_ERANGE, "lm_plan_solve_starts: too many starts");
    if (L->ncomp == 0) return 0;
    USE_DEVICE(c);
    int rc = lm_plan_starts_tables(L);
    if (rc) return rc;
    // the starts: through pinned memory, so that the caller may reuse x_starts the moment this returns and nothing waits
    const size_t in_bytes = (size_t)nstarts * (size_t)L->nfree * sizeof(double);
    if ((rc = ensure(c, L->starts_in, in_bytes))) return rc;
    if (in_bytes > 0 && in_bytes <= STARTS_STAGE_MAX_BYTES) {
        if (L->starts_stage_busy) { HIPCHK(c, hipEventSynchronize(L->starts_stage_ev)); L->starts_stage_busy = false; }
        if (L->starts_stage.bytes < in_bytes && (rc = halloc(c, L->starts_stage, in_bytes))) return rc;
        if (!L->starts_stage_ev) HIPCHK(c, hipEventCreateWithFlags(&L->starts_stage_ev, hipEventDisableTiming));
        std::memcpy(L->starts_stage.p, x_starts, in_bytes);
        HIPCHK(c, hipMemcpyAsync(L->starts_in.p, L->starts_stage.p, in_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(L->starts_stage_ev, c->stream));
        L->starts_stage_busy = true;
    } else if (in_bytes > 0) {
        HIPCHK(c, hipMemcpyAsync(L->starts_in.p, x_starts, in_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return lm_plan_enqueue_starts(L, "lm_plan_solve_starts", nstarts, L->starts_in.as<double>(), (long long)L->nfree, true, 0, maxiters, ftol);
}

extern "C" int rdis_hip_lm_plan_solve_starts_population(rdis_hip_lm_plan* L, rdis_hip_population* pop, int64_t first, int64_t count, int32_t maxiters,
                                                        double ftol) {
    if (!L || !pop) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    if (maxiters < 1) return fail(c, RDIS_HIP_EINVAL, "lm_plan_solve_starts_population: maxiters must be positive");
    const std::string why = lm_member_range_refusal("lm_plan_solve_starts_population", pop->prob == p, first, count, pop->nmembers);
    if (!why.empty()) return fail(c, RDIS_HIP_EINVAL, why);
    if (!lm_plan_starts_sizable(L, count)) return fail(c, RDIS_HIP_ERANGE, "lm_plan_solve_starts_population: too many starts");
    if (L->ncomp == 0) return 0;
    USE_DEVICE(c);
    const int rc = lm_plan_starts_tables(L);
    if (rc) return rc;
    // (the population is read only: its rows, its values and what rdis_hip_population_best answers stay as they are)
    return lm_plan_enqueue_starts(L, "lm_plan_solve_starts_population", count, pop->X.as<double>(), (long long)p->N, false, first, maxiters, ftol);
}

extern "C" int rdis_hip_lm_plan_fetch_starts(rdis_hip_lm_plan* L, double* x_out, double* fret, double* delta, double* info8, double* hist4, int64_t* nhist,
                                             int32_t* best) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_FETCH_STARTS, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    if (best && L->ncomp > 0)   // (on the stream, ahead of the download's wait -- or of this one's, where nothing else is asked for)
        HIPCHK(c, hipMemcpyAsync(best, static_cast<const char*>(L->out.p) + L->starts.best_offset(L->last_count), (size_t)L->ncomp * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, c->stream));
    const int rc = lm_plan_download(L, 0, L->last_count, x_out, fret, delta, info8, hist4, nhist);
    if (rc) return rc;
    if (best && L->ncomp > 0) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_lm_plan_objective_device(rdis_hip_lm_plan* L, void** dev_ptr) {
    if (!L || !dev_ptr) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_OBJECTIVE_DEVICE, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    if (!L->objective.p) { const int rc = dalloc(c, L->objective, sizeof(double)); if (rc) return rc; }
    HIPCHK(c, lm_plan_objective_launch(c->stream, L->ncomp, L->ncomp > 0 ? L->res_dev(L->last_rows, L->last_rows - 1) : nullptr, LM_BATCH_RES,
                                       L->objective.as<double>()));
    *dev_ptr = L->objective.p;
    return 0;
}

static_assert(RDIS_HIP_LM_SUMMARY_DOUBLES == LM_SUMMARY_DOUBLES, "the summary block of rdis_hip.h and lm_starts.hpp");

extern "C" int rdis_hip_lm_plan_summary_device(rdis_hip_lm_plan* L, void** dev_ptr) {
    if (!L || !dev_ptr) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_SUMMARY_DEVICE, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    if (!L->summary.p) { const int rc = dalloc(c, L->summary, sizeof(double) * LM_SUMMARY_DOUBLES); if (rc) return rc; }
    // the ordinary outputs' result rows, a component's stride as lm_plan_layout lays a row of them out
    const long long stride = L->ncomp > 0 ? L->layout.out.doubles(LM_PLAN_RES) / L->ncomp : 0;
    HIPCHK(c, lm_plan_summary_launch(c->stream, L->ncomp, L->ncomp > 0 ? L->res_dev(L->last_rows, L->last_rows - 1) : nullptr, stride, L->summary.as<double>()));
    *dev_ptr = L->summary.p;
    return 0;
}

extern "C" int rdis_hip_lm_plan_summary(rdis_hip_lm_plan* L, double* out16) {
    if (!L || !out16) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    void* dev = nullptr;
    const int rc = rdis_hip_lm_plan_summary_device(L, &dev);
    if (rc) return rc;
    USE_DEVICE(c);
    return lm_read_back(c, L->summary_pin, L->summary_pin_failed, dev, sizeof(double) * LM_SUMMARY_DOUBLES, out16);
}

// The summary per member of the last population solve: one launch over the whole range (the outputs of a solve that was split by
// workspace_bytes lie in one block all the same), one workgroup per member.
extern "C" int rdis_hip_lm_plan_summary_population_device(rdis_hip_lm_plan* L, void** dev_ptr) {
    if (!L || !dev_ptr) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    if (const char* why = lm_read_refusal(LM_READ_SUMMARY_POPULATION_DEVICE, L->last_kind)) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    const int64_t count = L->last_count;
    const int rc = ensure(c, L->member_summary, (size_t)count * sizeof(double) * LM_SUMMARY_DOUBLES);
    if (rc) return rc;
    const long long member_stride = L->layout.out.doubles(LM_PLAN_RES);
    const long long stride = L->ncomp > 0 ? member_stride / L->ncomp : 0;
    HIPCHK(c, lm_plan_summary_members_launch(c->stream, count, L->ncomp, L->ncomp > 0 ? L->res_dev(L->last_rows) : nullptr, member_stride, stride,
                                             L->member_summary.as<double>()));
    *dev_ptr = L->member_summary.p;
    return 0;
}

extern "C" int rdis_hip_lm_plan_summary_population(rdis_hip_lm_plan* L, double* out) {
    if (!L || !out) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    void* dev = nullptr;
    const int rc = rdis_hip_lm_plan_summary_population_device(L, &dev);
    if (rc) return rc;
    USE_DEVICE(c);
    return lm_read_back(c, L->member_summary_pin, L->member_summary_pin_failed, dev, (size_t)L->last_count * sizeof(double) * LM_SUMMARY_DOUBLES, out);
}

extern "C" int rdis_hip_lm_plan_set_option(rdis_hip_lm_plan* L, const char* name, int64_t value) {
    if (!L || !name) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    const std::string n(name);
    if (n != "workspace_bytes") return fail(c, RDIS_HIP_EINVAL, "lm_plan_set_option: unknown option '" + n + "' (workspace_bytes)");
    if (value < 0) return fail(c, RDIS_HIP_EINVAL, "lm_plan_set_option: workspace_bytes must be >= 0");
    L->workspace_bytes = value;
    return 0;
}

extern "C" int rdis_hip_lm_plan_get_info(rdis_hip_lm_plan* L, const char* name, int64_t* value) {
    if (!L || !name || !value) return RDIS_HIP_EINVAL;
    const std::string n(name);
    if (n == "members_per_launch") *value = L->last_per_launch;
    else if (n == "launches") *value = L->last_launches;
    else if (n == "device_bytes") *value = (int64_t)(L->tables.bytes + L->out.bytes + L->work.bytes + L->starts_tables.bytes + L->starts_in.bytes + L->objective.bytes + L->summary.bytes);
    else if (n == "workspace_bytes") *value = L->workspace_bytes;
    else if (n == "member_workspace_bytes") *value = L->layout.work.member_bytes();
    else return fail(L->prob->ctx, RDIS_HIP_EINVAL, "lm_plan_get_info: unknown name '" + n + "' (members_per_launch, launches, device_bytes, workspace_bytes, "
                                                    "member_workspace_bytes)");
    return 0;
}
