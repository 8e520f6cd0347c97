// population_entries.hip -- the C ABI's population entries (include/rdis_hip.h: rdis_hip_population_*): S complete states on the
// device, their storage, evaluation, argmin, gradients, options, and what a restart loop does between two solves (draw, rank,
// reorder).  Host code only: every launch goes through a *_launch function of population_kernels.hip or grad_fused.hip, and no
// header with a kernel is seen from here.  The rules the entries share are population_rules.hpp's; what they need of the problem
// and evaluation block of rdis_hip.hip is eval_api.hpp's.  The plan's solves on a population stay in rdis_hip.hip
// (solve_population_range), with the launch shapes they need.
#include "abi_state.hpp"

#include <new>

#include "eval_api.hpp"
#include "population_api.hpp"
#include "population_grid.hpp"
#include "population_rules.hpp"
#include "population_state.hpp"

namespace {
int population_range(rdis_hip_population* pop, const char* who, int64_t first, int64_t count, int64_t n, const int64_t* vid) {
    const PopulationRefusal r = population_range_refusal(who, first, count, n, vid != nullptr, pop->nmembers, pop->prob->N);
    return r.code ? fail(pop->prob->ctx, r.code, r.message) : 0;
}
}  // namespace

extern "C" int rdis_hip_population_create(rdis_hip_problem* p, int64_t nmembers, const double* x, rdis_hip_population** out) {
    if (!p || !out) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    USE_DEVICE(c);
    if (nmembers < 1) return fail(c, RDIS_HIP_EINVAL, "population_create: nmembers must be at least 1");
    if (too_many_rows(nmembers, std::max<int64_t>(p->N, 1)))
        return fail(c, RDIS_HIP_ERANGE, "population_create: too many members");
    rdis_hip_population* pop = new (std::nothrow) rdis_hip_population;
    if (!pop) return fail(c, RDIS_HIP_ENOMEM, "population_create: host allocation");
    pop->prob = p; pop->nmembers = nmembers;
    const size_t bytes = (size_t)nmembers * (size_t)p->N * sizeof(double);
    int rc = dalloc(c, pop->X, bytes);
    if (!rc) rc = dalloc(c, pop->f, (size_t)nmembers * sizeof(double));
    if (rc) { delete pop; return rc; }
    hipError_t e = hipSuccess;
    if (bytes > 0) {
        if (x) e = hipMemcpyAsync(pop->X.p, x, bytes, hipMemcpyHostToDevice, c->stream);
        else e = population_copy_rows_launch(c->stream, p->x.as<double>(), pop->X.as<double>(), p->N, nmembers);   // every member: the assigned x
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { delete pop; return fail(c, RDIS_HIP_EDEVICE, std::string("population_create: ") + hipGetErrorString(e)); }
    *out = pop;
    return 0;
}

extern "C" void rdis_hip_population_destroy(rdis_hip_population* pop) {
    if (!pop) return;
    if (pop->prob) { (void)make_current(pop->prob->ctx); (void)hipStreamSynchronize(pop->prob->ctx->stream); }
    delete pop;
}

extern "C" int rdis_hip_population_set_x(rdis_hip_population* pop, int64_t first, int64_t count, int64_t n, const int64_t* vid, const double* val) {
    if (!pop || n < 0 || (n && count > 0 && !val)) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    int rc = population_range(pop, "population_set_x", first, count, n, vid);
    if (rc) return rc;
    if (n == 0 || count == 0) return 0;
    USE_DEVICE(c);
    pop->x_written();
    const size_t bytes = (size_t)count * (size_t)n * sizeof(double);
    if (!vid && n == p->N) {   // whole rows: straight into place
        HIPCHK(c, hipMemcpyAsync(pop->row(first), val, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    const int* dv;
    if ((rc = problem_stage_ids(p, n, vid, p->N, &dv))) return rc;
    if ((rc = ensure(c, pop->tmp_val, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(pop->tmp_val.p, val, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, population_scatter_launch(c->stream, pop->X.as<double>(), p->N, first, count, dv, n, pop->tmp_val.as<double>()));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_population_get_x(rdis_hip_population* pop, int64_t first, int64_t count, int64_t n, const int64_t* vid, double* out) {
    if (!pop || n < 0 || (n && count > 0 && !out)) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    int rc = population_range(pop, "population_get_x", first, count, n, vid);
    if (rc) return rc;
    if (n == 0 || count == 0) return 0;
    USE_DEVICE(c);
    const size_t bytes = (size_t)count * (size_t)n * sizeof(double);
    if (!vid && n == p->N) return read_back(c, out, pop->row(first), bytes);
    const int* dv;
    if ((rc = problem_stage_ids(p, n, vid, p->N, &dv))) return rc;
    if ((rc = ensure(c, pop->tmp_out, bytes))) return rc;
    HIPCHK(c, population_pick_launch(c->stream, pop->X.as<double>(), p->N, first, count, dv, n, pop->tmp_out.as<double>()));
    return read_back(c, out, pop->tmp_out.p, bytes);
}

extern "C" int rdis_hip_population_assign(rdis_hip_population* pop, int64_t member) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    if (member < 0 || member >= pop->nmembers) return fail(c, RDIS_HIP_EINVAL, "population_assign: member out of range");
    USE_DEVICE(c);
    HIPCHK(c, population_copy_rows_launch(c->stream, pop->row(member), p->x.as<double>(), p->N, 1));
    return 0;
}

namespace {
// f[s] for every member, enqueued on the context's stream: pop->f on the device, nothing waited for.
// Batched (the default): the member is the grid's second dimension -- per launch of R members (population_grid.hpp) the rotation
// records of ITS members on the records branch (a replica serves another member in the next launch: rebuilt before every launch,
// the invariant of solver_quad_population.hpp), the chunk or block sums, one final-sum workgroup per member.  The branch, the
// chunk size and the block count are enqueue_eval's, so f[s] has rdis_hip_eval's bits.  The scratch is the population's: the
// problem's x, scalar, partial and xrot are not written.
int population_eval_enqueue(rdis_hip_population* pop, int64_t nf, const int* dfac) {
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    const int64_t S_n = pop->nmembers;
    int rc;
    pop->x_written();   // (f is written: until the launches below are enqueued it holds no evaluation of X)
    if (nf == 0) {
        HIPCHK(c, hipMemsetAsync(pop->f.p, 0, (size_t)S_n * sizeof(double), c->stream));
        pop->eval_per_launch = S_n; pop->eval_launches = 0; pop->eval_valid = true;
        return 0;
    }
    const bool fused = fused_path(p), records = fused && nf >= 4 * p->ncam_blocks;
    if (!pop->eval_batched) {
        // member by member, rdis_hip_eval's kernels with the view's x replaced, through the problem's partial / xrot
        for (int64_t s = 0; s < S_n; ++s)
            if ((rc = problem_enqueue_eval(p, pop->row(s), nf, dfac, pop->f.as<double>() + s))) return rc;
        pop->eval_per_launch = 1; pop->eval_launches = S_n * (records ? 3 : 2); pop->eval_valid = true;
        return 0;
    }
    const int64_t per = fused ? (nf + GRAD_LANES - 1) / GRAD_LANES : grid_for(c, nf, 256);   // a member's partials: chunks, or enqueue_eval's blocks
    const ReplicaLayout partials = population_eval_partial_layout(per), xr = population_eval_xr_layout(records, p->N);
    const int64_t R = members_per_launch(S_n, pop->eval_workspace_bytes, partials.member_bytes() + xr.member_bytes());
    if ((rc = ensure(c, pop->eval_partial, (size_t)partials.total_bytes(R)))) return rc;
    if (records && (rc = ensure(c, pop->eval_xr, (size_t)xr.total_bytes(R)))) return rc;
    const ProblemView V = p->view();
    double *X = pop->X.as<double>(), *part = pop->eval_partial.as<double>(), *XR = records ? pop->eval_xr.as<double>() : nullptr;
    int64_t launches = 0;
    for (int64_t first = 0; first < S_n; first += R) {
        const int ns = (int)std::min<int64_t>(R, S_n - first);
        if (fused) {
            if (records) {
                HIPCHK(c, population_rotations_launch(c->stream, X, p->N, first, ns, p->cam_blocks.as<int>(), (int)p->ncam_blocks, XR));
                ++launches;
            }
            HIPCHK(c, population_eval_chunks_launch(c->stream, (int)std::min<int64_t>(per, 16 * std::max(1, c->num_cus)), ns, V, X, first, XR, (int)nf, dfac, part));
        } else {
            HIPCHK(c, population_eval_sum_launch(c->stream, p->kind, (int)per, ns, V, X, first, (int)nf, dfac, part));
        }
        HIPCHK(c, population_final_sum_launch(c->stream, ns, (int)per, part, first, pop->f.as<double>()));
        launches += 2;
    }
    pop->eval_per_launch = R; pop->eval_launches = launches; pop->eval_valid = true;
    return 0;
}

// the argmin of the last evaluation, left in pop->best (enqueued; once per evaluation)
int population_select(rdis_hip_population* pop, int reader) {
    rdis_hip_ctx* c = pop->prob->ctx;
    if (!pop->eval_valid) return fail(c, RDIS_HIP_EINVAL, population_no_values_refusal(reader));
    if (pop->best_current) return 0;
    int rc;
    if ((rc = ensure(c, pop->best, sizeof(MemberValue)))) return rc;
    HIPCHK(c, population_argmin_launch(c->stream, (long long)pop->nmembers, pop->f.as<double>(), pop->best.as<MemberValue>()));
    pop->best_current = true;
    return 0;
}
}  // namespace

extern "C" int rdis_hip_population_eval_device(rdis_hip_population* pop, int64_t nf, const int64_t* fac, void** f_dev) {
    if (!pop || !f_dev) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    const int* dfac = nullptr;
    if (nf > 0 && (rc = problem_stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    if ((rc = population_eval_enqueue(pop, nf, dfac))) return rc;
    *f_dev = pop->f.p;
    return 0;
}

extern "C" int rdis_hip_population_eval(rdis_hip_population* pop, int64_t nf, const int64_t* fac, double* f) {
    if (!pop || !f) return RDIS_HIP_EINVAL;
    void* fd;
    int rc = rdis_hip_population_eval_device(pop, nf, fac, &fd);
    if (rc) return rc;
    return read_back(pop->prob->ctx, f, fd, (size_t)pop->nmembers * sizeof(double));
}

extern "C" int rdis_hip_population_best(rdis_hip_population* pop, int64_t* member, double* f) {
    if (!pop || !member || !f) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = pop->prob->ctx;
    USE_DEVICE(c);
    if (int rc = population_select(pop, POPULATION_READ_BEST)) return rc;
    MemberValue b;
    if (int rc = read_back(c, &b, pop->best.p, sizeof b)) return rc;
    *member = (int64_t)b.s; *f = b.f;
    return 0;
}

extern "C" int rdis_hip_population_assign_best(rdis_hip_population* pop) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    USE_DEVICE(c);
    if (int rc = population_select(pop, POPULATION_READ_ASSIGN_BEST)) return rc;
    if (p->N > 0)
        HIPCHK(c, population_copy_best_launch(c->stream, grid_for(c, p->N, 256), pop->X.as<double>(), (long long)p->N, pop->best.as<MemberValue>(), p->x.as<double>()));
    return 0;
}

namespace {
// Value and gradient of members first0 .. first0 + count - 1 (count >= 1), enqueued on the context's stream: pop->grad_f[count]
// and pop->grad_g[count][N] on the device.  Nothing is waited for but what grad_plan_for / stage_ids / the upload of an explicit
// list's gather lists wait for.  The member is the grid's second dimension; the branch is rdis_hip_eval_grad's (grad_branch_of),
// the kernels its kernels with the member's row for x, so row k has the bits of rdis_hip_eval_grad at X[first0 + k].
// Per round of R members (population_grid.hpp) every member has a replica of the per-call arrays in pop->grad_ws.  A replica
// serves another member in the next round, and every entry a round reads it has written itself:
//   fused:    the camera records are rebuilt before EVERY round; the fused kernel writes every cstage / pstage slot and every
//             chunk's sum before the combine kernel and the final sum read them (each slot belongs to one (block, chunk / tile));
//   short, two-pass: the gather lists name only slots of listed factors, which the round's partials have written.
// The scratch is the population's: X, f, eval_valid and best, the problem's x, scalar, g_all, camrec, partial, gfac and xrot and
// the cached GradPlan's own staging arrays are not written (its tables are read).
int population_grad_enqueue(rdis_hip_population* pop, int64_t first0, int64_t count, int64_t nf, const int64_t* fac) {
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    const int64_t N = p->N;
    int rc;
    if ((rc = refuse_exponential(p, nf, fac, "population_eval_grad"))) return rc;
    const int branch = grad_branch_of(p, nf, fac);
    // what the branch needs of the list, before anything of the last call is overwritten
    GradPlan* G = nullptr;
    GradMemberShape shape;
    size_t dyn = 0;
    const int *dfac = nullptr, *dptr = nullptr, *didx = nullptr;
    int blocks = 0;
    if (branch == GRAD_BRANCH_FUSED) {
        if ((rc = grad_plan_for(p, nf, fac, &G))) return rc;
        dyn = grad_lds_bytes(G->T.ncam_cap);
        if (dyn > (size_t)160 * 1024) return fail(c, RDIS_HIP_EINVAL, "population_eval_grad: a tile's cameras do not fit the LDS");
        shape.ncam_blocks = p->ncam_blocks; shape.cstage_slots = G->cstage_slots; shape.pstage_slots = G->pstage_slots; shape.nchunks = G->T.nchunks;
    } else if (branch != GRAD_BRANCH_NONE) {
        if ((rc = problem_stage_ids(p, nf, fac, p->F, &dfac))) return rc;
        blocks = branch == GRAD_BRANCH_SHORT ? 1 : grid_for(c, nf, 256);   // a member's value partials: the one chunk's, or eval_grad_two_pass's blocks
        shape.nslots = p->nslots(); shape.blocks = blocks;
        if (!fac) {
            if ((rc = all_factors_v2s(p, &dptr, &didx))) return rc;
        } else {   // built once per call, kept by the population: the launches below read them after this call has returned
            ivec ptr, idx;
            build_v2s(p, nf, fac, ptr, idx);
            if ((rc = ensure(c, pop->grad_v2s_ptr, ptr.size() * sizeof(int))) || (rc = ensure(c, pop->grad_v2s_idx, idx.size() * sizeof(int)))) return rc;
            HIPCHK(c, hipMemcpyAsync(pop->grad_v2s_ptr.p, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            if (!idx.empty()) HIPCHK(c, hipMemcpyAsync(pop->grad_v2s_idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host images go out of scope)
            dptr = pop->grad_v2s_ptr.as<int>(); didx = pop->grad_v2s_idx.as<int>();
        }
    }
    const ReplicaLayout ws = grad_member_layout(branch, shape);
    const int64_t R = branch == GRAD_BRANCH_NONE ? count : members_per_launch(count, pop->grad_workspace_bytes, ws.member_bytes());
    if ((rc = ensure(c, pop->grad_f, (size_t)count * sizeof(double)))) return rc;
    if ((rc = ensure(c, pop->grad_g, (size_t)count * (size_t)N * sizeof(double)))) return rc;
    if (branch != GRAD_BRANCH_NONE && (rc = ensure(c, pop->grad_ws, (size_t)ws.total_bytes(R)))) return rc;
    pop->grad_rows = count; pop->grad_per_launch = R; pop->grad_launches = 0; pop->grad_branch = branch;
    double *X = pop->X.as<double>(), *F_out = pop->grad_f.as<double>(), *G_out = pop->grad_g.as<double>(), *W = pop->grad_ws.as<double>();
    if (branch == GRAD_BRANCH_NONE) {
        HIPCHK(c, hipMemsetAsync(F_out, 0, (size_t)count * sizeof(double), c->stream));
        if (N > 0) HIPCHK(c, hipMemsetAsync(G_out, 0, (size_t)count * (size_t)N * sizeof(double), c->stream));
        return 0;
    }
    const ProblemView V = p->view();
    int64_t launches = 0;
    if (branch == GRAD_BRANCH_FUSED) {
        const GradTables& T = G->T;
        GradReplicas rep;
        rep.camrec = ws.at<double>(W, GRAD_FUSED_CAMREC, R); rep.camrec_stride = ws.doubles(GRAD_FUSED_CAMREC);
        rep.cstage = ws.at<double>(W, GRAD_FUSED_CSTAGE, R); rep.cstage_stride = ws.doubles(GRAD_FUSED_CSTAGE);
        rep.pstage = ws.at<double>(W, GRAD_FUSED_PSTAGE, R); rep.pstage_stride = ws.doubles(GRAD_FUSED_PSTAGE);
        rep.partial = ws.at<double>(W, GRAD_FUSED_PARTIAL, R); rep.partial_stride = ws.doubles(GRAD_FUSED_PARTIAL);   // (T.nchunks: at least one)
        const long long items = 9ll * T.ncs + 3ll * T.nps + T.nz;
        for (int64_t k = 0; k < count; k += R) {   // (rounds on one stream: the next takes the replicas when this one is done)
            const int ns = (int)std::min<int64_t>(R, count - k);
            const int64_t first = first0 + k;
            // the records of THIS round's members: the replicas held another round's until now
            HIPCHK(c, population_grad_camera_records_launch(c->stream, ns, X, N, first, p->cam_blocks.as<int>(), (int)p->ncam_blocks, rep.camrec, rep.camrec_stride));
            HIPCHK(c, population_grad_fused_launch(c->stream, ns, dyn, T, X, N, first, p->obs.as<double2>(), rep, G_out, k));
            if (items > 0) HIPCHK(c, population_grad_combine_launch(c->stream, grid_for(c, items, 256), ns, T, rep, G_out, N, k));
            // (population_final_sum_kernel adds a member's nchunks partials by final_sum_of, final_sum_kernel's own sum: the same order)
            HIPCHK(c, population_final_sum_launch(c->stream, ns, T.nchunks, rep.partial, k, F_out));
            launches += items > 0 ? 4 : 3;
        }
    } else {
        const long long nslots = ws.doubles(GRAD_LIST_GFAC);
        double *gfac = ws.at<double>(W, GRAD_LIST_GFAC, R), *part = ws.at<double>(W, GRAD_LIST_PARTIAL, R);   // [R][nslots], [R][blocks]
        for (int64_t k = 0; k < count; k += R) {
            const int ns = (int)std::min<int64_t>(R, count - k);
            const int64_t first = first0 + k;
            if (branch == GRAD_BRANCH_SHORT)
                HIPCHK(c, population_partials_launch(c->stream, grid_for(c, nf, 256), ns, V, X, first, (int)nf, dfac, gfac, nslots));
            else
                HIPCHK(c, population_eval_sum_grad_launch(c->stream, p->kind, blocks, ns, V, X, first, (int)nf, dfac, gfac, nslots, part));
            HIPCHK(c, population_gather_grad_launch(c->stream, grid_for(c, N, 256), ns, (int)N, dptr, didx, gfac, nslots, G_out, k));
            if (branch == GRAD_BRANCH_SHORT) {   // the value by the chunk kernel, as eval_grad_short takes it
                HIPCHK(c, population_eval_chunks_launch(c->stream, 1, ns, V, X, first, nullptr, (int)nf, dfac, part));
                ++launches;
            }
            HIPCHK(c, population_final_sum_launch(c->stream, ns, blocks, part, k, F_out));
            launches += 3;
        }
    }
    pop->grad_launches = launches;
    return 0;
}
}  // namespace

extern "C" int rdis_hip_population_eval_grad_device(rdis_hip_population* pop, int64_t first, int64_t count, int64_t nf, const int64_t* fac, void** f_dev,
                                                    void** g_dev) {
    if (!pop || !f_dev || !g_dev) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    int rc = population_range(pop, "population_eval_grad", first, count, p->N, nullptr);
    if (!rc) rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if (count > 0 && (rc = population_grad_enqueue(pop, first, count, nf, fac))) return rc;   // (count == 0: nothing happens)
    *f_dev = pop->grad_f.p;
    *g_dev = pop->grad_g.p;
    return 0;
}

extern "C" int rdis_hip_population_eval_grad(rdis_hip_population* pop, int64_t first, int64_t count, int64_t nf, const int64_t* fac, double* f, double* g) {
    if (!pop || (count > 0 && (!f || !g))) return RDIS_HIP_EINVAL;
    void *fd, *gd;
    int rc = rdis_hip_population_eval_grad_device(pop, first, count, nf, fac, &fd, &gd);
    if (rc || count == 0) return rc;
    rdis_hip_ctx* c = pop->prob->ctx;
    if (pop->prob->N > 0) HIPCHK(c, hipMemcpyAsync(g, gd, (size_t)count * (size_t)pop->prob->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return read_back(c, f, fd, (size_t)count * sizeof(double));   // (one wait for both copies)
}

extern "C" int rdis_hip_population_grad_max(rdis_hip_population* pop, double* gmax, void** gmax_dev) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = pop->prob->ctx;
    if (pop->grad_rows < 0)
        return fail(c, RDIS_HIP_EINVAL, "population_grad_max: evaluate the gradient first (rdis_hip_population_eval_grad or _eval_grad_device)");
    USE_DEVICE(c);
    const int64_t rows = pop->grad_rows;
    if (int rc = ensure(c, pop->grad_gmax, (size_t)rows * sizeof(double))) return rc;
    HIPCHK(c, population_grad_max_launch(c->stream, rows, (long long)pop->prob->N, pop->grad_g.as<double>(), pop->grad_gmax.as<double>()));
    if (gmax_dev) *gmax_dev = pop->grad_gmax.p;
    return gmax ? read_back(c, gmax, pop->grad_gmax.p, (size_t)rows * sizeof(double)) : 0;
}

extern "C" int rdis_hip_population_set_option(rdis_hip_population* pop, const char* name, int64_t value) {
    if (!pop || !name) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = pop->prob->ctx;
    const std::string n(name);
    if (n == "eval_workspace_bytes") {
        if (value < 0) return fail(c, RDIS_HIP_EINVAL, "population_set_option: eval_workspace_bytes must not be negative");
        USE_DEVICE(c);
        pop->eval_workspace_bytes = value;
        if (pop->eval_partial.bytes + pop->eval_xr.bytes > (size_t)value) {   // scratch beyond the new bound goes (the next evaluation takes what it needs)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            pop->eval_partial.release(); pop->eval_xr.release();
        }
    } else if (n == "eval_batched") {
        pop->eval_batched = value != 0;
    } else if (n == "grad_workspace_bytes") {
        if (value < 0) return fail(c, RDIS_HIP_EINVAL, "population_set_option: grad_workspace_bytes must not be negative");
        USE_DEVICE(c);
        pop->grad_workspace_bytes = value;
        if (pop->grad_ws.bytes > (size_t)value) {   // scratch beyond the new bound goes (the next gradient call takes what it needs)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            pop->grad_ws.release();
        }
    } else {
        return fail(c, RDIS_HIP_EINVAL, "population_set_option: unknown option '" + n + "' (eval_workspace_bytes, eval_batched, grad_workspace_bytes)");
    }
    return 0;
}

extern "C" int rdis_hip_population_get_info(rdis_hip_population* pop, const char* name, int64_t* value) {
    if (!pop || !name || !value) return RDIS_HIP_EINVAL;
    const std::string n(name);
    if (n == "eval_members_per_launch") *value = pop->eval_per_launch;
    else if (n == "eval_launches") *value = pop->eval_launches;
    else if (n == "eval_valid") *value = pop->eval_valid ? 1 : 0;
    else if (n == "grad_members_per_launch") *value = pop->grad_per_launch;
    else if (n == "grad_launches") *value = pop->grad_launches;
    else if (n == "grad_branch") *value = pop->grad_branch;
    else if (n == "nmembers") *value = pop->nmembers;
    else if (n == "problem_handle") *value = (int64_t)reinterpret_cast<intptr_t>(pop->prob);   // (to compare with the caller's rdis_hip_problem*)
    else return fail(pop->prob->ctx, RDIS_HIP_EINVAL, "population_get_info: unknown name '" + n + "' (eval_members_per_launch, eval_launches, eval_valid, "
                                                     "grad_members_per_launch, grad_launches, grad_branch, nmembers, problem_handle)");
    return 0;
}

// ---- what a restart loop does between two solves: draw, rank, keep (population_select.hpp) ----

extern "C" int rdis_hip_population_set_sampling(rdis_hip_population* pop, const double* lo, const double* hi) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    if (!lo && !hi) { pop->sampling_set = false; return 0; }   // the problem's domains again (the buffers stay: a later call reuses them)
    const std::string why = population_sampling_refusal(lo, hi, p->N);
    if (!why.empty()) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    const size_t bytes = (size_t)p->N * sizeof(double);
    int rc;
    if ((rc = ensure(c, pop->slo, bytes)) || (rc = ensure(c, pop->shi, bytes))) return rc;
    if (bytes > 0) {
        HIPCHK(c, hipMemcpyAsync(pop->slo.p, lo, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(pop->shi.p, hi, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (copied once: the caller's arrays are free again)
    }
    pop->sampling_set = true;
    return 0;
}

extern "C" int rdis_hip_population_sample(rdis_hip_population* pop, int64_t first, int64_t count, int64_t n, const int64_t* vid, uint64_t seed,
                                          int64_t stream) {
    if (!pop || n < 0) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = pop->prob;
    rdis_hip_ctx* c = p->ctx;
    if (stream < 0 || stream > 2147483646ll) return fail(c, RDIS_HIP_EINVAL, "population_sample: stream out of range (0 ... 2^31 - 2)");
    int rc = population_range(pop, "population_sample", first, count, n, vid);
    if (rc) return rc;
    if (n == 0 || count == 0) return 0;
    USE_DEVICE(c);
    const int* dv;
    if ((rc = problem_stage_ids(p, n, vid, p->N, &dv))) return rc;
    pop->x_written();
    const double *lo = p->lo.as<double>(), *hi = p->hi.as<double>();
    HIPCHK(c, population_sample_launch(c->stream, pop->X.as<double>(), p->N, first, count, dv, n, (unsigned long long)seed, stream,
                                       pop->sampling_set ? pop->slo.as<double>() : lo, pop->sampling_set ? pop->shi.as<double>() : hi, lo, hi));
    return 0;
}

namespace {
static_assert(sizeof(long long) == sizeof(int64_t), "order is copied in and out as it lies");
// What population_sort and population_permute share.  The buffers: the second one of X's size, the permuted values and the
// order, at the first reorder, in this order (a failure leaves the population as it was: nothing has been launched).
int reorder_buffers(rdis_hip_population* pop) {
    rdis_hip_ctx* c = pop->prob->ctx;
    int rc;
    if ((rc = ensure(c, pop->X2, pop->X.bytes)) || (rc = ensure(c, pop->f2, (size_t)pop->nmembers * sizeof(double))) ||
        (rc = ensure(c, pop->order, (size_t)pop->nmembers * sizeof(long long))))
        return rc;
    return 0;
}
// The application of pop->order: X_new[r] = X_old[order[r]], f likewise.  X and X2 swap roles (every entry reads pop->X when it
// is called, and the stream orders the work); f keeps its address -- what population_eval_device handed out stays valid -- and
// takes the permuted values (stale ones stay stale: eval_valid is left as it is).  The argmin has moved: selected again when
// it is asked for.
int reorder_apply(rdis_hip_population* pop) {
    rdis_hip_ctx* c = pop->prob->ctx;
    const int64_t S_n = pop->nmembers;
    HIPCHK(c, population_permute_rows_launch(c->stream, S_n, pop->prob->N, pop->order.as<long long>(), pop->X.as<double>(), pop->f.as<double>(),
                                             pop->X2.as<double>(), pop->f2.as<double>()));
    std::swap(pop->X.p, pop->X2.p);
    std::swap(pop->X.bytes, pop->X2.bytes);
    HIPCHK(c, hipMemcpyAsync(pop->f.p, pop->f2.p, (size_t)S_n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    pop->best_current = false;
    return 0;
}
}  // namespace

extern "C" int rdis_hip_population_sort(rdis_hip_population* pop, int64_t* order_out) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = pop->prob->ctx;
    const int64_t S_n = pop->nmembers;
    if (S_n > (1ll << 18))
        return fail(c, RDIS_HIP_ERANGE, "population_sort: rank by counting is quadratic in the members: at most 2^18 = 262144 (this population has " +
                                        std::to_string(S_n) + ")");
    if (!pop->eval_valid) return fail(c, RDIS_HIP_EINVAL, population_no_values_refusal(POPULATION_READ_SORT));
    USE_DEVICE(c);
    int rc;
    if ((rc = reorder_buffers(pop))) return rc;
    HIPCHK(c, population_rank_launch(c->stream, S_n, pop->f.as<double>(), pop->order.as<long long>()));
    if ((rc = reorder_apply(pop))) return rc;   // (the argmin is member 0 now; eval_valid stays set)
    return order_out ? read_back(c, order_out, pop->order.p, (size_t)S_n * sizeof(int64_t)) : 0;
}

// X_new[r] = X_old[order[r]] for an order the caller chose (population_sort: the order of the values): the sort's permute kernel
// and second buffer.  The list is checked on the host -- a permutation, nothing less -- before anything is allocated or launched.
extern "C" int rdis_hip_population_permute(rdis_hip_population* pop, const int64_t* order) {
    if (!pop) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = pop->prob->ctx;
    if (!order) return fail(c, RDIS_HIP_EINVAL, "population_permute: order is NULL (order[r]: the row that becomes row r)");
    const std::string why = population_permutation_refusal(order, pop->nmembers);
    if (!why.empty()) return fail(c, RDIS_HIP_EINVAL, why);
    USE_DEVICE(c);
    if (int rc = reorder_buffers(pop)) return rc;
    HIPCHK(c, hipMemcpyAsync(pop->order.p, order, (size_t)pop->nmembers * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (staged: the caller's array is free again)
    return reorder_apply(pop);
}
