// rdis_hip.hip -- implementation of the C ABI in include/rdis_hip.h: handle
// management, uploads, plan construction (validation + gather lists) and kernel
// launches.  gfx950 only; no CPU evaluation path exists in this library.  The collectives (comm.hip), a plan's queries
// (plan_query.hip), the Levenberg-Marquardt entries (lm_api.hip) and the population entries (population_entries.hip) are host-only
// translation units of their own; abi_state.hpp is what the five share.
#include "abi_state.hpp"
#include "eval_api.hpp"
#include "population_rules.hpp"
#include "population_state.hpp"

#include <array>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <new>
#include <numeric>

#include "eval_kernels.hpp"
#include "grad_tables.hpp"
#include "refround_api.hpp"
#include "solver_coop.hpp"
#include "solver_coop_population.hpp"
#include "solver_lds.hpp"
#include "population_api.hpp"
#include "population_grid.hpp"
#include "solver_pipe.hpp"
#include "solver_quad.hpp"
#include "solver_stream.hpp"

using namespace rdis_hip;

// what abi_state.hpp and plan_options.hpp restate of the headers above for the translation units that do not see them
static_assert(PLAN_INDEX_EINVAL == RDIS_HIP_EINVAL && PLAN_INDEX_EOVERLAP == RDIS_HIP_EOVERLAP && PLAN_INDEX_ERANGE == RDIS_HIP_ERANGE &&
              PLAN_INDEX_KIND_BA == KIND_BA && GRAD_TABLES_NO_ENTRY == GRAD_NO_ENTRY, "a restated constant differs from its original");
// grad_tables.hpp's pairs are uploaded as the int2 that grad_fused.hpp's tables name
static_assert(sizeof(IntPair) == sizeof(int2) && offsetof(IntPair, x) == offsetof(int2, x) && offsetof(IntPair, y) == offsetof(int2, y),
              "IntPair is not laid out as int2");
static_assert(ABI_LDS_MAX_BYTES == LDS_MAX_BYTES && ABI_PIPE_TM == PIPE_TM && OPTION_QUAD_MAX_VARS == QUAD_MAX_VARS &&
              OPTION_COOP_MAX_WG == COOP_MAX_WG && OPTION_PTM_MAX_GROUP == PTM_WIDE_MAX_GROUP && GRAD_MEMBER_REC == GRAD_REC &&
              REPLICA_PT_REC == PT_REC, "a restated constant differs from its original");
static_assert(sizeof(CoopState) % 32 == 0, "population_coop_layout keeps every state of ms_coop on 32 bytes");

// The one place that knows there are two roundings: a solver's launches in the default rounding (fused multiply-adds), and
// the set to use (refround_api.hpp).  A plan asks with coop_reference_rounding() or batch_reference_rounding().
static const SolverSet& solver_set(bool reference_rounding) {
    static const SolverSet fused = {launch_pipe, launch_coop, pipe_max_workgroups, coop_max_workgroups, launch_lds,
                                    launch_coop_population, coop_population_max_workgroups};
    return reference_rounding ? refround_solvers() : fused;
}

// (the plan's methods that need a solver header)
int rdis_hip_plan::coop_lanes() const { return pipelined() ? PIPE_LANES : coop_threads; }
bool rdis_hip_plan::lds_matrix_on(const rdis_hip_ctx* c) const {
    return lds_matrix != 0 && !emulate_stale && factor_rounding != 1 &&
           lds_matrix_offset(lds_bytes_for(lds_ns_cap, lds_ncb_cap, lds_chunk_cap)) + lds_matrix_bytes(lds_ncb_cap) <= c->lds_limit;
}
size_t rdis_hip_plan::lds_dyn_bytes(const rdis_hip_ctx* c) const {
    const size_t base = lds_bytes_for(lds_ns_cap, lds_ncb_cap, lds_chunk_cap);
    return lds_matrix_on(c) ? lds_matrix_offset(base) + lds_matrix_bytes(lds_ncb_cap) : base;
}


// =====================================================================================
// context
// =====================================================================================
extern "C" int rdis_hip_abi_version(void) { return RDIS_HIP_ABI_VERSION; }

extern "C" int rdis_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return (n > 0 && virtual_devices() > 0) ? virtual_devices() : n;
}

extern "C" int rdis_hip_create(int device, rdis_hip_ctx** out) {
    if (!out) return RDIS_HIP_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= (virtual_devices() > 0 ? virtual_devices() : n)) return RDIS_HIP_EDEVICE;
    rdis_hip_ctx* c = new (std::nothrow) rdis_hip_ctx;
    if (!c) return RDIS_HIP_ENOMEM;
    c->device = device;
    c->phys = virtual_devices() > 0 ? 0 : device;
    hipDeviceProp_t prop;
    if (make_current(c) != hipSuccess || hipGetDeviceProperties(&prop, c->phys) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return RDIS_HIP_EDEVICE;
    }
    c->own_stream = true;
    c->num_cus = prop.multiProcessorCount;
    if (prop.maxSharedMemoryPerMultiProcessor > 4096)
        c->lds_limit = std::min<size_t>((size_t)LDS_MAX_BYTES, (size_t)prop.maxSharedMemoryPerMultiProcessor - 4096);
    *out = c;
    return 0;
}

extern "C" void rdis_hip_destroy(rdis_hip_ctx* c) {
    if (!c) return;
    (void)make_current(c);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    delete c;
}

extern "C" const char* rdis_hip_last_error(const rdis_hip_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" int rdis_hip_set_stream(rdis_hip_ctx* c, void* s) {
    if (!c) return RDIS_HIP_EINVAL;
    USE_DEVICE(c);
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (s) { c->stream = (hipStream_t)s; c->own_stream = false; }
    else {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return 0;
}

extern "C" int rdis_hip_synchronize(rdis_hip_ctx* c) {
    if (!c) return RDIS_HIP_EINVAL;
    USE_DEVICE(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_copy_to_host(rdis_hip_ctx* c, void* dst, const void* src, int64_t bytes) {
    if (!c || bytes < 0 || (bytes && (!dst || !src))) return RDIS_HIP_EINVAL;
    if (bytes == 0) return 0;
    USE_DEVICE(c);
    return read_back(c, dst, src, (size_t)bytes);
}

// =====================================================================================
// problems
// =====================================================================================
namespace {
int upload_common(rdis_hip_ctx* c, rdis_hip_problem* p, int64_t nvars, const double* x0, const double* lo,
                  const double* hi) {
    int rc;
    if ((rc = upload(c, p->x, x0, (size_t)nvars))) return rc;
    if ((rc = upload(c, p->lo, lo, (size_t)nvars))) return rc;
    if ((rc = upload(c, p->hi, hi, (size_t)nvars))) return rc;
    if ((rc = dalloc(c, p->scalar, 64))) return rc;
    return 0;
}
}  // namespace

extern "C" int rdis_hip_upload_ba(rdis_hip_ctx* c, int64_t nvars, const double* x0, const double* lo,
                                  const double* hi, int64_t nfac, const int64_t* cam_vid0,
                                  const int64_t* pt_vid0, const double* obs, rdis_hip_problem** out) {
    if (!c || !out || nvars < 0 || nfac < 0 || (nvars && (!x0 || !lo || !hi)) ||
        (nfac && (!cam_vid0 || !pt_vid0 || !obs)))
        return fail(c, RDIS_HIP_EINVAL, "upload_ba: bad argument");
    if (nvars >= (1ll << 31) - 16 || nfac >= ((1ll << 31) - 16) / 12) return fail(c, RDIS_HIP_ERANGE, "upload_ba: too large for int32 device indices");
    USE_DEVICE(c);
    rdis_hip_problem* p = new (std::nothrow) rdis_hip_problem;
    if (!p) return fail(c, RDIS_HIP_ENOMEM, "upload_ba: host allocation");
    p->ctx = c; p->kind = KIND_BA; p->N = nvars; p->F = nfac;
    p->h_cam.resize((size_t)nfac); p->h_pt.resize((size_t)nfac);
    for (int64_t i = 0; i < nfac; ++i) {
        if (cam_vid0[i] < 0 || cam_vid0[i] + 9 > nvars || pt_vid0[i] < 0 || pt_vid0[i] + 3 > nvars) {
            delete p;
            return fail(c, RDIS_HIP_EINVAL, "upload_ba: variable id out of range in factor " + std::to_string(i));
        }
        p->h_cam[(size_t)i] = (int)cam_vid0[i];
        p->h_pt[(size_t)i] = (int)pt_vid0[i];
    }
    int rc = upload_common(c, p, nvars, x0, lo, hi);
    if (!rc) rc = upload(c, p->cam, p->h_cam);
    if (!rc) rc = upload(c, p->pt, p->h_pt);
    if (!rc) rc = upload(c, p->obs, obs, (size_t)(2 * nfac));
    ivec blocks;   // (alive until the copies below have completed)
    {   // the distinct camera blocks, for the rotation records of launches that leave the cameras constant
        p->h_block_of.assign((size_t)nvars, -1);
        blocks = p->h_cam;
        std::sort(blocks.begin(), blocks.end());
        blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
        // blocks that overlap without coinciding would share record slots: no records then
        bool disjoint = true;
        for (size_t i = 1; i < blocks.size(); ++i) disjoint = disjoint && blocks[i] - blocks[i - 1] >= 9;
        for (int cb : blocks)
            for (int k = 0; k < 9; ++k) p->h_block_of[(size_t)cb + k] = cb;
        for (int64_t i = 0; i < nfac && disjoint; ++i)   // a point block inside a camera block: likewise
            for (int k = 0; k < 3; ++k) disjoint = disjoint && p->h_block_of[(size_t)p->h_pt[(size_t)i] + k] < 0;
        if (disjoint) {   // the point blocks likewise: coinciding or at least 3 apart
            p->h_ptblock_of.assign((size_t)nvars, -1);
            for (int64_t i = 0; i < nfac && disjoint; ++i) {
                const int q = p->h_pt[(size_t)i];
                for (int k = 0; k < 3; ++k) {
                    int& o = p->h_ptblock_of[(size_t)q + k];
                    disjoint = disjoint && (o < 0 || o == q);
                    o = q;
                }
            }
        }
        p->ncam_blocks = disjoint ? (int64_t)blocks.size() : 0;
        if (!rc && p->ncam_blocks > 0) {
            rc = upload(c, p->cam_blocks, blocks);
            if (!rc) rc = dalloc(c, p->xrot, (size_t)nvars * sizeof(double));
        }
    }
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, RDIS_HIP_EDEVICE, "upload_ba: sync");
    if (rc) { delete p; return rc; }
    *out = p;
    return 0;
}

extern "C" int rdis_hip_upload_nlp(rdis_hip_ctx* c, int64_t nvars, const double* x0, const double* lo,
                                   const double* hi, int64_t nfac, const double* coeff,
                                   const int64_t* rowptr, const int64_t* vid, const double* expo,
                                   const double* cons, const uint8_t* sine, rdis_hip_problem** out) {
    if (!c || !out || nvars < 0 || nfac < 0 || (nvars && (!x0 || !lo || !hi)) || !rowptr || (nfac && !coeff))
        return fail(c, RDIS_HIP_EINVAL, "upload_nlp: bad argument");
    const int64_t nnz = rowptr[nfac];
    if (nnz < 0 || (nnz && (!vid || !expo || !cons || !sine))) return fail(c, RDIS_HIP_EINVAL, "upload_nlp: bad CSR");
    if (nvars >= (1ll << 31) - 16 || nfac >= (1ll << 31) - 16 || nnz >= (1ll << 31) - 16)
        return fail(c, RDIS_HIP_ERANGE, "upload_nlp: too large for int32 device indices");
    USE_DEVICE(c);
    rdis_hip_problem* p = new (std::nothrow) rdis_hip_problem;
    if (!p) return fail(c, RDIS_HIP_ENOMEM, "upload_nlp: host allocation");
    p->ctx = c; p->kind = KIND_NLP; p->N = nvars; p->F = nfac; p->nnz = nnz;
    p->h_rowptr.resize((size_t)nfac + 1); p->h_vid.resize((size_t)nnz);
    for (int64_t i = 0; i <= nfac; ++i) {
        if (rowptr[i] < 0 || (i && rowptr[i] < rowptr[i - 1])) { delete p; return fail(c, RDIS_HIP_EINVAL, "upload_nlp: rowptr not monotone"); }
        p->h_rowptr[(size_t)i] = (int)rowptr[i];
    }
    for (int64_t k = 0; k < nnz; ++k) {
        if (vid[k] < 0 || vid[k] >= nvars) { delete p; return fail(c, RDIS_HIP_EINVAL, "upload_nlp: variable id out of range"); }
        p->h_vid[(size_t)k] = (int)vid[k];
    }
    int rc = upload_common(c, p, nvars, x0, lo, hi);
    if (!rc) rc = upload(c, p->coeff, coeff, (size_t)nfac);
    if (!rc) rc = upload(c, p->rowptr, p->h_rowptr);
    if (!rc) rc = upload(c, p->vid, p->h_vid);
    if (!rc) rc = upload(c, p->expo, expo, (size_t)nnz);
    if (!rc) rc = upload(c, p->cons, cons, (size_t)nnz);
    if (!rc) rc = upload(c, p->sine, sine, (size_t)nnz);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, RDIS_HIP_EDEVICE, "upload_nlp: sync");
    if (rc) { delete p; return rc; }
    *out = p;
    return 0;
}

extern "C" int rdis_hip_nlp_set_exponential(rdis_hip_problem* p, const uint8_t* use_exp) {
    if (!p) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (p->kind != KIND_NLP) return fail(c, RDIS_HIP_EINVAL, "nlp_set_exponential: not a nonlinear-product problem");
    USE_DEVICE(c);
    bool any = false;
    for (int64_t i = 0; use_exp && i < p->F; ++i) any |= use_exp[i] != 0;
    if (!any) { p->h_useexp.clear(); return 0; }
    // (a kernel of an earlier call may still read the old flags: the copy is ordered after it on the stream)
    if (p->useexp.bytes < (size_t)p->F) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (int rc = dalloc(c, p->useexp, (size_t)p->F)) return rc;
    }
    p->h_useexp.assign(use_exp, use_exp + p->F);
    HIPCHK(c, hipMemcpyAsync(p->useexp.p, p->h_useexp.data(), (size_t)p->F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" void rdis_hip_free_problem(rdis_hip_problem* p) {
    if (!p) return;
    (void)make_current(p->ctx);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
}

namespace {
// stage an int64 id list as int32 on the device (nullptr stays nullptr)
int stage_ids(rdis_hip_problem* p, int64_t n, const int64_t* ids, int64_t limit, const int** dev) {
    rdis_hip_ctx* c = p->ctx;
    *dev = nullptr;
    if (!ids) return 0;
    ivec tmp((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= limit) return fail(c, RDIS_HIP_EINVAL, "id out of range");
        tmp[(size_t)i] = (int)ids[i];
    }
    if (p->tmp_idx.bytes < (size_t)n * sizeof(int)) { int rc = dalloc(c, p->tmp_idx, (size_t)n * sizeof(int)); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(p->tmp_idx.p, tmp.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // tmp goes out of scope
    *dev = p->tmp_idx.as<int>();
    return 0;
}
}  // namespace

// (for population_entries.hip, eval_api.hpp)
int rdis_hip::problem_stage_ids(rdis_hip_problem* p, int64_t n, const int64_t* ids, int64_t limit, const int** dev) { return stage_ids(p, n, ids, limit, dev); }

extern "C" int rdis_hip_set_x(rdis_hip_problem* p, int64_t n, const int64_t* vid, const double* val) {
    if (!p || n < 0 || (n && !val)) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (n == 0) return 0;
    USE_DEVICE(c);
    if (!vid) {
        if (n > p->N) return fail(c, RDIS_HIP_EINVAL, "set_x: n > nvars");
        HIPCHK(c, hipMemcpyAsync(p->x.p, val, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    const int* dv;
    int rc = stage_ids(p, n, vid, p->N, &dv);
    if (rc) return rc;
    if ((rc = ensure(c, p->tmp_val, (size_t)n * sizeof(double)))) return rc;
    HIPCHK(c, hipMemcpyAsync(p->tmp_val.p, val, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    scatter_x_kernel<<<grid_for(c, n, 256), 256, 0, c->stream>>>((int)n, dv, p->tmp_val.as<double>(), p->x.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_get_x(rdis_hip_problem* p, int64_t n, const int64_t* vid, double* out) {
    if (!p || n < 0 || (n && !out)) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (n == 0) return 0;
    USE_DEVICE(c);
    if (!vid) {
        if (n > p->N) return fail(c, RDIS_HIP_EINVAL, "get_x: n > nvars");
        HIPCHK(c, hipMemcpyAsync(out, p->x.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    const int* dv;
    int rc = stage_ids(p, n, vid, p->N, &dv);
    if (rc) return rc;
    if ((rc = ensure(c, p->tmp_out, (size_t)n * sizeof(double)))) return rc;
    gather_x_kernel<<<grid_for(c, n, 256), 256, 0, c->stream>>>((int)n, dv, p->x.as<double>(), p->tmp_out.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, p->tmp_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// =====================================================================================
// batched evaluation
// =====================================================================================
// (the functions defined as rdis_hip::... in this block are population_entries.hip's too: eval_api.hpp)

// for every variable the gradient slots that feed it, in factor-list order
void rdis_hip::build_v2s(const rdis_hip_problem* p, int64_t nf, const int64_t* fac, ivec& ptr,
                         ivec& idx) {
    ptr.assign((size_t)p->N + 1, 0);
    for (int64_t i = 0; i < nf; ++i) {
        const int f = (int)(fac ? fac[i] : i);
        for (int k = 0, a = p->arity(f); k < a; ++k) ++ptr[(size_t)p->var_of(f, k) + 1];
    }
    for (int64_t v = 0; v < p->N; ++v) ptr[(size_t)v + 1] += ptr[(size_t)v];
    idx.resize((size_t)ptr[(size_t)p->N]);
    ivec fill(ptr.begin(), ptr.end() - 1);
    for (int64_t i = 0; i < nf; ++i) {
        const int f = (int)(fac ? fac[i] : i);
        for (int k = 0, a = p->arity(f); k < a; ++k) idx[(size_t)fill[(size_t)p->var_of(f, k)]++] = p->slot_of(f, k);
    }
}

int rdis_hip::check_list(rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    if (nf < 0) return fail(p->ctx, RDIS_HIP_EINVAL, "negative factor count");
    if (!fac && nf != p->F) return fail(p->ctx, RDIS_HIP_EINVAL, "fac == NULL requires nf == factor count");
    return 0;
}

// NonlinearProductFactor::computeGradient asserts its factor has no exponential (src/NonlinearProductFactor.cpp:110):
// a gradient or a solve over a list that holds such a factor is refused, not computed from the plain product
int rdis_hip::refuse_exponential(rdis_hip_problem* p, int64_t nf, const int64_t* fac, const char* who) {
    if (p->h_useexp.empty()) return 0;
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t f = fac ? fac[i] : i;
        if (f >= 0 && f < p->F && p->h_useexp[(size_t)f])
            return fail(p->ctx, RDIS_HIP_EINVAL, std::string(who) + ": factor " + std::to_string(f) +
                        " is exponential; the reference's gradient asserts it is not (NonlinearProductFactor.cpp:110)");
    }
    return 0;
}

namespace {
template <bool GRAD>
int launch_eval_sum(rdis_hip_problem* p, const ProblemView& V, int nf, const int* dfac, int blocks, double* out_dev) {
    rdis_hip_ctx* c = p->ctx;
    if (p->kind == KIND_BA)
        eval_sum_kernel<KIND_BA, GRAD><<<blocks, 256, 0, c->stream>>>(V, nf, dfac, p->gfac.as<double>(), p->partial.as<double>());
    else
        eval_sum_kernel<KIND_NLP, GRAD><<<blocks, 256, 0, c->stream>>>(V, nf, dfac, p->gfac.as<double>(), p->partial.as<double>());
    HIPCHK(c, hipGetLastError());
    final_sum_kernel<<<1, 256, 0, c->stream>>>(blocks, p->partial.as<double>(), out_dev);
    HIPCHK(c, hipGetLastError());
    return 0;
}
}  // namespace

bool rdis_hip::fused_path(const rdis_hip_problem* p) { return p->kind == KIND_BA && p->ncam_blocks > 0; }

namespace {

// Factor lists whose tables the problem keeps: up to GRAD_PLAN_CACHE of them within GRAD_PLAN_BYTES of device memory (least
// recently used goes first).  A caller that asks for the gradients of a level's components in turn (computeGradient(facs, pg)
// per component, as the reference does) cycles through dozens of lists: with room for four (round 5) every call rebuilt and
// reallocated its tables.  A list of at most one chunk needs none (eval_grad_short).
constexpr size_t GRAD_PLAN_CACHE = 64;
constexpr size_t GRAD_PLAN_BYTES = (size_t)1 << 30;

// The tables of grad_fused.hpp for one factor list, built once per list: the index work is grad_tables.hpp's; here the tile
// size is chosen, the tables uploaded and the staging arrays allocated.
int build_grad_plan(rdis_hip_problem* p, int64_t nf64, const int64_t* fac, GradPlan& G) {
    rdis_hip_ctx* c = p->ctx;
    const int nf = (int)nf64, GW = GRAD_LANES;
    const int nchunks = (nf + GW - 1) / GW;
    const size_t N = (size_t)p->N, ncb = (size_t)p->ncam_blocks;
    if (p->h_cam_ord.empty()) {   // (camera blocks are the distinct values of h_cam, ascending: their ordinal = their rank)
        p->h_cam_ord.assign(N, -1);
        ivec blocks(p->h_cam);
        std::sort(blocks.begin(), blocks.end());
        blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
        for (size_t i = 0; i < blocks.size(); ++i) p->h_cam_ord[(size_t)blocks[i]] = (int)i;
    }
    // tiles: up to tile_chunks chunks, fewer where their cameras would not fit (a chunk alone always does)
    const int want_tiles = 8 * std::max(1, c->num_cus);
    int tile_chunks = std::max(1, std::min(GRAD_MAX_TILE_CHUNKS, nchunks / want_tiles));
    if (const char* ev = std::getenv("RDIS_HIP_GRAD_TILE_CHUNKS")) tile_chunks = std::max(1, std::min(64, std::atoi(ev)));   // (tuning)
    const int cam_soft = 192;
    GradIndex X;
    grad_tables_build(N, ncb, p->h_cam.data(), p->h_pt.data(), p->h_cam_ord.data(), nf, fac, GW, tile_chunks, cam_soft, X);
    int rc_ = upload(c, G.ints, X.blk);
    if (!rc_) rc_ = upload(c, G.shorts, X.sh.data(), X.sh.size());
    if (!rc_ && fac) {
        ivec f32((size_t)nf);
        for (int j = 0; j < nf; ++j) f32[(size_t)j] = (int)fac[j];
        rc_ = upload(c, G.fac, f32);
        if (!rc_) HIPCHK(c, hipStreamSynchronize(c->stream));   // (f32 goes out of scope)
    }
    if (!rc_) rc_ = dalloc(c, G.cstage, (size_t)std::max(X.cstage_slots, 1) * 9 * sizeof(double));
    if (!rc_) rc_ = dalloc(c, G.pstage, (size_t)std::max(X.pstage_slots, 1) * 3 * sizeof(double));
    if (!rc_) rc_ = dalloc(c, G.partial, (size_t)std::max(nchunks, 1) * sizeof(double));
    if (rc_) {   // (the uploads above are asynchronous copies out of host vectors that go out of scope with this call)
        (void)hipStreamSynchronize(c->stream);
        return rc_;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host images go out of scope)
    const int* I = G.ints.as<int>();
    const unsigned short* S = G.shorts.as<unsigned short>();
    GradTables& T = G.T;
    const size_t npad = X.npad;
    T.nf = nf; T.nchunks = nchunks; T.ntiles = X.ntiles; T.ncam_cap = X.ncam_cap;
    T.fac = fac ? G.fac.as<int>() : nullptr;
    T.cl = S; T.rc = S + npad; T.rp = S + 2 * npad;
    T.ptv = I + X.o_ptv; T.tile_chunk0 = I + X.o_tc0; T.tile_cam0 = I + X.o_tm0; T.tile_cam = reinterpret_cast<const int2*>(I + X.o_tcam);
    T.chunk_cseg0 = I + X.o_cs0; T.cseg = reinterpret_cast<const int2*>(I + X.o_cseg);
    T.chunk_pseg0 = I + X.o_ps0; T.pseg = reinterpret_cast<const int2*>(I + X.o_pseg);
    T.ncs = X.ncs; T.nps = X.nps; T.nz = X.nz;
    T.cs_var = I + X.o_csv; T.cs_ptr = I + X.o_csp; T.ps_var = I + X.o_psv; T.ps_ptr = I + X.o_psp; T.zvar = I + X.o_z;
    G.nf = nf64;
    G.cstage_slots = X.cstage_slots; G.pstage_slots = X.pstage_slots;
    return 0;
}
}  // namespace

// the tables of a list: found among the problem's (by two hashes of the ids) or built
int rdis_hip::grad_plan_for(rdis_hip_problem* p, int64_t nf, const int64_t* fac, GradPlan** out) {
    unsigned long long k0 = 0, k1 = 0;
    if (fac) {
        k0 = 1469598103934665603ull; k1 = 0x9E3779B97F4A7C15ull;
        for (int64_t i = 0; i < nf; ++i) {
            const unsigned long long v = (unsigned long long)fac[i];
            if (fac[i] < 0 || fac[i] >= p->F) return fail(p->ctx, RDIS_HIP_EINVAL, "id out of range");
            k0 = (k0 ^ v) * 1099511628211ull;
            k1 = (k1 + v + 0x632BE59BD9B4E019ull) * 0xFF51AFD7ED558CCDull; k1 ^= k1 >> 29;
        }
        if (k0 == 0 && k1 == 0) k1 = 1;
    }
    for (auto& g : p->grad_plans)
        if (g->nf == nf && g->key0 == k0 && g->key1 == k1 &&
            (fac ? g->ids.size() == (size_t)nf && std::memcmp(g->ids.data(), fac, (size_t)nf * sizeof(int64_t)) == 0 : g->ids.empty())) {
            g->used = ++p->grad_tick; *out = g.get(); return 0;
        }
    auto held = [&]() { size_t b = 0; for (auto& g : p->grad_plans) b += g->device_bytes(); return b; };
    bool synced = false;
    while (!p->grad_plans.empty() && (p->grad_plans.size() >= GRAD_PLAN_CACHE || held() > GRAD_PLAN_BYTES)) {
        size_t lru = 0;
        for (size_t i = 1; i < p->grad_plans.size(); ++i) if (p->grad_plans[i]->used < p->grad_plans[lru]->used) lru = i;
        if (!synced) { HIPCHK(p->ctx, hipStreamSynchronize(p->ctx->stream)); synced = true; }   // (a launch that reads its tables may be in flight)
        p->grad_plans.erase(p->grad_plans.begin() + (long)lru);
    }
    std::unique_ptr<GradPlan> G(new (std::nothrow) GradPlan);
    if (!G) return fail(p->ctx, RDIS_HIP_ENOMEM, "eval_grad: host allocation");
    int rc;
    try { rc = build_grad_plan(p, nf, fac, *G); } catch (const std::bad_alloc&) { return fail(p->ctx, RDIS_HIP_ENOMEM, "eval_grad: host allocation"); }
    if (rc) return rc;
    G->key0 = k0; G->key1 = k1; G->used = ++p->grad_tick;
    if (fac) G->ids.assign(fac, fac + nf);
    *out = G.get();
    p->grad_plans.push_back(std::move(G));
    return 0;
}

// the gather lists of all factors, built at their first use and kept by the problem
int rdis_hip::all_factors_v2s(rdis_hip_problem* p, const int** dptr, const int** didx) {
    rdis_hip_ctx* c = p->ctx;
    if (!p->have_all_v2s) {
        int rc;
        ivec ptr, idx;
        build_v2s(p, p->F, nullptr, ptr, idx);
        if ((rc = upload(c, p->all_v2s_ptr, ptr))) return rc;
        if ((rc = upload(c, p->all_v2s_idx, idx))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        p->have_all_v2s = true;
    }
    *dptr = p->all_v2s_ptr.as<int>(); *didx = p->all_v2s_idx.as<int>();
    return 0;
}

// the form a list's value + gradient takes (population_grid.hpp: GradBranch): the one rule of rdis_hip_eval_grad and of
// rdis_hip_population_eval_grad
int rdis_hip::grad_branch_of(const rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    if (nf == 0) return GRAD_BRANCH_NONE;
    if (fused_path(p) && fac && nf <= GRAD_LANES) return GRAD_BRANCH_SHORT;
    return fused_path(p) ? GRAD_BRANCH_FUSED : GRAD_BRANCH_TWO_PASS;
}

namespace {
// value and gradient of a list, left on the device: p->scalar[0] and p->g_all[N] (asynchronous on the context's stream)
int eval_grad_fused(rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    rdis_hip_ctx* c = p->ctx;
    GradPlan* G = nullptr;
    int rc = grad_plan_for(p, nf, fac, &G);
    if (rc) return rc;
    if ((rc = ensure(c, p->g_all, (size_t)p->N * sizeof(double)))) return rc;
    if ((rc = ensure(c, p->camrec, (size_t)p->ncam_blocks * GRAD_REC * sizeof(double)))) return rc;
    const GradTables& T = G->T;
    const size_t dyn = grad_lds_bytes(T.ncam_cap);
    if (dyn > (size_t)160 * 1024) return fail(c, RDIS_HIP_EINVAL, "eval_grad: a tile's cameras do not fit the LDS");
    HIPCHK(c, grad_camera_records_launch(c->stream, (int)((p->ncam_blocks + 255) / 256), p->x.as<double>(), p->cam_blocks.as<int>(),
                                         (int)p->ncam_blocks, p->camrec.as<double>()));
    HIPCHK(c, grad_fused_launch(c->stream, T.ntiles, dyn, T, p->x.as<double>(), p->obs.as<double2>(), p->camrec.as<double>(),
                                G->cstage.as<double>(), G->pstage.as<double>(), G->partial.as<double>(), p->g_all.as<double>()));
    const long long items = 9ll * T.ncs + 3ll * T.nps + T.nz;
    if (items > 0) HIPCHK(c, grad_combine_launch(c->stream, grid_for(c, items, 256), T, G->cstage.as<double>(), G->pstage.as<double>(), p->g_all.as<double>()));
    final_sum_kernel<<<1, 256, 0, c->stream>>>(T.nchunks, G->partial.as<double>(), p->scalar.as<double>());
    HIPCHK(c, hipGetLastError());
    return 0;
}

// the two-pass form (nonlinear-product functions; bundle adjustment whose blocks overlap): per-factor partials, then one
// lane per variable adds its slots in factor-list order
int eval_grad_two_pass(rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    rdis_hip_ctx* c = p->ctx;
    int rc;
    const int* dfac;
    if ((rc = stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    // gather lists: cached for the all-factors case
    const int *dptr, *didx;
    DevBuf lptr, lidx;
    if (!fac) {
        if ((rc = all_factors_v2s(p, &dptr, &didx))) return rc;
    } else {
        ivec ptr, idx;
        build_v2s(p, nf, fac, ptr, idx);
        if ((rc = upload(c, lptr, ptr))) return rc;
        if ((rc = upload(c, lidx, idx))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dptr = lptr.as<int>(); didx = lidx.as<int>();
    }
    const int blocks = grid_for(c, nf, 256);
    if ((rc = ensure(c, p->partial, (size_t)blocks * sizeof(double)))) return rc;
    if ((rc = ensure(c, p->gfac, (size_t)p->nslots() * sizeof(double)))) return rc;
    if ((rc = ensure(c, p->g_all, (size_t)p->N * sizeof(double)))) return rc;
    if ((rc = launch_eval_sum<true>(p, p->view(), (int)nf, dfac, blocks, p->scalar.as<double>()))) return rc;
    gather_grad_kernel<<<grid_for(c, p->N, 256), 256, 0, c->stream>>>((int)p->N, dptr, didx, p->gfac.as<double>(), p->g_all.as<double>());
    HIPCHK(c, hipGetLastError());
    if (fac) HIPCHK(c, hipStreamSynchronize(c->stream));   // (lptr / lidx go out of scope)
    return 0;
}

// A list of at most one chunk (GRAD_LANES entries: a component's handful of factors, a single factor) needs no tables: the
// per-factor partials, then one lane per variable adds its slots in list order -- which for one chunk is exactly the order of the
// fused pass (one chunk, one tile: every block's rows in list order), the same bits; the value by the chunk kernel rdis_hip_eval
// uses, the same bits too.  What the fused form would pay for such a list is its table build: six arrays over all N variables,
// half a dozen allocations, three uploads and two or three synchronisations (advisor, round 5).
int eval_grad_short(rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    rdis_hip_ctx* c = p->ctx;
    int rc;
    const int* dfac;
    if ((rc = stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    ivec ptr, idx;
    build_v2s(p, nf, fac, ptr, idx);
    DevBuf lptr, lidx;
    if ((rc = upload(c, lptr, ptr))) return rc;
    if ((rc = upload(c, lidx, idx))) { (void)hipStreamSynchronize(c->stream); return rc; }
    if ((rc = ensure(c, p->partial, sizeof(double)))) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (!rc) rc = ensure(c, p->gfac, (size_t)p->nslots() * sizeof(double));
    if (!rc) rc = ensure(c, p->g_all, (size_t)p->N * sizeof(double));
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    ProblemView V = p->view();
    partials_kernel<KIND_BA><<<grid_for(c, nf, 256), 256, 0, c->stream>>>(V, (int)nf, dfac, p->gfac.as<double>());
    HIPCHK(c, hipGetLastError());
    gather_grad_kernel<<<grid_for(c, p->N, 256), 256, 0, c->stream>>>((int)p->N, lptr.as<int>(), lidx.as<int>(), p->gfac.as<double>(), p->g_all.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, eval_chunks_launch(c->stream, 1, V, (int)nf, dfac, p->partial.as<double>()));
    final_sum_kernel<<<1, 256, 0, c->stream>>>(1, p->partial.as<double>(), p->scalar.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (lptr / lidx and the host vectors go out of scope)
    return 0;
}

int eval_grad_on_device(rdis_hip_problem* p, int64_t nf, const int64_t* fac) {
    if (int rc = refuse_exponential(p, nf, fac, "eval_grad")) return rc;
    const int branch = grad_branch_of(p, nf, fac);
    if (branch == GRAD_BRANCH_NONE) {
        rdis_hip_ctx* c = p->ctx;
        int rc = ensure(c, p->g_all, (size_t)p->N * sizeof(double));
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(p->g_all.p, 0, (size_t)p->N * sizeof(double), c->stream));
        HIPCHK(c, hipMemsetAsync(p->scalar.p, 0, sizeof(double), c->stream));
        return 0;
    }
    if (branch == GRAD_BRANCH_SHORT) return eval_grad_short(p, nf, fac);
    return branch == GRAD_BRANCH_FUSED ? eval_grad_fused(p, nf, fac) : eval_grad_two_pass(p, nf, fac);
}

}  // namespace

namespace {
// the value of the listed factors (dfac on the device, null: all) at x -- the problem's assigned x or a population member's --
// enqueued on the context's stream; the result is one double at out_dev.  p->partial and, for a long bundle-adjustment list,
// p->xrot are scratch of the call.
int enqueue_eval(rdis_hip_problem* p, double* x, int64_t nf, const int* dfac, double* out_dev) {
    rdis_hip_ctx* c = p->ctx;
    int rc;
    ProblemView V = p->view();
    V.x = x;
    if (fused_path(p)) {
        // chunk by chunk, the chunks' sums added in a fixed order: the value rdis_hip_eval_grad returns, bit for bit
        const int nchunks = (int)((nf + GRAD_LANES - 1) / GRAD_LANES);
        if ((rc = ensure(c, p->partial, (size_t)nchunks * sizeof(double)))) return rc;
        if (nf >= 4 * p->ncam_blocks) {   // a long list: the cameras' rotation records once per camera instead of once per factor (the same bits)
            camera_rotations_kernel<<<(int)((p->ncam_blocks + 255) / 256), 256, 0, c->stream>>>(x, p->cam_blocks.as<int>(), (int)p->ncam_blocks,
                                                                                                p->xrot.as<double>());
            V.xrot = p->xrot.as<double>(); V.rot_mode = ROT_CAMFIX;
        }
        HIPCHK(c, eval_chunks_launch(c->stream, std::min(nchunks, 16 * std::max(1, c->num_cus)), V, (int)nf, dfac, p->partial.as<double>()));
        final_sum_kernel<<<1, 256, 0, c->stream>>>(nchunks, p->partial.as<double>(), out_dev);
        HIPCHK(c, hipGetLastError());
    } else {
        const int blocks = grid_for(c, nf, 256);
        if ((rc = ensure(c, p->partial, (size_t)blocks * sizeof(double)))) return rc;
        if ((rc = launch_eval_sum<false>(p, V, (int)nf, dfac, blocks, out_dev))) return rc;
    }
    return 0;
}
}  // namespace

// The two kernels of a population's gradient that stay in eval_kernels.hpp (they compile to other text elsewhere), launched for
// population_entries.hip (population_api.hpp): grid (grid, members_of_launch)
hipError_t rdis_hip::population_partials_launch(hipStream_t stream, int grid, int members_of_launch, const ProblemView& P, double* X, long long first, int nf,
                                                const int* fac, double* gfac, long long nslots) {
    population_partials_kernel<<<dim3((unsigned)grid, (unsigned)members_of_launch), 256, 0, stream>>>(P, X, first, nf, fac, gfac, nslots);
    return hipGetLastError();
}
hipError_t rdis_hip::population_eval_sum_grad_launch(hipStream_t stream, int kind, int grid, int members_of_launch, const ProblemView& P, double* X,
                                                     long long first, int nf, const int* fac, double* gfac, long long nslots, double* partial) {
    const dim3 g((unsigned)grid, (unsigned)members_of_launch);
    if (kind == KIND_BA) population_eval_sum_grad_kernel<KIND_BA><<<g, 256, 0, stream>>>(P, X, first, nf, fac, gfac, nslots, partial);
    else population_eval_sum_grad_kernel<KIND_NLP><<<g, 256, 0, stream>>>(P, X, first, nf, fac, gfac, nslots, partial);
    return hipGetLastError();
}

// (for population_entries.hip's member-by-member evaluation, eval_api.hpp)
int rdis_hip::problem_enqueue_eval(rdis_hip_problem* p, double* x, int64_t nf, const int* dfac, double* out_dev) { return enqueue_eval(p, x, nf, dfac, out_dev); }

extern "C" int rdis_hip_eval(rdis_hip_problem* p, int64_t nf, const int64_t* fac, double* f) {
    if (!p || !f) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if (nf == 0) { *f = 0.0; return 0; }
    const int* dfac;
    if ((rc = stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    if ((rc = enqueue_eval(p, p->x.as<double>(), nf, dfac, p->scalar.as<double>()))) return rc;
    HIPCHK(c, hipMemcpyAsync(f, p->scalar.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_eval_grad(rdis_hip_problem* p, int64_t nf, const int64_t* fac, double* f, double* g) {
    if (!p || !f || !g) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if (nf == 0) { *f = 0.0; std::fill(g, g + p->N, 0.0); return 0; }
    if ((rc = eval_grad_on_device(p, nf, fac))) return rc;
    HIPCHK(c, hipMemcpyAsync(f, p->scalar.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(g, p->g_all.p, (size_t)p->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_eval_grad_device(rdis_hip_problem* p, int64_t nf, const int64_t* fac, void** f_dev, void** g_dev) {
    if (!p || !f_dev || !g_dev) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if ((rc = eval_grad_on_device(p, nf, fac))) return rc;
    *f_dev = p->scalar.p;
    *g_dev = p->g_all.p;
    return 0;
}

extern "C" int rdis_hip_set_factor_rounding(rdis_hip_problem* p, int32_t mode) {
    if (!p) return RDIS_HIP_EINVAL;
    if (mode != 0 && mode != 1) return fail(p->ctx, RDIS_HIP_EINVAL, "set_factor_rounding: 0 (fused multiply-adds) or 1 (the reference's rounding)");
    if (mode == 1 && p->kind != KIND_BA) return fail(p->ctx, RDIS_HIP_EINVAL, "set_factor_rounding: bundle adjustment only");
    p->each_rounding = mode;
    return 0;
}

extern "C" int rdis_hip_eval_each(rdis_hip_problem* p, int64_t nf, const int64_t* fac, double* fvals) {
    if (!p || (nf && !fvals)) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if (nf == 0) return 0;
    const int* dfac;
    if ((rc = stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    if ((rc = ensure(c, p->tmp_out, (size_t)nf * sizeof(double)))) return rc;
    ProblemView V = p->view();
    const int blocks = grid_for(c, nf, 256);
    if (p->kind == KIND_BA && p->each_rounding == 1) HIPCHK(c, refround_eval_each(blocks, c->stream, V, (int)nf, dfac, p->tmp_out.as<double>()));
    else if (p->kind == KIND_BA) eval_each_kernel<KIND_BA><<<blocks, 256, 0, c->stream>>>(V, (int)nf, dfac, p->tmp_out.as<double>());
    else eval_each_kernel<KIND_NLP><<<blocks, 256, 0, c->stream>>>(V, (int)nf, dfac, p->tmp_out.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(fvals, p->tmp_out.p, (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_grad_each_ba(rdis_hip_problem* p, int64_t nf, const int64_t* fac, double* g12) {
    if (!p || (nf && !g12)) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (p->kind != KIND_BA) return fail(c, RDIS_HIP_EINVAL, "grad_each_ba: not a bundle-adjustment problem");
    int rc = check_list(p, nf, fac);
    if (rc) return rc;
    USE_DEVICE(c);
    if (nf == 0) return 0;
    const int* dfac;
    if ((rc = stage_ids(p, nf, fac, p->F, &dfac))) return rc;
    if ((rc = ensure(c, p->gfac, (size_t)p->nslots() * sizeof(double)))) return rc;
    if ((rc = ensure(c, p->tmp_out, (size_t)nf * 12 * sizeof(double)))) return rc;
    ProblemView V = p->view();
    if (p->each_rounding == 1) {
        HIPCHK(c, refround_grad_each(grid_for(c, nf, 256), c->stream, V, (int)nf, dfac, p->tmp_out.as<double>()));
    } else {
        partials_kernel<KIND_BA><<<grid_for(c, nf, 256), 256, 0, c->stream>>>(V, (int)nf, dfac, p->gfac.as<double>());
        HIPCHK(c, hipGetLastError());
        gather_rows12_kernel<<<grid_for(c, nf * 12, 256), 256, 0, c->stream>>>((int)nf, dfac, p->gfac.as<double>(), p->tmp_out.as<double>());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(g12, p->tmp_out.p, (size_t)nf * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// =====================================================================================
// plans
// =====================================================================================
namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr size_t DIRECT_X_BYTES = 4u << 20;    // a result vector this long is copied straight into the caller's array (rdis_hip_plan_fetch)
constexpr size_t PINNED_OUT_MAX_BYTES = 64u << 20;   // a resident plan's host image of its results block is pinned up to this size
constexpr size_t STAGE_MAX_BYTES = 1u << 20;   // start points staged through pinned memory up to this size (resident plans)

// plan memory: a persistent plan owns hipMalloc'ed buffers; a transient one (cgd_batch, i.e.
// one optimize() call) carves them out of the problem's arena so that a call costs no
// hipMalloc / hipFree (each of which synchronises the device)
int plan_alloc(rdis_hip_plan* L, DevBuf& b, size_t bytes) {
    rdis_hip_problem* p = L->prob;
    if (!L->transient) {
        L->dev_bytes -= std::min(L->dev_bytes, b.owned ? b.bytes : 0);
        const int rc = dalloc(p->ctx, b, bytes);
        if (!rc) L->dev_bytes += b.bytes;
        return rc;
    }
    b.release();
    bytes = align_up(std::max<size_t>(bytes, 8), 256);
    // (the arena is sized from bounds, plan_create_impl; what exceeds them -- rare shapes -- gets memory of its own)
    if (p->arena_used + bytes > p->arena.bytes) return dalloc(p->ctx, b, bytes);
    b.p = static_cast<char*>(p->arena.p) + p->arena_used;
    b.bytes = bytes;
    b.owned = false;
    p->arena_used += bytes;
    return 0;
}

int ensure_problem_scratch(rdis_hip_problem* p) {
    rdis_hip_ctx* c = p->ctx;
    if (!p->dir.p) {
        int rc = dalloc(c, p->dir, (size_t)p->N * sizeof(double));
        if (!rc) rc = dalloc(c, p->coop_state, coop_state_bytes());
        if (!rc) rc = dalloc(c, p->coop_timing, PIPE_TM * sizeof(long long));
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(p->dir.p, 0, p->dir.bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(p->coop_timing.p, 0, p->coop_timing.bytes, c->stream));
        HIPCHK(c, hipEventCreate(&p->ev0));
        HIPCHK(c, hipEventCreate(&p->ev1));
        p->h_mark.assign((size_t)p->N, VarMark{0, -1, -1, 0});
        p->h_local.assign((size_t)p->N, -1);
        p->h_owner_stamp.assign((size_t)p->N, 0);
        p->h_fac_stamp.assign((size_t)p->F, 0);
    }
    return 0;
}

}  // namespace

int rdis_hip::problem_scratch(rdis_hip_problem* p) { return ensure_problem_scratch(p); }   // (for lm_api.hip's table building)

static int plan_create_impl(rdis_hip_problem* p, bool transient, int64_t ncomp, const int64_t* free_ptr,
                            const int64_t* free_vid, const int64_t* fac_ptr, const int64_t* fac_id,
                            rdis_hip_plan** out) {
    if (!p || !out || ncomp < 0 || !free_ptr || !fac_ptr) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    *out = nullptr;
    const int64_t nfree = free_ptr[ncomp], nfac = fac_ptr[ncomp];
    std::string why;
    if (int rc = plan_index_check(ncomp, free_ptr, free_vid, fac_ptr, fac_id, &why)) return fail(c, rc, why);
    if (int rc = refuse_exponential(p, nfac, fac_id, "plan_create")) return rc;
    USE_DEVICE(c);
    int rc = ensure_problem_scratch(p);
    if (rc) return rc;

    rdis_hip_plan* L = new (std::nothrow) rdis_hip_plan;
    if (!L) return fail(c, RDIS_HIP_ENOMEM, "plan_create: host allocation");
    struct Guard { rdis_hip_plan* l; ~Guard() { if (l) rdis_hip_plan_destroy(l); } } guard{L};
    L->prob = p; L->transient = transient; L->ncomp = ncomp; L->nfree = nfree; L->nfac = nfac;
    // (A/B runs of callers that cannot reach the plan's options, e.g. rdis_hip_cgd_batch: RDIS_HIP_COOP_PIPELINE=0 / 1)
    if (const char* ev = std::getenv("RDIS_HIP_COOP_PIPELINE")) L->coop_pipeline = std::atoi(ev) != 0;

    // the lists checked for independence and laid out as the plan's tables (plan_index.hpp)
    const IndexArrays P{p->kind, p->N, p->F, p->h_cam.data(), p->h_pt.data(), p->h_rowptr.data(), p->h_vid.data(),
                        p->h_block_of.data(), p->ncam_blocks, p->h_mark.data(), p->h_fac_stamp.data(), ++p->stamp};
    if ((rc = plan_index_build(P, ncomp, free_ptr, free_vid, fac_ptr, fac_id, *L, &why))) return fail(c, rc, why);
    const ivec& blk = L->h_blk;

    const size_t nc = (size_t)ncomp;
    L->out_bytes = ((size_t)nfree + 2 * nc) * 8 + 2 * nc * 8 + 3 * nc * 4;
    if (transient) {
        // everything this call can need, including what prepare_partition adds for the cooperative solver
        const size_t lanes_max = (size_t)COOP_MAX_WG * 512;
        size_t need = 4096 + 16 * 256;
        need += align_up(blk.size() * 4, 256) + align_up((size_t)(5 * nfree) * 8, 256) + align_up((size_t)L->ngfac * 8, 256);
        need += align_up((size_t)nfree * 8, 256) + align_up(L->out_bytes, 256) + 256;
        need += align_up(nc * 4, 256) + align_up((size_t)nfree * 8, 256);                       // rest_order, xi_glob
        need += align_up((size_t)nfree * 4, 256) + 8 * 256;                                      // long_vars of streaming components
        // lane_var / wave_var of the cooperative groups: at most 3 x the lanes a component needs, rounded up to workgroups
        need += 5 * (3 * (size_t)(nfac + nfree) + 2048 * (size_t)std::min<int64_t>(ncomp, 4096)) + align_up(lanes_max * 4, 256);
        need += align_up((size_t)(12 * nfac) * 4, 256) + 8 * 256;                               // slot_li of all cooperative components
        need += align_up((size_t)(2 * (12 * nfac + 9 * nfree) + 2 * nfac + 64 * (nfac / 64 + std::min<int64_t>(nfac, nfree / 9 + 1) + ncomp) + 3 * ncomp + 3) * 4, 256) + align_up((size_t)nfac * 16, 256) + 256;   // slot tables, observations of the LDS-resident solver
        need += align_up((size_t)(2 * nfac + nfree / 3 + 3 * ncomp + 16) * 4, 256) + align_up((size_t)(nfac + 1) * 20, 256) + align_up((size_t)(24 * nfac + 6 * nfree + 16 * ncomp + 2048) * 8, 256);   // ... of the streaming solver (records, point-major arrays, camera partials)
        need += (size_t)COOP_MAX_GROUPS * (4 * 256 + sizeof(CoopGroup)) + (size_t)COOP_MAX_WG * 4 + lanes_max * 4 + 64 * 256;  // groups, their alignment slack
        if (p->arena.bytes < need) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            rc = dalloc(c, p->arena, std::max(need, 2 * p->arena.bytes));
            if (rc) return rc;
        }
        p->arena_used = 0;
    }
    rc = plan_alloc(L, L->ints, blk.size() * sizeof(int));
    if (!rc) rc = plan_alloc(L, L->ws, (size_t)(5 * nfree) * sizeof(double));
    if (!rc) rc = plan_alloc(L, L->gfac, (size_t)L->ngfac * sizeof(double));
    if (!rc) rc = plan_alloc(L, L->xstart, (size_t)nfree * sizeof(double));
    if (!rc) rc = plan_alloc(L, L->outbuf, L->out_bytes);
    if (!rc) rc = plan_alloc(L, L->objective, 64);
    if (rc) return rc;
    if (!transient && L->out_bytes > 0) {
        // (a result vector of DIRECT_X_BYTES and more goes straight into the caller's array or is not fetched at all)
        const size_t base = (size_t)nfree * 8 >= DIRECT_X_BYTES ? (size_t)nfree * 8 : 0;
        if (L->out_bytes - base <= PINNED_OUT_MAX_BYTES) {
            const std::string err = c->err;
            if (halloc(c, L->h_pin, L->out_bytes - base) == 0) L->h_pin_base = base;
            else { (void)hipGetLastError(); c->err = err; }   // no pinned memory: the pageable block below, and no error
        }
    }
    if (!L->h_pin.p) L->h_out.resize(L->out_bytes);
    if (!blk.empty()) HIPCHK(c, hipMemcpyAsync(L->ints.p, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    guard.l = nullptr;
    *out = L;
    return 0;
}

extern "C" int rdis_hip_plan_create(rdis_hip_problem* p, int64_t ncomp, const int64_t* free_ptr,
                                    const int64_t* free_vid, const int64_t* fac_ptr, const int64_t* fac_id,
                                    rdis_hip_plan** out) {
    return plan_create_impl(p, false, ncomp, free_ptr, free_vid, fac_ptr, fac_id, out);
}

extern "C" void rdis_hip_plan_destroy(rdis_hip_plan* L) {
    if (!L) return;
    if (L->prob) (void)make_current(L->prob->ctx);
    if (L->prob && !L->transient) (void)hipStreamSynchronize(L->prob->ctx->stream);
    delete L;
}

extern "C" int rdis_hip_plan_set_start(rdis_hip_plan* L, const double* xs) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (L->nfree == 0) { L->have_start = true; return 0; }
    if (xs) {
        const size_t bytes = (size_t)L->nfree * sizeof(double);
        rdis_hip_problem* p = L->prob;
        if (!L->transient && bytes <= STAGE_MAX_BYTES) {
            // a resident plan's caller may reuse xs the moment this returns: the values go through a pinned staging
            // buffer of the problem (one host copy, an asynchronous upload) instead of a wait for the stream
            if (p->stage_busy) { HIPCHK(c, hipEventSynchronize(p->stage_ev)); p->stage_busy = false; }
            if (p->stage_x.bytes < bytes) { int rc = halloc(c, p->stage_x, std::max<size_t>(2 * bytes, 4096)); if (rc) return rc; }
            if (!p->stage_ev) HIPCHK(c, hipEventCreateWithFlags(&p->stage_ev, hipEventDisableTiming));
            std::memcpy(p->stage_x.p, xs, bytes);
            HIPCHK(c, hipMemcpyAsync(L->xstart.p, p->stage_x.p, bytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipEventRecord(p->stage_ev, c->stream));
            p->stage_busy = true;
        } else {
            // pageable source: a transient plan's caller keeps xs alive until the results are fetched
            HIPCHK(c, hipMemcpyAsync(L->xstart.p, xs, bytes, hipMemcpyHostToDevice, c->stream));
            if (!L->transient) HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    } else {
        gather_x_kernel<<<grid_for(c, L->nfree, 256), 256, 0, c->stream>>>((int)L->nfree, L->ip(L->off_free_vid), L->prob->x.as<double>(), L->xstart.as<double>());
        HIPCHK(c, hipGetLastError());
    }
    L->have_start = true;
    return 0;
}

extern "C" int rdis_hip_plan_set_option(rdis_hip_plan* L, const char* name, int64_t value) {
    if (!L || !name) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    // Every option's rule, message and effects: plan_options.hpp.  The value goes into a copy of the options first, so that
    // what only the plan can refuse is refused before anything is written.
    PlanOptions next = *L;
    std::string message;
    const PlanOptionRow* row = nullptr;
    const int effect = plan_option_set(next, name, value, &message, &row);
    if (effect < 0) return fail(c, RDIS_HIP_EINVAL, message);
    if ((effect & PLAN_OPTION_DUMP) && (double)value * 2.0 * (double)L->nfree > 4e9) return fail(c, RDIS_HIP_EINVAL, row->refusal);
    if ((effect & PLAN_OPTION_TRACE) && L->transient && value) return fail(c, RDIS_HIP_EINVAL, "tracing needs a persistent plan");
    if ((effect & PLAN_OPTION_DUMP) && L->transient && value) return fail(c, RDIS_HIP_EINVAL, "vector dumps need a persistent plan");
    static_cast<PlanOptions&>(*L) = next;   // the commit: every refusal is above this line, nothing of the plan is written above it
    if (effect & PLAN_OPTION_ROUNDS) L->rounds_threads = L->rounds_K = 0;   // (the round tables are built for one choice)
    if (effect & PLAN_OPTION_LOCAL) L->ptm_local_off = false;
    // (the bound holds from now on: replicas beyond it go; releasing device memory waits for the work that uses it)
    if ((effect & PLAN_OPTION_WORKSPACE) && L->ms_work.bytes + L->ms_ptm.bytes + L->ms_coop.bytes > (size_t)value) {
        for (DevBuf* b : {&L->ms_work, &L->ms_ptm, &L->ms_coop})
            if (b->p) { L->dev_bytes -= std::min(L->dev_bytes, b->bytes); b->release(); }
    }
    if ((effect & PLAN_OPTION_TRACE) && value > 0) {
        int rc = dalloc(c, L->trace, (size_t)L->ncomp * (size_t)value * 4 * sizeof(double));
        if (rc) return rc;
    }
    if ((effect & PLAN_OPTION_DUMP) && value > 0) {
        int rc = dalloc(c, L->vdump, (size_t)value * 2 * (size_t)L->nfree * sizeof(double));
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(L->vdump.p, 0, L->vdump.bytes, c->stream));
    }
    if (effect & PLAN_OPTION_DIRTY) L->partition_dirty = true;
    return 0;
}

namespace {
// ---- prepare_partition: which solver takes each component, and what that solver needs.  The decisions, the allocation and the
// uploads are here, in steps; every index table is built by plan_tables.hpp's host functions (tested without a device).

// what flows between the steps
struct Partition {
    bool coop_on = false, any_big = false;
    int cap = 0, scap = 0;               // workgroups a cooperative launch / the grid solver can have resident
    int64_t group_min = INT64_MAX;       // group mode: every component of at least this many factors gets a cooperative group
    int64_t max_n = 0;                   // running total of the cooperative components' variables
    std::vector<int64_t> nlong_of;       // per component: its variables on long lists (counted once: the layouts are compared)
    cvec wide_comp;                      // per component: it joined the batch list for a wide point-major group
    ivec cams, pts, deg, lane_var, wave_var, sl_own;   // scratch, reused from component to component
    // the slot tables, per component
    cvec kind_of;                        // 1 = LDS-resident, 2 = point-major streaming
    ivec ls_ncb, ls_gcount, pm_pt0, ls_fidx;
    ivec ls_pidx;                        // (host only) a listed factor's point block within its component: all 31 bits of it
    std::vector<ivec> vid_of, free_of, gp_of, pptr_of;
    std::vector<ivec> local_cams;        // per workgroup of the local group: its cameras (component numbers), ascending
    bool local_failed = false;
};

BlockArrays block_arrays(rdis_hip_problem* p) {
    if (p->h_blk_stamp.empty()) { p->h_blk_stamp.assign((size_t)p->N, 0); p->h_blk_idx.assign((size_t)p->N, 0); }
    return BlockArrays{p->h_cam.data(), p->h_pt.data(), p->h_block_of.data(), p->h_ptblock_of.data(),
                       p->h_blk_stamp.data(), p->h_blk_idx.data(), p->h_owner_stamp.data(), p->h_local.data()};
}
CompLists comp_lists(const rdis_hip_plan* L, int cc) {
    const int f0 = L->h_free_ptr[(size_t)cc], c0 = L->h_fac_ptr[(size_t)cc];
    return CompLists{L->h_fac_id.data() + c0, L->h_fac_ptr[(size_t)cc + 1] - c0, L->h_free_vid.data() + f0, L->h_free_ptr[(size_t)cc + 1] - f0,
                     L->h_v2s_ptr.data() + f0};
}
// no camera variable free among the components [r0, r1) of the batch list
bool cameras_fixed(const rdis_hip_plan* L, size_t r0, size_t r1) {
    for (size_t r = r0; r < r1; ++r) {
        const int cc = L->h_rest[r];
        for (int k = L->h_free_ptr[(size_t)cc]; k < L->h_free_ptr[(size_t)cc + 1]; ++k)
            if (L->prob->h_block_of[(size_t)L->h_free_vid[(size_t)k]] >= 0) return false;
    }
    return true;
}

// step 1: drop the previous partition
void drop_partition(rdis_hip_plan* L) {
    // (the device memory of the items about to be dropped leaves the plan's account with them)
    auto drop = [&](DevBuf& b) { if (!L->transient && b.owned) L->dev_bytes -= std::min(L->dev_bytes, b.bytes); b.release(); };
    for (CoopLaunch& cl : L->coop_launches) { drop(cl.groups); drop(cl.wg_group); }
    for (StreamItem& st : L->stream) drop(st.long_vars);
    L->coop.clear();
    L->h_coop_ints.clear();
    L->coop_launches.clear();
    L->h_coop_groups.clear();
    L->h_coop_wg.clear();
    L->stream.clear();
    L->h_rest.clear();
    L->objective_in_solver = false;
}

// workgroups of a component's cooperative group with `lanes` factor lanes each: a lane per factor / variable, a wave per long gradient run
int64_t groups_of(const rdis_hip_plan* L, Partition& S, int cc, int lanes) {
    const int wpw = lanes / 64;
    const int64_t m = L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc];
    const int64_t n = L->h_free_ptr[(size_t)cc + 1] - L->h_free_ptr[(size_t)cc];
    const int f0 = L->h_free_ptr[(size_t)cc];
    int64_t& nlong = S.nlong_of[(size_t)cc];
    if (nlong < 0) {
        nlong = 0;
        for (int64_t i = 0; i < n; ++i)
            if (L->h_v2s_ptr[(size_t)(f0 + i) + 1] - L->h_v2s_ptr[(size_t)(f0 + i)] > COOP_LONG_LIST) ++nlong;
    }
    const int64_t need = (std::max(m, n) + lanes - 1) / lanes;
    // (small groups only: a large one has its waves anyway, and more workgroups lengthen every sweep)
    const int64_t for_long = need < 16 ? std::min<int64_t>((nlong + wpw - 1) / wpw, 2 * need + 2) : 0;
    return std::max<int64_t>(1, std::max(need, for_long));
}
// workgroups a cooperative launch of the plain or the pipelined layout can have resident
int coop_cap(rdis_hip_plan* L, bool pipe) {
    rdis_hip_ctx* c = L->prob->ctx;
    // (the occupancy queries behind these are not free: asked once per context -- a device -- and layout;
    // calls on a context are serialised, include/rdis_hip.h)
    const int ti = L->coop_threads == 128 ? 0 : L->coop_threads == 256 ? 1 : 2;
    const bool rr = L->coop_reference_rounding();
    int& kc = rr ? c->cap_coop_rr[ti] : c->cap_coop[ti];
    int& kp = rr ? c->cap_pipe_rr : c->cap_pipe;
    if (pipe && kp < 0) kp = solver_set(rr).pipe_max_workgroups(c->num_cus);
    if (!pipe && kc < 0) kc = solver_set(rr).coop_max_workgroups(L->coop_threads, c->num_cus);
    int k = pipe ? kp : kc;
    if (L->coop_workgroups > 0) k = std::min(k, L->coop_workgroups);
    return k;
}

// step 2: the cooperative layout and its cap
void choose_coop_layout(rdis_hip_plan* L, Partition& S) {
    rdis_hip_problem* p = L->prob;
    S.nlong_of.assign((size_t)L->ncomp, -1);
    // The grid solvers are for a few large components that would leave the device idle as single
    // workgroups, one launch each.  When there are more large components than that, the batch
    // kernel fills the device by itself (one workgroup per component) and is the better fit.
    int64_t nbig = 0;
    for (int64_t cc = 0; cc < L->ncomp; ++cc)
        if (L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc] >= L->coop_min_factors) ++nbig;
    S.any_big = L->coop_min_factors > 0 && L->coop_max_components > 0 && L->nfac >= L->coop_min_factors && nbig <= L->coop_max_components;
    S.coop_on = L->coop_min_factors > 0 && L->coop_max_components > 0 && p->kind == KIND_BA && !L->force_stream;
    // The pipelined layout (solver_pipe.hpp) has half the factor lanes per workgroup: it is used when
    // everything that gets a cooperative group with the plain layout also gets one with it.
    bool pipe = false;
    // (factor_rounding = 1, the parity option: the reference's slope -- a gradient pass of the whole group per trial and one
    // sequential sum -- exists in the plain cooperative layout only, solver_coop.hpp)
    if (S.coop_on && L->coop_pipeline != 0 && L->factor_rounding != 1 && L->coop_threads == PIPE_THREADS) {
        struct Census { int64_t group_total = 0, group_count = 0, big_unfit = 0; bool groups_fit = false; };
        auto census = [&](bool piped) {
            const int k = coop_cap(L, piped), lanes = piped ? PIPE_LANES : L->coop_threads;
            Census r;
            for (int cc : L->h_order) {
                const int64_t m = L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc];
                if (L->coop_group_min_factors > 0 && m >= L->coop_group_min_factors) { r.group_total += groups_of(L, S, cc, lanes); ++r.group_count; }
                if (m >= L->coop_min_factors && groups_of(L, S, cc, lanes) > k) ++r.big_unfit;
            }
            r.groups_fit = r.group_count > 0 && r.group_total <= k && r.group_count <= COOP_MAX_GROUPS;
            return r;
        };
        const Census plain = census(false), piped = census(true);
        pipe = !((plain.groups_fit && !piped.groups_fit) || piped.big_unfit > plain.big_unfit);
    }
    L->use_pipe = pipe;
    if (S.coop_on) S.cap = coop_cap(L, pipe);
}

// step 3: group mode, and the grid solver's cap
void choose_group_mode(rdis_hip_plan* L, Partition& S) {
    rdis_hip_ctx* c = L->prob->ctx;
    // Group mode: every component of some size gets a cooperative group when all the groups are
    // resident at once -- a device that the batch kernel would leave mostly idle (49 camera components
    // of ladybug: 6.6 ms as one workgroup each).  Otherwise only the few very large ones do.
    if (S.coop_on && S.cap > 0 && L->coop_group_min_factors > 0) {
        int64_t total = 0, count = 0;
        for (int cc : L->h_order) {
            if (L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc] < L->coop_group_min_factors) break;   // heaviest first
            total += groups_of(L, S, cc, L->coop_lanes());
            ++count;
        }
        if (count > 0 && total <= S.cap && count <= COOP_MAX_GROUPS) { S.group_min = L->coop_group_min_factors; S.any_big = true; }
    }
    if (S.any_big) S.scap = stream_max_workgroups(L->prob->kind, c->num_cus);
    if (L->coop_workgroups > 0) S.scap = std::min(S.scap, L->coop_workgroups);
}

// a component too large for a cooperative group whose camera blocks fit a compute unit's LDS (or may be numbered per workgroup)
bool wide_ptm_ok(rdis_hip_plan* L, Partition& S, int cc) {
    rdis_hip_problem* p = L->prob;
    if (p->kind != KIND_BA || L->ptm_stream == 0 || p->ncam_blocks <= 0 || (L->lds_resident == 0 && L->ptm_stream != 2)) return false;
    if (L->factor_rounding == 1 || L->emulate_stale) return false;   // (instantiated for the cooperative and LDS-resident solvers only)
    const BlockArrays B = block_arrays(p);
    if (!block_census(B, comp_lists(L, cc), ++p->stamp, S.cams, nullptr)) return false;
    const int ncb = (int)S.cams.size();
    // (more cameras than fit: a wide group whose workgroups keep their own cameras only -- decided with the tables below)
    return ncb <= PTM_MAX_CAMERAS && (ptm_bytes_for(ncb, PTM_WIDE_THREADS) <= p->ctx->lds_limit || (L->ptm_local_cameras != 0 && !L->ptm_local_off));
}

// step 4: every component to the cooperative solver (with its owner tables), the grid solver, or the batch list
int assign_components(rdis_hip_plan* L, Partition& S) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    L->ptm_wide_wanted = false;
    S.wide_comp.assign((size_t)L->ncomp, 0);
    // (one allocation: growing this by appending costs a transient call on ladybug 1.5 ms in page faults)
    L->h_coop_ints.reserve((size_t)(S.any_big ? 12 * L->nfac + 4 * (L->nfac + L->nfree) + 4096 * (int64_t)std::min<int64_t>(L->ncomp, 64) : 0));
    auto append = [&](const int* v, size_t count) {
        const size_t off = L->h_coop_ints.size();
        L->h_coop_ints.insert(L->h_coop_ints.end(), v, v + count);
        L->h_coop_ints.resize((L->h_coop_ints.size() + 63) / 64 * 64, -1);
        return off;
    };
    for (int cc : L->h_order) {  // heaviest first
        const int64_t m = L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc];
        const int64_t n = L->h_free_ptr[(size_t)cc + 1] - L->h_free_ptr[(size_t)cc];
        const int64_t need = groups_of(L, S, cc, L->coop_lanes());
        const bool grouped = m >= S.group_min;
        const bool big = S.any_big && (grouped || (m >= L->coop_min_factors && (int)(L->coop.size() + L->stream.size()) < L->coop_max_components));
        const bool take = big && S.cap > 0 && need <= S.cap && S.coop_on;
        // A bundle-adjustment component too large for a cooperative group whose CAMERA blocks fit a compute unit's LDS goes to the
        // point-major streaming solver as a wide group -- a workgroup per compute unit on the one component (solver_ptm.hpp: a trial
        // streams 18 bytes a factor and 48 a point block, nothing is written; the grid solver below forms every trial point in x[]
        // and gathers 24 doubles a factor through L2).  It joins the batch list; the slot tables decide (cameras, LDS).
        if (!take && big && wide_ptm_ok(L, S, cc)) { L->h_rest.push_back(cc); L->ptm_wide_wanted = true; S.wide_comp[(size_t)cc] = 1; continue; }
        if (!take && big && S.scap > 0) {
            // too large for the register-resident solver (or not bundle adjustment): the streaming
            // grid solver; about two factors per lane and trial point, at most what is resident
            L->stream.emplace_back();
            StreamItem& st = L->stream.back();
            st.comp = cc;
            st.nwg = (int)std::max<int64_t>(1, std::min<int64_t>(S.scap, (std::max(m, n) + 2 * STREAM_THREADS - 1) / (2 * STREAM_THREADS)));
            const int f0s = L->h_free_ptr[(size_t)cc];
            ivec longv;
            for (int64_t i = 0; i < n; ++i)
                if (L->h_v2s_ptr[(size_t)(f0s + i) + 1] - L->h_v2s_ptr[(size_t)(f0s + i)] > STREAM_LONG_LIST) longv.push_back((int)i);
            st.nlong = (int)longv.size();
            int rcs = plan_alloc(L, st.long_vars, std::max<size_t>(longv.size(), 1) * sizeof(int));
            if (rcs) return rcs;
            if (!longv.empty()) {
                HIPCHK(c, hipMemcpyAsync(st.long_vars.p, longv.data(), longv.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));  // local
            }
            continue;
        }
        if (!take) { L->h_rest.push_back(cc); continue; }
        L->coop.emplace_back();
        CoopItem& it = L->coop.back();
        it.comp = cc;
        it.nwg = (int)need;
        it.xi_off = (size_t)S.max_n;
        const CompLists C = comp_lists(L, cc);
        // local free index of each factor slot: plan_create's table, or (a plan that did not keep it) formed here
        const int* sl = nullptr;
        if (!L->h_slot_li.empty()) sl = L->h_slot_li.data() + 12 * (size_t)L->h_fac_ptr[(size_t)cc];
        else { coop_slot_li(block_arrays(p), C, ++p->stamp, S.sl_own); sl = S.sl_own.data(); }
        coop_owner_tables(C, it.nwg * L->coop_lanes(), COOP_LONG_LIST, S.lane_var, S.wave_var);
        it.slot_li = append(sl, (size_t)(12 * m));
        it.lane_var = append(S.lane_var.data(), S.lane_var.size());
        it.wave_var = append(S.wave_var.data(), S.wave_var.size());
        S.max_n += n;
    }
    return 0;
}

// step 5: tiny components to the front of the batch list; how the list's factors get their rotations
void order_rest(rdis_hip_plan* L) {
    rdis_hip_problem* p = L->prob;
    // tiny bundle-adjustment components (at most QUAD_MAX_VARS free variables: a point against fixed
    // cameras) go first in the batch list: four lanes each (solver_quad.hpp) instead of a workgroup
    auto tiny = [&](int cc) {
        return p->kind == KIND_BA && L->quad_max_vars > 0 &&
               L->h_free_ptr[(size_t)cc + 1] - L->h_free_ptr[(size_t)cc] <= std::min(L->quad_max_vars, QUAD_MAX_VARS);
    };
    // ... when there are enough of them to fill the device: below that a wave's sixteen components
    // finish at different times and the wave runs as long as its slowest (measured: ladybug's 7776
    // points 2.8 ms with a workgroup each, 4.2 ms as quads; 31104 synthetic points 4.5 vs 2.3 ms)
    int64_t ntiny = 0;
    for (int cc : L->h_rest) ntiny += tiny(cc) ? 1 : 0;
    L->rest_tiny = 0;
    L->tiny_group = ntiny >= L->quad_min_components ? 4 : ntiny >= L->row_min_components ? 16 : 0;
    if (L->tiny_group != 0) {
        auto mid = std::stable_partition(L->h_rest.begin(), L->h_rest.end(), tiny);
        L->rest_tiny = (int)(mid - L->h_rest.begin());
    }
    L->rest_rot_mode = ROT_PER_FACTOR;
    if (p->kind == KIND_BA && L->camera_records != 0 && p->ncam_blocks > 0 && !L->h_rest.empty()) {
        const bool camfix = cameras_fixed(L, 0, L->h_rest.size());
        // Free cameras: rewriting their records at every trial point puts one lane's rotation latency in
        // front of the evaluation and takes the rotation out of every factor -- a gain only where a lane
        // has many factors per camera (64 components of 31843 factors: 74 against 79 ms; no difference
        // for ladybug's 49 camera components or 1000 small components).
        int64_t mf = 0;
        for (int cc : L->h_rest) mf = std::max<int64_t>(mf, L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc]);
        L->rest_rot_mode = camfix ? ROT_CAMFIX : (L->camera_records == 2 || mf > 2048) ? ROT_RECORDS : ROT_PER_FACTOR;
    }
}

// step 6, one component of the batch list: which of the two solvers below takes it, if any, and its tables
void component_slot_tables(rdis_hip_plan* L, Partition& S, const BlockArrays& B, int cc, int ptm_max_threads) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    const CompLists C = comp_lists(L, cc);
    if (C.m == 0) return;   // (an empty factor list needs no table: solver_wg.hpp returns 0 for it)
    const int stamp = ++p->stamp;
    bool free_cam = false;
    if (!block_census(B, C, stamp, S.cams, &S.pts, &free_cam) || S.cams.size() > (size_t)PTM_MAX_CAMERAS) return;
    const bool many_points = S.pts.size() >= (1u << 20);   // (beyond the LDS-resident solver's slot word; the streaming tables use ls_pidx)
    const int ncb = (int)S.cams.size(), npb = (int)S.pts.size(), ns = 9 * ncb + 3 * npb, m = C.m, c0 = L->h_fac_ptr[(size_t)cc];
    std::sort(S.cams.begin(), S.cams.end());
    number_blocks(B, S.cams);
    ivec& gp = S.gp_of[(size_t)cc];
    gradient_pass_order(B, C, ncb, free_cam, gp);
    const int nchunk = (int)gp.size() / 64;
    // (the streaming solver is for what is too LARGE for the LDS: with lds_resident = 0 such components stay with
    // solver_wg.hpp -- the comparison the bit-identity tests make; ptm_stream = 2 sends everything its tables fit)
    const bool lds_size_ok = !many_points && lds_bytes_for(ns, ncb, nchunk) <= c->lds_limit;
    const bool fits_lds = L->lds_resident != 0 && lds_size_ok && L->ptm_stream != 2;
    const bool wide = S.wide_comp[(size_t)cc] != 0;
    const bool want_local = wide && !L->ptm_local_off && L->ptm_local_cameras != 0 && !S.local_failed &&
                            (L->ptm_local_cameras == 1 || ptm_bytes_for(ncb, PTM_WIDE_THREADS) > c->lds_limit);
    const bool fits_ptm = !fits_lds && (L->ptm_stream == 2 || (L->ptm_stream == 1 && !lds_size_ok)) &&
                          (want_local || ptm_bytes_for(ncb, ptm_max_threads) <= c->lds_limit);
    if (want_local && L->ptm_local) { S.local_failed = true; gp.clear(); return; }   // (one such component a plan)
    if (!fits_lds && !fits_ptm) { gp.clear(); return; }
    if (fits_lds) std::sort(S.pts.begin(), S.pts.end());
    else {
        PtmLocalReport rep;
        const bool fits = ptm_point_order(B, C, ncb, want_local ? PtmDeal::LOCAL : wide ? PtmDeal::WIDE : PtmDeal::SPREAD, c->num_cus, c->lds_limit,
                                          S.pts, S.deg, L->loc.wg_chunk0, S.local_cams, rep);
        if (rep.dealt && std::getenv("RDIS_HIP_LOCAL_STATS"))
            std::fprintf(stderr, "local cameras: %d workgroups over %d chunks, %d cameras in the component, at most %zu in a workgroup (the LDS holds %zu)\n",
                         rep.K, rep.chunks, ncb, rep.worst, rep.cam_cap);
        if (!fits) { S.local_failed = true; gp.clear(); return; }
        if (want_local) { L->ptm_local = true; L->ptm_local_K = rep.K; L->ptm_local_comp = cc; }
    }
    slot_table(B, C, stamp, S.cams, S.pts, !fits_lds, S.vid_of[(size_t)cc], S.free_of[(size_t)cc], S.ls_fidx.data() + c0, S.ls_pidx.data() + c0, S.pptr_of[(size_t)cc]);
    S.ls_ncb[(size_t)cc] = ncb;
    S.ls_gcount[(size_t)cc] = nchunk;
    if (fits_lds) {
        S.kind_of[(size_t)cc] = 1;
        L->lds_ns_cap = std::max(L->lds_ns_cap, ns);
        L->lds_ncb_cap = std::max(L->lds_ncb_cap, ncb);
        L->lds_chunk_cap = std::max(L->lds_chunk_cap, nchunk);
        L->lds_max_factors = std::max<int64_t>(L->lds_max_factors, m);
    } else {
        S.kind_of[(size_t)cc] = 2;
        if (L->ptm_local && L->ptm_local_comp == cc) {   // (a workgroup's LDS holds its own cameras only)
            for (const ivec& lc : S.local_cams) L->ptm_ncb_cap = std::max(L->ptm_ncb_cap, (int)lc.size());
        } else {
            L->ptm_ncb_cap = std::max(L->ptm_ncb_cap, ncb);
        }
    }
}

// step 6: Slot tables.  The LDS-resident solver (solver_lds.hpp) takes the bundle-adjustment components of the
// batch list whose variables -- free ones and the constants their factors read -- fit a compute unit's
// LDS as slots: camera blocks (9 slots each, ascending by id), then point blocks (3 each, ascending).
// Of the others, those whose CAMERA blocks fit go to the point-major streaming solver (solver_ptm.hpp:
// point blocks as records in HBM, ordered by their number of factors, descending).  Both move to the
// end of the list (streaming ones first); what fits neither stays with solver_wg.hpp.
// false: local camera numbering did not work out (a workgroup's cameras beyond the LDS, too few chunks, a second streaming
// component in the plan).
bool build_slot_tables(rdis_hip_plan* L, Partition& S) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    L->rest_lds = L->rest_ptm = 0;
    L->h_lds_ints.clear();
    L->h_pm_jg.clear();
    L->lds_ns_cap = L->lds_ncb_cap = L->lds_chunk_cap = L->ptm_ncb_cap = 0;
    L->rounds_threads = L->rounds_K = 0;
    L->lds_max_factors = 0;
    L->pm_blocks = L->pm_entries = 0;
    if (!(p->kind == KIND_BA && (L->lds_resident != 0 || L->ptm_stream != 0) && p->ncam_blocks > 0 && (int)L->h_rest.size() > L->rest_tiny)) return true;
    const BlockArrays B = block_arrays(p);
    const size_t nc = (size_t)L->ncomp;
    S.kind_of.assign(nc, 0);
    // (the staging area of its gradient grows with the workgroup; a plan with a component meant for a wide group keeps to that group's 512 lanes)
    const int ptm_max_threads = L->ptm_threads ? L->ptm_threads : L->ptm_wide_wanted ? PTM_WIDE_THREADS : 768;
    S.ls_ncb.assign(nc, 0); S.ls_gcount.assign(nc, 0); S.pm_pt0.assign(nc, 0);
    S.ls_fidx.assign((size_t)L->nfac, 0); S.ls_pidx.assign((size_t)L->nfac, 0);
    S.vid_of.assign(nc, ivec()); S.free_of.assign(nc, ivec()); S.gp_of.assign(nc, ivec()); S.pptr_of.assign(nc, ivec());
    L->ptm_local = false; L->ptm_local_K = 0; L->ptm_local_comp = -1;
    L->loc.clear();
    for (size_t r = (size_t)L->rest_tiny; r < L->h_rest.size(); ++r) component_slot_tables(L, S, B, L->h_rest[r], ptm_max_threads);
    // (the maxima of a launch may come from different components: its LDS must hold them together)
    if (L->lds_ns_cap > 0 && lds_bytes_for(L->lds_ns_cap, L->lds_ncb_cap, L->lds_chunk_cap) > c->lds_limit)
        for (size_t cc = 0; cc < nc; ++cc) if (S.kind_of[cc] == 1) S.kind_of[cc] = 0;
    auto first_other = std::stable_partition(L->h_rest.begin() + L->rest_tiny, L->h_rest.end(), [&](int cc) { return S.kind_of[(size_t)cc] == 0; });
    auto first_lds = std::stable_partition(first_other, L->h_rest.end(), [&](int cc) { return S.kind_of[(size_t)cc] == 2; });
    L->rest_ptm = (int)(first_lds - first_other);
    L->rest_lds = (int)(L->h_rest.end() - first_lds);
    return !(S.local_failed || (L->ptm_local && L->rest_ptm != 1));
}

// step 6, the end: the components' tables as one int32 block, the streaming components' factor stream, the rotation modes
void assemble_slot_block(rdis_hip_plan* L, Partition& S) {
    if (L->rest_ptm + L->rest_lds == 0) return;
    const size_t nc = (size_t)L->ncomp;
    // one int32 block, tables in component order (a component without one has empty ranges)
    ivec sptr(nc + 1, 0), gptr(nc + 1, 0), svid, sfree, gperm;
    for (size_t cc = 0; cc < nc; ++cc) {
        const bool has = S.kind_of[cc] != 0;
        sptr[cc + 1] = sptr[cc] + (has ? (int)S.vid_of[cc].size() : 0);
        gptr[cc + 1] = gptr[cc] + (has ? S.ls_gcount[cc] : 0);
        if (!has) continue;
        svid.insert(svid.end(), S.vid_of[cc].begin(), S.vid_of[cc].end());
        sfree.insert(sfree.end(), S.free_of[cc].begin(), S.free_of[cc].end());
        gperm.insert(gperm.end(), S.gp_of[cc].begin(), S.gp_of[cc].end());
    }
    ivec pm_ch0v(nc, 0), cptr, cbase;
    L->h_pm_jg.clear();
    L->ptm_min_points = INT64_MAX;
    for (size_t cc = 0; cc < nc; ++cc) {
        if (S.kind_of[cc] != 2) continue;
        const int c0 = L->h_fac_ptr[cc], npb = (int)S.pptr_of[cc].size() - 1, e0 = (int)L->h_pm_jg.size();
        S.pm_pt0[cc] = (int)L->pm_blocks;
        pm_ch0v[cc] = (int)cptr.size();
        ptm_factor_stream(c0, L->h_fac_ptr[cc + 1] - c0, S.ls_pidx.data() + c0, S.pptr_of[cc], L->h_pm_jg, cptr, cbase);
        L->pm_blocks += npb;
        L->ptm_min_points = std::min<int64_t>(L->ptm_min_points, npb);
        if (L->ptm_local && L->ptm_local_comp == (int)cc) ptm_local_tables(S.ls_ncb[cc], S.local_cams, cbase, e0, L->h_pm_jg, S.ls_fidx.data(), L->loc);
    }
    L->pm_entries = (int64_t)L->h_pm_jg.size();
    L->pm_cptr_len = (int64_t)cptr.size();
    L->ls_total_chunks = gptr[nc];
    ivec& blk = L->h_lds_ints;
    auto put = [&](const ivec& v) { const size_t off = blk.size(); blk.insert(blk.end(), v.begin(), v.end()); return off; };
    L->off_ls_ptr = put(sptr); L->off_ls_vid = put(svid); L->off_ls_free = put(sfree);
    L->off_ls_ncb = put(S.ls_ncb); L->off_ls_fidx = put(S.ls_fidx); L->off_ls_gptr = put(gptr); L->off_ls_gperm = put(gperm);
    L->off_pm_pt0 = put(S.pm_pt0); L->off_pm_ch0 = put(pm_ch0v); L->off_pm_cptr = put(cptr); L->off_pm_jg = put(L->h_pm_jg);
    // rotations: no camera variable free among a launch's components -> records, read only; otherwise records
    // that follow the trial point when a lane has several factors per camera and trial (else each factor forms its own)
    const size_t r_lds = L->h_rest.size() - (size_t)L->rest_lds, r_ptm = r_lds - (size_t)L->rest_ptm;
    const bool records = L->lds_rot >= 0 ? L->lds_rot == 1 : L->lds_max_factors > 512;
    // (the stale-cache emulation is instantiated for per-factor rotations only: the same bits per factor, fewer kernels)
    L->lds_rot_mode = (L->camera_records == 0 || L->emulate_stale) ? ROT_PER_FACTOR : cameras_fixed(L, r_lds, L->h_rest.size()) ? ROT_CAMFIX : records ? ROT_RECORDS : ROT_PER_FACTOR;
    // (the streaming solver always works from per-camera records: rewritten at every trial point, or never)
    L->ptm_rot_mode = cameras_fixed(L, r_ptm, r_lds) ? ROT_CAMFIX : ROT_RECORDS;
}

// step 7: device memory and uploads
int upload_partition(rdis_hip_plan* L, Partition& S) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    if (L->rest_tiny > 0 && L->group_blocks4 == 0) {
        int b4 = 0, b16 = 0;
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4, cgd_group_kernel<4, QUAD_THREADS>, QUAD_THREADS, 0));
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b16, cgd_group_kernel<16, 64>, 64, 0));
        L->group_blocks4 = std::max(1, b4) * c->num_cus;
        L->group_blocks16 = std::max(1, b16) * c->num_cus;
    }
    int rc = plan_alloc(L, L->rest_order, std::max<size_t>(L->h_rest.size(), 1) * sizeof(int));
    if (!rc) rc = plan_alloc(L, L->queue, 256);
    if (!rc && S.max_n > 0) rc = plan_alloc(L, L->xi_glob, (size_t)S.max_n * sizeof(double));
    if (rc) return rc;
    if (L->rest_lds + L->rest_ptm > 0) {
        rc = plan_alloc(L, L->lds_ints, L->h_lds_ints.size() * sizeof(int));
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(L->lds_ints.p, L->h_lds_ints.data(), L->h_lds_ints.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        rc = plan_alloc(L, L->lds_obs, (size_t)std::max<int64_t>(L->nfac, 1) * sizeof(double2));
        if (rc) return rc;
        gather_obs_kernel<<<grid_for(c, L->nfac, 256), 256, 0, c->stream>>>((int)L->nfac, L->ip(L->off_fac_id), p->obs.as<double2>(), L->lds_obs.as<double2>());
        HIPCHK(c, hipGetLastError());
    }
    if (L->rest_ptm > 0) {   // the streaming components' point records and point-major factor arrays
        rc = plan_alloc(L, L->pm_rec, (size_t)L->pm_blocks * PT_REC * sizeof(double));
        if (!rc) rc = plan_alloc(L, L->pm_gh, (size_t)L->pm_blocks * PT_REC * sizeof(double));
        if (!rc) rc = plan_alloc(L, L->pm_cbox, (size_t)std::max<int64_t>(L->pm_cptr_len, 1) * 8 * sizeof(float));
        if (!rc) rc = plan_alloc(L, L->pm_bex, (size_t)L->pm_blocks * PT_BND * sizeof(double));
        // (a block of PTM_BLK slots is loaded whole: the last chunk's may reach past the last entry)
        if (!rc) rc = plan_alloc(L, L->pm_cam, ((size_t)L->pm_entries + 64 * PTM_BLK) * sizeof(short));
        if (!rc) rc = plan_alloc(L, L->pm_obs, ((size_t)L->pm_entries + 64 * PTM_BLK) * sizeof(double2));
        if (rc) return rc;
        const PlanView V = L->view();
        HIPCHK(c, ptm_gather_launch(grid_for(c, L->pm_entries, 256), c->stream, (int)L->pm_entries, L->lds_ints.as<int>() + L->off_pm_jg, V.ls_fidx, V.ls_obs,
                                    L->pm_cam.as<short>(), L->pm_obs.as<double2>()));
        if (L->ptm_local) {   // the stream names a factor's camera by its number in the workgroup that owns the chunk; the group's tables
            const PtmLocalTables& T = L->loc;
            HIPCHK(c, hipMemcpyAsync(L->pm_cam.p, T.pm_lcam.data(), std::min(T.pm_lcam.size(), (size_t)L->pm_entries + 64 * PTM_BLK) * sizeof(short),
                                     hipMemcpyHostToDevice, c->stream));
            rc = plan_alloc(L, L->lc_dev, T.lc.size() * sizeof(int));
            if (!rc) rc = plan_alloc(L, L->lc_off_dev, T.lc_off.size() * sizeof(long long));
            if (!rc) rc = plan_alloc(L, L->cr_ptr_dev, T.cr_ptr.size() * sizeof(int));
            if (!rc) rc = plan_alloc(L, L->cr_dev, std::max<size_t>(T.cr.size(), 1) * sizeof(int));
            if (!rc) rc = plan_alloc(L, L->ptm_tot, 2 * (size_t)PTM_CS * (T.cr_ptr.size() - 1) * sizeof(double));
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(L->lc_dev.p, T.lc.data(), T.lc.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(L->lc_off_dev.p, T.lc_off.data(), T.lc_off.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(L->cr_ptr_dev.p, T.cr_ptr.data(), T.cr_ptr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(L->cr_dev.p, T.cr.data(), T.cr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        }
    }
    if (!L->coop.empty()) {
        rc = plan_alloc(L, L->coop_ints, L->h_coop_ints.size() * sizeof(int));
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(L->coop_ints.p, L->h_coop_ints.data(), L->h_coop_ints.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// step 8: cooperative groups, packed into launches of at most `cap` workgroups
int pack_coop_launches(rdis_hip_plan* L, int cap) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    int rc = 0;
    size_t max_groups = 1;
    for (size_t i = 0; i < L->coop.size();) {
        CoopLaunch cl;
        cl.first = (int)i;
        std::vector<CoopGroup> hg;
        ivec hw;
        while (i < L->coop.size() && (cl.count == 0 || cl.total_wg + L->coop[i].nwg <= cap) && cl.count < COOP_MAX_GROUPS) {
            const CoopItem& it = L->coop[i];
            CoopGroup g{};
            g.a = CoopArgs{i == 0 ? p->coop_timing.as<long long>() : nullptr, nullptr /* set below */, L->coop_ints.as<int>() + it.slot_li,
                           L->coop_ints.as<int>() + it.lane_var, L->coop_ints.as<int>() + it.wave_var, L->xi_glob.as<double>() + it.xi_off, it.comp,
                           // (a small group's sweep is one entry per lane: polling early costs it less than waiting)
                           it.nwg * (L->coop_lanes() / 64) <= 64 ? std::min(4, L->coop_poll_delay) : L->coop_poll_delay,
                           L->coop_speculate, L->factor_rounding == 1 ? 1 : 0, (L->factor_rounding == 1 && L->emulate_stale) ? 1 : 0,
                           L->coop_poll_inflight, L->coop_poll_stagger, nullptr /* set below */};
            g.wg0 = cl.total_wg; g.nwg = it.nwg;
            hg.push_back(g);
            hw.insert(hw.end(), (size_t)it.nwg, cl.count);
            cl.total_wg += it.nwg; ++cl.count; ++i;
        }
        max_groups = std::max(max_groups, hg.size());
        if (p->coop_state.bytes < max_groups * sizeof(CoopState)) {   // one exchange state per concurrent group
            // The buffer moves: every other plan of this problem has its address in its uploaded group
            // tables.  The generation tells rdis_hip_plan_solve to rebuild theirs before they run again.
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->aux) HIPCHK(c, hipStreamSynchronize(c->aux));
            rc = dalloc(c, p->coop_state, std::max(max_groups, 2 * (p->coop_state.bytes / sizeof(CoopState))) * sizeof(CoopState));
            if (rc) return rc;
            ++p->coop_state_gen;
        }
        rc = plan_alloc(L, cl.groups, hg.size() * sizeof(CoopGroup));
        if (!rc) rc = plan_alloc(L, cl.wg_group, hw.size() * sizeof(int));
        if (rc) return rc;
        L->coop_launches.push_back(std::move(cl));
        L->h_coop_groups.push_back(std::move(hg));
        L->h_coop_wg.push_back(std::move(hw));   // (host images are kept: the uploads are asynchronous)
        HIPCHK(c, hipMemcpyAsync(L->coop_launches.back().wg_group.p, L->h_coop_wg.back().data(),
                                 L->h_coop_wg.back().size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    // a plan whose one launch is the single-group pipelined solver: that kernel stores the plan's objective with the component's
    // fret, and rdis_hip_plan_solve launches no objective_sum_kernel behind it
    L->objective_in_solver = L->pipelined() && L->ncomp == 1 && L->coop.size() == 1 && L->h_rest.empty() && L->stream.empty();
    // (the state pointers only now: the buffer may have moved while the launches were sized)
    for (size_t l = 0; l < L->coop_launches.size(); ++l) {
        std::vector<CoopGroup>& hg = L->h_coop_groups[l];
        for (size_t g = 0; g < hg.size(); ++g) hg[g].a.st = p->coop_state.as<CoopState>() + g;
        if (L->objective_in_solver) hg[0].a.objective = L->objective.as<double>();
        HIPCHK(c, hipMemcpyAsync(L->coop_launches[l].groups.p, hg.data(), hg.size() * sizeof(CoopGroup), hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

}  // namespace

// decide which solver takes each component and build what it needs (plan_query.hip calls it too)
int rdis_hip::prepare_partition(rdis_hip_plan* L) {
    rdis_hip_ctx* c = L->prob->ctx;
    Partition S;
    for (;;) {
        S = Partition();
        drop_partition(L);
        choose_coop_layout(L, S);
        choose_group_mode(L, S);
        int rc = assign_components(L, S);
        if (rc) return rc;
        order_rest(L);
        if (build_slot_tables(L, S)) break;
        // local camera numbering did not work out: once more without it -- the component then takes the grid solver
        // (once: the flag stays set, and without local numbering nothing above fails)
        L->ptm_local = false;
        L->ptm_local_off = true;
    }
    assemble_slot_block(L, S);
    int rc = upload_partition(L, S);
    if (!rc) rc = pack_coop_launches(L, S.cap);
    if (rc) return rc;
    // (a transient plan lives until its results are fetched, which waits for the stream)
    if (!L->transient) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!L->h_rest.empty()) HIPCHK(c, hipMemcpyAsync(L->rest_order.p, L->h_rest.data(), L->h_rest.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    L->partition_dirty = false;
    L->coop_state_gen = L->prob->coop_state_gen;
    return 0;
}

// ---- the launches of a solve, and their shapes ----
namespace {

template <int KIND>
int launch_wg(rdis_hip_plan* L, hipStream_t stream, int threads, int first, int grid, int maxiters, double ftol) {
    rdis_hip_ctx* c = L->prob->ctx;
    ProblemView P = L->prob->view();
    P.xrot = L->prob->xrot.as<double>(); P.rot_mode = L->rest_rot_mode;
    PlanView V = L->view();
    V.order += first;   // components [first, first + grid) of the batch list
    HIPCHK(c, (with_threads<64, 128, 256, 512, 768, 1024>(threads, [&](auto T) {
        return launch_dyn(cgd_wg_kernel<KIND, T.value>, grid, T.value, 0, stream, P, V, maxiters, ftol);
    })));
    return 0;
}
// The streaming solver's work tables for workgroups of `threads` lanes, K to a component: a trial's segment rows and the gradient's
// rounds (plan_tables.hpp: ptm_segment_rows, ptm_round_tables).  Built on the host from the plan's point-major tables, once per
// (threads, K); no rounds to build when no camera variable is free.
static PtmStreamTables ptm_stream_tables(const rdis_hip_plan* L) {
    const int* li = L->h_lds_ints.data();
    const size_t r_lds = L->h_rest.size() - (size_t)L->rest_lds, r_ptm = r_lds - (size_t)L->rest_ptm;
    PtmStreamTables T;
    T.ncomp = L->ncomp; T.pm_entries = L->pm_entries;
    T.comps = L->h_rest.data() + r_ptm; T.ncomps = r_lds - r_ptm;
    T.ls_ptr = li + L->off_ls_ptr; T.ls_ncb = li + L->off_ls_ncb; T.ls_fidx = li + L->off_ls_fidx;
    T.pm_ch0 = li + L->off_pm_ch0; T.cptr = li + L->off_pm_cptr; T.jg = li + L->off_pm_jg;
    T.local_comp = L->ptm_local ? L->ptm_local_comp : -1;
    T.local = &L->loc;
    return T;
}
static int ptm_build_segments(rdis_hip_plan* L, int threads, int K) {
    rdis_hip_ctx* c = L->prob->ctx;
    const size_t nwg = (size_t)L->ncomp * (size_t)K;
    std::vector<long long> off;
    ivec rows;
    ptm_segment_rows(ptm_stream_tables(L), threads, K, rows, off);
    int rc = plan_alloc(L, L->pm_segs, std::max<size_t>(rows.size(), 4) * sizeof(int));
    if (!rc) rc = plan_alloc(L, L->pm_sg_off, nwg * sizeof(long long));
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(L->pm_segs.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L->pm_sg_off.p, off.data(), nwg * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// the slots a gradient round evaluates and stages (solver_ptm.hpp: rs): two -- a whole block of slots -- where the LDS holds 2 x threads
// staging rows beside the cameras, else one
static int ptm_round_slots_for(const rdis_hip_plan* L, int threads) {
    if (L->ptm_round_slots == 1 || PTM_BLK != 2 || threads > PTM_PAIR_MAX_THREADS) return 1;
    // (workgroups of 256 lanes stand two to a compute unit: both must keep their place)
    return (size_t)(threads <= 256 ? 2 : 1) * ptm_bytes_for(L->ptm_ncb_cap, threads, 2) <= (size_t)L->prob->ctx->lds_limit ? 2 : 1;
}
int ptm_build_rounds(rdis_hip_plan* L, int threads, int K) {
    rdis_hip_ctx* c = L->prob->ctx;
    const int rs = ptm_round_slots_for(L, threads);
    if (L->rounds_threads == threads && L->rounds_K == K && L->rounds_slots == rs) return 0;
    // (the key is set when everything below has succeeded: a caller that frees memory and solves again after ENOMEM
    // must find the tables either complete or absent, never "already built" with buffers missing)
    L->rounds_threads = L->rounds_K = 0;
    { const int rc = ptm_build_segments(L, threads, K); if (rc) return rc; }
    if (L->ptm_rot_mode == ROT_CAMFIX) { L->rounds_threads = threads; L->rounds_K = K; L->rounds_slots = rs; return 0; }
    const PtmStreamTables T = ptm_stream_tables(L);
    const size_t nwg = (size_t)L->ncomp * (size_t)K;
    std::vector<long long> off;
    ivec nr;
    std::vector<unsigned short> tab, grow;
    ptm_round_tables(T, threads, K, rs, tab, grow, off, nr);
    if (std::getenv("RDIS_HIP_ROUND_STATS") && nwg > 0) {   // (tuning: how uneven are a round's camera segments?)
        const int cc = T.comps[0];
        const int ncb = T.ls_ncb[cc];
        const size_t stride = (size_t)ptm_round_stride(ncb);
        const unsigned short* t0 = tab.data() + off[(size_t)cc * K];
        long long sum_max = 0, worst = 0, rows = 0, active = 0;
        const int nrd = nr[(size_t)cc * K];
        for (int rr = 0; rr < nrd; ++rr) {
            const unsigned short* rec = t0 + (size_t)rr * stride;
            int mx = 0;
            for (int k = 0; k < ncb; ++k) { const int len = rec[k + 1] - rec[k]; mx = std::max(mx, len); active += len > 0; }
            sum_max += mx; worst = std::max<long long>(worst, mx); rows += rec[ncb];
        }
        std::fprintf(stderr, "ptm rounds (threads %d, K %d): first workgroup %d rounds, %d cameras; rows per round %.1f, active cameras per round %.1f, longest segment: mean %.1f, worst %lld\n",
                     threads, K, nrd, ncb, (double)rows / std::max(nrd, 1), (double)active / std::max(nrd, 1), (double)sum_max / std::max(nrd, 1), worst);
    }
    int rc = plan_alloc(L, L->pm_rounds, std::max<size_t>(tab.size(), 2) * sizeof(unsigned short));
    if (!rc) rc = plan_alloc(L, L->pm_grow, grow.size() * sizeof(unsigned short));
    if (!rc) rc = plan_alloc(L, L->pm_rd_off, nwg * sizeof(long long));
    if (!rc) rc = plan_alloc(L, L->pm_rd_n, nwg * sizeof(int));
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(L->pm_rounds.p, tab.data(), tab.size() * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L->pm_grow.p, grow.data(), grow.size() * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L->pm_rd_off.p, off.data(), nwg * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L->pm_rd_n.p, nr.data(), nwg * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host tables go out of scope; a launch on another stream follows)
    L->rounds_threads = threads; L->rounds_K = K; L->rounds_slots = rs;
    return 0;
}
int launch_ptm(rdis_hip_plan* L, hipStream_t stream, int threads, int first, int grid, int maxiters, double ftol) {
    rdis_hip_ctx* c = L->prob->ctx;
    int rc = ptm_build_rounds(L, threads, 1);
    if (rc) return rc;
    ProblemView P = L->prob->view();
    PlanView V = L->view();
    V.order += first;
    HIPCHK(c, ptm_launch(L->ptm_rot_mode, threads, grid, ptm_bytes_for(L->ptm_ncb_cap, threads, L->rounds_slots), stream, P, V, maxiters, ftol, L->ptm_ncb_cap));
    return 0;
}
// K workgroups per component (cgd_ptmg_kernel): how many groups of K fit the device, and the launch
int ptmg_resident_workgroups(rdis_hip_plan* L, int threads, int* out, bool wide = false) {
    rdis_hip_ctx* c = L->prob->ctx;
    const size_t dyn = ptm_bytes_for(L->ptm_ncb_cap, threads, ptm_round_slots_for(L, threads));
    const void* fn = ptmg_kernel_fn(L->ptm_rot_mode, threads, wide);
    if (dyn > 48 * 1024) HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    int per_cu = 0;
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, dyn));
    *out = per_cu * c->num_cus;
    return 0;
}
int launch_ptm_groups(rdis_hip_plan* L, hipStream_t stream, int threads, int first, int ngroups, int K, int maxiters, double ftol, bool wide = false) {
    const bool local = wide && L->ptm_local;
    rdis_hip_ctx* c = L->prob->ctx;
    int rc = ptm_build_rounds(L, threads, K);
    if (rc) return rc;
    ProblemView P = L->prob->view();
    PlanView V = L->view();
    V.order += first;
    const size_t dyn = ptm_bytes_for(L->ptm_ncb_cap, threads, L->rounds_slots);
    int ncc = L->ptm_ncb_cap;
    // (a wide group's workgroups and waves outnumber a small state's entries: a CoopState each)
    const size_t st_bytes = wide ? sizeof(CoopState) : sizeof(SmallCoopState);
    const size_t abort_off = wide ? offsetof(CoopState, abort_flag) : offsetof(SmallCoopState, abort_flag);
    if (L->ptm_state.bytes < (size_t)ngroups * st_bytes) {
        rc = plan_alloc(L, L->ptm_state, (size_t)ngroups * st_bytes);
        if (rc) return rc;
    }
    const size_t xch_bytes = (size_t)ngroups * (2 * (size_t)K + 2) * PTM_CS * (size_t)ncc * sizeof(double);
    if (L->ptm_xch.bytes < xch_bytes) {
        rc = plan_alloc(L, L->ptm_xch, xch_bytes);
        if (rc) return rc;
    }
    // arm every granule, clear the abort words
    HIPCHK(c, hipMemsetAsync(L->ptm_state.p, 0xFF, (size_t)ngroups * st_bytes, stream));
    HIPCHK(c, hipMemset2DAsync((char*)L->ptm_state.p + abort_off, st_bytes, 0, 64, (size_t)ngroups, stream));
    PtmGroupArgs A{L->ptm_state.p, L->ptm_xch.as<double>(), K, ngroups, wide ? L->coop_poll_delay : std::min(4, L->coop_poll_delay),
                   nullptr, nullptr, nullptr, nullptr, nullptr};
    if (local) {
        A.lc_off = L->lc_off_dev.as<long long>(); A.lc = L->lc_dev.as<int>(); A.cr_ptr = L->cr_ptr_dev.as<int>(); A.cr = L->cr_dev.as<int>();
        A.tot = L->ptm_tot.as<double>();
    }
    int mi = maxiters;
    double ft = ftol;
    void* args[] = {&P, &V, &A, &mi, &ft, &ncc};
    const int grid = wide ? K * ngroups : 8 * K * ((ngroups + 7) / 8);
    const void* fn = ptmg_kernel_fn(L->ptm_rot_mode, threads, wide, local);
    if (local && dyn > 48 * 1024) HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    HIPCHK(c, hipLaunchCooperativeKernel(fn, dim3(grid), dim3(threads), args, dyn, stream));
    return 0;
}
// The shape of the point-major launch of an ordinary solve (L->rest_ptm > 0): lanes a workgroup, workgroups a component (1:
// launch_ptm, else launch_ptm_groups) and whether the groups are wide.  `overlap`: the batch runs beside cooperative launches.
// (The population entry asks too: it takes a plan only where this says one workgroup a component -- the bits depend on it.)
int ptm_launch_shape(rdis_hip_plan* L, bool overlap, int* threads_out, int* K_out, bool* wide_out) {
    rdis_hip_ctx* c = L->prob->ctx;
    // 768 lanes, three waves per SIMD (1000 / 500 components of ladybug's size: 187 / 99 ms, 196 / 109 with 256 lanes and two
    // workgroups per compute unit).  Fewer components than resident workgroups: K workgroups share a component
    // (cooperative launch, every workgroup of it resident), of 256 lanes -- two per compute unit, the finer grain
    // loses less to whole wave-chunks -- as long as a workgroup keeps some twenty wave-chunks of points per trial point
    // (below that the exchange costs what the split saves: 125 components of 2048 points 9.6 ms alone, 9.7 as pairs;
    // of 7776 points 35.8 ms alone, 27.7 as groups of four)
    int threads = L->ptm_threads ? L->ptm_threads : L->ptm_wide_wanted ? PTM_WIDE_THREADS : 768;
    int K = 1;
    if (L->ptm_group != 1 && !overlap && L->coop.empty() && L->stream.empty()) {
        // groups of K workgroups: of 512 lanes (a workgroup per compute unit) or of 256 (two) -- whichever brings more
        // lanes to a component, at equal lanes the larger workgroup (125 components of ladybug's size: pairs of 512
        // lanes 16.0 ms, fours of 256 17.0, one workgroup of 768 each 24.2; round 4)
        const int slots8 = 8 * ((L->rest_ptm + 7) / 8);   // (groups are placed eight at a time, one per XCD)
        const int useful = (int)std::max<int64_t>(1, (L->ptm_min_points + 63) / 64 / 24);
        int best_lanes = 0, best_threads = 0, best_K = 1;
        const int cands[2] = {L->ptm_threads ? L->ptm_threads : 512, 256};
        for (int ci = 0; ci < (L->ptm_threads ? 1 : 2); ++ci) {
            const int gt = cands[ci];
            int cap = 0;
            int rc = ptmg_resident_workgroups(L, gt, &cap);
            if (rc) return rc;
            const int fit = std::min(std::min(PTM_MAX_GROUP, cap / slots8), SMALL_COOP_ENTRIES / (gt / 64));
            const int Kc = L->ptm_group > 1 ? std::min(L->ptm_group, fit) : std::min(fit, useful);
            if (Kc >= 2 && Kc * gt > best_lanes) { best_lanes = Kc * gt; best_threads = gt; best_K = Kc; }
        }
        // (a group must bring more lanes to a component than the one workgroup it replaces: 250 components of
        // ladybug's size 50.4 ms a workgroup of 768 lanes each, 56.0 as pairs of 256)
        if (best_K >= 2 && (L->ptm_group > 1 || best_lanes > threads)) { K = best_K; threads = best_threads; }
    }
    // A few components and a device: wide groups -- as many workgroups of 512 lanes a component as are resident and have some
    // twenty wave-chunks of points each (one component of 8e6 factors: 256 workgroups, 15 chunks a wave)
    bool wide = false;
    if (L->ptm_local) {   // (its tables are made for this group size)
        K = L->ptm_local_K; threads = PTM_WIDE_THREADS; wide = true;
        if (overlap || !L->coop.empty() || !L->stream.empty())
            return fail(c, RDIS_HIP_EINVAL, "a wide group with local camera numbering takes the device to itself: no cooperative or grid launch beside it");
    } else if (L->ptm_group != 1 && !overlap && L->coop.empty() && L->stream.empty() && L->rest_ptm <= 8 &&
        (L->ptm_threads == 0 || L->ptm_threads == PTM_WIDE_THREADS)) {
        int cap = 0;
        int rc = ptmg_resident_workgroups(L, PTM_WIDE_THREADS, &cap, true);
        if (rc) return rc;
        const int useful = (int)std::max<int64_t>(1, (L->ptm_min_points + 63) / 64 / 24);
        const int fit = std::min(std::min(PTM_WIDE_MAX_GROUP, cap / L->rest_ptm), COOP_MAX_WG * COOP_MAX_WAVES / (PTM_WIDE_THREADS / 64));
        const int Kw = L->ptm_group > 1 ? std::min(L->ptm_group, fit) : std::min(fit, useful);
        if (Kw > PTM_MAX_GROUP && Kw * PTM_WIDE_THREADS > K * threads) { K = Kw; threads = PTM_WIDE_THREADS; wide = true; }
    }
    *threads_out = threads; *K_out = std::max(K, 1); *wide_out = wide;
    return 0;
}
// the workgroup size of the LDS-resident launch (a sum's tree depends on it: the multi-start entry takes the same)
int lds_launch_threads(const rdis_hip_plan* L) {
    const rdis_hip_ctx* c = L->prob->ctx;
    const int64_t mf = L->lds_max_factors;
    int threads = L->lds_threads ? L->lds_threads : L->block_threads;
    // A lane per factor up to 512, then 768 lanes (three waves per SIMD) -- unless the launch has more
    // components than compute units: then 256 lanes, two workgroups per compute unit, so that one
    // component's arithmetic fills the unit while the other's control step (one lane) or barrier runs
    // (1000 x 2048 factors: 11.9 against 13.7 ms; 125 of them, a unit each: 3.5 against 4.7 ms)
    if (threads == 0) threads = mf <= 64 ? 64 : mf <= 128 ? 128 : mf <= 256 ? 256 : L->rest_lds > c->num_cus ? 256 : mf <= 512 ? 512 : 768;
    return threads;
}
// ... and of the plain batch solver's launch (solver_wg.hpp), likewise shared with the multi-start entry
int wg_launch_threads(const rdis_hip_plan* L) {
    int64_t mf = 0;
    for (size_t i = (size_t)L->rest_tiny; i < L->h_rest.size() - (size_t)L->rest_lds - (size_t)L->rest_ptm; ++i) {
        const int cc = L->h_rest[i];
        mf = std::max<int64_t>(mf, std::max<int64_t>(L->h_fac_ptr[(size_t)cc + 1] - L->h_fac_ptr[(size_t)cc],
                                                     (L->h_free_ptr[(size_t)cc + 1] - L->h_free_ptr[(size_t)cc]) / 4));
    }
    int threads = L->block_threads;
    // More than 512 factors: 768 lanes = three waves per SIMD at 168 registers (a few spills) beat
    // two waves at 250 and four at 128 (heavy spills): +20 % / +40 % throughput on large components,
    // and 5 % on the 361..906-factor camera components of ladybug.
    if (threads == 0) threads = mf <= 64 ? 64 : mf <= 128 ? 128 : mf <= 256 ? 256 : mf <= 512 ? 512 : 768;
    return threads;
}
// a plan made before rdis_hip_nlp_set_exponential marked one of its factors: the reference's gradient asserts the flag off,
// src/NonlinearProductFactor.cpp:110 -- refused at a solve as at plan_create, not solved with values and slopes of two functions
int refuse_late_exponential(rdis_hip_plan* L, const char* who) {
    rdis_hip_problem* p = L->prob;
    if (!p->h_useexp.empty())
        for (int f : L->h_fac_id)
            if (p->h_useexp[(size_t)f])
                return fail(p->ctx, RDIS_HIP_EINVAL, std::string(who) + ": factor " + std::to_string(f) + " is exponential (set after the plan was created); "
                                                     "the reference's gradient asserts it is not (NonlinearProductFactor.cpp:110)");
    return 0;
}
int launch_lds(rdis_hip_plan* L, hipStream_t stream, int threads, int first, int grid, int maxiters, double ftol) {
    rdis_hip_ctx* c = L->prob->ctx;
    ProblemView P = L->prob->view();
    PlanView V = L->view();
    V.order += first;
    // (lds_dyn_bytes is plain lds_bytes_for(...) under the stale cache and the parity option: lds_matrix_on() is false with either)
    HIPCHK(c, solver_set(L->batch_reference_rounding()).launch_lds(L->lds_rot_mode, L->emulate_stale ? 1 : 0, threads, grid, L->lds_dyn_bytes(c), stream, P, V,
                                                                   maxiters, ftol, L->lds_ns_cap, L->lds_ncb_cap, L->lds_chunk_cap));
    return 0;
}
}  // namespace

extern "C" int rdis_hip_plan_solve(rdis_hip_plan* L, int32_t maxiters, double ftol) {
    if (!L || maxiters <= 0) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    USE_DEVICE(c);
    if (int rc = refuse_late_exponential(L, "plan_solve")) return rc;
    if (!L->have_start) { int rc = rdis_hip_plan_set_start(L, nullptr); if (rc) return rc; }
    L->last_launches = 0;
    L->timed = false;
    if (L->ncomp == 0) return 0;

    // a few very large components go to the cooperative multi-workgroup solver, one
    // launch each; everything else is one batched launch, one workgroup per component
    // (also when another plan of the problem has moved the exchange-state buffer this plan's
    // cooperative group tables point into)
    if (L->partition_dirty || (!L->coop.empty() && L->coop_state_gen != p->coop_state_gen)) { int rc = prepare_partition(L); if (rc) return rc; }
    if (L->emulate_stale) {
        // implemented where config 5's components run: the LDS-resident batch solver (and per-factor rotations) -- and, under the
        // parity option, in the cooperative solver's plain layout
        if ((size_t)L->rest_lds != L->h_rest.size() || (!L->coop.empty() && L->factor_rounding != 1) || !L->stream.empty() ||
            (L->rest_lds > 0 && L->lds_rot_mode != ROT_PER_FACTOR))
            return fail(c, RDIS_HIP_EINVAL, "emulate_stale_cache: every component of the plan must run on the LDS-resident batch solver "
                                            "(bundle adjustment, variables fitting a compute unit's LDS; cooperative groups only with factor_rounding = 1)");
        if (!L->st_ev.p) {
            int rc = plan_alloc(L, L->st_ev, (size_t)std::max<int64_t>(L->nfac, 1) * sizeof(int));
            if (!rc) rc = plan_alloc(L, L->st_val, (size_t)std::max<int64_t>(L->nfac, 1) * sizeof(double));
            if (rc) return rc;
        }
    }
    if (L->factor_rounding == 1) {
        // instantiated for the solvers BASELINE's configs 3 - 5 reach: the cooperative ones and the LDS-resident batch solver
        if ((size_t)L->rest_lds != L->h_rest.size() || !L->stream.empty() || p->kind != KIND_BA)
            return fail(c, RDIS_HIP_EINVAL, "factor_rounding = 1: every component of the plan must run on a cooperative solver or on the "
                                            "LDS-resident batch solver (bundle adjustment; no streaming, tiny-component or plain launches)");
        if (!L->seq_val.p) {
            int rc = plan_alloc(L, L->seq_val, (size_t)std::max<int64_t>(L->nfac, 1) * sizeof(double));
            if (!rc) rc = plan_alloc(L, L->seq_ab, 2 * (size_t)std::max<int64_t>(L->nfree, 1) * sizeof(double));
            if (rc) return rc;
        }
    }
    PlanView V = L->view();
    HIPCHK(c, hipEventRecord(p->ev0, c->stream));
    // The batched launch is independent of the cooperative ones (disjoint components): it goes to a
    // second stream and fills the CUs the few workgroups of a cooperative solve leave idle.  The
    // cooperative kernels are enqueued first, so their workgroups are resident before the batch arrives.
    // (not next to a streaming solve: that grid takes every CU and waits for all of its workgroups)
    // (and only when the cooperative launches leave half of the device free: their workgroups must all be
    // resident and take a compute unit each; were the batch to arrive first on a full device, they would
    // wait for it -- serialised, and spinning meanwhile -- instead of running beside it)
    int coop_wg_max = 0;
    for (const CoopLaunch& cl : L->coop_launches) coop_wg_max = std::max(coop_wg_max, cl.total_wg);
    const bool overlap = L->overlap_batch && !L->h_rest.empty() && !L->coop.empty() && L->stream.empty() &&
                         2 * coop_wg_max <= c->num_cus;
    hipStream_t bs = c->stream;
    if (overlap) {
        if (!c->aux) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        }
        bs = c->aux;
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(bs, c->ev_fork, 0));
    }
    for (size_t l = 0; l < L->coop_launches.size(); ++l) {
        const CoopLaunch& cl = L->coop_launches[l];
        const ProblemView PVc = p->view();
        const SolverSet& S = solver_set(L->coop_reference_rounding());
        int rc = L->pipelined()
                     ? S.launch_pipe(c->stream, p->kind, PVc, V, L->h_coop_groups[l][0], cl.groups.as<CoopGroup>(), cl.wg_group.as<int>(),
                                     cl.count, cl.total_wg, maxiters, ftol)
                     : S.launch_coop(c->stream, p->kind, PVc, V, L->h_coop_groups[l][0], cl.groups.as<CoopGroup>(), cl.wg_group.as<int>(),
                                     cl.count, cl.total_wg, L->coop_threads, maxiters, ftol);
        if (rc != 0) return fail(c, RDIS_HIP_EDEVICE, std::string("cooperative solver launch: ") + hipGetErrorString((hipError_t)rc));
        ++L->last_launches;
    }
    for (size_t i = 0; i < L->stream.size(); ++i) {
        const StreamItem& it = L->stream[i];
        StreamArgs sa{p->coop_timing.as<long long>(), p->coop_state.as<CoopState>(), it.long_vars.as<int>(), it.nlong,
                      it.comp, L->coop_poll_delay};
        int rc = launch_stream(c->stream, p->kind, p->view(), V, sa, it.nwg, maxiters, ftol);
        if (rc != 0) return fail(c, RDIS_HIP_EDEVICE, std::string("streaming grid solver launch: ") + hipGetErrorString((hipError_t)rc));
        ++L->last_launches;
    }
    const int rest = (int)L->h_rest.size() - L->rest_tiny - L->rest_lds - L->rest_ptm;   // components of the plain batch solver
    // (the LDS-resident solver forms the records it reads itself)
    if (L->rest_rot_mode != ROT_PER_FACTOR && (L->rest_tiny > 0 || rest > 0)) {   // (cameras the batch reads are not free in the launches above)
        camera_rotations_kernel<<<(int)((p->ncam_blocks + 255) / 256), 256, 0, bs>>>(
            p->x.as<double>(), p->cam_blocks.as<int>(), (int)p->ncam_blocks, p->xrot.as<double>());
        HIPCHK(c, hipGetLastError());
    }
    if (L->rest_tiny > 0) {
        ProblemView PV = p->view();
        PV.xrot = p->xrot.as<double>();
        PV.rot_mode = L->rest_rot_mode == ROT_CAMFIX ? ROT_CAMFIX : ROT_PER_FACTOR;   // (the quad solver has no refresh)
        // persistent groups: as many blocks as are resident, every group draws components until the list is empty
        HIPCHK(c, hipMemsetAsync(L->queue.p, 0, sizeof(int), bs));
        if (L->tiny_group == 4) {
            const int gpb = QUAD_THREADS / 4;
            int grid = std::min((L->rest_tiny + gpb - 1) / gpb, std::max(1, L->group_blocks4));
            if (L->tiny_max_blocks > 0) grid = std::min(grid, L->tiny_max_blocks);
            cgd_group_kernel<4, QUAD_THREADS><<<grid, QUAD_THREADS, 0, bs>>>(
                PV, V, L->rest_order.as<int>(), L->rest_tiny, L->queue.as<int>(), maxiters, ftol);
        } else {
            int grid = std::min((L->rest_tiny + 3) / 4, std::max(1, L->group_blocks16));
            if (L->tiny_max_blocks > 0) grid = std::min(grid, L->tiny_max_blocks);
            cgd_group_kernel<16, 64><<<grid, 64, 0, bs>>>(
                PV, V, L->rest_order.as<int>(), L->rest_tiny, L->queue.as<int>(), maxiters, ftol);
        }
        HIPCHK(c, hipGetLastError());
        ++L->last_launches;
    }
    if (L->rest_lds > 0) {
        int rc = launch_lds(L, bs, lds_launch_threads(L), L->rest_tiny + rest + L->rest_ptm, L->rest_lds, maxiters, ftol);
        if (rc) return rc;
        ++L->last_launches;
    }
    if (L->rest_ptm > 0) {
        int threads = 0, K = 1;
        bool wide = false;
        if (int rc = ptm_launch_shape(L, overlap, &threads, &K, &wide)) return rc;
        L->ptm_last_group = std::max(K, 1);
        L->ptm_last_threads = threads;
        L->ptm_wide_last = wide;
        int rc = K >= 2 ? launch_ptm_groups(L, bs, threads, L->rest_tiny + rest, L->rest_ptm, K, maxiters, ftol, wide)
                        : launch_ptm(L, bs, threads, L->rest_tiny + rest, L->rest_ptm, maxiters, ftol);
        if (rc) return rc;
        ++L->last_launches;
    }
    if (rest > 0) {
        const int threads = wg_launch_threads(L);
        int rc = p->kind == KIND_BA ? launch_wg<KIND_BA>(L, bs, threads, L->rest_tiny, rest, maxiters, ftol)
                                    : launch_wg<KIND_NLP>(L, bs, threads, L->rest_tiny, rest, maxiters, ftol);
        if (rc) return rc;
        ++L->last_launches;
    }
    if (overlap) {
        HIPCHK(c, hipEventRecord(c->ev_join, bs));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    HIPCHK(c, hipEventRecord(p->ev1, c->stream));
    L->timed = true;
    p->last_timed_plan = L;
    if (!L->objective_in_solver) {   // (else the one launch above has stored it: pack_coop_launches)
        objective_sum_kernel<<<1, 256, 0, c->stream>>>((int)L->ncomp, V.fret, L->objective.as<double>());
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int rdis_hip_plan_fetch(rdis_hip_plan* L, double* x_out, double* fret, double* delta, int32_t* iters,
                                   int32_t* status, int64_t* nfeval, int64_t* ngeval) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    const size_t nc = (size_t)L->ncomp, nf = (size_t)L->nfree;
    USE_DEVICE(c);
    if (L->out_bytes == 0) return 0;
    // one D2H copy of the whole results block (x first: skipped when not wanted) -- or, for a long x, two: x straight
    // into the caller's array (no pass through the staging block and no host copy of it: 190 MB for the 1000-component
    // decomposition of the bench's strong-scaling block), the per-component results into the staging block
    const bool direct_x = x_out != nullptr && nf * 8 >= DIRECT_X_BYTES;
    const size_t skip = (x_out && !direct_x) ? 0 : nf * 8;
    if (direct_x) HIPCHK(c, hipMemcpyAsync(x_out, L->outbuf.p, nf * 8, hipMemcpyDeviceToHost, c->stream));
    // (a resident plan's image of the block is pinned and starts at byte h_pin_base of it, plan_create: never behind `skip`)
    const size_t base = L->h_pin.p ? L->h_pin_base : 0;
    char* const img = L->h_pin.p ? L->h_pin.as<char>() : L->h_out.data();
    HIPCHK(c, hipMemcpyAsync(img + (skip - base), static_cast<char*>(L->outbuf.p) + skip, L->out_bytes - skip, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (x_out && !direct_x) std::memcpy(x_out, img, nf * 8);
    const char* h = img + (nf * 8 - base);   // the per-component results
    if (fret) std::memcpy(fret, h, nc * 8);
    if (delta) std::memcpy(delta, h + nc * 8, nc * 8);
    const char* i64 = h + 2 * nc * 8;
    if (nfeval) std::memcpy(nfeval, i64, nc * 8);
    if (ngeval) std::memcpy(ngeval, i64 + nc * 8, nc * 8);
    const char* i32 = i64 + 2 * nc * 8;
    if (iters) std::memcpy(iters, i32, nc * 4);
    if (status) std::memcpy(status, i32 + nc * 4, nc * 4);
    return 0;
}

// =====================================================================================
// multi-start solves: one plan, many starting points, one launch (solver_lds_starts.hpp, solver_wg_starts.hpp)
// =====================================================================================
namespace {
// why a plan cannot be solved from many starts yet.  Two kinds of plan can: every component on the LDS-resident solver (bundle
// adjustment), or a nonlinear-product problem with every component on the plain batch solver -- *plain_solver says which
// (entry: "multi-start" or "population" -- rdis_hip_plan_solve_population shares these checks)
// (allow_tiny: the population entry with the plan option population_tiny -- tiny components beside LDS-resident ones pass;
// allow_ptm: with population_point_major, point-major components too -- the entry itself then asks for one workgroup a component;
// allow_coop: rdis_hip_plan_solve_population_cooperative -- cooperative components pass, in the plain layout and beside no grid solver)
int starts_refusal(rdis_hip_plan* L, const char* who, bool* plain_solver, const char* entry = "multi-start", bool allow_tiny = false, bool allow_ptm = false,
                   bool allow_coop = false) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    const std::string w(who), en(entry);
    if (L->transient) return fail(c, RDIS_HIP_EINVAL, w + ": needs a persistent plan");
    if (L->factor_rounding == 1) return fail(c, RDIS_HIP_EINVAL, w + ": the parity option (factor_rounding = 1) has no " + en + " entry");
    if (L->emulate_stale) return fail(c, RDIS_HIP_EINVAL, w + ": emulate_stale_cache has no " + en + " entry");
    if (L->trace_records > 0) return fail(c, RDIS_HIP_EINVAL, w + ": trace_records must be 0 (a trace belongs to one solve)");
    if (L->dump_iters > 0) return fail(c, RDIS_HIP_EINVAL, w + ": dump_iters must be 0 (a vector dump belongs to one solve)");
    if (L->partition_dirty || (!L->coop.empty() && L->coop_state_gen != p->coop_state_gen)) { int rc = prepare_partition(L); if (rc) return rc; }
    // an empty component (no factor: no table, nothing to solve) runs on either solver
    int64_t tiny = 0, ptm = 0, plain = 0;
    const size_t r_lds = L->h_rest.size() - (size_t)L->rest_lds, r_ptm = r_lds - (size_t)L->rest_ptm;
    for (size_t r = 0; r < r_lds; ++r) {
        const int cc = L->h_rest[r];
        if (L->h_fac_ptr[(size_t)cc + 1] == L->h_fac_ptr[(size_t)cc]) continue;
        if (r < (size_t)L->rest_tiny) ++tiny; else if (r >= r_ptm) ++ptm; else ++plain;
    }
    if (allow_coop && !L->stream.empty()) return fail(c, RDIS_HIP_EINVAL, population_coop_grid_refusal(who, (int64_t)L->stream.size()));
    if (allow_coop && !L->coop.empty() && L->use_pipe) return fail(c, RDIS_HIP_EINVAL, population_coop_pipelined_refusal(who));
    std::string others;
    auto note = [&](int64_t count, const char* solver) { if (count > 0) others += (others.empty() ? " " : ", ") + std::to_string(count) + " to the " + solver; };
    if (!allow_coop) note((int64_t)L->coop.size(), "cooperative solver");
    note((int64_t)L->stream.size(), "grid solver");
    if (!allow_tiny) note(tiny, "tiny-component solver");
    if (!allow_ptm) note(ptm, "point-major streaming solver");
    const bool plain_ok = plain > 0 && p->kind == KIND_NLP && others.empty();
    if (!plain_ok) note(plain, "plain batch solver");
    if (!others.empty()) {
        // (a bundle-adjustment component there reads its cameras' rotation records, ProblemView::xrot: they would need replicas too)
        const std::string ba_plain = plain > 0 && p->kind == KIND_BA ? " (bundle-adjustment components on the plain batch solver have no " + en + " entry, alone or "
                                                                       "beside LDS-resident ones: their rotation records would need replicas too)" : "";
        // (the population entry takes tiny components with an option of their own; the multi-start entry does not)
        const std::string tiny_hint = tiny > 0 && !allow_tiny && en == "population" ? " (tiny components are solved on a population with the plan option "
                                                                                      "population_tiny = 1: solver_quad_population.hpp)" : "";
        const std::string ptm_hint = ptm > 0 && !allow_ptm && en == "population" ? " (point-major components are solved on a population, one workgroup each, with "
                                                                                   "the plan option population_point_major = 1: solver_ptm_population.hpp)" : "";
        const std::string coop_hint = !L->coop.empty() && !allow_coop && en == "population" ? population_coop_hint() : "";
        return fail(c, RDIS_HIP_EINVAL, w + ": every component of the plan must run on the LDS-resident solver (bundle adjustment, variables fitting a "
                                        "compute unit's LDS) or, all of them, on the plain batch solver of a nonlinear-product problem; this plan sends" +
                                        others + ba_plain + tiny_hint + ptm_hint + coop_hint);
    }
    *plain_solver = plain_ok;
    return 0;
}

// rdis_hip_plan_fetch_starts and rdis_hip_plan_fetch_population: the rows of the last such solve (best: the former's only)
int fetch_many(rdis_hip_plan* L, bool population, double* x_out, double* fret, double* delta, int32_t* iters, int32_t* status, int64_t* nfeval,
               int64_t* ngeval, int32_t* best) {
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (L->ms_n < 1)
        return fail(c, RDIS_HIP_EINVAL, population ? "plan_fetch_population: no population solve to fetch (call rdis_hip_plan_solve_population first)"
                                                   : "plan_fetch_starts: no multi-start solve to fetch (call rdis_hip_plan_solve_starts first)");
    if (L->ms_population != population)
        return fail(c, RDIS_HIP_EINVAL, population ? "plan_fetch_population: the plan's last solve of this kind was a multi-start solve (fetch it with rdis_hip_plan_fetch_starts)"
                                                   : "plan_fetch_starts: the plan's last solve of this kind was a population solve (fetch it with rdis_hip_plan_fetch_population)");
    if (L->ncomp == 0) return 0;
    // every array is one contiguous piece of the outputs' block: straight into the caller's memory
    const StartsView S = L->starts_view(L->ms_n);
    const size_t sn = (size_t)L->ms_n * (size_t)L->nfree, sc = (size_t)L->ms_n * (size_t)L->ncomp;
    auto get = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIPCHK(c, get(x_out, S.xout, sn * 8));
    HIPCHK(c, get(fret, S.fret, sc * 8));
    HIPCHK(c, get(delta, S.delta, sc * 8));
    HIPCHK(c, get(nfeval, S.nfeval, sc * 8));
    HIPCHK(c, get(ngeval, S.ngeval, sc * 8));
    HIPCHK(c, get(iters, S.iters, sc * 4));
    HIPCHK(c, get(status, S.status, sc * 4));
    if (!population) HIPCHK(c, get(best, L->ms_best.p, (size_t)L->ncomp * 4));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The per-call buffers of both solve entries, grown where an earlier call left them too small, in this order: the launch's
// replicas (ms_work; ms_dir, which is zeroed here once -- the kernel leaves what it wrote zero again), the tiny-component launch's
// queue counters (0 bytes: it does not run), the start rows and the outputs of the call's n starts or members.
int grow_solve_buffers(rdis_hip_plan* L, size_t work_bytes, size_t dir_bytes, size_t queue_bytes, int64_t n) {
    rdis_hip_ctx* c = L->prob->ctx;
    int rc = 0;
    if (L->ms_work.bytes < work_bytes) rc = plan_alloc(L, L->ms_work, work_bytes);
    if (!rc && L->ms_dir.bytes < dir_bytes) {
        rc = plan_alloc(L, L->ms_dir, dir_bytes);
        if (!rc) HIPCHK(c, hipMemsetAsync(L->ms_dir.p, 0, L->ms_dir.bytes, c->stream));
    }
    if (!rc && L->ms_queue.bytes < queue_bytes) rc = plan_alloc(L, L->ms_queue, queue_bytes);
    const size_t in_bytes = (size_t)n * (size_t)L->nfree * sizeof(double);
    if (!rc && L->ms_in.bytes < in_bytes) rc = plan_alloc(L, L->ms_in, in_bytes);
    if (!rc && L->ms_out.bytes < L->ms_out_bytes(n)) rc = plan_alloc(L, L->ms_out, L->ms_out_bytes(n));
    return rc;
}

// behind the last launch of either entry: the end of the stretch rdis_hip_plan_last_kernel_ms reports ...
int end_timed_launches(rdis_hip_plan* L) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    HIPCHK(c, hipEventRecord(p->ev1, c->stream));
    L->timed = true;
    p->last_timed_plan = L;
    return 0;
}
// ... and what fetch_many and plan_get_info read of the call: n rows, R of them a launch, the launches counted in last_launches
void note_many_solve(rdis_hip_plan* L, bool population, int64_t n, int64_t R) {
    L->ms_population = population;
    L->ms_n = n;
    L->ms_per_launch = R;
    L->ms_launches = L->last_launches;
}
// a plan without components: nothing is launched, and n rows of nothing can be fetched
void note_empty_solve(rdis_hip_plan* L, bool population, int64_t n) {
    L->last_launches = 0;
    L->timed = false;
    note_many_solve(L, population, n, n);
}
}  // namespace

extern "C" int rdis_hip_plan_solve_starts(rdis_hip_plan* L, int64_t nstarts, const double* x_starts, int32_t maxiters, double ftol) {
    if (!L) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    USE_DEVICE(c);
    if (maxiters <= 0) return fail(c, RDIS_HIP_EINVAL, "plan_solve_starts: maxiters must be positive");
    if (nstarts < 1) return fail(c, RDIS_HIP_EINVAL, "plan_solve_starts: nstarts must be at least 1");
    if (!x_starts) return fail(c, RDIS_HIP_EINVAL, "plan_solve_starts: x_starts is NULL (a row of start values per start)");
    if (too_many_rows(nstarts, std::max<int64_t>(std::max(L->nfree, L->ncomp), 1)))
        return fail(c, RDIS_HIP_ERANGE, "plan_solve_starts: too many starts");
    if (int rc = refuse_late_exponential(L, "plan_solve_starts")) return rc;
    bool plain = false;
    if (int rc = starts_refusal(L, "plan_solve_starts", &plain)) return rc;
    if (L->ncomp == 0) { note_empty_solve(L, false, nstarts); return 0; }

    // replicas of the per-solve workspace (ws, gfac; the plain solver's x and dir too) a launch may hold within the budget: at least one
    const ReplicaLayout work = starts_work_layout(L->nfree, L->ngfac, plain, p->N), dir = solve_dir_layout(plain, p->N);
    const int64_t R = members_per_launch(nstarts, L->starts_workspace_bytes, work.member_bytes() + dir.member_bytes());
    int rc = grow_solve_buffers(L, (size_t)work.total_bytes(R), (size_t)dir.total_bytes(R), 0, nstarts);
    const size_t in_bytes = (size_t)nstarts * (size_t)L->nfree * sizeof(double);
    if (!rc && !L->ms_best.p) rc = plan_alloc(L, L->ms_best, (size_t)L->ncomp * sizeof(int));
    if (rc) return rc;
    L->ms_n = 0;   // (what an earlier call left is overwritten from here on)
    L->ms_population = false;

    // the starts: through pinned memory, so that the caller may reuse x_starts the moment this returns and nothing waits
    if (in_bytes > 0 && in_bytes <= STARTS_STAGE_MAX_BYTES) {
        if (L->ms_stage_busy) { HIPCHK(c, hipEventSynchronize(L->ms_stage_ev)); L->ms_stage_busy = false; }
        if (L->ms_stage.bytes < in_bytes) { rc = halloc(c, L->ms_stage, in_bytes); if (rc) return rc; }
        if (!L->ms_stage_ev) HIPCHK(c, hipEventCreateWithFlags(&L->ms_stage_ev, hipEventDisableTiming));
        std::memcpy(L->ms_stage.p, x_starts, in_bytes);
        HIPCHK(c, hipMemcpyAsync(L->ms_in.p, L->ms_stage.p, in_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(L->ms_stage_ev, c->stream));
        L->ms_stage_busy = true;
    } else if (in_bytes > 0) {
        HIPCHK(c, hipMemcpyAsync(L->ms_in.p, x_starts, in_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }

    const ProblemView P = p->view();
    PlanView V = L->view();   // (order: the whole batch list -- empty components and those of the plan's one solver, heaviest first)
    StartsView S = L->starts_view(nstarts);
    S.gfac = work.at<double>(S.ws, STARTS_GFAC, R);
    const int threads = plain ? wg_launch_threads(L) : L->rest_lds > 0 ? lds_launch_threads(L) : 64;
    const size_t dyn = L->lds_dyn_bytes(c);
    if (plain) {   // every replica's x: the problem's, for the constants (solver_wg_starts.hpp; once per call)
        S.x = work.at<double>(S.ws, STARTS_X, R);
        S.dir = L->ms_dir.as<double>();
        HIPCHK(c, starts_fill_x_launch(c->stream, P, S, R));
    }
    L->last_launches = 0;
    L->timed = false;
    HIPCHK(c, hipEventRecord(p->ev0, c->stream));
    for (int64_t first = 0; first < nstarts; first += R) {   // (launches on one stream: the next takes the replicas when this one is done)
        S.first = first;
        const int ns = (int)std::min(R, nstarts - first);
        if (plain) HIPCHK(c, starts_launch_wg(threads, (int)L->h_rest.size(), ns, c->stream, P, V, S, maxiters, ftol));
        else HIPCHK(c, starts_launch(L->lds_rot_mode, threads, (int)L->h_rest.size(), ns, dyn, c->stream, P, V, S,
                                     maxiters, ftol, L->lds_ns_cap, L->lds_ncb_cap, L->lds_chunk_cap));
        ++L->last_launches;
    }
    if ((rc = end_timed_launches(L))) return rc;
    // what the node keeps: the best start per component, as the plan's ordinary outputs and the assignment of its variables
    S.first = 0;
    HIPCHK(c, starts_select_launch(c->stream, P, V, S, nstarts, L->ms_best.as<int>()));
    objective_sum_kernel<<<1, 256, 0, c->stream>>>((int)L->ncomp, V.fret, L->objective.as<double>());
    HIPCHK(c, hipGetLastError());
    note_many_solve(L, false, nstarts, R);
    return 0;
}

extern "C" int rdis_hip_plan_fetch_starts(rdis_hip_plan* L, double* x_out, double* fret, double* delta, int32_t* iters, int32_t* status,
                                          int64_t* nfeval, int64_t* ngeval, int32_t* best) {
    if (!L) return RDIS_HIP_EINVAL;
    return fetch_many(L, false, x_out, fret, delta, iters, status, nfeval, ngeval, best);
}

// =====================================================================================
// populations: S complete states on the device, a plan solved on all of them at once (solver_lds_population.hpp; with the plan
// option population_plain, solver_wg_population.hpp for nonlinear-product plans)
// (rdis_hip_plan_solve_population_cooperative: the components of the cooperative solver too, solver_coop_population.hpp)
// (struct rdis_hip_population: population_state.hpp; the rdis_hip_population_* entries: population_entries.hip)
// =====================================================================================
namespace {
// rdis_hip_plan_solve_population on members first0 .. first0 + S_n - 1: the member base is X + first0 N, the per-call arrays
// (start rows, outputs, replicas) are sized and indexed for the S_n members of the range, so member first0 + i is row i of
// plan_fetch_population.  `who` names the entry in messages.
// `cooperative` (rdis_hip_plan_solve_population_cooperative): the components rdis_hip_plan_solve sends to the cooperative solver are
// taken too -- per range of R members one launch of cgd_coop_population_kernel for each CoopLaunch of the plan, on the context's
// stream, before the other kinds (the overlap_batch side stream is not used).  The replicas and exchange states are the plan's own
// (ms_coop): the problem's coop_state is neither used nor moved, so no other plan's group tables go stale.
int solve_population_range(rdis_hip_plan* L, rdis_hip_population* pop, int64_t first0, const int64_t S_n, int32_t maxiters, double ftol, const char* who_name,
                           bool cooperative = false) {
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    const std::string who(who_name);
    if (maxiters <= 0) return fail(c, RDIS_HIP_EINVAL, who + ": maxiters must be positive");
    if (pop->prob != p) return fail(c, RDIS_HIP_EINVAL, who + ": the population belongs to another problem than the plan's");
    if (p->kind != KIND_BA && !L->population_plain)
        return fail(c, RDIS_HIP_EINVAL, who + ": nonlinear-product plans are solved on a population only with the plan option population_plain = 1 "
                                        "(the plain batch solver, solver_wg_population.hpp; without it: bundle adjustment on the LDS-resident solver only)");
    if (too_many_rows(S_n, std::max<int64_t>(std::max(L->nfree, L->ncomp), 1)))
        return fail(c, RDIS_HIP_ERANGE, who + ": too many members");
    if (int rc = refuse_late_exponential(L, who_name)) return rc;   // (nonlinear products only: no bundle-adjustment factor is exponential)
    bool plain = false;
    if (int rc = starts_refusal(L, who_name, &plain, "population", L->population_tiny != 0, L->population_point_major != 0, cooperative)) return rc;
    // point-major components (option population_point_major: the refusal above let them pass) run as one workgroup a component, the
    // bits of launch_ptm -- a group, a wide group or local camera numbering changes the order of every sum
    const int nptm = (L->population_point_major && !plain) ? L->rest_ptm : 0;
    int ptm_threads = 0;
    if (nptm > 0) {
        int K = 1;
        bool wide = false;
        if (int rc = ptm_launch_shape(L, false, &ptm_threads, &K, &wide)) return rc;
        if (K >= 2)
            return fail(c, RDIS_HIP_EINVAL, who + ": point-major components are solved on a population as one workgroup a component, and this plan's "
                                            "ordinary solve would run them as " + std::string(wide ? "wide " : "") + "groups of " + std::to_string(K) +
                                            " workgroups (other sums, other bits): set the plan option ptm_group = 1");
    }
    // What the cooperative launches need of a member: gfac, the groups' directions and an exchange state a group; every workgroup of
    // such a launch is resident, which bounds R a second time -- by the NEW kernel's occupancy (solver_coop_population.hpp).  The
    // plan's launches were packed under the ordinary kernel's cap (pack_coop_launches): one that does not fit the new kernel's even
    // with a single member is refused here, before any row is written, not left to the runtime to reject
    const bool coop = cooperative && !L->coop.empty();
    const SolverSet& CS = solver_set(L->coop_reference_rounding());
    int64_t coop_groups = 0, coop_wg = 0, xi_doubles = 0;
    int coop_cap_wg = 0;
    if (coop) {
        for (const CoopLaunch& cl : L->coop_launches) { coop_groups = std::max<int64_t>(coop_groups, cl.count); coop_wg = std::max<int64_t>(coop_wg, cl.total_wg); }
        for (const CoopItem& it : L->coop) xi_doubles += L->h_free_ptr[(size_t)it.comp + 1] - L->h_free_ptr[(size_t)it.comp];
        const int ti = L->coop_threads == 128 ? 0 : L->coop_threads == 256 ? 1 : 2;
        int& cap = L->coop_reference_rounding() ? c->cap_coop_pop_rr[ti] : c->cap_coop_pop[ti];   // (asked once per context and layout: coop_cap)
        if (cap < 0) cap = CS.coop_population_max_workgroups(L->coop_threads, c->num_cus);
        coop_cap_wg = cap;
        if (coop_wg > coop_cap_wg) return fail(c, RDIS_HIP_EINVAL, population_coop_residency_refusal(who_name, coop_wg, coop_cap_wg));
    }
    pop->x_written();
    if (L->ncomp == 0) { note_empty_solve(L, true, S_n); return 0; }

    // what a launch runs: the tiny-component solver on the first rest_tiny entries of the batch list (option population_tiny: the
    // refusal above let them pass), the LDS-resident or the plain solver on the entries behind them, where there are any
    // (without the option nothing but empty components can be among the first rest_tiny: the whole list goes to the other solver, as before)
    // With point-major components the list behind the tiny ones splits once more: the point-major kernel takes the entries up to
    // the LDS-resident slice (empty components among them: it knows them), the LDS-resident kernel its own slice
    const int ntiny = (L->population_tiny && !plain) ? L->rest_tiny : 0;
    const int nptm_listed = nptm > 0 ? (int)L->h_rest.size() - ntiny - L->rest_lds : 0;
    const int nlisted = (int)L->h_rest.size() - ntiny - nptm_listed;
    const bool tiny_records = ntiny > 0 && L->rest_rot_mode == ROT_CAMFIX;   // (the tiny launch reads rotation records: a replica per member)
    // replicas a launch may hold within the budget, the multi-start entry's rule.  A replica holds only what the launch's kernels
    // read: ws and gfac where the LDS-resident or the plain solver runs (the plain solver's dir too -- its x is the member's row),
    // the cameras' rotation records [N] where the tiny-component solver reads records
    const ReplicaLayout work = population_work_layout(nlisted > 0, L->nfree, L->ngfac, tiny_records, p->N), dir = solve_dir_layout(plain, p->N);
    // ... and the four per-solve arrays of the point-major solver
    const ReplicaLayout ptm = population_ptm_layout(nptm > 0 ? L->pm_blocks : 0, L->pm_cptr_len);
    const ReplicaLayout cw = population_coop_layout(L->ngfac, xi_doubles, coop_groups, (int64_t)sizeof(CoopState));
    const int64_t R = coop_members_per_launch(S_n, L->starts_workspace_bytes, work.member_bytes() + dir.member_bytes() + ptm.member_bytes() + cw.member_bytes(),
                                              coop_cap_wg, coop_wg);
    int rc = 0;
    if (coop && L->ms_coop.bytes < (size_t)cw.total_bytes(R) && (rc = plan_alloc(L, L->ms_coop, (size_t)cw.total_bytes(R)))) return rc;
    if (nptm > 0) {
        // the round tables of that workgroup size, one workgroup a component, before the first launch (launch_ptm's)
        rc = ptm_build_rounds(L, ptm_threads, 1);
        if (!rc && L->ms_ptm.bytes < (size_t)ptm.total_bytes(R)) rc = plan_alloc(L, L->ms_ptm, (size_t)ptm.total_bytes(R));
        if (rc) return rc;
    }
    rc = grow_solve_buffers(L, (size_t)work.total_bytes(R), (size_t)dir.total_bytes(R), ntiny > 0 ? (size_t)R * sizeof(int) : 0, S_n);
    if (rc) return rc;
    L->ms_n = 0;   // (what an earlier call left is overwritten from here on)

    double* const Xb = pop->row(first0);   // the range's member 0: every launch below counts its members from here
    const ProblemView P = p->view();
    PlanView V = L->view();   // (order: the whole batch list -- tiny components first, then empty ones and those of the plan's other solver, heaviest first)
    StartsView S = L->starts_view(S_n);
    S.gfac = work.at<double>(S.ws, POPULATION_GFAC, R);
    double* const XR = tiny_records ? work.at<double>(S.ws, POPULATION_ROT, R) : nullptr;   // [R][N], behind the launch's replicas of ws and gfac
    if (plain) S.dir = L->ms_dir.as<double>();   // (no replica of x: the member's row serves, solver_wg_population.hpp)
    // every member's start row: its own x at the plan's free variables (plan_set_start(plan, NULL) on that x)
    HIPCHK(c, population_gather_launch(c->stream, Xb, p->N, V.free_vid, L->nfree, S_n, L->ms_in.as<double>()));
    const int threads = plain ? wg_launch_threads(L) : L->rest_lds > 0 ? lds_launch_threads(L) : 64;
    const size_t dyn = L->lds_dyn_bytes(c);
    ProblemView PT = P;   // the tiny launch's: records of the launch's members or per-factor rotations (the quad solver has no refresh)
    PT.rot_mode = tiny_records ? ROT_CAMFIX : ROT_PER_FACTOR;
    PlanView VM = V;      // the point-major launch's: the batch list behind the tiny components, up to the LDS-resident slice
    VM.order = V.order + ntiny;
    PlanView VR = V;      // the other launch's: the rest of the batch list
    VR.order = V.order + ntiny + nptm_listed;
    // the launch's replicas of pm_rec, pm_gh, pm_bex (six doubles a point block each) and, behind them, of pm_cbox
    PtmReplicas RP{nullptr, nullptr, nullptr, nullptr, L->pm_blocks, L->pm_cptr_len};
    if (nptm > 0) {
        void* const base = L->ms_ptm.p;
        RP.rec = ptm.at<double>(base, PTM_REPLICA_REC, R); RP.gh = ptm.at<double>(base, PTM_REPLICA_GH, R);
        RP.bex = ptm.at<double>(base, PTM_REPLICA_BEX, R); RP.cbox = ptm.at<float>(base, PTM_REPLICA_CBOX, R);
    }
    const size_t ptm_dyn = nptm > 0 ? ptm_bytes_for(L->ptm_ncb_cap, ptm_threads, L->rounds_slots) : 0;
    // the cooperative launches' view of the per-solve arrays: gfac is their own replica (a member's stride: the padded part)
    StartsView SC = S;
    // (RC.timing, the trailing null, must stay a value the kernel learns at run time: written into the kernel as a constant it
    // stops this compiler's gfx950 backend on the reference-rounding instantiation -- solver_coop_population.hpp; both SolverSet
    // tables launch with this RC)
    CoopReplicas RC{nullptr, L->xi_glob.as<double>(), 0, nullptr, (int)coop_groups, nullptr};
    if (coop) {
        void* const base = L->ms_coop.p;
        SC.gfac = cw.at<double>(base, COOP_REPLICA_GFAC, R); SC.ngfac = cw.doubles(COOP_REPLICA_GFAC);
        RC.xi = cw.at<double>(base, COOP_REPLICA_XI, R); RC.xi_doubles = cw.doubles(COOP_REPLICA_XI);
        RC.st = cw.at<CoopState>(base, COOP_REPLICA_STATE, R);
    }
    L->last_launches = 0;
    L->ms_coop_wg = (int)coop_wg; L->ms_coop_cap = coop ? coop_cap_wg : 0;
    L->ms_tiny_blocks = 0;
    L->ms_ptm_threads = nptm > 0 ? ptm_threads : 0;
    L->timed = false;
    HIPCHK(c, hipEventRecord(p->ev0, c->stream));
    for (int64_t first = 0; first < S_n; first += R) {   // (launches on one stream: the next takes the replicas when this one is done)
        S.first = first;
        const int ns = (int)std::min(R, S_n - first);
        if (coop) {
            SC.first = first;
            for (const CoopLaunch& cl : L->coop_launches) {   // (the states of this launch's groups are armed in front of it, for its members)
                const int e = CS.launch_coop_population(c->stream, p->kind, P, V, SC, RC, Xb, cl.groups.as<CoopGroup>(), cl.wg_group.as<int>(), cl.count,
                                                        cl.total_wg, ns, L->coop_threads, maxiters, ftol);
                if (e != 0) return fail(c, RDIS_HIP_EDEVICE, who + ": cooperative solver launch: " + hipGetErrorString((hipError_t)e));
                ++L->last_launches;
            }
        }
        if (ntiny > 0) {
            // the records of THIS launch's members: the replicas held another launch's until now (solver_quad_population.hpp)
            if (tiny_records) HIPCHK(c, population_rotations_launch(c->stream, Xb, p->N, first, ns, p->cam_blocks.as<int>(), (int)p->ncam_blocks, XR));
            HIPCHK(c, hipMemsetAsync(L->ms_queue.p, 0, (size_t)ns * sizeof(int), c->stream));
            const int G = L->tiny_group == 4 ? 4 : 16;
            const int gx = tiny_population_blocks(ntiny, (G == 4 ? QUAD_THREADS : 64) / G, L->tiny_population_fill * std::max(1, G == 4 ? L->group_blocks4 : L->group_blocks16), ns, L->tiny_max_blocks);
            HIPCHK(c, population_launch_tiny(G, gx, ns, c->stream, PT, V, S, Xb, XR, L->rest_order.as<int>(), ntiny, L->ms_queue.as<int>(), maxiters, ftol));
            L->ms_tiny_blocks = gx;
            ++L->last_launches;
        }
        if (nptm_listed > 0) {
            HIPCHK(c, population_launch_ptm(L->ptm_rot_mode, ptm_threads, nptm_listed, ns, ptm_dyn, c->stream, P, VM, S, RP, Xb, maxiters, ftol,
                                            L->ptm_ncb_cap));
            ++L->last_launches;
        }
        if (nlisted > 0) {
            if (plain) HIPCHK(c, population_launch_wg(threads, nlisted, ns, c->stream, P, VR, S, Xb, maxiters, ftol));
            else HIPCHK(c, population_launch(L->lds_rot_mode, threads, nlisted, ns, dyn, c->stream, P, VR, S, Xb,
                                        maxiters, ftol, L->lds_ns_cap, L->lds_ncb_cap, L->lds_chunk_cap));
            ++L->last_launches;
        }
    }
    if ((rc = end_timed_launches(L))) return rc;
    note_many_solve(L, true, S_n, R);
    return 0;
}
}  // namespace

extern "C" int rdis_hip_plan_solve_population(rdis_hip_plan* L, rdis_hip_population* pop, int32_t maxiters, double ftol) {
    if (!L || !pop) return RDIS_HIP_EINVAL;
    USE_DEVICE(L->prob->ctx);
    return solve_population_range(L, pop, 0, pop->nmembers, maxiters, ftol, "plan_solve_population");
}

extern "C" int rdis_hip_plan_solve_population_range(rdis_hip_plan* L, rdis_hip_population* pop, int64_t first, int64_t count, int32_t maxiters,
                                                    double ftol) {
    if (!L || !pop) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (count < 1 || first < 0 || first > pop->nmembers || count > pop->nmembers - first)
        return fail(c, RDIS_HIP_EINVAL, "plan_solve_population_range: members out of range (count >= 1, first + count <= nmembers)");
    return solve_population_range(L, pop, first, count, maxiters, ftol, "plan_solve_population_range");
}

extern "C" int rdis_hip_plan_solve_population_cooperative(rdis_hip_plan* L, rdis_hip_population* pop, int64_t first, int64_t count, int32_t maxiters,
                                                          double ftol) {
    if (!L || !pop) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (count < 1 || first < 0 || first > pop->nmembers || count > pop->nmembers - first)
        return fail(c, RDIS_HIP_EINVAL, "plan_solve_population_cooperative: members out of range (count >= 1, first + count <= nmembers)");
    return solve_population_range(L, pop, first, count, maxiters, ftol, "plan_solve_population_cooperative", true);
}

extern "C" int rdis_hip_plan_fetch_population(rdis_hip_plan* L, double* x_out, double* fret, double* delta, int32_t* iters, int32_t* status,
                                              int64_t* nfeval, int64_t* ngeval) {
    if (!L) return RDIS_HIP_EINVAL;
    return fetch_many(L, true, x_out, fret, delta, iters, status, nfeval, ngeval, nullptr);
}

extern "C" int rdis_hip_plan_last_kernel_ms(rdis_hip_plan* L, double* ms, int32_t* launches) {
    if (!L || !ms) return RDIS_HIP_EINVAL;
    rdis_hip_problem* p = L->prob;
    rdis_hip_ctx* c = p->ctx;
    *ms = 0.0;
    USE_DEVICE(c);
    if (launches) *launches = L->last_launches;
    if (!L->timed || p->last_timed_plan != L) return 0;  // the events belong to the problem's last solve
    HIPCHK(c, hipEventSynchronize(p->ev1));
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, p->ev0, p->ev1));
    *ms = t;
    return 0;
}

extern "C" int rdis_hip_components(rdis_hip_problem* p, const uint8_t* assigned, int64_t* ncomp, int64_t* nfree, int64_t* nfac) {
    if (!p) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = p->ctx;
    if (!assigned && p->N > 0) return fail(c, RDIS_HIP_EINVAL, "components: assigned is null");
    USE_DEVICE(c);
    if (p->N >= INT32_MAX || p->F >= INT32_MAX) return fail(c, RDIS_HIP_ERANGE, "components: problem too large for 32-bit ids");
    int rc = dalloc(c, p->assigned, (size_t)std::max<int64_t>(p->N, 1));
    if (rc) return rc;
    if (p->N > 0) HIPCHK(c, hipMemcpyAsync(p->assigned.p, assigned, (size_t)p->N, hipMemcpyHostToDevice, c->stream));
    const int e = device_components(c->stream, p->kind, (int)p->N, (int)p->F, p->cam.as<int>(), p->pt.as<int>(),
                                    p->rowptr.as<int>(), p->vid.as<int>(), p->assigned.as<unsigned char>(), &p->cc_ws, &p->comps);
    if (e != 0) return fail(c, RDIS_HIP_EDEVICE, std::string("components: ") + hipGetErrorString((hipError_t)e));
    if (ncomp) *ncomp = p->comps.ncomp;
    if (nfree) *nfree = p->comps.nfree;
    if (nfac) *nfac = p->comps.nfac;
    return 0;
}

extern "C" int rdis_hip_components_fetch(rdis_hip_problem* p, int64_t* free_ptr, int64_t* free_vid, int64_t* fac_ptr, int64_t* fac_id) {
    if (!p) return RDIS_HIP_EINVAL;
    const ComponentLists& L = p->comps;
    if (L.free_ptr.empty()) return fail(p->ctx, RDIS_HIP_EINVAL, "components_fetch: call rdis_hip_components first");
    if (free_ptr) std::memcpy(free_ptr, L.free_ptr.data(), L.free_ptr.size() * sizeof(int64_t));
    if (fac_ptr) std::memcpy(fac_ptr, L.fac_ptr.data(), L.fac_ptr.size() * sizeof(int64_t));
    if (free_vid && !L.free_vid.empty()) std::memcpy(free_vid, L.free_vid.data(), L.free_vid.size() * sizeof(int64_t));
    if (fac_id && !L.fac_id.empty()) std::memcpy(fac_id, L.fac_id.data(), L.fac_id.size() * sizeof(int64_t));
    return 0;
}

// one optimize() call: a transient plan in the problem's arena -- no hipMalloc / hipFree, one
// H2D copy of the decomposition, one of the start, the launch(es), one D2H copy of the results
extern "C" int rdis_hip_cgd_batch(rdis_hip_problem* p, int64_t ncomp, const int64_t* free_ptr,
                                  const int64_t* free_vid, const int64_t* fac_ptr, const int64_t* fac_id,
                                  double* x_inout, int32_t maxiters, double ftol, double* fret, double* delta,
                                  int32_t* iters, int32_t* status, int64_t* nfeval, int64_t* ngeval) {
    rdis_hip_plan* L = nullptr;
    // RDIS_HIP_TIMING=1: where a one-shot call's host time goes (stderr), for the tuning of this path
    static const bool timing = std::getenv("RDIS_HIP_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = timing ? now() : 0.0;
    int rc = plan_create_impl(p, true, ncomp, free_ptr, free_vid, fac_ptr, fac_id, &L);
    if (rc) return rc;
    const double t1 = timing ? now() : 0.0;
    rc = rdis_hip_plan_set_start(L, x_inout);
    double t2 = 0.0, t3 = 0.0;
    if (!rc && timing) { t2 = now(); rc = prepare_partition(L); t3 = now(); }
    if (!rc) rc = rdis_hip_plan_solve(L, maxiters, ftol);
    const double t4 = timing ? now() : 0.0;
    if (!rc) rc = rdis_hip_plan_fetch(L, x_inout, fret, delta, iters, status, nfeval, ngeval);
    if (timing)
        std::fprintf(stderr, "rdis_hip_cgd_batch: lists + index tables %.3f ms, start %.3f, partition %.3f, launch %.3f, wait + results %.3f\n",
                     t1 - t0, t2 - t1, t3 - t2, t4 - t3, now() - t4);
    if (rc) {   // kernels or copies that use the plan's host staging vectors / arena slices may still be queued
        (void)hipStreamSynchronize(p->ctx->stream);
        if (p->ctx->aux) (void)hipStreamSynchronize(p->ctx->aux);
    }
    rdis_hip_plan_destroy(L);
    return rc;
}
