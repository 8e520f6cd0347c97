// plan_query.hip -- the C ABI's query and debug entries of a plan (include/rdis_hip.h): what the partition decided, device
// memory, trace, counters and vector dump, the objective's device address.  Host code only, and none of it on a path that a
// benchmark times (rdis_hip_plan_last_kernel_ms, which bench.py calls in every timed step, is rdis_hip.hip's).
#include "abi_state.hpp"

extern "C" int rdis_hip_plan_objective_device(rdis_hip_plan* L, void** dev_ptr) {
    if (!L || !dev_ptr) return RDIS_HIP_EINVAL;
    *dev_ptr = L->objective.p;
    return 0;
}

extern "C" int rdis_hip_plan_get_info(rdis_hip_plan* L, const char* name, int64_t* value) {
    if (!L || !name || !value) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (L->partition_dirty) { int rc = prepare_partition(L); if (rc) return rc; }
    const std::string n(name);
    const int64_t rest = (int64_t)L->h_rest.size() - L->rest_tiny - L->rest_lds - L->rest_ptm;
    if (n == "components_cooperative") *value = (int64_t)L->coop.size();
    else if (n == "components_grid_stream") *value = (int64_t)L->stream.size();
    else if (n == "grid_stream_workgroups") *value = L->stream.empty() ? 0 : L->stream.front().nwg;   // (of the first such component)
    else if (n == "components_tiny") *value = L->rest_tiny;
    else if (n == "components_lds") *value = L->rest_lds;
    else if (n == "components_point_major") *value = L->rest_ptm;
    else if (n == "point_major_wide") *value = L->ptm_wide_last ? 1 : 0;
    else if (n == "point_major_local_cameras") *value = (L->ptm_wide_last && L->ptm_local) ? L->ptm_ncb_cap : 0;
    else if (n == "components_plain") *value = rest;
    else if (n == "pipelined") *value = L->pipelined() ? 1 : 0;
    else if (n == "coop_poll_delay") *value = L->coop_poll_delay;
    else if (n == "coop_poll_inflight") *value = L->coop_poll_inflight;
    else if (n == "coop_poll_stagger") *value = L->coop_poll_stagger;
    else if (n == "point_major_group") *value = L->ptm_last_group;
    else if (n == "point_major_threads") *value = L->ptm_last_threads;
    else if (n == "point_major_round_slots") *value = L->rounds_slots;
    else if (n == "starts_per_launch") *value = L->ms_per_launch;
    else if (n == "starts_launches") *value = L->ms_launches;
    else if (n == "population_tiny_blocks") *value = L->ms_tiny_blocks;
    else if (n == "population_point_major_threads") *value = L->ms_ptm_threads;
    else if (n == "population_cooperative_workgroups") *value = L->ms_coop_wg;
    else if (n == "population_cooperative_cap") *value = L->ms_coop_cap;
    else return fail(c, RDIS_HIP_EINVAL, "plan_get_info: unknown name '" + n + "'");
    return 0;
}

extern "C" int rdis_hip_plan_device_bytes(rdis_hip_plan* L, int64_t* bytes) {
    if (!L || !bytes) return RDIS_HIP_EINVAL;
    USE_DEVICE(L->prob->ctx);
    // (the solvers' tables are built on demand: counted once they exist -- built here if they do not yet; what a first
    // solve adds for its launch shape, e.g. the streaming solver's round tables, shows in a query after that solve)
    if (L->partition_dirty && !L->transient) { int rc = prepare_partition(L); if (rc) return rc; }
    *bytes = (int64_t)(L->dev_bytes + L->trace.bytes + L->vdump.bytes);
    return 0;
}

extern "C" int rdis_hip_plan_get_trace(rdis_hip_plan* L, int64_t comp, double* rec4, int64_t cap, int64_t* nrec) {
    if (!L || !nrec || comp < 0 || comp >= L->ncomp) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (L->trace_records <= 0) { *nrec = 0; return 0; }
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, L->view().trace_n + comp, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *nrec = n;
    const int64_t k = std::min<int64_t>(std::min<int64_t>(n, L->trace_records), cap);
    if (rec4 && k > 0) {
        HIPCHK(c, hipMemcpyAsync(rec4, L->trace.as<double>() + 4ll * L->trace_records * comp, (size_t)k * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int rdis_hip_plan_debug_counters(rdis_hip_plan* L, int64_t* out48) {
    if (!L || !out48) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    HIPCHK(c, hipMemcpyAsync(out48, L->prob->coop_timing.p, ABI_PIPE_TM * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int rdis_hip_plan_get_vectors(rdis_hip_plan* L, int64_t comp, double* out, int64_t cap_doubles) {
    if (!L || !out || comp < 0 || comp >= L->ncomp) return RDIS_HIP_EINVAL;
    rdis_hip_ctx* c = L->prob->ctx;
    USE_DEVICE(c);
    if (L->dump_iters <= 0) return fail(c, RDIS_HIP_EINVAL, "get_vectors: dump_iters is 0");
    const int64_t n = L->h_free_ptr[(size_t)comp + 1] - L->h_free_ptr[(size_t)comp];
    const int64_t want = 2ll * L->dump_iters * n;
    if (cap_doubles < want) return fail(c, RDIS_HIP_EINVAL, "get_vectors: buffer too small");
    if (want == 0) return 0;
    HIPCHK(c, hipMemcpyAsync(out, L->vdump.as<double>() + 2ll * L->dump_iters * L->h_free_ptr[(size_t)comp],
                             (size_t)want * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
