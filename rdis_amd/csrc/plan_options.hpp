// plan_options.hpp -- the options of a plan (rdis_hip_plan_set_option) as data: the fields with their defaults, and one table
// with a row per option -- its name, its member, the rule a value must meet, the message a refused value gets, and whether a
// change makes the plan build its partition again.  plan_option_set() is the whole of what a name and a value do to the
// options; what needs the plan itself (buffers to release or allocate) stays with the caller, told by the effect bits.
// Plain C++: no HIP header, no allocation, no environment; tests/cpp/plan_options_test.cpp runs it without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

namespace rdis_hip {

// the three bounds that are constants of HIP headers, restated (rdis_hip.hip asserts each equal to its original)
constexpr int OPTION_QUAD_MAX_VARS = 4;         // solver_quad.hpp: QUAD_MAX_VARS
constexpr int OPTION_COOP_MAX_WG = 512;         // device_views.hpp: COOP_MAX_WG
constexpr int OPTION_PTM_MAX_GROUP = 512;       // ptm_api.hpp: PTM_WIDE_MAX_GROUP

// (the name of an option is the name of its field, but for "emulate_stale_cache")
struct PlanOptions {
    int block_threads = 0;
    int64_t coop_min_factors = 4096;  // cooperative solver from this many factors ...
    int64_t quad_min_components = 16384;  // the quad solver only for at least this many tiny components
    int64_t coop_group_min_factors = 256;  // ... or for every component of at least this many factors when all their groups fit the device at once
    int tiny_max_blocks = 0;          // (tests): cap on the grid of the tiny-component kernels, 0 = what is resident
    int overlap_batch = 1;            // run the batched launch concurrently with cooperative launches
    int64_t row_min_components = 4096; // sixteen lanes each from this many tiny components (below: a workgroup each)
    int camera_records = 1;           // 0 = every factor forms its rotation itself, 1 = auto, 2 = records wherever possible
    int quad_max_vars = OPTION_QUAD_MAX_VARS; // 0 = never use the quad solver
    int coop_max_components = 48;     // ... for at most this many components per plan (packed two or more to a launch)
    int coop_workgroups = 0, coop_threads = 256;
    int coop_speculate = 1;           // guesses at the following trial steps ride along with every line-search trial
    int coop_pipeline = 1;            // cooperative groups with a control wave of their own (solver_pipe.hpp); 0 = solver_coop.hpp
    int lds_resident = 1;             // 0 = never
    int ptm_stream = 1;               // 0 = never, 1 = components too large for the LDS, 2 = every component
    int ptm_group = 0;                // 0 = auto, 1 = never, k = k workgroups per component
    int ptm_round_slots = 0;          // 0 = two where the LDS holds their staging rows, 1, 2
    int ptm_threads = 0;              // its workgroup size, 0 = auto
    int ptm_local_cameras = -1;       // -1 = where the cameras do not fit, 0 = never, 1 = for every wide component (tests)
    int emulate_stale = 0;            // the reference's factor cache, emulated (solver_lds.hpp; that solver only)
    int factor_rounding = -1;         // -1 = auto (the cooperative solvers round like the reference's build -- it costs them 4 % --, the batch
                                      // solvers use fused multiply-adds), 0 = fused multiply-adds everywhere, 1 = the reference's rounding (and, in the LDS-resident
                                      // solver, its association of a trial's slope) everywhere: refround_api.hpp
    int lds_camera_sums = 1;          // 0 = camera partials through gfac[] like the plain batch solver
    int lds_matrix = 0;               // 1 = line-search trials in matrix form where the cameras' trial records fit the LDS too (solver_lds.hpp);
                                      // measured slower there (a camera's records are a lone lane's chain in front of every trial: 1000 x 2048 factors 16.6 against 10.7 ms)
    int lds_rot = -1;                 // rotation records in that solver, -1 = auto, 0 = per factor, 1 = records
    int lds_threads = 0;              // its workgroup size, 0 = auto
    int force_stream = 0;             // send large components to the streaming grid solver even if they fit the register-resident one
    int coop_poll_delay = 16;
    int coop_poll_inflight = 0;       // the pipelined collector keeps PIPE_POLLS polls of a value+slope slot in flight (solver_pipe.hpp: sweep_ring)
    int coop_poll_stagger = 2;        // ... one issued every so many x64 cycles (off by default: no setting of the scan beat one poll at a time)
    int64_t starts_workspace_bytes = 1ll << 30;   // bounds the replicas of the per-solve workspace a launch of a many-solve entry holds
    int population_point_major = 0;   // 1 = rdis_hip_plan_solve_population takes a plan with components on the point-major streaming solver, a workgroup each (solver_ptm_population.hpp)
    int population_plain = 0;         // 1 = ... a nonlinear-product plan on the plain batch solver (solver_wg_population.hpp)
    int population_tiny = 0;          // 1 = ... a bundle-adjustment plan with components on the tiny-component solver (solver_quad_population.hpp)
    int tiny_population_fill = 1;     // (measurement): the population launch of that solver takes this many times the resident blocks
    int trace_records = 0;
    int dump_iters = 0;
};

// what plan_option_set returns: negative, or the effect bits of the row
constexpr int PLAN_OPTION_UNKNOWN = -2, PLAN_OPTION_REFUSED = -1;
constexpr int PLAN_OPTION_DIRTY = 1;        // a table of the partition depends on it: the partition is built again
constexpr int PLAN_OPTION_ROUNDS = 2;       // the round tables are built for one choice: the caller forgets which they were built for
constexpr int PLAN_OPTION_LOCAL = 4;        // local camera numbering is tried again
constexpr int PLAN_OPTION_WORKSPACE = 8;    // the bound holds from now on: the caller releases the replicas beyond it
constexpr int PLAN_OPTION_TRACE = 16;       // the caller refuses a transient plan and allocates the trace ...
constexpr int PLAN_OPTION_DUMP = 32;        // ... the vector dump (after its bound by the plan's free variables)

struct PlanOptionRow {
    enum Rule { FLAG, RANGE, ONE_OF };
    const char* name;
    int PlanOptions::*i32;            // the member: an int ...
    int64_t PlanOptions::*i64;        // ... or an int64_t
    Rule rule;                        // FLAG: stored as value != 0; RANGE: lo <= value <= hi; ONE_OF: value among allowed[0 .. nallowed)
    int64_t lo, hi;
    const int64_t* allowed;
    int nallowed;
    const char* refusal;              // the message of a value that does not meet the rule
    int effect;                       // PLAN_OPTION_* bits
};

namespace plan_option_rows {
using I32 = int PlanOptions::*;
using I64 = int64_t PlanOptions::*;
constexpr int DIRTY = PLAN_OPTION_DIRTY, CLEAN = 0;   // (CLEAN: no table depends on it)
constexpr int64_t NO_LIMIT = INT64_MAX;
constexpr PlanOptionRow flag(const char* name, I32 m, int effect = DIRTY) {
    return {name, m, nullptr, PlanOptionRow::FLAG, 0, 1, nullptr, 0, nullptr, effect};
}
constexpr PlanOptionRow range(const char* name, I32 m, int64_t lo, int64_t hi, const char* refusal, int effect = DIRTY) {
    return {name, m, nullptr, PlanOptionRow::RANGE, lo, hi, nullptr, 0, refusal, effect};
}
constexpr PlanOptionRow range(const char* name, I64 m, int64_t lo, int64_t hi, const char* refusal, int effect = DIRTY) {
    return {name, nullptr, m, PlanOptionRow::RANGE, lo, hi, nullptr, 0, refusal, effect};
}
template <int N>
constexpr PlanOptionRow one_of(const char* name, I32 m, const int64_t (&allowed)[N], const char* refusal) {
    return {name, m, nullptr, PlanOptionRow::ONE_OF, 0, 0, allowed, N, refusal, DIRTY};
}
inline constexpr int64_t WORKGROUP_SIZES[] = {0, 64, 128, 256, 512, 768, 1024};
inline constexpr int64_t COOP_SIZES[] = {128, 256, 512};
inline constexpr int64_t PTM_SIZES[] = {0, 256, 512, 768};
}  // namespace plan_option_rows

// the table: rows[0 .. *count)
inline const PlanOptionRow* plan_option_table(size_t* count) {
    using namespace plan_option_rows;
    using O = PlanOptions;
    static constexpr PlanOptionRow rows[] = {
        one_of("block_threads", &O::block_threads, WORKGROUP_SIZES, "block_threads must be 0, 64, 128, 256, 512, 768 or 1024"),
        range("coop_min_factors", &O::coop_min_factors, 0, NO_LIMIT, "coop_min_factors < 0"),
        range("quad_min_components", &O::quad_min_components, 0, NO_LIMIT, "quad_min_components < 0"),
        range("coop_group_min_factors", &O::coop_group_min_factors, 0, NO_LIMIT, "coop_group_min_factors < 0"),
        range("tiny_max_blocks", &O::tiny_max_blocks, 0, 1 << 20, "tiny_max_blocks out of range"),
        flag("overlap_batch", &O::overlap_batch),
        range("row_min_components", &O::row_min_components, 0, NO_LIMIT, "row_min_components < 0"),
        range("camera_records", &O::camera_records, 0, 2, "camera_records must be 0, 1 or 2"),
        range("quad_max_vars", &O::quad_max_vars, 0, OPTION_QUAD_MAX_VARS, "quad_max_vars out of range"),
        range("coop_max_components", &O::coop_max_components, 0, 4096, "coop_max_components out of range"),
        range("coop_workgroups", &O::coop_workgroups, 0, OPTION_COOP_MAX_WG, "coop_workgroups out of range"),
        one_of("coop_threads", &O::coop_threads, COOP_SIZES, "coop_threads must be 128, 256 or 512"),
        flag("coop_speculate", &O::coop_speculate),
        flag("coop_pipeline", &O::coop_pipeline),
        flag("lds_resident", &O::lds_resident),
        range("ptm_stream", &O::ptm_stream, 0, 2, "ptm_stream must be 0 (never), 1 (components too large for the LDS) or 2 (every component its tables fit)"),
        range("ptm_group", &O::ptm_group, 0, OPTION_PTM_MAX_GROUP, "ptm_group must be 0 (auto), 1 (never) or the number of workgroups per component (at most 16; up to 512 for the wide groups of a few large components)", CLEAN),
        range("ptm_round_slots", &O::ptm_round_slots, 0, 2, "ptm_round_slots must be 0 (two where the LDS holds them), 1 or 2", CLEAN | PLAN_OPTION_ROUNDS),
        one_of("ptm_threads", &O::ptm_threads, PTM_SIZES, "ptm_threads must be 0, 256, 512 or 768"),
        range("ptm_local_cameras", &O::ptm_local_cameras, -1, 1, "ptm_local_cameras must be -1 (where a wide group's cameras do not fit the LDS), 0 (never) or 1 (every wide group)", DIRTY | PLAN_OPTION_LOCAL),
        flag("emulate_stale_cache", &O::emulate_stale),
        range("factor_rounding", &O::factor_rounding, -1, 1, "factor_rounding must be -1 (auto), 0 (fused multiply-adds) or 1 (the reference's rounding)"),
        flag("lds_camera_sums", &O::lds_camera_sums),
        flag("lds_matrix", &O::lds_matrix, CLEAN),
        range("lds_rot", &O::lds_rot, -1, 1, "lds_rot must be -1, 0 or 1"),
        one_of("lds_threads", &O::lds_threads, WORKGROUP_SIZES, "lds_threads must be 0, 64, 128, 256, 512, 768 or 1024"),
        flag("force_stream", &O::force_stream),
        range("coop_poll_delay", &O::coop_poll_delay, 0, 1024, "coop_poll_delay out of range"),
        range("coop_poll_inflight", &O::coop_poll_inflight, 0, 1, "coop_poll_inflight must be 0 (one poll at a time) or 1 (a ring of polls in flight)"),
        range("coop_poll_stagger", &O::coop_poll_stagger, 0, 64, "coop_poll_stagger out of range (0 ... 64)"),
        range("starts_workspace_bytes", &O::starts_workspace_bytes, 0, NO_LIMIT, "starts_workspace_bytes < 0", CLEAN | PLAN_OPTION_WORKSPACE),
        flag("population_point_major", &O::population_point_major, CLEAN),
        flag("population_plain", &O::population_plain, CLEAN),
        flag("population_tiny", &O::population_tiny, CLEAN),
        range("tiny_population_fill", &O::tiny_population_fill, 1, 64, "tiny_population_fill out of range (1 ... 64)", CLEAN),
        range("trace_records", &O::trace_records, 0, 1 << 22, "trace_records out of range", DIRTY | PLAN_OPTION_TRACE),
        range("dump_iters", &O::dump_iters, 0, 4096, "dump_iters out of range", DIRTY | PLAN_OPTION_DUMP),
    };
    *count = sizeof rows / sizeof rows[0];
    return rows;
}

inline const PlanOptionRow* plan_option_find(const char* name) {
    size_t n = 0;
    const PlanOptionRow* rows = plan_option_table(&n);
    for (size_t i = 0; i < n; ++i)
        if (std::strcmp(rows[i].name, name) == 0) return rows + i;
    return nullptr;
}

// options.name = value, where the option's rule takes the value.  PLAN_OPTION_UNKNOWN: no such option; PLAN_OPTION_REFUSED: the
// value does not meet the rule (either way *message says so and nothing is written); else the row's effect bits.
// *row_out (where wanted): the option's row, null for an unknown name.
inline int plan_option_set(PlanOptions& options, const char* name, int64_t value, std::string* message, const PlanOptionRow** row_out = nullptr) {
    const PlanOptionRow* row = plan_option_find(name);
    if (row_out) *row_out = row;
    if (!row) { *message = "unknown option " + std::string(name); return PLAN_OPTION_UNKNOWN; }
    bool ok = true;
    if (row->rule == PlanOptionRow::RANGE) ok = value >= row->lo && value <= row->hi;
    if (row->rule == PlanOptionRow::ONE_OF) {
        ok = false;
        for (int i = 0; i < row->nallowed; ++i) ok = ok || value == row->allowed[i];
    }
    if (!ok) { *message = row->refusal; return PLAN_OPTION_REFUSED; }
    if (row->rule == PlanOptionRow::FLAG) value = value != 0;
    if (row->i32) options.*(row->i32) = (int)value;
    else options.*(row->i64) = value;
    return row->effect;
}

}  // namespace rdis_hip
