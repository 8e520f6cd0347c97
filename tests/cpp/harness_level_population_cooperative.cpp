// harness_level_population_cooperative.cpp -- what tests/test_gpu_level_population_cooperative.py calls (through ctypes) of the
// level driver on a population with the level option populationCooperative: the single-state CGD driver from a start vector
// passed in, and the population run from a [S][N] array of starts with the option on or off.  The whole file is loaded (the
// tree of full ladybug has components on the cooperative solver).  Built by that test's fixture against librdis_host.so, the
// way tests/test_gpu_level_population.py builds harness_level_population.cpp.
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include "../../include/rdis_hip.h"
#include "../../rdis_amd/host/rdis_host.h"
#include "../../rdis_amd/host/rdis_levels.h"

using namespace rdis;

namespace {
// declared after the function whose problem the population belongs to: destroyed before it on every way out, a throw included
struct PopulationGuard {
    rdis_hip_population* p = nullptr;
    ~PopulationGuard() { if (p) rdis_hip_population_destroy(p); }
};
constexpr int TRACE_COLS = 12;   // (harness_level_population.cpp's rows)
void put_trace(const std::vector<HipRDISLevelOptimizer::Step>& tr, double* trace_out, long long trace_cap) {
    if (!trace_out) return;
    for (size_t i = 0; i < tr.size() && (long long)i < trace_cap; ++i) {
        const auto& st = tr[i];
        double* r = trace_out + TRACE_COLS * i;
        r[0] = st.sweep; r[1] = st.depth; r[2] = st.kind; r[3] = (double)st.ncomp; r[4] = (double)st.nvars; r[5] = (double)st.nfactors;
        r[6] = (double)st.iters; r[7] = st.objective; r[8] = (double)st.singles; r[9] = (double)st.fevals; r[10] = (double)st.invalid;
        r[11] = (double)st.nonfinite;
    }
}
// the CGD driver with the options both runs share (the level driver's defaults otherwise)
struct Run {
    HipCGDSubspaceOptimizer cgd;
    HipRDISLevelOptimizer rdis;
    Run(BundleAdjustmentFunction& f, int maxit, int max_sweeps, int cooperative) : cgd(f), rdis(f, cgd) {
        Options o; o.set("SSmaxit", maxit);
        cgd.setParameters(o);
        Options ro; ro.set("maxSweeps", max_sweeps); ro.set("populationCooperative", cooperative);
        rdis.setParameters(ro);
    }
};
}  // namespace

extern "C" {

// optimize() alone from x_start[N].  out = {final value, initial value, sweeps, launches a sweep, trace steps}; x_out: all
// variables at the end
int harness_coop_single(const char* path, int maxit, int max_sweeps, const double* x_start, double* out, double* trace_out, long long trace_cap,
                        double* x_out) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, 0, 0)) return -1;
        const size_t N = f.getVariables().size();
        f.assignAll(NumericVec(x_start, x_start + N));
        const Numeric before = f.eval();
        Run R(f, maxit, max_sweeps, 0);
        const Numeric fin = R.rdis.optimize(false);
        out[0] = fin; out[1] = before; out[2] = R.rdis.sweepsDone(); out[3] = (double)R.rdis.numPlans(); out[4] = (double)R.rdis.trace().size();
        put_trace(R.rdis.trace(), trace_out, trace_cap);
        for (size_t i = 0; i < N; ++i) x_out[i] = f.getVariables()[i]->eval();
        return 0;
    } catch (const std::exception& e) { std::cerr << "harness_coop_single: " << e.what() << std::endl; return -2; }
}

// optimizePopulation() on a population made from starts[S][N], populationCooperative = cooperative.  Returns 0, or 1 when the
// call threw: msg holds the message.  In both cases rows_out[S][N] are the population's rows afterwards and x_problem[N] the device
// problem's x (x_before[N]: before the call); after a run also out = {returned value, best member, launches a sweep, permutes},
// member_out[S][4] = {initial, final, sum of deltas, sweeps}, trace_n[S] and trace_out[S][trace_cap][12].
int harness_coop_run(const char* path, int maxit, int max_sweeps, int cooperative, long long S, const double* starts, double* out, double* member_out,
                     double* trace_out, long long trace_cap, long long* trace_n, double* rows_out, double* x_before, double* x_problem, char* msg,
                     long long msg_cap) {
    try {
        BundleAdjustmentFunction f;
        PopulationGuard guard;
        rdis_hip_population*& pop = guard.p;
        if (!f.load(path, 0, 0)) return -1;
        f.assignAll(f.getInitialState());
        const size_t N = f.getVariables().size();
        Run R(f, maxit, max_sweeps, cooperative);
        rdis_hip_problem* p = f.deviceProblem();
        if (rdis_hip_population_create(p, S, starts, &pop) != 0) return -4;
        if (rdis_hip_get_x(p, (int64_t)N, nullptr, x_before) != 0) return -5;
        int threw = 0;
        try {
            const Numeric fin = R.rdis.optimizePopulation(pop, false);
            out[0] = fin; out[1] = (double)R.rdis.bestMember(); out[2] = (double)R.rdis.numPlans(); out[3] = R.rdis.permutes();
            for (long long s = 0; s < S; ++s) {
                const auto& m = R.rdis.memberResults()[(size_t)s];
                double* r = member_out + 4 * s;
                r[0] = m.initial; r[1] = m.final; r[2] = m.sumOfDeltas; r[3] = m.sweeps;
                const auto& tr = R.rdis.memberTrace((size_t)s);
                trace_n[s] = (long long)tr.size();
                put_trace(tr, trace_out + s * trace_cap * TRACE_COLS, trace_cap);
            }
        } catch (const std::exception& e) {
            threw = 1;
            if (msg && msg_cap > 0) { std::strncpy(msg, e.what(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        }
        int rc = rdis_hip_population_get_x(pop, 0, S, (int64_t)N, nullptr, rows_out);
        if (!rc) rc = rdis_hip_get_x(p, (int64_t)N, nullptr, x_problem);
        return rc ? -5 : threw;
    } catch (const std::exception& e) {
        std::cerr << "harness_coop_run: " << e.what() << std::endl;
        return -2;
    }
}

}  // extern "C"
