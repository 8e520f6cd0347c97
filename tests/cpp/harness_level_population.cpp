// harness_level_population.cpp -- what tests/test_gpu_level_population.py calls (through ctypes) of the level driver on a
// population (HipRDISLevelOptimizer::optimizePopulation): the single-state driver from a start vector passed in, the population
// run from a [S][N] array of starts, and the states rdis_optba_run_samples draws.  Built by that test's fixture against
// librdis_host.so.
#include <cmath>
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
constexpr int TRACE_COLS = 12;
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
// the driver over either optimiser, with the options both runs share
struct Run {
    std::unique_ptr<HipCGDSubspaceOptimizer> cgd;
    std::unique_ptr<HipLMSubspaceOptimizer> lm;
    std::unique_ptr<HipRDISLevelOptimizer> rdis;
    Run(BundleAdjustmentFunction& f, int use_cgd, int maxit, int max_sweeps, double blkpct, double seppct, int model, int batch) {
        Options o; o.set("SSmaxit", maxit);
        if (use_cgd) {
            cgd.reset(new HipCGDSubspaceOptimizer(f));
            cgd->setParameters(o);
            rdis.reset(new HipRDISLevelOptimizer(f, *cgd));
        } else {
            o.set("LMmodel", model); o.set("LMsingleMinFactors", 0.0);
            lm.reset(new HipLMSubspaceOptimizer(f));
            lm->setParameters(o);
            rdis.reset(new HipRDISLevelOptimizer(f, *lm));
        }
        Options ro; ro.set("AVblkpct", blkpct); ro.set("sepPiecePct", seppct); ro.set("maxSweeps", max_sweeps); ro.set("batch", batch);
        ro.set("lmStepDetail", 0);
        rdis->setParameters(ro);
    }
};
}  // namespace

extern "C" {

// optimize() alone from x_start[N].  out = {final value, initial value, sweeps, launches a sweep, trace steps}; trace rows of 12
// doubles as harness_lm_levels.cpp's; x_out: all variables at the end
int harness_pop_single(const char* path, long long ncams, long long npts, int use_cgd, int maxit, int max_sweeps, double blkpct, double seppct, int model,
                       const double* x_start, double* out, double* trace_out, long long trace_cap, double* x_out) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        const size_t N = f.getVariables().size();
        f.assignAll(NumericVec(x_start, x_start + N));
        const Numeric before = f.eval();
        Run R(f, use_cgd, maxit, max_sweeps, blkpct, seppct, model, 1);
        const Numeric fin = R.rdis->optimize(false);
        out[0] = fin; out[1] = before; out[2] = R.rdis->sweepsDone(); out[3] = (double)R.rdis->numPlans(); out[4] = (double)R.rdis->trace().size();
        put_trace(R.rdis->trace(), trace_out, trace_cap);
        for (size_t i = 0; i < N; ++i) x_out[i] = f.getVariables()[i]->eval();
        return 0;
    } catch (const std::exception& e) { std::cerr << "harness_pop_single: " << e.what() << std::endl; return -2; }
}

// optimizePopulation() on a population made from starts[S][N]; the function itself stands at the file's state.
// mode 0: the run; 1: the population is made on ANOTHER problem (a second load of the same file).
// Returns 0, or 1 when the call threw: msg holds the message.  In both cases rows_out[S][N] are the population's rows afterwards
// and x_problem[N] the device problem's x (x_before[N]: before the call); after a run also: out = {returned value, best member, launches a sweep, permutes},
// member_out[S][9] = {initial, final, sum of deltas, sweeps, calls, iters, fevals, invalid, nonfinite}, trace_n[S] and
// trace_out[S][trace_cap][12], x_mirror[N] the host mirror of the values.
int harness_pop_run(const char* path, long long ncams, long long npts, int use_cgd, int maxit, int max_sweeps, double blkpct, double seppct, int model,
                    int batch, int mode, long long S, const double* starts, double* out, double* member_out, double* trace_out, long long trace_cap,
                    long long* trace_n, double* rows_out, double* x_before, double* x_problem, double* x_mirror, char* msg, long long msg_cap) {
    try {
        BundleAdjustmentFunction f, other;
        PopulationGuard guard;
        rdis_hip_population*& pop = guard.p;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        const size_t N = f.getVariables().size();
        Run R(f, use_cgd, maxit, max_sweeps, blkpct, seppct, model, batch);
        rdis_hip_problem* p = f.deviceProblem();
        rdis_hip_problem* owner = p;
        if (mode == 1) {
            if (!other.load(path, ncams, npts)) return -1;
            other.assignAll(other.getInitialState());
            owner = other.deviceProblem();
        }
        if (rdis_hip_population_create(owner, S, starts, &pop) != 0) return -4;
        if (rdis_hip_get_x(p, (int64_t)N, nullptr, x_before) != 0) return -5;
        int threw = 0;
        try {
            const Numeric fin = R.rdis->optimizePopulation(pop, false);
            out[0] = fin; out[1] = (double)R.rdis->bestMember(); out[2] = (double)R.rdis->numPlans(); out[3] = R.rdis->permutes();
            for (long long s = 0; s < S; ++s) {
                const auto& m = R.rdis->memberResults()[(size_t)s];
                double* r = member_out + 9 * s;
                r[0] = m.initial; r[1] = m.final; r[2] = m.sumOfDeltas; r[3] = m.sweeps; r[4] = (double)m.calls; r[5] = (double)m.iters;
                r[6] = (double)m.fevals; r[7] = (double)m.invalid; r[8] = (double)m.nonfinite;
                const auto& tr = R.rdis->memberTrace((size_t)s);
                trace_n[s] = (long long)tr.size();
                put_trace(tr, trace_out + s * trace_cap * TRACE_COLS, trace_cap);
            }
            for (size_t i = 0; i < N; ++i) x_mirror[i] = f.getVariables()[i]->eval();
        } catch (const std::exception& e) {
            threw = 1;
            if (msg && msg_cap > 0) { std::strncpy(msg, e.what(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        }
        int rc = rdis_hip_population_get_x(pop, 0, S, (int64_t)N, nullptr, rows_out);
        if (!rc) rc = rdis_hip_get_x(p, (int64_t)N, nullptr, x_problem);
        return rc ? -5 : threw;
    } catch (const std::exception& e) {
        std::cerr << "harness_pop_run: " << e.what() << std::endl;
        return -2;
    }
}

// The S states rdis_optba_run_samples(randinit 1) starts from, twice: drawn on the device as that entry draws them
// (dev[S][N]) and from HipRDISLevelOptimizer::restartValue(seed, 0, s, v, dom) on the host (host[S][N])
int harness_pop_drawn_starts(const char* path, long long ncams, long long npts, long long S, unsigned long long seed, double* dev, double* host) {
    try {
        BundleAdjustmentFunction f;
        PopulationGuard guard;
        rdis_hip_population*& pop = guard.p;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        const size_t N = f.getVariables().size();
        std::vector<double> slo(N), shi(N);
        for (size_t v = 0; v < N; ++v) { slo[v] = f.getVariables()[v]->getDomain().samplingMin(); shi[v] = f.getVariables()[v]->getDomain().samplingMax(); }
        int rc = rdis_hip_population_create(f.deviceProblem(), S, nullptr, &pop);
        if (!rc) rc = rdis_hip_population_set_sampling(pop, slo.data(), shi.data());
        if (!rc) rc = rdis_hip_population_sample(pop, 0, S, (int64_t)N, nullptr, seed, 0);
        if (!rc) rc = rdis_hip_population_get_x(pop, 0, S, (int64_t)N, nullptr, dev);
        if (rc) return -5;
        for (long long s = 0; s < S; ++s)
            for (size_t v = 0; v < N; ++v)
                host[(size_t)s * N + v] = HipRDISLevelOptimizer::restartValue(seed, 0, (int)s, (VariableID)v, f.getVariables()[v]->getDomain());
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "harness_pop_drawn_starts: " << e.what() << std::endl;
        return -2;
    }
}

}  // extern "C"
