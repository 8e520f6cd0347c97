// harness_lm_levels.cpp -- what tests/test_gpu_lm_levels.py calls (through ctypes) of the level driver over
// HipLMSubspaceOptimizer (optBA's useCGD = false): the driver's sweeps, the lists of its launches, optimizeBatch on its own, the
// reference schedule.  Built by that test's fixture against librdis_host.so; harness.cpp is the CGD side and is left alone.
#include <cmath>
#include <cstring>
#include <iostream>
#include <memory>

#include "../../rdis_amd/host/rdis_host.h"
#include "../../rdis_amd/host/rdis_levels.h"

using namespace rdis;

namespace {
constexpr int TRACE_COLS = 12;
void put_trace(const HipRDISLevelOptimizer& rdis, double* trace_out, long long trace_cap) {
    if (!trace_out) return;
    for (size_t i = 0; i < rdis.trace().size() && (long long)i < trace_cap; ++i) {
        const auto& st = rdis.trace()[i];
        double* r = trace_out + TRACE_COLS * i;
        r[0] = st.sweep; r[1] = st.depth; r[2] = st.kind; r[3] = (double)st.ncomp; r[4] = (double)st.nvars; r[5] = (double)st.nfactors;
        r[6] = (double)st.iters; r[7] = st.objective; r[8] = (double)st.singles; r[9] = (double)st.fevals; r[10] = (double)st.invalid;
        r[11] = (double)st.nonfinite;
    }
}
}  // namespace

extern "C" {

// The level driver's sweeps (schedule 0) with Levenberg-Marquardt from the file's state.
// out = {final value (f.eval() at the end), initial value, sweeps, launches a sweep, trace steps};
// trace rows of 12 doubles: sweep, depth, kind, ncomp, nvars, nfactors, iters, objective, singles, residual evaluations,
// components with stop code 7, components with a value that is not finite; x_out: all variables at the end
int harness_lm_level_driver(const char* path, long long ncams, long long npts, int maxit, int max_sweeps, double blkpct, double seppct,
                            int model, int batch, int detail, double single_min_factors, double* out, double* trace_out, long long trace_cap,
                            double* x_out) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        const Numeric before = f.eval();
        HipLMSubspaceOptimizer lm(f);
        Options o; o.set("SSmaxit", maxit); o.set("LMmodel", model); o.set("LMsingleMinFactors", single_min_factors);
        lm.setParameters(o);
        HipRDISLevelOptimizer rdis(f, lm);
        Options ro; ro.set("AVblkpct", blkpct); ro.set("sepPiecePct", seppct); ro.set("maxSweeps", max_sweeps); ro.set("batch", batch);
        ro.set("lmStepDetail", detail);
        rdis.setParameters(ro);
        const Numeric fin = rdis.optimize(false);
        out[0] = fin; out[1] = before; out[2] = rdis.sweepsDone(); out[3] = (double)rdis.numPlans(); out[4] = (double)rdis.trace().size();
        put_trace(rdis, trace_out, trace_cap);
        if (x_out) for (size_t i = 0; i < f.getVariables().size(); ++i) x_out[i] = f.getVariables()[i]->eval();
        return 0;
    } catch (const std::exception& e) { std::cerr << "harness_lm_level_driver: " << e.what() << std::endl; return -2; }
}

// The lists of the driver's launches (planLists), nothing solved.  out (capacity cap int64): #plans, per plan {depth, kind,
// #components, free_ptr.. (ncomp + 1), #free, free_vid.., fac_ptr.. (ncomp + 1), #fac, fac_id..}.  Returns the entries written.
long long harness_lm_plan_lists(const char* path, long long ncams, long long npts, double blkpct, double seppct, long long* out, long long cap) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        HipLMSubspaceOptimizer lm(f);
        HipRDISLevelOptimizer rdis(f, lm);
        Options ro; ro.set("AVblkpct", blkpct); ro.set("sepPiecePct", seppct);
        rdis.setParameters(ro);
        rdis.decompose();
        long long n = 0;
        auto put = [&](long long v) { if (n < cap) out[n] = v; ++n; };
        put((long long)rdis.numPlans());
        for (size_t i = 0; i < rdis.numPlans(); ++i) {
            int depth, kind;
            std::vector<int64_t> fp, fv, cp, ci;
            rdis.planLists(i, depth, kind, fp, fv, cp, ci);
            put(depth); put(kind); put((long long)fp.size() - 1);
            for (auto v : fp) put(v);
            put((long long)fv.size());
            for (auto v : fv) put(v);
            for (auto v : cp) put(v);
            put((long long)ci.size());
            for (auto v : ci) put(v);
        }
        return n <= cap ? n : -3;
    } catch (const std::exception& e) { std::cerr << "harness_lm_plan_lists: " << e.what() << std::endl; return -2; }
}

// HipLMSubspaceOptimizer::optimizeBatch on its own: every launch of the level tree (its separators, then its leaves, ...) as one
// call, from the file's state, `rounds` times over.  Per component of every call, in call order: res rows of 6 doubles {fret,
// deltaFval, iters, status, residual evaluations, Jacobian evaluations} and its xval after the call in x_out (concatenated).
// out = {calls made, components in all, cache hits, cache misses, cache entries, singles of the last call, sum of the returned values}
int harness_lm_optimize_batch(const char* path, long long ncams, long long npts, int maxit, int model, int cache, int rounds, double* out,
                              double* res, long long res_cap, double* x_out, long long x_cap) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        HipLMSubspaceOptimizer lm(f);
        Options o; o.set("SSmaxit", maxit); o.set("LMmodel", model);
        lm.setParameters(o);
        lm.setPlanCache((size_t)cache);
        HipRDISLevelOptimizer rdis(f, lm);
        rdis.decompose();
        const VariablePtrVec& vars = f.getVariables();
        const FactorPtrVec& facs = f.getFactors();
        long long calls = 0, ncomp = 0, nx = 0;
        double total = 0.0;
        for (int r = 0; r < rounds; ++r)
            for (size_t i = 0; i < rdis.numPlans(); ++i) {
                int depth, kind;
                std::vector<int64_t> fp, fv, cp, ci;
                rdis.planLists(i, depth, kind, fp, fv, cp, ci);
                std::vector<HipLMSubspaceOptimizer::Component> comps(fp.size() - 1);
                for (size_t c = 0; c + 1 < fp.size(); ++c) {
                    for (int64_t k = fp[c]; k < fp[c + 1]; ++k) { comps[c].vars.push_back(vars[(size_t)fv[(size_t)k]]); comps[c].xval.push_back(vars[(size_t)fv[(size_t)k]]->eval()); }
                    for (int64_t k = cp[c]; k < cp[c + 1]; ++k) comps[c].factors.push_back(facs[(size_t)ci[(size_t)k]]);
                }
                total += lm.optimizeBatch(comps, false);
                ++calls;
                for (const auto& C : comps) {
                    if (ncomp >= res_cap || nx + (long long)C.xval.size() > x_cap) return -3;
                    double* row = res + 6 * ncomp++;
                    row[0] = C.fret; row[1] = C.deltaFval; row[2] = C.iters; row[3] = C.status; row[4] = (double)C.nfeval; row[5] = (double)C.ngeval;
                    for (double v : C.xval) x_out[nx++] = v;
                    for (size_t k = 0; k < C.vars.size(); ++k) if (C.vars[k]->eval() != C.xval[k]) return -4;   // the variables are left assigned
                }
            }
        out[0] = (double)calls; out[1] = (double)ncomp; out[2] = (double)lm.planCacheHits(); out[3] = (double)lm.planCacheMisses();
        out[4] = (double)lm.planCacheEntries(); out[5] = (double)lm.lastBatchSingles(); out[6] = total;
        return 0;
    } catch (const std::exception& e) { std::cerr << "harness_lm_optimize_batch: " << e.what() << std::endl; return -2; }
}

// The reference's schedule over Levenberg-Marquardt: harness.cpp's harness_level_reference with the other optimiser.
// out = {final value, value before, nodes, steps, LM iterations, residual evaluations, optimizeBatch calls}; trace rows of 10 doubles:
// node, kind, nrr, va, fret, delta, value, newMin, start hash (high 32 bits, low 32 bits).  Returns the number of steps.
long long harness_lm_level_reference(const char* path, long long ncams, long long npts, int maxit, int model, double blkpct, double seppct, int nrr_per_lvl,
                                     int max_na_to_rr, double seed, double max_calls, double steptol, double* out, double* trace_out, long long trace_cap,
                                     double* x_out) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        f.assignAll(f.getInitialState());
        const Numeric before = f.eval();
        HipLMSubspaceOptimizer lm(f);
        Options o; o.set("SSmaxit", maxit); o.set("LMmodel", model);
        lm.setParameters(o);
        HipRDISLevelOptimizer rdis(f, lm);
        Options ro; ro.set("AVblkpct", blkpct); ro.set("sepPiecePct", seppct); ro.set("nRRperLvl", nrr_per_lvl);
        ro.set("maxNAtoRR", max_na_to_rr); ro.set("restartSeed", seed); ro.set("maxCalls", max_calls); ro.set("steptol", steptol);
        rdis.setParameters(ro);
        const Numeric fin = rdis.optimizeReferenceSchedule(false);
        const auto& tr = rdis.refTrace();
        out[0] = fin; out[1] = before; out[2] = (double)rdis.nodes().size(); out[3] = (double)tr.size();
        out[4] = (double)rdis.refIterations(); out[5] = (double)rdis.refFEvals(); out[6] = (double)rdis.refBatches();
        for (size_t i = 0; i < tr.size() && (long long)i < trace_cap; ++i) {
            double* r = trace_out + 10 * i;
            r[0] = tr[i].node; r[1] = tr[i].kind; r[2] = tr[i].nrr; r[3] = tr[i].va; r[4] = tr[i].fret; r[5] = tr[i].delta;
            r[6] = tr[i].value; r[7] = tr[i].newMin; r[8] = (double)(tr[i].startHash >> 32); r[9] = (double)(tr[i].startHash & 0xFFFFFFFFull);
        }
        if (x_out) for (size_t i = 0; i < f.getVariables().size(); ++i) x_out[i] = f.getVariables()[i]->eval();
        return (long long)tr.size();
    } catch (const std::exception& e) { std::cerr << "harness_lm_level_reference: " << e.what() << std::endl; return -2; }
}

// Two devices listed: optimizeBatch must refuse, with a message that says why.  Returns 1 when it threw such a message.
int harness_lm_refuses_several_devices(const char* path) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, 5, 30)) return -1;
        f.setDevices(std::vector<int>(2, 0));
        f.assignAll(f.getInitialState());
        HipLMSubspaceOptimizer lm(f);
        std::vector<HipLMSubspaceOptimizer::Component> comps(1);
        for (int k = 0; k < 3; ++k) { Variable* v = f.getVariables()[(size_t)(45 + k)]; comps[0].vars.push_back(v); comps[0].xval.push_back(v->eval()); }
        comps[0].factors = f.getVariables()[45]->getFactors();
        try { lm.optimizeBatch(comps, false); } catch (const std::logic_error& e) { return std::strstr(e.what(), "one device only") ? 1 : 0; }
        return 0;
    } catch (const std::exception& e) { std::cerr << "harness_lm_refuses_several_devices: " << e.what() << std::endl; return -2; }
}

}  // extern "C"
