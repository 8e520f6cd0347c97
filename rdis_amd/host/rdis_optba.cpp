// rdis_optba.cpp -- include/rdis_optba.h: optBA's core over the level driver, as a C entry of librdis_host.so.
#include "../../include/rdis_optba.h"

#include <chrono>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rdis_hip.h"
#include "rdis_levels.h"

using namespace rdis;

extern "C" int rdis_optba_run(const char* bal_file, int64_t ncams, int64_t npts, int32_t schedule, int32_t nopts,
                              const char* const* opt_names, const double* opt_vals, int32_t device, double* out, double* x_out) {
    return rdis_optba_run_hist(bal_file, ncams, npts, schedule, nopts, opt_names, opt_vals, device, out, x_out, nullptr, 0);
}

extern "C" int rdis_optba_run_hist(const char* bal_file, int64_t ncams, int64_t npts, int32_t schedule, int32_t nopts,
                                   const char* const* opt_names, const double* opt_vals, int32_t device, double* out, double* x_out,
                                   double* hist, int32_t hist_rows) {
    if (hist_rows < 0 || (hist_rows > 0 && !hist)) return -3;
    if (!bal_file || !out || (schedule != 0 && schedule != 1) || nopts < 0 || (nopts > 0 && (!opt_names || !opt_vals))) return -3;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    try {
        BundleAdjustmentFunction f;
        if (!f.load(bal_file, ncams, npts)) return -1;
        f.initDevice(device);
        f.assignAll(f.getInitialState());                       // "--randinit 0" (optBA.cpp:189-193)
        Options ss, lv;
        static const char* const level_opts[] = {"AVblkpct", "steptol", "maxSweeps", "sepPiecePct", "nRRperLvl", "nRRatTop", "minRR",
                                                 "maxNAtoRR", "noAssignLimitAtTop", "restartSeed", "maxCalls", "batch", "lmStepDetail"};
        bool use_cgd = true;
        for (int i = 0; i < nopts; ++i) {
            const std::string n(opt_names[i] ? opt_names[i] : "");
            if (n == "SSmaxit" || n == "SSftol") { ss.set(n, opt_vals[i]); continue; }
            // optBA's --useCGD (optBA.cpp:155-158) and the Levenberg-Marquardt optimiser's own options: whole numbers only
            const double ov = opt_vals[i];
            if (n == "useCGD") { if (ov != 0.0 && ov != 1.0) return -3; use_cgd = ov == 1.0; continue; }
            if (n == "LMmodel") { if (ov != 1.0 && ov != 2.0) return -3; ss.set(n, ov); continue; }
            if (n == "LMsingleMinFactors") { if (!(ov >= 0.0) || ov != (double)(long long)ov || ov > 9.0e15) return -3; ss.set(n, ov); continue; }
            bool known = false;
            for (const char* k : level_opts) known = known || n == k;
            if (!known) { std::cerr << "rdis_optba_run: unknown option '" << n << "'" << std::endl; return -3; }
            lv.set(n, opt_vals[i]);
        }
        // (only the optimiser the switch selects is made: the other one's plans, caches and options do not exist)
        std::unique_ptr<HipCGDSubspaceOptimizer> cgd;
        std::unique_ptr<HipLMSubspaceOptimizer> lm;
        std::unique_ptr<HipRDISLevelOptimizer> driver;
        if (use_cgd) {
            cgd.reset(new HipCGDSubspaceOptimizer(f));
            cgd->setParameters(ss);
            driver.reset(new HipRDISLevelOptimizer(f, *cgd));
        } else {
            lm.reset(new HipLMSubspaceOptimizer(f));
            lm->setParameters(ss);
            driver.reset(new HipRDISLevelOptimizer(f, *lm));
        }
        HipRDISLevelOptimizer& rdis = *driver;
        rdis.setParameters(lv);
        const Numeric before = f.eval();
        for (int i = 0; i < RDIS_OPTBA_NOUT; ++i) out[i] = 0.0;
        out[1] = before;
        const double t0 = now();
        if (schedule == 1) {
            out[0] = rdis.optimizeReferenceSchedule(false);
            const double t1 = now();
            out[2] = (double)rdis.refCalls(); out[3] = (double)rdis.refIterations(); out[4] = (double)rdis.refBatches();
            out[6] = rdis.decompositionMs() * 1e-3; out[5] = t1 - t0 - out[6];
            out[8] = (double)rdis.refFEvals(); out[9] = (double)rdis.refTrace().size();
            // where the calls go: per depth of the tree -- nodes, their free variables, and the steps of the reference's schedule
            // by kind (src/RDISOptimizer.cpp:1131-1133), those that made no progress beyond steptol, those that were a new minimum
            for (int r = 0; r < hist_rows; ++r) for (int k = 0; k < RDIS_OPTBA_HIST_COLS; ++k) hist[RDIS_OPTBA_HIST_COLS * r + k] = 0.0;
            for (const auto& nd : rdis.nodes())
                if (nd.depth < hist_rows) {
                    double* h = hist + RDIS_OPTBA_HIST_COLS * nd.depth;
                    h[0] += 1.0; h[1] += (double)(nd.leaf ? nd.vars.size() : nd.separator.size());
                }
            for (const auto& st : rdis.refTrace()) {
                const int d = rdis.nodes()[(size_t)st.node].depth;
                if (d >= hist_rows) continue;
                double* h = hist + RDIS_OPTBA_HIST_COLS * d;
                h[2 + st.kind] += 1.0;
                if (st.value != st.value) h[5] += 1.0;
                if (st.newMin) h[6] += 1.0;
            }
        } else {
            out[0] = rdis.optimize(false);
            const double t1 = now();
            long long calls = 0, iters = 0, fevals = 0;
            for (const auto& st : rdis.trace()) { calls += st.ncomp; iters += st.iters; fevals += st.fevals; }
            out[2] = (double)calls; out[3] = (double)iters; out[4] = (double)rdis.trace().size();
            if (!use_cgd) out[8] = (double)fevals;
            out[6] = rdis.decompositionMs() * 1e-3; out[5] = t1 - t0 - out[6];
            out[9] = rdis.sweepsDone();
        }
        out[7] = (double)rdis.nodes().size();
        if (x_out) for (size_t i = 0; i < f.getVariables().size(); ++i) x_out[i] = f.getVariables()[i]->eval();
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "rdis_optba_run: " << e.what() << std::endl;
        return -2;
    }
}

// optBA's sample loop (optBA.cpp:184-211, 224-297) as one population run of the level driver
extern "C" int rdis_optba_run_samples(const char* bal_file, int64_t ncams, int64_t npts, int32_t nopts, const char* const* opt_names,
                                      const double* opt_vals, int32_t device, int64_t nsamples, uint64_t seed, int32_t randinit, double* out,
                                      double* member_out, double* x_out) {
    if (!bal_file || !out || !member_out || nopts < 0 || (nopts > 0 && (!opt_names || !opt_vals))) return -3;
    if (nsamples < 1 || (randinit != 0 && randinit != 1) || (randinit == 0 && nsamples != 1)) return -3;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    try {
        BundleAdjustmentFunction f;
        if (!f.load(bal_file, ncams, npts)) return -1;
        // (declared after f: destroyed before it on every way out, a throw included -- the population dies before its problem)
        struct PopulationGuard {
            rdis_hip_population* p = nullptr;
            ~PopulationGuard() { if (p) rdis_hip_population_destroy(p); }
        } guard;
        rdis_hip_population*& pop = guard.p;
        f.initDevice(device);
        f.assignAll(f.getInitialState());
        Options ss, lv;
        // (schedule 0 only: the options of the reference's per-node schedule have no meaning here)
        static const char* const level_opts[] = {"AVblkpct", "steptol", "maxSweeps", "sepPiecePct", "batch", "populationCooperative"};
        bool use_cgd = true;
        for (int i = 0; i < nopts; ++i) {
            const std::string n(opt_names[i] ? opt_names[i] : "");
            if (n == "SSmaxit" || n == "SSftol") { ss.set(n, opt_vals[i]); continue; }
            const double ov = opt_vals[i];
            if (n == "useCGD") { if (ov != 0.0 && ov != 1.0) return -3; use_cgd = ov == 1.0; continue; }
            if (n == "LMmodel") { if (ov != 1.0 && ov != 2.0) return -3; ss.set(n, ov); continue; }
            if (n == "LMsingleMinFactors") { if (!(ov >= 0.0) || ov != (double)(long long)ov || ov > 9.0e15) return -3; continue; }   // accepted, ignored
            if (n == "lmStepDetail") continue;                                                                                        // accepted, ignored
            bool known = false;
            for (const char* k : level_opts) known = known || n == k;
            if (!known) { std::cerr << "rdis_optba_run_samples: option '" << n << "' is unknown or has no meaning in a population run" << std::endl; return -3; }
            lv.set(n, opt_vals[i]);
        }
        std::unique_ptr<HipCGDSubspaceOptimizer> cgd;
        std::unique_ptr<HipLMSubspaceOptimizer> lm;
        std::unique_ptr<HipRDISLevelOptimizer> driver;
        if (use_cgd) {
            cgd.reset(new HipCGDSubspaceOptimizer(f));
            cgd->setParameters(ss);
            driver.reset(new HipRDISLevelOptimizer(f, *cgd));
        } else {
            lm.reset(new HipLMSubspaceOptimizer(f));
            lm->setParameters(ss);
            driver.reset(new HipRDISLevelOptimizer(f, *lm));
        }
        HipRDISLevelOptimizer& rdis = *driver;
        rdis.setParameters(lv);
        rdis_hip_problem* p = f.deviceProblem();
        rdis_hip_ctx* ctx = f.deviceContext();
        auto chk = [&](int rc, const char* where) { if (rc != 0) throw HipError(rc, std::string(where) + ": " + rdis_hip_last_error(ctx)); };
        const size_t N = f.getVariables().size();
        chk(rdis_hip_population_create(p, nsamples, nullptr, &pop), "rdis_hip_population_create");   // every member the file's state ("--randinit 0")
        if (randinit) {
            // sampleRandomState's intervals (RDISOptimizer.cpp:1196-1216); member s, variable v: restartValue(seed, 0, s, v, dom)
            std::vector<double> slo(N), shi(N);
            for (size_t v = 0; v < N; ++v) { slo[v] = f.getVariables()[v]->getDomain().samplingMin(); shi[v] = f.getVariables()[v]->getDomain().samplingMax(); }
            chk(rdis_hip_population_set_sampling(pop, slo.data(), shi.data()), "rdis_hip_population_set_sampling");
            chk(rdis_hip_population_sample(pop, 0, nsamples, (int64_t)N, nullptr, seed, 0), "rdis_hip_population_sample");
        }
        for (int i = 0; i < RDIS_OPTBA_NOUT; ++i) out[i] = 0.0;
        const double t0 = now();
        out[0] = rdis.optimizePopulation(pop, false);
        const double t1 = now();
        const auto& res = rdis.memberResults();
        const size_t best = (size_t)rdis.bestMember();
        long long calls = 0, iters = 0, fevals = 0;
        int sweeps = 0;
        for (size_t s = 0; s < res.size(); ++s) {
            const auto& m = res[s];
            double* r = member_out + RDIS_OPTBA_MEMBER_COLS * s;
            r[0] = m.initial; r[1] = m.final; r[2] = m.sweeps; r[3] = (double)m.calls; r[4] = (double)m.iters; r[5] = (double)m.fevals;
            r[6] = (double)m.invalid; r[7] = (double)m.nonfinite;
            calls += m.calls; iters += m.iters; fevals += m.fevals;
            if (m.sweeps > sweeps) sweeps = m.sweeps;
        }
        out[1] = res[best].initial;
        out[2] = (double)calls; out[3] = (double)iters; out[4] = (double)rdis.memberTrace(best).size();
        if (!use_cgd) out[8] = (double)fevals;
        out[6] = rdis.decompositionMs() * 1e-3; out[5] = t1 - t0 - out[6];
        out[7] = (double)rdis.nodes().size();
        out[9] = sweeps;
        if (x_out) for (size_t i = 0; i < N; ++i) x_out[i] = f.getVariables()[i]->eval();
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "rdis_optba_run_samples: " << e.what() << std::endl;
        return -2;
    }
}
