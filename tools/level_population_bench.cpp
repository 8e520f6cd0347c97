// level_population_bench.cpp -- the C++ side of tools/bench_level_population.py (compiled by that tool against librdis_host.so):
// HipRDISLevelOptimizer::optimizePopulation on S drawn members against a loop over the members of assignAll + optimize() on the
// same driver object.  Both from the same starts; rounds alternate between the two; the decomposition (buildTree) is taken out
// of both timings, the plans each run makes are inside (a population run makes them once, optimize() once per member).
#include <chrono>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "../include/rdis_hip.h"
#include "../rdis_amd/host/rdis_host.h"
#include "../rdis_amd/host/rdis_levels.h"

using namespace rdis;

namespace {
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}

// loop_s, pop_s, permute_s: [rounds] seconds; info = {members whose final value differs between the two (bits), best value of the
// loop, best value of the population run, sum of the members' sweeps, largest sweep count, permutes of a run, launches a sweep,
// members with a final value that is not finite, the fewest members a launch of a CGD plan held}.  cooperative: the level option
// populationCooperative of the population run (the loop is optimize() as it is).  Returns 0; 1: the population run was refused
// (msg says why); < 0: an error.
extern "C" int bench_level_population_option(const char* path, long long ncams, long long npts, int use_cgd, int maxit, int max_sweeps, int model,
                                             long long S, unsigned long long seed, int rounds, int cooperative, double* loop_s, double* pop_s,
                                             double* permute_s, double* info, char* msg, long long msg_cap) {
    try {
        BundleAdjustmentFunction f;
        if (!f.load(path, ncams, npts)) return -1;
        struct PopulationGuard {   // (after f: the population is destroyed before its problem on every way out)
            rdis_hip_population* p = nullptr;
            ~PopulationGuard() { if (p) rdis_hip_population_destroy(p); }
        } guard;
        rdis_hip_population*& pop = guard.p;
        f.initDevice(0);
        f.assignAll(f.getInitialState());
        const size_t N = f.getVariables().size();
        Options o; o.set("SSmaxit", maxit);
        std::unique_ptr<HipCGDSubspaceOptimizer> cgd;
        std::unique_ptr<HipLMSubspaceOptimizer> lm;
        std::unique_ptr<HipRDISLevelOptimizer> driver;
        if (use_cgd) {
            cgd.reset(new HipCGDSubspaceOptimizer(f)); cgd->setParameters(o);
            driver.reset(new HipRDISLevelOptimizer(f, *cgd));
        } else {
            o.set("LMmodel", model); o.set("LMsingleMinFactors", 0.0);   // (every component in its launch's plan: the population run's computation)
            lm.reset(new HipLMSubspaceOptimizer(f)); lm->setParameters(o);
            driver.reset(new HipRDISLevelOptimizer(f, *lm));
        }
        Options ro; ro.set("maxSweeps", max_sweeps); ro.set("lmStepDetail", 0); ro.set("populationCooperative", cooperative);
        driver->setParameters(ro);
        rdis_hip_problem* p = f.deviceProblem();
        rdis_hip_ctx* ctx = f.deviceContext();
        auto chk = [&](int rc, const char* where) { if (rc != 0) throw HipError(rc, std::string(where) + ": " + rdis_hip_last_error(ctx)); };
        // the members rdis_optba_run_samples would draw
        std::vector<double> slo(N), shi(N), starts((size_t)S * N);
        for (size_t v = 0; v < N; ++v) { slo[v] = f.getVariables()[v]->getDomain().samplingMin(); shi[v] = f.getVariables()[v]->getDomain().samplingMax(); }
        chk(rdis_hip_population_create(p, S, nullptr, &pop), "rdis_hip_population_create");
        chk(rdis_hip_population_set_sampling(pop, slo.data(), shi.data()), "rdis_hip_population_set_sampling");
        chk(rdis_hip_population_sample(pop, 0, S, (int64_t)N, nullptr, seed, 0), "rdis_hip_population_sample");
        chk(rdis_hip_population_get_x(pop, 0, S, (int64_t)N, nullptr, starts.data()), "rdis_hip_population_get_x");
        std::vector<double> fin_loop((size_t)S), fin_pop((size_t)S);
        for (int r = -1; r < rounds; ++r) {   // (round -1: the warm-up of both)
            double t = 0;
            for (long long s = 0; s < S; ++s) {
                const double t0 = now_s();
                f.assignAll(NumericVec(starts.begin() + (long)((size_t)s * N), starts.begin() + (long)((size_t)(s + 1) * N)));
                fin_loop[(size_t)s] = driver->optimize(false);
                t += now_s() - t0 - driver->decompositionMs() * 1e-3;
            }
            if (r >= 0) loop_s[r] = t;
            chk(rdis_hip_population_set_x(pop, 0, S, (int64_t)N, nullptr, starts.data()), "rdis_hip_population_set_x");
            chk(rdis_hip_synchronize(ctx), "rdis_hip_synchronize");
            const double t0 = now_s();
            try {
                driver->optimizePopulation(pop, false);
            } catch (const HipError& e) {
                if (msg && msg_cap > 0) { std::strncpy(msg, e.what(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
                return 1;
            }
            const double tp = now_s() - t0 - driver->decompositionMs() * 1e-3;
            if (r >= 0) { pop_s[r] = tp; permute_s[r] = driver->permuteSeconds(); }
        }
        const auto& res = driver->memberResults();
        long long differ = 0, sweeps = 0, most = 0, bad = 0;
        double best_loop = 0, best_pop = 0;
        bool have = false;
        for (long long s = 0; s < S; ++s) {
            fin_pop[(size_t)s] = res[(size_t)s].final;
            if (std::memcmp(&fin_pop[(size_t)s], &fin_loop[(size_t)s], sizeof(double)) != 0) ++differ;
            sweeps += res[(size_t)s].sweeps;
            if (res[(size_t)s].sweeps > most) most = res[(size_t)s].sweeps;
            const double a = fin_loop[(size_t)s];
            if (!(a - a == 0.0)) { ++bad; continue; }
            if (!have || a < best_loop) { best_loop = a; have = true; }
        }
        best_pop = res[(size_t)driver->bestMember()].final;
        info[0] = (double)differ; info[1] = best_loop; info[2] = best_pop; info[3] = (double)sweeps; info[4] = (double)most;
        info[5] = driver->permutes(); info[6] = (double)driver->numPlans(); info[7] = (double)bad; info[8] = (double)driver->membersPerLaunch();
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "bench_level_population: " << e.what() << std::endl;
        return -2;
    }
}

// (info: eight doubles, as before the option existed)
extern "C" int bench_level_population(const char* path, long long ncams, long long npts, int use_cgd, int maxit, int max_sweeps, int model, long long S,
                                      unsigned long long seed, int rounds, double* loop_s, double* pop_s, double* permute_s, double* info, char* msg,
                                      long long msg_cap) {
    double all[9] = {0};
    const int rc = bench_level_population_option(path, ncams, npts, use_cgd, maxit, max_sweeps, model, S, seed, rounds, 0, loop_s, pop_s, permute_s, all, msg,
                                                 msg_cap);
    for (int i = 0; i < 8; ++i) info[i] = all[i];
    return rc;
}
