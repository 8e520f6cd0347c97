/*
 * rdis_optba_samples.h -- the second C entry of the caller side of the path (rdis_amd/lib/librdis_host.so; rdis_optba.h includes
 * this header and describes the options, the out block and the return codes referred to below).  A header of its own because
 * rdis_optba.h's own list of entries is pinned (tests/test_capi_cpu.py); include rdis_optba.h, which brings this one along.
 */
#ifndef RDIS_OPTBA_SAMPLES_H_
#define RDIS_OPTBA_SAMPLES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rdis_optba_run_samples: optBA's sample loop -- the whole optimisation from nsamples initial states, the best kept
 * (optBA.cpp:184-211, 224-297) -- as ONE population run of the level driver (HipRDISLevelOptimizer::optimizePopulation,
 * rdis_levels.h): every member runs schedule 0's sweeps, all members of a step in one launch, a member that has stopped is not
 * solved again.
 *   randinit  1: member s is drawn on the device (rdis_hip_population_sample(seed, stream 0)) from every variable's sampling
 *                interval: its values are HipRDISLevelOptimizer::restartValue(seed, 0, s, v, dom), so a member does not depend on
 *                nsamples (optBA's sampleOffset is not carried over for that reason).  NOT the reference's random numbers.
 *             0: nsamples must be 1 and the member is the file's state (optBA.cpp:189-193).
 *   options   rdis_optba_run's for schedule 0: SSmaxit, SSftol, AVblkpct, steptol, maxSweeps, sepPiecePct, batch (must stay 1),
 *             useCGD, LMmodel; LMsingleMinFactors and lmStepDetail are accepted and ignored (every component goes into its
 *             launch's plan; a component of more than 64 cameras with useCGD 0 is refused: -2); populationCooperative (0 or
 *             1, default 0; with useCGD 1 only it has an effect): 1 lets the run take trees with components on the cooperative
 *             solver -- full ladybug, optBA's default configuration, refused (-2) without it -- a cooperative group per
 *             (member, component) through rdis_hip_plan_solve_population_cooperative; every member's result keeps the bits
 *             of rdis_optba_run from its start.  The options of schedule 1
 *             (nRRperLvl, nRRatTop, minRR, maxNAtoRR, noAssignLimitAtTop, restartSeed, maxCalls) have no meaning here: -3.
 *   out       rdis_optba_run's meaning for the BEST member (lowest final value, lowest index on a tie, never one that is not a
 *             number), except: [1] that member's start value; [2], [3] and [8] summed over all members; [9] the largest sweep
 *             count of a member.
 *   member_out  [nsamples][RDIS_OPTBA_MEMBER_COLS]: [0] start value, [1] final value, [2] sweeps, [3] subspace-optimizer calls,
 *             [4] their iterations, [5] their evaluations (useCGD 0: residual evaluations; else 0), [6] components that ended
 *             with stop code 7, [7] components whose value was not finite (both useCGD 0 only).
 *   x_out     may be NULL; else the best member's final state.
 * Returns 0, -1, -2, -3 as above; nsamples < 1, randinit not 0 or 1, randinit 0 with nsamples != 1: -3. */
#define RDIS_OPTBA_MEMBER_COLS 8
int rdis_optba_run_samples(const char *bal_file, int64_t ncams, int64_t npts, int32_t nopts, const char *const *opt_names,
                           const double *opt_vals, int32_t device, int64_t nsamples, uint64_t seed, int32_t randinit,
                           double *out /*RDIS_OPTBA_NOUT*/, double *member_out /*[nsamples][RDIS_OPTBA_MEMBER_COLS]*/,
                           double *x_out);

#ifdef __cplusplus
}
#endif
#endif /* RDIS_OPTBA_SAMPLES_H_ */
