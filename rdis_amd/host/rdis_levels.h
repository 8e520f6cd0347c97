// rdis_levels.h -- the caller side of the path, re-thought for a batch device: what
// RDISOptimizer's recursion does around ssopt.optimize (reference
// src/RDISOptimizer.cpp:253-334 doOptimization: choose variables, value them with the subspace
// optimizer, assign, decompose, recurse into the children; :971-1117 getValueFromDomain: the
// call itself, made with every other variable of the component held at its current value --
// alternating minimisation), as a LEVEL driver:
//
//   * the decomposition is computed once (the reference's staticDecomp, :1846-1856): a tree of
//     components, each either a LEAF (optimised as a whole: at most AVblkpct of the function's
//     variables, like :342) or split by a SEPARATOR -- a set of variable blocks chosen from the
//     degree structure of the factor graph (chooseSeparator below; stands in for the PaToH call
//     site, :779-865, whose library is binary-only) -- into children: the connected components of
//     what is left (Component::createChildren, src/Component.cpp:508-549), labelled on the device
//     (rdis_hip_components), children ordered as the reference orders them (:603-608);
//   * nodes of equal depth are independent of each other, so each depth becomes at most two
//     persistent device plans (all its separator solves; all its leaves) -- siblings in ONE launch
//     (HipCGDSubspaceOptimizer::optimizeBatch semantics) instead of the reference's serial loop over
//     children (:292-314);
//   * a sweep runs the plans top-down, everything resident on the device; sweeps repeat while the
//     objective improves by more than steptol (the reference's per-node "iterative improvement"
//     steps, :1091-1108), at most maxSweeps times.
//
// Not carried over (they are what makes sibling order observable in the reference, SURVEY.md 7
// hard part 6): branch and bound, the component cache.  With them and the random restarts off the
// reference's own recursion is this alternation (optimize()).  optimizeReferenceSchedule() (round 4) runs the
// tree under the reference's own per-node schedule instead -- iterative improvement node by node and random
// restarts, with restart values drawn per (node, restart, variable) so that siblings stay independent.
#ifndef RDIS_LEVELS_H_
#define RDIS_LEVELS_H_

#include "rdis_host.h"

struct rdis_hip_plan;
struct rdis_hip_population;

namespace rdis {

class HipRDISLevelOptimizer {
public:
    struct Node {
        int depth;
        int parent;                        // index into nodes(), -1 for a top component
        bool leaf;
        std::vector<VariableID> vars;      // ascending (Component.cpp:78-79)
        std::vector<FactorID> factors;     // every factor that reads one of vars, ascending
        std::vector<VariableID> separator; // ascending; empty for a leaf
        std::vector<FactorID> sepFactors;  // the factors that read a separator variable
    };
    struct Step {                          // one launch (or, unbatched, one group of calls)
        int sweep, depth, kind;            // kind 0: separators of this depth, 1: leaves of this depth
        long long ncomp, nvars, nfactors, iters;
        double objective;                  // of the whole function after the step
        double ms;                         // wall time of the step, host side
        // Levenberg-Marquardt steps only (0 otherwise): components solved by a call of their own (lm_routing.h), residual
        // evaluations, components that ended with stop code 7 (invalid values) and components whose value is not finite --
        // the last two are reported here, not thrown (the entries of include/rdis_hip.h return 0 for them)
        long long singles = 0, fevals = 0, invalid = 0, nonfinite = 0;
    };

    HipRDISLevelOptimizer(OptimizableFunction& f, HipCGDSubspaceOptimizer& ssopt);
    // optBA's --useCGD false (src/bundleadjust/optBA.cpp:155-158): every node valued by Levenberg-Marquardt.  The same tree,
    // separators and planLists (the same buildTree).  optimize(): every launch of a sweep is a resident rdis_hip_lm_plan (made
    // with RDIS_HIP_LM_WIDE) of the components lm_routing.h sends to a plan, plus the list of those it sends to a call of their
    // own; a step is the plan's solve from the device's assigned x, the single calls in list order, then
    // rdis_hip_lm_plan_summary -- 128 bytes instead of every component's arrays.  The running objective adds summary [1] and
    // then the singles' deltas in list order; Step::iters is summary [2] plus theirs (Levenberg-Marquardt iterations, no + 1).
    // With the level option lmStepDetail = 0 that is all a step brings back, and the host mirror of the values is brought up to
    // date once, after the last sweep (one rdis_hip_get_x); lmStepDetail = 1 adds a full fetch and mirror after every step (the
    // per-component arrays are filled) and produces the same bits.  1 is the default: on full ladybug the two were measured
    // within the spread between rounds of each other, so the summary-only step has not earned its place as
    // the default.  batch = 0 runs one HipLMSubspaceOptimizer::optimize per component: that is rdis_hip_lm_optimize, a different
    // kernel family from the plans', so -- unlike CGD -- it is NOT promised to equal the batched run bit for bit.
    // optimizeReferenceSchedule() calls HipLMSubspaceOptimizer::optimizeBatch; refIterations() then counts Levenberg-Marquardt
    // iterations and refFEvals() residual evaluations.  One device only (optimize() and optimizeBatch throw otherwise).
    HipRDISLevelOptimizer(OptimizableFunction& f, HipLMSubspaceOptimizer& ssopt);
    ~HipRDISLevelOptimizer();
    HipRDISLevelOptimizer(const HipRDISLevelOptimizer&) = delete;
    HipRDISLevelOptimizer& operator=(const HipRDISLevelOptimizer&) = delete;

    // AVblkpct (0.2), steptol (1e-4), maxSweeps (20), SSmaxit / SSftol (forwarded to the subspace
    // optimizer by the caller), batch (1; 0 = one ssopt.optimize call per component, in the
    // reference's child order: the same results bit for bit, for tests and comparison), sepPiecePct (0: a
    // separator leaves pieces that are leaves; > 0: pieces of up to that fraction of the node, which are
    // split again -- deeper trees, like the reference's two-way partitions), lmStepDetail (1; see the second constructor),
    // populationCooperative (0; 1: optimizePopulation takes CGD trees with components on the cooperative solver, see there)
    void setParameters(const Options& options);

    // Every variable must be assigned (the initial state, optBA.cpp:189-205).  Returns the final
    // value of the function; the variables are left assigned to the optimum found.
    Numeric optimize(bool printInfo = false);

    // optimize() for every member of a population at once: optBA's loop over nsamples initial states (src/bundleadjust/
    // optBA.cpp:184-211, 224-297) as ONE run.  The tree and the per-depth lists are buildTree()'s -- they depend on the structure
    // only --, the plans are made for this run (a later optimize() makes its own): Levenberg-Marquardt plans with
    // RDIS_HIP_LM_WIDE holding EVERY component of their launch (LMsingleMinFactors is ignored here: a call of its own cannot take
    // a member), CGD plans with the plan option population_tiny = 1 and nothing else.  The run: obj[s] =
    // rdis_hip_population_eval over all factors; all S rows active; in every sweep every plan solves rows 0 .. A - 1
    // (rdis_hip_lm_plan_solve_population / rdis_hip_plan_solve_population_range) and each active member's running objective
    // takes the step's delta sum on the host in the single-state step's order (Levenberg-Marquardt: field [1] of the member's row
    // of rdis_hip_lm_plan_summary_population; CGD: plan_fetch_population's deltas in component order, RDIS_HIP_EXIT_EMPTY skipped,
    // iterations counted + 1, RDIS_HIP_EXIT_SYNC_TIMEOUT thrown -- runPlan's loop); after the sweep's last plan every active
    // member is tested with optimize()'s stop rule (level_members.h); where some but not all stopped, the rows are permuted
    // (rdis_hip_population_permute, the stable partition: active rows first) and A shrinks -- not after sweep maxSweeps, which no
    // solve follows --; the loop ends at A == 0 or maxSweeps.
    // Then one permute puts member s back into row s, rdis_hip_population_eval gives every member's final value,
    // rdis_hip_population_assign_best makes the best member the problem's x, the host mirror of the values is brought up to date
    // once, and that member's value is returned.
    // The contract: for every member s, row s afterwards, memberResults()[s] and memberTrace(s) (sweep, depth, kind, ncomp, iters,
    // objective, fevals, invalid, nonfinite) are bit for bit what optimize() leaves and records when it runs alone from that
    // member's start (Levenberg-Marquardt: with LMsingleMinFactors = 0); a member is never solved again once it has stopped; the
    // only rows written are the members'.  Step::ms is the step's wall time, shared by the members of the step.  trace() and
    // sweepsDone() afterwards describe the best member.
    // Throws, before anything is solved or written, with a message that names the cause: batch = 0; several devices; a population
    // of another problem than f.deviceProblem(); Levenberg-Marquardt and a component of more than RDIS_HIP_LM_WIDE_MAX_CAMERAS
    // cameras (the message names the node and its camera count: beyond every plan, and refused rather than routed); a CGD plan the
    // population entry refuses -- cooperative, pipelined or grid components, point-major components in groups -- with that
    // entry's own message (every plan is proved on a scratch population of one member first, so no row has been written).
    // With the level option populationCooperative = 1 the CGD plans of the run also get the plan option coop_pipeline = 0, and
    // their population steps and that proof go through rdis_hip_plan_solve_population_cooperative: cooperative components --
    // full ladybug's 46-camera separator, its camera level as groups side by side -- are solved a group per member, in the
    // plain cooperative layout, whose bits are the pipelined layout's (what optimize() runs): the contract above holds as it
    // stands.  Still refused then: components on the grid solver, point-major components in groups.  Default 0: the run and
    // its refusals as they were.
    struct MemberResult {
        double initial, final, sumOfDeltas;   // f at the start; f evaluated at the end; the running objective (initial + the deltas)
        int sweeps;
        long long calls, iters, fevals, invalid, nonfinite;   // summed over the member's steps as Step counts them (calls: ncomp)
    };
    Numeric optimizePopulation(rdis_hip_population* pop, bool printInfo = false);
    const std::vector<MemberResult>& memberResults() const { return member_results_; }
    const std::vector<Step>& memberTrace(size_t s) const { return member_traces_.at(s); }
    long long bestMember() const { return best_member_; }
    // of the last optimizePopulation: seconds in rdis_hip_population_permute calls (waits included), and how many there were
    double permuteSeconds() const { return permute_s_; }
    int permutes() const { return permutes_; }
    // ... and, of the first sweep's steps, the fewest members a launch held (plan_get_info "starts_per_launch") among the CGD
    // plans that had cooperative launches (populationCooperative: the resident workgroups bound it as well as the budget); where
    // no plan had one, among all CGD plans (the budget alone); 0 without CGD plans.  Later sweeps run fewer members: not read
    long long membersPerLaunch() const { return members_per_launch_; }

    // The same tree under the REFERENCE'S schedule (round 4): what doOptimization / getValueFromDomain do at every node
    // (src/RDISOptimizer.cpp:253-334, 971-1147, 1507-1577) with branch and bound and the component cache off --
    //   * a node is valued again and again: first from its initial values (step type "initial values"), then, with its
    //     children re-optimised in between, from where it stands ("iterative improvement", :1131-1133) for as long as
    //     the subspace optimizer makes progress beyond steptol (:1086-1101); its children run their own such loops to
    //     their end before the node is valued again (the recursion of :292-314);
    //   * when a step makes no progress the node is restarted from a random state (:1088-1094, sampleRandomState
    //     :1196-1216: uniform over each variable's sampling interval), at most numRestarts = max(minRR, nRRperLvl >>
    //     depth) times (nRRatTop at depth 0; :978-983), and after maxNAtoRR assignments without one a restart is forced
    //     below the top (:992-994); the children of a node restarted after NO PROGRESS start from random states too
    //     (:1162-1171), those of a node whose FORCED restart made progress start from the values they had in the
    //     node's previous evaluation (setInitialValFromChildren, :1112-1114, 1713-1724);
    //   * every evaluation of a node is compared with its best so far (updateDomain :1507-1577: a new minimum only beyond
    //     steptol), a node is done when its last evaluation was no new minimum and its restarts are spent (:997-999),
    //     and it is left at its best.
    // What is NOT the reference's: the tree (chooseSeparator in place of PaToH), the random numbers -- a restart's
    // values are drawn per (node, restart, variable) from splitmix64(restartSeed ...), so siblings can be solved in any
    // order or together (the reference draws from one shared mt19937 in visiting order, :1139, 1223-1225) -- and that
    // every variable keeps a value throughout (the reference's alwaysUseAllFactors, :1029-1030, 1165-1182).  Independent
    // nodes run in lock-step: all first evaluations of a set of siblings in one optimizeBatch, all their children
    // together, and so on.  Options: nRRperLvl (2), nRRatTop (nRRperLvl), minRR (1), maxNAtoRR (10),
    // noAssignLimitAtTop (1), restartSeed, maxCalls (100000 subspace-optimizer calls: the reference's time limit, :317-321 --
    // when it is reached every node's loop ends where it stands, at its best).  End-to-end parity with the reference stays unpinned (PaToH, Boost's
    // generator); what is pinned is the schedule: oracle/levels.py restates it from the reference's lines and must take
    // the same decisions, and draw the same restart values, bit for bit, from the values this run's solves returned.
    struct RefStep {
        int node, kind;                    // kind 0: initial values, 1: iterative improvement, 2: random restart
        int nrr, va;                       // the node's restart count and assignments since the last one, after the step
        double fret, delta;                // what the subspace optimizer returned
        double value;                      // the node's value after its children ran (NaN: the step made no progress)
        int newMin;                        // updateDomain's verdict
        unsigned long long startHash;      // FNV-1a over the bits of the start vector
    };
    Numeric optimizeReferenceSchedule(bool printInfo = false);
    const std::vector<RefStep>& refTrace() const { return ref_trace_; }
    // of the last optimizeReferenceSchedule: subspace-optimizer calls (ssopt.optimize, src/RDISOptimizer.cpp:1067), their CG
    // iterations (Frprmn outer iterations) and objective evaluations, and the optimizeBatch launches that carried them
    long long refCalls() const { return ref_calls_; }
    long long refIterations() const { return ref_iters_; }
    long long refFEvals() const { return ref_fevals_; }
    long long refBatches() const { return ref_batches_; }
    static double restartValue(unsigned long long seed, int node, int restart, VariableID vid, const VariableDomain& dom);

    // The decomposition alone -- tree and per-depth plans, nothing solved (what optimize() does first): for callers
    // that want to look at it, and for the parity tests against oracle/levels.py.
    void decompose();
    // the launches of a sweep, in order: plan i solves the separators (kind 0) or the leaves (kind 1) of one depth;
    // its lists are the arguments of rdis_hip_plan_create
    size_t numPlans() const { return plans_.size(); }
    void planLists(size_t i, int& depth, int& kind, std::vector<int64_t>& free_ptr, std::vector<int64_t>& free_vid,
                   std::vector<int64_t>& fac_ptr, std::vector<int64_t>& fac_id) const;

    const std::vector<Node>& nodes() const { return nodes_; }
    const std::vector<Step>& trace() const { return trace_; }
    int sweepsDone() const { return sweeps_; }
    double decompositionMs() const { return decomp_ms_; }

    // The separator of one component: variable blocks (OptimizableFunction::getBlockRangeByVid) are
    // put back into an empty graph in order of ascending degree (number of the component's factors
    // that read the block; ties by block id) for as long as the largest connected piece of what has
    // been put back stays within maxPiece variables; from the first block that does not fit on, blocks are
    // separator blocks.
    // Then, like ensureFactorWillBeAssigned (RDISOptimizer.cpp:412-458), the remaining variables of the
    // first factor (in list order) that reads a separator variable and has the fewest other
    // variables are added, with their blocks.  On ladybug-49-7776 with maxPiece = 0.2 x 23769: 46 of
    // the 49 cameras and one point -- the shape PaToH's cut has in the reference's own run.
    static void chooseSeparator(const OptimizableFunction& f, const std::vector<VariableID>& vars,
                                const std::vector<FactorID>& factors, size_t maxPiece,
                                std::vector<VariableID>& separator);

private:
    struct LevelPlan;
    void buildTree();
    void buildPlans(bool forPopulation = false);
    void releasePlans();
    double runPlan(LevelPlan& lp, int sweep, double objective, bool printInfo);
    OptimizableFunction& f_;
    HipCGDSubspaceOptimizer* cgd_;         // exactly one of the two is set
    HipLMSubspaceOptimizer* lm_;
    SubspaceOptimizer& ss_;
    double runLmPlan(LevelPlan& lp, int sweep, double objective, bool printInfo);
    bool lm_step_detail_ = true;
    bool population_cooperative_ = false;   // level option populationCooperative
    double blkpct_, steptol_, seppct_;
    int maxSweeps_;
    bool batch_;
    size_t ssmaxit_;
    double ssftol_;
    std::vector<Node> nodes_;
    std::vector<LevelPlan*> plans_;
    std::vector<Step> trace_;
    int sweeps_;
    double decomp_ms_;
    // population run
    void stepPopulation(LevelPlan& lp, rdis_hip_population* pop, int sweep, const std::vector<int64_t>& rowToMember, int64_t active,
                        std::vector<double>& objective);
    std::vector<MemberResult> member_results_;
    std::vector<std::vector<Step> > member_traces_;
    long long best_member_ = -1;
    double permute_s_ = 0;
    int permutes_ = 0;
    long long members_per_launch_ = 0;
    // reference schedule
    struct NodeState;
    void runSet(const std::vector<int>& set, const std::vector<char>& randomInit, std::vector<NodeState>& st, bool printInfo);
    unsigned nrr_per_lvl_, nrr_at_top_, min_rr_, max_na_to_rr_;
    bool no_assign_limit_at_top_, nrr_at_top_set_;
    unsigned long long restart_seed_;
    long long ref_iters_ = 0, ref_fevals_ = 0, ref_batches_ = 0;
    long long max_calls_, ref_calls_;   // budget of subspace-optimizer calls (the reference: a time limit, :317-321), calls so far
    std::vector<std::vector<int> > children_;
    std::vector<RefStep> ref_trace_;
};

}  // namespace rdis
#endif  // RDIS_LEVELS_H_
