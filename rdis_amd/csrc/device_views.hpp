// device_views.hpp -- plain structs handed to the kernels by value: where a packed
// problem and a decomposition plan live in HBM.
//
// HBM layout (structure of arrays, everything fp64 / int32, resident for the
// lifetime of the handle):
//   x[N]          currently assigned value of every variable (Variable::m_value);
//                 during a solve the free entries hold the clamped trial point
//   lo[N], hi[N]  single-interval domain (VariableDomain::interval())
//   BA  factors:  cam[F], pt[F] first variable id of the camera / point block,
//                 obs[F] (double2, one 16-byte load per factor);
//                 cam_blocks[] the distinct camera blocks, xrot[N] their rotation records
//   NLP factors:  coeff[F], rowptr[F+1], vid/expo/cons/sine[nnz]   (CSR)
//   plan:         order[ncomp] (heaviest component first), free_ptr/free_vid,
//                 fac_ptr/fac_id, v2s_ptr + slot_pos (gfac is variable-major: the
//                 partials that feed free variable i are the contiguous range
//                 gfac[v2s_ptr[i] .. v2s_ptr[i+1]) in factor-list order; slot_pos maps
//                 a factor's slot to its position there, so factor lanes scatter and
//                 variable lanes read a contiguous run),
//                 ws[5 * nfree] (p, xi, g, h, x_init per component, contiguous),
//                 dir[N] (search direction scattered by variable id; zero at
//                 non-free variables), gfac[12F | nnz] (per-factor partials of the
//                 last full-gradient evaluation), xstart[nfree], outputs.
//
// These types and the constants that size them live in namespace rdis_views, which namespace rdis_hip imports.
// refround_kernels.hip compiles the solver headers a second time with rdis_hip renamed: the import below is renamed
// with them, the types are not, so the host and both instantiations hand each other the very same structs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rdis_views {

constexpr int KIND_BA = 0;
constexpr int KIND_NLP = 1;
constexpr int ROT_PER_FACTOR = 0, ROT_RECORDS = 1, ROT_CAMFIX = 2;

struct ProblemView {
    int kind;
    int N, F;
    double* x;
    const double* lo;
    const double* hi;
    const int* cam;
    const int* pt;
    const double2* obs;
    double* xrot;         // null, or a shadow of x holding at every camera block's first id the camera's
                          // rotation record (7 doubles, factors.hpp), current for the assigned x at launch
    int rot_mode;         // ROT_PER_FACTOR: not used; ROT_RECORDS: factors read the records and a component rewrites
                          // those of its free cameras (PlanView::cb) at every trial point; ROT_CAMFIX: no camera
                          // variable is free in the launch -- records only read, point partials only
    const double* coeff;
    const int* rowptr;
    const int* vid;
    const double* expo;
    const double* cons;
    const uint8_t* sine;
    const uint8_t* useexp;  // null, or per factor: value = coeff * exp(-product) (NonlinearProductFactor.cpp:140)
};

struct PlanView {
    int ncomp;
    const int* order;
    const int* free_ptr;
    const int* free_vid;
    const int* fac_ptr;
    const int* fac_id;
    const int* v2s_ptr;   // [nfree_total + 1]
    const int* slot_base; // [nfac_total + 1] first slot of each LISTED factor (plan-local: 12 per BA factor, arity per NLP factor)
    const int* cb_ptr;    // [ncomp + 1] ...
    const int* cb;        // ... camera blocks (first variable id) with a free rotation variable, per component
    const int* cb_li;     // [3 per block] local index of the block's three rotation variables, -1 = constant
    const int* slot_pos;  // [slot_base[nfac_total]] listed factor's slot -> position in gfac (variable-major), -1 = not a free variable
    // LDS-resident batch solver (solver_lds.hpp): a component's variables -- free ones and the constants its
    // factors read -- as slots, camera blocks first (9 each), then point blocks (3 each)
    const int* ls_ptr;    // [ncomp + 1] first slot of a component (equal to the next: the component has no table)
    const int* ls_vid;    // [slots] variable id
    const int* ls_free;   // [slots] local free index, -1 = constant
    const int* ls_ncb;    // [ncomp] camera blocks of the component
    const double2* ls_obs;    // [nfac_total] observation of every listed factor (copy in listed order: no indirection in the trial loop)
    int ls_cam_gfac;          // option lds_camera_sums = 0: camera partials through gfac[] like solver_wg.hpp (bit-for-bit comparisons)
    int ls_matrix;            // 1: line-search trials in matrix form (factors.hpp: ba_camera_trial / ba_trial_value / ba_trial_slope) -- a camera's
                              // rotation matrix and its derivative along the direction once per camera and trial, 16 + 16 doubles in LDS behind
                              // the solver's other arrays; 0: the vector form per factor (the bits of solver_wg.hpp)
    const int* ls_gptr;       // [ncomp + 1] wave-chunks (64 entries) of ls_gperm, per component
    const int* ls_gperm;      // per component: local indices of its listed factors grouped by camera block (listed order inside a
                          // group), every group padded to whole chunks with -1
    const unsigned* ls_fidx;  // [nfac_total] listed factor -> camera block | point block << 12 (block numbers within the component)
    // point-major streaming solver (solver_ptm.hpp): the same slot tables, point blocks ordered by their number of factors
    // and taken 64 at a time (a wave-chunk)
    const int* pm_pt0;    // [ncomp] a component's first point block in pm_rec
    const int* pm_ch0;    // [ncomp] its first entry in pm_cptr (which has one more entry than wave-chunks per component)
    const int* pm_cptr;   // a wave-chunk's factors: entries [pm_cptr[c], pm_cptr[c + 1]) of pm_cam / pm_obs / pm_cgp, slot-major --
                          // entry pm_cptr[c] + 64 t + lane is the t-th factor of the lane's point block
    double* pm_rec;       // [blocks][6] p, xi of a point block's three variables
    double* pm_gh;        // [blocks][6] g, h of the Polak-Ribiere recurrence for them
    float* pm_cbox;       // [entries of pm_cptr][8] per wave-chunk a box inside the domains of its blocks: lo[3], -, hi[3], - (floats, rounded inward)
    double* pm_bex;       // [blocks][6] the blocks' exact bounds lo[3], hi[3]
    const short* pm_cam;  // [entries] camera block (number within the component), -1 = no factor ...
    const double2* pm_obs;  // ... and observation of a point's factor
    // the gradient's rounds (solver_ptm.hpp: gradient_to_xi), for workgroup w = component * K + rank of the launch:
    const unsigned short* pm_grow;     // [entries] the factor's staging row in its round: its rank among the round's factors ordered by camera
    const unsigned short* pm_rounds;   // per round ptm_round_stride(ncb) 16-bit words: per camera the first row of its segment [ncb + 1]
    const long long* pm_rd_off;        // [ncomp * K] a workgroup's first word in pm_rounds ...
    const int* pm_rd_n;                // ... and its number of rounds
    int pm_round_slots;                // slots a round evaluates and stages (1 or 2): what the tables above were built for
    // a trial's work by wave (solver_ptm.hpp: eval_line): rows (wave-chunk, first entry, end entry); wave w of workgroup
    // (component, rank) takes the rows w, w + waves, w + 2 waves, ... up to the first empty one.  A workgroup's table:
    // its number of rows R and three ints of nothing, then the rows' chunks [R], first entries [R], end entries [R]
    const int* pm_segs;
    const long long* pm_sg_off;        // [ncomp * K] a workgroup's table in pm_segs
    int* st_ev;           // stale-cache emulation (solver_lds.hpp): per listed factor the assignment of its last value evaluation ...
    double* st_val;       // ... and that value; null unless the plan's option emulate_stale_cache is set
    // the parity option (plan option factor_rounding = 1; solver_coop.hpp / solver_lds.hpp in refround_kernels.hip): sums in the
    // reference's order are added from these by one lane / wave
    double* seq_val;      // [nfac_total] a listed factor's value at the trial point at hand
    double* seq_ab;       // [2][seq_n] by free index: the terms of gg and dgg (cooperative solver)
    int seq_n;            // nfree_total
    long long* timing;    // debug counters of the batch solvers (-DRDIS_COOP_TIMING builds), or null
    double* ws;           // 5 vectors per component, component c at 5*free_ptr[c]
    double* dir;          // [N]
    double* gfac;         // [v2s_ptr[nfree_total]] per-factor partials, variable-major
    const double* xstart; // [nfree_total]
    double* xout;         // [nfree_total]
    double* fret;
    double* delta;
    int* iters;
    int* status;
    long long* nfeval;
    long long* ngeval;
    double* trace;        // [ncomp][trace_cap][4] or null
    int* trace_n;         // [ncomp]
    int trace_cap;
    double* vdump;        // [2 * dump_iters * nfree_total] p, xi at the start of each line search, or null
    int dump_iters;
};

// ---- exchange state of the cooperative solvers (grid_sync.hpp has the protocol) ----
constexpr int COOP_MAX_WG = 512;
constexpr int COOP_SPEC = 1;  // line-search trial points evaluated per exchange (minimizer.hpp: speculation)
constexpr int COOP_K = (2 * COOP_SPEC > 3 ? 2 * COOP_SPEC : 3);  // values per exchange
constexpr int COOP_NBUF = 4;
constexpr int COOP_MAX_WAVES = 8;  // waves per workgroup of the grid solvers (512 lanes)
constexpr int COOP_KP = (COOP_K + 1) / 2 * 2;   // granules per entry, padded to 16-byte pairs
struct CoopState {
    // [COOP_NBUF buffers][entries: workgroup * waves + wave][COOP_KP] granules -- the values an entry
    // publishes in one exchange are neighbours, written and read two at a time (16 bytes: half the
    // memory operations of a sweep; each half is still checked on its own, nothing relies on the
    // pair arriving together) -- then an abort word
    alignas(32) unsigned long long granule[COOP_NBUF][COOP_MAX_WG * COOP_MAX_WAVES][COOP_KP];
    unsigned int abort_flag;
    unsigned int pad[15];
};

// the same for a small group: a component shared by a few workgroups of the point-major streaming solver
// (solver_ptm.hpp), one state per group that runs concurrently -- up to a hundred or so per launch
constexpr int SMALL_COOP_ENTRIES = 256;   // workgroups x waves of a group
struct SmallCoopState {
    alignas(32) unsigned long long granule[COOP_NBUF][SMALL_COOP_ENTRIES][COOP_KP];
    unsigned int abort_flag;
    unsigned int pad[15];
};

// ... and for a WIDE group of that solver (a large share of the device on one component): a CoopState whose entries are one per
// WORKGROUP -- its first wave publishes values the caller has already summed over the workgroup (every lane holds them) --
// 256 entries to sweep instead of 2048
struct WideCoopState : CoopState {};

// ---- arguments of the cooperative solvers (solver_coop.hpp, solver_pipe.hpp) ----
struct CoopArgs {
    long long* timing;     // [8] cycle accumulators written by lane 0 (profiling aid)
    CoopState* st;
    const int* slot_li;    // [12 * m]: local free index of each factor slot or -1 (constant)
    const int* lane_var;   // [nwg * threads]: free variable owned by this lane or -1
    const int* wave_var;   // [nwg * threads / 64]: free variable owned by this wave or -1
    double* xi_glob;       // [n] published search direction
    int comp;
    int poll_delay;        // x64 cycles between publishing and the first sweep (a store needs about that long to land)
    int speculate;         // evaluate guesses at the following trial steps with every line-search trial (minimizer.hpp)
    int reference_slope;   // plan option factor_rounding = 1, the PARITY option: every sum a trial or a CG iteration forms is added in the
                           // reference's order -- the objective over the factors in list order, every variable's partials in factor-list
                           // order, gradient times direction and the Polak-Ribiere sums over the variables in list order (solver_coop.hpp:
                           // ordered_sums; looked at by the reference-rounding instantiation only, refround_kernels.hip)
    int stale;             // ... with it, plan option emulate_stale_cache: the reference's factor cache (Variable.cpp:66-76, Factor.h:228-234)
    int poll_inflight;     // pipelined solver, plan option coop_poll_inflight: the collector keeps several polls of a slot in flight (solver_pipe.hpp: sweep_ring)
    int poll_stagger;      // ... x64 cycles between two of them (coop_poll_stagger)
    double* objective;     // pipelined solver, a plan whose one launch is this group: where the lane that writes fret stores the plan's
                           // objective as well (what objective_sum_kernel would make of the one fret); nullptr otherwise
};

// One launch solves several components side by side: workgroups [wg0, wg0 + nwg) of the grid form
// the group of component a.comp, with its own exchange state; groups never talk to each other.
struct CoopGroup {
    CoopArgs a;
    int wg0, nwg;
};

}  // namespace rdis_views

namespace rdis_hip { using namespace rdis_views; }
