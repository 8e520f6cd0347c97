// hot_split_test.hip -- CgdMachine::hot_pre + hot_post (the pipelined solver's split Brent step, rdis_amd/csrc/minimizer.hpp)
// against CgdMachine::hot() on random machine states in S_DB_EVAL and on edge cases: the same decision, the same next trial
// step and the same new state and counters, bit for bit.  Built by tests/test_hot_split.py with
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o hot_split_test hot_split_test.hip
// and run as `hot_split_test host N SEED` (the CPU) or `hot_split_test device N SEED` (one case per GPU thread).  Prints one
// line: cases, mismatches, and how often each branch of the step was taken.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../rdis_amd/csrc/minimizer.hpp"
using namespace rdis_hip;

enum { C_CASES, C_BAD, C_TAKEN, C_LE, C_C1, C_C2, C_NAN, C_CONV, C_ITMAX, C_TINY, C_ACCEPT, C_N };

__host__ __device__ inline unsigned long long mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct Rng {
    unsigned long long s;
    __host__ __device__ unsigned long long next() { s = mix(s); return s; }
    __host__ __device__ double unit() { return (double)(next() >> 11) * 0x1.0p-53; }
    __host__ __device__ int below(int n) { return (int)(next() % (unsigned long long)n); }
};
__host__ __device__ inline double bits_to_double(unsigned long long b) { double d; memcpy(&d, &b, 8); return d; }
__host__ __device__ inline bool same(double a, double b) { unsigned long long x, y; memcpy(&x, &a, 8); memcpy(&y, &b, 8); return x == y; }

// a value near the line's scale: mostly small steps of a line search, some exact ties and specials
__host__ __device__ inline double pick(Rng& r, const double* tie, int ntie) {
    switch (r.below(12)) {
    case 0: return tie[r.below(ntie)];
    case 1: return r.below(2) ? 0.0 : -0.0;
    case 2: return bits_to_double(0x7FF8000000000000ull);
    case 3: return (r.unit() - 0.5) * 1e-9;
    case 4: return (r.unit() - 0.5) * 3.2;
    default: return (r.unit() - 0.3) * 1e-3 * r.unit();
    }
}

// case k of a run: a machine in S_DB_EVAL and a reply
__host__ __device__ inline void make_case(unsigned long long seed, long long k, CgdMachine& M, double& fu, double& du) {
    Rng r{mix(seed ^ mix((unsigned long long)k))};
    memset(&M, 0, sizeof(M));
    M.st = CgdMachine::S_DB_EVAL;
    M.pp_tag = TR_NONE;
    M.maxiters = 25; M.ftol = 3e-8;
    const int kind = r.below(8);
    double a = -1.6 * r.unit(), b = r.unit();
    if (kind == 0) { const double m = (r.unit() - 0.5) * 1e-6; a = m - r.unit() * 1e-12; b = m + r.unit() * 1e-12; }   // (nearly) converged
    if (kind == 1) { a = b = (r.unit() - 0.5) * 1e-4; }
    const double t0[2] = {a, b};
    double x = a + (b - a) * r.unit();
    if (kind == 2) x = t0[r.below(2)];
    const double tx[3] = {a, b, x};
    double w = r.below(4) == 0 ? x : pick(r, tx, 3), v = r.below(4) == 0 ? w : (r.below(4) == 0 ? x : pick(r, tx, 3));
    double uu = r.below(6) == 0 ? x : x + (r.unit() - 0.5) * (b - a);
    if (kind == 3) uu = x + (r.below(2) ? 1.0 : -1.0) * (3.0e-8 * (x < 0 ? -x : x) + 2.220446049250313e-19);
    const double fbase = 100.0 * r.unit();
    double fx = fbase, fw = r.below(5) == 0 ? fx : fbase + r.unit(), fv = r.below(5) == 0 ? fw : fbase + 2.0 * r.unit();
    const double sl[4] = {0.0, -0.0, 1.0, -1.0};
    double dx = pick(r, sl, 4), dw = r.below(4) == 0 ? dx : pick(r, sl, 4), dv = r.below(4) == 0 ? dx : (r.below(4) == 0 ? dw : pick(r, sl, 4));
    const double te[3] = {0.0, b - a, 1e-9};
    M.a = a; M.b = b; M.x = x; M.w = w; M.v = v; M.fx = fx; M.fw = fw; M.fv = fv;
    M.dx = dx; M.dw = dw; M.dv = dv; M.uu = uu;
    M.d = pick(r, te, 3); M.e = pick(r, te, 3);
    M.it = r.below(3) == 0 ? 97 + r.below(4) : r.below(100);
    M.tiny = r.below(4) == 0;
    M.saw_nan = r.below(8) == 0;
    M.nfeval = (long long)r.below(100000); M.ngeval = (long long)r.below(100000);
    const double tf[3] = {fx, fw, fv};
    fu = r.below(3) == 0 ? tf[r.below(3)] : (r.below(16) == 0 ? bits_to_double(0x7FF8000000000000ull) : fbase + (r.unit() - 0.5) * 4.0);
    const double td[3] = {dx, dw, dv};
    du = r.below(3) == 0 ? td[r.below(3)] : pick(r, sl, 4);
}

__host__ __device__ inline bool same_machine(const CgdMachine& p, const CgdMachine& q) {
    return same(p.a, q.a) && same(p.b, q.b) && same(p.x, q.x) && same(p.w, q.w) && same(p.v, q.v) && same(p.fx, q.fx) &&
           same(p.fw, q.fw) && same(p.fv, q.fv) && same(p.dx, q.dx) && same(p.dw, q.dw) && same(p.dv, q.dv) && same(p.d, q.d) &&
           same(p.e, q.e) && same(p.uu, q.uu) && p.it == q.it && p.tiny == q.tiny && p.saw_nan == q.saw_nan &&
           p.nfeval == q.nfeval && p.ngeval == q.ngeval && p.pp_tag == q.pp_tag && p.st == q.st;
}

// one case: counts into c[C_N]
__host__ __device__ inline void run_case(unsigned long long seed, long long k, unsigned long long* c) {
    CgdMachine M;
    double fu, du;
    make_case(seed, k, M, fu, du);
    CgdMachine A = M;
    double un1 = 0.0, pa = 0.0, pb = 0.0, pc = 0.0;
    int ptag = -1;
    Predictor G;
    const bool ok1 = A.hot(fu, du, un1, ptag, pa, pb, pc, G);
    const BrentHot s = M.brent();
    HotPre P;
    CgdMachine::hot_pre(s, P);
    BrentHot n;
    double un2 = 0.0;
    const bool ok2 = CgdMachine::hot_post(s, P, fu, du, n, un2);
    CgdMachine B = M;
    if (ok2) { B.set_brent(n); B.pp_tag = TR_NONE; }
    bool good = ok1 == ok2 && same_machine(A, B);
    if (ok1) good = good && same(un1, un2) && ptag == TR_NONE;
    c[C_CASES] += 1;
    c[C_BAD] += good ? 0 : 1;
    const bool le = fu <= M.fx;
    const bool c1 = !le && (fu <= M.fw || M.w == M.x);
    c[C_TAKEN] += ok1;
    c[C_LE] += ok1 && le;
    c[C_C1] += ok1 && c1;
    c[C_C2] += ok1 && !le && !c1 && (fu < M.fv || M.v == M.x || M.v == M.w);
    c[C_NAN] += ok1 && fu != fu;
    c[C_CONV] += !ok1 && M.it + 1 < 100 && !(M.tiny && fu > M.fx);
    c[C_ITMAX] += M.it + 1 >= 100;
    c[C_TINY] += M.tiny && fu > M.fx;
    c[C_ACCEPT] += ok1 && same(A.e, M.d);   // (the secant step was taken, or the bisection came out the same)
}

__global__ void check_kernel(unsigned long long seed, long long n, unsigned long long* out) {
    unsigned long long c[C_N] = {};
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) run_case(seed, k, c);
    for (int i = 0; i < C_N; ++i) if (c[i]) atomicAdd(&out[i], c[i]);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s host|device N SEED\n", argv[0]); return 2; }
    const long long n = atoll(argv[2]);
    const unsigned long long seed = strtoull(argv[3], nullptr, 0);
    unsigned long long c[C_N] = {};
    if (strcmp(argv[1], "device") == 0) {
        unsigned long long* d = nullptr;
        if (hipMalloc(&d, sizeof(c)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 3; }
        if (hipMemset(d, 0, sizeof(c)) != hipSuccess) return 3;
        check_kernel<<<1024, 256>>>(seed, n, d);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 3; }
        if (hipMemcpy(c, d, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return 3;
        (void)hipFree(d);
    } else {
        for (long long k = 0; k < n; ++k) run_case(seed, k, c);
    }
    printf("cases %llu bad %llu taken %llu le %llu c1 %llu c2 %llu nan %llu conv %llu itmax %llu tiny %llu accept %llu\n",
           c[C_CASES], c[C_BAD], c[C_TAKEN], c[C_LE], c[C_C1], c[C_C2], c[C_NAN], c[C_CONV], c[C_ITMAX], c[C_TINY], c[C_ACCEPT]);
    return c[C_BAD] == 0 ? 0 : 1;
}
