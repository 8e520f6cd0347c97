// level_members.h -- the bookkeeping of a population run of the level driver (HipRDISLevelOptimizer::optimizePopulation,
// rdis_levels.h): every member of a population runs the driver's sweeps, the members stop after different numbers of sweeps, and
// the population solves of include/rdis_hip.h take a contiguous range of rows.  So the rows are kept partitioned -- the members
// still running in rows 0 .. active - 1, the stopped ones behind them -- by permuting the population (rdis_hip_population_permute)
// whenever some, but not all, of the running members stop; one last permutation puts member s back into row s.
// Pure host functions: nothing of HIP, no call of the C ABI -- tests/cpp/level_members_test.cpp runs them on the CPU.
#ifndef RDIS_LEVEL_MEMBERS_H_
#define RDIS_LEVEL_MEMBERS_H_

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rdis {

// The driver's own stop test of a sweep (HipRDISLevelOptimizer::optimize: `if (!(before - objective > steptol_)) break;`,
// RDISOptimizer.cpp:1089-1108): no progress beyond steptol.  Written as the negation of the comparison, so that an objective
// that is not a number stops the member, and a gain of exactly steptol does; an objective of -inf goes on.
inline bool levelMemberStops(double before, double objective, double steptol) { return !(before - objective > steptol); }

class LevelMembers {
public:
    explicit LevelMembers(int64_t nmembers) : member_((size_t)(nmembers > 0 ? nmembers : 0)), active_(nmembers > 0 ? nmembers : 0) {
        for (size_t r = 0; r < member_.size(); ++r) member_[r] = (int64_t)r;
    }
    int64_t size() const { return (int64_t)member_.size(); }
    int64_t active() const { return active_; }                       // rows 0 .. active() - 1 hold the members still running
    int64_t memberOfRow(int64_t row) const { return member_[(size_t)row]; }
    const std::vector<int64_t>& rowToMember() const { return member_; }

    // stopped[r] != 0, r < active(): the member in row r has stopped.  The stable partition of the rows -- the running ones first,
    // then the stopped ones, both groups in their current row order (rows active() .. size() - 1, stopped earlier, keep their
    // places) -- as the order of rdis_hip_population_permute: new row r holds what row order[r] held.  The map and active() are
    // those of the permuted rows afterwards.  Returns whether order moves a row at all (false: the identity, no permute needed).
    bool partition(const std::vector<char>& stopped, std::vector<int64_t>& order) {
        const size_t n = member_.size(), a = (size_t)active_;
        order.resize(n);
        size_t k = 0;
        for (size_t r = 0; r < a; ++r) if (!stopped[r]) order[k++] = (int64_t)r;
        const size_t still = k;
        for (size_t r = 0; r < a; ++r) if (stopped[r]) order[k++] = (int64_t)r;
        for (size_t r = a; r < n; ++r) order[r] = (int64_t)r;
        return apply(order, (int64_t)still);
    }

    // The permutation that restores the original numbering: order[s] = the row member s stands in, so that afterwards row s is
    // member s again (the map is the identity; active() is left as it is).  Returns whether it moves a row.
    bool restore(std::vector<int64_t>& order) {
        const size_t n = member_.size();
        order.resize(n);
        for (size_t r = 0; r < n; ++r) order[(size_t)member_[r]] = (int64_t)r;
        return apply(order, active_);
    }

private:
    bool apply(const std::vector<int64_t>& order, int64_t active) {
        std::vector<int64_t> next(member_.size());
        bool moved = false;
        for (size_t r = 0; r < member_.size(); ++r) {
            next[r] = member_[(size_t)order[r]];
            moved = moved || order[r] != (int64_t)r;
        }
        member_.swap(next);
        active_ = active;
        return moved;
    }
    std::vector<int64_t> member_;   // row -> member
    int64_t active_;
};

}  // namespace rdis
#endif  // RDIS_LEVEL_MEMBERS_H_
