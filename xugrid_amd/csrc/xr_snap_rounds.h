// xr_snap_rounds.h -- the host side of the decision rounds of xr_snap.hip, free of HIP so that a stand-alone program can run it
// (tests/native/snap_rounds_main.cpp): when the status words are read, when the loop stops, and the guard on the adjacency's size.
#pragma once
#include <cstdint>

namespace xr {

// launches between two reads of the status words by the host
static constexpr int SNAP_ROUNDS_PER_READ = 4;

// the adjacency is indexed with int32
inline bool snap_pairs_fit(unsigned long long n_pair) { return n_pair <= (unsigned long long)INT32_MAX; }

// launch(round) for round = 1, 2, ..; decided = read() behind round 1 and behind every SNAP_ROUNDS_PER_READ-th round, until it says
// that all n points are decided.  Every launch decides at least the lowest undecided point, so n launches always suffice: a loop
// that is still running SNAP_ROUNDS_PER_READ launches later is given up.  -> the launches made, -1 when given up.
template <typename Launch, typename Read> int64_t snap_run_rounds(int64_t n, Launch &&launch, Read &&read) {
    int64_t decided = 0, round = 0;
    while (decided < n) {
        if (round >= n + SNAP_ROUNDS_PER_READ) return -1;
        launch(++round);
        if (round == 1 || round % SNAP_ROUNDS_PER_READ == 0) decided = read();
    }
    return round;
}

} // namespace xr
