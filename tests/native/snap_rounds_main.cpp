// Stand-alone check of xugrid_amd/csrc/xr_snap_rounds.h (tests/test_snap_cpu.py compiles and runs it under the sanitizers): the
// round loop of snap_nodes against a pretend device that decides `step` points of a chain per launch.
#include <cstdio>
#include <cstdlib>

#include "../../xugrid_amd/csrc/xr_snap_rounds.h"

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
            failures++;                                              \
        }                                                            \
    } while (0)

struct Run {
    int64_t launches, reads, decided, needed;
};

// a device that decides `step` more points per launch (0: stuck)
static Run run(int64_t n, int64_t step) {
    Run r{0, 0, 0, step > 0 ? (n + step - 1) / step : -1};
    int64_t last_round = 0;
    r.launches = xr::snap_run_rounds(
        n,
        [&](int64_t round) {
            CHECK(round == last_round + 1);
            last_round = round;
            r.decided = r.decided + step < n ? r.decided + step : n;
        },
        [&]() {
            r.reads++;
            return r.decided;
        });
    return r;
}

int main() {
    using xr::SNAP_ROUNDS_PER_READ;
    CHECK(xr::snap_pairs_fit(0) && xr::snap_pairs_fit(2147483647ull));
    CHECK(!xr::snap_pairs_fit(2147483648ull) && !xr::snap_pairs_fit(~0ull));
    CHECK(xr::snap_run_rounds(0, [](int64_t) { std::abort(); }, []() -> int64_t { std::abort(); }) == 0);
    const int64_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 300, 2050};
    const int64_t steps[] = {1, 2, 4, 5, 64, 5000};
    for (int64_t n : sizes)
        for (int64_t step : steps) {
            const Run r = run(n, step);
            CHECK(r.decided == n);
            // stops at the first read that sees the end: the launches needed, rounded up to a read
            const int64_t due = r.needed <= 1 ? 1 : (r.needed + SNAP_ROUNDS_PER_READ - 1) / SNAP_ROUNDS_PER_READ * SNAP_ROUNDS_PER_READ;
            CHECK(r.launches == due);
            CHECK(r.launches < r.needed + SNAP_ROUNDS_PER_READ && r.launches <= n + SNAP_ROUNDS_PER_READ);
            CHECK(r.reads == 1 + r.launches / SNAP_ROUNDS_PER_READ); // behind round 1 and behind every SNAP_ROUNDS_PER_READ-th
        }
    for (int64_t n : sizes) {
        const Run r = run(n, 0); // never decides anything: given up, after a bounded number of launches
        CHECK(r.launches == -1);
    }
    std::printf(failures ? "SNAP_ROUNDS_FAILED %d\n" : "SNAP_ROUNDS_OK\n", failures);
    return failures ? 1 : 0;
}
