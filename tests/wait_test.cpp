// Stand-alone check of the one bounded wait (sph-pie_amd/csrc/pie_wait.h) with fake `ready` / `probe` callables: every way
// the loop can end, and the probe cadence of each pace constant.  Built with ASan + UBSan by tests/test_wait.py; no GPU,
// nothing of it is loaded into python.
#include "../sph-pie_amd/csrc/pie_wait.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>

using namespace pie;

static int fails = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

static const WaitPace kPaces[] = {kPaceSummary, kPaceEvent, kPaceSideSummary, kPaceCommEvent};
constexpr double kLong = 60000.0; // a deadline no case below comes near

static double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the word lands after `land_at` spins: the probe runs only on spins that are a multiple of the cadence, and on all of those
static void check_cadence(WaitPace pace, unsigned long long land_at)
{
    unsigned long long spins = 0, probes = 0, off_beat = 0;
    const WaitResult r = bounded_wait([&] { return ++spins > land_at; },
                                      [&] {
                                          ++probes;
                                          if (spins % ((unsigned long long)pace.probe_mask + 1) != 0) ++off_beat;
                                          return kProbeNotReady;
                                      },
                                      kLong, kNoGraceLimit, pace);
    CHECK(r.end == WaitEnd::Ready && r.err == 0);
    CHECK(spins == land_at + 1);
    CHECK(off_beat == 0);
    CHECK(probes == land_at / ((unsigned long long)pace.probe_mask + 1));
}

int main()
{
    // the paces are the sites' own (pie_wait.h): a change here is a change of a tuned wait
    CHECK(kPaceSummary.probe_mask == 0x3FFFF && kPaceSummary.relax == WaitPace::Pause);
    CHECK(kPaceEvent.probe_mask == 0 && kPaceEvent.relax_after == 65 && kPaceEvent.relax == WaitPace::Yield);
    CHECK(kPaceSideSummary.probe_mask == 0xFF && kPaceSideSummary.relax_after == 4096 && kPaceSideSummary.relax == WaitPace::Yield);
    CHECK(kPaceCommEvent.probe_mask == 0 && kPaceCommEvent.relax_after == 256 && kPaceCommEvent.relax == WaitPace::Nap20us);

    for (const WaitPace pace : kPaces) {
        // Ready at once: the probe is never called
        int probes = 0;
        WaitResult r = bounded_wait([] { return true; }, [&] { ++probes; return 7; }, kLong, 0.0, pace);
        CHECK(r.end == WaitEnd::Ready && probes == 0 && r.waited_ms == 0);
        // Failed carries the probe's code
        r = bounded_wait([] { return false; }, [] { return 709; }, kLong, 0.0, pace);
        CHECK(r.end == WaitEnd::Failed && r.err == 709);
        // Drained at once with grace 0: at the first probe point
        unsigned long long spins = 0;
        probes = 0;
        r = bounded_wait([&] { ++spins; return false; }, [&] { ++probes; return kProbeDone; }, kLong, 0.0, pace);
        CHECK(r.end == WaitEnd::Drained && probes == 1 && spins == (unsigned long long)pace.probe_mask + 2); // + the look after the probe
        // a word that lands between the last spin and the probe's "done" is Ready, not Drained
        bool done_seen = false;
        r = bounded_wait([&] { return done_seen; }, [&] { done_seen = true; return kProbeDone; }, kLong, 0.0, pace);
        CHECK(r.end == WaitEnd::Ready);
    }
    // the cadence: a few probe points for the sparse paces, past the turn to yield / nap for the dense ones
    check_cadence(kPaceSummary, 3ull * 0x40000 + 5);
    check_cadence(kPaceSideSummary, 4096 + 3 * 256 + 17);
    check_cadence(kPaceEvent, 200);
    check_cadence(kPaceCommEvent, 300);
    check_cadence(kPaceSideSummary, 255); // lands one spin before the first probe point

    // the word lands from another thread while the loop spins
    {
        std::atomic<unsigned long long> word{0};
        std::thread flip([&] {
            std::this_thread::sleep_for(std::chrono::milliseconds(5));
            word.store(42, std::memory_order_release);
        });
        const WaitResult r = bounded_wait([&] { return word.load(std::memory_order_relaxed) == 42; }, [] { return kProbeNotReady; }, kLong, 0.0, kPaceSideSummary);
        flip.join();
        CHECK(r.end == WaitEnd::Ready);
    }
    // Drained with grace G: not before G has passed ...
    const double G = 30.0;
    {
        const auto t0 = std::chrono::steady_clock::now();
        const WaitResult r = bounded_wait([] { return false; }, [] { return kProbeDone; }, kLong, G, kPaceSideSummary);
        CHECK(r.end == WaitEnd::Drained && r.waited_ms >= G && ms_since(t0) >= G);
    }
    // ... and not at all if the word lands within G
    {
        std::atomic<bool> landed{false};
        std::thread flip([&] {
            std::this_thread::sleep_for(std::chrono::milliseconds(5));
            landed.store(true, std::memory_order_release);
        });
        const WaitResult r = bounded_wait([&] { return landed.load(std::memory_order_relaxed); }, [] { return kProbeDone; }, kLong, 1000.0, kPaceSideSummary);
        flip.join();
        CHECK(r.end == WaitEnd::Ready);
    }
    // no grace limit: a drained probe with a word that never lands ends in Deadline
    {
        const WaitResult r = bounded_wait([] { return false; }, [] { return kProbeDone; }, 20.0, kNoGraceLimit, kPaceSideSummary);
        CHECK(r.end == WaitEnd::Deadline && r.waited_ms >= 20.0);
    }
    // Deadline, for every pace: the call returns, not before 20 ms, and within 50 x that — a hang guard, not a measurement
    for (const WaitPace pace : kPaces) {
        const auto t0 = std::chrono::steady_clock::now();
        const WaitResult r = bounded_wait([] { return false; }, [] { return kProbeNotReady; }, 20.0, 0.0, pace);
        const double took = ms_since(t0);
        CHECK(r.end == WaitEnd::Deadline && r.err == 0 && r.waited_ms >= 20.0 && took >= 20.0 && took < 50 * 20.0);
    }
    if (fails) return 1;
    std::printf("bounded wait ok\n");
    return 0;
}
