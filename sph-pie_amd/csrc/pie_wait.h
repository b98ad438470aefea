// pie_wait.h — the one bounded wait: every host wait on the device (a summary word in mapped memory, an event) goes through
// bounded_wait, so none outlives PIE_WAIT_DEADLINE_MS.  Plain templates, no HIP, so a host-only program can drive the loop with
// fake callables (tests/wait_test.cpp); the call sites pass lambdas around hipStreamQuery / hipEventQuery.
#ifndef PIE_WAIT_H
#define PIE_WAIT_H

#include <ctime>
#include <limits>
#include <sched.h>

namespace pie {

enum class WaitEnd { Ready, Drained, Failed, Deadline };
struct WaitResult {
    WaitEnd end;
    int err;          // Failed: what the probe returned
    double waited_ms; // at the last probe point (0 when none was reached)
};

// what a probe returns besides an error code of its own
constexpr int kProbeDone = 0;      // the stream / event behind the awaited thing has finished
constexpr int kProbeNotReady = -1; // still running
// A spin is one ready() call.  The probe and the clock are consulted on spins (counted from 1) that are a multiple of
// probe_mask + 1; on those past `relax_after` the loop relaxes as `relax` says, on every other spin it pauses.
struct WaitPace {
    unsigned probe_mask, relax_after;
    enum Relax { Pause, Yield, Nap20us } relax;
};
// The paces were tuned against the measured finish latencies of their sites; they are not interchangeable.
constexpr WaitPace kPaceSummary{0x3FFFF, 0, WaitPace::Pause};   // scan_finish, batch_finish, pie_expired_queue: a probe per ~1 ms of pauses
constexpr WaitPace kPaceEvent{0, 65, WaitPace::Yield};          // wide_finish, flight_slot_landed: the event every spin
constexpr WaitPace kPaceSideSummary{0xFF, 4096, WaitPace::Yield}; // expq_land
constexpr WaitPace kPaceCommEvent{0, 256, WaitPace::Nap20us};   // wait_event (pie_comm.hip)
constexpr double kNoGraceLimit = std::numeric_limits<double>::infinity(); // drained_grace_ms: a done probe never ends the wait

// Spins until ready() (Ready, behind an acquire fence: what was published before the awaited word may be read), the probe
// returns an error (Failed), the probe has said kProbeDone while ready() stayed false for drained_grace_ms (Drained), or
// deadline_ms has passed (Deadline) — checked in that order at each probe point.
template <class Ready, class Probe>
inline WaitResult bounded_wait(Ready ready, Probe probe, double deadline_ms, double drained_grace_ms, WaitPace pace)
{
    timespec t0{};
    clock_gettime(CLOCK_MONOTONIC, &t0);
    double waited_ms = 0;
    for (unsigned long long spins = 1;; ++spins) {
        if (ready()) break;
        if ((spins & pace.probe_mask) != 0) {
            __builtin_ia32_pause();
            continue;
        }
        const int e = probe();
        timespec t1{};
        clock_gettime(CLOCK_MONOTONIC, &t1);
        waited_ms = (double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6;
        if (e != kProbeDone && e != kProbeNotReady) return {WaitEnd::Failed, e, waited_ms};
        if (e == kProbeDone) {
            if (ready()) break;
            if (waited_ms >= drained_grace_ms) return {WaitEnd::Drained, 0, waited_ms};
        }
        if (waited_ms > deadline_ms) return {WaitEnd::Deadline, 0, waited_ms};
        const timespec nap{0, 20000};
        if (pace.relax == WaitPace::Pause || spins <= pace.relax_after) __builtin_ia32_pause();
        else if (pace.relax == WaitPace::Yield) sched_yield();
        else nanosleep(&nap, nullptr);
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return {WaitEnd::Ready, 0, waited_ms};
}

} // namespace pie

#endif
