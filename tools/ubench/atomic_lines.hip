// Micro-benchmark: rate of returning integer atomics (agent scope) on a histogram of U counters, by how many 64-byte lines the
// 64 lanes of one wave instruction name.  The question it answers: is the cost of a histogram atomic per lane or per line?
//   random      every lane a counter of its own, anywhere in the histogram (a hot-index bin in row order)
//   lines k     64 ascending addresses inside a window of k lines (16 k counters): sorted random draws, so with gaps and a few
//               repeats, as 64 neighbours of a bin ordered by histogram slot give; the window moves through the histogram
//   half        the same with every second lane inactive (a batch that selects half of the records)
// Reported per pattern: G lanes/s (atomics executed) and G requests/s (distinct lines named per instruction, counted on the
// host from the same address generator).
// usage: atomic_lines [U] [wave instructions]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
__host__ __device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// the counter lane `lane` of wave instruction `w` adds to; k = 0: random
__host__ __device__ inline int address_of(long long w, int lane, int k, int n_users)
{
    if (k == 0) return (int)(mix64((unsigned long long)(w * 64 + lane) * 0x9E3779B97F4A7C15ULL + 1) % (unsigned long long)n_users);
    const int span = 16 * k; // counters in the window
    const int windows = n_users / span;
    const int base = (int)(mix64((unsigned long long)w + 0x1234567ULL) % (unsigned long long)windows) * span;
    // ascending with gaps and repeats: lane * span / 64 plus a jitter below one step and a half
    const int step = span / 64 > 0 ? span / 64 : 1;
    const int jit = (int)(mix64((unsigned long long)(w * 64 + lane) + 77) % (unsigned long long)(step + step / 2 + 1));
    const int at = lane * span / 64 + jit;
    return base + (at < span ? at : span - 1);
}
template <bool HALF>
__global__ __launch_bounds__(256) void k_lines(int* counts, int n_users, long long waves, int k, int* sink)
{
    const int lane = threadIdx.x & 63;
    const long long gw = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6, W = ((long long)gridDim.x * 256) >> 6;
    int acc = 0;
    for (long long w = gw; w < waves; w += W) {
        const int u = address_of(w, lane, k, n_users);
        if (!HALF || (lane & 1)) acc += __hip_atomic_fetch_add(&counts[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (acc == 0x7fffffff) *sink = acc;
}
int main(int argc, char** argv)
{
    const int U = argc > 1 ? atoi(argv[1]) : 100000;
    const long long waves = argc > 2 ? atoll(argv[2]) : 400000LL;
    if (U < 16 * 32 || waves < 1) {
        fprintf(stderr, "U must be at least 512, wave instructions at least 1\n");
        return 2;
    }
    int *counts, *sink;
    if (hipMalloc(&counts, (size_t)U * 4) != hipSuccess || hipMalloc(&sink, 4) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    printf("%-22s %9s %12s %14s %12s\n", "pattern", "ms", "G lanes/s", "G requests/s", "lines/instr");
    auto run = [&](const char* name, int k, bool half) {
        // distinct lines per instruction, from a sample of the generator
        double lines = 0;
        const long long sample = std::min<long long>(waves, 2000);
        for (long long w = 0; w < sample; ++w) {
            std::vector<int> l;
            for (int lane = 0; lane < 64; ++lane)
                if (!half || (lane & 1)) l.push_back(address_of(w, lane, k, U) / 16);
            std::sort(l.begin(), l.end());
            lines += (double)(std::unique(l.begin(), l.end()) - l.begin());
        }
        lines /= (double)sample;
        float best = 1e9f;
        for (int r = 0; r < 5; ++r) {
            hipMemset(counts, 0, (size_t)U * 4);
            hipEventRecord(e0);
            if (half) hipLaunchKernelGGL(k_lines<true>, dim3(2048), dim3(256), 0, 0, counts, U, waves, k, sink);
            else hipLaunchKernelGGL(k_lines<false>, dim3(2048), dim3(256), 0, 0, counts, U, waves, k, sink);
            hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        std::vector<int> h((size_t)U);
        hipMemcpy(h.data(), counts, h.size() * 4, hipMemcpyDeviceToHost);
        long long tot = 0;
        for (int v : h) tot += v;
        const long long ops = waves * (half ? 32 : 64);
        printf("%-22s %9.4f %12.1f %14.2f %12.1f  %s\n", name, best, ops / best / 1e6, waves * lines / best / 1e6, lines, tot == ops ? "exact" : "LOST UPDATES");
    };
    char name[64];
    run("random", 0, false);
    run("random, half", 0, true);
    for (int k : {4, 6, 8, 16, 32}) {
        snprintf(name, sizeof name, "lines %d", k);
        run(name, k, false);
        snprintf(name, sizeof name, "lines %d, half", k);
        run(name, k, true);
    }
    return 0;
}
