/* Stand-alone driver of the addon's n_q ring (sph-pie_amd/csrc/pie_nq_ring.h), built with -fsanitize=address,undefined by
 * tests/test_comm_cpu.py: push / front / pop / clear, a full ring refusing a push, and many wraparounds at both capacities the
 * addon uses (16 ordinary, 8 wide).  The ring lives in a heap block of exactly its size, so a slot index outside it is an ASan
 * report, and two rings side by side never see each other's entries. */
#include <stdio.h>
#include <stdlib.h>

#include "../sph-pie_amd/csrc/pie_nq_ring.h"

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static int drive(unsigned cap)
{
    pie_nq_ring *a = calloc(1, sizeof *a), *b = calloc(1, sizeof *b);
    EXPECT(a && b);
    EXPECT(nq_ring_count(a) == 0 && nq_ring_front(a, cap) == 0);
    nq_ring_pop(a); /* empty: nothing happens */
    EXPECT(nq_ring_count(a) == 0);
    /* fill, refuse, drain in order */
    for (unsigned i = 0; i < cap; ++i) EXPECT(nq_ring_push(a, cap, 100 + (int)i));
    EXPECT(!nq_ring_push(a, cap, 999) && nq_ring_count(a) == cap && nq_ring_count(b) == 0);
    for (unsigned i = 0; i < cap; ++i) {
        EXPECT(nq_ring_front(a, cap) == 100 + (int)i);
        EXPECT(nq_ring_front(a, cap) == 100 + (int)i); /* front leaves the entry in place */
        nq_ring_pop(a);
    }
    EXPECT(nq_ring_count(a) == 0);
    /* two communicators interleaved, a few entries held, across many wraparounds (and across the unsigned counters' own wrap) */
    a->head = a->tail = 0xFFFFFFF0u;
    int next_a = 1, next_b = 1000, want_a = 1, want_b = 1000;
    for (int round = 0; round < 1000; ++round) {
        for (int k = 0; k < 1 + round % 3; ++k) {
            EXPECT(nq_ring_push(a, cap, next_a++));
            EXPECT(nq_ring_push(b, cap, next_b++));
        }
        while (nq_ring_count(b)) {
            EXPECT(nq_ring_front(b, cap) == want_b++);
            nq_ring_pop(b);
        }
        while (nq_ring_count(a)) {
            EXPECT(nq_ring_front(a, cap) == want_a++);
            nq_ring_pop(a);
        }
    }
    EXPECT(want_a == next_a && want_b == next_b);
    /* clear with entries held: empty, and usable again */
    EXPECT(nq_ring_push(a, cap, 7) && nq_ring_push(a, cap, 8));
    nq_ring_clear(a);
    EXPECT(nq_ring_count(a) == 0 && nq_ring_front(a, cap) == 0);
    EXPECT(nq_ring_push(a, cap, 9) && nq_ring_front(a, cap) == 9);
    free(a);
    free(b);
    return 0;
}

int main(void)
{
    if (drive(16) || drive(8)) return 1;
    printf("nq ring ok\n");
    return 0;
}
