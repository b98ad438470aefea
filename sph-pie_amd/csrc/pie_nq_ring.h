/* The n_q of the pipelined steps begun and not yet finished on ONE communicator, oldest first: what the addon needs to size the
 * counts a finish returns.  One ring per communicator and kind (comm_box), never file-static: two communicators, or two Node
 * workers, must not pop each other's n_q.  cap is the kind's number of buffer sets (16 ordinary, 8 wide), a power of two; the
 * library refuses a begin long before the ring is full (12 / 6 steps begun ahead).  Host code only: tests/nq_ring_test.c drives
 * it under ASan + UBSan. */
#ifndef PIE_NQ_RING_H
#define PIE_NQ_RING_H

#define PIE_NQ_RING_MAX 16

typedef struct {
    int nq[PIE_NQ_RING_MAX];
    unsigned head, tail; /* pushes / pops so far; head - tail = entries held */
} pie_nq_ring;

static inline unsigned nq_ring_count(const pie_nq_ring *r) { return r->head - r->tail; }

/* 0 when `cap` entries are already held */
static inline int nq_ring_push(pie_nq_ring *r, unsigned cap, int n_q)
{
    if (nq_ring_count(r) >= cap) return 0;
    r->nq[r->head++ & (cap - 1)] = n_q;
    return 1;
}

/* the oldest entry, left in place (a finish that consumed nothing is repeated); 0 when the ring is empty */
static inline int nq_ring_front(const pie_nq_ring *r, unsigned cap) { return nq_ring_count(r) ? r->nq[r->tail & (cap - 1)] : 0; }

static inline void nq_ring_pop(pie_nq_ring *r)
{
    if (nq_ring_count(r)) r->tail++;
}

static inline void nq_ring_clear(pie_nq_ring *r) { r->tail = r->head; }

#endif /* PIE_NQ_RING_H */
