/* Seeds whose first draws hold a far-tail uniform ("Where chance never goes").  A consumer kernel starts its lanes
 * and days at 0 and the Philox key is not invertible, so a far-tail draw (min(u, 1 - u) < e^-25, 2.8e-11 per draw) inside a consumer
 * is found by walking seeds: for every seed of [start, start + count) the box t < 3, lane < 64 of stream 0 is generated and every
 * uniform whose lattice index n = (w_a >> 6) 2^26 + (w_b >> 6) has n <= far or 2^52 - 1 - n <= far is reported as a line
 *     seed stream t row lane n
 * box 3: rows 0, 1, 2 (two blocks per (t, lane): the pair (0, 1), and row 2 from words (0, 1) of the block q = 1)
 * box 1: row 0 only (one block per (t, lane))
 * The suite runs a small range around a recorded seed only (tests/test_noise_place.py); tests/golden/noise_far_tail_seeds.json
 * holds what the full search found.  Its own Philox: no code is shared with csrc/noise.hpp or tests/noise_ref.c.
 *
 *     cc -O3 -pthread noise_seed_search.c -o noise_seed_search;  noise_seed_search START COUNT BOX FAR [THREADS] */
#include <inttypes.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define BOX_T 3
#define BOX_LANES 64

typedef struct { uint64_t start, count; int box, tid, nthreads; uint64_t far; } job_t;

static pthread_mutex_t out_lock = PTHREAD_MUTEX_INITIALIZER;

static inline void block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)c0 * 0xD2511F53u, p1 = (uint64_t)c2 * 0xCD9E8D57u;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0; c1 = (uint32_t)p1;
        c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

static void report(uint64_t seed, uint32_t t, int row, uint32_t lane, uint32_t wa, uint32_t wb, uint64_t far)
{
    const uint64_t n = ((uint64_t)(wa >> 6) << 26) + (uint64_t)(wb >> 6), top = ((uint64_t)1 << 52) - 1;
    if (n <= far || top - n <= far) {
        pthread_mutex_lock(&out_lock);
        printf("%" PRIu64 " 0 %u %d %u %" PRIu64 "\n", seed, t, row, lane, n);
        fflush(stdout);
        pthread_mutex_unlock(&out_lock);
    }
}

static void *scan(void *arg)
{
    const job_t *j = (const job_t *)arg;
    const int nq = j->box == 3 ? 2 : 1;
    for (uint64_t i = (uint64_t)j->tid; i < j->count; i += (uint64_t)j->nthreads) {
        const uint64_t seed = j->start + i;
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        for (uint32_t t = 0; t < BOX_T; t++)
            for (int q = 0; q < nq; q++)
                for (uint32_t lane = 0; lane < BOX_LANES; lane++) {
                    uint32_t w[4];
                    block(lane, 0u, t, 0x80000000u | (uint32_t)q, k0, k1, w);
                    /* the 26 high bits of the index all zeros or all ones: one uniform in 2^25 gets past this */
                    if ((((w[0] >> 6) + 1u) & 0x3ffffffu) <= 1u) report(seed, t, 2 * q, lane, w[0], w[1], j->far);
                    if (j->box == 3 && q == 0 && (((w[2] >> 6) + 1u) & 0x3ffffffu) <= 1u) report(seed, t, 1, lane, w[2], w[3], j->far);
                }
    }
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s START COUNT BOX(3|1) FAR [THREADS]\n", argv[0]);
        return 2;
    }
    const uint64_t start = strtoull(argv[1], NULL, 0), count = strtoull(argv[2], NULL, 0), far = strtoull(argv[4], NULL, 0);
    const int box = atoi(argv[3]);
    int nthreads = argc > 5 ? atoi(argv[5]) : 1;
    if ((box != 3 && box != 1) || nthreads < 1 || nthreads > 256) return 2;
    pthread_t th[256];
    job_t jobs[256];
    for (int k = 0; k < nthreads; k++) {
        jobs[k] = (job_t){start, count, box, k, nthreads, far};
        if (pthread_create(&th[k], NULL, scan, &jobs[k])) return 1;
    }
    for (int k = 0; k < nthreads; k++) pthread_join(th[k], NULL);
    return 0;
}
