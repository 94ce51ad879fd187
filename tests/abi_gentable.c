/* A C99 program that solves an LMDE with a host-sampled generator through the C-ABI only (include/midyn_gentable.h):
 *     y' = G y,  G = -i w X  (constant),  y(0) = e0   =>   y(t) = cos(w t) e0 - i sin(w t) e1,
 * Magnus order 1, the step propagators applied in step order, the R sampled rows pushed in two pushes.  Built and run by
 * tests/test_gpu_callable_generator.py with gcc; libmidyn.so and the HIP runtime are dlopen'ed as a non-Python host would.
 * Exit code 0 and a line "GENTABLE_OK ..." on success. */
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/midyn_gentable.h"

#define LOAD(name)                                              \
    *(void**)(&p_##name) = dlsym(h, #name);                     \
    if (!p_##name) {                                            \
        fprintf(stderr, "missing symbol %s\n", #name);          \
        return 2;                                               \
    }

static int (*p_midyn_ctx_create)(int, midyn_ctx**);
static int (*p_midyn_ctx_destroy)(midyn_ctx*);
static const char* (*p_midyn_last_error)(midyn_ctx*);
static int (*p_midyn_gentable_create)(midyn_ctx*, int, int, int, int, const int*, const double*, const int*, int, int, int,
                                      const midyn_complex*, midyn_gentable**);
static int (*p_midyn_gentable_push)(midyn_gentable*, int, int, const midyn_complex*);
static int (*p_midyn_gentable_info)(midyn_gentable*, long long*);
static int (*p_midyn_gentable_finish)(midyn_gentable*, midyn_complex*);
static int (*p_midyn_gentable_destroy)(midyn_gentable*);

#define CHECK(ctx, call)                                                              \
    do {                                                                              \
        if ((call) != 0) {                                                            \
            fprintf(stderr, "%s failed: %s\n", #call, p_midyn_last_error(ctx));       \
            return 10;                                                                \
        }                                                                             \
    } while (0)

enum { NSTEPS = 40, P = 3 };

int main(int argc, char** argv) {
    if (argc < 3) return 64;
    if (!dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL)) {   /* ONE HIP runtime, global, before libmidyn */
        fprintf(stderr, "hip runtime: %s\n", dlerror());
        return 3;
    }
    void* h = dlopen(argv[2], RTLD_NOW);
    if (!h) {
        fprintf(stderr, "libmidyn: %s\n", dlerror());
        return 4;
    }
    LOAD(midyn_ctx_create) LOAD(midyn_ctx_destroy) LOAD(midyn_last_error) LOAD(midyn_gentable_create)
    LOAD(midyn_gentable_push) LOAD(midyn_gentable_info) LOAD(midyn_gentable_finish) LOAD(midyn_gentable_destroy)

    const double w = 1.7, T = 2.0, dt = T / NSTEPS;
    midyn_ctx* ctx = NULL;
    CHECK(NULL, p_midyn_ctx_create(0, &ctx));
    /* Magnus 1: one row per step (its midpoint); the state is saved after step NSTEPS/2 - 1 (slot 1) and at the end (2) */
    int rows[3 * NSTEPS], save[NSTEPS];
    double hs[NSTEPS];
    for (int s = 0; s < NSTEPS; ++s) {
        rows[3 * s] = rows[3 * s + 1] = rows[3 * s + 2] = s;
        hs[s] = dt;
        save[s] = s == NSTEPS / 2 - 1 ? 1 : (s == NSTEPS - 1 ? 2 : -1);
    }
    midyn_complex y0[2] = {1.0, 0.0};
    midyn_complex G[NSTEPS][2][2];
    for (int r = 0; r < NSTEPS; ++r) {
        G[r][0][0] = G[r][1][1] = 0.0;
        G[r][0][1] = G[r][1][0] = -I * w;
    }
    midyn_gentable* gt = NULL;
    CHECK(ctx, p_midyn_gentable_create(ctx, 2, 1, NSTEPS, NSTEPS, rows, hs, save, P, 1, 0, y0, &gt));
    long long info[4];
    CHECK(ctx, p_midyn_gentable_info(gt, info));
    const int first = NSTEPS / 3;
    CHECK(ctx, p_midyn_gentable_push(gt, 0, first, &G[0][0][0]));
    CHECK(ctx, p_midyn_gentable_push(gt, first, NSTEPS - first, &G[first][0][0]));
    midyn_complex Y[P][2];
    CHECK(ctx, p_midyn_gentable_finish(gt, &Y[0][0]));
    CHECK(ctx, p_midyn_gentable_destroy(gt));
    double err = 0.0;
    for (int p = 0; p < P; ++p) {
        const double t = p == 0 ? 0.0 : (p == 1 ? T / 2 : T);
        const midyn_complex e0 = cos(w * t), e1 = -I * sin(w * t);
        err = fmax(err, cabs(Y[p][0] - e0));
        err = fmax(err, cabs(Y[p][1] - e1));
    }
    CHECK(ctx, p_midyn_ctx_destroy(ctx));
    if (!(err <= 1e-12)) {
        fprintf(stderr, "max |y - closed form| = %.3e\n", err);
        return 20;
    }
    printf("GENTABLE_OK max|d|=%.2e steps_per_chunk=%lld route=%lld\n", err, info[0], info[3]);
    return 0;
}
