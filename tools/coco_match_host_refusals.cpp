// Stand-alone host check of the refusing paths of mu_coco_match (maskunet_amd/csrc/instances.hip): null pointers, the limits of
// mu_coco_match_supported, thresholds outside (0, 1], an area range with lo > hi, NaNs and a short workspace.  Every call returns before
// a launch, so it needs no GPU.  Meant for the host sanitizers (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         maskunet_amd/csrc/instances.hip tools/coco_match_host_refusals.cpp -o /tmp/coco_match_host_refusals && /tmp/coco_match_host_refusals
#include <cmath>
#include <cstdio>
#include "../include/maskunet_hip.h"
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Args {
    const int* in[8];
    void* out[13];
    void* ws;
    int B = 2, H = 16, W = 16, mp = 8, mg = 8, nc = 5, K = 8, max_dets = 100, T = 10, A = 4;
    long ws_bytes = 2 * 8 * 4;
    const double *thr, *rng;
};

static int run(const Args& a) {
    return mu_coco_match(a.in[0], a.in[1], a.in[2], (const float*)a.in[3], a.in[4], a.in[5], a.in[6], a.in[7], nullptr, nullptr, a.B, a.H,
                         a.W, a.mp, a.mg, a.nc, a.K, a.max_dets, a.thr, a.T, a.rng, a.A, (int*)a.out[0], (int*)a.out[1], (int*)a.out[2],
                         (float*)a.out[3], (int*)a.out[4], (double*)a.out[5], (unsigned char*)a.out[6], (int*)a.out[7], (int*)a.out[8],
                         (int*)a.out[9], (double*)a.out[10], (int*)a.out[11], (int*)a.out[12], a.ws, a.ws_bytes, nullptr);
}

int main() {
    static double fb[8];                                       // a non-null address: no call here reads or writes through it
    double thr[33], rng[5][2] = {{0, 1e10}, {0, 1024}, {1024, 9216}, {9216, 1e10}, {0, 1}};
    for (int t = 0; t < 33; ++t) thr[t] = 0.5 + 0.45 * t / 32.0;
    const int ARG = MU_ERR_ARG, SHAPE = MU_ERR_SHAPE, WS = MU_ERR_WORKSPACE;
    Args ok;
    for (auto& p : ok.in) p = (const int*)fb;
    for (auto& p : ok.out) p = fb;
    ok.ws = fb;
    ok.thr = thr;
    ok.rng = &rng[0][0];

    CHECK(mu_coco_match_supported(16, 16, 8, 8, 5, 8, 100, 10, 4) == MU_OK && mu_coco_match_supported(256, 256, 4096, 4096, 1024, 4096, 1, 32, 1) == MU_OK);
    CHECK(mu_coco_match_supported(16, 16, 8, 8, 5, 8, 100, 10, 0) == SHAPE && mu_coco_match_supported(16, 16, 8, 8, 5, 8, 100, 10, 5) == SHAPE);
    CHECK(mu_coco_match_supported(16, 16, 8, 8, 5, 8, 100, 33, 4) == SHAPE && mu_coco_match_supported(16, 16, 8, 8, 5, 8, 100, 0, 4) == SHAPE);
    CHECK(mu_coco_match_supported(257, 256, 8, 8, 5, 8, 100, 10, 4) == SHAPE && mu_coco_match_supported(16, 16, 4097, 8, 5, 8, 100, 10, 4) == SHAPE);
    CHECK(mu_coco_match_supported(16, 16, 8, 0, 5, 8, 100, 10, 4) == SHAPE && mu_coco_match_supported(16, 16, 8, 8, 1025, 8, 100, 10, 4) == SHAPE);
    CHECK(mu_coco_match_supported(16, 16, 8, 8, 5, 9, 100, 10, 4) == SHAPE && mu_coco_match_supported(16, 16, 8, 8, 5, 8, 0, 10, 4) == SHAPE);
    CHECK(mu_coco_match_workspace_bytes(2, 8) == 64 && mu_coco_match_workspace_bytes(0, 8) == 0 && mu_coco_match_workspace_bytes(2, 4097) == 0);

    for (int i = 0; i < 8; ++i) {                              // every required pointer
        Args a = ok;
        a.in[i] = nullptr;
        CHECK(run(a) == ARG);
    }
    for (int i = 0; i < 13; ++i) {
        Args a = ok;
        a.out[i] = nullptr;
        CHECK(run(a) == ARG);
    }
    Args a = ok;
    a.ws = nullptr;
    CHECK(run(a) == ARG);
    a = ok, a.thr = nullptr;
    CHECK(run(a) == ARG);
    a = ok, a.rng = nullptr;
    CHECK(run(a) == ARG);
    a = ok, a.B = 0;
    CHECK(run(a) == ARG);
    a = ok, a.A = 5;
    CHECK(run(a) == SHAPE);
    a = ok, a.T = 33;
    CHECK(run(a) == SHAPE);
    a = ok, a.K = 9;
    CHECK(run(a) == SHAPE);
    a = ok, a.nc = 1025;
    CHECK(run(a) == SHAPE);
    const double bad_thr[4] = {0.0, -0.5, 1.5, NAN};
    for (double v : bad_thr) {
        double t2[10];
        for (int t = 0; t < 10; ++t) t2[t] = thr[t];
        t2[9] = v;
        a = ok, a.thr = t2;
        CHECK(run(a) == ARG);
    }
    const double bad_rng[3][2] = {{9.0, 4.0}, {NAN, 4.0}, {0.0, NAN}};
    for (auto& r : bad_rng) {
        double r2[4][2];
        for (int i = 0; i < 4; ++i) r2[i][0] = rng[i][0], r2[i][1] = rng[i][1];
        r2[3][0] = r[0], r2[3][1] = r[1];
        a = ok, a.rng = &r2[0][0];
        CHECK(run(a) == ARG);
    }
    a = ok, a.ws_bytes = 63;
    CHECK(run(a) == WS);
    printf("mu_coco_match host refusals OK\n");
    return 0;
}
