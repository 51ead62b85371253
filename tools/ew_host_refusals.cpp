// Stand-alone host check of the refusing paths of maskunet_amd/csrc/elementwise.hip and of the cross-entropy / IoU part of
// maskunet_amd/csrc/loss.hip: null pointers, MU_F32X where it is not taken, an unknown dtype, a partial vector, a short workspace and
// the two MU_F32X shape refusals of mu_prep_weight.  Every call returns before a launch, so it needs no GPU (mu_mean_iou clears its
// counts before it reads the dtype, so only its argument refusals are here).  Meant for the host sanitizers (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         maskunet_amd/csrc/elementwise.hip maskunet_amd/csrc/loss.hip tools/ew_host_refusals.cpp -o /tmp/ew_host_refusals && /tmp/ew_host_refusals
#include <cstdio>
#include "../include/maskunet_hip.h"
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    static float fb[64];                                       // a non-null address: no call here reads or writes through it
    void* b = fb;
    const float* w = fb;
    const long* lab = (const long*)fb;
    unsigned char* u8 = (unsigned char*)fb;
    const int ARG = MU_ERR_ARG, SHAPE = MU_ERR_SHAPE, WS = MU_ERR_WORKSPACE;
    const int bad[2] = {MU_F32X, 99};
    for (int d : bad) {
        CHECK(mu_transpose_pad(b, d, 4, b, MU_F32, 4, 1, 1, 4, 4, nullptr) == ARG && mu_transpose_pad(b, MU_F16, 5, b, d, 3, 1, 3, 5, 3, nullptr) == ARG);
        CHECK(mu_transpose(b, d, 4, b, d, 4, 1, 1, 4, nullptr) == ARG);
        CHECK(mu_cast(b, d, b, MU_F16, 4, nullptr) == ARG && mu_cast(b, MU_F32, b, d, 15, nullptr) == ARG);
        CHECK(mu_maxpool2_fwd(b, b, 1, 2, 2, 8, d, nullptr) == ARG);
        CHECK(mu_maxpool2_bwd(b, b, b, 1, 2, 2, 8, d, nullptr) == ARG && mu_maxpool2_bwd_acc(b, b, b, b, b, 1, 3, 3, 8, d, nullptr) == ARG);
        CHECK(mu_upcat_fwd(b, b, b, 1, 1, 1, 8, 8, d, nullptr) == ARG);
        CHECK(mu_upcat_bwd(b, b, b, 1, 1, 1, 8, 8, d, nullptr) == ARG && mu_upcat_bwd_acc(b, b, b, b, 1, 1, 1, 8, 8, d, nullptr) == ARG);
        CHECK(mu_upcat_compact_fwd(b, b, b, 1, 1, 1, 8, 3, 8, 5, 8, d, nullptr) == ARG);
        CHECK(mu_upcat_compact_bwd(b, b, b, 1, 1, 1, 8, 3, 8, 5, 8, d, nullptr) == ARG);
        CHECK(mu_upcat_compact_fwd(b, b, b, 1, 1, 1, 8, 9, 8, 5, 8, d, nullptr) == SHAPE);      // the channel counts are looked at first
        CHECK(mu_dropout(b, b, 8, 0.3f, 1, nullptr, nullptr, d, nullptr) == ARG && mu_dropout_step(b, b, 8, 0.3f, 1, nullptr, nullptr, nullptr, d, nullptr) == ARG);
        CHECK(mu_dropout(b, b, 3, 0.3f, 1, nullptr, nullptr, d, nullptr) == ARG);               // unknown dtype before the partial vector
        CHECK(mu_add(b, b, b, 8, d, nullptr) == ARG && mu_add(b, b, b, 3, d, nullptr) == ARG && mu_add(nullptr, b, b, 3, d, nullptr) == ARG);
        CHECK(mu_u8_to_nhwc(u8, b, 1, 3, 8, d, nullptr) == ARG);
        CHECK(mu_prep_qkv(w, w, w, w, w, w, b, fb, d, 32, nullptr) == ARG);
        CHECK(mu_resize_u8_nhwc(u8, 1, 2, 2, 3, 0, b, u8, 1, 1, 8, d, nullptr) == ARG);
        CHECK(mu_resize_u8_nhwc(u8, 1, 2, 2, 5, 0, b, u8, 1, 1, 8, d, nullptr) == SHAPE);
        const long ws = mu_ce_workspace_bytes();
        CHECK(mu_ce_fwd(b, lab, 1, 8, 2, -100, fb, fb, fb, b, ws, d, nullptr) == ARG && mu_ce_fwd(b, lab, 1, 8, 2, -100, fb, fb, fb, b, ws - 1, d, nullptr) == WS);
        CHECK(mu_ce_bwd(b, lab, fb, fb, fb, 1.f, 1, 8, 2, -100, b, d, nullptr) == ARG);
        for (long HW = 3; HW <= 4; ++HW) {
            CHECK(mu_ce_nchw_fwd(b, lab, 1, 2, HW, -100, fb, fb, fb, b, ws, d, nullptr) == ARG);
            CHECK(mu_ce_nchw_fwd(b, lab, 1, 2, HW, -100, fb, fb, fb, b, ws - 1, d, nullptr) == WS);
            CHECK(mu_ce_nchw_bwd(b, lab, fb, fb, fb, 1.f, 1, 2, HW, -100, b, d, nullptr) == ARG);
        }
    }
    CHECK(mu_prep_weight(w, b, 99, 4, 4, 9, 4, 4, 0, nullptr) == ARG && mu_prep_weights_multi(b, 1, 1, b, 99, nullptr) == ARG);
    for (int dt = MU_F32; dt <= MU_F32X; ++dt) {               // the argument refusals do not depend on the dtype
        CHECK(mu_prep_weight(nullptr, b, dt, 4, 4, 9, 4, 4, 0, nullptr) == ARG && mu_prep_weight(w, b, dt, 4, 4, 4, 4, 4, 0, nullptr) == ARG);
        CHECK(mu_prep_weight(w, b, dt, 4, 4, 9, 4, 4, 3, nullptr) == ARG && mu_prep_weight(w, b, dt, 8, 4, 9, 4, 4, 0, nullptr) == ARG);
        CHECK(mu_add(b, b, b, 0, dt, nullptr) == ARG && mu_dropout(b, b, 8, 1.0f, 1, nullptr, nullptr, dt, nullptr) == ARG);
        CHECK(mu_maxpool2_fwd(b, nullptr, 1, 2, 2, 8, dt, nullptr) == ARG && mu_maxpool2_fwd(b, b, 1, 1, 2, 8, dt, nullptr) == ARG);
        CHECK(mu_upcat_fwd(b, b, b, 1, 1, 1, 8, 4, dt, nullptr) == ARG && mu_upcat_bwd(b, nullptr, b, 1, 1, 1, 8, 8, dt, nullptr) == ARG);
        CHECK(mu_transpose_pad(b, dt, 3, b, dt, 4, 1, 1, 4, 4, nullptr) == ARG && mu_cast(b, dt, nullptr, dt, 4, nullptr) == ARG);
        CHECK(mu_mean_iou(nullptr, lab, 1, 2, 1, 0, 1, 8, 1e-6f, (unsigned int*)fb, fb, dt, nullptr) == ARG);
        CHECK(mu_mean_iou(b, lab, 1, 4097, 1, 0, 1, 8, 1e-6f, (unsigned int*)fb, fb, dt, nullptr) == ARG);
    }
    for (int dt = MU_F32; dt <= MU_F16; ++dt) {                // a partial vector: four floats or eight halves
        CHECK(mu_add(b, b, b, dt == MU_F32 ? 6 : 12, dt, nullptr) == SHAPE);
        CHECK(mu_dropout_step(b, b, dt == MU_F32 ? 3 : 7, 0.3f, 1, nullptr, nullptr, nullptr, dt, nullptr) == SHAPE);
    }
    // MU_F32X: rows_pad / cols_pad no multiple of four, a data-gradient row longer than 8192 (9 taps only): refused before the launch
    CHECK(mu_prep_weight(w, b, MU_F32X, 4, 4, 9, 6, 4, 0, nullptr) == SHAPE && mu_prep_weight(w, b, MU_F32X, 4, 4, 9, 4, 6, 0, nullptr) == SHAPE);
    CHECK(mu_prep_weight(w, b, MU_F32X, 4, 4, 1, 6, 6, 2, nullptr) == SHAPE);
    CHECK(mu_prep_weight(w, b, MU_F32X, 1, 1, 9, 4, 8196, 1, nullptr) == SHAPE && mu_prep_weight(w, b, MU_F32X, 1, 1, 9, 8196, 4, 2, nullptr) == SHAPE);
    printf("elementwise / loss host refusals OK\n");
    return 0;
}
