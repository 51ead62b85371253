// The restated OpenCV 4.10 index and coefficient rules of cv2.resize for 8-bit images (modules/imgproc/src/resize.cpp), shared by the uniform
// kernels of elementwise.hip and the ragged ones of cv2_ragged.hip: one piece of code, so the two cannot drift apart.
#pragma once
#include "common.h"

// what cv::resize derives from dsize: inv_scale = dsize / ssize, scale = 1 / inv_scale -- two separately rounded fp64 operations
__host__ __device__ __forceinline__ double cv_scale(int dn, int sn) { return 1.0 / ((double)dn / (double)sn); }

// INTER_LINEAR, CV_8U: first source index and the two 11-bit fixed-point coefficients of destination index d
__device__ __forceinline__ void cv_lin_coef(int d, double scale, int sn, bool clamp_taps, int& s, int& c0, int& c1) {
    // two separately rounded double operations, as the host code this restates runs them: no fused multiply-add contraction (HIP's
    // __dmul_rn / __dadd_rn are plain operators and would contract)
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int si = (int)floorf(f);
    f -= (float)si;
    if (clamp_taps) {
        if (si < 0) { f = 0.f; si = 0; }
        if (si + 1 >= sn) { f = 0.f; si = sn - 1; }
    }
    s = si;
    c0 = __float2int_rn((1.0f - f) * 2048.0f);               // cvRound: round half to even
    c1 = __float2int_rn(f * 2048.0f);
}

// INTER_NEAREST: source index min(floor(d * scale), n - 1), no half-pixel offset
__device__ __forceinline__ int cv_nearest_index(int d, double scale, int sn) {
    const int s = (int)floor((double)d * scale);
    return s < sn - 1 ? s : sn - 1;
}
