// SURVEY 8-f4, the cv2 half for RAGGED batches: the sample preparation of the loaders that read with OpenCV (ADE20K semantic / panoptic,
// Cityscapes semantic / instance / panoptic, COCO semantic / panoptic) -- cv2.resize(.., INTER_LINEAR) of images that each have a size of
// their own, cv2.resize(.., INTER_NEAREST) of 8 / 16 / 32-bit id maps with the Cityscapes clean-ups folded in, and the COCO panoptic target
// (rgb2id, the segments_info loop, two nearest resizes: coco_panoptic.py:70-89).  include/maskunet_hip.h holds the contracts; the index
// and coefficient rules are those of the uniform kernels (cv2_rule.h).  Built with -ffp-contract=off like every file that restates
// separately rounded fp64 operations.
//
// One launch each.  An image owns a contiguous slice of the grid (b = blockIdx.x / per_img, the layout of pil_resample_kernel), so its
// h, w, offset, scales and the 2x-shortcut decision are wave-uniform.  Per output pixel the work is a handful of byte loads: nothing is
// staged in LDS but the segment table of the panoptic kernel, which every workgroup loads once and binary-searches.
#include "common.h"
#include "cv2_rule.h"

namespace {

constexpr int CVR_THREADS = 256;
constexpr int CVR_PAN_PIX = 4;                             // output pixels per thread of the panoptic kernel: the table is loaded once per 1024
constexpr int CVR_MAX_SIDE = 16384;

// h, w as the device holds them and the byte range of image b inside the flat buffer.  An image is refused where its size leaves
// [1, max], its start is negative or not a multiple of `align`, or its slot is shorter than h * w * bpp bytes.
__device__ __forceinline__ bool cvr_image_ok(const long* __restrict__ offsets, const int* __restrict__ sizes, int b, int bpp, int align, int max_h,
                                             int max_w, int& h, int& w, long& off) {
    h = sizes[2 * b];
    w = sizes[2 * b + 1];
    off = offsets[b];
    if (h < 1 || h > max_h || w < 1 || w > max_w) return false;
    if (off < 0 || off % align) return false;
    return offsets[b + 1] - off >= (long)h * w * bpp;
}

// ---- images: INTER_LINEAR + BGR2RGB + ToTensor ------------------------------------------------------------------------------------
template <typename T, int C>
__global__ __launch_bounds__(CVR_THREADS) void cvr_linear_kernel(const uint8_t* __restrict__ src, const long* __restrict__ offsets,
                                                                 const int* __restrict__ sizes, int max_h, int max_w, int swap_rb,
                                                                 T* __restrict__ dst, uint8_t* __restrict__ u8_out, uint8_t* __restrict__ valid,
                                                                 int Hd, int Wd, int Cp, int per_img) {
    constexpr int N = Vec16<T>::N;
    const int b = blockIdx.x / per_img, slice = blockIdx.x - b * per_img;
    int Hs, Ws;
    long off;
    const bool ok = cvr_image_ok(offsets, sizes, b, C, 1, max_h, max_w, Hs, Ws, off);
    if (slice == 0 && threadIdx.x == 0) valid[b] = ok ? 1 : 0;
    const int p = slice * CVR_THREADS + threadIdx.x;
    if (p >= Hd * Wd) return;
    const int dy = p / Wd, dx = p - dy * Wd;
    int v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    if (ok) {                                                // block-uniform
        const uint8_t* img = src + off;
        if (Ws == 2 * Wd && Hs == 2 * Hd) {                  // cv::resize's INTER_AREA shortcut, decided per image
            const uint8_t* p0 = img + ((long)(2 * dy) * Ws + 2 * dx) * C;
            const uint8_t* p1 = p0 + (long)Ws * C;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = ((int)p0[c] + (int)p0[C + c] + (int)p1[c] + (int)p1[C + c] + 2) >> 2;
        } else {
            const double scale_x = cv_scale(Wd, Ws), scale_y = cv_scale(Hd, Hs);
            int sx, a0, a1, sy, b0, b1;
            cv_lin_coef(dx, scale_x, Ws, true, sx, a0, a1);
            cv_lin_coef(dy, scale_y, Hs, false, sy, b0, b1);
            const int sx1 = sx + 1 < Ws ? sx + 1 : Ws - 1;       // weight 0 there at the right edge
            const int r0 = sy < 0 ? 0 : (sy < Hs ? sy : Hs - 1), r1 = sy + 1 < 0 ? 0 : (sy + 1 < Hs ? sy + 1 : Hs - 1);
            const uint8_t *q00 = img + ((long)r0 * Ws + sx) * C, *q01 = img + ((long)r0 * Ws + sx1) * C;
            const uint8_t *q10 = img + ((long)r1 * Ws + sx) * C, *q11 = img + ((long)r1 * Ws + sx1) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int d0 = (int)q00[c] * a0 + (int)q01[c] * a1, d1 = (int)q10[c] * a0 + (int)q11[c] * a1;
                v[c] = ((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2) & 0xFF;
            }
        }
        if (swap_rb && C == 3) { const int t = v[0]; v[0] = v[C - 1]; v[C - 1] = t; }
    }
    const long idx = (long)b * Hd * Wd + p;
    if (u8_out) {
#pragma unroll
        for (int c = 0; c < C; ++c) u8_out[idx * C + c] = (uint8_t)v[c];
    }
    for (int c0 = 0; c0 < Cp; c0 += N) {
        Vec16<T> o;
        o.zero();
        if (c0 == 0) {                                       // C <= 3 < N: the image channels sit in the first vector
#pragma unroll
            for (int c = 0; c < C; ++c) o.set(c, mu_u8_unit(v[c]));
        }
        o.store(dst + idx * Cp + c0);
    }
}

// ---- id maps: INTER_NEAREST of 8 / 16 / 32-bit and RGB-coded maps, floor division, class clean-up ------------------------------------
template <int KIND> struct MapKind;
template <> struct MapKind<MU_MAP_U8> { static constexpr int BPP = 1, ALIGN = 1; };
template <> struct MapKind<MU_MAP_U16> { static constexpr int BPP = 2, ALIGN = 2; };
template <> struct MapKind<MU_MAP_I32> { static constexpr int BPP = 4, ALIGN = 4; };
template <> struct MapKind<MU_MAP_RGB8> { static constexpr int BPP = 3, ALIGN = 1; };
template <> struct MapKind<MU_MAP_BGR8> { static constexpr int BPP = 3, ALIGN = 1; };

template <int KIND>
__device__ __forceinline__ long cvr_map_value(const uint8_t* __restrict__ img, long pix) {
    if (KIND == MU_MAP_U8) return (long)img[pix];
    if (KIND == MU_MAP_U16) return (long)reinterpret_cast<const uint16_t*>(img)[pix];
    if (KIND == MU_MAP_I32) return (long)reinterpret_cast<const int*>(img)[pix];
    const uint8_t* q = img + 3 * pix;                        // rgb2id: R + 256 G + 65536 B
    const long c0 = q[0], c1 = q[1], c2 = q[2];
    return KIND == MU_MAP_RGB8 ? c0 + 256 * c1 + 65536 * c2 : c2 + 256 * c1 + 65536 * c0;
}

template <int KIND>
__global__ __launch_bounds__(CVR_THREADS) void cvr_nearest_kernel(const uint8_t* __restrict__ src, const long* __restrict__ offsets,
                                                                  const int* __restrict__ sizes, int max_h, int max_w, int divisor, int n_classes,
                                                                  long fill, long* __restrict__ dst, uint8_t* __restrict__ valid, int Hd, int Wd,
                                                                  int per_img) {
    const int b = blockIdx.x / per_img, slice = blockIdx.x - b * per_img;
    int Hs, Ws;
    long off;
    const bool ok = cvr_image_ok(offsets, sizes, b, MapKind<KIND>::BPP, MapKind<KIND>::ALIGN, max_h, max_w, Hs, Ws, off);
    if (slice == 0 && threadIdx.x == 0) valid[b] = ok ? 1 : 0;
    const int p = slice * CVR_THREADS + threadIdx.x;
    if (p >= Hd * Wd) return;
    long v = fill;
    if (ok) {
        const int dy = p / Wd, dx = p - dy * Wd;
        const int sx = cv_nearest_index(dx, cv_scale(Wd, Ws), Ws), sy = cv_nearest_index(dy, cv_scale(Hd, Hs), Hs);
        v = cvr_map_value<KIND>(src + off, (long)sy * Ws + sx);
        if (divisor > 1) {                                   // Python's //: toward minus infinity
            const long q = v / divisor;
            v = (v % divisor != 0 && v < 0) ? q - 1 : q;
        }
        if (n_classes > 0 && (v < 0 || v >= n_classes)) v = fill;
    }
    dst[(long)b * Hd * Wd + p] = v;
}

// ---- COCO panoptic targets: rgb2id of the nearest-sampled PNG pixel, looked up in the image's sorted segment table ---------------------
__global__ __launch_bounds__(CVR_THREADS) void cvr_panoptic_kernel(const uint8_t* __restrict__ png, const long* __restrict__ offsets,
                                                                   const int* __restrict__ sizes, const int* __restrict__ seg_ids,
                                                                   const int* __restrict__ seg_labels, const int* __restrict__ img_seg_offsets,
                                                                   int S, int max_h, int max_w, int swap_rb, long fill,
                                                                   long* __restrict__ semantic, long* __restrict__ instance,
                                                                   uint8_t* __restrict__ valid, int Hd, int Wd, int per_img) {
    __shared__ int ids[MU_PANOPTIC_SEG_MAX], labels[MU_PANOPTIC_SEG_MAX];
    const int t = threadIdx.x;
    const int b = blockIdx.x / per_img, slice = blockIdx.x - b * per_img;
    int Hs, Ws;
    long off;
    bool ok = cvr_image_ok(offsets, sizes, b, 3, 1, max_h, max_w, Hs, Ws, off);
    const int s0 = img_seg_offsets[b], s1 = img_seg_offsets[b + 1];
    ok = ok && s0 >= 0 && s0 <= s1 && s1 <= S && s1 - s0 <= MU_PANOPTIC_SEG_MAX;
    const int n = ok ? s1 - s0 : 0;                          // block-uniform, like everything above
    int unsorted = 0;
    for (int i = t; i < n; i += CVR_THREADS) {
        const int id = seg_ids[s0 + i];
        ids[i] = id;
        labels[i] = seg_labels[s0 + i];
        if (i > 0 && seg_ids[s0 + i - 1] >= id) unsorted = 1;
    }
    ok = !__syncthreads_or(unsorted) && ok;                  // the barrier also publishes the table
    if (slice == 0 && t == 0) valid[b] = ok ? 1 : 0;
    const uint8_t* img = png + (ok ? off : 0);
    const double ifx = ok ? cv_scale(Wd, Ws) : 0.0, ify = ok ? cv_scale(Hd, Hs) : 0.0;
#pragma unroll
    for (int k = 0; k < CVR_PAN_PIX; ++k) {
        const int p = (slice * CVR_PAN_PIX + k) * CVR_THREADS + t;
        if (p >= Hd * Wd) break;
        long sem = fill, inst = 0;
        if (ok) {
            const int dy = p / Wd, dx = p - dy * Wd;
            const int sx = cv_nearest_index(dx, ifx, Ws), sy = cv_nearest_index(dy, ify, Hs);
            const long pix = (long)sy * Ws + sx;
            const int id = (int)(swap_rb ? cvr_map_value<MU_MAP_BGR8>(img, pix) : cvr_map_value<MU_MAP_RGB8>(img, pix));
            int lo = 0, hi = n;                              // lower bound of id in ids[0, n)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ids[mid] < id) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < n && ids[lo] == id;
            sem = hit ? (long)labels[lo] : 0;
            inst = hit ? (long)id : 0;
        }
        const long idx = (long)b * Hd * Wd + p;
        semantic[idx] = sem;
        instance[idx] = inst;
    }
}

// blocks of one image at `pix_per_block` output pixels each; the whole grid must fit blockIdx.x
inline bool cvr_grid(int B, int Hd, int Wd, int pix_per_block, int& per_img, long& blocks) {
    per_img = mu_cdiv((long)Hd * Wd, pix_per_block);
    blocks = (long)B * per_img;
    return blocks <= 0x7fffffffL;
}

}  // namespace

extern "C" int mu_cv2_ragged_supported(int B, int max_h, int max_w, int Hd, int Wd) {
    if (B < 1 || max_h < 1 || max_w < 1 || Hd < 1 || Wd < 1) return MU_ERR_SHAPE;
    if (max_h > CVR_MAX_SIDE || max_w > CVR_MAX_SIDE || Hd > CVR_MAX_SIDE || Wd > CVR_MAX_SIDE) return MU_ERR_SHAPE;
    int per_img;
    long blocks;
    return cvr_grid(B, Hd, Wd, CVR_THREADS, per_img, blocks) ? MU_OK : MU_ERR_SHAPE;
}

extern "C" int mu_cv2_resize_ragged_u8_nhwc(const unsigned char* src, const long* offsets, const int* sizes, int B, int C, int max_h, int max_w,
                                            int swap_rb, void* dst, unsigned char* u8_out, unsigned char* valid, int Hd, int Wd, int Cp,
                                            int dtype, void* stream) {
    if (!src || !offsets || !sizes || !dst || !valid || B < 1 || (dtype != MU_F32 && dtype != MU_F16)) return MU_ERR_ARG;
    if ((C != 1 && C != 3) || Cp < C || Cp % 8 || mu_cv2_ragged_supported(B, max_h, max_w, Hd, Wd) != MU_OK) return MU_ERR_SHAPE;
    int per_img;
    long blocks;
    cvr_grid(B, Hd, Wd, CVR_THREADS, per_img, blocks);
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto tag, auto channels) -> int {
        using T = decltype(tag);
        constexpr int CC = decltype(channels)::value;
        cvr_linear_kernel<T, CC><<<(unsigned)blocks, CVR_THREADS, 0, st>>>(src, offsets, sizes, max_h, max_w, swap_rb, (T*)dst, u8_out, valid, Hd, Wd,
                                                                          Cp, per_img);
        MU_CHECK_LAUNCH();
        return MU_OK;
    };
    return with_storage(dtype, [&](auto tag) -> int {
        return C == 1 ? launch(tag, std::integral_constant<int, 1>{}) : launch(tag, std::integral_constant<int, 3>{});
    });
}

extern "C" int mu_cv2_nearest_ragged(const void* src, const long* offsets, const int* sizes, int kind, int B, int max_h, int max_w, int divisor,
                                     int n_classes, long fill, long* dst, unsigned char* valid, int Hd, int Wd, void* stream) {
    if (!src || !offsets || !sizes || !dst || !valid || B < 1 || divisor < 1 || n_classes < 0) return MU_ERR_ARG;
    if (kind != MU_MAP_U8 && kind != MU_MAP_U16 && kind != MU_MAP_I32 && kind != MU_MAP_RGB8 && kind != MU_MAP_BGR8) return MU_ERR_ARG;
    const int align = kind == MU_MAP_U16 ? 2 : (kind == MU_MAP_I32 ? 4 : 1);
    if ((uintptr_t)src % align) return MU_ERR_ARG;           // the offsets are relative to src: both must be element-aligned
    if (mu_cv2_ragged_supported(B, max_h, max_w, Hd, Wd) != MU_OK) return MU_ERR_SHAPE;
    int per_img;
    long blocks;
    cvr_grid(B, Hd, Wd, CVR_THREADS, per_img, blocks);
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto k) -> int {
        constexpr int KIND = decltype(k)::value;
        cvr_nearest_kernel<KIND><<<(unsigned)blocks, CVR_THREADS, 0, st>>>((const uint8_t*)src, offsets, sizes, max_h, max_w, divisor, n_classes, fill,
                                                                          dst, valid, Hd, Wd, per_img);
        MU_CHECK_LAUNCH();
        return MU_OK;
    };
    switch (kind) {
        case MU_MAP_U8: return launch(std::integral_constant<int, MU_MAP_U8>{});
        case MU_MAP_U16: return launch(std::integral_constant<int, MU_MAP_U16>{});
        case MU_MAP_I32: return launch(std::integral_constant<int, MU_MAP_I32>{});
        case MU_MAP_RGB8: return launch(std::integral_constant<int, MU_MAP_RGB8>{});
        default: return launch(std::integral_constant<int, MU_MAP_BGR8>{});
    }
}

extern "C" int mu_panoptic_targets(const unsigned char* png, const long* offsets, const int* sizes, const int* seg_ids, const int* seg_labels,
                                   const int* img_seg_offsets, int B, int S, int max_h, int max_w, int swap_rb, long fill, long* semantic,
                                   long* instance, unsigned char* valid, int Hd, int Wd, void* stream) {
    if (!png || !offsets || !sizes || !img_seg_offsets || !semantic || !instance || !valid || B < 1 || S < 0) return MU_ERR_ARG;
    if (S > 0 && (!seg_ids || !seg_labels)) return MU_ERR_ARG;
    if (mu_cv2_ragged_supported(B, max_h, max_w, Hd, Wd) != MU_OK) return MU_ERR_SHAPE;
    int per_img;
    long blocks;
    cvr_grid(B, Hd, Wd, CVR_THREADS * CVR_PAN_PIX, per_img, blocks);
    cvr_panoptic_kernel<<<(unsigned)blocks, CVR_THREADS, 0, (hipStream_t)stream>>>(png, offsets, sizes, seg_ids, seg_labels, img_seg_offsets, S, max_h,
                                                                                  max_w, swap_rb, fill, semantic, instance, valid, Hd, Wd, per_img);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
