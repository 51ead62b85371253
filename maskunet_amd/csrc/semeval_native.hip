// Semantic evaluation at the labels' OWN resolution (contract: include/maskunet_hip.h, mu_sem_eval_native): the logits of a batch are
// upsampled bilinearly (torch's upsample_bilinear2d(align_corners=False) formula, every fp32 operation rounded on its own) to the size of
// each image's label map, the first arg-max is taken and counted against the labels -- without the upsampled logits ever existing.  The
// labels are a ragged uint8 batch as mu_pil_resize_u8_nhwc takes one.  Built with -ffp-contract=off: no FMA anywhere in this file.
//
//   sem_native_prepare_kernel  zeroes img_counts; one thread per image validates it, writes valid[b] and the image's descriptor
//                              (offset, size, the two scale quotients) into the workspace.
//   sem_native_kernel          one workgroup per (image, tile of SN_TH x SN_TW label pixels); the grid is sized by the bounds max_h, max_w
//                              and a tile outside its image (or of a refused image) leaves at once.  The source window of the tile --
//                              rows y0(first row) .. y1(last row), columns likewise; the taps are monotone in the output index -- is
//                              staged in LDS as fp32, channel-major with an odd plane stride (a wave's lanes run along X, so at a
//                              fixed channel they read consecutive words; the staging stores of consecutive channels fall on
//                              different banks).  A lane owns one pixel (SN_THREADS = SN_TH * SN_TW: the counters of 150 classes
//                              and the window leave room for ONE workgroup per CU, which then still has 4 waves per SIMD; measured
//                              against 256 threads and 4 rows per lane: 0.49 ms instead of 0.76 ms at 150 classes, 0.36 ms instead of
//                              0.34 ms at 19), keeps the four tap offsets and weights
//                              in registers and walks the channels with a running maximum.  A window larger than the LDS share
//                              (strong downscaling, large C x window) is not staged: the same taps are then read from global memory
//                              (L2) and enter the same arithmetic, so both paths give the same bits.  Label and class-map bytes are
//                              read and written along X, one byte per lane: image starts need no alignment.
//                              Counters: [3][C] per block in LDS; the (C+1) x C confusion counters too where they fit beside the
//                              window, two 16-bit counters per LDS word (a tile has SN_TH * SN_TW < 2^16 pixels, so a half never
//                              carries into its neighbour), else one 64-bit global atomic per pixel.  Integer atomics only.
#include "common.h"

namespace {

constexpr int SN_TH = MU_SEM_NATIVE_TILE_H;
constexpr int SN_TW = MU_SEM_NATIVE_TILE_W;
constexpr int SN_THREADS = 1024;
constexpr int SN_ROWS = SN_TH / (SN_THREADS / SN_TW);        // rows of the tile per lane
constexpr long SN_WIN_FLOATS = MU_SEM_NATIVE_WINDOW_BYTES / 4;
constexpr long SN_LDS_BYTES = MU_SEM_NATIVE_LDS_BYTES;
static_assert(SN_TW == 64 && SN_THREADS % SN_TW == 0 && SN_TH % (SN_THREADS / SN_TW) == 0, "a wave is one row of the tile");
static_assert(SN_TH * SN_TW < 65536, "two 16-bit confusion counters share an LDS word");
static_assert(SN_LDS_BYTES <= 160 * 1024, "the LDS of a CU");

struct NativeImage {                     // the workspace: one per image
    long off;                            // byte offset of the label map (and of the class map)
    int H, W;                            // 0, 0 for a refused image
    float sy, sx;                        // fp32(h) / fp32(H), fp32(w) / fp32(W)
    int pad[2];
};
static_assert(sizeof(NativeImage) == 32, "workspace layout");

struct NativeParams {
    const void* logits;
    const unsigned char* labels;
    const NativeImage* images;
    int C, h, w;
    long HW, M, inner, outer, cs, ps;
    long ignore;
    int* img_counts;
    unsigned long long* confusion;
    unsigned char* classes;
    int tiles_x, tiles_per_image;
    int win_floats;                      // the LDS share of the source window, in floats
    int lds_conf;                        // the confusion counters of a block live in LDS
};

// what the host can say about the LDS of a launch: the window share is the whole source where that is smaller than the cap
struct NativeLds { long win_floats, conf_words, bytes; bool lds_conf; };
inline NativeLds native_lds(int C, int h, int w) {
    NativeLds l;
    const long whole = (long)C * (((long)h * w) | 1);
    l.win_floats = whole < SN_WIN_FLOATS ? whole : SN_WIN_FLOATS;
    l.conf_words = ((long)(C + 1) * C + 1) / 2;
    l.lds_conf = (3L * C + l.conf_words + l.win_floats) * 4 <= SN_LDS_BYTES;
    l.bytes = (3L * C + (l.lds_conf ? l.conf_words : 0) + l.win_floats) * 4;
    return l;
}

// One axis of the contract: output index i of an axis scaled by s = fp32(n_in) / fp32(n_out) -> taps i0, i1 and the weight of i1.
// Every operation is one rounded fp32 operation, in the contract's order; monotone in i.
__device__ __forceinline__ void native_taps(float s, int i, int n_in, int& i0, int& i1, float& l1) {
    const float f = fmaxf(s * ((float)i + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)f, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = f - (float)i0;
}

// offset of source pixel p = y * w + x of image b, i.e. of row r = b * HW + p in the addressing of mu_sem_eval: the two layouts a module
// output has are division-free
__device__ __forceinline__ long native_pixel_offset(const NativeParams& P, long b, long p) {
    if (P.inner >= P.M) return (b * P.HW + p) * P.ps;                       // NHWC rows: one outer block
    if (P.inner == P.HW) return b * P.outer + p * P.ps;                     // NCHW: one outer block per image
    const long r = b * P.HW + p;
    return (r / P.inner) * P.outer + (r % P.inner) * P.ps;
}

__global__ __launch_bounds__(256) void sem_native_prepare_kernel(const long* __restrict__ offsets, const int* __restrict__ sizes, int B, int h,
                                                                 int w, int max_h, int max_w, NativeImage* __restrict__ images,
                                                                 unsigned char* __restrict__ valid, int* __restrict__ img_counts, long n_counts) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    for (long i = t; i < n_counts; i += step) img_counts[i] = 0;
    for (long b = t; b < B; b += step) {
        const int H = sizes[2 * b], W = sizes[2 * b + 1];
        const long off = offsets[b];
        const bool ok = H >= 1 && H <= max_h && W >= 1 && W <= max_w && off >= 0 && offsets[b + 1] - off >= (long)H * W;
        NativeImage im;
        im.off = ok ? off : 0;
        im.H = ok ? H : 0;
        im.W = ok ? W : 0;
        im.sy = ok ? (float)h / (float)H : 0.f;
        im.sx = ok ? (float)w / (float)W : 0.f;
        im.pad[0] = im.pad[1] = 0;
        images[b] = im;
        valid[b] = ok ? 1 : 0;
    }
}

// the first maximum over the C real channels of the interpolated value; IN_LDS: taps from the staged window, else from global memory
template <typename T, bool IN_LDS, typename O>
__device__ __forceinline__ int native_argmax(const float* __restrict__ win, int plane, const T* __restrict__ g, long cs, int C,
                                             const O (&o)[4], float lx0, float lx1, float ly0, float ly1) {
    float best = -INFINITY;                                      // the logits are finite; a NaN (outside the contract) leaves class 0
    int arg = 0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        float a00, a01, a10, a11;
        if (IN_LDS) {
            const float* p = win + c * plane;
            a00 = p[o[0]]; a01 = p[o[1]]; a10 = p[o[2]]; a11 = p[o[3]];
        } else {
            const T* p = g + c * cs;
            a00 = (float)p[o[0]]; a01 = (float)p[o[1]]; a10 = (float)p[o[2]]; a11 = (float)p[o[3]];
        }
        const float v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11);
        if (v > best) { best = v; arg = c; }                     // ascending channels: the first maximum stays
    }
    return arg;
}

template <typename T>
__global__ __launch_bounds__(SN_THREADS) void sem_native_kernel(const NativeParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned sn_lds[];
    const int b = blockIdx.x / P.tiles_per_image, tile = blockIdx.x - b * P.tiles_per_image;
    const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const NativeImage im = P.images[b];
    const int Y0 = ty * SN_TH, X0 = tx * SN_TW;
    if (Y0 >= im.H || X0 >= im.W) return;                        // block-uniform: outside the image, or a refused image (H = W = 0)
    const int C = P.C, h = P.h, w = P.w, tid = threadIdx.x;
    const int nrows = min(SN_TH, im.H - Y0), ncols = min(SN_TW, im.W - X0);

    unsigned* hist = sn_lds;                                     // [3][C]: I, P, L of this tile
    const int conf_words = P.lds_conf ? ((C + 1) * C + 1) / 2 : 0;
    unsigned* conf = P.lds_conf ? sn_lds + 3 * C : nullptr;      // [(C + 1) * C] 16-bit counters, two per word
    float* win = reinterpret_cast<float*>(sn_lds + 3 * C + conf_words);
    for (int i = tid; i < 3 * C + conf_words; i += SN_THREADS) sn_lds[i] = 0;

    // the source window of the tile: the taps are monotone in the output index, so its corners bound every tap
    int ya, yb, xa, xb, unused;
    float unused_l;
    native_taps(im.sy, Y0, h, ya, unused, unused_l);
    native_taps(im.sy, Y0 + nrows - 1, h, unused, yb, unused_l);
    native_taps(im.sx, X0, w, xa, unused, unused_l);
    native_taps(im.sx, X0 + ncols - 1, w, unused, xb, unused_l);
    const int wy = yb - ya + 1, wx = xb - xa + 1, npix = wy * wx, plane = npix | 1;
    const bool in_lds = (long)plane * C <= (long)P.win_floats;
    const T* logits = (const T*)P.logits;
    if (in_lds) {
        const int total = npix * C;
        if (P.cs == 1) {                                         // NHWC rows: consecutive lanes take consecutive channels
            for (int i = tid; i < total; i += SN_THREADS) {
                const int pix = i / C, c = i - pix * C, yy = pix / wx, xx = pix - yy * wx;
                win[c * plane + pix] = (float)logits[native_pixel_offset(P, b, (long)(ya + yy) * w + xa + xx) + c];
            }
        } else {                                                 // NCHW and anything else: consecutive lanes along x
            for (int i = tid; i < total; i += SN_THREADS) {
                const int c = i / npix, pix = i - c * npix, yy = pix / wx, xx = pix - yy * wx;
                win[c * plane + pix] = (float)logits[native_pixel_offset(P, b, (long)(ya + yy) * w + xa + xx) + c * P.cs];
            }
        }
    }
    __syncthreads();                                             // the counters are zero, the window is staged

    const int lx = tid & (SN_TW - 1), X = X0 + lx;
    if (lx < ncols) {
        int x0, x1;
        float lx1;
        native_taps(im.sx, X, w, x0, x1, lx1);
        const float lx0 = 1.0f - lx1;
        const unsigned char* lab_img = P.labels + im.off;
#pragma unroll 1
        for (int k = 0; k < SN_ROWS; ++k) {
            const int ly = (tid >> 6) + k * (SN_THREADS / SN_TW);
            if (ly >= nrows) break;
            const int Y = Y0 + ly;
            int y0, y1;
            float ly1;
            native_taps(im.sy, Y, h, y0, y1, ly1);
            const float ly0 = 1.0f - ly1;
            int pred;
            if (in_lds) {
                const int o[4] = {(y0 - ya) * wx + (x0 - xa), (y0 - ya) * wx + (x1 - xa), (y1 - ya) * wx + (x0 - xa), (y1 - ya) * wx + (x1 - xa)};
                pred = native_argmax<T, true>(win, plane, (const T*)nullptr, 0, C, o, lx0, lx1, ly0, ly1);
            } else {
                const long o[4] = {native_pixel_offset(P, b, (long)y0 * w + x0), native_pixel_offset(P, b, (long)y0 * w + x1),
                                   native_pixel_offset(P, b, (long)y1 * w + x0), native_pixel_offset(P, b, (long)y1 * w + x1)};
                pred = native_argmax<T, false>(nullptr, 0, logits, P.cs, C, o, lx0, lx1, ly0, ly1);
            }
            const long at = (long)Y * im.W + X;
            const int lab = lab_img[at];
            const bool counted = (long)lab != P.ignore && lab < C;
            atomicAdd(&hist[C + pred], 1u);                      // P counts every pixel, void ones included
            if (counted) {
                atomicAdd(&hist[2 * C + lab], 1u);
                if (lab == pred) atomicAdd(&hist[pred], 1u);
            }
            const int cell = (counted ? lab : C) * C + pred;
            if (conf) atomicAdd(&conf[cell >> 1], 1u << ((cell & 1) * 16));
            else atomicAdd(&P.confusion[cell], 1ull);
            if (P.classes) P.classes[im.off + at] = (unsigned char)pred;
        }
    }
    __syncthreads();                                             // every LDS counter of the tile is final
    for (int i = tid; i < 3 * C; i += SN_THREADS)
        if (hist[i]) atomicAdd(&P.img_counts[(long)b * 3 * C + i], (int)hist[i]);
    if (conf) {
        const int cells = (C + 1) * C;
        for (int i = tid; i < conf_words; i += SN_THREADS) {
            const unsigned v = conf[i];
            if (v & 0xffffu) atomicAdd(&P.confusion[2 * i], (unsigned long long)(v & 0xffffu));
            if ((v >> 16) && 2 * i + 1 < cells) atomicAdd(&P.confusion[2 * i + 1], (unsigned long long)(v >> 16));
        }
    }
}

struct NativeWs {
    MuCarve c;
    NativeImage* images;        // [B] written by the prepare kernel, read by the sweep
    constexpr NativeWs(void* ws, int B) : c(ws), images(c.take<NativeImage>(B)) {}
};
static_assert(NativeWs(nullptr, 2).c.bytes == 64 && NativeWs(nullptr, 5).c.bytes == 160, "mu_sem_eval_native workspace");

}  // namespace

extern "C" int mu_sem_eval_native_supported(int C, int h, int w) {
    return C >= 1 && C <= 256 && h >= 1 && w >= 1 && (long)h * w <= 65536 ? MU_OK : MU_ERR_SHAPE;
}

extern "C" long mu_sem_eval_native_workspace_bytes(int B, int C, int h, int w, int max_h, int max_w) {
    if (B < 1 || max_h < 1 || max_w < 1 || max_h > 16384 || max_w > 16384 || mu_sem_eval_native_supported(C, h, w) != MU_OK) return 0;
    return NativeWs(nullptr, B).c.bytes;
}

extern "C" int mu_sem_eval_native(const void* logits, int B, int C, int h, int w, long inner, long outer_stride, long c_stride, long p_stride,
                                  const unsigned char* labels, const long* offsets, const int* sizes, int max_h, int max_w, long ignore_index,
                                  int* img_counts, long* confusion, unsigned char* valid, unsigned char* classes_or_null, void* workspace,
                                  long ws_bytes, int dtype, void* stream) {
    if (!logits || !labels || !offsets || !sizes || !img_counts || !confusion || !valid || !workspace) return MU_ERR_ARG;
    if (B < 1 || inner < 1 || max_h < 1 || max_w < 1 || max_h > 16384 || max_w > 16384 || ((uintptr_t)workspace & 7)) return MU_ERR_ARG;
    if (dtype != MU_F32 && dtype != MU_F16) return MU_ERR_ARG;
    if (mu_sem_eval_native_supported(C, h, w) != MU_OK) return MU_ERR_SHAPE;
    const int tiles_y = mu_cdiv(max_h, SN_TH), tiles_x = mu_cdiv(max_w, SN_TW);
    const long blocks = (long)B * tiles_y * tiles_x;
    if (blocks > 0x7fffffffL) return MU_ERR_SHAPE;
    if (ws_bytes < mu_sem_eval_native_workspace_bytes(B, C, h, w, max_h, max_w)) return MU_ERR_WORKSPACE;
    const NativeLds lds = native_lds(C, h, w);
    const NativeWs ws(workspace, B);
    hipStream_t st = (hipStream_t)stream;
    NativeParams P;
    P.logits = logits; P.labels = labels; P.images = ws.images;
    P.C = C; P.h = h; P.w = w;
    P.HW = (long)h * w; P.M = (long)B * P.HW; P.inner = inner; P.outer = outer_stride; P.cs = c_stride; P.ps = p_stride;
    P.ignore = ignore_index;
    P.img_counts = img_counts; P.confusion = (unsigned long long*)confusion; P.classes = classes_or_null;
    P.tiles_x = tiles_x; P.tiles_per_image = tiles_y * tiles_x;
    P.win_floats = (int)lds.win_floats; P.lds_conf = lds.lds_conf ? 1 : 0;
    const long n_counts = (long)B * 3 * C;
    return with_storage(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (lds.bytes > 48 * 1024 && !mu_lds_grant<sem_native_kernel<T>>((int)SN_LDS_BYTES)) return MU_ERR_LAUNCH;
        sem_native_prepare_kernel<<<mu_grid(n_counts > B ? n_counts : B, 256, 1024), 256, 0, st>>>(offsets, sizes, B, h, w, max_h, max_w, ws.images,
                                                                                                valid, img_counts, n_counts);
        MU_CHECK_LAUNCH();
        sem_native_kernel<T><<<(unsigned)blocks, SN_THREADS, (size_t)lds.bytes, st>>>(P);
        MU_CHECK_LAUNCH();
        return MU_OK;
    });
}
