// SURVEY 8-f4, the Pillow half: decoded image bytes of a RAGGED batch -> the network input, by Pillow's antialiased bilinear resample
// (Image.resize(.., BILINEAR), what T.ToPILImage() -> T.Resize((128, 128)) -> T.ToTensor() runs in coco_instance.py:43-47,68).
// include/maskunet_hip.h holds the contract; tests/_pil_reference.py restates it in numpy and tests/golden/pil/ pins it to Pillow's bytes.
// Built with -ffp-contract=off: the coefficient rule rounds every fp64 operation on its own.
//
//   pil_coeff_kernel     one thread per (image, axis, output index): xmin, n and the n 22-bit integer coefficients into the workspace
//                        (the only fp64 code; a few KB per image, read back through L2).  Thread 0 of an image writes valid[b].
//   pil_resample_kernel  one workgroup per (image, band of R output rows, 64 output columns); a thread owns one (column, channel) and
//                        R int32 accumulators.  The source rows ymin(first row) .. ymax(last row) stream through a double-buffered LDS
//                        tile of several row segments (16-byte loads from the 16-byte-aligned address below a segment's first byte; a
//                        chunk that crosses the image's first or last byte is assembled from byte loads).  Per source row a thread forms the horizontal
//                        result of its (column, channel) as a u8 -- over several tiles where the taps of 64 columns span more than
//                        one -- and adds k_y * u8 into those accumulators whose [ymin, ymin + n) holds the row: a fully unrolled,
//                        predicated loop, no dynamic register index.  No intermediate image, no limit on the scale factor.
#include "common.h"

namespace {

constexpr int PIL_R = 8;             // output rows per band
constexpr int PIL_COLS = 64;         // output columns per workgroup: 64 * C threads, whole waves for C = 1 and 3
constexpr int PIL_CHUNKS = 2;        // 16-byte chunks a thread stages per tile
constexpr int PIL_KCAP = 32;         // horizontal taps per column kept in LDS (scale <= 15); beyond that they are read through L2
constexpr int PIL_BITS = 22;

struct PilLayout {                   // the workspace of one image, in ints: [xmin Wd][n Wd][k Wd * ksx][ymin Hd][n Hd][k Hd * ksy]
    int ksx, ksy;
    long per_image;
};

// taps per output index that a source axis of at most n_in can need: 2 * ceil(max(n_in / n_out, 1)) + 1, in exact integer arithmetic
// (never below the fp64 ksize of the contract: ceil of the rounded quotient cannot exceed the ceil of the exact one)
__host__ __device__ inline int pil_ksize_bound(int n_in, int n_out) {
    const int s = n_in <= n_out ? 1 : (n_in + n_out - 1) / n_out;
    return 2 * s + 1;
}
__host__ __device__ inline PilLayout pil_layout(int max_h, int max_w, int Hd, int Wd) {
    PilLayout l;
    l.ksx = pil_ksize_bound(max_w, Wd);
    l.ksy = pil_ksize_bound(max_h, Hd);
    l.per_image = (long)Wd * (2 + l.ksx) + (long)Hd * (2 + l.ksy);
    return l;
}
// Wd * ksx <= 2 * (max_w + Wd) + Wd: an upper bound that grows with every argument (Wd * ceil(max_w / Wd) itself does not)
inline long pil_ws_ints(int max_h, int max_w, int Hd, int Wd) { return 5L * Wd + 2L * max_w + 5L * Hd + 2L * max_h; }

// h, w as the device holds them; the byte range of image b inside src.  An image is refused where its size leaves [1, max], it is taller
// than 100 widths and shrinks vertically (Pillow 12 resizes those vertically first), or its slot of src is shorter than h * w * C.
__device__ __forceinline__ bool pil_image_ok(const long* __restrict__ offsets, const int* __restrict__ sizes, int b, int C, int max_h, int max_w,
                                             int Hd, int& h, int& w, long& off) {
    h = sizes[2 * b];
    w = sizes[2 * b + 1];
    off = offsets[b];
    if (h < 1 || h > max_h || w < 1 || w > max_w) return false;
    if (h > 100 * w && Hd < h) return false;
    return off >= 0 && offsets[b + 1] - off >= (long)h * w * C;
}

__global__ __launch_bounds__(256) void pil_coeff_kernel(const long* __restrict__ offsets, const int* __restrict__ sizes, int B, int C, int max_h,
                                                        int max_w, int Hd, int Wd, int* __restrict__ ws, unsigned char* __restrict__ valid) {
    const PilLayout L = pil_layout(max_h, max_w, Hd, Wd);
    const long total = (long)B * (Wd + Hd);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx / (Wd + Hd)), j = (int)(idx % (Wd + Hd));
        int h, w;
        long off;
        const bool ok = pil_image_ok(offsets, sizes, b, C, max_h, max_w, Hd, h, w, off);
        if (j == 0) valid[b] = ok ? 1 : 0;
        const bool xaxis = j < Wd;
        const int xx = xaxis ? j : j - Wd, n_out = xaxis ? Wd : Hd, n_in = xaxis ? w : h, ks = xaxis ? L.ksx : L.ksy;
        int* base = ws + (long)b * L.per_image + (xaxis ? 0 : (long)Wd * (2 + L.ksx));
        int* kout = base + 2L * n_out + (long)xx * ks;
        if (!ok) {
            base[xx] = 0;
            base[n_out + xx] = 0;
            continue;
        }
        // every operation below is one rounded fp64 operation of the contract, in its order
        const double scale = (double)n_in / (double)n_out;
        const double fs = scale < 1.0 ? 1.0 : scale;
        const double support = fs;
        const double ss = 1.0 / fs;
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        int n = xmax - xmin;
        n = n < 0 ? 0 : (n > ks ? ks : n);                   // n <= 2 * support + 1 <= ks by construction
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            ww += a < 1.0 ? 1.0 - a : 0.0;
        }
        for (int x = 0; x < n; ++x) {                        // the same operations again give the same w: nothing is stored in between
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            double wv = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) wv /= ww;
            kout[x] = (int)(0.5 + wv * 4194304.0);
        }
        base[xx] = xmin;
        base[n_out + xx] = n;
    }
}

template <typename T, int C>
__global__ __launch_bounds__(PIL_COLS * C) void pil_resample_kernel(const uint8_t* __restrict__ src, const long* __restrict__ offsets,
                                                                   const int* __restrict__ sizes, int max_h, int max_w, int swap_rb,
                                                                   T* __restrict__ dst, uint8_t* __restrict__ u8_out, int Hd, int Wd, int Cp,
                                                                   const int* __restrict__ ws, int bands, int chunks) {
    constexpr int NT = PIL_COLS * C;                         // threads
    constexpr int TILE = NT * PIL_CHUNKS * 16;               // bytes of one LDS tile buffer
    constexpr int TP = (TILE - 16) / C;                      // source pixels per tile: up to 15 bytes of the buffer lie below the first one
    constexpr int N = Vec16<T>::N;
    __shared__ __attribute__((aligned(16))) uint8_t tile[2][TILE];
    __shared__ int kxs[PIL_KCAP * PIL_COLS];                 // [tap][column]: conflict-free across the columns of a wave
    __shared__ uint8_t obytes[PIL_R][PIL_COLS][4];

    const int t = threadIdx.x;
    const int per_img = bands * chunks;
    const int b = blockIdx.x / per_img, band = (blockIdx.x % per_img) / chunks, chunk = blockIdx.x % chunks;
    const int lcol = t / C, ch = t - lcol * C;
    const int col0 = chunk * PIL_COLS, ncols = min(PIL_COLS, Wd - col0), col = col0 + lcol;
    const int row0 = band * PIL_R, nrows = min(PIL_R, Hd - row0);

    int h, w;
    long off;
    const bool ok = pil_image_ok(offsets, sizes, b, C, max_h, max_w, Hd, h, w, off);
    const PilLayout L = pil_layout(max_h, max_w, Hd, Wd);
    const int* wx = ws + (long)b * L.per_image;
    const int* wy = wx + (long)Wd * (2 + L.ksx);
    const int* kxg = wx + 2L * Wd + (long)col * L.ksx;

    // this thread's horizontal taps, the band's vertical ones (block-uniform)
    const bool active = ok && lcol < ncols;
    const int xmin = active ? wx[col] : 0, xn = active ? wx[Wd + col] : 0;
    int ymin[PIL_R], yn[PIL_R];
#pragma unroll
    for (int i = 0; i < PIL_R; ++i) {
        const bool in = ok && i < nrows;
        ymin[i] = in ? wy[row0 + i] : 0;
        yn[i] = in ? wy[Hd + row0 + i] : 0;
    }
    int segx0 = 0, segx1 = 0, r0 = 0, r1 = 0;                // source columns / rows this workgroup reads
    if (ok) {
        segx0 = wx[col0];
        segx1 = wx[col0 + ncols - 1] + wx[Wd + col0 + ncols - 1];
        r0 = wy[row0];
        r1 = wy[row0 + nrows - 1] + wy[Hd + row0 + nrows - 1];
    }
    // The stream: a step is one tile of source pixels [lo, hi) of G consecutive source rows.  Where the columns' windows fit one tile
    // (the usual case: 330 pixels at 640 -> 128) a tile holds G = TILE / slot whole row segments, each in a slot of cps 16-byte chunks
    // that starts at the 16-byte-aligned address below the segment's first byte; wider windows take one row per step, tile after tile.
    const int ntiles = segx1 > segx0 ? (segx1 - segx0 + TP - 1) / TP : 0;
    const int cps = ntiles == 1 ? ((segx1 - segx0) * C + 15 + 15) >> 4 : TILE / 16;       // chunks per slot
    const int G = (TILE / 16) / cps;                                                      // >= 1: cps <= TILE / 16
    const int steps = (r1 > r0 && ntiles > 0) ? ((r1 - r0 + G - 1) / G) * ntiles : 0;
    const bool k_global = __syncthreads_or(xn > PIL_KCAP) != 0;
    if (!k_global) {
        if (ch == 0)
            for (int x = 0; x < xn; ++x) kxs[x * PIL_COLS + lcol] = kxg[x];
    }
    const uint8_t* img_lo = src + (ok ? off : 0);
    const uint8_t* img_hi = img_lo + (ok ? (long)h * w * C : 0);

    uint4 stg[PIL_CHUNKS];
    int cg[PIL_CHUNKS], cc[PIL_CHUNKS];                       // the slot (row of the step) and the chunk inside it that this thread stages
#pragma unroll
    for (int q = 0; q < PIL_CHUNKS; ++q) {
        const int c = t + q * NT;
        cg[q] = c / cps;
        cc[q] = c - cg[q] * cps;
    }
    // step `s`: its first source row, its source pixels [lo, hi)
    auto step_of = [&](int s, int& lo, int& hi) {
        const int j = s % ntiles;
        lo = segx0 + j * TP;
        hi = min(lo + TP, segx1);
        return r0 + (s / ntiles) * G;
    };
    auto load_regs = [&](int s) {
        int lo, hi, mask = 0;
        const int rbase = step_of(s, lo, hi);
#pragma unroll
        for (int q = 0; q < PIL_CHUNKS; ++q) {
            const int r = rbase + cg[q];
            if (cg[q] < G && r < r1) {
                const uint8_t* g = img_lo + ((long)r * w + lo) * C;
                const int head = (int)((uintptr_t)g & 15);
                if (cc[q] < ((head + (hi - lo) * C + 15) >> 4)) {
                    const uint8_t* p = g - head + 16L * cc[q];
                    if (p >= img_lo && p + 16 <= img_hi) {
                        stg[q] = *reinterpret_cast<const uint4*>(p);
                    } else {                                 // the image's first or last bytes: nothing outside [img_lo, img_hi) is read
                        uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const uint8_t* a = p + i;
                            const uint32_t v = (a >= img_lo && a < img_hi) ? (uint32_t)*a : 0u;
                            wd[i >> 2] |= v << (8 * (i & 3));
                        }
                        stg[q] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                    }
                    mask |= 1 << q;
                }
            }
        }
        return mask;
    };
    auto store_lds = [&](int buf, int mask) {
#pragma unroll
        for (int q = 0; q < PIL_CHUNKS; ++q)
            if (mask & (1 << q)) *reinterpret_cast<uint4*>(&tile[buf][16 * (t + q * NT)]) = stg[q];
    };

    int acc[PIL_R];
#pragma unroll
    for (int i = 0; i < PIL_R; ++i) acc[i] = 0;
    int hacc = 0;
    if (steps > 0) store_lds(0, load_regs(0));
    __syncthreads();                                         // tile 0 and kxs
    for (int s = 0; s < steps; ++s) {
        int mask_next = 0;
        if (s + 1 < steps) mask_next = load_regs(s + 1);     // in flight while tile s is consumed
        int lo, hi;
        const int rbase = step_of(s, lo, hi), j = s % ntiles;
        const int xa = max(0, lo - xmin), xb = min(xn, hi - xmin);
        const uint8_t* tb = tile[s & 1];
        const int rows = min(G, r1 - rbase);
        for (int g = 0; g < rows; ++g) {
            const int r = rbase + g;
            const int head = (int)((uintptr_t)(img_lo + ((long)r * w + lo) * C) & 15);
            const int o = g * cps * 16 + head + (xmin - lo) * C + ch;            // byte of tap 0 (below the slot where xa > 0)
            if (j == 0) hacc = 0;
            if (!k_global) {
                for (int x = xa; x < xb; ++x) hacc += (int)tb[o + x * C] * kxs[x * PIL_COLS + lcol];
            } else {
                for (int x = xa; x < xb; ++x) hacc += (int)tb[o + x * C] * kxg[x];
            }
            if (j == ntiles - 1) {
                int hb = (hacc + (1 << (PIL_BITS - 1))) >> PIL_BITS;             // the u8 intermediate of the horizontal pass
                hb = hb < 0 ? 0 : (hb > 255 ? 255 : hb);
#pragma unroll
                for (int i = 0; i < PIL_R; ++i) {
                    const int d = r - ymin[i];
                    if (d >= 0 && d < yn[i]) acc[i] += wy[2L * Hd + (long)(row0 + i) * L.ksy + d] * hb;
                }
            }
        }
        if (s + 1 < steps) store_lds((s + 1) & 1, mask_next);
        __syncthreads();
    }

    // epilogue: clamp and shift; bytes to u8_out, byte / 255 to dst as 16-byte stores with zero padding channels
    const int cout = (swap_rb && C == 3) ? 2 - ch : ch;
#pragma unroll
    for (int i = 0; i < PIL_R; ++i) {
        int v = (acc[i] + (1 << (PIL_BITS - 1))) >> PIL_BITS;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        if (!ok) v = 0;
        obytes[i][lcol][cout] = (uint8_t)v;
        if (u8_out && i < nrows && lcol < ncols) u8_out[(((long)b * Hd + row0 + i) * Wd + col) * C + cout] = (uint8_t)v;
    }
    __syncthreads();
    const int vpp = Cp / N;                                  // 16-byte vectors per pixel
    for (int it = t; it < nrows * ncols * vpp; it += NT) {
        const int i = it / (ncols * vpp), rem = it - i * (ncols * vpp), lc = rem / vpp, v = rem - lc * vpp;
        Vec16<T> o;
        o.zero();
        if (v == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) o.set(c, mu_u8_unit(obytes[i][lc][c]));
        }
        o.store(dst + (((long)b * Hd + row0 + i) * Wd + col0 + lc) * Cp + v * N);
    }
}

}  // namespace

extern "C" long mu_pil_resize_workspace_bytes(int B, int max_h, int max_w, int Hd, int Wd) {
    if (B < 1 || max_h < 1 || max_w < 1 || Hd < 1 || Wd < 1 || max_h > 16384 || max_w > 16384 || (long)Hd * Wd > 65536) return -1;
    return (long)B * pil_ws_ints(max_h, max_w, Hd, Wd) * (long)sizeof(int);
}

extern "C" int mu_pil_resize_u8_nhwc(const unsigned char* src, const long* offsets, const int* sizes, int B, int C, int max_h, int max_w,
                                     int swap_rb, void* dst, unsigned char* u8_out, unsigned char* valid, int Hd, int Wd, int Cp, int dtype,
                                     void* workspace, long workspace_bytes, void* stream) {
    if (!src || !offsets || !sizes || !dst || !valid || !workspace) return MU_ERR_ARG;
    if (B < 1 || (C != 1 && C != 3) || Cp < C || Cp % 32 || (dtype != MU_F32 && dtype != MU_F16)) return MU_ERR_ARG;
    const long need = mu_pil_resize_workspace_bytes(B, max_h, max_w, Hd, Wd);
    if (need < 0 || workspace_bytes < need) return MU_ERR_ARG;
    const int bands = mu_cdiv(Hd, PIL_R), chunks = mu_cdiv(Wd, PIL_COLS);
    const long blocks = (long)B * bands * chunks;
    if (blocks > 0x7fffffffL) return MU_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    pil_coeff_kernel<<<mu_grid((long)B * (Wd + Hd), 256, 65536), 256, 0, st>>>(offsets, sizes, B, C, max_h, max_w, Hd, Wd, (int*)workspace, valid);
    MU_CHECK_LAUNCH();
    auto resample = [&](auto tag, auto channels) -> int {
        using T = decltype(tag);
        constexpr int CC = decltype(channels)::value;
        pil_resample_kernel<T, CC><<<(unsigned)blocks, PIL_COLS * CC, 0, st>>>(src, offsets, sizes, max_h, max_w, swap_rb, (T*)dst, u8_out, Hd, Wd, Cp,
                                                                              (const int*)workspace, bands, chunks);
        MU_CHECK_LAUNCH();
        return MU_OK;
    };
    return with_storage(dtype, [&](auto tag) -> int {
        return C == 1 ? resample(tag, std::integral_constant<int, 1>{}) : resample(tag, std::integral_constant<int, 3>{});
    });
}
