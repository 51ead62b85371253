// COCO ground truth on the device (gfx950): what coco_instance.py:52-83, 331-338 do per image on the host -- annToMask of every
// annotation (rleFrPoly per polygon, their union, rleDecode; crowd annotations carry an RLE), cv2.resize(.., INTER_NEAREST) of every
// mask, torch.sum over the masks -- from the parsed vertex lists / counts of the annotation file.  The rasterisation is restated from the
// published maskApi.c (rleFrPoly); the contract is spelled out in include/maskunet_hip.h.
//
// coco_masks_kernel: one workgroup per annotation.  Two COLUMN-MAJOR bitmaps of the original image live in LDS (2^19 bits each):
//   T   the toggles of the polygon at hand.  A bitmap IS the sorted set of maskApi's qsort, and atomicXor cancels equal toggles the way
//       its merge of zero-length runs does; so no sort.
//   U   the union of the annotation's polygons.
// Per polygon, in chunks of CM_THREADS edges:
//   edges    one per thread: scaled end points, slope, point count max(dx, dy) + 1 and the LAST point of the edge before it (computed by
//            that edge's own formula: with negative coordinates truncation makes it differ from the vertex);
//   points   a workgroup scan of the counts (wave_prims.h) gives every edge its first point; point q of the chunk finds its edge by
//            bisection and is computed in closed form from (edge, d), so a long edge is shared by all threads;
//   toggles  where u changes between a point and its predecessor: atomicXor on T;
//   fill     prefix parity of T over the span of words that were touched: shift-XOR ladder inside a word, the parity of the words
//            before it by a scan; U |= the result, T back to zero.
// An RLE's toggles are the prefix sums of its counts; the rest is the same.  From U: area by popcount; the nearest samples read single
// bits; cover by integer atomicAdd, ids by atomicMax, masks by plain stores.  Integer atomics only: bit-identical from run to run.
// fp64: every operation of the contract is rounded on its own.  Ties at .5 are common on 5x-scaled vertices, so a fused multiply-add
// changes masks: this file is built with -ffp-contract=off (Makefile) and says so itself below.
#include "wave_prims.h"

#pragma clang fp contract(off)

#define CM_THREADS 512
#define CM_WAVES (CM_THREADS / 64)
#define CM_MAX_PIXELS (1 << 19)
#define CM_WORDS (CM_MAX_PIXELS / 32)
#define CM_MAX_OUT_PIXELS 65536
#define CM_MAX_POINTS (1 << 21)                        // the counts of a chunk of edges, each clamped to max_points + 1, sum in an int
#define CM_COORD_LIMIT 16777216.0

struct CocoMaskParams {
    const double* xy;
    const int *poly_off, *ann_poly_off, *rle_counts, *ann_rle_off, *img_ann_off, *sizes;
    int B, A, P, n_points, n_counts, Ho, Wo, max_points;
    unsigned long long* cover;
    int* ids;
    unsigned char* masks;
    int *area, *valid;
};

// (int)(5 c + .5); false where c is not finite or the sum reaches 2^24 in magnitude
__device__ __forceinline__ bool cm_scale(double c, int& X) {
    double s = 5.0 * c;
    s = s + .5;
    X = 0;
    if (!(fabs(s) < CM_COORD_LIMIT)) return false;
    X = (int)s;
    return true;
}

__device__ __forceinline__ int cm_edge_count(int xs, int ys, int xe, int ye) { return max(abs(xe - xs), abs(ys - ye)) + 1; }

// the slope of the walk along the longer axis (after the flip); 0 for a degenerate edge
__device__ __forceinline__ double cm_edge_slope(int xs, int ys, int xe, int ye) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    if ((dx | dy) == 0) return 0.0;
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (dx >= dy) return (double)(flip ? ys - ye : ye - ys) / (double)dx;
    return (double)(flip ? xs - xe : xe - xs) / (double)dy;
}

// point d (0 .. max(dx, dy)) of the edge, counted from its original start
__device__ __forceinline__ void cm_edge_point(int xs, int ys, int xe, int ye, double s, int d, int& u, int& v) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    if ((dx | dy) == 0) {
        u = xs;
        v = ys;
        return;
    }
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    const int x0 = flip ? xe : xs, y0 = flip ? ye : ys;
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        double f = s * (double)t;
        f = (double)y0 + f;
        f = f + .5;
        u = t + x0;
        v = (int)f;
    } else {
        const int t = flip ? dy - d : d;
        double f = s * (double)t;
        f = (double)x0 + f;
        f = f + .5;
        v = t + y0;
        u = (int)f;
    }
}

// the toggle of point (u, v) with predecessor (pu, pv), pu != u: -1 where the crossing is no pixel column of the image, else 0..N
__device__ __forceinline__ int cm_toggle_pos(int u, int v, int pu, int pv, int h, int w) {
    double xd = (double)(u < pu ? u : u - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0.0 || xd > (double)(w - 1)) return -1;
    double yd = (double)(v < pv ? v : pv);
    yd = (yd + .5) / 5.0 - .5;
    if (yd < 0.0) yd = 0.0;
    else if (yd > (double)h) yd = (double)h;
    yd = ceil(yd);
    return (int)xd * h + (int)yd;
}

// Workgroup state of the fill: lo / hi = the span of words of T that hold toggles, `turn` picks one of two sets of wave totals (a wave may
// start the next scan while another still reads the totals of this one; two barriers lie between two uses of the same set).
struct CmScan {
    unsigned tot[2][CM_WAVES];
    int lo, hi;
};

// workgroup exclusive scan of one value per thread; returns the sum over the threads below, `total` the sum over all.  Holds a barrier.
__device__ __forceinline__ unsigned cm_block_scan(unsigned v, CmScan& S, int& turn, int lane, int wave, unsigned& total) {
    const unsigned incl = wave_scan_incl(v, lane);
    const unsigned below = block_exclusive_base((unsigned)__shfl((int)incl, 63), S.tot[turn & 1], lane, wave, CM_WAVES, total);
    ++turn;
    return below + incl - v;
}

// a toggle at position a <= N; position N holds no pixel (cm_fill runs an odd parity on to the last word by itself)
__device__ __forceinline__ void cm_apply(unsigned* T, int a, int N, int& tlo, int& thi) {
    if (a >= N) return;
    atomicXor(&T[a >> 5], 1u << (a & 31));
    tlo = min(tlo, a >> 5);
    thi = max(thi, a >> 5);
}

// U |= prefix parity of T over the touched span; T back to zero.  Every thread of the workgroup calls it.
__device__ __forceinline__ void cm_fill(unsigned* T, unsigned* U, CmScan& S, int& turn, int& tlo, int& thi, int N, int nwords, int tid,
                                        int lane, int wave) {
    const int wlo = (int)wave_min((unsigned)tlo), whi = (int)wave_max((unsigned)(thi + 1)) - 1;
    if (lane == 0) {
        atomicMin(&S.lo, wlo);
        atomicMax(&S.hi, whi);
    }
    __syncthreads();                                   // the toggles and the span are complete
    const int lo = S.lo, hi = S.hi;
    unsigned carry = 0;
    for (int base = lo; base <= hi; base += CM_THREADS) {
        const int wd = base + tid;
        unsigned x = wd <= hi ? T[wd] : 0u;
        x ^= x << 1;
        x ^= x << 2;
        x ^= x << 4;
        x ^= x << 8;
        x ^= x << 16;                                  // bit i = parity of the word's bits 0..i
        unsigned total;
        const unsigned before = carry + cm_block_scan(x >> 31, S, turn, lane, wave, total);
        if (before & 1u) x = ~x;
        if (wd <= hi) {
            if (wd == nwords - 1 && (N & 31)) x &= (1u << (N & 31)) - 1u;
            U[wd] |= x;
            T[wd] = 0u;
        }
        carry += total;
    }
    if (carry & 1u)                                    // an odd number of toggles below N: ones up to position N - 1
        for (int wd = max(hi, -1) + 1 + tid; wd < nwords; wd += CM_THREADS)
            U[wd] = (wd == nwords - 1 && (N & 31)) ? (1u << (N & 31)) - 1u : ~0u;
    __syncthreads();                                   // everyone has read the span
    if (tid == 0) {
        S.lo = 0x7fffffff;
        S.hi = -1;
    }
    tlo = 0x7fffffff;
    thi = -1;
}

// Dynamic LDS: T and U, CM_WORDS words each (128 KiB); static: the edges of a chunk and the scan state (18 KiB).
__global__ __launch_bounds__(CM_THREADS) void coco_masks_kernel(const CocoMaskParams P) {
    extern __shared__ unsigned cm_lds[];
    __shared__ int e_xs[CM_THREADS], e_ys[CM_THREADS], e_xe[CM_THREADS], e_ye[CM_THREADS], e_pu[CM_THREADS], e_pv[CM_THREADS];
    __shared__ int e_start[CM_THREADS];
    __shared__ double e_s[CM_THREADS];
    __shared__ CmScan S;
    unsigned* T = cm_lds;
    unsigned* U = cm_lds + CM_WORDS;
    const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ho = P.Ho, Wo = P.Wo, out_n = Ho * Wo;
    unsigned char* mask_out = P.masks ? P.masks + (long)a * out_n : nullptr;

    // the image of this annotation: the last b with img_ann_off[b] <= a.  Every value read below is uniform over the workgroup.
    int b = 0;
    for (int hi = P.B; hi - b > 1;) {
        const int mid = (b + hi) >> 1;
        if (P.img_ann_off[mid] <= a) b = mid;
        else hi = mid;
    }
    const int row0 = P.img_ann_off[b];
    const bool placed = row0 <= a && a < P.img_ann_off[b + 1];
    const int h = P.sizes[2 * b], w = P.sizes[2 * b + 1];
    const int p0 = P.ann_poly_off[a], p1 = P.ann_poly_off[a + 1], r0 = P.ann_rle_off[a], r1 = P.ann_rle_off[a + 1];
    bool ok = placed && h >= 1 && w >= 1 && (long)h * w <= CM_MAX_PIXELS && 0 <= p0 && p0 <= p1 && p1 <= P.P && 0 <= r0 && r0 <= r1 &&
              r1 <= P.n_counts && !(p1 > p0 && r1 > r0);
    const int N = ok ? h * w : 0, nwords = (N + 31) >> 5;

    for (int i = tid; i < nwords; i += CM_THREADS) {
        T[i] = 0u;
        U[i] = 0u;
    }
    if (tid == 0) {
        S.lo = 0x7fffffff;
        S.hi = -1;
    }
    int turn = 0, tlo = 0x7fffffff, thi = -1;
    __syncthreads();

    if (ok && r1 > r0) {
        // ---- one RLE: counts non-negative and summing to N, toggles = their prefix sums without the last
        const int n = r1 - r0;
        const int* rc = P.rle_counts + r0;
        int bad = 0;
        unsigned sum = 0;                              // saturates at N + 1 per thread: 512 * (2^19 + 1) fits
        for (int i = tid; i < n; i += CM_THREADS) {
            const int c = rc[i];
            bad |= (c < 0 || c > N);
            sum = min(sum + (unsigned)(bad ? 0 : c), (unsigned)N + 1u);
        }
        unsigned total;
        cm_block_scan(sum, S, turn, lane, wave, total);
        if (__syncthreads_or(bad) || total != (unsigned)N) ok = false;
        if (ok) {
            unsigned carry = 0;
            for (int base = 0; base < n; base += CM_THREADS) {
                const int i = base + tid;
                const unsigned c = i < n ? (unsigned)rc[i] : 0u;
                const unsigned end = carry + cm_block_scan(c, S, turn, lane, wave, total) + c;
                if (i < n - 1) cm_apply(T, (int)end, N, tlo, thi);
                carry += total;
            }
            cm_fill(T, U, S, turn, tlo, thi, N, nwords, tid, lane, wave);
        }
    }

    for (int p = p0; ok && p < p1; ++p) {
        // ---- one polygon
        const int q0 = P.poly_off[p], q1 = P.poly_off[p + 1];
        if (!(0 <= q0 && q0 <= q1 && q1 <= P.n_points)) {
            ok = false;
            break;
        }
        const int k = q1 - q0;
        const double* xy = P.xy + 2 * (long)q0;
        long emitted = 0;
        for (int base = 0; base < k; base += CM_THREADS) {
            const int j = base + tid, in_chunk = min(CM_THREADS, k - base);
            int xs = 0, ys = 0, xe = 0, ye = 0, pu = 0, pv = 0, n = 0;
            double s = 0.0;
            int bad = 0;
            if (j < k) {
                const int jn = j + 1 < k ? j + 1 : 0;
                bad |= !cm_scale(xy[2 * j], xs) | !cm_scale(xy[2 * j + 1], ys) | !cm_scale(xy[2 * jn], xe) | !cm_scale(xy[2 * jn + 1], ye);
                if (j > 0) {
                    int xb, yb;
                    bad |= !cm_scale(xy[2 * j - 2], xb) | !cm_scale(xy[2 * j - 1], yb);
                    cm_edge_point(xb, yb, xs, ys, cm_edge_slope(xb, yb, xs, ys), cm_edge_count(xb, yb, xs, ys) - 1, pu, pv);
                }
                s = cm_edge_slope(xs, ys, xe, ye);
                n = min(cm_edge_count(xs, ys, xe, ye), P.max_points + 1);
            }
            if (__syncthreads_or(bad)) {               // also: the points of the chunk before are done with e_*
                ok = false;
                break;
            }
            e_xs[tid] = xs;
            e_ys[tid] = ys;
            e_xe[tid] = xe;
            e_ye[tid] = ye;
            e_pu[tid] = pu;
            e_pv[tid] = pv;
            e_s[tid] = s;
            unsigned total;
            e_start[tid] = (int)cm_block_scan((unsigned)n, S, turn, lane, wave, total);
            emitted += total;
            if (emitted > P.max_points) {
                ok = false;
                break;
            }
            __syncthreads();                           // e_* complete
            for (int q = tid; q < (int)total; q += CM_THREADS) {
                int e = 0;
                for (int hi = in_chunk; hi - e > 1;) {
                    const int mid = (e + hi) >> 1;
                    if (e_start[mid] <= q) e = mid;
                    else hi = mid;
                }
                const int d = q - e_start[e];
                if (d == 0 && base + e == 0) continue; // the polygon's first point has no predecessor
                int u, v, qu = e_pu[e], qv = e_pv[e];
                cm_edge_point(e_xs[e], e_ys[e], e_xe[e], e_ye[e], e_s[e], d, u, v);
                if (d > 0) cm_edge_point(e_xs[e], e_ys[e], e_xe[e], e_ye[e], e_s[e], d - 1, qu, qv);
                if (u == qu) continue;
                const int pos = cm_toggle_pos(u, v, qu, qv, h, w);
                if (pos >= 0) cm_apply(T, pos, N, tlo, thi);
            }
        }
        if (ok) cm_fill(T, U, S, turn, tlo, thi, N, nwords, tid, lane, wave);
    }
    __syncthreads();

    if (!ok) {                                         // an invalid row paints nothing
        if (tid == 0) {
            P.area[a] = 0;
            P.valid[a] = 0;
        }
        if (mask_out)
            for (int i = tid; i < out_n; i += CM_THREADS) mask_out[i] = 0;
        return;
    }
    unsigned bits = 0;
    for (int i = tid; i < nwords; i += CM_THREADS) bits += __popc(U[i]);
    unsigned area;
    cm_block_scan(bits, S, turn, lane, wave, area);
    if (tid == 0) {
        P.area[a] = (int)area;
        P.valid[a] = 1;
    }
    // cv2.resize(.., INTER_NEAREST): source index min(floor(d * (1 / (dst / src))), src - 1)
    const double ifx = 1.0 / ((double)Wo / (double)w), ify = 1.0 / ((double)Ho / (double)h);
    unsigned long long* cover = P.cover + (long)b * out_n;
    int* ids = P.ids + (long)b * out_n;
    for (int i = tid; i < out_n; i += CM_THREADS) {
        const int oy = i / Wo, ox = i - oy * Wo;
        const int sx = min((int)floor((double)ox * ifx), w - 1), sy = min((int)floor((double)oy * ify), h - 1);
        const int pos = sx * h + sy;
        const unsigned bit = (U[pos >> 5] >> (pos & 31)) & 1u;
        if (mask_out) mask_out[i] = (unsigned char)bit;
        if (bit) {
            atomicAdd(&cover[i], 1ull);
            atomicMax(&ids[i], a - row0 + 1);
        }
    }
}

__global__ __launch_bounds__(256) void coco_zero_kernel(unsigned long long* __restrict__ cover, int* __restrict__ ids, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        cover[i] = 0ull;
        ids[i] = 0;
    }
}

// dynamic LDS of coco_masks_kernel: both bitmaps, always at their full size; granted as such (common.h: mu_lds_grant)
#define CM_LDS_BYTES (2 * CM_WORDS * (int)sizeof(unsigned))

extern "C" int mu_coco_masks_supported(int Ho, int Wo, int max_points) {
    if (Ho <= 0 || Wo <= 0 || (long)Ho * Wo > CM_MAX_OUT_PIXELS || max_points < 1 || max_points > CM_MAX_POINTS) return MU_ERR_SHAPE;
    return MU_OK;
}

extern "C" long mu_coco_masks_workspace_bytes(int B, int A, int Ho, int Wo) {
    (void)B, (void)A, (void)Ho, (void)Wo;              // both bitmaps live in LDS: no global scratch
    return 0;
}

extern "C" int mu_coco_masks(const double* xy, const int* poly_offsets, const int* ann_poly_offsets, const int* rle_counts,
                             const int* ann_rle_offsets, const int* img_ann_offsets, const int* sizes, int B, int A, int P, long n_points,
                             long n_counts, int Ho, int Wo, int max_points, long* cover, int* ids, unsigned char* masks_or_null, int* area,
                             int* valid, void* workspace, long ws_bytes, void* stream) {
    if (!poly_offsets || !ann_poly_offsets || !ann_rle_offsets || !img_ann_offsets || !sizes || !cover || !ids) return MU_ERR_ARG;
    if (B <= 0 || A < 0 || P < 0 || n_points < 0 || n_counts < 0 || n_points > 0x3fffffffL || n_counts > 0x7fffffffL || Ho <= 0 ||
        Wo <= 0 || max_points <= 0 || ws_bytes < 0)
        return MU_ERR_ARG;
    if ((n_points > 0 && !xy) || (n_counts > 0 && !rle_counts) || (A > 0 && (!area || !valid))) return MU_ERR_ARG;
    if (mu_coco_masks_supported(Ho, Wo, max_points) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_coco_masks_workspace_bytes(B, A, Ho, Wo)) return MU_ERR_WORKSPACE;
    (void)workspace;
    if (A > 0 && !mu_lds_grant<coco_masks_kernel>(CM_LDS_BYTES)) return MU_ERR_LAUNCH;
    const long n_out = (long)B * Ho * Wo;
    coco_zero_kernel<<<mu_grid(n_out, 256, 4096), 256, 0, (hipStream_t)stream>>>((unsigned long long*)cover, ids, n_out);
    MU_CHECK_LAUNCH();
    if (A == 0) return MU_OK;
    CocoMaskParams K;
    K.xy = xy;
    K.poly_off = poly_offsets;
    K.ann_poly_off = ann_poly_offsets;
    K.rle_counts = rle_counts;
    K.ann_rle_off = ann_rle_offsets;
    K.img_ann_off = img_ann_offsets;
    K.sizes = sizes;
    K.B = B;
    K.A = A;
    K.P = P;
    K.n_points = (int)n_points;
    K.n_counts = (int)n_counts;
    K.Ho = Ho;
    K.Wo = Wo;
    K.max_points = max_points;
    K.cover = (unsigned long long*)cover;
    K.ids = ids;
    K.masks = masks_or_null;
    K.area = area;
    K.valid = valid;
    coco_masks_kernel<<<A, CM_THREADS, CM_LDS_BYTES, (hipStream_t)stream>>>(K);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
