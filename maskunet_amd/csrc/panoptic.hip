// Panoptic segments on the device (gfx950): mu_panoptic merges a semantic map and the instances of mu_instances / mu_dbscan_instances /
// mu_id_instances into COCO panoptic segments -- every kept thing instance one segment, every kept stuff class ONE segment however
// many pieces it has, everything else void -- and writes the segment map, its table, the COCO segment ids and panopticapi's id2rgb
// image.  The rule is in include/maskunet_hip.h and DESIGN.md 10.
// Scheme: ONE launch, one workgroup of 1024 threads per image, integer LDS atomics only.  A pixel's candidate is a KEY: k - 1 for thing
// instance k, max_inst + c for stuff class c.  Dynamic LDS (ints), all of it tallies:
//   slot[max_inst + num_classes]   >= 0: a live key, the lowest pixel seen so far (0x7fffffff: none yet); -1: its pixels are void;
//                                  -2 (instances only): not a thing, its pixels fall through to the stuff rule;
//   segno[max_inst + num_classes]  the key's segment number;
//   cnt[num_classes]               stuff candidate pixels per class, later the class_rank counters of the counting sort;
//   val[max_seg]                   the segment's class, later its COCO id (0: not representable);
//   area / xmin / xmax / ymax [max_seg]   (y_min is the row of the first pixel: segments are numbered in raster order).
// 124 KiB at the limits (4096 + 1024 keys, 4096 segments): beside them the 8-byte keys of the score order (32 KiB) do not fit a
// workgroup's grant, so those are sorted in the workspace; at 1024 instances, 1024 segments and 150 classes the kernel holds 30 KiB.
// Passes over the pixels (P) and the barriers between them:
//   P1  first pixel per key (atomicMin), stuff pixels per class;  then stuff classes below the area limit become void keys;
//   P2  heads (pixel == slot[key]) in raster order: count per wave segment, exclusive base over the waves, flag rank = the segment
//       number; the head writes segno[key], the segment's class, first pixel, source and score;
//       then wave 0 walks the segments in order through wave_sort_chunk: class_rank, COCO id, invalid bit 0;
//   P3  seg, seg_cls, id_map, rgb per pixel; area and box by LDS atomics (one set per wave where 64 pixels share a segment);
//   then the table rows, the zero rows and the score order.
#include "wave_prims.h"

#define PAN_THREADS 1024
#define PAN_WAVES (PAN_THREADS / 64)
#define PAN_MAX_PIXELS 65536
#define PAN_MAX_ROWS 4096                                      // max_inst and max_seg
#define PAN_MAX_CLASSES 1024
#define PAN_NONE 0x7fffffff

struct PanParams {
    const int* cls;
    const int* ids;
    const int* table;
    const float* score;
    const int* count;
    const int* kind;
    const int* category;
    int N, W, max_inst, num_classes, max_seg, P;
    int label_divisor, stuff_area_limit, thing_area_limit, bgr;
    float score_threshold;
    int *seg, *seg_cls, *seg_table, *seg_count, *seg_order, *seg_source, *seg_values, *id_map, *invalid;
    float* seg_score;
    unsigned char* rgb;
    unsigned long long* keys;
};

// the key of pixel i (see above), -1 = void.  c = the pixel's class; inv collects bit 2 (an instance past max_inst).
__device__ __forceinline__ int pan_key(const PanParams& P, const int* cls, const int* ids, const int* slot, int cnt_in, int i, int& c,
                                       unsigned& inv) {
    const int k = ids[i];
    c = cls[i];
    if (k >= 1 && k <= cnt_in) {
        if (k > P.max_inst) {
            inv |= 4u;
            return -1;
        }
        const int st = slot[k - 1];
        if (st >= -1) return st >= 0 ? k - 1 : -1;             // a thing: kept or void, never stuff
    }
    if ((unsigned)c >= (unsigned)P.num_classes) return -1;
    return slot[P.max_inst + c] >= 0 ? P.max_inst + c : -1;
}

// the class of a key's segment: the instance's for a thing, the pixel's (c) for stuff.  A second load that depends on the first, so
// only where the class is needed (heads, and the thing pixels of P3)
__device__ __forceinline__ int pan_class(const int* table, int key, int max_inst, int c) {
    return key < max_inst ? table[(long)key * 8] : c;
}

__global__ __launch_bounds__(PAN_THREADS) void panoptic_kernel(const PanParams P) {
    extern __shared__ int pan_lds[];
    __shared__ unsigned wave_total[PAN_WAVES];
    __shared__ unsigned red;                                   // the invalid bits
    const int n_keys = P.max_inst + P.num_classes;
    int* slot = pan_lds;
    int* segno = slot + n_keys;
    int* cnt = segno + n_keys;
    int* val = cnt + P.num_classes;
    unsigned* area = (unsigned*)(val + P.max_seg);
    unsigned* xmin = area + P.max_seg;
    unsigned* xmax = xmin + P.max_seg;
    unsigned* ymax = xmax + P.max_seg;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = P.N, W = P.W, max_inst = P.max_inst, max_seg = P.max_seg;
    const int* cls = P.cls + (long)b * N;
    const int* ids = P.ids + (long)b * N;
    const int* table = P.table + (long)b * max_inst * 8;
    const float* score = P.score + (long)b * max_inst;
    int* seg = P.seg + (long)b * N;
    int* seg_cls = P.seg_cls + (long)b * N;
    int* id_map = P.id_map + (long)b * N;
    unsigned char* rgb = P.rgb + (long)b * N * 3;
    int* seg_table = P.seg_table + (long)b * max_seg * 8;
    float* seg_score = P.seg_score + (long)b * max_seg;
    int* seg_order = P.seg_order + (long)b * max_seg;
    int* seg_source = P.seg_source + (long)b * max_seg;
    int* seg_values = P.seg_values + (long)b * max_seg;
    unsigned long long* keys = P.keys + (long)b * P.P;
    const int cnt_in = P.count[b], K = max(0, min(cnt_in, max_inst));

    // the keys' states
    if (tid == 0) red = 0u;
    for (int k = tid; k < max_inst; k += PAN_THREADS) {
        int st = -2;
        if (k < K) {
            const int c = table[(long)k * 8];
            if ((unsigned)c < (unsigned)P.num_classes && P.kind[c] == 2)
                st = (table[(long)k * 8 + 1] >= P.thing_area_limit && score[k] >= P.score_threshold) ? PAN_NONE : -1;
        }
        slot[k] = st;
    }
    for (int c = tid; c < P.num_classes; c += PAN_THREADS) {
        slot[max_inst + c] = P.kind[c] == 1 ? PAN_NONE : -1;
        cnt[c] = 0;
    }
    for (int r = tid; r < max_seg; r += PAN_THREADS) {
        area[r] = 0u;
        xmin[r] = 0x7fffffffu;
        xmax[r] = 0u;
        ymax[r] = 0u;
    }
    __syncthreads();

    // P1
    unsigned inv = 0;
    for (int base = wave * 64; base < N; base += PAN_THREADS) {
        const int i = base + lane;
        int c = 0;
        const int key = i < N ? pan_key(P, cls, ids, slot, cnt_in, i, c, inv) : -1;
        const int key0 = __shfl(key, 0);
        if (__ballot(key == key0) == ~0ull) {                  // 64 pixels of one key (or none): lane 0 speaks for them
            if (key0 >= 0 && lane == 0) {
                atomicMin(&slot[key0], base);
                if (key0 >= max_inst) atomicAdd(&cnt[key0 - max_inst], 64);
            }
        } else if (key >= 0) {
            atomicMin(&slot[key], i);
            if (key >= max_inst) atomicAdd(&cnt[key - max_inst], 1);
        }
    }
    for (int o = 32; o > 0; o >>= 1) inv |= (unsigned)__shfl_xor((int)inv, o);
    __syncthreads();
    for (int c = tid; c < P.num_classes; c += PAN_THREADS) {
        if (cnt[c] < max(P.stuff_area_limit, 1)) slot[max_inst + c] = -1;
        cnt[c] = 0;                                            // from here on: segments of the class so far (class_rank)
    }
    __syncthreads();

    // P2: a head is the first pixel of a live key; every live key with a pixel has exactly one
    int lo, hi;
    wave_segment(N, PAN_WAVES, wave, lo, hi);
    unsigned mine = 0, total, other = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        int c = 0;
        const int key = i < hi ? pan_key(P, cls, ids, slot, cnt_in, i, c, other) : -1;
        mine += __popcll(__ballot(key >= 0 && slot[key] == i));
    }
    unsigned running = block_exclusive_base(mine, wave_total, lane, wave, PAN_WAVES, total);
    const int n = (int)total, M = min(n, max_seg);
    if (n > max_seg) inv |= 2u;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        int c = 0;
        const int key = i < hi ? pan_key(P, cls, ids, slot, cnt_in, i, c, other) : -1;
        const bool head = key >= 0 && slot[key] == i;
        const int r = (int)wave_flag_rank(head, lane, running);
        if (head) {
            segno[key] = r + 1;
            if (r < max_seg) {
                const bool thing = key < max_inst;
                val[r] = pan_class(table, key, max_inst, c);
                seg_table[(long)r * 8 + 6] = i;
                seg_source[r] = thing ? key + 1 : 0;
                seg_score[r] = thing ? score[key] : 1.f;
            }
        }
    }
    __syncthreads();                 // LDS, and the rows this workgroup wrote to global memory, are visible past this barrier

    // class_rank and the COCO id: a counting sort by class over the segments in order, whose slot within the class IS the rank - 1
    if (wave == 0) {
        for (int base = 0; base < M; base += 64) {
            const int r = base + lane;
            const bool has = r < M;
            const int c = has ? val[r] : 0;
            const int rank = wave_sort_chunk<true>(c, has, lane, cnt) + 1;
            if (has) {
                const bool thing = P.kind[c] == 2;
                const long long v = (long long)P.category[c] * P.label_divisor + (thing ? rank : 0);
                const bool bad = v <= 0 || v >= (1ll << 24) || (thing && rank >= P.label_divisor);
                if (bad) inv |= 1u;
                val[r] = bad ? 0 : (int)v;
                seg_values[r] = bad ? 0 : (int)v;
                seg_table[(long)r * 8] = c;
                seg_table[(long)r * 8 + 7] = rank;
            }
        }
        for (int o = 32; o > 0; o >>= 1) inv |= (unsigned)__shfl_xor((int)inv, o);
    }
    if (lane == 0 && inv) atomicOr(&red, inv);
    __syncthreads();
    if (tid == 0) {
        P.seg_count[b] = n;
        P.invalid[b] = (int)red;
    }

    // P3
    for (int base = wave * 64; base < N; base += PAN_THREADS) {
        const int i = base + lane;
        int c = 0;
        const int key = i < N ? pan_key(P, cls, ids, slot, cnt_in, i, c, other) : -1;
        const int s = key >= 0 ? segno[key] : 0;
        const unsigned x = (unsigned)(i % W), y = (unsigned)(i / W);
        if (i < N) {
            const int v = (s >= 1 && s <= max_seg) ? val[s - 1] : 0;
            const unsigned char c0 = (unsigned char)(v & 255), c1 = (unsigned char)((v >> 8) & 255), c2 = (unsigned char)(v >> 16);
            seg[i] = s;
            seg_cls[i] = s ? pan_class(table, key, max_inst, c) : 0;
            id_map[i] = v;
            rgb[3 * i] = P.bgr ? c2 : c0;
            rgb[3 * i + 1] = c1;
            rgb[3 * i + 2] = P.bgr ? c0 : c2;
        }
        const bool active = s >= 1 && s <= max_seg;
        const int s0 = __shfl(s, 0);
        if (__ballot(i < N && s == s0) == ~0ull) {
            if (s0 >= 1 && s0 <= max_seg) {
                const unsigned x0 = wave_min(x), x1 = wave_max(x), y1 = wave_max(y);
                if (lane == 0) {
                    atomicAdd(&area[s0 - 1], 64u);
                    atomicMin(&xmin[s0 - 1], x0);
                    atomicMax(&xmax[s0 - 1], x1);
                    atomicMax(&ymax[s0 - 1], y1);
                }
            }
        } else if (active) {
            atomicAdd(&area[s - 1], 1u);
            atomicMin(&xmin[s - 1], x);
            atomicMax(&xmax[s - 1], x);
            atomicMax(&ymax[s - 1], y);
        }
    }
    __syncthreads();

    // the rows, zero past M; the sort keys, padding last
    for (int r = tid; r < max(max_seg, P.P); r += PAN_THREADS) {
        unsigned long long key = ~0ull;
        if (r < M) {
            int* row = seg_table + (long)r * 8;
            row[1] = (int)area[r];
            row[2] = (int)xmin[r];
            row[3] = row[6] / W;
            row[4] = (int)xmax[r];
            row[5] = (int)ymax[r];
            key = score_order_key(seg_score[r], r);
        } else if (r < max_seg) {
            int* row = seg_table + (long)r * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) row[j] = 0;
            seg_score[r] = 0.f;
            seg_source[r] = 0;
            seg_values[r] = 0;
        }
        if (r < P.P) keys[r] = key;
    }
    int S = 1;
    while (S < M) S <<= 1;
    block_sort_u64(keys, S, tid, PAN_THREADS);
    for (int r = tid; r < max_seg; r += PAN_THREADS) seg_order[r] = r < M ? (int)(unsigned)(keys[r] & 0xffffffffull) : 0;
}

// dynamic LDS of panoptic_kernel; more than 64 KiB at the limits, so granted to the most it can ask for (common.h: mu_lds_grant)
static constexpr size_t pan_lds_bytes(int max_inst, int num_classes, int max_seg) {
    return (size_t)(2 * (max_inst + num_classes) + num_classes + 5 * max_seg) * sizeof(int);
}
#define PAN_LDS_MAX ((int)pan_lds_bytes(PAN_MAX_ROWS, PAN_MAX_CLASSES, PAN_MAX_ROWS))

extern "C" int mu_panoptic_supported(int H, int W, int max_inst, int num_classes, int max_seg, int label_divisor, int stuff_area_limit,
                                     int thing_area_limit) {
    if (H <= 0 || W <= 0 || (long)H * W > PAN_MAX_PIXELS) return MU_ERR_SHAPE;
    if (max_inst < 1 || max_inst > PAN_MAX_ROWS || max_seg < 1 || max_seg > PAN_MAX_ROWS) return MU_ERR_SHAPE;
    if (num_classes < 1 || num_classes > PAN_MAX_CLASSES) return MU_ERR_SHAPE;
    if (label_divisor < 1 || stuff_area_limit < 0 || thing_area_limit < 0) return MU_ERR_SHAPE;
    return MU_OK;
}

struct PanWs {
    MuCarve c;
    unsigned long long* keys;       // [B][max_seg rounded up to a power of two] the score order is sorted here
    constexpr PanWs(void* ws, int B, int max_seg) : c(ws), keys(c.take<unsigned long long>((long)B * mu_pow2(max_seg))) {}
};
static_assert(PanWs(nullptr, 2, 5).c.bytes == 2 * 8 * 8 && PanWs(nullptr, 3, 4096).c.bytes == 3 * 4096 * 8, "mu_panoptic workspace");

extern "C" long mu_panoptic_workspace_bytes(int B, int H, int W, int max_inst, int num_classes, int max_seg) {
    if (B <= 0 || mu_panoptic_supported(H, W, max_inst, num_classes, max_seg, 1, 0, 0) != MU_OK) return 0;
    return PanWs(nullptr, B, max_seg).c.bytes;
}

extern "C" int mu_panoptic(const int* cls, const int* ids, const int* table, const float* score, const int* count, const int* kind,
                           const int* category, int B, int H, int W, int max_inst, int num_classes, int label_divisor,
                           int stuff_area_limit, int thing_area_limit, float score_threshold, int max_seg, int bgr, int* seg,
                           int* seg_cls, int* seg_table, float* seg_score, int* seg_count, int* seg_order, int* seg_source,
                           int* seg_values, int* id_map, unsigned char* rgb, int* invalid, void* workspace, long ws_bytes,
                           void* stream) {
    if (!cls || !ids || !table || !score || !count || !kind || !category || !seg || !seg_cls || !seg_table || !seg_score || !seg_count ||
        !seg_order || !seg_source || !seg_values || !id_map || !rgb || !invalid || !workspace || B <= 0 || H <= 0 || W <= 0)
        return MU_ERR_ARG;
    if (bgr != 0 && bgr != 1) return MU_ERR_ARG;
    if (mu_panoptic_supported(H, W, max_inst, num_classes, max_seg, label_divisor, stuff_area_limit, thing_area_limit) != MU_OK)
        return MU_ERR_SHAPE;
    if (ws_bytes < mu_panoptic_workspace_bytes(B, H, W, max_inst, num_classes, max_seg)) return MU_ERR_WORKSPACE;
    if (!mu_lds_grant<panoptic_kernel>(PAN_LDS_MAX)) return MU_ERR_LAUNCH;
    PanParams P;
    P.cls = cls;
    P.ids = ids;
    P.table = table;
    P.score = score;
    P.count = count;
    P.kind = kind;
    P.category = category;
    P.N = H * W;
    P.W = W;
    P.max_inst = max_inst;
    P.num_classes = num_classes;
    P.max_seg = max_seg;
    P.P = mu_pow2(max_seg);
    P.label_divisor = label_divisor;
    P.stuff_area_limit = stuff_area_limit;
    P.thing_area_limit = thing_area_limit;
    P.bgr = bgr;
    P.score_threshold = score_threshold;
    P.seg = seg;
    P.seg_cls = seg_cls;
    P.seg_table = seg_table;
    P.seg_count = seg_count;
    P.seg_order = seg_order;
    P.seg_source = seg_source;
    P.seg_values = seg_values;
    P.id_map = id_map;
    P.invalid = invalid;
    P.seg_score = seg_score;
    P.rgb = rgb;
    P.keys = PanWs(workspace, B, max_seg).keys;
    panoptic_kernel<<<B, PAN_THREADS, pan_lds_bytes(max_inst, num_classes, max_seg), (hipStream_t)stream>>>(P);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
