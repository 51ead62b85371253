// On-device instance extraction for the instance / panoptic evaluation scripts (gfx950):
//   mu_argmax_prob  softmax(outputs / T) + argmax of evaluate_instances (ade_instance.py:407-411) in ONE read of the logits;
//   mu_instances    get_instances_from_mask (ade_instance.py:367-397) and generate_instance_mask (ade_panoptic.py:36-47):
//                   8-connected components per class, per-instance bbox / area / mean probability, and the score order of
//                   sorted(..., key=score, reverse=True) (ade_instance.py:417-419).
// Scheme (DESIGN.md "Instance extraction"): one workgroup per image.
//   label kernel  union-find over 16-bit links held in LDS (2 bytes per pixel: 128 KiB at the 65536-pixel limit).  Links always
//                 point to a smaller raster index, so a component's root is its first pixel in raster order and the instance ids are
//                 an exclusive scan over root flags.
//   stats kernel  integer LDS atomics per instance (area, bbox, 2^-24 fixed-point probability sum: order-independent, so scores
//                 are bit-identical from run to run), class_rank, and a bitonic sort of (score desc, id asc) keys in LDS.
#include "wave_prims.h"

#define INST_THREADS 1024
#define INST_WAVES (INST_THREADS / 64)
#define INST_MAX_PIXELS 65536
#define INST_MAX_INSTANCES 4096

// ------------------------------------------------------------------------------------------
// arg-max + probability of the arg-max class.  Element (pixel r, class c) at
//   logits[(r / inner) * outer_stride + c * c_stride + (r % inner) * p_stride]            (the convention of mu_mean_iou, loss.hip)
// One thread per pixel walks the channels in ascending order with an online maximum and sum, so NCHW (lanes along pixels:
// coalesced) and NHWC (16-byte loads along channels) do the SAME arithmetic per pixel and agree bit for bit.
//   first maximum wins (strict >, as torch.argmax / mu_mean_iou);  prob = 1 / sum_c exp((x_c - x_max) / T)
// Logits are assumed finite (inf - inf in the running update would give NaN).
// ------------------------------------------------------------------------------------------
struct ArgmaxState {
    float m, k;             // running maximum; k = log2(e) / T
    double s;               // sum of exp2((x - m) * k).  fp64: an fp32 running sum near 1 drops every term below 2^-25, and with 150
                            // classes the dropped tail reaches several 1e-6 of the probability.  Costs a convert and an fp64 add
                            // per channel and one fp64 divide per pixel (not timed apart from the pass)
    int arg;
    __device__ __forceinline__ void first(float v) { m = v; s = 1.0; arg = 0; }
    __device__ __forceinline__ void next(float v, int c) {
        if (v > m) {
            s = s * (double)__builtin_amdgcn_exp2f((m - v) * k) + 1.0;
            m = v;
            arg = c;
        } else {
            s += (double)__builtin_amdgcn_exp2f((v - m) * k);
        }
    }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void argmax_prob_kernel(const T* __restrict__ logits, long M, int C, long inner, long outer_stride,
                                                          long c_stride, long p_stride, float k, int* __restrict__ cls,
                                                          float* __restrict__ prob) {
    constexpr int V = 16 / sizeof(T);              // elements per 16-byte load
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < M; r += (long)gridDim.x * 256) {
        const T* base = logits + (r / inner) * outer_stride + (r % inner) * p_stride;
        ArgmaxState st;
        st.k = k;
        if (VEC) {                                  // c_stride == 1, rows 16-byte aligned: vector loads along the channels
            typedef T TV __attribute__((ext_vector_type(V)));
            const int Cv = C / V * V;
            for (int c0 = 0; c0 < Cv; c0 += V) {
                const TV v = *(const TV*)(base + c0);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (c0 + j == 0) st.first((float)v[j]);
                    else st.next((float)v[j], c0 + j);
                }
            }
            for (int c = Cv; c < C; ++c) {
                if (c == 0) st.first((float)base[c]);
                else st.next((float)base[c], c);
            }
        } else {                                    // strided channels: four independent loads in flight, then the ordered update
            st.first((float)base[0]);
            int c = 1;
            for (; c + 4 <= C; c += 4) {
                const float v0 = (float)base[(long)c * c_stride], v1 = (float)base[(long)(c + 1) * c_stride];
                const float v2 = (float)base[(long)(c + 2) * c_stride], v3 = (float)base[(long)(c + 3) * c_stride];
                st.next(v0, c);
                st.next(v1, c + 1);
                st.next(v2, c + 2);
                st.next(v3, c + 3);
            }
            for (; c < C; ++c) st.next((float)base[(long)c * c_stride], c);
        }
        cls[r] = st.arg;
        if (prob) prob[r] = (float)(1.0 / st.s);
    }
}

template <typename T>
static int argmax_prob_launch(const void* logits, long M, int C, long inner, long outer_stride, long c_stride, long p_stride, float k,
                              int* cls, float* prob, hipStream_t st) {
    constexpr long V = 16 / sizeof(T);
    const bool vec = c_stride == 1 && p_stride % V == 0 && outer_stride % V == 0 && ((uintptr_t)logits & 15) == 0;
    const long blocks = (M + 255) / 256;
    const int g = (int)(blocks > 65536 ? 65536 : blocks);
    if (vec) argmax_prob_kernel<T, true><<<g, 256, 0, st>>>((const T*)logits, M, C, inner, outer_stride, c_stride, p_stride, k, cls, prob);
    else argmax_prob_kernel<T, false><<<g, 256, 0, st>>>((const T*)logits, M, C, inner, outer_stride, c_stride, p_stride, k, cls, prob);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

extern "C" int mu_argmax_prob(const void* logits, long M, int C, long inner, long outer_stride, long c_stride, long p_stride,
                              float inv_temperature, int* cls, float* prob_or_null, int dtype, void* stream) {
    if (!logits || !cls || M <= 0 || C <= 0 || inner <= 0 || !(inv_temperature > 0.f)) return MU_ERR_ARG;
    if (dtype != MU_F32 && dtype != MU_F16) return MU_ERR_ARG;
    const float k = inv_temperature * 1.44269504088896340736f;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MU_F16) return argmax_prob_launch<h16>(logits, M, C, inner, outer_stride, c_stride, p_stride, k, cls, prob_or_null, st);
    return argmax_prob_launch<float>(logits, M, C, inner, outer_stride, c_stride, p_stride, k, cls, prob_or_null, st);
}

// ------------------------------------------------------------------------------------------
// Labelling: union-find with 16-bit links in LDS.
// ------------------------------------------------------------------------------------------
typedef unsigned short u16;

__device__ __forceinline__ unsigned uf_find(const volatile u16* p, unsigned x) {
    for (;;) {
        const unsigned q = p[x];
        if (q == x) return x;
        x = q;
    }
}

// compare-and-swap on one 16-bit link through the 32-bit word that holds it (LDS has no 16-bit atomics); returns the link's
// previous value.  A neighbour changing the other half of the word only costs a retry.
__device__ __forceinline__ unsigned uf_cas16(u16* p, unsigned idx, unsigned expect, unsigned val) {
    unsigned* w = (unsigned*)p + (idx >> 1);
    const unsigned sh = (idx & 1u) * 16u;
    unsigned old = *(volatile unsigned*)w;
    for (;;) {
        const unsigned cur = (old >> sh) & 0xffffu;
        if (cur != expect) return cur;
        const unsigned nw = (old & ~(0xffffu << sh)) | (val << sh);
        const unsigned prev = atomicCAS(w, old, nw);
        if (prev == old) return cur;
        old = prev;
    }
}

// hook the larger root under the smaller one; only roots are ever re-linked, so every link points to a smaller index of the
// same component at all times.  No thread waits for another: a failed CAS means someone else made progress.
__device__ __forceinline__ void uf_unite(u16* p, unsigned a, unsigned b) {
    for (;;) {
        a = uf_find(p, a);
        b = uf_find(p, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = uf_cas16(p, a, a, b);
        if (old == a) return;
        a = old;
    }
}

// cls[B][N] -> ids[B][N] (1..count in raster order of the first pixel, 0 = background), count[B], first[B][max_inst] (first pixel
// of ids 1..max_inst).  Dynamic LDS: u16 parent[N rounded up to 2] then unsigned wave_total[INST_WAVES].
__global__ __launch_bounds__(INST_THREADS) void inst_label_kernel(const int* __restrict__ cls_all, int N, int W, int max_inst,
                                                                   int* __restrict__ ids_all, int* __restrict__ count,
                                                                   int* __restrict__ first_all) {
    extern __shared__ unsigned inst_lds[];
    u16* parent = (u16*)inst_lds;
    unsigned* wave_total = inst_lds + ((N + 1) >> 1);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* cls = cls_all + (long)b * N;
    int* ids = ids_all + (long)b * N;
    int* first = first_all + (long)b * max_inst;

    // 1. horizontal runs inside each 64-pixel chunk: every pixel links to the start of its run (no chains along rows)
    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const int i = base + lane;
        const bool valid = i < N;
        const int c = valid ? cls[i] : 0;
        const bool link = valid && c > 0 && (i % W) > 0 && cls[i - 1] == c;
        const unsigned long long mask = __ballot(link);
        const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const unsigned long long zeros = ~mask & upto;                 // pixels at or before this lane that start a run
        const int start = zeros ? 63 - __builtin_clzll(zeros) : 0;     // none: the run comes in from the previous chunk
        if (valid) parent[i] = (u16)(base + start);
    }
    __syncthreads();

    // 2. unions across chunk borders and with the row above.  A union is skipped where the pixel to the left (or right) makes the
    //    same connection: with W and NW of the class, i-1 ~ NW and NW ~ N already; with E of the class, E unites with NE itself.
    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const int i = base + lane;
        if (i >= N) continue;
        const int c = cls[i];
        if (c <= 0) continue;
        const int x = i % W;
        const bool w = x > 0 && cls[i - 1] == c;
        if (lane == 0 && w) uf_unite(parent, i, i - 1);
        if (i < W) continue;
        if (cls[i - W] == c) {
            const bool nw = x > 0 && cls[i - W - 1] == c;
            if (!(w && nw)) uf_unite(parent, i, i - W);
        } else {
            if (x > 0 && !w && cls[i - W - 1] == c) uf_unite(parent, i, i - W - 1);
            if (x < W - 1 && cls[i - W + 1] == c && cls[i + 1] != c) uf_unite(parent, i, i - W + 1);
        }
    }
    __syncthreads();

    // 3. flatten, in raster order: ancestors have smaller indices, so most chains are already short when a pixel is reached
    for (int i = tid; i < N; i += INST_THREADS) {
        const unsigned r = uf_find(parent, i);
        parent[i] = (u16)r;          // a concurrent reader sees the old link or the root: both are ancestors
    }
    __syncthreads();

    // 4. ids = exclusive scan of the root flags in raster order, every wave over its segment of the pixels
    int lo, hi;
    wave_segment(N, INST_WAVES, wave, lo, hi);
    unsigned mine = 0, total;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool root = i < hi && parent[i] == i && cls[i] > 0;
        mine += __popcll(__ballot(root));
    }
    unsigned running = block_exclusive_base(mine, wave_total, lane, wave, INST_WAVES, total);
    if (tid == 0) count[b] = (int)total;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool valid = i < hi;
        const bool fg = valid && cls[i] > 0;
        const bool root = fg && parent[i] == i;
        const unsigned id = wave_flag_rank(root, lane, running) + 1u;
        if (root) {
            ids[i] = (int)id;
            if (id <= (unsigned)max_inst) first[id - 1] = i;
        } else if (valid && !fg) {
            ids[i] = 0;
        }
    }
    __syncthreads();                 // the roots' ids (global memory, same workgroup) are visible past this barrier
    for (int i = tid; i < N; i += INST_THREADS) {
        const unsigned r = parent[i];
        if (r != (unsigned)i) ids[i] = ids[r];
    }
}

// ------------------------------------------------------------------------------------------
// Per-instance statistics, table, score order.  The class of an instance is inst_cls[k] where the caller has one per id (id maps: the
// median), else the class of its first pixel (components of one class).  Dynamic LDS, P = max_inst rounded up to a power of two:
//   unsigned long long acc[P] (fixed-point sums, then the sort keys);  unsigned area[P], xmin[P], ymin[P], xmax[P], ymax[P]
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long prob_fixed(float p) {      // round(p * 2^24), two's complement
    return (unsigned long long)(long long)__float2ll_rn(p * 16777216.f);
}

__global__ __launch_bounds__(INST_THREADS) void inst_stats_kernel(const int* __restrict__ cls_all, const float* __restrict__ prob_all,
                                                                   const int* __restrict__ ids_all, const int* __restrict__ count,
                                                                   const int* __restrict__ first_all,
                                                                   const int* __restrict__ inst_cls_all, int N, int W, int max_inst,
                                                                   int P, int* __restrict__ table_all, float* __restrict__ score_all,
                                                                   int* __restrict__ order_all) {
    extern __shared__ unsigned inst_lds[];
    unsigned long long* acc = (unsigned long long*)inst_lds;      // first: 8-byte aligned for every P (P = 1 included)
    unsigned* area = inst_lds + 2 * P;
    unsigned* xmin = area + P;
    unsigned* ymin = xmin + P;
    unsigned* xmax = ymin + P;
    unsigned* ymax = xmax + P;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* cls = cls_all + (long)b * N;
    const int* ids = ids_all + (long)b * N;
    const float* prob = prob_all ? prob_all + (long)b * N : nullptr;
    const int* first = first_all + (long)b * max_inst;
    const int* inst_cls = inst_cls_all ? inst_cls_all + (long)b * max_inst : nullptr;      // null: the class of the first pixel
    int* table = table_all + (long)b * max_inst * 8;
    float* score = score_all + (long)b * max_inst;
    int* order = order_all + (long)b * max_inst;
    const int K = min(count[b], max_inst);

    for (int k = tid; k < P; k += INST_THREADS) {
        area[k] = 0;
        xmin[k] = 0x7fffffffu;
        ymin[k] = 0x7fffffffu;
        xmax[k] = 0;
        ymax[k] = 0;
        acc[k] = 0;
    }
    __syncthreads();

    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const int i = base + lane;
        const bool valid = i < N;
        const int id = valid ? ids[i] : 0;
        const bool active = id > 0 && id <= K;
        const unsigned x = (unsigned)(i % W), y = (unsigned)(i / W);
        const unsigned long long q = (active && prob) ? prob_fixed(prob[i]) : 0ull;
        const int id0 = __shfl(id, 0);
        if (__ballot(valid && id == id0) == ~0ull) {          // the whole wave inside one instance: one set of atomics per wave
            if (id0 > 0 && id0 <= K) {
                const unsigned x0 = wave_min(x), x1 = wave_max(x), y0 = wave_min(y), y1 = wave_max(y);
                const unsigned long long qs = wave_sum(q);
                if (lane == 0) {
                    const int k = id0 - 1;
                    atomicAdd(&area[k], 64u);
                    atomicMin(&xmin[k], x0);
                    atomicMax(&xmax[k], x1);
                    atomicMin(&ymin[k], y0);
                    atomicMax(&ymax[k], y1);
                    if (prob) atomicAdd(&acc[k], qs);
                }
            }
        } else if (active) {
            const int k = id - 1;
            atomicAdd(&area[k], 1u);
            atomicMin(&xmin[k], x);
            atomicMax(&xmax[k], x);
            atomicMin(&ymin[k], y);
            atomicMax(&ymax[k], y);
            if (prob) atomicAdd(&acc[k], q);
        }
    }
    __syncthreads();

    // table columns 0..6, scores, sort keys; xmin[] is re-used for the class of the instance (class_rank below)
    for (int k = tid; k < P; k += INST_THREADS) {
        unsigned long long key = ~0ull;                        // padding sorts last
        int c = 0;
        if (k < K) {
            const int f = first[k];
            c = inst_cls ? inst_cls[k] : cls[f];
            const float s = prob ? (float)((double)(long long)acc[k] / ((double)area[k] * 16777216.0)) : 1.f;
            int* row = table + (long)k * 8;
            row[0] = c;
            row[1] = (int)area[k];
            row[2] = (int)xmin[k];
            row[3] = (int)ymin[k];
            row[4] = (int)xmax[k];
            row[5] = (int)ymax[k];
            row[6] = f;
            score[k] = s;
            key = score_order_key(s, k);
        } else if (k < max_inst) {
            int* row = table + (long)k * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) row[j] = 0;
            score[k] = 0.f;
        }
        acc[k] = key;
        xmin[k] = (unsigned)c;
    }
    __syncthreads();

    // class_rank: 1-based rank among the instances of the same class, in id order (what generate_instance_mask writes)
    for (int k = tid; k < K; k += INST_THREADS) {
        const unsigned c = xmin[k];
        int rank = 1;
        for (int j = 0; j < k; ++j) rank += (xmin[j] == c);
        table[(long)k * 8 + 7] = rank;
    }

    // the keys in ascending order, over the power of two that holds K
    int S = 1;
    while (S < K) S <<= 1;
    block_sort_u64(acc, S, tid, INST_THREADS);
    for (int k = tid; k < max_inst; k += INST_THREADS) order[k] = k < K ? (int)(unsigned)(acc[k] & 0xffffffffull) : 0;
}

// Dynamic LDS of the two kernels that need a grant (common.h: mu_lds_grant), and the most each can ever ask for
static constexpr size_t inst_label_lds(int N) { return (size_t)((N + 1) >> 1) * 4 + INST_WAVES * sizeof(unsigned); }
static constexpr size_t inst_stats_lds(int P) { return (size_t)P * (5 * sizeof(unsigned) + sizeof(unsigned long long)); }
#define INST_LDS_LABEL_MAX ((int)inst_label_lds(INST_MAX_PIXELS))
#define INST_LDS_STATS_MAX ((int)inst_stats_lds(INST_MAX_INSTANCES))
static_assert(INST_LDS_LABEL_MAX == INST_MAX_PIXELS * 2 + INST_WAVES * 4 && INST_LDS_STATS_MAX == INST_MAX_INSTANCES * 28, "the grants");
static bool inst_stats_granted() { return mu_lds_grant<inst_stats_kernel>(INST_LDS_STATS_MAX); }

extern "C" int mu_instances_supported(int H, int W, int max_inst) {
    if (H <= 0 || W <= 0 || (long)H * W > INST_MAX_PIXELS) return MU_ERR_SHAPE;
    if (max_inst < 1 || max_inst > INST_MAX_INSTANCES) return MU_ERR_SHAPE;
    return MU_OK;
}

struct InstancesWs {
    MuCarve c;
    int* first;     // [B][max_inst] first pixel of every instance: the label kernel's hand-over to the statistics kernel
    constexpr InstancesWs(void* ws, int B, int max_inst) : c(ws), first(c.take<int>((long)B * max_inst)) {}
};
static_assert(InstancesWs(nullptr, 2, 5).c.bytes == 2 * 5 * 4 && InstancesWs(nullptr, 3, 4096).c.bytes == 3 * 4096 * 4, "mu_instances workspace");

extern "C" long mu_instances_workspace_bytes(int B, int H, int W, int max_inst) {
    if (B <= 0 || mu_instances_supported(H, W, max_inst) != MU_OK) return 0;
    return InstancesWs(nullptr, B, max_inst).c.bytes;
}

extern "C" int mu_instances(const int* cls, const float* prob_or_null, int B, int H, int W, int max_inst, int* ids, int* table,
                            float* score, int* count, int* order, void* workspace, long ws_bytes, void* stream) {
    if (!cls || !ids || !table || !score || !count || !order || !workspace || B <= 0 || H <= 0 || W <= 0) return MU_ERR_ARG;
    if (mu_instances_supported(H, W, max_inst) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_instances_workspace_bytes(B, H, W, max_inst)) return MU_ERR_WORKSPACE;
    if (!mu_lds_grant<inst_label_kernel>(INST_LDS_LABEL_MAX) || !inst_stats_granted()) return MU_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    const int N = H * W, P = mu_pow2(max_inst);
    const InstancesWs ws(workspace, B, max_inst);
    inst_label_kernel<<<B, INST_THREADS, inst_label_lds(N), st>>>(cls, N, W, max_inst, ids, count, ws.first);
    MU_CHECK_LAUNCH();
    inst_stats_kernel<<<B, INST_THREADS, inst_stats_lds(P), st>>>(cls, prob_or_null, ids, count, ws.first, nullptr, N, W, max_inst, P, table,
                                                                   score, order);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// mu_dbscan_instances: instances of the 3-head model from its embedding head, get_instances_from_embeddings + get_instance_annotations
// (city_instance.py:405-449): per image and class c >= 1, sklearn's DBSCAN(eps, min_samples) over the class's pixel embeddings.
// Contract: points of a class in raster order; i ~ j iff sum_k (double(a_k) - double(b_k))^2 <= double(eps)^2; core =
// at least min_samples neighbours (itself included); a cluster = a connected component of core points, ordered by its lowest core
// point; a non-core point joins the first cluster that holds a core neighbour of it, else it is noise (id 0).
//
// The neighbour decision is plain fp64 VALU (sub + fma per dimension): fp32 and fp16 values widen exactly, so the decision is the
// contract's for both and for every layout.  Kernels, all stream-ordered, nothing read back:
//   group   one workgroup per image: stable counting sort of the pixels by class -> perm (class ascending, raster within a class),
//           pos_of (its inverse, -1 = background), seg[c] (start of class c in perm), one tile descriptor per DB_TR points of a class;
//   sweep   grid (worst-case tiles, B), early exit past ntiles[b].  A workgroup keeps DB_TR points of one class in registers (one per
//           lane) and streams the class's points through LDS in chunks of DB_TC; every lane reads the same column value (broadcast).
//             COUNT   neighbours per row point -> link[pos] = pos (core) or -1;
//             UNION   core x core, column < row: union-find on link[] in global memory.  Only roots are re-linked, by CAS, always to the
//                     smaller index (the discipline of inst_label_kernel), so a cluster's root is its lowest core point whatever the
//                     order; every access to link[] that can race is an agent-scope atomic.  A pair is skipped when the column's link
//                     (snapshot in LDS) equals the row's last known root: both are ancestors, so the two are already joined;
//             BORDER  lab[pos] = root (core), min root over the core neighbours (border) or -1 (noise); link[] is only read here;
//   number  one workgroup per image: ids = exclusive scan of the root flags in perm order, scattered through pos_of; first pixel of
//           each id by integer atomicMin in LDS (a border pixel may precede the root); then inst_stats_kernel as for mu_instances.
// Tile sizes.  DB_TR = 256: one row point per lane holds DP doubles in registers (DP = D padded to 4 / 16 / 32 / 64: up to 128
// VGPRs), four waves share one LDS chunk.  DB_TC = 64: 64 x DP doubles = 8 KiB at DP = 16, 32 KiB at DP = 64, so at least four
// workgroups fit a CU's 160 KiB; per column the inner loop is one broadcast LDS read of 16 bytes per two dimensions against four
// fp64 VALU instructions, i.e. VALU-bound (fp64 runs at a quarter of a wave per cycle, the LDS serves a broadcast read in one).
// ------------------------------------------------------------------------------------------
#define DB_TR 256
#define DB_TC 64
#define DB_GROUP_THREADS 512
#define DB_GROUP_WAVES (DB_GROUP_THREADS / 64)
#define DB_MAX_CLASSES 1024
#define DB_MAX_D 64

struct DbParams {
    const void* emb;
    int N, D, nc, max_tiles, min_samples;
    long inner, outer_stride, c_stride, p_stride;
    double eps2;
    int *perm, *pos_of, *link, *lab, *seg, *tiles, *ntiles;      // per image: N, N, N, N, nc + 1, 2 * max_tiles, 1 ints
};

// Dynamic LDS: int wcnt[DB_GROUP_WAVES][nc], start[nc], cnt[nc], toff[nc]   (44 KiB at 1024 classes)
__global__ __launch_bounds__(DB_GROUP_THREADS) void db_group_kernel(const int* __restrict__ cls_all, DbParams P) {
    extern __shared__ unsigned inst_lds[];
    const int N = P.N, nc = P.nc;
    int* wcnt = (int*)inst_lds;
    int* start = wcnt + DB_GROUP_WAVES * nc;
    int* cnt = start + nc;
    int* toff = cnt + nc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* cls = cls_all + (long)b * N;
    int* perm = P.perm + (long)b * N;
    int* pos_of = P.pos_of + (long)b * N;
    int* seg = P.seg + (long)b * (nc + 1);
    int* tiles = P.tiles + (long)b * P.max_tiles * 2;

    for (int k = tid; k < DB_GROUP_WAVES * nc; k += DB_GROUP_THREADS) wcnt[k] = 0;
    __syncthreads();

    // 1. per wave and class: pixels of the wave's raster range [lo, hi).  The counters of a wave are its own: no atomics.
    int lo, hi;
    wave_segment(N, DB_GROUP_WAVES, wave, lo, hi);
    int* mine = wcnt + wave * nc;
    for (int base = lo; base < hi; base += 64) {
        const int c = base + lane < hi ? cls[base + lane] : 0;
        wave_sort_chunk<false>(c, c >= 1 && c < nc, lane, mine);
    }
    __syncthreads();

    // 2. per class: exclusive prefix over the waves, total
    for (int c = tid; c < nc; c += DB_GROUP_THREADS) {
        int run = 0;
        for (int v = 0; v < DB_GROUP_WAVES; ++v) {
            const int t = wcnt[v * nc + c];
            wcnt[v * nc + c] = run;
            run += t;
        }
        cnt[c] = run;
    }
    __syncthreads();

    // 3. wave 0: exclusive scans over the classes of the point counts (segment starts) and of the tile counts
    if (wave == 0) {
        for (int c = lane; c < nc; c += 64) toff[c] = (cnt[c] + DB_TR - 1) / DB_TR;
        const int n_all = wave_scan_excl_array(cnt, start, nc, lane), t_all = wave_scan_excl_array(toff, toff, nc, lane);
        for (int c = lane; c < nc; c += 64) seg[c] = start[c];
        if (lane == 0) {
            seg[nc] = n_all;
            P.ntiles[b] = t_all;
        }
    }
    __syncthreads();

    // 4. tile descriptors (class, first point); the waves' counters become absolute positions.
    //    sum_c ceil(n_c / DB_TR) <= N / DB_TR + (classes with points) <= max_tiles
    for (int c = tid; c < nc; c += DB_GROUP_THREADS) {
        const int n = cnt[c], s = start[c], t0 = toff[c];
        for (int k = 0; k * DB_TR < n; ++k) {
            tiles[2 * (t0 + k)] = c;
            tiles[2 * (t0 + k) + 1] = s + k * DB_TR;
        }
        for (int v = 0; v < DB_GROUP_WAVES; ++v) wcnt[v * nc + c] += s;
    }
    __syncthreads();

    // 5. placement, stable: the same walk as step 1
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const int c = i < hi ? cls[i] : 0;
        const bool fg = c >= 1 && c < nc;
        const int pos = wave_sort_chunk<true>(c, fg, lane, mine);
        if (fg) perm[pos] = i;
        if (i < hi) pos_of[i] = fg ? pos : -1;
    }
}

__device__ __forceinline__ int db_find(const int* p, int x) {
    for (;;) {
        const int q = mu_ld_agent(p + x);
        if (q == x) return x;
        x = q;                               // links strictly decrease along a chain
    }
}
// joins the sets of a and b; returns a common ancestor of both (the root at the time of the call)
__device__ __forceinline__ int db_unite(int* p, int a, int b) {
    for (;;) {
        a = db_find(p, a);
        b = db_find(p, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(p + a, a, b);         // agent scope; fails only if someone else re-linked the root a: progress
        if (old == a) return b;
        a = old;
    }
}
__device__ __forceinline__ int db_find_plain(const int* p, int x) {      // no writer in the same kernel
    for (;;) {
        const int q = p[x];
        if (q == x) return x;
        x = q;
    }
}

enum { DB_COUNT = 0, DB_UNION = 1, DB_BORDER = 2 };

template <typename T, int DP, int MODE>
__global__ __launch_bounds__(DB_TR) void db_sweep_kernel(DbParams P) {
    __shared__ double cols[DB_TC * DP];
    __shared__ long poff[DB_TC];
    __shared__ int lk[DB_TC];
    const int b = blockIdx.y, tid = threadIdx.x;
    if ((int)blockIdx.x >= P.ntiles[b]) return;
    const int N = P.N, D = P.D;
    const int* td = P.tiles + ((long)b * P.max_tiles + blockIdx.x) * 2;
    const int c = td[0], row0 = td[1];
    const int* seg = P.seg + (long)b * (P.nc + 1);
    const int s0 = seg[c], s1 = seg[c + 1];
    const int* perm = P.perm + (long)b * N;
    int* link = P.link + (long)b * N;
    const T* emb = (const T*)P.emb;
    const long cs = P.c_stride;

    const int gi = row0 + tid;
    const bool rvalid = gi < s1;
    int mylink = 0;
    if (MODE != DB_COUNT) mylink = rvalid ? link[gi] : 0;
    bool active = rvalid;
    if (MODE == DB_UNION) active = rvalid && mylink >= 0;
    if (MODE == DB_BORDER) {
        active = rvalid && mylink < 0;
        if (rvalid && mylink >= 0) P.lab[(long)b * N + gi] = db_find_plain(link, gi);
    }
    if (MODE != DB_COUNT && !__syncthreads_or(active)) return;

    double r[DP];
    {
        long off = 0;
        if (rvalid) {
            const long g = (long)b * N + perm[gi];
            off = (g / P.inner) * P.outer_stride + (g % P.inner) * P.p_stride;
        }
#pragma unroll
        for (int k = 0; k < DP; ++k) r[k] = (rvalid && k < D) ? (double)(float)emb[off + k * cs] : 0.0;
    }

    int acc_i = MODE == DB_BORDER ? 0x7fffffff : (MODE == DB_UNION ? gi : 0);      // neighbour count / last known root / min root
    const int c_end = MODE == DB_UNION ? min(s1, row0 + DB_TR) : s1;                // UNION: only columns below the rows
    for (int c0 = s0; c0 < c_end; c0 += DB_TC) {
        const int jn = min(DB_TC, c_end - c0);
        __syncthreads();                        // the previous chunk has been consumed
        if (tid < DB_TC) {
            long off = 0;
            int l = -1;
            if (tid < jn) {
                const long g = (long)b * N + perm[c0 + tid];
                off = (g / P.inner) * P.outer_stride + (g % P.inner) * P.p_stride;
                if (MODE == DB_UNION) l = link[c0 + tid];              // a hint: any value seen here is an ancestor (or -1: not core)
                if (MODE == DB_BORDER) {
                    l = link[c0 + tid];
                    if (l >= 0) l = db_find_plain(link, l);
                }
            }
            poff[tid] = off;
            lk[tid] = l;
        }
        __syncthreads();
        for (int e = tid; e < DB_TC * DP; e += DB_TR) {
            int j, k;
            if (cs == 1) { k = e % DP; j = e / DP; }                   // channels contiguous (NHWC)
            else { j = e % DB_TC; k = e / DB_TC; }                     // pixels contiguous (NCHW)
            cols[j * DP + k] = (j < jn && k < D) ? (double)(float)emb[poff[j] + k * cs] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            if (MODE != DB_COUNT && lk[j] < 0) continue;               // uniform: the column is not a core point
            const double* cj = cols + j * DP;
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < DP; ++k) {
                const double d = r[k] - cj[k];
                d2 = fma(d, d, d2);
            }
            const bool near = d2 <= P.eps2;
            if (MODE == DB_COUNT) {
                acc_i += near ? 1 : 0;
            } else if (MODE == DB_UNION) {
                const int gj = c0 + j;
                if (active && near && gj < gi && lk[j] != acc_i) {
                    const int root = db_unite(link, gi, gj);
                    // shorten both chains: root < x makes x a non-root for good, and non-roots are never the target of a CAS
                    if (root < gi) __hip_atomic_store(link + gi, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (root < gj) __hip_atomic_store(link + gj, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    acc_i = root;
                }
            } else {
                if (active && near) acc_i = min(acc_i, lk[j]);
            }
        }
    }
    if (MODE == DB_COUNT) {
        if (rvalid) link[gi] = acc_i >= P.min_samples ? gi : -1;
    } else if (MODE == DB_BORDER) {
        if (active) P.lab[(long)b * N + gi] = acc_i == 0x7fffffff ? -1 : acc_i;
    }
}

// Dynamic LDS: int first[max_inst], unsigned wave_total[INST_WAVES].  link[] is dead after the border sweep and takes the roots' ids.
__global__ __launch_bounds__(INST_THREADS) void db_number_kernel(DbParams P, int max_inst, int* __restrict__ ids_all,
                                                                  int* __restrict__ count, int* __restrict__ first_all) {
    extern __shared__ unsigned inst_lds[];
    int* first = (int*)inst_lds;
    unsigned* wave_total = inst_lds + max_inst;
    const int N = P.N;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* lab = P.lab + (long)b * N;
    const int* pos_of = P.pos_of + (long)b * N;
    int* rid = P.link + (long)b * N;
    int* ids = ids_all + (long)b * N;
    const int nfg = P.seg[(long)b * (P.nc + 1) + P.nc];

    for (int k = tid; k < max_inst; k += INST_THREADS) first[k] = 0x7fffffff;
    int lo, hi;
    wave_segment(nfg, INST_WAVES, wave, lo, hi);
    unsigned mine = 0, total;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        mine += __popcll(__ballot(i < hi && lab[i] == i));
    }
    unsigned running = block_exclusive_base(mine, wave_total, lane, wave, INST_WAVES, total);
    if (tid == 0) count[b] = (int)total;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool root = i < hi && lab[i] == i;
        const unsigned id = wave_flag_rank(root, lane, running) + 1u;
        if (root) rid[i] = (int)id;
    }
    __syncthreads();                 // the roots' ids (global memory, same workgroup) are visible past this barrier
    for (int i = tid; i < N; i += INST_THREADS) {
        const int pos = pos_of[i];
        int id = 0;
        if (pos >= 0) {
            const int l = lab[pos];
            if (l >= 0) id = rid[l];
        }
        ids[i] = id;
        if (id > 0 && id <= max_inst) atomicMin(&first[id - 1], i);
    }
    __syncthreads();
    for (int k = tid; k < max_inst; k += INST_THREADS) first_all[(long)b * max_inst + k] = first[k];
}

extern "C" int mu_dbscan_supported(int H, int W, int D, int num_classes, int max_inst) {
    if (H <= 0 || W <= 0 || (long)H * W > INST_MAX_PIXELS) return MU_ERR_SHAPE;
    if (D < 1 || D > DB_MAX_D || num_classes < 1 || num_classes > DB_MAX_CLASSES) return MU_ERR_SHAPE;
    if (max_inst < 1 || max_inst > INST_MAX_INSTANCES) return MU_ERR_SHAPE;
    return MU_OK;
}

static constexpr int db_max_tiles(int N, int num_classes) { return N / DB_TR + num_classes; }

struct DbscanWs {
    MuCarve c;
    int* perm;      // [B][N] pixels by class, raster order within a class
    int* pos_of;    // [B][N] its inverse, -1 = background
    int* link;      // [B][N] union-find parents of the core points
    int* lab;       // [B][N] root per point, -1 = noise
    int* seg;       // [B][num_classes + 1] start of every class in perm
    int* tiles;     // [B][max_tiles][2] tile descriptors
    int* ntiles;    // [B] tiles in use
    int* first;     // [B][max_inst] first pixel of every instance, for the statistics kernel
    constexpr DbscanWs(void* ws, int B, int N, int num_classes, int max_inst)
        : c(ws), perm(c.take<int>((long)B * N)), pos_of(c.take<int>((long)B * N)), link(c.take<int>((long)B * N)),
          lab(c.take<int>((long)B * N)), seg(c.take<int>((long)B * (num_classes + 1))),
          tiles(c.take<int>((long)B * db_max_tiles(N, num_classes) * 2)), ntiles(c.take<int>(B)), first(c.take<int>((long)B * max_inst)) {}
};
static_assert(DbscanWs(nullptr, 2, 63, 3, 5).c.bytes == 2L * (4 * 63 + 3 + 1 + 2 * (63 / DB_TR + 3) + 1 + 5) * 4 &&
              DbscanWs(nullptr, 3, 65536, 1024, 4096).c.bytes == 3L * (4 * 65536 + 1024 + 1 + 2 * (65536 / DB_TR + 1024) + 1 + 4096) * 4,
              "mu_dbscan_instances workspace");

extern "C" long mu_dbscan_workspace_bytes(int B, int H, int W, int num_classes, int max_inst) {
    if (B <= 0 || mu_dbscan_supported(H, W, 1, num_classes, max_inst) != MU_OK) return 0;
    return DbscanWs(nullptr, B, H * W, num_classes, max_inst).c.bytes;
}

// dynamic LDS of the group and number kernels (44 KiB and 16 KiB at the limits: no grant needed)
static size_t db_group_lds(int num_classes) { return (size_t)(DB_GROUP_WAVES + 3) * num_classes * sizeof(int); }
static size_t db_number_lds(int max_inst) { return (size_t)(max_inst + INST_WAVES) * sizeof(int); }

template <typename T, int DP>
static int db_sweeps(const DbParams& P, int B, hipStream_t st) {
    const dim3 grid(P.max_tiles, B);
    db_sweep_kernel<T, DP, DB_COUNT><<<grid, DB_TR, 0, st>>>(P);
    MU_CHECK_LAUNCH();
    db_sweep_kernel<T, DP, DB_UNION><<<grid, DB_TR, 0, st>>>(P);
    MU_CHECK_LAUNCH();
    db_sweep_kernel<T, DP, DB_BORDER><<<grid, DB_TR, 0, st>>>(P);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

template <typename T>
static int db_sweeps_d(const DbParams& P, int B, hipStream_t st) {
    if (P.D <= 4) return db_sweeps<T, 4>(P, B, st);
    if (P.D <= 16) return db_sweeps<T, 16>(P, B, st);
    if (P.D <= 32) return db_sweeps<T, 32>(P, B, st);
    return db_sweeps<T, 64>(P, B, st);
}

extern "C" int mu_dbscan_instances(const int* cls, const void* emb, int B, int H, int W, int D, long inner, long outer_stride,
                                   long c_stride, long p_stride, int dtype, int num_classes, float eps, int min_samples, int max_inst,
                                   int* ids, int* table, float* score, int* count, int* order, void* workspace, long ws_bytes,
                                   void* stream) {
    if (!cls || !emb || !ids || !table || !score || !count || !order || !workspace || B <= 0 || H <= 0 || W <= 0 || inner <= 0)
        return MU_ERR_ARG;
    if (dtype != MU_F32 && dtype != MU_F16) return MU_ERR_ARG;
    if (mu_dbscan_supported(H, W, D, num_classes, max_inst) != MU_OK || min_samples < 1 || !(eps > 0.f) || B > 65535) return MU_ERR_SHAPE;
    if (ws_bytes < mu_dbscan_workspace_bytes(B, H, W, num_classes, max_inst)) return MU_ERR_WORKSPACE;
    if (!inst_stats_granted()) return MU_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    const int N = H * W, PW = mu_pow2(max_inst);
    const DbscanWs ws(workspace, B, N, num_classes, max_inst);
    DbParams P;
    P.emb = emb;
    P.N = N;
    P.D = D;
    P.nc = num_classes;
    P.max_tiles = db_max_tiles(N, num_classes);
    P.min_samples = min_samples;
    P.inner = inner;
    P.outer_stride = outer_stride;
    P.c_stride = c_stride;
    P.p_stride = p_stride;
    P.eps2 = (double)eps * (double)eps;
    P.perm = ws.perm;
    P.pos_of = ws.pos_of;
    P.link = ws.link;
    P.lab = ws.lab;
    P.seg = ws.seg;
    P.tiles = ws.tiles;
    P.ntiles = ws.ntiles;
    db_group_kernel<<<B, DB_GROUP_THREADS, db_group_lds(num_classes), st>>>(cls, P);
    MU_CHECK_LAUNCH();
    const int rc = with_storage(dtype, [&](auto tag) -> int { return db_sweeps_d<decltype(tag)>(P, B, st); });
    if (rc != MU_OK) return rc;
    db_number_kernel<<<B, INST_THREADS, db_number_lds(max_inst), st>>>(P, max_inst, ids, count, ws.first);
    MU_CHECK_LAUNCH();
    inst_stats_kernel<<<B, INST_THREADS, inst_stats_lds(PW), st>>>(cls, nullptr, ids, count, ws.first, nullptr, N, W, max_inst, PW, table, score,
                                                                    order);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// Instance matching: the second half of evaluate_instances / evaluate_panoptic_metrics, restated from the published
// algorithms (COCOeval.evaluateImg, maskUtils.iou, panopticapi's pq_compute_single_core) on id maps instead of RLE masks.
//   mu_instance_pairs   the intersection counts of two id maps as a table sorted by (pred id, gt id);
//   mu_instance_match   COCO's greedy matching per (image, class, threshold) and the panoptic IoU > 0.5 matching over that table.
//
// Pair table: one workgroup per image, no sort and no hash.  A bitmap over (pred id, gt id) IS the sorted set: bit g of row p - 1 says
// that the pair occurs, and the number of set bits before it is the pair's row in the output.
//   1. zero the bitmap; every run of equal (p, g) inside a 64-pixel chunk (one ballot, as inst_stats_kernel) sets its bit: atomicOr;
//   2. exclusive scan of the words' popcounts -> pre[]; every set bit writes its (p, g, 0) row; rows past the total are zeroed;
//   3. the runs again: row = pre[word] + popcount(bits below), atomicAdd of the run length.
// Integer atomics only, and neither the set of bits nor the sums depend on their order: bit-identical from run to run.  At most one
// new pair per pixel, so H*W rows always suffice.
// ------------------------------------------------------------------------------------------
#define MATCH_MAX_CLASSES 1024
#define MATCH_MAX_T 32

// key of pixel i: (p << 13) | g with ids outside 1..max folded to 0; 0 past the image
__device__ __forceinline__ unsigned pair_key(const int* __restrict__ pred, const int* __restrict__ gt, int i, int N, int mp, int mg) {
    if (i >= N) return 0u;
    int p = pred[i], g = gt[i];
    if (p < 1 || p > mp) p = 0;
    if (g < 1 || g > mg) g = 0;
    return ((unsigned)p << 13) | (unsigned)g;
}

__global__ __launch_bounds__(INST_THREADS) void inst_pairs_kernel(const int* __restrict__ pred_all, const int* __restrict__ gt_all, int N,
                                                                   int mp, int mg, int GW, unsigned* __restrict__ bits_all,
                                                                   unsigned* __restrict__ pre_all, int* __restrict__ pairs_all,
                                                                   int* __restrict__ n_pairs) {
    __shared__ unsigned wave_total[INST_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* pred = pred_all + (long)b * N;
    const int* gt = gt_all + (long)b * N;
    const int NW = mp * GW;                           // at most 4096 * 129 words
    unsigned* bits = bits_all + (long)b * NW;
    unsigned* pre = pre_all + (long)b * NW;
    int* pairs = pairs_all + (long)b * N * 3;

    for (int w = tid; w < NW; w += INST_THREADS) bits[w] = 0u;
    __syncthreads();

    // 1. which pairs occur
    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const unsigned key = pair_key(pred, gt, base + lane, N, mp, mg);
        const unsigned prev = (unsigned)__shfl_up((int)key, 1);
        if ((key >> 13) != 0u && (lane == 0 || key != prev)) {
            const unsigned g = key & 0x1fffu;
            atomicOr(&bits[((key >> 13) - 1u) * GW + (g >> 5)], 1u << (g & 31u));
        }
    }
    __syncthreads();

    // 2. rows, every wave over its segment of the words (bits[]: written by atomics of other waves)
    int lo, hi;
    wave_segment(NW, INST_WAVES, wave, lo, hi);
    unsigned mine = 0, total;
    for (int base = lo; base < hi; base += 64) {
        const int w = base + lane;
        mine += w < hi ? __popc(mu_ld_agent(bits + w)) : 0;
    }
    unsigned running = block_exclusive_base(wave_sum(mine), wave_total, lane, wave, INST_WAVES, total);
    if (tid == 0) n_pairs[b] = (int)total;
    for (int base = lo; base < hi; base += 64) {
        const int w = base + lane;
        unsigned word = w < hi ? mu_ld_agent(bits + w) : 0u;
        unsigned row = wave_scan_excl((unsigned)__popc(word), lane, running);
        if (w < hi) pre[w] = row;
        const int p = w / GW + 1, g0 = (w % GW) * 32;
        while (word) {
            const int bit = __ffs((int)word) - 1;
            word &= word - 1u;
            int* r = pairs + (long)row * 3;
            r[0] = p;
            r[1] = g0 + bit;
            r[2] = 0;
            ++row;
        }
    }
    for (long e = (long)total * 3 + tid; e < (long)N * 3; e += INST_THREADS) pairs[e] = 0;
    __syncthreads();

    // 3. the counts
    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const unsigned key = pair_key(pred, gt, base + lane, N, mp, mg);
        const unsigned prev = (unsigned)__shfl_up((int)key, 1);
        const bool edge = lane == 0 || key != prev;
        const unsigned long long edges = __ballot(edge);
        if (edge && (key >> 13) != 0u) {
            const unsigned long long higher = lane == 63 ? 0ull : (edges >> (lane + 1));
            const int len = higher ? __ffsll((long long)higher) : 64 - lane;
            const unsigned g = key & 0x1fffu;
            const unsigned w = ((key >> 13) - 1u) * GW + (g >> 5);
            const unsigned row = mu_ld_agent(pre + w) + __popc(mu_ld_agent(bits + w) & ((1u << (g & 31u)) - 1u));
            atomicAdd(&pairs[(long)row * 3 + 2], len);
        }
    }
}

static constexpr int pair_row_words(int max_inst_gt) { return (max_inst_gt + 1 + 31) >> 5; }      // bits 0..max_inst_gt

extern "C" int mu_instance_pairs_supported(int H, int W, int max_inst_pred, int max_inst_gt) {
    if (H <= 0 || W <= 0 || (long)H * W > INST_MAX_PIXELS) return MU_ERR_SHAPE;
    if (max_inst_pred < 1 || max_inst_pred > INST_MAX_INSTANCES || max_inst_gt < 1 || max_inst_gt > INST_MAX_INSTANCES) return MU_ERR_SHAPE;
    return MU_OK;
}

struct PairsWs {
    MuCarve c;
    unsigned* bits;     // [B][max_inst_pred][words] bit g of row p - 1: the pair (p, g) occurs
    unsigned* pre;      // [B][max_inst_pred][words] set bits before each word: the pair's row
    constexpr PairsWs(void* ws, int B, int max_inst_pred, int max_inst_gt)
        : c(ws), bits(c.take<unsigned>((long)B * max_inst_pred * pair_row_words(max_inst_gt))),
          pre(c.take<unsigned>((long)B * max_inst_pred * pair_row_words(max_inst_gt))) {}
};
static_assert(PairsWs(nullptr, 2, 5, 8).c.bytes == 2L * 5 * 1 * 2 * 4 && PairsWs(nullptr, 3, 4096, 4096).c.bytes == 3L * 4096 * 129 * 2 * 4,
              "mu_instance_pairs workspace");

extern "C" long mu_instance_pairs_workspace_bytes(int B, int H, int W, int max_inst_pred, int max_inst_gt) {
    if (B <= 0 || mu_instance_pairs_supported(H, W, max_inst_pred, max_inst_gt) != MU_OK) return 0;
    return PairsWs(nullptr, B, max_inst_pred, max_inst_gt).c.bytes;
}

extern "C" int mu_instance_pairs(const int* pred_ids, const int* gt_ids, int B, int H, int W, int max_inst_pred, int max_inst_gt,
                                 int* pairs, int* n_pairs, void* workspace, long ws_bytes, void* stream) {
    if (!pred_ids || !gt_ids || !pairs || !n_pairs || !workspace || B <= 0 || H <= 0 || W <= 0) return MU_ERR_ARG;
    if (mu_instance_pairs_supported(H, W, max_inst_pred, max_inst_gt) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_instance_pairs_workspace_bytes(B, H, W, max_inst_pred, max_inst_gt)) return MU_ERR_WORKSPACE;
    const PairsWs ws(workspace, B, max_inst_pred, max_inst_gt);
    inst_pairs_kernel<<<B, INST_THREADS, 0, (hipStream_t)stream>>>(pred_ids, gt_ids, H * W, max_inst_pred, max_inst_gt,
                                                                    pair_row_words(max_inst_gt), ws.bits, ws.pre, pairs, n_pairs);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// Matching: one workgroup per image.  Row k of every [B,K] output is the detection order[b][k]; it is evaluated (det_valid) iff its id
// is one of 1..min(count, max_inst_pred), its class one of 1..num_classes-1 and fewer than max_dets rows before it have that class.
// A ground truth takes part iff its id is one of 1..min(count, max_inst_gt) and its class one of 1..num_classes-1; the pixels of every
// other ground-truth id are void.
//   COCO      one thread per (class, threshold) walks the class's detections in order -- the greedy chain is sequential -- and for each
//             the detection's rows of the pair table (ascending gt id): iou = double(i) / double(a_p + a_g - i), one correctly rounded
//             division; a row is skipped if matched at this threshold or iou < best so far (which starts at min(t, 1 - 1e-10)), so of
//             equal IoUs the later gt wins.  matched[g] holds one bit per threshold: chains of one class share the words, not the bits.
//   panoptic  one thread per detection: v = its overlap with void, match iff double(i) / double(a_p + a_g - i - v) > 0.5 (at most one),
//             else a false positive unless double(v) / double(a_p) > 0.5.
// Dynamic LDS (ints): info[K] (class | rank << 16), list[K] (rows by class, in order), matched[max_inst_gt], ccnt[nc], cstart[nc + 1]:
// 56 KiB at the limits.
// ------------------------------------------------------------------------------------------
struct MatchParams {
    const int *pairs, *n_pairs, *ptable, *porder, *pcount, *gtable, *gcount;
    const float* pscore;
    int N, mp, mg, nc, K, max_dets, T;
    int *det_valid, *det_class, *det_gt, *gt_per_class, *pq_gt, *pq_fp, *overflow, *dstart;
    float* det_score;
    double *det_iou, *pq_iou;
    double thr[MATCH_MAX_T];                           // by value: nothing to upload, nothing that outlives the call
};

__global__ __launch_bounds__(INST_THREADS) void inst_match_kernel(const MatchParams P) {
    extern __shared__ unsigned inst_lds[];
    const int K = P.K, nc = P.nc, T = P.T;
    unsigned* info = inst_lds;
    int* list = (int*)(info + K);
    unsigned* matched = (unsigned*)(list + K);
    int* ccnt = (int*)(matched + P.mg);
    int* cstart = ccnt + nc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* pairs = P.pairs + (long)b * P.N * 3;
    const int n = min(max(P.n_pairs[b], 0), P.N);
    const int* ptable = P.ptable + (long)b * P.mp * 8;
    const int* gtable = P.gtable + (long)b * P.mg * 8;
    const int* porder = P.porder + (long)b * P.mp;
    const int Kp = min(max(P.pcount[b], 0), P.mp), Kg = min(max(P.gcount[b], 0), P.mg);
    int* dstart = P.dstart + (long)b * K;

    if (tid == 0) P.overflow[b] = (P.pcount[b] > P.mp || P.gcount[b] > P.mg) ? 1 : 0;
    for (int c = tid; c < nc; c += INST_THREADS) ccnt[c] = 0;
    for (int g = tid; g < P.mg; g += INST_THREADS) matched[g] = 0u;
    __syncthreads();
    for (int g = tid; g < Kg; g += INST_THREADS) {
        const int c = gtable[(long)g * 8];
        if (c >= 1 && c < nc) atomicAdd(&ccnt[c], 1);
    }
    for (int k = tid; k < K; k += INST_THREADS) {
        const int p = porder[k];
        int c = (p >= 1 && p <= Kp) ? ptable[(long)(p - 1) * 8] : 0;
        if (c < 1 || c >= nc) c = 0;
        info[k] = (unsigned)c;
    }
    __syncthreads();
    for (int c = tid; c < nc; c += INST_THREADS) {
        P.gt_per_class[(long)b * nc + c] = ccnt[c];
        ccnt[c] = 0;
    }
    __syncthreads();

    // rank of every row among the rows of its class (the low half of info[] does not change)
    for (int k = tid; k < K; k += INST_THREADS) {
        const unsigned c = info[k] & 0xffffu;
        unsigned rank = 0xffffu;
        if (c) {
            rank = 0;
            for (int j = 0; j < k; ++j) rank += ((info[j] & 0xffffu) == c);
            if (rank < (unsigned)P.max_dets) atomicAdd(&ccnt[c], 1);
            else rank = 0xffffu;
        }
        info[k] = c | (rank << 16);
    }
    __syncthreads();
    if (wave == 0) {                                   // cstart = exclusive scan of the evaluated rows per class
        const int evaluated = wave_scan_excl_array(ccnt, cstart, nc, lane);
        if (lane == 0) cstart[nc] = evaluated;
    }
    __syncthreads();

    // per row: the [B,K] outputs, the row's place in its class's list, its first row in the pair table, the panoptic match
    for (int k = tid; k < K; k += INST_THREADS) {
        const unsigned c = info[k] & 0xffffu, rank = info[k] >> 16;
        const bool valid = c != 0u && rank != 0xffffu;
        const long o = (long)b * K + k;
        int m_gt = 0, m_fp = 0;
        double m_iou = 0.0;
        if (valid) {
            const int p = porder[k];
            list[cstart[c] + (int)rank] = k;
            int lo = 0, hi = n;                        // lower bound of p in the pair table
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pairs[(long)mid * 3] < p) lo = mid + 1;
                else hi = mid;
            }
            dstart[k] = lo;
            const int a_p = ptable[(long)(p - 1) * 8 + 1];
            int v = 0;
            for (int r = lo; r < n && pairs[(long)r * 3] == p; ++r) {
                const int g = pairs[(long)r * 3 + 1];
                const int gc = (g >= 1 && g <= Kg) ? gtable[(long)(g - 1) * 8] : 0;
                if (gc < 1 || gc >= nc) v += pairs[(long)r * 3 + 2];
            }
            for (int r = lo; r < n && pairs[(long)r * 3] == p; ++r) {
                const int g = pairs[(long)r * 3 + 1];
                if (g < 1 || g > Kg || gtable[(long)(g - 1) * 8] != (int)c) continue;
                const int i = pairs[(long)r * 3 + 2];
                const int u = a_p + gtable[(long)(g - 1) * 8 + 1] - i - v;
                if (u <= 0) continue;
                const double iou = (double)i / (double)u;
                if (iou > 0.5) {
                    m_gt = g;
                    m_iou = iou;
                }
            }
            if (!m_gt) m_fp = (a_p > 0 && (double)v / (double)a_p > 0.5) ? 0 : 1;
            P.det_score[o] = P.pscore[(long)b * P.mp + p - 1];
        } else {
            dstart[k] = 0;
            P.det_score[o] = 0.f;
            for (int t = 0; t < T; ++t) {
                P.det_gt[((long)b * T + t) * K + k] = 0;
                P.det_iou[((long)b * T + t) * K + k] = 0.0;
            }
        }
        P.det_valid[o] = valid ? 1 : 0;
        P.det_class[o] = valid ? (int)c : 0;
        P.pq_gt[o] = m_gt;
        P.pq_iou[o] = m_iou;
        P.pq_fp[o] = m_fp;
    }
    __syncthreads();

    // COCO: chain q = (class, threshold); the T chains of a class sit in neighbouring lanes and read the same rows
    for (int q = tid; q < (nc - 1) * T; q += INST_THREADS) {
        const int c = 1 + q / T, t = q % T;
        const double floor_iou = fmin(P.thr[t], 1.0 - 1e-10);
        for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
            const int k = list[s];
            const int p = porder[k];
            const int a_p = ptable[(long)(p - 1) * 8 + 1];
            double best = floor_iou;
            int best_g = 0;
            for (int r = dstart[k]; r < n && pairs[(long)r * 3] == p; ++r) {
                const int g = pairs[(long)r * 3 + 1];
                if (g < 1 || g > Kg || gtable[(long)(g - 1) * 8] != c) continue;
                if ((*(volatile unsigned*)&matched[g - 1] >> t) & 1u) continue;
                const int i = pairs[(long)r * 3 + 2];
                const int u = a_p + gtable[(long)(g - 1) * 8 + 1] - i;
                if (u <= 0) continue;
                const double iou = (double)i / (double)u;
                if (iou < best) continue;
                best = iou;
                best_g = g;
            }
            if (best_g) atomicOr(&matched[best_g - 1], 1u << t);
            P.det_gt[((long)b * T + t) * K + k] = best_g;
            P.det_iou[((long)b * T + t) * K + k] = best_g ? best : 0.0;
        }
    }
}

extern "C" int mu_instance_match_supported(int H, int W, int max_inst_pred, int max_inst_gt, int num_classes, int K, int max_dets, int T) {
    if (mu_instance_pairs_supported(H, W, max_inst_pred, max_inst_gt) != MU_OK) return MU_ERR_SHAPE;
    if (num_classes < 1 || num_classes > MATCH_MAX_CLASSES || T < 1 || T > MATCH_MAX_T) return MU_ERR_SHAPE;
    if (K < 1 || K > max_inst_pred || max_dets < 1) return MU_ERR_SHAPE;
    return MU_OK;
}

struct MatchWs {
    MuCarve c;
    int* dstart;    // [B][K] where each detection's rows start in the pair table
    constexpr MatchWs(void* ws, int B, int K) : c(ws), dstart(c.take<int>((long)B * K)) {}
};
static_assert(MatchWs(nullptr, 2, 5).c.bytes == 2 * 5 * 4 && MatchWs(nullptr, 3, 4096).c.bytes == 3 * 4096 * 4, "mu_instance_match workspace");

extern "C" long mu_instance_match_workspace_bytes(int B, int K) {
    if (B <= 0 || K < 1 || K > INST_MAX_INSTANCES) return 0;
    return MatchWs(nullptr, B, K).c.bytes;
}

// dynamic LDS of the two match kernels: 57348 and 58372 bytes at the limits, no grant needed
static size_t inst_match_lds(int K, int max_inst_gt, int num_classes) { return (size_t)(2 * K + max_inst_gt + 2 * num_classes + 1) * sizeof(int); }

extern "C" int mu_instance_match(const int* pairs, const int* n_pairs, const int* pred_table, const float* pred_score,
                                 const int* pred_order, const int* pred_count, const int* gt_table, const int* gt_count, int B, int H,
                                 int W, int max_inst_pred, int max_inst_gt, int num_classes, int K, int max_dets, const double* thr,
                                 int T, int* det_valid, int* det_class, float* det_score, int* det_gt, double* det_iou,
                                 int* gt_per_class, int* pq_gt, double* pq_iou, int* pq_fp, int* overflow, void* workspace,
                                 long ws_bytes, void* stream) {
    if (!pairs || !n_pairs || !pred_table || !pred_score || !pred_order || !pred_count || !gt_table || !gt_count || !thr || !det_valid ||
        !det_class || !det_score || !det_gt || !det_iou || !gt_per_class || !pq_gt || !pq_iou || !pq_fp || !overflow || !workspace ||
        B <= 0 || H <= 0 || W <= 0)
        return MU_ERR_ARG;
    if (mu_instance_match_supported(H, W, max_inst_pred, max_inst_gt, num_classes, K, max_dets, T) != MU_OK) return MU_ERR_SHAPE;
    for (int t = 0; t < T; ++t)
        if (!(thr[t] > 0.0 && thr[t] <= 1.0)) return MU_ERR_ARG;      // a threshold of 0 would match pairs that do not overlap
    if (ws_bytes < mu_instance_match_workspace_bytes(B, K)) return MU_ERR_WORKSPACE;
    MatchParams P;
    P.pairs = pairs;
    P.n_pairs = n_pairs;
    P.ptable = pred_table;
    P.pscore = pred_score;
    P.porder = pred_order;
    P.pcount = pred_count;
    P.gtable = gt_table;
    P.gcount = gt_count;
    P.N = H * W;
    P.mp = max_inst_pred;
    P.mg = max_inst_gt;
    P.nc = num_classes;
    P.K = K;
    P.max_dets = max_dets;
    P.T = T;
    P.det_valid = det_valid;
    P.det_class = det_class;
    P.det_score = det_score;
    P.det_gt = det_gt;
    P.det_iou = det_iou;
    P.gt_per_class = gt_per_class;
    P.pq_gt = pq_gt;
    P.pq_iou = pq_iou;
    P.pq_fp = pq_fp;
    P.overflow = overflow;
    P.dstart = MatchWs(workspace, B, K).dstart;
    for (int t = 0; t < MATCH_MAX_T; ++t) P.thr[t] = t < T ? thr[t] : 1.0;
    inst_match_kernel<<<B, INST_THREADS, inst_match_lds(K, max_inst_gt, num_classes), (hipStream_t)stream>>>(P);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// mu_coco_match: COCOeval.evaluateImg in full (iscrowd, area ranges, the ignore flags) and panopticapi's crowd rules over the same pair
// table; inst_match_kernel above is untouched.  The same shape: one workgroup per image, rows, ranks and lists as there, then the A
// area ranges one after the other -- matched[] and the per-class counters are reused, only two bitmaps over the ground truths are new:
//   crowd[]  bit g - 1: ground truth g takes part and is iscrowd (built once);
//   ig[]     bit g - 1: gtIg of the current range = crowd || area < lo || area > hi (area: gt_area if given, else the pixel area).
// COCO's visiting order (the stable argsort of gtIg: non-ignored first, ascending id inside each group) is two walks over the
// detection's rows of the pair table, which are in ascending gt id: first the non-ignored ground truths, then -- only if nothing
// matched, that is evaluateImg's break -- the ignored ones.  Against a crowd ground truth iou = double(i) / double(a_p), and its
// matched bit never excludes it.
// Panoptic: a crowd ground truth is no candidate and is not counted; an unmatched detection is no false positive if
// double(v + i_crowd) / double(a_p) > 0.5 with i_crowd its overlap with the highest crowd id of its class (ccnt[] holds that id
// between the scan and the first range).
// Dynamic LDS: the layout above plus 2 * 2 * ceil(max_inst_gt / 64) words: 58 372 bytes at the limits.
// ------------------------------------------------------------------------------------------
#define COCO_MAX_A 4

struct CocoParams {
    const int *pairs, *n_pairs, *ptable, *porder, *pcount, *gtable, *gcount, *gcrowd;
    const float* pscore;
    const double* garea;
    int N, mp, mg, nc, K, max_dets, T, A;
    int *det_valid, *det_class, *det_rank, *det_gt, *gt_counted, *pq_gt_per_class, *pq_gt, *pq_fp, *overflow, *dstart;
    float* det_score;
    double *det_iou, *pq_iou;
    unsigned char* det_ignore;
    double thr[MATCH_MAX_T];
    double rng[COCO_MAX_A][2];
};

static int coco_bit_words(int max_inst_gt) { return ((max_inst_gt + 63) >> 6) << 1; }      // whole 64-lane ballots
static size_t coco_match_lds(int K, int max_inst_gt, int num_classes) {
    return inst_match_lds(K, max_inst_gt, num_classes) + (size_t)2 * coco_bit_words(max_inst_gt) * sizeof(int);
}

__device__ __forceinline__ bool coco_bit(const unsigned* bits, int g) { return (bits[(g - 1) >> 5] >> ((g - 1) & 31)) & 1u; }

__global__ __launch_bounds__(INST_THREADS) void coco_match_kernel(const CocoParams P) {
    extern __shared__ unsigned inst_lds[];
    const int K = P.K, nc = P.nc, T = P.T, A = P.A;
    const int GB = ((P.mg + 63) >> 6) << 1;
    unsigned* info = inst_lds;
    int* list = (int*)(info + K);
    unsigned* matched = (unsigned*)(list + K);
    int* ccnt = (int*)(matched + P.mg);
    int* cstart = ccnt + nc;
    unsigned* crowd = (unsigned*)(cstart + nc + 1);
    unsigned* ig = crowd + GB;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* pairs = P.pairs + (long)b * P.N * 3;
    const int n = min(max(P.n_pairs[b], 0), P.N);
    const int* ptable = P.ptable + (long)b * P.mp * 8;
    const int* gtable = P.gtable + (long)b * P.mg * 8;
    const int* porder = P.porder + (long)b * P.mp;
    const int* gcrowd = P.gcrowd ? P.gcrowd + (long)b * P.mg : nullptr;
    const double* garea = P.garea ? P.garea + (long)b * P.mg : nullptr;
    const int Kp = min(max(P.pcount[b], 0), P.mp), Kg = min(max(P.gcount[b], 0), P.mg);
    int* dstart = P.dstart + (long)b * K;

    if (tid == 0) P.overflow[b] = (P.pcount[b] > P.mp || P.gcount[b] > P.mg) ? 1 : 0;
    for (int c = tid; c < nc; c += INST_THREADS) ccnt[c] = 0;
    __syncthreads();
    // the ground truths that take part: crowd bits, and the non-crowd ones per class (what panoptic counts)
    for (int g0 = wave * 64; g0 < GB * 32; g0 += INST_THREADS) {
        const int g = g0 + lane;                       // id g + 1
        const int c = g < Kg ? gtable[(long)g * 8] : 0;
        const bool part = c >= 1 && c < nc;
        const bool cr = part && gcrowd && gcrowd[g] != 0;
        if (part && !cr) atomicAdd(&ccnt[c], 1);
        const unsigned long long m = __ballot(cr);
        if (lane == 0) {
            crowd[g0 >> 5] = (unsigned)m;
            crowd[(g0 >> 5) + 1] = (unsigned)(m >> 32);
        }
    }
    for (int k = tid; k < K; k += INST_THREADS) {
        const int p = porder[k];
        int c = (p >= 1 && p <= Kp) ? ptable[(long)(p - 1) * 8] : 0;
        if (c < 1 || c >= nc) c = 0;
        info[k] = (unsigned)c;
    }
    __syncthreads();
    for (int c = tid; c < nc; c += INST_THREADS) {
        P.pq_gt_per_class[(long)b * nc + c] = ccnt[c];
        ccnt[c] = 0;
    }
    __syncthreads();

    // rank of every row among the rows of its class, as in inst_match_kernel
    for (int k = tid; k < K; k += INST_THREADS) {
        const unsigned c = info[k] & 0xffffu;
        unsigned rank = 0xffffu;
        if (c) {
            rank = 0;
            for (int j = 0; j < k; ++j) rank += ((info[j] & 0xffffu) == c);
            if (rank < (unsigned)P.max_dets) atomicAdd(&ccnt[c], 1);
            else rank = 0xffffu;
        }
        info[k] = c | (rank << 16);
    }
    __syncthreads();
    if (wave == 0) {
        const int evaluated = wave_scan_excl_array(ccnt, cstart, nc, lane);
        if (lane == 0) cstart[nc] = evaluated;
    }
    __syncthreads();

    // ccnt[c] = the highest crowd id of class c, 0 = none
    for (int c = tid; c < nc; c += INST_THREADS) ccnt[c] = 0;
    __syncthreads();
    for (int g = 1 + tid; g <= Kg; g += INST_THREADS)
        if (coco_bit(crowd, g)) atomicMax(&ccnt[gtable[(long)(g - 1) * 8]], g);
    __syncthreads();

    // per row: the [B,K] outputs, the row's place in its class's list, its first row in the pair table, the panoptic match
    for (int k = tid; k < K; k += INST_THREADS) {
        const unsigned c = info[k] & 0xffffu, rank = info[k] >> 16;
        const bool valid = c != 0u && rank != 0xffffu;
        const long o = (long)b * K + k;
        int m_gt = 0, m_fp = 0;
        double m_iou = 0.0;
        if (valid) {
            const int p = porder[k];
            list[cstart[c] + (int)rank] = k;
            int lo = 0, hi = n;                        // lower bound of p in the pair table
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pairs[(long)mid * 3] < p) lo = mid + 1;
                else hi = mid;
            }
            dstart[k] = lo;
            const int a_p = ptable[(long)(p - 1) * 8 + 1];
            const int last_crowd = ccnt[c];
            int v = 0, i_crowd = 0;
            for (int r = lo; r < n && pairs[(long)r * 3] == p; ++r) {
                const int g = pairs[(long)r * 3 + 1];
                const int gc = (g >= 1 && g <= Kg) ? gtable[(long)(g - 1) * 8] : 0;
                if (gc < 1 || gc >= nc) v += pairs[(long)r * 3 + 2];
                else if (g == last_crowd) i_crowd = pairs[(long)r * 3 + 2];
            }
            for (int r = lo; r < n && pairs[(long)r * 3] == p; ++r) {
                const int g = pairs[(long)r * 3 + 1];
                if (g < 1 || g > Kg || gtable[(long)(g - 1) * 8] != (int)c || coco_bit(crowd, g)) continue;
                const int i = pairs[(long)r * 3 + 2];
                const int u = a_p + gtable[(long)(g - 1) * 8 + 1] - i - v;
                if (u <= 0) continue;
                const double iou = (double)i / (double)u;
                if (iou > 0.5) {
                    m_gt = g;
                    m_iou = iou;
                }
            }
            if (!m_gt) m_fp = (a_p > 0 && (double)(v + i_crowd) / (double)a_p > 0.5) ? 0 : 1;
            P.det_score[o] = P.pscore[(long)b * P.mp + p - 1];
        } else {
            dstart[k] = 0;
            P.det_score[o] = 0.f;
            for (int at = 0; at < A * T; ++at) {
                P.det_gt[((long)b * A * T + at) * K + k] = 0;
                P.det_iou[((long)b * A * T + at) * K + k] = 0.0;
                P.det_ignore[((long)b * A * T + at) * K + k] = 0;
            }
        }
        P.det_valid[o] = valid ? 1 : 0;
        P.det_class[o] = valid ? (int)c : 0;
        P.det_rank[o] = valid ? (int)rank : 0;
        P.pq_gt[o] = m_gt;
        P.pq_iou[o] = m_iou;
        P.pq_fp[o] = m_fp;
    }

    for (int a = 0; a < A; ++a) {
        const double lo_a = P.rng[a][0], hi_a = P.rng[a][1];
        __syncthreads();                               // the rows above / the chains of the range before are done with ccnt, matched, ig
        for (int c = tid; c < nc; c += INST_THREADS) ccnt[c] = 0;
        for (int g = tid; g < P.mg; g += INST_THREADS) matched[g] = 0u;
        __syncthreads();
        for (int g0 = wave * 64; g0 < GB * 32; g0 += INST_THREADS) {
            const int g = g0 + lane;
            const int c = g < Kg ? gtable[(long)g * 8] : 0;
            const bool part = c >= 1 && c < nc;
            bool ignored = false;
            if (part) {
                const double area = garea ? garea[g] : (double)gtable[(long)g * 8 + 1];
                ignored = ((crowd[g >> 5] >> (g & 31)) & 1u) || area < lo_a || area > hi_a;
                if (!ignored) atomicAdd(&ccnt[c], 1);
            }
            const unsigned long long m = __ballot(ignored);
            if (lane == 0) {
                ig[g0 >> 5] = (unsigned)m;
                ig[(g0 >> 5) + 1] = (unsigned)(m >> 32);
            }
        }
        __syncthreads();
        for (int c = tid; c < nc; c += INST_THREADS) P.gt_counted[((long)b * A + a) * nc + c] = ccnt[c];

        // chain q = (class, threshold), as in inst_match_kernel
        for (int q = tid; q < (nc - 1) * T; q += INST_THREADS) {
            const int c = 1 + q / T, t = q % T;
            const double floor_iou = fmin(P.thr[t], 1.0 - 1e-10);
            const long at = ((long)b * A + a) * T + t;
            for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
                const int k = list[s];
                const int p = porder[k];
                const int a_p = ptable[(long)(p - 1) * 8 + 1];
                double best = floor_iou;
                int best_g = 0;
                for (int pass = 0; pass < 2 && !best_g; ++pass) {      // the non-ignored ground truths, then the ignored ones
                    for (int r = dstart[k]; r < n && pairs[(long)r * 3] == p; ++r) {
                        const int g = pairs[(long)r * 3 + 1];
                        if (g < 1 || g > Kg || gtable[(long)(g - 1) * 8] != c) continue;
                        if ((int)coco_bit(ig, g) != pass) continue;
                        const bool cr = coco_bit(crowd, g);
                        if (!cr && ((*(volatile unsigned*)&matched[g - 1] >> t) & 1u)) continue;
                        const int i = pairs[(long)r * 3 + 2];
                        const int u = cr ? a_p : a_p + gtable[(long)(g - 1) * 8 + 1] - i;
                        if (u <= 0) continue;
                        const double iou = (double)i / (double)u;
                        if (iou < best) continue;
                        best = iou;
                        best_g = g;
                    }
                }
                if (best_g) atomicOr(&matched[best_g - 1], 1u << t);
                P.det_gt[at * K + k] = best_g;
                P.det_iou[at * K + k] = best_g ? best : 0.0;
                P.det_ignore[at * K + k] = best_g ? (unsigned char)coco_bit(ig, best_g)
                                                  : (unsigned char)((double)a_p < lo_a || (double)a_p > hi_a);
            }
        }
    }
}

extern "C" int mu_coco_match_supported(int H, int W, int max_inst_pred, int max_inst_gt, int num_classes, int K, int max_dets, int T,
                                       int A) {
    if (mu_instance_match_supported(H, W, max_inst_pred, max_inst_gt, num_classes, K, max_dets, T) != MU_OK) return MU_ERR_SHAPE;
    if (A < 1 || A > COCO_MAX_A) return MU_ERR_SHAPE;
    return MU_OK;
}

// MatchWs, as mu_instance_match
extern "C" long mu_coco_match_workspace_bytes(int B, int K) { return mu_instance_match_workspace_bytes(B, K); }

extern "C" int mu_coco_match(const int* pairs, const int* n_pairs, const int* pred_table, const float* pred_score, const int* pred_order,
                             const int* pred_count, const int* gt_table, const int* gt_count, const int* gt_crowd_or_null,
                             const double* gt_area_or_null, int B, int H, int W, int max_inst_pred, int max_inst_gt, int num_classes,
                             int K, int max_dets, const double* thr, int T, const double* area_rng, int A, int* det_valid,
                             int* det_class, int* det_rank, float* det_score, int* det_gt, double* det_iou, unsigned char* det_ignore,
                             int* gt_counted, int* pq_gt_per_class, int* pq_gt, double* pq_iou, int* pq_fp, int* overflow,
                             void* workspace, long ws_bytes, void* stream) {
    if (!pairs || !n_pairs || !pred_table || !pred_score || !pred_order || !pred_count || !gt_table || !gt_count || !thr || !area_rng ||
        !det_valid || !det_class || !det_rank || !det_score || !det_gt || !det_iou || !det_ignore || !gt_counted || !pq_gt_per_class ||
        !pq_gt || !pq_iou || !pq_fp || !overflow || !workspace || B <= 0 || H <= 0 || W <= 0)
        return MU_ERR_ARG;
    if (mu_coco_match_supported(H, W, max_inst_pred, max_inst_gt, num_classes, K, max_dets, T, A) != MU_OK) return MU_ERR_SHAPE;
    for (int t = 0; t < T; ++t)
        if (!(thr[t] > 0.0 && thr[t] <= 1.0)) return MU_ERR_ARG;      // NaN included
    for (int a = 0; a < A; ++a)
        if (!(area_rng[2 * a] <= area_rng[2 * a + 1])) return MU_ERR_ARG;
    if (ws_bytes < mu_coco_match_workspace_bytes(B, K)) return MU_ERR_WORKSPACE;
    CocoParams P;
    P.pairs = pairs;
    P.n_pairs = n_pairs;
    P.ptable = pred_table;
    P.pscore = pred_score;
    P.porder = pred_order;
    P.pcount = pred_count;
    P.gtable = gt_table;
    P.gcount = gt_count;
    P.gcrowd = gt_crowd_or_null;
    P.garea = gt_area_or_null;
    P.N = H * W;
    P.mp = max_inst_pred;
    P.mg = max_inst_gt;
    P.nc = num_classes;
    P.K = K;
    P.max_dets = max_dets;
    P.T = T;
    P.A = A;
    P.det_valid = det_valid;
    P.det_class = det_class;
    P.det_rank = det_rank;
    P.det_score = det_score;
    P.det_gt = det_gt;
    P.det_iou = det_iou;
    P.det_ignore = det_ignore;
    P.gt_counted = gt_counted;
    P.pq_gt_per_class = pq_gt_per_class;
    P.pq_gt = pq_gt;
    P.pq_iou = pq_iou;
    P.pq_fp = pq_fp;
    P.overflow = overflow;
    P.dstart = MatchWs(workspace, B, K).dstart;
    for (int t = 0; t < MATCH_MAX_T; ++t) P.thr[t] = t < T ? thr[t] : 1.0;
    for (int a = 0; a < COCO_MAX_A; ++a) {
        P.rng[a][0] = a < A ? area_rng[2 * a] : 0.0;
        P.rng[a][1] = a < A ? area_rng[2 * a + 1] : 0.0;
    }
    coco_match_kernel<<<B, INST_THREADS, coco_match_lds(K, max_inst_gt, num_classes), (hipStream_t)stream>>>(P);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// mu_id_instances: ground-truth instances from an id map the dataset supplies -- get_instance_annotations
// (city_instance.py:431-449) on Cityscapes instanceIds, panopticapi's rgb2id of a COCO panoptic PNG, or coco_masks(...).ids.  Instance
// k is the set of pixels that hold the k-th distinct non-zero value in ascending signed order (np.unique); its class is the median of
// the semantic map over its pixels.  Four launches, one workgroup per image, stream-ordered, integer atomics only:
//   rank    effective values (dropped pixels count as 0) -> run heads in raster order, compacted -> LSD radix sort, 8 bits per pass,
//           passes whose digit is the same in every key skipped -> distinct list (count, values) -> every pixel finds its rank by
//           bisection (once per run of a 64-pixel chunk); first pixel by atomicMin in LDS;
//   pairs   inst_pairs_kernel on (ids, semantic map): the (id, class, pixels) rows sorted by (id, class);
//   median  one thread per instance walks its rows to the cumulative positions (n - 1) / 2 and n / 2;
//   stats   inst_stats_kernel with the per-id class array.
// ------------------------------------------------------------------------------------------
#define IDMAP_MAX_CLASSES 1024
#define IDMAP_DIGITS 256

template <int KIND>
__device__ __forceinline__ const void* idmap_image(const void* map, int b, int N) {
    if (KIND == MU_IDMAP_I32) return (const int*)map + (long)b * N;
    if (KIND == MU_IDMAP_I64) return (const long long*)map + (long)b * N;
    return (const unsigned char*)map + (long)b * N * 3;
}

// effective value of pixel i; inv collects why pixels were dropped (bit 0: class outside [0, class_cap), bit 1: an int64 id outside int32)
template <int KIND>
__device__ __forceinline__ int idmap_value(const void* __restrict__ map, const int* __restrict__ sem, int i, int class_cap, unsigned& inv) {
    int v;
    bool fits = true;
    if (KIND == MU_IDMAP_I32) {
        v = ((const int*)map)[i];
    } else if (KIND == MU_IDMAP_I64) {
        const long long w = ((const long long*)map)[i];
        v = (int)w;
        fits = (long long)v == w;
        if (!fits) v = 1;                                      // non-zero whatever the low word holds
    } else {
        const unsigned char* p = (const unsigned char*)map + 3 * i;
        v = (int)p[0] | ((int)p[1] << 8) | ((int)p[2] << 16);  // panopticapi's rgb2id
    }
    if (v == 0) return 0;
    const unsigned bad = ((unsigned)sem[i] >= (unsigned)class_cap ? 1u : 0u) | (fits ? 0u : 2u);
    inv |= bad;
    return bad ? 0 : v;
}

// one 64-pixel chunk of the wave's segment [.., hi): v = the lane's effective value; true where a run of a non-zero value starts
template <int KIND>
__device__ __forceinline__ bool idmap_head(const void* __restrict__ map, const int* __restrict__ sem, int base, int lane, int hi,
                                           int class_cap, int& v, unsigned& inv) {
    const int i = base + lane;
    v = i < hi ? idmap_value<KIND>(map, sem, i, class_cap, inv) : 0;
    int pv = __shfl_up(v, 1);
    if (lane == 0) {
        unsigned other = 0;                                    // that pixel reports its own bits
        pv = base > 0 ? idmap_value<KIND>(map, sem, base - 1, class_cap, other) : 0;
    }
    return v != 0 && v != pv;
}

// keys_all: 2 * N words per image (the two sides of the sort).  Dynamic LDS (ints): cnt[INST_WAVES][256], tot[256], first[max_inst]:
// 33 KiB at the limits, no grant needed.
template <int KIND>
__global__ __launch_bounds__(INST_THREADS) void idmap_rank_kernel(const void* __restrict__ map_all, const int* __restrict__ sem_all, int N,
                                                                   int max_inst, int class_cap, unsigned* keys_all,
                                                                   int* __restrict__ ids_all, int* __restrict__ count,
                                                                   int* __restrict__ values_all, int* __restrict__ invalid,
                                                                   int* __restrict__ first_all) {
    extern __shared__ unsigned inst_lds[];
    __shared__ unsigned wave_total[INST_WAVES];
    __shared__ unsigned red[3];                                // dropped-pixel bits; OR and AND of the keys
    int* cnt = (int*)inst_lds;
    int* tot = cnt + INST_WAVES * IDMAP_DIGITS;
    int* first = tot + IDMAP_DIGITS;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const void* map = idmap_image<KIND>(map_all, b, N);
    const int* sem = sem_all + (long)b * N;
    unsigned* src = keys_all + (long)b * N * 2;
    unsigned* dst = src + N;
    int* ids = ids_all + (long)b * N;
    int* values = values_all + (long)b * max_inst;

    if (tid == 0) {
        red[0] = 0u;
        red[1] = 0u;
        red[2] = ~0u;
    }
    for (int k = tid; k < max_inst; k += INST_THREADS) first[k] = 0x7fffffff;

    // 1. run heads in raster order, compacted: keys = value with the sign bit flipped (unsigned order = signed order)
    int lo, hi, v;
    wave_segment(N, INST_WAVES, wave, lo, hi);
    unsigned mine = 0, total, inv = 0, kor = 0u, kand = ~0u;
    for (int base = lo; base < hi; base += 64) mine += __popcll(__ballot(idmap_head<KIND>(map, sem, base, lane, hi, class_cap, v, inv)));
    unsigned running = block_exclusive_base(mine, wave_total, lane, wave, INST_WAVES, total);
    const int nh = (int)total;
    for (int base = lo; base < hi; base += 64) {
        const bool head = idmap_head<KIND>(map, sem, base, lane, hi, class_cap, v, inv);
        const unsigned pos = wave_flag_rank(head, lane, running);
        if (head) {
            const unsigned key = (unsigned)v ^ 0x80000000u;
            src[pos] = key;
            kor |= key;
            kand &= key;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        inv |= (unsigned)__shfl_xor((int)inv, o);
        kor |= (unsigned)__shfl_xor((int)kor, o);
        kand &= (unsigned)__shfl_xor((int)kand, o);
    }
    if (lane == 0) {
        atomicOr(&red[0], inv);
        atomicOr(&red[1], kor);
        atomicAnd(&red[2], kand);
    }
    __syncthreads();                 // the keys (global memory, same workgroup) and red[] are visible past this barrier
    if (tid == 0) invalid[b] = (int)red[0];
    const unsigned live = nh ? red[1] ^ red[2] : 0u;          // the bits in which two keys differ

    // 2. stable LSD radix sort of the heads.  Every wave owns a segment of the keys and its own counters: no atomics, a fixed order.
    wave_segment(nh, INST_WAVES, wave, lo, hi);
    int* my_cnt = cnt + wave * IDMAP_DIGITS;
    for (int shift = 0; shift < 32; shift += 8) {
        if (((live >> shift) & 255u) == 0u) continue;          // the same digit in every key (uniform over the workgroup)
        for (int k = tid; k < INST_WAVES * IDMAP_DIGITS; k += INST_THREADS) cnt[k] = 0;
        __syncthreads();
        for (int base = lo; base < hi; base += 64) {
            const bool has = base + lane < hi;
            const unsigned key = has ? src[base + lane] : 0u;
            wave_sort_chunk<false>((int)((key >> shift) & 255u), has, lane, my_cnt);
        }
        __syncthreads();
        if (tid < IDMAP_DIGITS) {                              // per digit: exclusive prefix over the waves, total
            int run = 0;
            for (int w = 0; w < INST_WAVES; ++w) {
                const int t = cnt[w * IDMAP_DIGITS + tid];
                cnt[w * IDMAP_DIGITS + tid] = run;
                run += t;
            }
            tot[tid] = run;
        }
        __syncthreads();
        if (wave == 0) wave_scan_excl_array(tot, tot, IDMAP_DIGITS, lane);
        __syncthreads();
        for (int k = tid; k < INST_WAVES * IDMAP_DIGITS; k += INST_THREADS) cnt[k] += tot[k & (IDMAP_DIGITS - 1)];
        __syncthreads();
        for (int base = lo; base < hi; base += 64) {
            const bool has = base + lane < hi;
            const unsigned key = has ? src[base + lane] : 0u;
            const int pos = wave_sort_chunk<true>((int)((key >> shift) & 255u), has, lane, my_cnt);
            if (has) dst[pos] = key;
        }
        __syncthreads();
        unsigned* t = src;
        src = dst;
        dst = t;
    }

    // 3. the distinct keys, ascending: dst[0..n)
    mine = 0;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const unsigned key = j < hi ? src[j] : 0u;
        unsigned prev = (unsigned)__shfl_up((int)key, 1);
        if (lane == 0 && j > 0 && j < hi) prev = src[j - 1];
        mine += __popcll(__ballot(j < hi && (j == 0 || key != prev)));
    }
    running = block_exclusive_base(mine, wave_total, lane, wave, INST_WAVES, total);
    const int n = (int)total;
    if (tid == 0) count[b] = n;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const unsigned key = j < hi ? src[j] : 0u;
        unsigned prev = (unsigned)__shfl_up((int)key, 1);
        if (lane == 0 && j > 0 && j < hi) prev = src[j - 1];
        const bool fresh = j < hi && (j == 0 || key != prev);
        const unsigned r = wave_flag_rank(fresh, lane, running);
        if (fresh) {
            dst[r] = key;
            if (r < (unsigned)max_inst) values[r] = (int)(key ^ 0x80000000u);
        }
    }
    for (int k = n + tid; k < max_inst; k += INST_THREADS) values[k] = 0;
    __syncthreads();

    // 4. ids: one bisection per run of a 64-pixel chunk, the run's pixels take its result
    for (int base = wave * 64; base < N; base += INST_THREADS) {
        const int i = base + lane;
        unsigned other = 0;
        v = i < N ? idmap_value<KIND>(map, sem, i, class_cap, other) : 0;
        const int pv = __shfl_up(v, 1);
        const bool edge = lane == 0 || v != pv;
        int id = 0;
        if (edge && v != 0) {
            const unsigned key = (unsigned)v ^ 0x80000000u;
            int a = 0, z = n;                                  // the first position whose key is not below: the key is in the list
            while (a < z) {
                const int m = (a + z) >> 1;
                if (dst[m] < key) a = m + 1;
                else z = m;
            }
            id = a + 1;
            if (id <= max_inst) atomicMin(&first[id - 1], i);
        }
        const unsigned long long edges = __ballot(edge) & (lanes_below(lane) | (1ull << lane));      // lane 0 is always one
        id = __shfl(id, 63 - __builtin_clzll(edges));
        if (i < N) ids[i] = id;
    }
    __syncthreads();
    for (int k = tid; k < max_inst; k += INST_THREADS) first_all[(long)b * max_inst + k] = first[k];
}

// pairs: the rows of inst_pairs_kernel on (ids, semantic map), sorted by (id, class).  inst_cls[k] = (c_(n-1)/2 + c_n/2) / 2 over the
// sorted classes of id k + 1: int(np.median(..)); 0 past min(count, max_inst).
__global__ __launch_bounds__(INST_THREADS) void idmap_median_kernel(const int* __restrict__ pairs_all, const int* __restrict__ n_pairs,
                                                                     const int* __restrict__ count, int N, int max_inst,
                                                                     int* __restrict__ inst_cls_all) {
    const int b = blockIdx.x;
    const int* pairs = pairs_all + (long)b * N * 3;
    int* inst_cls = inst_cls_all + (long)b * max_inst;
    const int rows = n_pairs[b], K = min(count[b], max_inst);
    for (int k = threadIdx.x; k < max_inst; k += INST_THREADS) {
        int c = 0;
        if (k < K) {
            int a = 0, z = rows;                               // the first row of id k + 1
            while (a < z) {
                const int m = (a + z) >> 1;
                if (pairs[3 * m] < k + 1) a = m + 1;
                else z = m;
            }
            int n = 0;
            for (int r = a; r < rows && pairs[3 * r] == k + 1; ++r) n += pairs[3 * r + 2];
            const int t0 = (n - 1) >> 1, t1 = n >> 1;
            int cum = 0, c0 = -1, c1 = 0;
            for (int r = a; r < rows && pairs[3 * r] == k + 1; ++r) {
                cum += pairs[3 * r + 2];
                if (c0 < 0 && cum > t0) c0 = pairs[3 * r + 1];
                if (cum > t1) {
                    c1 = pairs[3 * r + 1];
                    break;
                }
            }
            c = (c0 + c1) / 2;
        }
        inst_cls[k] = c;
    }
}

extern "C" int mu_id_instances_supported(int H, int W, int max_inst, int class_cap) {
    if (mu_instances_supported(H, W, max_inst) != MU_OK) return MU_ERR_SHAPE;
    if (class_cap < 1 || class_cap > IDMAP_MAX_CLASSES) return MU_ERR_SHAPE;
    return MU_OK;
}

struct IdmapWs {
    MuCarve c;
    unsigned* keys;     // [B][2][N] the radix sort's two key buffers
    int* first;         // [B][max_inst] first pixel of every instance, for the statistics kernel
    int* inst_cls;      // [B][max_inst] the median class of every instance
    unsigned* bits;     // [B][max_inst][words] the pair bitmap of (id, class), as PairsWs
    unsigned* pre;      // [B][max_inst][words]
    int* pairs;         // [B][N][3] the pair table of (id, class)
    int* n_pairs;       // [B] its rows
    constexpr IdmapWs(void* ws, int B, int N, int max_inst, int class_cap)
        : c(ws), keys(c.take<unsigned>((long)B * N * 2)), first(c.take<int>((long)B * max_inst)), inst_cls(c.take<int>((long)B * max_inst)),
          bits(c.take<unsigned>((long)B * max_inst * pair_row_words(class_cap - 1))),
          pre(c.take<unsigned>((long)B * max_inst * pair_row_words(class_cap - 1))), pairs(c.take<int>((long)B * N * 3)),
          n_pairs(c.take<int>(B)) {}
};
static_assert(IdmapWs(nullptr, 2, 63, 5, 4).c.bytes == 2L * (5 * 63 + 2 * 5 * (1 + 1) + 1) * 4 &&
              IdmapWs(nullptr, 3, 65536, 4096, 1024).c.bytes == 3L * (5 * 65536 + 2L * 4096 * (1 + 32) + 1) * 4, "mu_id_instances workspace");

extern "C" long mu_id_instances_workspace_bytes(int B, int H, int W, int max_inst, int class_cap) {
    if (B <= 0 || mu_id_instances_supported(H, W, max_inst, class_cap) != MU_OK) return 0;
    return IdmapWs(nullptr, B, H * W, max_inst, class_cap).c.bytes;
}

// kind dispatch (host): f(integral_constant<int, KIND>) for the three id-map kinds; any other kind is MU_ERR_ARG
template <typename F>
static inline int with_idmap_kind(int id_kind, F&& f) {
    if (id_kind == MU_IDMAP_I32) return f(std::integral_constant<int, MU_IDMAP_I32>{});
    if (id_kind == MU_IDMAP_I64) return f(std::integral_constant<int, MU_IDMAP_I64>{});
    if (id_kind == MU_IDMAP_RGB8) return f(std::integral_constant<int, MU_IDMAP_RGB8>{});
    return MU_ERR_ARG;
}
static size_t idmap_rank_lds(int max_inst) { return (size_t)((INST_WAVES + 1) * IDMAP_DIGITS + max_inst) * sizeof(int); }      // 13 KiB + 16 KiB

extern "C" int mu_id_instances(const void* id_map, int id_kind, const int* sem, int B, int H, int W, int max_inst, int class_cap, int* ids,
                               int* table, float* score, int* count, int* order, int* values, int* invalid, void* workspace,
                               long ws_bytes, void* stream) {
    if (!id_map || !sem || !ids || !table || !score || !count || !order || !values || !invalid || !workspace || B <= 0 || H <= 0 || W <= 0)
        return MU_ERR_ARG;
    if (id_kind != MU_IDMAP_I32 && id_kind != MU_IDMAP_I64 && id_kind != MU_IDMAP_RGB8) return MU_ERR_ARG;
    if (mu_id_instances_supported(H, W, max_inst, class_cap) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_id_instances_workspace_bytes(B, H, W, max_inst, class_cap)) return MU_ERR_WORKSPACE;
    if (!inst_stats_granted()) return MU_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    const int N = H * W, P = mu_pow2(max_inst);
    const IdmapWs ws(workspace, B, N, max_inst, class_cap);
    const int rc = with_idmap_kind(id_kind, [&](auto kind) -> int {
        idmap_rank_kernel<decltype(kind)::value><<<B, INST_THREADS, idmap_rank_lds(max_inst), st>>>(id_map, sem, N, max_inst, class_cap, ws.keys, ids,
                                                                                                     count, values, invalid, ws.first);
        MU_CHECK_LAUNCH();
        return MU_OK;
    });
    if (rc != MU_OK) return rc;
    inst_pairs_kernel<<<B, INST_THREADS, 0, st>>>(ids, sem, N, max_inst, class_cap - 1, pair_row_words(class_cap - 1), ws.bits, ws.pre, ws.pairs,
                                                   ws.n_pairs);
    MU_CHECK_LAUNCH();
    idmap_median_kernel<<<B, INST_THREADS, 0, st>>>(ws.pairs, ws.n_pairs, count, N, max_inst, ws.inst_cls);
    MU_CHECK_LAUNCH();
    inst_stats_kernel<<<B, INST_THREADS, inst_stats_lds(P), st>>>(sem, nullptr, ids, count, ws.first, ws.inst_cls, N, W, max_inst, P, table, score,
                                                                   order);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
