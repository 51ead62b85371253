// Semantic evaluation in ONE read of the logits (contract: include/maskunet_hip.h, mu_sem_eval): what a validation batch of the
// reference needs from its outputs -- criterion(outputs, labels) (ade_semantic.py:454; ignore_index 255: city_semantic.py:341),
// mean_iou (city_panoptic.py:225-236), compute_iou_for_image (city_panoptic.py:212-222) and softmax(outputs / 0.5) + argmax
// (ade_instance.py:408-411) -- plus the confusion matrix that the scripts' sklearn metrics are functions of.
// Scheme: a block works on the pixels of ONE image (grid = images x blocks-per-image), so the per-image class counts are a
// block-private LDS histogram and the loss partials are per image.  The (C+1) x C confusion counters are privatised in LDS up to
// MU_SEM_EVAL_LDS_MAX_C classes (90.6 KB at C = 150: one workgroup per CU, hence 1024 threads = 4 waves per SIMD) and flushed with
// 64-bit integer atomics; above that every pixel row issues one 64-bit integer atomic on the global matrix.  Only integer atomics, and
// the fp64 loss sums in a fixed order (per-block partials, then an ordered finalize): every output is bit-identical from run to run.
//   vector path   c_stride == 1 and 16-byte aligned rows (the NHWC module output): 16 lanes per pixel row, 16-byte loads, rows of up
//                 to 3 x 16 vectors held in registers as ce_rows_in_regs (loss.hip) with several rows per lane group in flight; max,
//                 first arg-max, both exponential sums and the target fetch from that one read.  Wider rows: two passes (L2).
//   strided path  anything else (NCHW): one thread per pixel, lanes along the pixels, online maximum; same outputs.
#include "common.h"

#define SE_THREADS 1024                 // vector path: 64 pixel rows per pass
#define SE_WAVES (SE_THREADS / 64)
#define SE_STRIDED_THREADS 256
#define SE_ROWS_PER_BLOCK 512           // a block is given at least this many pixels (it zeroes and flushes its LDS counters once)
#define SE_TARGET_BLOCKS 512
#define SE_LOG2E 1.4426950408889634f

struct SemParams {
    const void* logits;
    const long* labels;
    long HW, M;
    int C, bpi;                         // bpi = blocks per image
    long inner, outer, cs, ps;
    long ignore;
    float k2;                           // log2(e) / temperature
    int* img_counts;
    unsigned long long* confusion;
    int* cls;
    float* prob;
    double* part;                       // [B][bpi][2]
    int lds_conf;                       // the confusion counters of this block live in LDS
};

static inline int sem_bpi(int B, long HW) {
    const long by_rows = (HW + SE_ROWS_PER_BLOCK - 1) / SE_ROWS_PER_BLOCK;
    const long by_grid = B >= SE_TARGET_BLOCKS ? 1 : (SE_TARGET_BLOCKS + B - 1) / B;
    return (int)(by_rows < by_grid ? by_rows : by_grid);
}
static constexpr size_t sem_lds_bytes(int C, bool lds_conf) {
    return ((size_t)3 * C + (lds_conf ? (size_t)(C + 1) * C : 0)) * sizeof(unsigned);
}
#define SE_LDS_MAX ((int)sem_lds_bytes(MU_SEM_EVAL_LDS_MAX_C, true))
static_assert(SE_LDS_MAX + 1024 <= 160 * 1024, "the privatised confusion matrix must fit the 160 KiB of a CU");

// offset of pixel row r = b * HW + p: the two layouts a module output has are division-free
__device__ __forceinline__ long sem_row_offset(const SemParams& P, long b, long p) {
    if (P.inner >= P.M) return (b * P.HW + p) * P.ps;                       // NHWC rows: one outer block
    if (P.inner == P.HW) return b * P.outer + p * P.ps;                     // NCHW: one outer block per image
    const long r = b * P.HW + p;
    return (r / P.inner) * P.outer + (r % P.inner) * P.ps;
}

// everything a finished pixel row contributes; called by ONE lane per row
__device__ __forceinline__ void sem_row_out(const SemParams& P, unsigned* hist, unsigned* conf, long r, int arg, long lab, float lse,
                                            float tgt, double s2, double& loss, double& cnt) {
    const int C = P.C;
    const bool counted = lab != P.ignore && lab >= 0 && lab < C;
    if ((unsigned)arg >= (unsigned)C) arg = 0;                               // a row of NaN (outside the contract) must not index past the counters
    atomicAdd(&hist[C + arg], 1u);                                          // P counts every pixel, void ones included
    if (counted) {
        atomicAdd(&hist[2 * C + (int)lab], 1u);
        if ((int)lab == arg) atomicAdd(&hist[arg], 1u);
        loss += (double)(lse - tgt);
        cnt += 1.0;
    }
    const int row = counted ? (int)lab : C;
    if (conf) atomicAdd(&conf[row * C + arg], 1u);
    else atomicAdd(&P.confusion[(long)row * C + arg], 1ull);
    if (P.cls) P.cls[r] = arg;
    if (P.prob) P.prob[r] = (float)(1.0 / s2);
}

// (max, first index of it) over the 16 lanes of a row
__device__ __forceinline__ void sem_argmax16(float& mx, int& arg) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float om = __shfl_xor(mx, o);
        const int oa = __shfl_xor(arg, o);
        if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
    }
}
__device__ __forceinline__ float sem_sum16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double sem_sum16(double v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// The probability sum of one 16-byte vector: a pairwise fp32 tree over its 4 / 8 terms (at most 2 / 3 roundings of 2^-24 on a sum of
// terms in [0, 1]), the vectors and lanes then add in fp64.  A plain fp32 running sum over 150 classes loses several 1e-6 of the
// probability (ArgmaxState, instances.hip); an fp64 add per element costs a convert and a half-rate add per logit.
template <int VN>
__device__ __forceinline__ float sem_tree(const float* t) {
    if (VN == 8) return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    return (t[0] + t[1]) + (t[2] + t[3]);
}

// NV > 0: rows of up to NV * 16 vectors in registers, U rows per lane group and pass.  NV == 0: any width, two passes per row.
template <typename T, int NV, int U, bool PROB>
__global__ __launch_bounds__(SE_THREADS) void sem_eval_vec_kernel(const SemParams P) {
    constexpr int VN = Vec16<T>::N;
    extern __shared__ unsigned se_lds[];
    __shared__ double sh[SE_WAVES * 2];
    const int C = P.C, tid = threadIdx.x, l16 = tid & 15, rowl = tid >> 4;
    unsigned* hist = se_lds;                                   // [3][C]: I, P, L of this block's pixels
    unsigned* conf = P.lds_conf ? se_lds + 3 * C : nullptr;    // [C + 1][C]
    const int nlds = 3 * C + (P.lds_conf ? (C + 1) * C : 0);
    for (int i = tid; i < nlds; i += SE_THREADS) se_lds[i] = 0;
    __syncthreads();
    const long b = blockIdx.x / P.bpi, HW = P.HW;
    const int j = blockIdx.x % P.bpi;
    const T* logits = (const T*)P.logits;
    const long* labels = P.labels + b * HW;
    const int nvec = (C + VN - 1) / VN;                        // vectors that hold a real channel
    const float k2 = P.k2;
    double loss = 0.0, cnt = 0.0;
    constexpr int ROWS = (SE_THREADS / 16) * (NV > 0 ? U : 1);
    for (long p0 = (long)j * ROWS; p0 < HW; p0 += (long)P.bpi * ROWS) {
        if constexpr (NV > 0) {
            Vec16<T> v[U][NV];
            long lab[U];
            bool ok[U];
            const T* base[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long p = p0 + u * (SE_THREADS / 16) + rowl;
                ok[u] = p < HW;
                const long pp = ok[u] ? p : HW - 1;
                lab[u] = labels[pp];
                base[u] = logits + sem_row_offset(P, b, pp);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int vi = k * 16 + l16;
                    if (k + 1 < NV || vi < nvec) v[u][k].load(base[u] + vi * VN);      // only the last turn can lie past the row
                    else v[u][k].zero();
                }
            }
            float tgt[U];
#pragma unroll
            for (int u = 0; u < U; ++u)                        // one more lane-group-uniform load instead of a select per element
                tgt[u] = (lab[u] != P.ignore && lab[u] >= 0 && lab[u] < C) ? (float)base[u][lab[u]] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[NV * VN];
                float mx = -INFINITY;
                int arg = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int c = (k * 16 + l16) * VN;
                    const bool whole = (k + 1) * 16 * VN <= C;                         // uniform: every channel of this turn is real
#pragma unroll
                    for (int i = 0; i < VN; ++i) {
                        const float x = (whole || c + i < C) ? v[u][k].get(i) : -INFINITY;   // padding is never a maximum, exp -> 0
                        f[k * VN + i] = x;
                        if (x > mx) { mx = x; arg = c + i; }                          // ascending channels: the first maximum stays
                    }
                }
                sem_argmax16(mx, arg);
                // x - max first (exact for fp16 logits), then the scale: a rounded max * k folded into an FMA would move EVERY term
                // of the row, the maximum's own 1.0 included, by the same factor (up to 6.6e-7 at |max| k = 23)
                float se = 0.f;
#pragma unroll
                for (int q = 0; q < NV * VN; ++q) {
                    f[q] -= mx;
                    se += __builtin_amdgcn_exp2f(f[q] * SE_LOG2E);
                }
                se = sem_sum16(se);
                double s2 = 1.0;
                if (PROB) {
                    s2 = 0.0;
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        float t[VN];
#pragma unroll
                        for (int i = 0; i < VN; ++i) t[i] = __builtin_amdgcn_exp2f(f[k * VN + i] * k2);
                        s2 += (double)sem_tree<VN>(t);
                    }
                    s2 = sem_sum16(s2);
                }
                if (ok[u] && l16 == 0)
                    sem_row_out(P, hist, conf, b * HW + p0 + u * (SE_THREADS / 16) + rowl, arg, lab[u], mx + __logf(se), tgt[u], s2, loss, cnt);
            }
        } else {
            const long p = p0 + rowl;
            const bool ok = p < HW;
            const long pp = ok ? p : HW - 1;
            const long lab = labels[pp];
            const T* base = logits + sem_row_offset(P, b, pp);
            float mx = -INFINITY;
            int arg = 0x7fffffff;
            for (int vi = l16; vi < nvec; vi += 16) {
                Vec16<T> v;
                v.load(base + vi * VN);
#pragma unroll
                for (int i = 0; i < VN; ++i) {
                    const float x = vi * VN + i < C ? v.get(i) : -INFINITY;
                    if (x > mx) { mx = x; arg = vi * VN + i; }
                }
            }
            sem_argmax16(mx, arg);
            float se = 0.f;
            double s2 = 0.0;
            for (int vi = l16; vi < nvec; vi += 16) {
                Vec16<T> v;
                v.load(base + vi * VN);
                float t[VN];
#pragma unroll
                for (int i = 0; i < VN; ++i) {
                    const float d = (vi * VN + i < C ? v.get(i) : -INFINITY) - mx;
                    se += __builtin_amdgcn_exp2f(d * SE_LOG2E);
                    t[i] = PROB ? __builtin_amdgcn_exp2f(d * k2) : 0.f;
                }
                if (PROB) s2 += (double)sem_tree<VN>(t);
            }
            se = sem_sum16(se);
            s2 = PROB ? sem_sum16(s2) : 1.0;
            const float tgt = (lab != P.ignore && lab >= 0 && lab < C) ? (float)base[lab] : 0.f;
            if (ok && l16 == 0) sem_row_out(P, hist, conf, b * HW + p, arg, lab, mx + __logf(se), tgt, s2, loss, cnt);
        }
    }
    loss = wave_sum_d(loss);
    cnt = wave_sum_d(cnt);
    if ((tid & 63) == 0) { sh[(tid >> 6) * 2] = loss; sh[(tid >> 6) * 2 + 1] = cnt; }
    __syncthreads();                                           // also: every LDS counter of the block is final
    if (tid == 0) {
        double a = 0.0, n = 0.0;
        for (int w = 0; w < SE_WAVES; ++w) { a += sh[w * 2]; n += sh[w * 2 + 1]; }
        P.part[(long)blockIdx.x * 2] = a;
        P.part[(long)blockIdx.x * 2 + 1] = n;
    }
    for (int i = tid; i < 3 * C; i += SE_THREADS)
        if (hist[i]) atomicAdd(&P.img_counts[b * 3 * C + i], (int)hist[i]);
    if (conf)
        for (int i = tid; i < (C + 1) * C; i += SE_THREADS)
            if (conf[i]) atomicAdd(&P.confusion[i], (unsigned long long)conf[i]);
}

// One thread per pixel, channels in ascending order with an online maximum: the lse sum in fp32 (rescaled as ce_nchw_fwd_kernel,
// loss.hip), the probability sum in fp64 (ArgmaxState, instances.hip).  Four loads in flight.
template <typename T>
__global__ __launch_bounds__(SE_STRIDED_THREADS) void sem_eval_strided_kernel(const SemParams P) {
    extern __shared__ unsigned se_lds[];
    __shared__ double sh[(SE_STRIDED_THREADS / 64) * 2];
    const int C = P.C, tid = threadIdx.x;
    unsigned* hist = se_lds;
    unsigned* conf = P.lds_conf ? se_lds + 3 * C : nullptr;
    const int nlds = 3 * C + (P.lds_conf ? (C + 1) * C : 0);
    for (int i = tid; i < nlds; i += SE_STRIDED_THREADS) se_lds[i] = 0;
    __syncthreads();
    const long b = blockIdx.x / P.bpi, HW = P.HW;
    const int j = blockIdx.x % P.bpi;
    const float k2 = P.k2;
    double loss = 0.0, cnt = 0.0;
    for (long p = (long)j * SE_STRIDED_THREADS + tid; p < HW; p += (long)P.bpi * SE_STRIDED_THREADS) {
        const T* base = (const T*)P.logits + sem_row_offset(P, b, p);
        const long lab = P.labels[b * HW + p];
        float m = (float)base[0], s1 = 1.f;
        double s2 = 1.0;
        int arg = 0;
        auto next = [&](float v, int c) {
            if (v > m) {
                s1 = s1 * __builtin_amdgcn_exp2f((m - v) * SE_LOG2E) + 1.f;
                s2 = s2 * (double)__builtin_amdgcn_exp2f((m - v) * k2) + 1.0;
                m = v;
                arg = c;
            } else {
                s1 += __builtin_amdgcn_exp2f((v - m) * SE_LOG2E);
                s2 += (double)__builtin_amdgcn_exp2f((v - m) * k2);
            }
        };
        int c = 1;
        for (; c + 4 <= C; c += 4) {
            const float v0 = (float)base[(long)c * P.cs], v1 = (float)base[(long)(c + 1) * P.cs];
            const float v2 = (float)base[(long)(c + 2) * P.cs], v3 = (float)base[(long)(c + 3) * P.cs];
            next(v0, c);
            next(v1, c + 1);
            next(v2, c + 2);
            next(v3, c + 3);
        }
        for (; c < C; ++c) next((float)base[(long)c * P.cs], c);
        const float tgt = (lab != P.ignore && lab >= 0 && lab < C) ? (float)base[lab * P.cs] : 0.f;
        sem_row_out(P, hist, conf, b * HW + p, arg, lab, m + __logf(s1), tgt, s2, loss, cnt);
    }
    loss = wave_sum_d(loss);
    cnt = wave_sum_d(cnt);
    if ((tid & 63) == 0) { sh[(tid >> 6) * 2] = loss; sh[(tid >> 6) * 2 + 1] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, n = 0.0;
        for (int w = 0; w < SE_STRIDED_THREADS / 64; ++w) { a += sh[w * 2]; n += sh[w * 2 + 1]; }
        P.part[(long)blockIdx.x * 2] = a;
        P.part[(long)blockIdx.x * 2 + 1] = n;
    }
    for (int i = tid; i < 3 * C; i += SE_STRIDED_THREADS)
        if (hist[i]) atomicAdd(&P.img_counts[b * 3 * C + i], (int)hist[i]);
    if (conf)
        for (int i = tid; i < (C + 1) * C; i += SE_STRIDED_THREADS)
            if (conf[i]) atomicAdd(&P.confusion[i], (unsigned long long)conf[i]);
}

// img_loss[b] = the partials of image b's blocks, added in block order
__global__ void sem_loss_final_kernel(const double* __restrict__ part, int B, int bpi, double* __restrict__ img_loss) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double a = 0.0, n = 0.0;
    for (int j = 0; j < bpi; ++j) { a += part[((long)b * bpi + j) * 2]; n += part[((long)b * bpi + j) * 2 + 1]; }
    img_loss[b * 2] = a;
    img_loss[b * 2 + 1] = n;
}

// The sweep kernel of a call, picked before anything is enqueued: its launch, and its LDS grant (common.h: mu_lds_grant), which a call
// asks for only where it needs more than 48 KiB.  The kernels are launched by name: a host object built with the sanitizers drops a launch
// through a kernel-valued template parameter (tools/post_host_launches.cpp would record no sweep).
struct SemSweep {
    void (*launch)(const SemParams& P, int grid, size_t lds, hipStream_t st);
    bool (*grant)(int max_bytes);
};
template <typename T, int NV, int RPW, bool PROB>
static SemSweep sem_sweep_vec_as() {
    return {[](const SemParams& P, int grid, size_t lds, hipStream_t st) { sem_eval_vec_kernel<T, NV, RPW, PROB><<<grid, SE_THREADS, lds, st>>>(P); },
            mu_lds_grant<sem_eval_vec_kernel<T, NV, RPW, PROB>>};
}
template <typename T>
static SemSweep sem_sweep_strided() {
    return {[](const SemParams& P, int grid, size_t lds, hipStream_t st) { sem_eval_strided_kernel<T><<<grid, SE_STRIDED_THREADS, lds, st>>>(P); },
            mu_lds_grant<sem_eval_strided_kernel<T>>};
}
template <typename T, bool PROB>
static SemSweep sem_sweep_vec(const SemParams& P) {
    constexpr int VN = Vec16<T>::N;
    const int nv = (P.C + 16 * VN - 1) / (16 * VN);
    if (nv == 1) return sem_sweep_vec_as<T, 1, 4, PROB>();
    if (nv == 2) return sem_sweep_vec_as<T, 2, 4, PROB>();
    if (nv == 3) return sem_sweep_vec_as<T, 3, 2, PROB>();
    return sem_sweep_vec_as<T, 0, 1, PROB>();
}
template <typename T>
static SemSweep sem_sweep_t(const SemParams& P) {
    constexpr long VN = Vec16<T>::N;
    const long row = (P.C + VN - 1) / VN * VN;                 // what the 16-byte loads of a row touch
    const bool vec = P.cs == 1 && P.ps % VN == 0 && P.outer % VN == 0 && ((uintptr_t)P.logits & 15) == 0 && P.ps >= row;
    if (!vec) return sem_sweep_strided<T>();
    return P.prob ? sem_sweep_vec<T, true>(P) : sem_sweep_vec<T, false>(P);
}

extern "C" int mu_sem_eval_supported(int C) { return C >= 1 && C <= 4096 ? MU_OK : MU_ERR_SHAPE; }

struct SemWs {
    MuCarve c;
    double* part;       // [B][blocks per image][2] (loss sum, counted pixels) of every block
    constexpr SemWs(void* ws, int B, int bpi) : c(ws), part(c.take<double>((long)B * bpi * 2)) {}
};
static_assert(SemWs(nullptr, 2, 3).c.bytes == 2 * 3 * 2 * 8 && SemWs(nullptr, 5, 1).c.bytes == 5 * 2 * 8, "mu_sem_eval workspace");

extern "C" long mu_sem_eval_workspace_bytes(int B, long HW, int C) {
    if (B < 1 || HW < 1 || HW >= (1L << 31) || mu_sem_eval_supported(C) != MU_OK) return 0;
    return SemWs(nullptr, B, sem_bpi(B, HW)).c.bytes;
}

extern "C" int mu_sem_eval(const void* logits, const long* labels, int B, long HW, int C, long inner, long outer_stride, long c_stride,
                           long p_stride, long ignore_index, float inv_temperature, int* img_counts, double* img_loss, long* confusion,
                           int* cls_or_null, float* prob_or_null, void* workspace, long ws_bytes, int dtype, void* stream) {
    if (!logits || !labels || !img_counts || !img_loss || !confusion || !workspace) return MU_ERR_ARG;
    if (B < 1 || HW < 1 || HW >= (1L << 31) || inner < 1 || !(inv_temperature > 0.f)) return MU_ERR_ARG;
    if (dtype != MU_F32 && dtype != MU_F16) return MU_ERR_ARG;
    if (mu_sem_eval_supported(C) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_sem_eval_workspace_bytes(B, HW, C)) return MU_ERR_WORKSPACE;
    const int bpi = sem_bpi(B, HW);
    if ((long)B * bpi > 0x7fffffffL) return MU_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    SemParams P;
    P.logits = logits; P.labels = labels; P.HW = HW; P.M = (long)B * HW; P.C = C; P.bpi = bpi;
    P.inner = inner; P.outer = outer_stride; P.cs = c_stride; P.ps = p_stride;
    P.ignore = ignore_index; P.k2 = inv_temperature * 1.44269504088896340736f;
    P.img_counts = img_counts; P.confusion = (unsigned long long*)confusion; P.cls = cls_or_null; P.prob = prob_or_null;
    P.part = SemWs(workspace, B, bpi).part;
    P.lds_conf = C <= MU_SEM_EVAL_LDS_MAX_C;
    const size_t lds = sem_lds_bytes(C, P.lds_conf);
    SemSweep sweep;
    if (int e = with_storage(dtype, [&](auto tag) -> int { sweep = sem_sweep_t<decltype(tag)>(P); return MU_OK; })) return e;
    if (lds > 48 * 1024 && !sweep.grant(SE_LDS_MAX)) return MU_ERR_LAUNCH;
    if (hipMemsetAsync(img_counts, 0, (size_t)B * 3 * C * sizeof(int), st) != hipSuccess) return MU_ERR_LAUNCH;
    sweep.launch(P, B * bpi, lds, st);
    sem_loss_final_kernel<<<(B + 255) / 256, 256, 0, st>>>(P.part, B, bpi, img_loss);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
