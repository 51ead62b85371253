// COCO run-length masks on the device (gfx950): what mask_to_rle / maskUtils.encode do to every prediction of the evaluation scripts
// (ade_instance.py, ade_panoptic.py, city_instance.py:399-403, city_panoptic.py:176-181, coco_instance.py:351,397) and annToMask
// (coco_instance.py:63) in the other direction.  The format is restated from the published maskApi.c (rleEncode, rleDecode, rleToString,
// rleArea); the contract is spelled out in include/maskunet_hip.h.
//
// mu_rle_encode: one workgroup per image, every selected instance in one pass, no sort.
//   table    id -> row + 1 (integer atomicMin: of equal ids in `sel` the lowest row wins, whatever the order);
//   rowmap   the row + 1 of every pixel in COLUMN-MAJOR order (the walk of the format), 16 bits each: all later passes read it coalesced;
//   events   boundary j (0..N) lies between positions j - 1 and j; where the row changes there, the row left and the row entered get one
//            event (row, j) each.  A row's events in ascending j ARE its boundaries b_0 < b_1 < ...  They are bucketed by row with the
//            stable counting sort of wave_prims.h (wave_segment, wave_sort_chunk), here with two keys per lane (rle_sort_chunk): every
//            wave owns a contiguous range of boundaries and counters of its own per row (no atomics);
//   counts   differences of neighbouring boundaries, one wave per row; the closing count unless the row covers position N - 1;
//   string   per count the 5-bit groups of rleToString; two scans give the offsets (counts per row, characters per row), a wave scan
//            the place of every count's characters inside its row.
// mu_rle_decode: one workgroup per image, one wave per row: the row is checked (sum == N, no negative count), then its odd runs are
// painted with integer atomicMax of row + 1, so overlapping rows give the same map in any order.
// Integer arithmetic only: bit-identical from run to run.
#include "wave_prims.h"

#define RLE_THREADS 512
#define RLE_WAVES (RLE_THREADS / 64)
#define RLE_MAX_PIXELS 65536
#define RLE_MAX_ROWS 4096
#define RLE_MAX_ID 65536
#define RLE_NONE 0x7fffffff

typedef unsigned short rle_u16;

// characters of one value of the string (rleToString): 5 bits each, bit 4 of the last one is the sign.  |x| <= 65536 (a count or
// the difference of two) takes at most 4; they are returned packed, first character in the low byte
__device__ __forceinline__ int rle_chars(int x, unsigned& packed) {
    int n = 0;
    bool more;
    packed = 0u;
    do {
        int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        packed |= (unsigned)(c + 48) << (8 * n);
        ++n;
    } while (more && n < 4);
    return n;
}

// count i of a row with m boundaries bnd[0..m) (i <= m; i == m is the closing count)
__device__ __forceinline__ int rle_count(const int* bnd, int m, int N, int i) {
    const int hi = i < m ? bnd[i] : N;
    return hi - (i > 0 ? bnd[i - 1] : 0);
}
// the value the string holds for count i: the count itself, from the fourth on its difference to the count two before
__device__ __forceinline__ int rle_value(const int* bnd, int m, int N, int i) {
    const int c = rle_count(bnd, m, N, i);
    return i > 2 ? c - rle_count(bnd, m, N, i - 2) : c;
}

struct RleParams {
    const int *ids, *sel;
    int N, H, W, K, max_id, L;                         // L = 2 * N + K: the counts of an image
    long ws_stride;                                    // ints of workspace per image
    int *offsets, *counts, *area, *str_offsets;
    unsigned char* str_bytes;
    int* ws;                                           // per image: int table[max_id + 1], int bnd[2 * N], u16 rowmap[N]
};

// One 64-boundary chunk of the bucketing of the events by row: wave_sort_chunk (wave_prims.h) with two keys per lane.  `leave` / `enter`
// = row + 1 of the run that ends / starts at boundary j (this lane's; j < hi <= N + 1), 0 where there is none.  A row never does both
// at one boundary, and both events of a row are peeled in ONE round, so a row's events keep their order along the walk.
// mine[] = the wave's own counters.  PLACE: the event goes to bnd[ev0[row] + counter + (the row's events in the lanes below)].
template <bool PLACE>
__device__ __forceinline__ void rle_sort_chunk(const rle_u16* rowmap, int N, int j, int hi, int lane, rle_u16* mine, const int* ev0,
                                               int* bnd) {
    int leave = 0, enter = 0;
    if (j < hi) {
        const int prev = j > 0 ? rowmap[j - 1] : 0, cur = j < N ? rowmap[j] : 0;
        if (prev != cur) {
            leave = prev;
            enter = cur;
        }
    }
    unsigned long long rem_l = __ballot(leave != 0), rem_e = __ballot(enter != 0);
    while (rem_l | rem_e) {
        const int r0 = rem_l ? __shfl(leave, __ffsll((long long)rem_l) - 1) : __shfl(enter, __ffsll((long long)rem_e) - 1);
        const unsigned long long ml = __ballot(leave == r0), me = __ballot(enter == r0);
        const int at = mine[r0 - 1];
        if (PLACE && (leave == r0 || enter == r0)) bnd[ev0[r0 - 1] + at + __popcll((ml | me) & lanes_below(lane))] = j;
        if (lane == 0) mine[r0 - 1] = (rle_u16)(at + __popcll(ml) + __popcll(me));
        rem_l &= ~ml;
        rem_e &= ~me;
    }
}

// Dynamic LDS: int m[K] (events per row), ev0[K] (first event), off[K] (first count), soff[K] (characters, then the first character),
// then u16 wcnt[RLE_WAVES][K], then int totals[2] (counts, characters of the image): 128 KiB at 4096 rows.
__global__ __launch_bounds__(RLE_THREADS) void rle_encode_kernel(const RleParams P) {
    extern __shared__ unsigned rle_lds[];
    const int N = P.N, H = P.H, W = P.W, K = P.K, L = P.L;
    int* m_of = (int*)rle_lds;
    int* ev0 = m_of + K;
    int* off = ev0 + K;
    int* soff = off + K;
    rle_u16* wcnt = (rle_u16*)(soff + K);
    int* totals = (int*)(wcnt + RLE_WAVES * K);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* ids = P.ids + (long)b * N;
    const int* sel = P.sel + (long)b * K;
    int* table = P.ws + (long)b * P.ws_stride;
    int* bnd = table + P.max_id + 1;
    rle_u16* rowmap = (rle_u16*)(bnd + 2 * (long)N);
    int* offsets = P.offsets + (long)b * (K + 1);
    int* counts = P.counts + (long)b * L;
    int* area = P.area + (long)b * K;
    int* str_offsets = P.str_offsets + (long)b * (K + 1);
    unsigned char* str = P.str_bytes + (long)b * L * 4;

    for (int i = tid; i <= P.max_id; i += RLE_THREADS) table[i] = RLE_NONE;
    for (int k = tid; k < K; k += RLE_THREADS) m_of[k] = 0;
    for (int k = tid; k < RLE_WAVES * K; k += RLE_THREADS) wcnt[k] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += RLE_THREADS) {
        const int s = sel[k];
        if (s >= 1 && s <= P.max_id) atomicMin(&table[s], k + 1);
    }
    __syncthreads();

    // the walk: position j = x * H + y
    for (int j = tid; j < N; j += RLE_THREADS) {
        const int x = j / H, y = j - x * H;
        const int id = ids[y * W + x];
        int r = 0;
        if (id >= 1 && id <= P.max_id) {
            const int t = mu_ld_agent(table + id);             // written by atomicMin of other waves
            if (t != RLE_NONE) r = t;
        }
        rowmap[j] = (rle_u16)r;
    }
    __syncthreads();                                   // rowmap (global memory, same workgroup) is visible past this barrier

    // events per (wave, row): every wave over its segment of at most span = 8256 of the boundaries 0..N.  A row has at most one event
    // per boundary, so a wave's counter is at most span and the events of the waves before it at most 7 * span < 65536: 16 bits hold both.
    int lo, hi;
    wave_segment(N + 1, RLE_WAVES, wave, lo, hi);
    rle_u16* mine = wcnt + wave * K;
    for (int base = lo; base < hi; base += 64) rle_sort_chunk<false>(rowmap, N, base + lane, hi, lane, mine, ev0, bnd);
    __syncthreads();

    // per row: exclusive prefix over the waves, events m, counts n = m + 1 unless the row covers the last position
    const int last_row = rowmap[N - 1];
    for (int k = tid; k < K; k += RLE_THREADS) {
        int run = 0;
        for (int v = 0; v < RLE_WAVES; ++v) {
            const int t = wcnt[v * K + k];
            wcnt[v * K + k] = (rle_u16)run;
            run += t;
        }
        m_of[k] = run;
        const int s = sel[k];
        off[k] = (s >= 1 && s <= P.max_id) ? run + (last_row != k + 1 ? 1 : 0) : 0;
    }
    __syncthreads();
    if (wave == 0) {
        wave_scan_excl_array(m_of, ev0, K, lane);
        for (int k = lane; k < K; k += 64) soff[k] = off[k];                 // n per row, kept until the counts are written
        const int total = wave_scan_excl_array(off, off, K, lane);
        for (int k = lane; k < K; k += 64) offsets[k] = off[k];
        if (lane == 0) {
            offsets[K] = total;
            totals[0] = total;
        }
    }
    __syncthreads();

    // placement, stable: the same walk
    for (int base = lo; base < hi; base += 64) rle_sort_chunk<true>(rowmap, N, base + lane, hi, lane, mine, ev0, bnd);
    __syncthreads();                                   // bnd (global memory, same workgroup) is visible past this barrier

    // counts, area and the characters per row: one wave per row
    for (int k = wave; k < K; k += RLE_WAVES) {
        const int n = soff[k], m = m_of[k];
        const int* rb = bnd + ev0[k];
        int a = 0, ch = 0;
        for (int i = lane; i < n; i += 64) {
            const int c = rle_count(rb, m, N, i);
            unsigned packed;
            counts[off[k] + i] = c;
            if (i & 1) a += c;
            ch += rle_chars(i > 2 ? c - rle_count(rb, m, N, i - 2) : c, packed);
        }
        a = wave_sum(a);
        ch = wave_sum(ch);
        if (lane == 0) {                               // soff[k] belongs to the wave that owns row k
            area[k] = a;
            soff[k] = ch;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int total = wave_scan_excl_array(soff, soff, K, lane);
        for (int k = lane; k < K; k += 64) str_offsets[k] = soff[k];
        if (lane == 0) {
            str_offsets[K] = total;
            totals[1] = total;
        }
    }
    __syncthreads();

    // the strings: one wave per row, a running offset over the row's counts
    for (int k = wave; k < K; k += RLE_WAVES) {
        const int m = m_of[k];
        const int n = (k + 1 < K ? off[k + 1] : totals[0]) - off[k];
        const int* rb = bnd + ev0[k];
        int carry = soff[k];
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            unsigned packed = 0u;
            const int nc = i < n ? rle_chars(rle_value(rb, m, N, i), packed) : 0;
            unsigned char* dst = str + wave_scan_excl(nc, lane, carry);
            for (int q = 0; q < nc; ++q) dst[q] = (unsigned char)(packed >> (8 * q));
        }
    }
    // the unused tails are zero
    for (int i = totals[0] + tid; i < L; i += RLE_THREADS) counts[i] = 0;
    const int used = totals[1], word0 = (used + 3) & ~3;
    if (tid < word0 - used) str[used + tid] = 0;
    int* strw = (int*)str;                             // 4 * L bytes per image: every image starts on a word
    for (int i = word0 / 4 + tid; i < L; i += RLE_THREADS) strw[i] = 0;
}

// dynamic LDS of rle_encode_kernel; granted to the most it can ask for (common.h: mu_lds_grant)
static constexpr size_t rle_lds_bytes(int K) { return (size_t)K * (4 * sizeof(int) + RLE_WAVES * sizeof(rle_u16)) + 2 * sizeof(int); }
#define RLE_LDS_MAX ((int)rle_lds_bytes(RLE_MAX_ROWS))

extern "C" int mu_rle_encode_supported(int H, int W, int K, int max_id) {
    if (H <= 0 || W <= 0 || (long)H * W > RLE_MAX_PIXELS) return MU_ERR_SHAPE;
    if (K < 1 || K > RLE_MAX_ROWS || max_id < 1 || max_id > RLE_MAX_ID) return MU_ERR_SHAPE;
    return MU_OK;
}

// ints of workspace per image, carved by the kernel: table [max_id + 1], bnd [2 N], rowmap [N] as 16-bit values
static constexpr long rle_ws_ints(long N, int max_id) { return (long)max_id + 1 + 2 * N + (N + 1) / 2; }
struct RleWs {
    MuCarve c;
    int* images;    // [B][rle_ws_ints] one slab per image (RleParams::ws, ws_stride)
    constexpr RleWs(void* ws, int B, long N, int max_id) : c(ws), images(c.take<int>((long)B * rle_ws_ints(N, max_id))) {}
};
static_assert(RleWs(nullptr, 2, 63, 5).c.bytes == 2L * (5 + 1 + 2 * 63 + 32) * 4 && RleWs(nullptr, 3, 64, 8).c.bytes == 3L * (8 + 1 + 2 * 64 + 32) * 4,
              "mu_rle_encode workspace");

extern "C" long mu_rle_encode_workspace_bytes(int B, int H, int W, int K, int max_id) {
    if (B <= 0 || mu_rle_encode_supported(H, W, K, max_id) != MU_OK) return 0;
    return RleWs(nullptr, B, (long)H * W, max_id).c.bytes;
}

extern "C" int mu_rle_encode(const int* ids, const int* sel, int B, int H, int W, int K, int max_id, int* offsets, int* counts, int* area,
                             int* str_offsets, unsigned char* str_bytes, void* workspace, long ws_bytes, void* stream) {
    if (!ids || !sel || !offsets || !counts || !area || !str_offsets || !str_bytes || !workspace || B <= 0 || H <= 0 || W <= 0)
        return MU_ERR_ARG;
    if ((uintptr_t)str_bytes & 3) return MU_ERR_ARG;      // the tail of the strings is zeroed by words
    if (mu_rle_encode_supported(H, W, K, max_id) != MU_OK) return MU_ERR_SHAPE;
    if (ws_bytes < mu_rle_encode_workspace_bytes(B, H, W, K, max_id)) return MU_ERR_WORKSPACE;
    if (!mu_lds_grant<rle_encode_kernel>(RLE_LDS_MAX)) return MU_ERR_LAUNCH;
    RleParams P;
    P.ids = ids;
    P.sel = sel;
    P.N = H * W;
    P.H = H;
    P.W = W;
    P.K = K;
    P.max_id = max_id;
    P.L = 2 * P.N + K;
    P.ws_stride = rle_ws_ints(P.N, max_id);
    P.offsets = offsets;
    P.counts = counts;
    P.area = area;
    P.str_offsets = str_offsets;
    P.str_bytes = str_bytes;
    P.ws = RleWs(workspace, B, P.N, max_id).images;
    rle_encode_kernel<<<B, RLE_THREADS, rle_lds_bytes(K), (hipStream_t)stream>>>(P);
    MU_CHECK_LAUNCH();
    return MU_OK;
}

// ------------------------------------------------------------------------------------------
// Decode.  Runs of at most RLE_SHORT_RUN positions are painted by the lane that holds them; longer ones by the whole wave, one after
// the other (a full-image run in one lane would be 65536 atomics in a row).
// ------------------------------------------------------------------------------------------
#define RLE_SHORT_RUN 16

__device__ __forceinline__ void rle_paint(int* ids, int H, int W, int p, int v) {
    const int x = p / H, y = p - x * H;
    atomicMax(&ids[y * W + x], v);
}

__global__ __launch_bounds__(RLE_THREADS) void rle_decode_kernel(const int* __restrict__ offsets_all, const int* __restrict__ counts_all,
                                                                  int N, int H, int W, int K, long L, int* __restrict__ ids_all,
                                                                  int* __restrict__ valid_all) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* offsets = offsets_all + (long)b * (K + 1);
    const int* counts = counts_all + (long)b * L;
    int* ids = ids_all + (long)b * N;
    for (int i = tid; i < N; i += RLE_THREADS) ids[i] = 0;
    __syncthreads();
    for (int k = wave; k < K; k += RLE_WAVES) {
        const long o0 = offsets[k], o1 = offsets[k + 1];
        bool ok = o0 >= 0 && o0 <= o1 && o1 <= L;
        const int n = ok ? (int)(o1 - o0) : 0;
        const int* rc = counts + o0;
        long long sum = 0;
        int bad = 0;
        for (int i = lane; i < n; i += 64) {
            const int c = rc[i];
            bad |= (c < 0 || c > N);
            sum += c;
        }
        ok = ok && __ballot(bad != 0) == 0ull && (long long)wave_sum((unsigned long long)sum) == (long long)N;
        if (lane == 0) valid_all[(long)b * K + k] = ok ? 1 : 0;
        if (!ok) continue;
        int carry = 0;                                  // every count is in 0..N and they sum to N from here on
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const int c = i < n ? rc[i] : 0;
            const int start = wave_scan_excl(c, lane, carry);
            const bool one = (i & 1) && c > 0;
            if (one && c <= RLE_SHORT_RUN)
                for (int p = start; p < start + c; ++p) rle_paint(ids, H, W, p, k + 1);
            unsigned long long big = __ballot(one && c > RLE_SHORT_RUN);
            while (big) {
                const int l = __ffsll((long long)big) - 1;
                big &= big - 1ull;
                const int s0 = __shfl(start, l), len = __shfl(c, l);
                for (int p = s0 + lane; p < s0 + len; p += 64) rle_paint(ids, H, W, p, k + 1);
            }
        }
    }
}

extern "C" int mu_rle_decode_supported(int H, int W, int K) {
    if (H <= 0 || W <= 0 || (long)H * W > RLE_MAX_PIXELS || K < 1 || K > RLE_MAX_ROWS) return MU_ERR_SHAPE;
    return MU_OK;
}

extern "C" int mu_rle_decode(const int* offsets, const int* counts, int B, int H, int W, int K, long counts_per_image, int* ids,
                             int* valid, void* stream) {
    if (!offsets || !counts || !ids || !valid || B <= 0 || H <= 0 || W <= 0 || counts_per_image < 1 || counts_per_image > 0x7fffffffL)
        return MU_ERR_ARG;
    if (mu_rle_decode_supported(H, W, K) != MU_OK) return MU_ERR_SHAPE;
    rle_decode_kernel<<<B, RLE_THREADS, 0, (hipStream_t)stream>>>(offsets, counts, H * W, H, W, K, counts_per_image, ids, valid);
    MU_CHECK_LAUNCH();
    return MU_OK;
}
