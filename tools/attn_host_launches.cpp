// Stand-alone launch recorder for the host halves of maskunet_amd/csrc/attn.hip and attn_wide.hip: what every mu_attn_* entry point (and
// the six row entries of the generic path, and mu_split_encode_h) returns, sizes and WOULD enqueue -- kernel instantiation, grid, block,
// dynamic LDS, every scalar argument by value, every pointer argument as an offset into the buffer it was derived from, and the memset of
// dqkv as a pseudo-launch -- without a GPU and without the HIP runtime (tools/host_launches.h).  Two trees whose outputs are equal make
// the same launches for every row, so it is the check of a host-only change to these files, and the target of the host sanitizers.
//
// Build (from the repository root; S1 / S2 = the one undefined __hip_fatbin_* symbol of each object, as `nm` prints it):
//   F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-value -Wno-pass-failed"                        # csrc/Makefile: FLAGS
//   hipcc $F -fno-slp-vectorize --cuda-host-only -c maskunet_amd/csrc/attn.hip -o /tmp/attn_host.o          # + FLAGS_attn
//   hipcc $F --cuda-host-only -c maskunet_amd/csrc/attn_wide.hip -o /tmp/attn_wide_host.o
//   D=$(for o in /tmp/attn_host.o /tmp/attn_wide_host.o; do nm $o | awk '$1 == "U" && $2 ~ /^__hip_fatbin_/ {print "-Wl,--defsym=" $2 "=0"}'; done)
//   hipcc -O1 -g -std=c++17 -x c++ tools/attn_host_launches.cpp -x none /tmp/attn_host.o /tmp/attn_wide_host.o -rdynamic -ldl $D -o /tmp/attn_host_launches
// Host sanitizers: add `-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined` to the two object lines and
// `-fsanitize=address,undefined -fno-sanitize-recover=undefined` to the last.
//
// Rows `B N C c_valid nkmax` arrive on stdin.  The row set that straddles every threshold of the two files -- N around 128 (forward / dQ
// grid), B * N around 64, 65536 and 262144 (the rows / 64 clamps), B * N * C / 8 around 8192 * 512 (encode grid cap; B = 64, N = 4096,
// C = 128 is exactly the cap), nkmax around 64, 128 and 192 (the dK/dV tile per dtype at each C), nkmax == N and != N, N % 4 != 0, every
// width and refused widths, c_valid 1 / C - 1 / C, and the (N, C) of every attention block of maskunet_amd/modules.py at the benchmark's
// sizes (B = 64, 128 x 128 input):
//   python -c "
//   S = [(1, 60), (1, 64), (1, 68), (1, 124), (1, 126), (1, 128), (1, 132), (2, 36), (2, 64), (3, 127), (1, 196), (16, 4092), (16, 4096), (16, 4100), (64, 4092),
//        (64, 4096), (64, 4100)]
//   for C in (32, 64, 128, 256, 0, 16, 96, 512):
//       for cv in sorted({1, C - 1, C}):
//           for B, N in S:
//               for nk in sorted({k for k in (63, 64, 65, 127, 128, 129, 191, 192, 193) if k <= N} | {N}): print(B, N, C, cv, nk)
//   for N, C in ((4096, 128), (1024, 256), (256, 256), (1024, 128), (4096, 64), (16384, 64)): print(64, N, C, C, N)" | /tmp/attn_host_launches > launches.txt
// Per row and dtype: the workspace query, the forward's launches, the backward's for phases 1, 2, 4 and 7 each with the flag bits 0, 8, 16
// and 24, the smallest workspace the backward accepts, then the refusing tuples of both `_padded` entries -- the row's call with one fault
// and with two, one letter per call (0 ok, A MU_ERR_ARG, S MU_ERR_SHAPE, L MU_ERR_LAUNCH, W MU_ERR_WORKSPACE) and the number of launches,
// memsets included, that the REFUSED calls among them made (a refused call enqueues nothing: 0).  With c_valid == C the forwarding entries
// (mu_attn_fwd, mu_attn_bwd_phases, mu_attn_bwd) are recorded too.  After the rows: the six attn_wide entries either side of their
// 4096-block cap and mu_split_encode_h either side of its 8192-block cap, every dtype code.
#include "../include/maskunet_hip.h"

static const char* const BUF_NAMES[] = {nullptr, "qkv", "x", "oattn", "gout", "kidx", "kcnt", "lse2", "mean", "rstd", "gamma", "beta", "out",
                                        "dY", "delta", "dqkv", "dgamma", "dbeta", "ws", "src", "dst"};
enum Buf { B_QKV = 1, B_X, B_OATTN, B_GOUT, B_KIDX, B_KCNT, B_LSE2, B_MEAN, B_RSTD, B_GAMMA, B_BETA, B_OUT, B_DY, B_DELTA, B_DQKV, B_DGAMMA,
           B_DBETA, B_WS, B_SRC, B_DST, B_COUNT };
#include "host_launches.h"

// ---- one argument tuple for both directions ------------------------------------------------------------------------------------------
enum { NPTR_FWD = 11, NPTR_BWD = 16 };
struct Args {
    void* p[B_COUNT];          // indexed by Buf
    int B, N, C, cv, nkmax, dtype, phases;
    long ws_bytes;
    float eps;
};
// the pointer arguments of each entry in signature order (what the null-pointer faults walk over)
static const int FWD_PTRS[NPTR_FWD] = {B_QKV, B_X, B_KIDX, B_KCNT, B_GAMMA, B_BETA, B_OUT, B_OATTN, B_LSE2, B_MEAN, B_RSTD};
static const int BWD_PTRS[NPTR_BWD] = {B_QKV, B_X, B_OATTN, B_GOUT, B_KIDX, B_KCNT, B_LSE2, B_MEAN, B_RSTD, B_GAMMA, B_DY, B_DELTA, B_DQKV,
                                       B_DGAMMA, B_DBETA, B_WS};
enum Entry { E_FWD_PADDED, E_BWD_PADDED, E_FWD, E_BWD_PHASES, E_BWD, E_COUNT };
static const char* const ENTRY_NAMES[E_COUNT] = {"fwd_padded", "bwd_phases_padded", "fwd", "bwd_phases", "bwd"};
static long g_calls = 0;

static int call(int e, const Args& a) {
    ++g_calls;
    void* const* p = a.p;
    const int *kidx = (const int*)p[B_KIDX], *kcnt = (const int*)p[B_KCNT];
    float *lse2 = (float*)p[B_LSE2], *mean = (float*)p[B_MEAN], *rstd = (float*)p[B_RSTD], *gamma = (float*)p[B_GAMMA], *beta = (float*)p[B_BETA];
    float *delta = (float*)p[B_DELTA], *dg = (float*)p[B_DGAMMA], *db = (float*)p[B_DBETA];
    switch (e) {
    case E_FWD_PADDED:
        return mu_attn_fwd_padded(p[B_QKV], p[B_X], kidx, kcnt, gamma, beta, p[B_OUT], p[B_OATTN], lse2, mean, rstd, a.B, a.N, a.C, a.cv, a.nkmax, a.eps,
                                  a.dtype, nullptr);
    case E_FWD:
        return mu_attn_fwd(p[B_QKV], p[B_X], kidx, kcnt, gamma, beta, p[B_OUT], p[B_OATTN], lse2, mean, rstd, a.B, a.N, a.C, a.nkmax, a.eps, a.dtype, nullptr);
    case E_BWD_PADDED:
        return mu_attn_bwd_phases_padded(p[B_QKV], p[B_X], p[B_OATTN], p[B_GOUT], kidx, kcnt, lse2, mean, rstd, gamma, p[B_DY], delta, p[B_DQKV], dg, db,
                                         a.B, a.N, a.C, a.cv, a.nkmax, p[B_WS], a.ws_bytes, a.dtype, a.phases, nullptr);
    case E_BWD_PHASES:
        return mu_attn_bwd_phases(p[B_QKV], p[B_X], p[B_OATTN], p[B_GOUT], kidx, kcnt, lse2, mean, rstd, gamma, p[B_DY], delta, p[B_DQKV], dg, db, a.B, a.N,
                                  a.C, a.nkmax, p[B_WS], a.ws_bytes, a.dtype, a.phases, nullptr);
    case E_BWD:
        return mu_attn_bwd(p[B_QKV], p[B_X], p[B_OATTN], p[B_GOUT], kidx, kcnt, lse2, mean, rstd, gamma, p[B_DY], delta, p[B_DQKV], dg, db, a.B, a.N, a.C,
                           a.nkmax, p[B_WS], a.ws_bytes, a.dtype, nullptr);
    }
    return 1;
}

// the faults of the refusing tuples: each edits the valid tuple of the entry (a null-pointer fault beyond the entry's pointer list leaves
// the call valid).  The workspace faults come last: applied after a fault that changes the query's arguments, they are short of the
// query of the tuple as it then stands; every other call of the fault loops has an ample workspace.
enum Fault {
    F_NULL0, F_NULL_LAST = F_NULL0 + NPTR_BWD - 1, F_B_ZERO, F_N_NEG, F_NK_ZERO, F_CV_ZERO, F_CV_BIG, F_DTYPE, F_N_6, F_N_ODD, F_C_96, F_C_512,
    F_WS_ZERO, F_WS_SHORT, F_COUNT
};
static void apply(int f, int e, Args& a) {
    if (f >= F_NULL0 && f <= F_NULL_LAST) {
        const int i = f - F_NULL0;
        if (e == E_FWD_PADDED) { if (i < NPTR_FWD) a.p[FWD_PTRS[i]] = nullptr; }
        else a.p[BWD_PTRS[i]] = nullptr;
        return;
    }
    switch (f) {
    case F_B_ZERO: a.B = 0; break;
    case F_N_NEG: a.N = -1; break;
    case F_NK_ZERO: a.nkmax = 0; break;
    case F_CV_ZERO: a.cv = 0; break;
    case F_CV_BIG: a.cv = a.C + 1; break;
    case F_DTYPE: a.dtype = 7; break;
    case F_N_6: a.N = 6; break;
    case F_N_ODD: a.N += 1; break;
    case F_C_96: a.C = 96; break;                              // a multiple of 32 the sweeps have no width for
    case F_C_512: a.C = 512; break;
    case F_WS_ZERO: a.ws_bytes = 0; break;
    case F_WS_SHORT: a.ws_bytes = mu_attn_bwd_workspace_bytes(a.B, a.N, a.C) - 1; break;
    }
}

static void run(const char* tag, int e, const Args& a) {
    g_launches.clear();
    const int rc = call(e, a);
    printf("  %s -> %d, %zu launches\n", tag, rc, g_launches.size());
    for (const Launch& l : g_launches) printf("    %s\n", l.text.c_str());
}
// smallest ws_bytes the backward accepts for the tuple (bisection between 0 and the query; -1: it refuses the query's size too)
static long smallest_workspace(Args a) {
    g_record = false;
    long lo = 0, hi = a.ws_bytes;
    if (call(E_BWD_PADDED, a) != MU_OK) hi = -1;
    while (hi > 0 && lo + 1 < hi) {
        a.ws_bytes = lo + (hi - lo) / 2;
        (call(E_BWD_PADDED, a) == MU_OK ? hi : lo) = a.ws_bytes;
    }
    g_record = true;
    g_launches.clear();
    return hi;
}
// the code of one call of the fault loops, and the launches it made if it was refused
static char refused(int e, const Args& a, size_t& enqueued) {
    const size_t before = g_launches.size();
    const int rc = call(e, a);
    if (rc != MU_OK) enqueued += g_launches.size() - before;
    return letter(rc);
}

static void wide_entries() {
    static const long ROWS[] = {1, 4095, 4096, 4097, 16383, 16384, 16385, 16388, 16389};
    void *src = buf(B_SRC), *dst = buf(B_DST), *x = buf(B_X), *out = buf(B_OUT);
    const int *idx = (const int*)buf(B_KIDX), *cnt = (const int*)buf(B_KCNT);
    float *mean = (float*)buf(B_MEAN), *rstd = (float*)buf(B_RSTD), *gamma = (float*)buf(B_GAMMA), *beta = (float*)buf(B_BETA);
    for (int dtype : {MU_F32, MU_F16, MU_F32X, 7})
        for (long n : ROWS) {
            printf("wide dtype %d n %ld\n", dtype, n);
            auto show = [&](const char* tag, int rc) {
                printf("  %s -> %d, %zu launches\n", tag, rc, g_launches.size());
                for (const Launch& l : g_launches) printf("    %s\n", l.text.c_str());
                g_launches.clear();
            };
            g_launches.clear();
            show("gather_rows", mu_gather_rows(src, 3 * 288, idx, cnt, dst, (int)n, 288, dtype, nullptr));
            show("scatter_rows", mu_scatter_rows((const float*)src, idx, cnt, dst, 3 * 288, (int)n, 288, dtype, nullptr));
            show("softmax_rows", mu_softmax_rows(dst, (int)n, 96, cnt, 0.25f, dtype, nullptr));
            show("attn_wide_ds", mu_attn_wide_ds(src, dst, (int)n, 96, cnt, 0.25f, dtype, nullptr));
            show("ln_rows_fwd", mu_ln_rows_fwd(src, x, gamma, beta, out, mean, rstd, n, 288, 280, 1e-5f, dtype, nullptr));
            show("ln_rows_bwd", mu_ln_rows_bwd(src, dst, x, mean, rstd, gamma, out, buf(B_DY), n, 288, 280, dtype, nullptr));
        }
    for (long n : {0L, 7L, 8L, 4096L, 8192L * 512 * 8 - 8, 8192L * 512 * 8, 8192L * 512 * 8 + 8, 1L << 40}) {
        g_launches.clear();
        const int rc = mu_split_encode_h(src, dst, n, nullptr);
        printf("split_encode_h n %ld -> %d, %zu launches\n", n, rc, g_launches.size());
        for (const Launch& l : g_launches) printf("    %s\n", l.text.c_str());
    }
}

int main() {
    static const char* const DT[3] = {"fp32", "fp16", "fp32x"};
    static const int PHASES[4] = {1, 2, 4, 7}, FLAGS[4] = {0, MU_ATTN_KIDX_PERMUTATION, MU_ATTN_DQKV_ENCODED, MU_ATTN_KIDX_PERMUTATION | MU_ATTN_DQKV_ENCODED};
    int B, N, C, cv, nkmax;
    long rows = 0;
    while (scanf("%d %d %d %d %d", &B, &N, &C, &cv, &nkmax) == 5) {
        ++rows;
        const long ws_q = mu_attn_bwd_workspace_bytes(B, N, C);
        printf("row %d %d %d %d %d\n workspace %ld\n", B, N, C, cv, nkmax, ws_q);
        Args v = {};
        for (int b = 1; b < B_COUNT; ++b) v.p[b] = buf(b);
        v.B = B; v.N = N; v.C = C; v.cv = cv; v.nkmax = nkmax; v.phases = 7; v.ws_bytes = ws_q; v.eps = 1e-5f;
        for (int d = 0; d < 3; ++d) {
            Args a = v;
            a.dtype = d;
            printf(" %s:\n", DT[d]);
            run("fwd_padded", E_FWD_PADDED, a);
            for (int ph : PHASES)
                for (int fl : FLAGS) {
                    a.phases = ph | fl;
                    char tag[48];
                    snprintf(tag, sizeof tag, "bwd_phases_padded phases %d flags %d", ph, fl);
                    run(tag, E_BWD_PADDED, a);
                }
            a.phases = 7;
            if (cv == C) {
                run("fwd", E_FWD, a);
                run("bwd_phases 7", E_BWD_PHASES, a);
                run("bwd", E_BWD, a);
            }
            printf("  smallest workspace %ld\n", smallest_workspace(a));
        }
        // refusing tuples: one fault, then every pair
        g_record = false;
        for (int e : {E_FWD_PADDED, E_BWD_PADDED})
            for (int d = 0; d < 3; ++d) {
                Args a = v;
                a.dtype = d;
                a.ws_bytes = 1L << 60;
                std::string codes;
                size_t enqueued = 0;
                g_launches.clear();
                for (int f = 0; f < F_COUNT; ++f) {
                    Args n = a;
                    apply(f, e, n);
                    codes += refused(e, n, enqueued);
                }
                codes += ' ';
                for (int f = 0; f < F_COUNT; ++f)
                    for (int g = f + 1; g < F_COUNT; ++g) {
                        Args n = a;
                        apply(f, e, n);
                        apply(g, e, n);
                        codes += refused(e, n, enqueued);
                    }
                printf(" faults %s %s: %s, %zu launches by refused calls\n", ENTRY_NAMES[e], DT[d], codes.c_str(), enqueued);
            }
        g_record = true;
        g_launches.clear();
    }
    wide_entries();
    printf("%ld rows, %ld calls\n", rows, g_calls);
    return 0;
}
