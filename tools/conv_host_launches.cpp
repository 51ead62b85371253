// Stand-alone launch recorder for the host half of maskunet_amd/csrc/conv.hip: what every mu_conv_* entry point returns, plans, sizes
// and WOULD launch (kernel instantiation, grid, block, dynamic LDS, every scalar argument by value, every pointer argument as an offset
// into the buffer it was derived from) -- without a GPU and without the HIP runtime.  tools/host_launches.h defines the few runtime symbols the
// host code of a HIP object refers to; hipLaunchKernel records instead of launching.  Two trees whose outputs are equal make the same
// launches for every row, so it is the check of a host-only change to conv.hip, and the target of the host sanitizers.
//
// Build (from the repository root; S = the one undefined __hip_fatbin_* symbol of the object, as `nm` prints it):
//   F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-value -Wno-pass-failed -fno-slp-vectorize"      # csrc/Makefile: FLAGS + FLAGS_conv
//   hipcc $F --cuda-host-only -c maskunet_amd/csrc/conv.hip -o /tmp/conv_host.o
//   S=$(nm /tmp/conv_host.o | awk '$1 == "U" && $2 ~ /^__hip_fatbin_/ {print $2}')
//   hipcc -O1 -g -std=c++17 -x c++ tools/conv_host_launches.cpp -x none /tmp/conv_host.o -rdynamic -ldl -Wl,--defsym=$S=0 -o /tmp/conv_host_launches
// Host sanitizers: add `-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined` to the first line and
// `-fsanitize=address,undefined -fno-sanitize-recover=undefined` to the last.
//
// Rows `B H W Cin Cout taps cin_valid` arrive on stdin.  The row set that straddles every threshold of the file:
//   python -c "import itertools as I; from tests import _conv_cases as C; from tests.test_conv_plan_coverage import MODEL_PLANS as P
//   for c in C.LAYERS: print(c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps'], c['cin'])
//   for (B, hw, ci, co, t, cv) in P: print(B, hw, hw, ci, co, t, cv)
//   for B, H, W, ci, co, t in I.product((1, 2, 3, 64), (5, 8, 16, 32), (7, 16, 32, 64, 96, 160, 288), *[(32, 64, 96, 128, 160, 192, 256, 512, 576)] * 2, (1, 9)):
//       for cv in ((ci, 3) if ci == 32 else (ci,)): print(B, H, W, ci, co, t, cv)" | /tmp/conv_host_launches > launches.txt
// Per row: every entry point in every dtype (code, plan id and name, statistics rows, both workspace queries, the launches), the smallest
// workspace each weight-gradient entry accepts, then the refusing tuples -- the row's call with one fault and with two, one letter per
// call (0 ok, A MU_ERR_ARG, S MU_ERR_SHAPE, L MU_ERR_LAUNCH, W MU_ERR_WORKSPACE) and the number of launches those calls made.
#include "../include/maskunet_hip.h"

// the buffers of a call (tools/host_launches.h: a pointer argument names its range)
static const char* const BUF_NAMES[] = {nullptr, "x", "w", "bias", "y", "scale", "res", "stat", "dyscale", "dw", "db", "ws"};
enum Buf { B_X = 1, B_W, B_BIAS, B_Y, B_SCALE, B_RES, B_STAT, B_DYS, B_DW, B_DB, B_WS, B_COUNT };
#include "host_launches.h"

// ---- one argument tuple for every entry point ------------------------------------------------------------------------------------------
struct Args {
    void *x, *w, *bias, *y, *scale, *res, *stat, *dys, *dw, *db, *ws;
    int B, H, W, Cin, Cout, taps, cin_valid, cout_valid, dtype, act;
    long x_ld, y_ld, ws_bytes, M;
};
enum Entry { E_FWD, E_STATS, E_FUSED, E_DGRAD_H, E_ADD, E_ENC_H, E_WGRAD, E_WGRAD_BIAS, E_WGRAD_H, E_WGRAD_H1, E_COUNT };
static const char* const ENTRY_NAMES[E_COUNT] = {"fwd", "fwd_stats", "fused", "dgrad_h", "conv1x1_fwd_add", "conv1x1_fwd_enc_h",
                                                "wgrad", "wgrad_bias", "wgrad_h", "wgrad_h1"};
static bool entry_is_wgrad(int e) { return e >= E_WGRAD; }
static bool entry_has_dtype(int e) { return e == E_FWD || e == E_STATS || e == E_FUSED || e == E_ADD || e == E_WGRAD || e == E_WGRAD_BIAS; }
static long g_calls = 0;

static int call(int e, const Args& a) {
    ++g_calls;
    float *dw = (float*)a.dw, *db = (float*)a.db, *dys = (float*)a.dys;
    switch (e) {
    case E_FWD: return mu_conv_fwd(a.x, a.w, (float*)a.bias, a.y, a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.x_ld, a.y_ld, a.dtype, nullptr);
    case E_STATS:
        return mu_conv_fwd_stats(a.x, a.w, (float*)a.bias, a.y, a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.x_ld, a.y_ld, a.dtype, (float*)a.stat, nullptr);
    case E_FUSED:
        return mu_conv_fwd_fused(a.x, a.w, (float*)a.scale, (float*)a.bias, a.res, a.act, a.y, a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.x_ld, a.y_ld,
                                 a.dtype, nullptr);
    case E_DGRAD_H: return mu_conv_dgrad_h(a.x, a.w, dys, a.y, a.B, a.H, a.W, a.Cin, a.Cout, a.x_ld, a.y_ld, nullptr);
    case E_ADD: return mu_conv1x1_fwd_add(a.x, a.w, a.res, a.y, a.M, a.Cin, a.Cout, a.x_ld, a.y_ld, a.dtype, nullptr);
    case E_ENC_H: return mu_conv1x1_fwd_enc_h(a.x, a.w, (float*)a.bias, a.y, a.M, a.Cin, a.Cout, a.x_ld, a.y_ld, nullptr);
    case E_WGRAD:
        return mu_conv_wgrad(a.x, a.y, dw, a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.cin_valid, a.cout_valid, a.x_ld, a.y_ld, a.ws, a.ws_bytes, a.dtype, nullptr);
    case E_WGRAD_BIAS:
        return mu_conv_wgrad_bias(a.x, a.y, dw, db, a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.cin_valid, a.cout_valid, a.x_ld, a.y_ld, a.ws, a.ws_bytes,
                                  a.dtype, nullptr);
    case E_WGRAD_H:
        return mu_conv_wgrad_h(a.x, a.y, dys, dw, a.B, a.H, a.W, a.Cin, a.Cout, a.cin_valid, a.cout_valid, a.x_ld, a.y_ld, a.ws, a.ws_bytes, nullptr);
    case E_WGRAD_H1:
        return mu_conv_wgrad_h1(a.x, a.y, dys, dw, a.B, a.H, a.W, a.Cin, a.Cout, a.cin_valid, a.cout_valid, a.x_ld, a.y_ld, a.ws, a.ws_bytes, nullptr);
    }
    return 1;
}

// the faults of the refusing tuples: each edits the valid tuple of the entry (a fault the entry does not look at leaves the call valid)
enum Fault {
    F_X_NULL, F_W_NULL, F_OUT_NULL, F_B_ZERO, F_H_NEG, F_W_ZERO, F_M_ZERO, F_M_HUGE, F_CIN_ZERO, F_CIN_ODD, F_COUT_ODD, F_COUT_96,
    F_XLD_SMALL, F_XLD_MISALIGNED, F_YLD_SMALL, F_YLD_MISALIGNED, F_YLD_PLUS4, F_TAPS, F_DTYPE, F_ACT_HIGH, F_ACT_LOW, F_CINV_ZERO, F_CINV_BIG,
    F_CINV_3, F_COUTV_ZERO, F_COUTV_BIG, F_DYS_NULL, F_RES_NULL, F_DB_NULL, F_WS_NULL, F_WS_ZERO, F_WS_SHORT, F_COUNT
};
static void apply(int f, int e, Args& a, long ws_min) {
    switch (f) {
    case F_X_NULL: a.x = nullptr; break;
    case F_W_NULL: a.w = nullptr; break;
    case F_OUT_NULL: (entry_is_wgrad(e) ? a.dw : a.y) = nullptr; break;       // (the weight gradients read a.y as dy)
    case F_B_ZERO: a.B = 0; break;
    case F_H_NEG: a.H = -1; break;
    case F_W_ZERO: a.W = 0; break;
    case F_M_ZERO: a.M = 0; break;
    case F_M_HUGE: a.M = 0x80000000L; break;
    case F_CIN_ZERO: a.Cin = 0; break;
    case F_CIN_ODD: a.Cin += 16; break;
    case F_COUT_ODD: a.Cout += 16; break;
    case F_COUT_96: a.Cout = 96; a.y_ld = 96; break;                          // a multiple of 32 but not of 64 (the 1x1 entries)
    case F_XLD_SMALL: a.x_ld = a.Cin - 8; break;
    case F_XLD_MISALIGNED: a.x_ld += 4; break;
    case F_YLD_SMALL: a.y_ld = a.Cout - 8; break;
    case F_YLD_MISALIGNED: a.y_ld += 2; break;
    case F_YLD_PLUS4: a.y_ld += 4; break;                                     // (fine for the fp32 rows of mu_conv_dgrad_h alone)
    case F_TAPS: a.taps = 3; break;
    case F_DTYPE: a.dtype = 7; break;
    case F_ACT_HIGH: a.act = MU_ACT_RELU + 1; break;
    case F_ACT_LOW: a.act = MU_ACT_NONE - 1; break;
    case F_CINV_ZERO: a.cin_valid = 0; break;
    case F_CINV_BIG: a.cin_valid = a.Cin + 1; break;
    case F_CINV_3: a.cin_valid = 3; break;
    case F_COUTV_ZERO: a.cout_valid = 0; break;
    case F_COUTV_BIG: a.cout_valid = a.Cout + 1; break;
    case F_DYS_NULL: a.dys = nullptr; break;
    case F_RES_NULL: a.res = nullptr; break;
    case F_DB_NULL: a.db = nullptr; break;
    case F_WS_NULL: a.ws = nullptr; break;
    case F_WS_ZERO: a.ws_bytes = 0; break;
    case F_WS_SHORT: a.ws_bytes = ws_min - 1; break;
    }
}

static const char* name_or_dash(int op, int id) {
    const char* n = mu_conv_plan_name(op, id);
    return n ? n : "-";
}
static void run(const char* tag, int e, const Args& a) {
    g_launches.clear();
    const int rc = call(e, a);
    printf("  %s -> %d, %zu launches\n", tag, rc, g_launches.size());
    for (const Launch& l : g_launches) printf("    %s\n", l.text.c_str());
}
// smallest ws_bytes the entry accepts for the tuple (bisection between 0 and its query; -1: it refuses the query's size too)
static long smallest_workspace(int e, Args a) {
    const long hi0 = a.ws_bytes;
    g_record = false;
    long lo = 0, hi = hi0;
    if (call(e, a) != MU_OK) hi = -1;
    while (hi > 0 && lo + 1 < hi) {
        a.ws_bytes = lo + (hi - lo) / 2;
        (call(e, a) == MU_OK ? hi : lo) = a.ws_bytes;
    }
    g_record = true;
    g_launches.clear();
    return hi;
}

int main() {
    static const char* const DT[3] = {"fp32", "fp16", "fp32x"};
    int B, H, W, Cin, Cout, taps, cv;
    long rows = 0;
    while (scanf("%d %d %d %d %d %d %d", &B, &H, &W, &Cin, &Cout, &taps, &cv) == 7) {
        ++rows;
        printf("row %d %d %d %d %d %d %d\n", B, H, W, Cin, Cout, taps, cv);
        Args v = {buf(B_X), buf(B_W), buf(B_BIAS), buf(B_Y), buf(B_SCALE), buf(B_RES), buf(B_STAT), buf(B_DYS), buf(B_DW), buf(B_DB), buf(B_WS),
                  B, H, W, Cin, Cout, taps, cv, Cout > 3 ? Cout - 3 : Cout, MU_F16, MU_ACT_NONE, Cin + 8, Cout + 8, 0, (long)B * H * W};
        const long ws_q = mu_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, taps), ws_h = mu_conv_wgrad_h_workspace_bytes(B, H, W, Cin, Cout);
        printf(" workspace %ld, wgrad_h workspace %ld, dgrad_h plan %d %s / transposed %d %s, wgrad_h plan %d %s\n", ws_q, ws_h,
               mu_conv_dgrad_h_plan(B, H, W, Cin, Cout), name_or_dash(2, mu_conv_dgrad_h_plan(B, H, W, Cin, Cout)),
               mu_conv_dgrad_h_plan(B, H, W, Cout, Cin), name_or_dash(2, mu_conv_dgrad_h_plan(B, H, W, Cout, Cin)),
               mu_conv_wgrad_plan(B, H, W, Cin, Cout, taps, cv, MU_F16, 1), name_or_dash(3, mu_conv_wgrad_plan(B, H, W, Cin, Cout, taps, cv, MU_F16, 1)));
        long ws_min[E_COUNT][3] = {};
        for (int d = 0; d < 3; ++d) {
            Args a = v;
            a.dtype = d;
            a.ws_bytes = ws_q;
            const int pf = mu_conv_fwd_plan(B, H, W, Cin, Cout, taps, d, 0), ps = mu_conv_fwd_plan(B, H, W, Cin, Cout, taps, d, 1);
            const int pu = mu_conv_fwd_fused_plan(B, H, W, Cin, Cout, taps, d), pw = mu_conv_wgrad_plan(B, H, W, Cin, Cout, taps, cv, d, 0);
            const int pb = mu_conv_wgrad_bias_plan(B, H, W, Cin, Cout, taps, cv, d);
            printf(" %s: fwd %d %s, fwd_stats %d %s, fused %d %s, wgrad %d %s, wgrad_bias %d %s, stats_rows %d, add_supported %d, bias_supported %d\n",
                   DT[d], pf, name_or_dash(0, pf), ps, name_or_dash(0, ps), pu, name_or_dash(1, pu), pw, name_or_dash(3, pw), pb, name_or_dash(3, pb),
                   mu_conv_stats_rows(B, H, W, Cin, Cout, taps, d), mu_conv1x1_add_supported(Cin, Cout, d),
                   mu_conv_wgrad_bias_supported(Cin, Cout, taps, d));
            run("fwd", E_FWD, a);
            run("fwd_stats", E_STATS, a);
            Args n = a;
            n.stat = nullptr;
            run("fwd_stats without a buffer", E_STATS, n);
            n = a;                                            // the fp16 data gradient: the transposed layer
            n.Cin = a.Cout; n.Cout = a.Cin; n.x_ld = a.y_ld; n.y_ld = a.x_ld;
            run("dgrad", E_FWD, n);
            for (int act = MU_ACT_NONE; act <= MU_ACT_RELU; ++act) {
                n = a;
                n.act = act;
                char tag[32];
                snprintf(tag, sizeof tag, "fused act %d", act);
                run(tag, E_FUSED, n);
            }
            n = a;
            n.res = n.scale = n.bias = nullptr;
            run("fused plain", E_FUSED, n);
            run("conv1x1_fwd_add", E_ADD, a);
            for (int e : {E_WGRAD, E_WGRAD_BIAS}) {
                run(ENTRY_NAMES[e], e, a);
                ws_min[e][d] = smallest_workspace(e, a);
                printf("  %s smallest workspace %ld\n", ENTRY_NAMES[e], ws_min[e][d]);
            }
        }
        {
            Args a = v;
            a.dtype = MU_F32X;
            run("conv1x1_fwd_enc_h", E_ENC_H, a);
            run("dgrad_h", E_DGRAD_H, a);
            Args n = a;                                       // as the product calls it: dy has the layer's Cout channels
            n.Cin = a.Cout; n.Cout = a.Cin; n.x_ld = a.y_ld; n.y_ld = a.x_ld;
            run("dgrad_h transposed", E_DGRAD_H, n);
            for (int e : {E_WGRAD_H, E_WGRAD_H1}) {
                a.ws_bytes = e == E_WGRAD_H ? ws_h : ws_q;
                run(ENTRY_NAMES[e], e, a);
                ws_min[e][0] = smallest_workspace(e, a);
                printf("  %s smallest workspace %ld\n", ENTRY_NAMES[e], ws_min[e][0]);
            }
        }
        // refusing tuples: one fault, then every pair
        g_record = false;
        for (int e = 0; e < E_COUNT; ++e)
            for (int d = 0; d < (entry_has_dtype(e) ? 3 : 1); ++d) {
                Args a = v;
                if (entry_has_dtype(e)) a.dtype = d;
                a.ws_bytes = e == E_WGRAD_H ? ws_h : ws_q;
                const long wm = ws_min[e][d];
                std::string codes;
                g_launches.clear();
                for (int f = 0; f < F_COUNT; ++f) {
                    Args n = a;
                    apply(f, e, n, wm);
                    codes += letter(call(e, n));
                }
                codes += ' ';
                for (int f = 0; f < F_COUNT; ++f)
                    for (int g = f + 1; g < F_COUNT; ++g) {
                        Args n = a;
                        apply(f, e, n, wm);
                        apply(g, e, n, wm);
                        codes += letter(call(e, n));
                    }
                printf(" faults %s %s: %s, %zu launches\n", ENTRY_NAMES[e], entry_has_dtype(e) ? DT[d] : "-", codes.c_str(), g_launches.size());
            }
        g_record = true;
    }
    printf("%ld rows, %ld calls\n", rows, g_calls);
    return 0;
}
