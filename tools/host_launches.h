// The runtime half of the stand-alone launch recorders (tools/conv_host_launches.cpp, tools/attn_host_launches.cpp): the few runtime
// symbols the host code of a HIP object refers to, defined so that nothing is launched -- hipLaunchKernel records the kernel
// instantiation (demangled), grid, block, dynamic LDS, every scalar argument by value and every pointer argument as an offset into the
// buffer it was derived from; hipMemsetAsync records a pseudo-launch of the same form.  No GPU and no HIP runtime are needed.
//
// The including program names its buffers BEFORE the #include:
//   static const char* const BUF_NAMES[] = {nullptr, "x", "w", ...};      // index 0 is unused
// buf(i) is then the address of buffer i: disjoint 1 TiB ranges that are never dereferenced.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <cxxabi.h>
#include <dlfcn.h>
#include "../include/maskunet_hip.h"

struct Dim3 { unsigned x, y, z; };
struct Launch { std::string text; };
static std::vector<Launch> g_launches;
static bool g_record = true;          // false: count the launches only (the refusing tuples)
static Dim3 g_grid, g_block;
static size_t g_lds;
static void* g_stream;

static void* buf(int b) { return (void*)((uintptr_t)b << 40); }

static std::string ptr_text(const void* p) {
    if (!p) return "null";
    const uintptr_t u = (uintptr_t)p, b = u >> 40;
    char s[64];
    if (b >= 1 && b < sizeof(BUF_NAMES) / sizeof(*BUF_NAMES)) snprintf(s, sizeof s, "%s+%llu", BUF_NAMES[b], (unsigned long long)(u - (b << 40)));
    else snprintf(s, sizeof s, "?%p", p);
    return s;
}

// the parameter list of a demangled function signature, split at top-level commas
static std::vector<std::string> params_of(const std::string& sig) {
    std::vector<std::string> out;
    const size_t end = sig.rfind(')');
    if (end == std::string::npos) return out;
    int depth = 0;
    size_t beg = end;
    for (size_t i = end + 1; i-- > 0;) {
        if (sig[i] == ')' || sig[i] == '>') ++depth;
        if (sig[i] == '(' || sig[i] == '<') --depth;
        if (depth == 0) { beg = i; break; }
    }
    std::string cur;
    depth = 0;
    for (size_t i = beg + 1; i < end; ++i) {
        const char ch = sig[i];
        if (ch == '(' || ch == '<') ++depth;
        if (ch == ')' || ch == '>') --depth;
        if (ch == ',' && depth == 0) { out.push_back(cur); cur.clear(); continue; }
        if (ch == ' ' && cur.empty()) continue;
        cur += ch;
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

extern "C" {
int __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t lds, void* stream) {
    g_grid = grid; g_block = block; g_lds = lds; g_stream = stream;
    return 0;
}
int __hipPopCallConfiguration(Dim3* grid, Dim3* block, size_t* lds, void** stream) {
    *grid = g_grid; *block = g_block; *lds = g_lds; *stream = g_stream;
    return 0;
}
int hipLaunchKernel(const void* func, Dim3 grid, Dim3 block, void** args, size_t lds, void* stream) {
    (void)stream;
    if (!g_record) { g_launches.push_back({}); return 0; }
    Dl_info info;
    std::string name = "?";
    if (dladdr(func, &info) && info.dli_sname) {
        // (the C++ runtime's demangler predates DF16_ = _Float16: hand it Dh = half, which is no substitution candidate either)
        std::string m = info.dli_sname;
        for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");
        int st = 0;
        char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
        name = st == 0 && d ? d : info.dli_sname;
        free(d);
        for (size_t i = 0; (i = name.find("half", i)) != std::string::npos; i += 8) name.replace(i, 4, "_Float16");
    }
    char s[160];
    snprintf(s, sizeof s, " grid (%u,%u,%u) block (%u,%u,%u) lds %zu args", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    const std::vector<std::string> ps = params_of(name);
    std::string t = name.substr(0, name.rfind('(')) + s;
    for (size_t i = 0; i < ps.size(); ++i) {
        const std::string& p = ps[i];
        t += ' ';
        if (!p.empty() && p.back() == '*') t += ptr_text(*(void**)args[i]);
        else if (p == "int") t += std::to_string(*(int*)args[i]);
        else if (p == "long") t += std::to_string(*(long*)args[i]) + "L";
        else if (p == "float") { snprintf(s, sizeof s, "%.9gf", *(float*)args[i]); t += s; }
        else if (p == "bool") t += *(bool*)args[i] ? "true" : "false";
        else t += "?" + p;
    }
    g_launches.push_back({t});
    return 0;
}
// a memset on the stream is work enqueued like a launch, and is recorded as one
int hipMemsetAsync(void* dst, int value, size_t bytes, void* stream) {
    (void)stream;
    if (!g_record) { g_launches.push_back({}); return 0; }
    char s[64];
    snprintf(s, sizeof s, " value %d bytes %zu", value, bytes);
    g_launches.push_back({"hipMemsetAsync " + ptr_text(dst) + s});
    return 0;
}
int hipGetLastError() { return 0; }
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}

static char letter(int rc) {
    return rc == MU_OK ? '0' : rc == MU_ERR_ARG ? 'A' : rc == MU_ERR_SHAPE ? 'S' : rc == MU_ERR_LAUNCH ? 'L' : rc == MU_ERR_WORKSPACE ? 'W' : '?';
}
