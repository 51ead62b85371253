// The runtime half of the stand-alone launch recorders (tools/conv_host_launches.cpp, tools/attn_host_launches.cpp,
// tools/post_host_launches.cpp): the few runtime symbols the host code of a HIP object refers to, defined so that nothing is launched --
// hipLaunchKernel records the kernel instantiation (demangled), grid, block, dynamic LDS, every scalar argument by value and every
// pointer argument as an offset into the buffer it was derived from; hipMemsetAsync records a pseudo-launch of the same form;
// hipFuncSetAttribute records a grant (kernel and bytes), which is no launch, and fails for the whole process once g_grant_fails is set.
// No GPU and no HIP runtime are needed.
//
// A by-value struct argument is printed field by field where the including program has set g_struct_layouts: a table from the type's
// name (or "kernel:type", looked up first, where two kernels' types share a name) to its fields in declaration order, as tokens
// p pointer, i int, l long, f float, d double, x one byte of declared padding, each optionally followed by a count ("p7 i5 l4 d").
// Alignment padding is implied.  Any other struct prints as ?Type.
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

struct StructLayout { const char *type, *fields; };
static const StructLayout* g_struct_layouts = nullptr;
static size_t g_struct_layout_count = 0;
static std::vector<std::string> g_grants;          // "kernel bytes" of every hipFuncSetAttribute call, in call order
static bool g_grant_fails = false;

static void* buf(int b) { return (void*)((uintptr_t)b << 40); }

static std::string ptr_text(const void* p) {
    if (!p) return "null";
    const uintptr_t u = (uintptr_t)p, b = u >> 40;
    char s[64];
    if (b >= 1 && b < sizeof(BUF_NAMES) / sizeof(*BUF_NAMES)) snprintf(s, sizeof s, "%s+%llu", BUF_NAMES[b], (unsigned long long)(u - (b << 40)));
    else snprintf(s, sizeof s, "?%p", p);
    return s;
}

// where the parameter list of a demangled function signature opens: the partner of its last ')' (npos: there is none)
static size_t params_open(const std::string& sig) {
    const size_t end = sig.rfind(')');
    if (end == std::string::npos) return end;
    int depth = 0;
    for (size_t i = end + 1; i-- > 0;) {
        if (sig[i] == ')' || sig[i] == '>') ++depth;
        if (sig[i] == '(' || sig[i] == '<') --depth;
        if (depth == 0) return i;
    }
    return end;
}
// the parameter list, split at top-level commas
static std::vector<std::string> params_of(const std::string& sig) {
    std::vector<std::string> out;
    const size_t end = sig.rfind(')'), beg = params_open(sig);
    if (end == std::string::npos) return out;
    std::string cur;
    int depth = 0;
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

// kernels as the objects register them (before main): host handle -> mangled name.  The dynamic symbol table (the fall-back) knows
// the global ones under that name too, but not the kernels of an anonymous namespace, and a sanitizer build renames its entries.
static std::vector<std::pair<const void*, std::string>>& registered_kernels() {
    static std::vector<std::pair<const void*, std::string>> v;
    return v;
}
// the demangled instantiation behind a kernel's host handle
static std::string kernel_text(const void* func) {
    Dl_info info;
    std::string name = "?";
    const char* mangled = nullptr;
    for (const auto& k : registered_kernels())
        if (!mangled && k.first == func) mangled = k.second.c_str();
    if (!mangled && dladdr(func, &info)) mangled = info.dli_sname;
    if (mangled) {
        // (the C++ runtime's demangler predates DF16_ = _Float16: hand it Dh = half, which is no substitution candidate either)
        std::string m = mangled;
        for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");
        int st = 0;
        char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
        name = st == 0 && d ? d : mangled;
        free(d);
        for (size_t i = 0; (i = name.find("half", i)) != std::string::npos; i += 8) name.replace(i, 4, "_Float16");
    }
    return name;
}
// the field tokens of struct `type` as an argument of kernel `sig`, or null
static const char* layout_of(const std::string& sig, const std::string& type) {
    for (size_t i = 0; i < g_struct_layout_count; ++i) {
        const char* colon = strchr(g_struct_layouts[i].type, ':');
        if (colon && type == colon + 1 && sig.find(std::string(g_struct_layouts[i].type, colon) + "(") != std::string::npos)
            return g_struct_layouts[i].fields;
    }
    for (size_t i = 0; i < g_struct_layout_count; ++i)
        if (type == g_struct_layouts[i].type) return g_struct_layouts[i].fields;
    return nullptr;
}
static std::string struct_text(const std::string& type, const char* fields, const char* at) {
    std::string t = type + "{";
    size_t off = 0;
    char s[64];
    for (const char* f = fields; *f;) {
        const char kind = *f++;
        if (kind == ' ') continue;
        long n = 1;
        if (*f >= '0' && *f <= '9') n = strtol(f, (char**)&f, 10);
        const size_t size = kind == 'x' ? 1 : (kind == 'i' || kind == 'f') ? 4 : 8;
        off = (off + size - 1) / size * size;
        for (long k = 0; k < n; ++k, off += size) {
            if (kind == 'x') continue;
            if (t.back() != '{') t += ' ';
            if (kind == 'p') { void* v; memcpy(&v, at + off, 8); t += ptr_text(v); }
            else if (kind == 'i') { int v; memcpy(&v, at + off, 4); t += std::to_string(v); }
            else if (kind == 'l') { long v; memcpy(&v, at + off, 8); t += std::to_string(v) + "L"; }
            else if (kind == 'f') { float v; memcpy(&v, at + off, 4); snprintf(s, sizeof s, "%.9gf", v); t += s; }
            else if (kind == 'd') { double v; memcpy(&v, at + off, 8); snprintf(s, sizeof s, "%.17g", v); t += s; }
        }
    }
    return t + "}";
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
    const std::string name = kernel_text(func);
    char s[160];
    snprintf(s, sizeof s, " grid (%u,%u,%u) block (%u,%u,%u) lds %zu args", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    const std::vector<std::string> ps = params_of(name);
    std::string t = name.substr(0, name.rfind('(')) + s;      // (cut at the LAST '(': a parenthesis inside the parameters shows; kept, the recorded outputs are compared byte for byte)
    for (size_t i = 0; i < ps.size(); ++i) {
        const std::string& p = ps[i];
        t += ' ';
        if (!p.empty() && p.back() == '*') t += ptr_text(*(void**)args[i]);
        else if (p == "int") t += std::to_string(*(int*)args[i]);
        else if (p == "long") t += std::to_string(*(long*)args[i]) + "L";
        else if (p == "float") { snprintf(s, sizeof s, "%.9gf", *(float*)args[i]); t += s; }
        else if (p == "bool") t += *(bool*)args[i] ? "true" : "false";
        else if (const char* fields = layout_of(name, p)) t += struct_text(p, fields, (const char*)args[i]);
        else t += "?" + p;
    }
    g_launches.push_back({t});
    return 0;
}
// the grant of dynamic LDS to a kernel: recorded, never a launch
int hipFuncSetAttribute(const void* func, int attr, int value) {
    (void)attr;
    const std::string name = kernel_text(func);
    g_grants.push_back(name.substr(0, params_open(name)) + " " + std::to_string(value));
    return g_grant_fails ? 1 : 0;
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
void __hipRegisterFunction(void**, const void* host, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    registered_kernels().push_back({host, device_name});
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}

static char letter(int rc) {
    return rc == MU_OK ? '0' : rc == MU_ERR_ARG ? 'A' : rc == MU_ERR_SHAPE ? 'S' : rc == MU_ERR_LAUNCH ? 'L' : rc == MU_ERR_WORKSPACE ? 'W' : '?';
}
