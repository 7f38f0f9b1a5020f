// Source generator and cache key of the run-time compiled pooled kernel: see baked_kernel.h.  Host C++ only -- no HIP call, no device.
#include "baked_kernel.h"

#include <hip/hip_vector_types.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "kparams.h"

// the device headers, preprocessed into one text at build time (Makefile: baked_headers.inc, not committed): nothing is read from
// disk at run time
static const unsigned char kBakedHeaders[] = {
#include "baked_headers.inc"
    0};

#ifndef CLSIMHIP_BAKED_FLAGS
#error "the Makefile passes the run-time compiler's options as CLSIMHIP_BAKED_FLAGS"
#endif

namespace clsimhip {

namespace {

struct Member {
    const char *type, *name;
    size_t offset, size, count;     // count 0: a scalar
    bool launch;
    char kind;                      // configuration members: 'f' float, 'i' int32_t, 'u' uint32_t
};
template <typename T> constexpr char kind_of();
template <> constexpr char kind_of<float>() { return 'f'; }
template <> constexpr char kind_of<int32_t>() { return 'i'; }
template <> constexpr char kind_of<uint32_t>() { return 'u'; }

#define KP_L(T, N) {#T, #N, offsetof(KParams, N), sizeof(KParams::N), 0, true, 0},
#define KP_LA(T, N, C) {#T, #N, offsetof(KParams, N), sizeof(KParams::N), (size_t)(C), true, 0},
#define KP_C(T, N) {#T, #N, offsetof(KParams, N), sizeof(KParams::N), 0, false, kind_of<T>()},
#define KP_CA(T, N, C) {#T, #N, offsetof(KParams, N), sizeof(KParams::N), (size_t)(C), false, kind_of<T>()},
const Member kMembers[] = {
#include "kparams_members.inc"
};
#undef KP_L
#undef KP_LA
#undef KP_C
#undef KP_CA
constexpr size_t kNumMembers = sizeof(kMembers) / sizeof(kMembers[0]);

void append(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void append(std::string &s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n > 0) s.append(buf, (size_t)n < sizeof buf ? (size_t)n : sizeof buf - 1);
}

// one configuration word as an expression of its type: bit patterns, never decimal text
void append_value(std::string &s, char kind, uint32_t word)
{
    if (kind == 'f') append(s, "__builtin_bit_cast(float, 0x%08xu)", word);
    else if (kind == 'i') append(s, "(int32_t)0x%08xu", word);
    else append(s, "0x%08xu", word);
}

uint64_t fnv1a(uint64_t h, const void *data, size_t n)
{
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

} // namespace

// The list must name every member in order: each member starts exactly where natural alignment puts it behind the one before, and the
// last one ends within the struct's tail padding.  A member added to KParams and not to the list moves the next one off its place -- or
// hides in alignment padding, and is then missing from the generated struct: a kernel that reads it does not compile.  Either way the
// precompiled kernel runs.
bool baked_layout_ok(std::string *why)
{
    size_t cursor = 0;
    for (size_t i = 0; i < kNumMembers; ++i) {
        const Member &m = kMembers[i];
        const size_t align = (m.count ? m.size / m.count : m.size) < 8 ? 4 : 8;
        const size_t expected = (cursor + align - 1) / align * align;
        if (m.offset != expected) {
            if (why) *why = std::string("kparams_members.inc: ") + m.name + " is not where the list puts it";
            return false;
        }
        if (!m.launch && (m.count ? m.size / m.count : m.size) != 4) {
            if (why) *why = std::string("kparams_members.inc: configuration member ") + m.name + " is not a 32-bit word";
            return false;
        }
        cursor = m.offset + m.size;
    }
    if ((cursor + 7) / 8 * 8 != sizeof(KParams)) {
        if (why) *why = "kparams_members.inc does not reach the end of KParams";
        return false;
    }
    return true;
}

std::string baked_params_struct(const KParams &P)
{
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(&P);
    std::string s = "struct KParams { \\\n";
    size_t cursor = 0;
    int pads = 0;
    for (size_t i = 0; i < kNumMembers; ++i) {
        const Member &m = kMembers[i];
        if (m.launch) {
            if (m.offset > cursor) append(s, "    char baked_pad_%d[%zu]; \\\n", pads++, m.offset - cursor);
            if (m.count) append(s, "    %s %s[%zu]; \\\n", m.type, m.name, m.count);
            else append(s, "    %s %s; \\\n", m.type, m.name);
            cursor = m.offset + m.size;
            continue;
        }
        uint32_t w;
        if (!m.count) {
            std::memcpy(&w, bytes + m.offset, 4);
            append(s, "    static constexpr %s %s = ", m.type, m.name);
            append_value(s, m.kind, w);
            s += "; \\\n";
        } else {
            append(s, "    static constexpr %s %s[%zu] = {", m.type, m.name, m.count);
            for (size_t k = 0; k < m.count; ++k) {
                std::memcpy(&w, bytes + m.offset + 4 * k, 4);
                if (k) s += ", ";
                append_value(s, m.kind, w);
            }
            s += "}; \\\n";
        }
    }
    if (sizeof(KParams) > cursor) append(s, "    char baked_pad_%d[%zu]; \\\n", pads++, sizeof(KParams) - cursor);
    s += "};\n";
    return s;
}

std::string baked_kernel_name(const BakedVariant &v)
{
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN8clsimhip16prop_pool_kernelILi%dELb%dELb%dELb%dELb%dELb%dEEEvNS_7KParamsE", v.lengths, (int)v.tilt, (int)v.aniso,
             (int)v.flasher, (int)v.fast, (int)v.keep);
    return buf;
}

std::string baked_source(const KParams &P, const BakedVariant &v)
{
    if (!baked_layout_ok(nullptr)) return std::string();
    std::string s = "// generated: the pooled propagation kernel of one configuration (baked_source.cpp)\n";
    // (the run-time compiler has no <stdint.h>; the types are those of the host's, so that every overload resolves as it does there)
    s += "typedef signed char int8_t;\ntypedef unsigned char uint8_t;\ntypedef short int16_t;\ntypedef unsigned short uint16_t;\n"
         "typedef int int32_t;\ntypedef unsigned int uint32_t;\ntypedef long int64_t;\ntypedef unsigned long uint64_t;\ntypedef unsigned long uintptr_t;\n";
    s += "#define KPARAMS_BAKED_STRUCT \\\n";
    s += baked_params_struct(P);
    s += reinterpret_cast<const char *>(kBakedHeaders);
    // a layout that differs from the host's must be a compile error, never a launch
    s += "\nnamespace clsimhip {\n";
    append(s, "static_assert(sizeof(KParams) == %zu, \"baked KParams: size\");\n", sizeof(KParams));
    for (size_t i = 0; i < kNumMembers; ++i) {
        const Member &m = kMembers[i];
        if (m.launch) append(s, "static_assert(__builtin_offsetof(KParams, %s) == %zu, \"baked KParams: %s\");\n", m.name, m.offset, m.name);
    }
    append(s, "template __global__ void prop_pool_kernel<%d, %s, %s, %s, %s, %s>(const KParams);\n", v.lengths, v.tilt ? "true" : "false",
           v.aniso ? "true" : "false", v.flasher ? "true" : "false", v.fast ? "true" : "false", v.keep ? "true" : "false");
    s += "} // namespace clsimhip\n";
    return s;
}

const char *baked_default_flags() { return CLSIMHIP_BAKED_FLAGS; }

std::string baked_cache_key(const std::string &source, const std::string &flags, const std::string &arch, const std::string &compiler_version)
{
    // two FNV-1a streams with different offsets, each part followed by its length so that parts cannot run into each other
    uint64_t h[2] = {0xcbf29ce484222325ull, 0x84222325cbf29ce4ull};
    const std::string *parts[] = {&source, &flags, &arch, &compiler_version};
    for (const std::string *p : parts) {
        const uint64_t n = p->size();
        for (uint64_t &x : h) {
            x = fnv1a(x, p->data(), p->size());
            x = fnv1a(x, &n, sizeof n);
        }
        h[1] = h[1] * 0x9e3779b97f4a7c15ull + 1u;
    }
    char buf[40];
    snprintf(buf, sizeof buf, "%016llx%016llx", (unsigned long long)h[0], (unsigned long long)h[1]);
    return buf;
}

std::string baked_config_bytes(const KParams &P, const BakedVariant &v)
{
    const char *bytes = reinterpret_cast<const char *>(&P);
    std::string s;
    for (size_t i = 0; i < kNumMembers; ++i)
        if (!kMembers[i].launch) s.append(bytes + kMembers[i].offset, kMembers[i].size);
    const char tag[6] = {(char)v.lengths, (char)v.tilt, (char)v.aniso, (char)v.flasher, (char)v.fast, (char)v.keep};
    s.append(tag, sizeof tag);
    return s;
}

} // namespace clsimhip
