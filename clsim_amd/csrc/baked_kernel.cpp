// Run-time compilation of the pooled kernel: see baked_kernel.h.  hiprtc is loaded at run time (dlopen), as comm.cpp loads RCCL: a
// host without it, or with one that cannot compile the kernel, runs the precompiled kernels.
#include "baked_kernel.h"

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <hip/hiprtc.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <sstream>
#include <utility>

#include "kparams.h"

namespace clsimhip {

namespace {

struct Hiprtc {
    void *handle = nullptr;
    std::string error;              // why it cannot be used
    decltype(&hiprtcVersion) Version = nullptr;
    decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
    decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
    decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
    decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
    decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
    decltype(&hiprtcGetCode) GetCode = nullptr;
    decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
};

std::mutex g_library_mutex;
std::string g_library;              // baked_set_compiler_library: the library to take, and then no other is tried

// (the library reads no environment variable for this: the Python binding hands the caller's choice in through the C ABI)
const Hiprtc &hiprtc()
{
    static Hiprtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<std::string> names;
        {
            std::lock_guard<std::mutex> lk(g_library_mutex);
            if (!g_library.empty()) names.push_back(g_library);
        }
        if (names.empty()) names = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
        for (const std::string &n : names) {
            r.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (r.handle) break;
        }
        if (!r.handle) {
            const char *e = dlerror();
            r.error = std::string("cannot load hiprtc: ") + (e ? e : names.front().c_str());
            return;
        }
        auto sym = [&](const char *name) {
            void *p = dlsym(r.handle, name);
            if (!p && r.error.empty()) r.error = std::string("hiprtc symbol missing: ") + name;
            return p;
        };
        r.Version = reinterpret_cast<decltype(r.Version)>(sym("hiprtcVersion"));
        r.CreateProgram = reinterpret_cast<decltype(r.CreateProgram)>(sym("hiprtcCreateProgram"));
        r.CompileProgram = reinterpret_cast<decltype(r.CompileProgram)>(sym("hiprtcCompileProgram"));
        r.DestroyProgram = reinterpret_cast<decltype(r.DestroyProgram)>(sym("hiprtcDestroyProgram"));
        r.GetProgramLog = reinterpret_cast<decltype(r.GetProgramLog)>(sym("hiprtcGetProgramLog"));
        r.GetProgramLogSize = reinterpret_cast<decltype(r.GetProgramLogSize)>(sym("hiprtcGetProgramLogSize"));
        r.GetCode = reinterpret_cast<decltype(r.GetCode)>(sym("hiprtcGetCode"));
        r.GetCodeSize = reinterpret_cast<decltype(r.GetCodeSize)>(sym("hiprtcGetCodeSize"));
    });
    return r;
}

struct Module {
    hipModule_t module = nullptr;
    hipFunction_t function = nullptr;      // nullptr: this configuration runs the precompiled kernel
    std::string key, why;
};
std::mutex g_mutex;
// (device, configuration bytes + variant) -> loaded module; modules live as long as the process, like the library's own code objects
std::map<std::pair<int, std::string>, Module> g_modules;
// cache key -> code object: a second device, or a second converter whose launch members differ, compiles nothing
std::map<std::string, std::vector<char>> g_code;

void say_once(const std::string &key, const std::string &why)
{
    std::fprintf(stderr, "clsimhip: the pooled kernel of configuration %s runs precompiled (%s)\n", key.empty() ? "(no key)" : key.c_str(), why.c_str());
}

} // namespace

void baked_set_compiler_library(const std::string &path)
{
    std::lock_guard<std::mutex> lk(g_library_mutex);
    g_library = path;
}

BakedResult baked_compile(const KParams &P, const BakedVariant &v, const char *arch, const char *flags)
{
    BakedResult r;
    const Hiprtc &rtc = hiprtc();
    if (!rtc.error.empty()) { r.why = rtc.error; return r; }
    std::string layout;
    if (!baked_layout_ok(&layout)) { r.why = layout; return r; }
    int major = 0, minor = 0;
    if (rtc.Version(&major, &minor) != HIPRTC_SUCCESS) { r.why = "hiprtcVersion failed"; return r; }
    r.compiler_version = std::to_string(major) + "." + std::to_string(minor);
    const std::string source = baked_source(P, v);
    const std::string all_flags = flags ? flags : baked_default_flags();
    r.key = baked_cache_key(source, all_flags, arch, r.compiler_version);
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        const auto it = g_code.find(r.key);
        if (it != g_code.end()) { r.code = it->second; r.ok = true; return r; }
    }
    std::vector<std::string> words;
    {
        std::istringstream in(all_flags);
        for (std::string w; in >> w;) words.push_back(w);
        words.push_back(std::string("--offload-arch=") + arch);
    }
    std::vector<const char *> options;
    for (const std::string &w : words) options.push_back(w.c_str());
    hiprtcProgram prog = nullptr;
    if (rtc.CreateProgram(&prog, source.c_str(), "prop_pool_kernel_baked.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) { r.why = "hiprtcCreateProgram failed"; return r; }
    const auto t0 = std::chrono::steady_clock::now();
    const hiprtcResult compiled = rtc.CompileProgram(prog, (int)options.size(), options.data());
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (compiled != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (rtc.GetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            if (rtc.GetProgramLog(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
        }
        r.why = "compile error: " + log.substr(0, 2000);
    } else {
        size_t n = 0;
        if (rtc.GetCodeSize(prog, &n) == HIPRTC_SUCCESS && n != 0) {
            r.code.resize(n);
            if (rtc.GetCode(prog, r.code.data()) == HIPRTC_SUCCESS) r.ok = true;
        }
        if (!r.ok) { r.code.clear(); r.why = "hiprtcGetCode failed"; }
    }
    rtc.DestroyProgram(&prog);
    if (r.ok) {
        std::lock_guard<std::mutex> lk(g_mutex);
        g_code[r.key] = r.code;
    }
    return r;
}

void *baked_pool_function(const KParams &P, const BakedVariant &v, std::string *why, std::string *key_out)
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); if (why) *why = "no current device"; return nullptr; }
    const std::pair<int, std::string> id(device, baked_config_bytes(P, v));
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        const auto it = g_modules.find(id);
        if (it != g_modules.end()) {
            if (why) *why = it->second.why;
            if (key_out) *key_out = it->second.key;
            return it->second.function;
        }
    }
    // (compiled outside the lock: seconds.  Two threads that meet the same new configuration both compile; the first module stays.)
    Module m;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); m.why = "no device properties"; }
    else {
        std::string arch = prop.gcnArchName;
        arch = arch.substr(0, arch.find(':'));           // (gfx950:sramecc+:xnack- -> gfx950: the library's own code objects are built for the plain name)
        BakedResult r = baked_compile(P, v, arch.c_str(), nullptr);
        m.key = r.key;
        if (!r.ok) m.why = r.why;
        else if (const hipError_t e = hipModuleLoadData(&m.module, r.code.data())) { (void)hipGetLastError(); m.module = nullptr; m.why = std::string("module load: ") + hipGetErrorString(e); }
        else {
            hipFunction_t f = nullptr;
            int regs = 0, scratch = 0;
            if (const hipError_t e2 = hipModuleGetFunction(&f, m.module, baked_kernel_name(v).c_str())) { (void)hipGetLastError(); m.why = std::string("kernel not in the module: ") + hipGetErrorString(e2); }
            else if (hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, f) != hipSuccess || hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f) != hipSuccess) {
                (void)hipGetLastError();
                m.why = "function attributes unavailable";
            } else if (regs > 80 || scratch != 0) m.why = "the compiled kernel takes " + std::to_string(regs) + " vector registers and " + std::to_string(scratch) + " bytes of scratch (at most 80 and none)";
            else m.function = f;
            if (!m.function) { (void)hipModuleUnload(m.module); m.module = nullptr; }
        }
    }
    std::lock_guard<std::mutex> lk(g_mutex);
    const auto placed = g_modules.emplace(id, m);
    if (!placed.second && m.module) (void)hipModuleUnload(m.module);
    else if (!m.function) say_once(m.key, m.why);
    if (why) *why = placed.first->second.why;
    if (key_out) *key_out = placed.first->second.key;
    return placed.first->second.function;
}

void baked_disable(const KParams &P, const BakedVariant &v, const std::string &why)
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lk(g_mutex);
    Module &m = g_modules[std::make_pair(device, baked_config_bytes(P, v))];
    if (m.function || m.why.empty()) say_once(m.key, why);
    m.function = nullptr;           // (the module stays loaded: a launch in flight on another stream may still run it)
    m.why = why;
}

} // namespace clsimhip
