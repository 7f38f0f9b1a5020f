// The pooled propagation kernel compiled at run time for ONE configuration, with the configuration's constants as literals.
//
// About 170 wave-uniform words of KParams are fixed from Compile() until the next Compile(); the precompiled kernels read them from
// the kernarg segment in every loop trip and use them as scalar-register operands.  The reference generates its kernel source per
// configuration with these values as literals (MediumPropertiesSource.cxx, GeometrySource.cxx); this does the same through hiprtc:
//   * baked_source.cpp (no HIP, no device): the generated KParams -- configuration members as `static constexpr`, launch members as
//     fields at their kernarg offsets (kparams_members.inc says which is which) -- in front of the embedded device headers, and the
//     cache key;
//   * baked_kernel.cpp: hiprtc through dlopen (which one: clsimhip_baked_set_compiler_library -- the library reads no environment), the in-process cache of loaded modules, the checks on the loaded function.
// Every failure -- no library, a compile error, a layout mismatch, too many registers, scratch, a load error -- leaves the caller
// with the precompiled kernel: nothing here throws.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace clsimhip {

struct KParams;

// the instantiation of prop_pool_kernel (prop_pool_kernel.hip.h) that is compiled
struct BakedVariant { int lengths; bool tilt, aniso, flasher, fast, keep; };

// "baked_state" of clsimhip_get_tuning
enum { kBakedUnused = 0, kBakedActive = 1, kBakedFallback = 2 };

// What a pooled launch is asked and answers (KVariant::baked)
struct BakedReport {
    int wanted = 0;                 // in: 0 no; 1 take the run-time compiled kernel where it was measured to pay (prop_pool_kernel.hip.h:
                                    // kBakedPays); 2 wherever it can be had
    int state = kBakedUnused;       // out: kBakedActive or kBakedFallback when it was wanted
    std::string key, why;           // out: the module's cache key; the reason of a fallback
};

// ---- baked_source.cpp ----
// false: kparams_members.inc does not describe KParams (a member missing or out of order); `why` says which
bool baked_layout_ok(std::string *why);
// `struct KParams { ... };` of the generated translation unit, as the body of the macro kparams.h expands in its place
std::string baked_params_struct(const KParams &P);
// the whole translation unit; empty when the layout check fails
std::string baked_source(const KParams &P, const BakedVariant &v);
// the lowered name of the instantiation in the code object
std::string baked_kernel_name(const BakedVariant &v);
// the options the library was built with (Makefile: BAKED_FLAGS), one string
const char *baked_default_flags();
// 32 hexadecimal digits over source (which holds the baked values), flags, architecture and compiler version
std::string baked_cache_key(const std::string &source, const std::string &flags, const std::string &arch, const std::string &compiler_version);
// the configuration members' bytes and the variant: what a launch looks its module up by (compared whole: no hash to collide)
std::string baked_config_bytes(const KParams &P, const BakedVariant &v);

// ---- baked_kernel.cpp ----
struct BakedResult {
    bool ok = false;
    std::string why;                // the reason of a fallback
    std::string key;                // cache key
    std::string compiler_version;
    double seconds = 0.0;           // of hiprtcCompileProgram
    std::vector<char> code;         // the code object
};
// clsimhip_baked_set_compiler_library: the hiprtc to dlopen (empty: the usual names); counts until the first compilation of the process
void baked_set_compiler_library(const std::string &path);
// compiles without a device (the CPU tests read the code object); flags = nullptr: baked_default_flags()
BakedResult baked_compile(const KParams &P, const BakedVariant &v, const char *arch, const char *flags);
// the loaded function (a hipFunction_t) for the current device, compiled on first use; nullptr = run the precompiled kernel
// (*why then holds the reason; it is reported on stderr once per process and key).  key_out: the cache key of the module.
void *baked_pool_function(const KParams &P, const BakedVariant &v, std::string *why, std::string *key_out);
// a launch through the function failed: forget it, so that later launches take the precompiled kernel at once
void baked_disable(const KParams &P, const BakedVariant &v, const std::string &why);

} // namespace clsimhip
