// Stand-alone check of the run-time compiled kernel's source generator and cache key (baked_source.cpp), built with
// -fsanitize=address,undefined (Makefile: baked_source_check) and run by tests/test_baked_kernel.py.  No HIP call, no device.
#include <hip/hip_vector_types.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "baked_kernel.h"
#include "kparams.h"

using namespace clsimhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main()
{
    std::string why;
    CHECK(baked_layout_ok(&why));
    if (!why.empty()) std::fprintf(stderr, "%s\n", why.c_str());

    KParams P;
    std::memset(&P, 0, sizeof P);
    P.num_layers = 171;
    P.layer_thickness = 10.0f;
    P.prox_n = 512;
    P.tilt_dz = -0.0f;
    P.post_renorm = -1;
    for (int i = 0; i < 9; ++i) P.pre[i] = 0.125f * (float)i;
    for (int i = 0; i < kMaxGenerators; ++i) P.off_gen_yv[i] = 0xfffffff0u + (uint32_t)i;
    P.tables = reinterpret_cast<const uint32_t *>(0x1234);       // (a launch member: must not reach the source)
    P.n_steps = 77;
    const BakedVariant v{1, true, false, false, true, false};

    const std::string body = baked_params_struct(P);
    CHECK(body.find("static constexpr int32_t num_layers = (int32_t)0x000000abu;") != std::string::npos);
    CHECK(body.find("static constexpr float layer_thickness = __builtin_bit_cast(float, 0x41200000u);") != std::string::npos);
    CHECK(body.find("static constexpr float tilt_dz = __builtin_bit_cast(float, 0x80000000u);") != std::string::npos);
    CHECK(body.find("static constexpr int32_t post_renorm = (int32_t)0xffffffffu;") != std::string::npos);
    CHECK(body.find("static constexpr float pre[9] = {__builtin_bit_cast(float, 0x00000000u), __builtin_bit_cast(float, 0x3e000000u)") != std::string::npos);
    CHECK(body.find("0xfffffff7u}") != std::string::npos);
    CHECK(body.find("const uint32_t * tables;") != std::string::npos);
    CHECK(body.find("uint32_t n_steps;") != std::string::npos);
    CHECK(body.find("static constexpr uint32_t n_steps") == std::string::npos);
    CHECK(body.find("1234") == std::string::npos);
    // every line but the last continues the macro it is the body of
    for (size_t at = 0, end; (end = body.find('\n', at)) != std::string::npos; at = end + 1)
        CHECK(end + 1 == body.size() || (end > 0 && body[end - 1] == '\\'));

    const std::string source = baked_source(P, v);
    CHECK(!source.empty());
    CHECK(source.find("static_assert(sizeof(KParams) == " + std::to_string(sizeof(KParams))) != std::string::npos);
    CHECK(source.find("static_assert(__builtin_offsetof(KParams, k_packed) == " + std::to_string(offsetof(KParams, k_packed))) != std::string::npos);
    CHECK(source.find("template __global__ void prop_pool_kernel<1, true, false, false, true, false>(const KParams);") != std::string::npos);
    CHECK(source.find("__launch_bounds__(kPoolBlock, kPoolMinWaves) prop_pool_kernel") != std::string::npos);     // the embedded headers
    CHECK(source.find("#include") == std::string::npos);                                                          // ... preprocessed
    CHECK(baked_kernel_name(v) == "_ZN8clsimhip16prop_pool_kernelILi1ELb1ELb0ELb0ELb1ELb0EEEvNS_7KParamsE");

    // keys: launch members do not count, one configuration word does, so do the variant, the flags, the architecture, the compiler
    const std::string flags = baked_default_flags();
    CHECK(flags.find("-ffp-contract=off") != std::string::npos && flags.find("-amdgpu-sdwa-peephole=0") != std::string::npos);
    const std::string key = baked_cache_key(source, flags, "gfx950", "7.2");
    CHECK(key.size() == 32);
    KParams Q = P;
    Q.tables = nullptr;
    Q.n_steps = 78;
    Q.k_packed = 5;
    CHECK(baked_cache_key(baked_source(Q, v), flags, "gfx950", "7.2") == key);
    CHECK(baked_config_bytes(Q, v) == baked_config_bytes(P, v));
    Q.hg_g = 0.5f;
    CHECK(baked_cache_key(baked_source(Q, v), flags, "gfx950", "7.2") != key);
    CHECK(baked_config_bytes(Q, v) != baked_config_bytes(P, v));
    BakedVariant w = v;
    w.keep = true;
    CHECK(baked_cache_key(baked_source(P, w), flags, "gfx950", "7.2") != key);
    CHECK(baked_config_bytes(P, w) != baked_config_bytes(P, v));
    CHECK(baked_cache_key(source, flags + " -DX", "gfx950", "7.2") != key);
    CHECK(baked_cache_key(source, flags, "gfx942", "7.2") != key);
    CHECK(baked_cache_key(source, flags, "gfx950", "7.3") != key);
    CHECK(baked_cache_key(source + "gfx", flags, "950", "7.2") != baked_cache_key(source, flags, "gfx950", "7.2"));     // parts do not run into each other

    if (failures) return 1;
    std::printf("baked source check ok: %zu bytes of source, key %s\n", source.size(), key.c_str());
    return 0;
}
