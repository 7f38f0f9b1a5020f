// Host program of tests/test_launch_dispatch.py: calls prop_launch.h's dispatch_variant with a functor that records the tags it is
// given, and check_lengths, and prints one line per call for the test to judge.  No device code, no HIP call: the header's API types only.
#include <cstdio>

#include "prop_launch.h"

using namespace clsimhip;

struct Seen { int calls = 0, lengths = -1, tilt = -1, aniso = -1, flasher = -1, fast = -1; };

template <bool ALWAYS_FLASHER>
static void one(const char *form, int lengths, bool tilt, bool aniso, bool flasher, bool fast)
{
    KVariant v{};
    v.lengths = lengths; v.tilt = tilt; v.aniso = aniso; v.flasher = flasher;
    Seen s;
    const hipError_t rc = dispatch_variant<ALWAYS_FLASHER>(v, fast, [&](auto l, auto t, auto a, auto f, auto q) {
        // (the tags must be usable as template arguments: constant expressions of the tag TYPES)
        constexpr int cl = decltype(l)::value;
        constexpr bool ct = decltype(t)::value, ca = decltype(a)::value, cf = decltype(f)::value, cq = decltype(q)::value;
        static_assert(!ALWAYS_FLASHER || cf, "the table maker's form instantiates flasher = true only");
        s.calls += 1; s.lengths = cl; s.tilt = ct; s.aniso = ca; s.flasher = cf; s.fast = cq;
        return hipSuccess;
    });
    std::printf("%s in %d %d %d %d %d rc %d calls %d tags %d %d %d %d %d\n", form, lengths, (int)tilt, (int)aniso, (int)flasher, (int)fast,
                (int)rc, s.calls, s.lengths, s.tilt, s.aniso, s.flasher, s.fast);
}

int main()
{
    std::printf("codes %d %d lengths %d %d %d\n", (int)hipSuccess, (int)hipErrorInvalidValue, CLSIMHIP_LENGTHS_CONSTANT, CLSIMHIP_LENGTHS_ICECUBE,
                CLSIMHIP_LENGTHS_TABLE);
    for (int lengths = CLSIMHIP_LENGTHS_CONSTANT - 1; lengths <= CLSIMHIP_LENGTHS_TABLE + 1; ++lengths)
        for (int bits = 0; bits < 16; ++bits) {
            one<false>("variant", lengths, bits & 8, bits & 4, bits & 2, bits & 1);
            // the table maker: v.flasher is whatever the converter's medium says and must not matter
            one<true>("tab", lengths, bits & 8, bits & 4, bits & 2, bits & 1);
        }
    {
        static const float table[8] = {0};
        KParams P{};
        KVariant v{};
        v.lengths = CLSIMHIP_LENGTHS_TABLE;
        P.len_table = nullptr; P.len_tab_n = 2;
        std::printf("check_lengths null_table %d\n", (int)check_lengths(P, v));
        P.len_table = table; P.len_tab_n = 1;
        std::printf("check_lengths one_bin %d\n", (int)check_lengths(P, v));
        P.len_tab_n = 2;
        std::printf("check_lengths table_ok %d\n", (int)check_lengths(P, v));
        v.lengths = CLSIMHIP_LENGTHS_ICECUBE; P.len_table = nullptr; P.len_tab_n = 0;
        std::printf("check_lengths no_table_needed %d\n", (int)check_lengths(P, v));
        v.lengths = CLSIMHIP_LENGTHS_CONSTANT - 1;
        std::printf("check_lengths below %d\n", (int)check_lengths(P, v));
        v.lengths = CLSIMHIP_LENGTHS_TABLE + 1;
        std::printf("check_lengths above %d\n", (int)check_lengths(P, v));
    }
    return 0;
}
