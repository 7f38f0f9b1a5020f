// The MCPE merging host twin (clsim_amd/csrc/mcpe_merge.cpp) as a stand-alone program, for the sanitizers: no Python, no GPU.
//   mcpe_merge_host_main IN OUT
// IN:  uint64 n, n_series; double window; uint64 reserved; n clsimhip_mcpe; n_series clsimhip_mcpe_series
// OUT: uint64 n_merged, n_parents; the merged records, the merged series table, the parents, the ranges
// Output arrays are allocated at exactly the sizes the interface names, so a write past them is seen.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_model.h"
#include "mcpe_merge.h"

template <class T>
static bool read_array(std::FILE *f, std::vector<T> &v)
{
    return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T>
static bool write_array(std::FILE *f, const T *p, size_t n)
{
    return n == 0 || std::fwrite(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    uint64_t sizes[2], reserved;
    double window;
    if (std::fread(sizes, 8, 2, in) != 2 || std::fread(&window, 8, 1, in) != 1 || std::fread(&reserved, 8, 1, in) != 1) { std::fprintf(stderr, "short header\n"); return 2; }
    std::vector<clsimhip_mcpe> records(sizes[0]);
    std::vector<clsimhip_mcpe_series> series(sizes[1]);
    if (!read_array(in, records) || !read_array(in, series)) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(in);
    // exactly n and n_series entries, on the heap (an empty vector's data() may be null: n = 0 must not need them)
    std::vector<clsimhip_mcpe_merged> merged(records.size());
    std::vector<clsimhip_mcpe_parent> parents(records.size());
    std::vector<clsimhip_mcpe_series> merged_series(series.size());
    std::vector<clsimhip_mcpe_parent_range> ranges(series.size());
    size_t n_merged = 0, n_parents = 0;
    try {
        clsimhip::mcpe_merge_host(records.data(), records.size(), series.data(), series.size(), window, merged.data(), merged_series.data(), parents.data(),
                                  ranges.data(), &n_merged, &n_parents);
    } catch (const clsimhip::Error &e) {
        std::fprintf(stderr, "refused (%d): %s\n", e.code, e.what());
        return 3;
    }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const uint64_t made[2] = {n_merged, n_parents};
    const bool ok = std::fwrite(made, 8, 2, out) == 2 && write_array(out, merged.data(), n_merged) && write_array(out, merged_series.data(), series.size()) &&
                    write_array(out, parents.data(), n_parents) && write_array(out, ranges.data(), series.size());
    std::fclose(out);
    if (!ok) { std::fprintf(stderr, "short write\n"); return 2; }
    std::printf("%zu records in %zu series -> %zu merged records, %zu parents\n", records.size(), series.size(), n_merged, n_parents);
    return 0;
}
