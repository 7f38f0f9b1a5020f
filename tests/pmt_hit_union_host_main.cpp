// The PMT hit frame store's host twins and host store (clsim_amd/csrc/pmt_hit_union.cpp) as a stand-alone program, for the sanitizers: no
// Python, no GPU.
//   pmt_hit_union_host_main IN OUT
// IN is a sequence of commands, each a uint64 code and its arguments (sizes are uint64, a series form is n, n_series, n clsimhip_pmt_hit,
// n_series clsimhip_pmt_series):
//   1 union:  capacity, A, B                         -> status, the union
//   2 split:  last_frame, head_capacity, tail_capacity, X -> status, the head, the tail
//   3 store:  capacity                               -> status          (replaces the program's one store)
//   4 add:    X                                      -> status
//   5 drain:  last_frame, capacity                   -> status, the head
//   6 size:   last_frame                             -> status, n, n_series
// OUT: per command a uint64 status (0, or the error code of a refusal as a positive number) and, with status 0, its results as series
// forms.  Output arrays are allocated at exactly the sizes the interface names, so a write past them is seen.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "host_model.h"
#include "pmt_hit_union.h"

namespace {
struct Form { std::vector<clsimhip_pmt_hit> records; std::vector<clsimhip_pmt_series> series; };

bool read_u64(std::FILE *f, uint64_t &v) { return std::fread(&v, 8, 1, f) == 1; }
bool read_form(std::FILE *f, Form &x)
{
    uint64_t n, n_series;
    if (!read_u64(f, n) || !read_u64(f, n_series)) return false;
    x.records.resize(n);
    x.series.resize(n_series);
    return (n == 0 || std::fread(x.records.data(), sizeof(clsimhip_pmt_hit), n, f) == n) &&
           (n_series == 0 || std::fread(x.series.data(), sizeof(clsimhip_pmt_series), n_series, f) == n_series);
}
void write_u64(std::FILE *f, uint64_t v) { std::fwrite(&v, 8, 1, f); }
void write_form(std::FILE *f, const Form &x, size_t n, size_t n_series)
{
    write_u64(f, n);
    write_u64(f, n_series);
    if (n) std::fwrite(x.records.data(), sizeof(clsimhip_pmt_hit), n, f);
    if (n_series) std::fwrite(x.series.data(), sizeof(clsimhip_pmt_series), n_series, f);
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    std::unique_ptr<clsimhip::PmtHitStore> store;
    uint64_t code, commands = 0, refused = 0;
    while (read_u64(in, code)) {
        ++commands;
        try {
            if (code == 1u) {
                uint64_t capacity;
                Form a, b;
                if (!read_u64(in, capacity) || !read_form(in, a) || !read_form(in, b)) { std::fprintf(stderr, "short input\n"); return 2; }
                Form u;
                u.records.resize(capacity);
                u.series.resize(capacity);
                size_t n = 0, n_series = 0;
                clsimhip::pmt_hits_union_host(a.records.data(), a.records.size(), a.series.data(), a.series.size(), b.records.data(), b.records.size(), b.series.data(),
                                                 b.series.size(), u.records.data(), u.series.data(), capacity, &n, &n_series);
                write_u64(out, 0);
                write_form(out, u, n, n_series);
            } else if (code == 2u) {
                uint64_t last_frame, head_capacity, tail_capacity;
                Form x;
                if (!read_u64(in, last_frame) || !read_u64(in, head_capacity) || !read_u64(in, tail_capacity) || !read_form(in, x)) { std::fprintf(stderr, "short input\n"); return 2; }
                Form head, tail;
                head.records.resize(head_capacity); head.series.resize(head_capacity);
                tail.records.resize(tail_capacity); tail.series.resize(tail_capacity);
                size_t sizes[4] = {0, 0, 0, 0};
                clsimhip::pmt_hits_split_host(x.records.data(), x.records.size(), x.series.data(), x.series.size(), static_cast<uint32_t>(last_frame), head.records.data(),
                                                 head.series.data(), head_capacity, &sizes[0], &sizes[1], tail.records.data(), tail.series.data(), tail_capacity, &sizes[2],
                                                 &sizes[3]);
                write_u64(out, 0);
                write_form(out, head, sizes[0], sizes[1]);
                write_form(out, tail, sizes[2], sizes[3]);
            } else if (code == 3u) {
                uint64_t capacity;
                if (!read_u64(in, capacity)) { std::fprintf(stderr, "short input\n"); return 2; }
                store = clsimhip::make_host_pmt_hit_store(capacity);
                write_u64(out, 0);
            } else if (code == 4u) {
                Form x;
                if (!read_form(in, x) || !store) { std::fprintf(stderr, "short input or no store\n"); return 2; }
                store->add_host(x.records.data(), x.records.size(), x.series.data(), x.series.size());
                write_u64(out, 0);
            } else if (code == 5u) {
                uint64_t last_frame, capacity;
                if (!read_u64(in, last_frame) || !read_u64(in, capacity) || !store) { std::fprintf(stderr, "short input or no store\n"); return 2; }
                Form head;
                head.records.resize(capacity); head.series.resize(capacity);
                size_t n = 0, n_series = 0;
                store->drain_host(static_cast<uint32_t>(last_frame), head.records.data(), head.series.data(), capacity, &n, &n_series);
                write_u64(out, 0);
                write_form(out, head, n, n_series);
            } else if (code == 6u) {
                uint64_t last_frame;
                if (!read_u64(in, last_frame) || !store) { std::fprintf(stderr, "short input or no store\n"); return 2; }
                size_t n = 0, n_series = 0;
                store->size(static_cast<uint32_t>(last_frame), &n, &n_series);
                write_u64(out, 0);
                write_u64(out, n);
                write_u64(out, n_series);
            } else {
                std::fprintf(stderr, "unknown command %llu\n", static_cast<unsigned long long>(code));
                return 2;
            }
        } catch (const clsimhip::Error &e) {
            ++refused;
            std::fprintf(stderr, "refused (%d): %s\n", e.code, e.what());
            write_u64(out, static_cast<uint64_t>(-e.code));
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) { std::fprintf(stderr, "short write\n"); return 2; }
    std::printf("%llu commands, %llu refused\n", static_cast<unsigned long long>(commands), static_cast<unsigned long long>(refused));
    return 0;
}
