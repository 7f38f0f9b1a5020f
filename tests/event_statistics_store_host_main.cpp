// The event statistics frame store's host twins and host store (clsim_amd/csrc/event_stats_store.cpp) as a stand-alone program, for the
// sanitizers: no Python, no GPU.
//   event_statistics_store_host_main IN OUT
// IN is a sequence of commands, each a uint64 code and its arguments (sizes are uint64; a list is n and n clsimhip_event_statistics, a
// map n_map and n_map clsimhip_relabel):
//   1 canonical: capacity, map, L                       -> status, the form, RELABELLED, EMPTY_DROPPED
//   2 combine:   capacity, A, B                         -> status, the form
//   3 split:     last_frame, head_capacity, tail_capacity, X -> status, the head, the tail
//   4 store:     capacity                               -> status          (replaces the program's one store)
//   5 add:       map, L                                 -> status
//   6 drain:     last_frame, capacity, map              -> status, the head
//   7 size:      last_frame                             -> status, n
// OUT: per command a uint64 status (0, or the error code of a refusal as a positive number) and, with status 0, its results.  Output
// arrays are allocated at exactly the sizes the interface names, so a write past them is seen.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "event_stats_store.h"
#include "host_model.h"

namespace {
using List = std::vector<clsimhip_event_statistics>;
using Map = std::vector<clsimhip_relabel>;

bool read_u64(std::FILE *f, uint64_t &v) { return std::fread(&v, 8, 1, f) == 1; }
template <class T>
bool read_array(std::FILE *f, std::vector<T> &x)
{
    uint64_t n;
    if (!read_u64(f, n)) return false;
    x.resize(n);
    return n == 0 || std::fread(x.data(), sizeof(T), n, f) == n;
}
void write_u64(std::FILE *f, uint64_t v) { std::fwrite(&v, 8, 1, f); }
void write_list(std::FILE *f, const List &x, size_t n)
{
    write_u64(f, n);
    if (n) std::fwrite(x.data(), sizeof(clsimhip_event_statistics), n, f);
}
int short_input() { std::fprintf(stderr, "short input or no store\n"); return 2; }
} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    std::unique_ptr<clsimhip::EventStatsStore> store;
    uint64_t code, commands = 0, refused = 0;
    while (read_u64(in, code)) {
        ++commands;
        try {
            if (code == 1u) {
                uint64_t capacity;
                Map map;
                List x;
                if (!read_u64(in, capacity) || !read_array(in, map) || !read_array(in, x)) return short_input();
                List made(capacity);
                size_t n = 0;
                uint64_t counters[2] = {0, 0};
                clsimhip::event_stats_canonical_host(x.data(), x.size(), map.data(), map.size(), made.data(), capacity, &n, counters);
                write_u64(out, 0);
                write_list(out, made, n);
                write_u64(out, counters[0]);
                write_u64(out, counters[1]);
            } else if (code == 2u) {
                uint64_t capacity;
                List a, b;
                if (!read_u64(in, capacity) || !read_array(in, a) || !read_array(in, b)) return short_input();
                List made(capacity);
                size_t n = 0;
                clsimhip::event_stats_combine_host(a.data(), a.size(), b.data(), b.size(), made.data(), capacity, &n);
                write_u64(out, 0);
                write_list(out, made, n);
            } else if (code == 3u) {
                uint64_t last_frame, head_capacity, tail_capacity;
                List x;
                if (!read_u64(in, last_frame) || !read_u64(in, head_capacity) || !read_u64(in, tail_capacity) || !read_array(in, x)) return short_input();
                List head(head_capacity), tail(tail_capacity);
                size_t n_head = 0, n_tail = 0;
                clsimhip::event_stats_split_host(x.data(), x.size(), static_cast<uint32_t>(last_frame), head.data(), head_capacity, &n_head, tail.data(), tail_capacity,
                                                 &n_tail);
                write_u64(out, 0);
                write_list(out, head, n_head);
                write_list(out, tail, n_tail);
            } else if (code == 4u) {
                uint64_t capacity;
                if (!read_u64(in, capacity)) return short_input();
                store = clsimhip::make_host_event_stats_store(capacity);
                write_u64(out, 0);
            } else if (code == 5u) {
                Map map;
                List x;
                if (!read_array(in, map) || !read_array(in, x) || !store) return short_input();
                store->add_host(x.data(), x.size(), map.data(), map.size());
                write_u64(out, 0);
            } else if (code == 6u) {
                uint64_t last_frame, capacity;
                Map map;
                if (!read_u64(in, last_frame) || !read_u64(in, capacity) || !read_array(in, map) || !store) return short_input();
                List head(capacity);
                size_t n = 0;
                store->drain_host(static_cast<uint32_t>(last_frame), map.data(), map.size(), head.data(), capacity, &n);
                write_u64(out, 0);
                write_list(out, head, n);
            } else if (code == 7u) {
                uint64_t last_frame;
                if (!read_u64(in, last_frame) || !store) return short_input();
                size_t n = 0;
                store->size(static_cast<uint32_t>(last_frame), &n);
                write_u64(out, 0);
                write_u64(out, n);
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
