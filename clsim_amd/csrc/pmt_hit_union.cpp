// PMT hit frame store (pmt_hit_union.h): the host twins and the host store, which are series_union_host.h's over PmtHitUnion, under
// the names the rest of the library calls them by.  Host only: no HIP call.  The kernels, the device calls and the device store are
// in pmt_hit_union_kernel.hip.
#include "pmt_hit_union.h"

#include "series_union_host.h"

namespace clsimhip {

void pmt_hits_form_check(const char *what, const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series)
{
    series_form_check<PmtHitUnion>(what, records, n, series, n_series);
}

void pmt_hits_union_host(const clsimhip_pmt_hit *a_records, size_t n_a, const clsimhip_pmt_series *a_series, size_t n_series_a, const clsimhip_pmt_hit *b_records,
                         size_t n_b, const clsimhip_pmt_series *b_series, size_t n_series_b, clsimhip_pmt_hit *out_records, clsimhip_pmt_series *out_series,
                         size_t out_capacity, size_t *n, size_t *n_series)
{
    series_union_host<PmtHitUnion>(a_records, n_a, a_series, n_series_a, b_records, n_b, b_series, n_series_b, out_records, out_series, out_capacity, n, n_series);
}

void pmt_hits_split_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series, uint32_t last_frame,
                         clsimhip_pmt_hit *head_records, clsimhip_pmt_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                         clsimhip_pmt_hit *tail_records, clsimhip_pmt_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail)
{
    series_split_host<PmtHitUnion>(records, n, series, n_series, last_frame, head_records, head_series, head_capacity, n_head, n_series_head, tail_records, tail_series,
                                   tail_capacity, n_tail, n_series_tail);
}

std::unique_ptr<PmtHitStore> make_host_pmt_hit_store(size_t capacity) { return make_host_frame_store_of<PmtHitUnion>(capacity); }

} // namespace clsimhip
