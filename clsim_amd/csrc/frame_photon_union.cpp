// Frame photon store (frame_photon_union.h): the host twins and the host store, which are series_union_host.h's over FramePhotonUnion,
// under the names the rest of the library calls them by.  Host only: no HIP call.  The kernels, the device calls and the device
// store are in frame_photon_union_kernel.hip.
#include "frame_photon_union.h"

#include "series_union_host.h"

namespace clsimhip {

void frame_photons_form_check(const char *what, const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series)
{
    series_form_check<FramePhotonUnion>(what, records, n, series, n_series);
}

void frame_photons_union_host(const clsimhip_frame_photon *a_records, size_t n_a, const clsimhip_mcpe_series *a_series, size_t n_series_a,
                              const clsimhip_frame_photon *b_records, size_t n_b, const clsimhip_mcpe_series *b_series, size_t n_series_b,
                              clsimhip_frame_photon *out_records, clsimhip_mcpe_series *out_series, size_t out_capacity, size_t *n, size_t *n_series)
{
    series_union_host<FramePhotonUnion>(a_records, n_a, a_series, n_series_a, b_records, n_b, b_series, n_series_b, out_records, out_series, out_capacity, n, n_series);
}

void frame_photons_split_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, uint32_t last_frame,
                              clsimhip_frame_photon *head_records, clsimhip_mcpe_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                              clsimhip_frame_photon *tail_records, clsimhip_mcpe_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail)
{
    series_split_host<FramePhotonUnion>(records, n, series, n_series, last_frame, head_records, head_series, head_capacity, n_head, n_series_head, tail_records,
                                        tail_series, tail_capacity, n_tail, n_series_tail);
}

std::unique_ptr<FramePhotonStore> make_host_frame_photon_store(size_t capacity) { return make_host_frame_store_of<FramePhotonUnion>(capacity); }

} // namespace clsimhip
