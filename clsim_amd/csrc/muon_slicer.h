// Muon slicer: a muon with a length is cut into slices between its stochastic losses, each with the energy the muon still has there
// (include/clsimhip.h: "Muon slicer").  Sequential binary64 host code, no HIP call.  It restates
//   SliceMuonOrCopySubtree   private/clsim/util/I3MuonSlicer.cxx:182-493, with its helpers DistanceFromInfiniteTrack (:145-168),
//                            GetTotalEnergyOfParticles (:127-143), AreParticlesSortedInTime (:105-125), IsAnyOfType (:95-103)
//   the primaries loop       :531-555
// on a flattened tree in depth-first pre-order.  The reference recurses on the C stack; here an explicit stack of frames walks the
// child lists built from the parent indices.  The block under TRY_TO_CORRECT_MMC (:344-368) is compiled out upstream and is not here.
//
// One departure, on purpose.  AreParticlesSortedInTime never clears its firstIt flag, so upstream it returns false exactly when some
// daughter's time is NaN and never notices descending times.  Here it is what its text means to be: the first daughter's time must
// not be NaN and no daughter's time may be less than its predecessor's (a comparison with a NaN is false, so a later NaN passes and
// the daughter is dropped at :335, with its subtree, as the reference's loop body does it).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/clsimhip.h"

namespace clsimhip {

enum MuonSlicerCounter : int { MS_OFF_TRACK = 0, MS_ENERGY_RESET = 1, MS_STOPS_BEFORE_START = 2, MS_ZERO_DURATION = 3, MS_LONG_SLICE = 4 };

// throws Error (CLSIMHIP_ERR_ARGUMENT) before anything is written
void slice_muons(const clsimhip_tree_particle *tree, size_t n, const clsimhip_mmc_track *tracks, size_t n_tracks, uint32_t first_slice_identifier,
                 clsimhip_tree_particle *out, size_t capacity, size_t *n_out, clsimhip_relabel *relabel, size_t relabel_capacity, size_t *n_relabel,
                 uint64_t counters[5]);

} // namespace clsimhip
