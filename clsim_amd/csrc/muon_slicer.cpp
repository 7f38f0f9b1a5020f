// Muon slicer (muon_slicer.h): the reference's SliceMuonOrCopySubtree on a flattened tree, with an explicit stack.  Host only, binary64,
// every formula in the reference's operation order (this file is compiled with -ffp-contract=off like the rest of the host code).
#include "muon_slicer.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_model.h"

namespace clsimhip {

namespace {

// I3Units: m = ns = GeV = 1; I3Constants::c in m/ns
constexpr double kC = 0.299792458;
constexpr double kMillimetre = 1e-3, kKilometre = 1e3;
constexpr double kLog10 = 2.302585092994046;                            // log(10.)

bool is_muon(int32_t type) { return type == CLSIMHIP_PARTICLE_MUMINUS || type == CLSIMHIP_PARTICLE_MUPLUS; }

// gsl_hypot3
double hypot3(double x, double y, double z)
{
    const double xa = std::fabs(x), ya = std::fabs(y), za = std::fabs(z);
    const double yz = ya > za ? ya : za;
    const double w = xa > yz ? xa : yz;
    if (w == 0.) return 0.;
    return w * std::sqrt((xa / w) * (xa / w) + (ya / w) * (ya / w) + (za / w) * (za / w));
}

// DistanceFromInfiniteTrack (:145-168)
double distance_from_track(const clsimhip_particle &p, const clsimhip_particle &muon, double &on_track)
{
    const double hx = p.x - muon.x, hy = p.y - muon.y, hz = p.z - muon.z;
    const double s = muon.dx * hx + muon.dy * hy + muon.dz * hz;
    const double x2 = muon.x + s * muon.dx, y2 = muon.y + s * muon.dy, z2 = muon.z + s * muon.dz;
    on_track = s;
    return hypot3(x2 - p.x, y2 - p.y, z2 - p.z);
}

struct Frame {
    uint32_t node, out;
    bool slicing;
    size_t cursor;                                                      // next daughter
    double energy, time, dEdt, tf;                                      // currentEnergy, currentTime
    unsigned iteration;
    bool invalid_ei, invalid_ef;
};

struct Slicer {
    const clsimhip_tree_particle *tree;
    size_t n;
    std::vector<uint32_t> child_first, children;                        // node i: children[child_first[i] .. child_first[i + 1])
    std::vector<std::pair<uint32_t, uint32_t>> tracks;                  // (identifier, index), ascending
    const clsimhip_mmc_track *track_list;
    uint64_t first_slice;
    std::vector<clsimhip_tree_particle> out;
    std::vector<clsimhip_relabel> relabel;
    uint64_t counters[5] = {0, 0, 0, 0, 0};

    [[noreturn]] void fatal(uint32_t node, const std::string &what) const
    {
        throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: node " + std::to_string(node) + " (identifier " + std::to_string(tree[node].particle.identifier) + "): " + what);
    }
    size_t n_children(uint32_t node) const { return child_first[node + 1] - child_first[node]; }
    uint32_t child(uint32_t node, size_t k) const { return children[child_first[node] + k]; }

    uint32_t append(const clsimhip_tree_particle &p, int32_t parent)
    {
        out.push_back(p);
        out.back().parent = parent;
        return static_cast<uint32_t>(out.size() - 1u);
    }

    void append_slice(const Frame &f, double length)
    {
        const clsimhip_tree_particle &muon = tree[f.node];
        const double from_vertex = (f.time - muon.particle.time) * kC;  // lengthFromVertexToSliceStart
        clsimhip_tree_particle s = muon;                                // type, shape, direction, speed, flags as on input
        s.particle.x = muon.particle.x + muon.particle.dx * from_vertex;
        s.particle.y = muon.particle.y + muon.particle.dy * from_vertex;
        s.particle.z = muon.particle.z + muon.particle.dz * from_vertex;
        s.particle.time = f.time;
        s.particle.length = length;
        s.particle.energy = f.energy;
        const uint64_t identifier = first_slice + relabel.size();
        if (identifier > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: the slice identifiers wrap beyond 2^32 - 1");
        s.particle.identifier = static_cast<uint32_t>(identifier);
        s.particle.reserved = 0u;
        if (length > 1. * kKilometre) ++counters[MS_LONG_SLICE];
        append(s, static_cast<int32_t>(f.out));
        relabel.push_back(clsimhip_relabel{static_cast<uint32_t>(identifier), muon.particle.identifier});
    }

    // what SliceMuonOrCopySubtree does before its loops (:200-304): the frame a node is walked with
    Frame enter(uint32_t node, uint32_t out_index)
    {
        Frame f{};
        f.node = node; f.out = out_index;
        const clsimhip_particle &p = tree[node].particle;
        if (!((!std::isnan(p.length)) && (p.length > 0.) && is_muon(p.type))) return f;
        const size_t nc = n_children(node);
        for (size_t k = 0; k < nc; ++k) {
            const int32_t t = tree[child(node, k)].particle.type;
            if (is_muon(t) || t == 0) fatal(child(node, k), "a muon or a particle of type 0 below a muon with a length (sliced already?)");
        }
        const double speed = tree[node].speed;
        if (std::isnan(speed)) fatal(node, "the muon must have a speed");
        if (std::isnan(p.energy)) fatal(node, "the muon must have an energy");
        if (std::isnan(p.time)) fatal(node, "the muon must have a time");
        double ti = NAN, Ei = NAN, tf = NAN, Ef = NAN;
        const auto it = std::lower_bound(tracks.begin(), tracks.end(), std::make_pair(p.identifier, 0u));
        if (it != tracks.end() && it->first == p.identifier) {
            const clsimhip_mmc_track &t = track_list[it->second];
            ti = t.ti; Ei = t.Ei; tf = t.tf; Ef = t.Ef;
        }
        // AreParticlesSortedInTime, as its text means it (muon_slicer.h)
        for (size_t k = 0; k < nc; ++k) {
            const double t = tree[child(node, k)].particle.time;
            if (k == 0 ? std::isnan(t) : t < tree[child(node, k - 1)].particle.time) fatal(child(node, k), "the muon's daughters are not sorted in time (ascending)");
        }
        if ((Ei <= 0.) || std::isnan(Ei)) { Ei = p.energy; ti = p.time; f.invalid_ei = true; }
        if ((Ef < 0.) || std::isnan(Ef)) { Ef = 0.; tf = p.time + p.length / speed; f.invalid_ef = true; }
        if (std::isnan(ti)) fatal(node, "t_initial is NaN");
        if (std::isnan(tf)) fatal(node, "t_final is NaN");
        if (Ei <= 0) {
            if (nc > 0) fatal(node, "a muon with energy <= 0 has children");
        } else if (tf < ti) {
            ++counters[MS_STOPS_BEFORE_START];
            out[out_index].flags |= CLSIMHIP_TREE_DARK;
        } else if (tf == ti) {
            ++counters[MS_ZERO_DURATION];
            out[out_index].flags |= CLSIMHIP_TREE_DARK;
        } else {
            out[out_index].flags |= CLSIMHIP_TREE_DARK;
            double in_cascades = 0.;                                    // GetTotalEnergyOfParticles
            for (size_t k = 0; k < nc; ++k) {
                const clsimhip_particle &d = tree[child(node, k)].particle;
                if ((d.time < ti) || (d.time > tf)) continue;
                in_cascades += d.energy;
            }
            const double dEdt_calc = ((Ef - Ei + in_cascades) / (ti - tf));
            const double dEdt_max = (0.21 + 8.8e-3 * std::log(Ei / 1.) / kLog10) * (1. / 1.) * kC;
            f.dEdt = std::min(dEdt_calc, dEdt_max);
            f.slicing = true;
            f.energy = Ei;
            f.time = ti;
            f.tf = tf;
        }
        return f;
    }

    void walk(uint32_t root)
    {
        std::vector<Frame> stack;
        stack.push_back(enter(root, append(tree[root], -1)));
        while (!stack.empty()) {
            Frame &f = stack.back();
            const size_t nc = n_children(f.node);
            if (f.cursor < nc) {
                const uint32_t d = child(f.node, f.cursor++);
                if (!f.slicing) {                                       // something else, or a muon without slices: copy and recurse (:479-491)
                    const Frame next = enter(d, append(tree[d], static_cast<int32_t>(f.out)));
                    stack.push_back(next);                              // (f is dead from here)
                    continue;
                }
                const clsimhip_tree_particle &muon = tree[f.node];
                const clsimhip_particle &daughter = tree[d].particle;
                if (f.energy < 0.) { ++counters[MS_ENERGY_RESET]; f.energy = 0.; }
                double on_track = NAN;
                const double off_track = distance_from_track(daughter, muon.particle, on_track);
                if (off_track > 1. * kMillimetre) {                     // appended, not recursed into, the muon not split (:326-333)
                    ++counters[MS_OFF_TRACK];
                    append(tree[d], static_cast<int32_t>(f.out));
                    continue;
                }
                if (std::isnan(daughter.time)) continue;
                const double expected = muon.particle.time + on_track / muon.speed;
                double duration = expected - f.time;
                if (duration < 0.) duration = 0.;
                const double length = duration * kC;
                if (length >= 0.1 * kMillimetre) append_slice(f, length);       // (a slice the reference warns about as long is one it emits)
                const uint32_t at = append(tree[d], static_cast<int32_t>(f.out));
                f.time += duration;
                f.energy -= daughter.energy + f.dEdt * duration;
                ++f.iteration;
                const Frame next = enter(d, at);
                stack.push_back(next);
                continue;
            }
            if (f.slicing) {                                            // behind the last daughter (:421-470)
                const bool outgoing = f.iteration == 0 && f.invalid_ei && f.invalid_ef;
                if (!outgoing && !(f.energy < 0.)) {
                    const double length = (f.tf - f.time) * kC;
                    if (!(length <= 0.1 * kMillimetre)) append_slice(f, length);
                }
            }
            stack.pop_back();
        }
    }
};

} // namespace

void slice_muons(const clsimhip_tree_particle *tree, size_t n, const clsimhip_mmc_track *tracks, size_t n_tracks, uint32_t first_slice_identifier,
                 clsimhip_tree_particle *out, size_t capacity, size_t *n_out, clsimhip_relabel *relabel, size_t relabel_capacity, size_t *n_relabel,
                 uint64_t counters[5])
{
    if (n && !tree) throw Error(CLSIMHIP_ERR_ARGUMENT, "tree is (null)");
    if (n_tracks && !tracks) throw Error(CLSIMHIP_ERR_ARGUMENT, "tracks is (null)");
    if (capacity && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
    if (relabel_capacity && !relabel) throw Error(CLSIMHIP_ERR_ARGUMENT, "relabel is (null)");
    if (n > 0x7fffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: more than 2^31 - 1 nodes");
    Slicer S;
    S.tree = tree; S.n = n; S.track_list = tracks; S.first_slice = first_slice_identifier;
    S.tracks.reserve(n_tracks);
    for (size_t k = 0; k < n_tracks; ++k) S.tracks.emplace_back(tracks[k].identifier, static_cast<uint32_t>(k));
    std::sort(S.tracks.begin(), S.tracks.end());
    for (size_t k = 1; k < n_tracks; ++k)
        if (S.tracks[k].first == S.tracks[k - 1].first)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: identifier " + std::to_string(S.tracks[k].first) + " is more than once in the track list (entry " +
                                                   std::to_string(S.tracks[k].second) + ")");
    S.child_first.assign(n + 1u, 0u);
    for (size_t i = 0; i < n; ++i) {
        const int32_t p = tree[i].parent;
        if (p < -1 || (p >= 0 && static_cast<size_t>(p) >= i))
            throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: node " + std::to_string(i) + " has parent " + std::to_string(p) + " (a parent lies in front of its children; -1: a primary)");
        if (p >= 0) ++S.child_first[static_cast<size_t>(p) + 1u];
    }
    for (size_t i = 0; i < n; ++i) S.child_first[i + 1u] += S.child_first[i];
    S.children.resize(S.child_first[n]);
    {
        std::vector<uint32_t> filled(S.child_first.begin(), S.child_first.end() - 1);
        for (size_t i = 0; i < n; ++i)
            if (tree[i].parent >= 0) S.children[filled[static_cast<size_t>(tree[i].parent)]++] = static_cast<uint32_t>(i);
    }
    S.out.reserve(n + n / 2u);
    for (size_t i = 0; i < n; ++i)                                      // the primaries loop (:531-555)
        if (tree[i].parent < 0) S.walk(static_cast<uint32_t>(i));
    const uint64_t slices = S.relabel.size();
    for (size_t i = 0; i < n && slices; ++i) {
        const uint64_t id = tree[i].particle.identifier;
        if (id >= S.first_slice && id - S.first_slice < slices)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "muon slicer: node " + std::to_string(i) + " carries identifier " + std::to_string(id) + ", which is one of the " +
                                                   std::to_string(slices) + " slice identifiers from " + std::to_string(S.first_slice));
    }
    std::copy(S.out.begin(), S.out.begin() + std::min(capacity, S.out.size()), out);
    std::copy(S.relabel.begin(), S.relabel.begin() + std::min(relabel_capacity, S.relabel.size()), relabel);
    if (n_out) *n_out = S.out.size();
    if (n_relabel) *n_relabel = S.relabel.size();
    if (counters) std::copy(S.counters, S.counters + 5, counters);
}

} // namespace clsimhip
