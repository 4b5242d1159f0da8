// ltm_api_plane.cpp -- C ABI: RANSAC plane segmentation of the keyframes of a scan set or of one cloud (include/ltm.h, "planes"), the counterpart of
// pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC.  Kernels in ltm_k_plane.hip.
#include "ltm_internal.h"

struct ltm_planes : RecordSet {               // blocks: labels, hyp_counts, hyp_valid and the records' results
    size_t kf_begin = 0;                      // the range of the scan set the handle was made from (a cloud: one record)
    bool of_cloud = false;
    uint32_t max_iterations = 0;
    uint8_t* labels = nullptr;                // n_points
    uint32_t* counts = nullptr;               // n_records x max_iterations
    uint8_t* valid = nullptr;                 // n_records x max_iterations
    PlaneOut* out = nullptr;                  // n_records
    using RecordSet::RecordSet;
};

namespace {

// the parameters, checked, as the kernels take them
PlaneLaunch plane_launch(const ltm_plane_params* p)
{
    LTM_REQUIRE(p, "null argument");
    LTM_REQUIRE(std::isfinite(p->distance_threshold) && p->distance_threshold > 0.0, "distance_threshold must be finite and > 0");
    LTM_REQUIRE(p->max_iterations >= 1 && p->max_iterations <= (uint32_t)kPlaneMaxIterations, "need 1 <= max_iterations <= 4096");
    LTM_REQUIRE(std::isfinite(p->axis[0]) && std::isfinite(p->axis[1]) && std::isfinite(p->axis[2]), "axis must be finite");
    PlaneLaunch L;
    memset(&L, 0, sizeof L);
    L.thr = p->distance_threshold;
    L.max_iterations = p->max_iterations; L.seed = p->seed;
    L.has_axis = p->axis[0] != 0.0 || p->axis[1] != 0.0 || p->axis[2] != 0.0;
    L.refine = p->refine != 0;
    L.c2 = 0.0;
    if (L.has_axis) {
        LTM_REQUIRE(std::isfinite(p->eps_angle) && p->eps_angle >= 0.0, "eps_angle must be finite and >= 0");
        for (int d = 0; d < 3; ++d) L.axis[d] = p->axis[d];
        L.constrained = p->eps_angle < 1.5707963267948966;      // pi / 2 and beyond: every normal is within the angle
        if (L.constrained) { const double cs = cos(p->eps_angle); L.c2 = cs * cs; }
    }
    return L;
}

// records [0, bounds.size() - 1) of pts: record k holds points [bounds[k], bounds[k + 1])
std::unique_ptr<ltm_planes> segment(ltm_ctx* c, const float4* pts, std::vector<uint64_t> bounds, const PlaneLaunch& L)
{
    std::unique_ptr<ltm_planes> P(new ltm_planes(c));
    P->bounds = std::move(bounds);
    P->max_iterations = L.max_iterations;
    const size_t nr = P->n_records(), np = P->n_points(), H = L.max_iterations;
    if (!nr) return P;
    LTM_REQUIRE(nr < 0x7fffffffull / 16, "too many records");
    std::vector<PlaneRec> recs(nr);
    BlockTable table;
    uint64_t chunks = 0;
    for (size_t k = 0; k < nr; ++k) {
        const uint64_t n = P->bounds[k + 1] - P->bounds[k];
        if (n >= 0x80000000ull || chunks >= 0x80000000ull) throw Err{LTM_E_UNSUPPORTED, "a record of ltm_scanset_segment_planes must have fewer than 2^31 points"};
        PlaneRec& R = recs[k];
        R.pts = pts + P->bounds[k]; R.base = P->bounds[k]; R.n = (uint32_t)n; R.chunk0 = (uint32_t)chunks;
        if (!table.add((uint32_t)k, n, kPlaneBlockPoints, &R.span)) throw Err{LTM_E_UNSUPPORTED, "too many points in one ltm_scanset_segment_planes"};
        chunks += n / kPlaneChunk + (n % kPlaneChunk ? 1 : 0);
    }
    P->labels = P->blocks.alloc<uint8_t>(np);
    P->counts = P->blocks.alloc<uint32_t>(nr * H);
    P->valid = P->blocks.alloc<uint8_t>(nr * H);
    P->out = P->blocks.alloc<PlaneOut>(nr);
    unsigned long long* stats = c->plane_stats.get(c);
    ProfScope ps(c, "planes", (double)np * (double)H, 16.0 * (double)np + 64.0 * (double)(nr * H));
    DevBuf d_recs = to_device(c, recs), d_owner = to_device(c, table.owner());      // uploads: nothing is read back
    DevBuf hyp(c, nr * H * sizeof(PlaneHyp)), partials(c, std::max<uint64_t>(chunks, 1) * kPlaneMoments * sizeof(double));
    LTM_HIP(hipMemsetAsync(P->counts, 0, nr * H * sizeof(uint32_t), c->stream));
    LTM_HIP(hipMemsetAsync(P->out, 0, nr * sizeof(PlaneOut), c->stream));
    LTM_HIP(plane_segment(d_recs.as<PlaneRec>(), d_owner.as<uint32_t>(), table.size(), (uint32_t)nr, L, hyp.as<PlaneHyp>(), P->valid, P->counts,
                          partials.as<double>(), P->out, P->labels, stats, c->stream));
    return P;
}

} // namespace

extern "C" {

void ltm_plane_default_params(ltm_plane_params* p)
{
    if (!p) return;
    p->distance_threshold = 0.0;      // PCL's default: must be set
    p->max_iterations = 128;
    p->seed = 0;
    p->axis[0] = p->axis[1] = p->axis[2] = 0.0;      // SACMODEL_PLANE
    p->eps_angle = 0.0;
    p->refine = 1;                    // setOptimizeCoefficients(true)
}

uint32_t ltm_plane_block_points(void) { return (uint32_t)kPlaneBlockPoints; }

int ltm_scanset_segment_planes(ltm_ctx* c, ltm_scanset hs, size_t kf_begin, size_t kf_end, const ltm_plane_params* params, ltm_planes** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        const PlaneLaunch L = plane_launch(params);
        LTM_REQUIRE(out, "null argument");
        const ScanSet& s = get_ss(c, hs);
        LTM_REQUIRE(kf_begin <= kf_end && kf_end <= s.nkf(), "keyframe range out of bounds");
        const uint64_t first = s.off[kf_begin];
        std::vector<uint64_t> bounds(kf_end - kf_begin + 1);
        for (size_t j = 0; j < bounds.size(); ++j) bounds[j] = s.off[kf_begin + j] - first;
        // an error leaves nothing behind: the handle dies with `made`, its blocks with it, scratch with its DevBufs
        std::unique_ptr<ltm_planes> made = segment(c, s.d + first, std::move(bounds), L);
        made->kf_begin = kf_begin;
        *out = c->open.planes.adopt(made);
    });
}

int ltm_cloud_segment_plane(ltm_ctx* c, ltm_cloud hcloud, const ltm_plane_params* params, ltm_planes** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        const PlaneLaunch L = plane_launch(params);
        LTM_REQUIRE(out, "null argument");
        const Cloud cloud = get_cloud(c, hcloud);
        std::unique_ptr<ltm_planes> made = segment(c, cloud.d, std::vector<uint64_t>{0, (uint64_t)cloud.n}, L);
        made->of_cloud = true;
        *out = c->open.planes.adopt(made);
    });
}

int ltm_planes_info(ltm_ctx* c, ltm_planes* h, size_t* n_records, size_t* n_points, uint32_t* max_iterations)
{
    return guarded(c, [&] {
        const ltm_planes* s = c->open.planes.get(h);
        if (n_records) *n_records = s->n_records();
        if (n_points) *n_points = s->n_points();
        if (max_iterations) *max_iterations = s->max_iterations;
    });
}

int ltm_planes_device(ltm_ctx* c, ltm_planes* h, const uint8_t** labels_dev, const uint32_t** hyp_counts_dev, const uint8_t** hyp_valid_dev)
{
    return guarded(c, [&] {
        const ltm_planes* s = c->open.planes.get(h);
        if (labels_dev) *labels_dev = s->labels;
        if (hyp_counts_dev) *hyp_counts_dev = s->counts;
        if (hyp_valid_dev) *hyp_valid_dev = s->valid;
    });
}

int ltm_planes_download(ltm_ctx* c, ltm_planes* h, uint8_t* found, int32_t* best, uint32_t* consensus, uint32_t* n_valid, uint32_t* n_inliers, uint8_t* refined,
                        double* coeff4, double* point3, uint8_t* labels, uint32_t* hyp_counts, uint8_t* hyp_valid)
{
    return guarded(c, [&] {
        const ltm_planes* s = c->open.planes.get(h);
        const size_t nr = s->n_records(), H = s->max_iterations;
        if (nr && (found || best || consensus || n_valid || n_inliers || refined || coeff4 || point3)) {
            std::vector<PlaneOut> o(nr);
            d2h(c, o.data(), s->out, nr * sizeof(PlaneOut));
            for (size_t k = 0; k < nr; ++k) {
                if (found) found[k] = o[k].found;
                if (best) best[k] = o[k].best;
                if (consensus) consensus[k] = o[k].consensus;
                if (n_valid) n_valid[k] = o[k].n_valid;
                if (n_inliers) n_inliers[k] = o[k].n_inliers;
                if (refined) refined[k] = o[k].refined;
                if (coeff4) memcpy(coeff4 + 4 * k, o[k].coeff, 4 * sizeof(double));
                if (point3) memcpy(point3 + 3 * k, o[k].point, 3 * sizeof(double));
            }
        }
        if (labels) d2h(c, labels, s->labels, s->n_points());
        if (hyp_counts) d2h(c, hyp_counts, s->counts, nr * H * sizeof(uint32_t));
        if (hyp_valid) d2h(c, hyp_valid, s->valid, nr * H);
    });
}

int ltm_planes_split_scanset(ltm_ctx* c, ltm_planes* h, ltm_scanset hs, ltm_scanset* inliers, ltm_scanset* rest)
{
    return guarded(c, [&] {
        const ltm_planes* s = c->open.planes.get(h);
        LTM_REQUIRE(!s->of_cloud, "the plane set was made from a cloud (ltm_planes_split_cloud)");
        const ScanSet& ss = get_ss(c, hs);
        const size_t nr = s->n_records(), kb = s->kf_begin;
        LTM_REQUIRE(kb + nr <= ss.nkf(), "the scan set is not the one the plane set was made from (keyframe range)");
        const uint64_t first = ss.off[kb];
        for (size_t j = 0; j <= nr; ++j)
            LTM_REQUIRE(ss.off[kb + j] - first == s->bounds[j], "the scan set is not the one the plane set was made from (point counts differ)");
        LTM_REQUIRE(inliers && rest, "null argument");
        FlagSplit split(c);
        split_by_flag(c, ss.d + first, s->labels, s->n_points(), s->bounds, ss.off_dev, kb, first, split);
        split.hand_over(inliers, rest);
    });
}

int ltm_planes_split_cloud(ltm_ctx* c, ltm_planes* h, ltm_cloud hcloud, ltm_cloud* inliers, ltm_cloud* rest)
{
    return guarded(c, [&] {
        const ltm_planes* s = c->open.planes.get(h);
        LTM_REQUIRE(s->of_cloud, "the plane set was made from a scan set (ltm_planes_split_scanset)");
        LTM_REQUIRE(inliers && rest, "null argument");
        const Cloud cloud = get_cloud(c, hcloud);
        LTM_REQUIRE(cloud.n == s->n_points(), "the cloud is not the one the plane set was made from (point counts differ)");
        do_partition(c, cloud, s->labels, rest, inliers);
    });
}

int ltm_planes_free(ltm_ctx* c, ltm_planes* h)
{
    return guarded(c, [&] { c->open.planes.free(h); });
}

int ltm_debug_plane_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] { c->plane_stats.read(c, stats, reset); });
}

} // extern "C"
