// ltm_api_outlier.cpp -- C ABI: statistical and radius outlier removal over the targets of search indices (include/ltm.h, "outlier filters"), the
// counterparts of pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval.  Kernels in ltm_k_outlier.hip; the split is the planes' (split_by_flag,
// do_partition).
#include "ltm_internal.h"

struct ltm_outliers : IndexRecordSet {        // blocks: offsets, labels, distances or counts and the records' rows
    int kind = LTM_OUTLIERS_STATISTICAL;
    uint8_t* labels = nullptr;                // n_points, every record in its target's original order
    float* dist = nullptr;                    // n_points (statistical)
    uint32_t* counts = nullptr;               // n_points (radius)
    OutlierRec* out = nullptr;                // n_records
    using IndexRecordSet::IndexRecordSet;
};

namespace {

// The listed indices as the records of one call, checked before the device is touched, and the owner tables: per_block finite points per workgroup,
// kOutlierChunk original positions per chunk
struct Batch {
    std::vector<OutlierSeg> segs;
    BlockTable points, chunks;
    uint64_t total_f = 0;
};
std::unique_ptr<ltm_outliers> open_batch(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, int kind, uint32_t per_block, Batch& B)
{
    check_listed_indices(n_idx, idx, 0x7fffffffull / 16);
    std::unique_ptr<ltm_outliers> P(new ltm_outliers(c, n_idx));
    P->kind = kind;
    B.segs.resize(n_idx);
    const char* over_table = "too many target points in one outlier filter call";
    for_listed_indices(c, n_idx, idx, B.points, per_block, true, "the indices of one outlier filter call must have fewer than 2^31 target points in all", over_table,
                       [&](size_t k, const ListedIndex& L) {
        OutlierSeg& S = B.segs[k];
        memset(&S, 0, sizeof S);
        S.t = L.t; S.n_target = L.n_target; S.tbase = L.tbase; S.span = L.span;
        P->set_record(k, L);
        B.total_f += S.t.Mf;
        if (!B.chunks.add((uint32_t)k, L.n_target, kOutlierChunk, &S.tspan)) throw Err{LTM_E_UNSUPPORTED, over_table};
    });
    return P;
}

// the arrays every handle has: offsets (uploaded), labels and the records' rows; values: 4 bytes per position, zeroed like the labels
void* alloc_arrays(ltm_ctx* c, ltm_outliers* P)
{
    const size_t nr = P->n_records(), np = P->n_points();
    P->offsets = P->blocks.alloc<uint64_t>(nr + 1);
    P->labels = P->blocks.alloc<uint8_t>(np);
    void* values = P->blocks.alloc<uint32_t>(np);
    P->out = P->blocks.alloc<OutlierRec>(nr);
    h2d(c, P->offsets, P->bounds.data(), (nr + 1) * sizeof(uint64_t));
    if (np) {
        LTM_HIP(hipMemsetAsync(P->labels, 0, np, c->stream));
        LTM_HIP(hipMemsetAsync(values, 0, np * 4, c->stream));      // non-finite positions: label 0, distance 0.0f, count 0
    }
    return values;
}

} // namespace

extern "C" {

void ltm_sor_default_params(ltm_sor_params* p)
{
    if (!p) return;
    p->mean_k = 1;            // PCL's constructor
    p->stddev_mul = 0.0;
}

void ltm_ror_default_params(ltm_ror_params* p)
{
    if (!p) return;
    p->radius = 0.0;          // PCL's default: must be set
    p->min_neighbors = 1;
}

int ltm_search_filter_statistical(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, const ltm_sor_params* params, ltm_outliers** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(params && out, "null argument");
        LTM_REQUIRE(params->mean_k >= 1 && params->mean_k <= (uint32_t)(kOutlierMaxSlots - 1), "need 1 <= mean_k <= 63");
        LTM_REQUIRE(std::isfinite(params->stddev_mul), "stddev_mul must be finite");
        const int mean_k = (int)params->mean_k;
        Batch B;
        // an error leaves nothing behind: the handle dies with `made`, its blocks with it, scratch with its DevBufs
        std::unique_ptr<ltm_outliers> made = open_batch(c, n_idx, idx, LTM_OUTLIERS_STATISTICAL, (uint32_t)outlier_sor_block(mean_k), B);
        made->dist = static_cast<float*>(alloc_arrays(c, made.get()));
        if (n_idx) {
            unsigned long long* stats = c->outlier_stats.get(c);
            ProfScope ps(c, "outliers_sor", (double)B.total_f * (double)(mean_k + 1), 24.0 * (double)B.total_f + 5.0 * (double)made->n_points());
            DevBuf d_segs = to_device(c, B.segs), d_points = to_device(c, B.points.owner()), d_chunks = to_device(c, B.chunks.owner());      // uploads: nothing is read back
            DevBuf partials(c, std::max<size_t>(B.chunks.size(), 1) * 2 * sizeof(double));
            LTM_HIP(outlier_statistical(d_segs.as<OutlierSeg>(), d_points.as<uint32_t>(), B.points.size(), d_chunks.as<uint32_t>(), B.chunks.size(), (uint32_t)n_idx,
                                        mean_k, params->stddev_mul, made->dist, partials.as<double>(), made->out, made->labels, stats, c->stream));
        }
        *out = c->open.outliers.adopt(made);
    });
}

int ltm_search_filter_radius(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, const ltm_ror_params* params, ltm_outliers** out)
{
    if (out) *out = nullptr;
    return guarded(c, [&] {
        LTM_REQUIRE(params && out, "null argument");
        LTM_REQUIRE(std::isfinite(params->radius) && params->radius > 0.0, "radius must be finite and > 0");
        LTM_REQUIRE(params->min_neighbors >= 1, "need min_neighbors >= 1");
        const float r2 = (float)(params->radius * params->radius);
        Batch B;
        std::unique_ptr<ltm_outliers> made = open_batch(c, n_idx, idx, LTM_OUTLIERS_RADIUS, kOutlierBlock, B);
        made->counts = static_cast<uint32_t*>(alloc_arrays(c, made.get()));
        if (n_idx) {
            unsigned long long* stats = c->outlier_stats.get(c);
            ProfScope ps(c, "outliers_ror", (double)B.total_f, 24.0 * (double)B.total_f + 5.0 * (double)made->n_points());
            DevBuf d_segs = to_device(c, B.segs), d_points = to_device(c, B.points.owner());
            LTM_HIP(outlier_radius(d_segs.as<OutlierSeg>(), d_points.as<uint32_t>(), B.points.size(), (uint32_t)n_idx, r2, params->min_neighbors, made->counts,
                                   made->out, made->labels, stats, c->stream));
        }
        *out = c->open.outliers.adopt(made);
    });
}

int ltm_outliers_info(ltm_ctx* c, ltm_outliers* h, int* kind, size_t* n_records, size_t* n_points)
{
    return guarded(c, [&] {
        const ltm_outliers* s = c->open.outliers.get(h);
        if (kind) *kind = s->kind;
        if (n_records) *n_records = s->n_records();
        if (n_points) *n_points = s->n_points();
    });
}

int ltm_outliers_device(ltm_ctx* c, ltm_outliers* h, const uint64_t** offsets_dev, const uint8_t** labels_dev, const float** distances_dev,
                        const uint32_t** counts_dev)
{
    return guarded(c, [&] {
        const ltm_outliers* s = c->open.outliers.get(h);
        if (offsets_dev) *offsets_dev = s->offsets;
        if (labels_dev) *labels_dev = s->labels;
        if (distances_dev) *distances_dev = s->dist;
        if (counts_dev) *counts_dev = s->counts;
    });
}

int ltm_outliers_download(ltm_ctx* c, ltm_outliers* h, uint32_t* n_target, uint32_t* n_finite, uint32_t* n_kept, double* mean, double* stddev, double* threshold,
                          uint8_t* labels, float* distances, uint32_t* counts)
{
    return guarded(c, [&] {
        const ltm_outliers* s = c->open.outliers.get(h);
        const bool sor = s->kind == LTM_OUTLIERS_STATISTICAL;
        LTM_REQUIRE(sor || !(mean || stddev || threshold || distances), "a radius outlier set has no statistics and no distances");
        LTM_REQUIRE(!sor || !counts, "a statistical outlier set has no counts");
        const size_t nr = s->n_records();
        s->record_sizes(n_target, n_finite);
        if (nr && (n_kept || mean || stddev || threshold)) {
            std::vector<OutlierRec> o(nr);
            d2h(c, o.data(), s->out, nr * sizeof(OutlierRec));
            for (size_t k = 0; k < nr; ++k) {
                if (n_kept) n_kept[k] = o[k].n_kept;
                if (mean) mean[k] = o[k].mean;
                if (stddev) stddev[k] = o[k].stddev;
                if (threshold) threshold[k] = o[k].threshold;
            }
        }
        if (labels) d2h(c, labels, s->labels, s->n_points());
        if (distances) d2h(c, distances, s->dist, s->n_points() * sizeof(float));
        if (counts) d2h(c, counts, s->counts, s->n_points() * sizeof(uint32_t));
    });
}

int ltm_outliers_split_scanset(ltm_ctx* c, ltm_outliers* h, ltm_scanset hs, ltm_scanset* kept, ltm_scanset* removed)
{
    return guarded(c, [&] {
        const ltm_outliers* s = c->open.outliers.get(h);
        const ScanSet& ss = get_ss(c, hs);
        const size_t nr = s->n_records();
        LTM_REQUIRE(ss.nkf() == nr, "the scan set has not one keyframe per record of the outlier set");
        for (size_t j = 0; j <= nr; ++j) LTM_REQUIRE(ss.off[j] == s->bounds[j], "a keyframe of the scan set has not as many points as its record's target");
        LTM_REQUIRE(kept && removed, "null argument");
        FlagSplit split(c);
        split_by_flag(c, ss.d, s->labels, s->n_points(), s->bounds, ss.off_dev, 0, 0, split);
        split.hand_over(kept, removed);
    });
}

int ltm_outliers_split_cloud(ltm_ctx* c, ltm_outliers* h, ltm_cloud hcloud, ltm_cloud* kept, ltm_cloud* removed)
{
    return guarded(c, [&] {
        const ltm_outliers* s = c->open.outliers.get(h);
        LTM_REQUIRE(s->n_records() == 1, "ltm_outliers_split_cloud takes an outlier set of one record (ltm_outliers_split_scanset)");
        LTM_REQUIRE(kept && removed, "null argument");
        const Cloud cloud = get_cloud(c, hcloud);
        LTM_REQUIRE(cloud.n == s->n_points(), "the cloud has not as many points as the record's target");
        do_partition(c, cloud, s->labels, removed, kept);
    });
}

int ltm_outliers_free(ltm_ctx* c, ltm_outliers* h)
{
    return guarded(c, [&] { c->open.outliers.free(h); });
}

int ltm_debug_outlier_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] { c->outlier_stats.read(c, stats, reset); });
}

} // extern "C"
