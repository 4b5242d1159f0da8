// ltm_api_cluster.cpp -- C ABI: Euclidean cluster extraction over the targets of search indices (include/ltm.h, "clusters"), the counterpart of
// pcl::EuclideanClusterExtraction.  Kernels in ltm_k_cluster.hip, the union-find in ltm_unionfind.h.
#include "ltm_internal.h"

struct ltm_clusters {
    std::shared_ptr<PoolBlocks> batch;        // every pointer below points into the blocks that the cluster sets of one ltm_search_cluster share
    size_t n_target = 0, n_clusters = 0, n_points = 0;
    int32_t* labels = nullptr;                // n_target, the target's original order
    uint64_t* offsets = nullptr;              // n_clusters + 1
    int32_t* idx = nullptr;                   // n_points
    uint32_t* sizes = nullptr; int32_t* first = nullptr; float* box = nullptr; double* centroid = nullptr;
};

namespace {

void cluster_batch(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, const ltm_cluster_params& p, std::vector<std::unique_ptr<ltm_clusters>>& out)
{
    const float r2 = (float)(p.tolerance * p.tolerance);
    const uint32_t min_size = p.min_size, max_size = p.max_size ? p.max_size : 0xffffffffu;
    auto batch = std::make_shared<PoolBlocks>(c);
    std::vector<ClusterSeg> segs(n_idx);
    BlockTable table;
    uint64_t total_f = 0, total_t = 0;
    out.resize(n_idx);
    for_listed_indices(c, n_idx, idx, table, kClusterBlock, false, "the indices of one ltm_search_cluster must have fewer than 2^31 target points in all",
                       "too many target points in one ltm_search_cluster", [&](size_t k, const ListedIndex& L) {
        ClusterSeg& S = segs[k];
        memset(&S, 0, sizeof S);
        S.t = L.t; S.n_target = L.n_target; S.fbase = L.fbase; S.tbase = L.tbase; S.span = L.span;
        while (((uint32_t)1 << S.logP) < S.t.P) ++S.logP;
        total_f += S.t.Mf; total_t += L.n_target;
        out[k].reset(new ltm_clusters);
        out[k]->batch = batch;
        out[k]->n_target = L.n_target;
    });
    const uint32_t n_blocks = table.size();
    int32_t* labels = batch->alloc<int32_t>(total_t);
    LTM_HIP(fill_u32(reinterpret_cast<uint32_t*>(labels), 0xffffffffu, total_t, c->stream));
    std::vector<uint64_t> coff(n_idx + 1, 0), poff(n_idx + 1, 0);
    if (total_f) {
        ProfScope ps(c, "cluster", (double)total_f, 48.0 * (double)total_f);
        DevBuf d_segs = to_device(c, segs), d_bs = to_device(c, table.owner());
        const size_t n_cnt = 6 + 2 * n_idx;
        DevBuf parent(c, total_f * 4), root(c, total_f * 4), size(c, total_f * 4), minidx(c, total_f * 4), cid(c, total_f * 4), keep(c, total_f), pos(c, total_f * 4),
            cnt(c, n_cnt * 8);
        LTM_HIP(hipMemsetAsync(cnt.p, 0, n_cnt * 8, c->stream));
        LTM_HIP(cluster_hook(d_segs.as<ClusterSeg>(), d_bs.as<uint32_t>(), n_blocks, r2, c->cluster_clique, parent.as<uint32_t>(), root.as<uint32_t>(),
                             size.as<uint32_t>(), minidx.as<uint32_t>(), cid.as<int32_t>(), cnt.as<unsigned long long>(), c->stream));
        LTM_HIP(cluster_roots(d_segs.as<ClusterSeg>(), d_bs.as<uint32_t>(), n_blocks, root.as<uint32_t>(), size.as<uint32_t>(), min_size, max_size,
                              keep.as<uint8_t>(), cnt.as<unsigned long long>() + 6, c->stream));
        scan_flags(c, keep.as<uint8_t>(), total_f, pos);
        std::vector<uint64_t> h_cnt(n_cnt);
        d2h(c, h_cnt.data(), cnt.p, n_cnt * 8);      // the one read-back: counters, and the clusters and clustered points of every index, which size the handles
        for (int i = 0; i < 6; ++i) c->cluster_stats[i] += h_cnt[i];
        for (size_t k = 0; k < n_idx; ++k) {
            out[k]->n_clusters = h_cnt[6 + 2 * k];
            out[k]->n_points = h_cnt[6 + 2 * k + 1];
            if (out[k]->n_clusters > segs[k].t.Mf || out[k]->n_points > segs[k].t.Mf) throw Err{LTM_E_DEVICE, "cluster counts outside the index"};
            coff[k + 1] = coff[k] + out[k]->n_clusters;
            poff[k + 1] = poff[k] + out[k]->n_points;
        }
        const uint64_t nc = coff[n_idx], np = poff[n_idx];
        uint64_t* offsets = batch->alloc<uint64_t>(nc + n_idx);      // (no cluster, no clustered point: the pool's smallest block)
        int32_t* pidx = batch->alloc<int32_t>(np);
        uint32_t* sizes = batch->alloc<uint32_t>(nc);
        int32_t* first = batch->alloc<int32_t>(nc);
        float* box = batch->alloc<float>(nc * 6);
        double* centroid = batch->alloc<double>(nc * 3);
        LTM_HIP(hipMemsetAsync(offsets, 0, (nc + n_idx) * 8, c->stream));
        if (nc) {
            DevBuf d_coff = to_device(c, coff);
            const size_t tb = cluster_temp_bytes(nc, n_idx);
            DevBuf keys(c, nc * 8), keys_s(c, nc * 8), vals(c, nc * 4), vals_s(c, nc * 4), csize(c, (nc + 1) * 4), cfirst(c, nc * 4), cseg(c, nc * 4),
                cchunks(c, (nc + 1) * 4), goff(c, (nc + 1) * 4), choff(c, (nc + 1) * 4), temp(c, tb);
            LTM_HIP(cluster_number(keep.as<uint8_t>(), pos.as<uint32_t>(), total_f, size.as<uint32_t>(), minidx.as<uint32_t>(), (uint32_t)nc, d_coff.as<uint64_t>(),
                                   (uint32_t)n_idx, keys.as<uint64_t>(), keys_s.as<uint64_t>(), vals.as<uint32_t>(), vals_s.as<uint32_t>(), cid.as<int32_t>(),
                                   csize.as<uint32_t>(), cfirst.as<int32_t>(), cseg.as<uint32_t>(), cchunks.as<uint32_t>(), goff.as<uint32_t>(), choff.as<uint32_t>(),
                                   temp.p, tb, c->stream));
            DevBuf pkeys(c, np * 8), pkeys_s(c, np * 8), pvals(c, np * 4), pvals_s(c, np * 4), cursor(c, 4);
            LTM_HIP(cluster_labels(d_segs.as<ClusterSeg>(), d_bs.as<uint32_t>(), n_blocks, root.as<uint32_t>(), cid.as<int32_t>(), d_coff.as<uint64_t>(), labels,
                                   pkeys.as<uint64_t>(), pvals.as<uint32_t>(), cursor.as<uint32_t>(), c->stream));
            unsigned cbits = 1;
            while (cbits < 32 && ((uint64_t)1 << cbits) < nc) ++cbits;
            {
                const size_t stb = sort_temp_bytes(np);
                DevBuf stemp(c, stb);
                LTM_HIP(sort_pairs_u64(pkeys.as<uint64_t>(), pkeys_s.as<uint64_t>(), pvals.as<uint32_t>(), pvals_s.as<uint32_t>(), np, 32 + cbits, stemp.p, stb,
                                       c->stream));
            }
            const size_t mc = cluster_max_chunks(nc, np);
            DevBuf psum(c, mc * 3 * sizeof(double)), pbox(c, mc * 6 * sizeof(uint32_t));
            LTM_HIP(cluster_finish(d_segs.as<ClusterSeg>(), pkeys_s.as<uint64_t>(), pvals_s.as<uint32_t>(), (uint32_t)nc, np, csize.as<uint32_t>(), cfirst.as<int32_t>(),
                                   cseg.as<uint32_t>(), goff.as<uint32_t>(), choff.as<uint32_t>(), d_coff.as<uint64_t>(), psum.as<double>(), pbox.as<uint32_t>(), pidx,
                                   sizes, first, box, centroid, offsets, c->stream));
        }
        for (size_t k = 0; k < n_idx; ++k) {
            ltm_clusters* s = out[k].get();
            s->offsets = offsets + coff[k] + k; s->idx = pidx + poff[k];
            s->sizes = sizes + coff[k]; s->first = first + coff[k]; s->box = box + 6 * coff[k]; s->centroid = centroid + 3 * coff[k];
        }
    } else {
        uint64_t* offsets = batch->alloc<uint64_t>(n_idx);
        LTM_HIP(hipMemsetAsync(offsets, 0, n_idx * 8, c->stream));
        for (size_t k = 0; k < n_idx; ++k) out[k]->offsets = offsets + k;
    }
    for (size_t k = 0; k < n_idx; ++k) out[k]->labels = labels + segs[k].tbase;
}

} // namespace

extern "C" {

void ltm_cluster_default_params(ltm_cluster_params* p)
{
    if (!p) return;
    p->tolerance = 0.0;      // PCL's default: must be set
    p->min_size = 1;
    p->max_size = 0;         // no upper limit (PCL: INT_MAX)
}

int ltm_search_cluster(ltm_ctx* c, size_t n_idx, ltm_search* const* idx, const ltm_cluster_params* params, ltm_clusters** out)
{
    return guarded(c, [&] {
        LTM_REQUIRE(params, "null argument");
        LTM_REQUIRE(std::isfinite(params->tolerance) && params->tolerance > 0.0, "tolerance must be finite and > 0");
        LTM_REQUIRE(params->min_size >= 1 && (params->max_size == 0 || params->max_size >= params->min_size), "need 1 <= min_size <= max_size (max_size 0: no limit)");
        if (!n_idx) return;
        LTM_REQUIRE(out, "null argument");
        check_listed_indices(n_idx, idx, 0x7fffffffull);
        std::vector<std::unique_ptr<ltm_clusters>> made;
        // an error leaves nothing behind: the handles die with `made`, the shared blocks with the last reference to the batch, scratch with its DevBufs
        cluster_batch(c, n_idx, idx, *params, made);
        c->open.clusters.adopt(made, out);
    });
}

int ltm_clusters_info(ltm_ctx* c, ltm_clusters* h, size_t* n_target, size_t* n_clusters, size_t* n_clustered_points)
{
    return guarded(c, [&] {
        const ltm_clusters* s = c->open.clusters.get(h);
        if (n_target) *n_target = s->n_target;
        if (n_clusters) *n_clusters = s->n_clusters;
        if (n_clustered_points) *n_clustered_points = s->n_points;
    });
}

int ltm_clusters_device(ltm_ctx* c, ltm_clusters* h, const int32_t** labels_dev, const uint64_t** offsets_dev, const int32_t** idx_dev)
{
    return guarded(c, [&] {
        const ltm_clusters* s = c->open.clusters.get(h);
        if (labels_dev) *labels_dev = s->labels;
        if (offsets_dev) *offsets_dev = s->offsets;
        if (idx_dev) *idx_dev = s->idx;
    });
}

int ltm_clusters_download(ltm_ctx* c, ltm_clusters* h, int32_t* labels, uint32_t* sizes, int32_t* first_idx, float* box6, double* centroid3)
{
    return guarded(c, [&] {
        const ltm_clusters* s = c->open.clusters.get(h);
        if (labels) d2h(c, labels, s->labels, s->n_target * 4);
        if (sizes) d2h(c, sizes, s->sizes, s->n_clusters * 4);
        if (first_idx) d2h(c, first_idx, s->first, s->n_clusters * 4);
        if (box6) d2h(c, box6, s->box, s->n_clusters * 6 * sizeof(float));
        if (centroid3) d2h(c, centroid3, s->centroid, s->n_clusters * 3 * sizeof(double));
    });
}

int ltm_clusters_extract(ltm_ctx* c, ltm_clusters* h, ltm_cloud hcloud, ltm_scanset* out)
{
    return guarded(c, [&] {
        const ltm_clusters* s = c->open.clusters.get(h);
        LTM_REQUIRE(out, "null argument");
        const Cloud cloud = get_cloud(c, hcloud);
        LTM_REQUIRE(cloud.n == s->n_target, "the cloud is not the one the index was built over (point counts differ)");
        std::vector<uint64_t> off(s->n_clusters + 1, 0);
        d2h(c, off.data(), s->offsets, off.size() * 8);
        if (off.back() != s->n_points) throw Err{LTM_E_DEVICE, "cluster offsets do not end at the point count"};
        float4* d = reinterpret_cast<float4*>(c->pool.alloc(std::max<size_t>(s->n_points, 1) * sizeof(float4)));
        try {
            LTM_HIP(gather_points(cloud.d, reinterpret_cast<const uint32_t*>(s->idx), s->n_points, d, c->stream));
            *out = new_scanset(c, d, std::move(off));
        } catch (...) {
            c->pool.free(d);
            throw;
        }
    });
}

int ltm_clusters_free(ltm_ctx* c, ltm_clusters* h)
{
    return guarded(c, [&] { c->open.clusters.free(h); });
}

int ltm_debug_cluster_stats(ltm_ctx* c, uint64_t* stats, int reset)
{
    return guarded(c, [&] {
        if (stats) for (int i = 0; i < 6; ++i) stats[i] = c->cluster_stats[i];
        if (reset) for (int i = 0; i < 6; ++i) c->cluster_stats[i] = 0;
    });
}

} // extern "C"
