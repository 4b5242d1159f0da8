// DeviceEuclideanClusterExtraction.h -- stands in for a pcl::EuclideanClusterExtraction<PointType> over the clusters section of the C ABI (include/ltm.h,
// "clusters").  The reference extracts no clusters; this is for users of the change maps (nd_map, pd_map, scans_pd...) who want objects instead of points.
// Header-only: the host sources the build lists stay as they are.  It keeps EuclideanClusterExtraction's user-side names (setClusterTolerance,
// setMinClusterSize, setMaxClusterSize, setInputCloud, extract).  Semantics are those of include/ltm.h: clusters by size descending, ties to the cluster
// with the lower first point; inside a cluster the indices ascend (PCL lists them in its breadth-first order).
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
#pragma once
#include <climits>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

struct PointIndices { std::vector<int> indices; };      // pcl::PointIndices without its header

class DeviceEuclideanClusterExtraction
{
public:
    explicit DeviceEuclideanClusterExtraction(ltm_ctx* ctx) : ctx_(ctx) {}
    ~DeviceEuclideanClusterExtraction() { reset(); }
    DeviceEuclideanClusterExtraction(const DeviceEuclideanClusterExtraction&) = delete;
    DeviceEuclideanClusterExtraction& operator=(const DeviceEuclideanClusterExtraction&) = delete;

    void setClusterTolerance(double tolerance) { tolerance_ = tolerance; }
    double getClusterTolerance() const { return tolerance_; }
    void setMinClusterSize(int n) { min_size_ = n; }
    int getMinClusterSize() const { return min_size_; }
    void setMaxClusterSize(int n) { max_size_ = n; }      // INT_MAX (PCL's default): no limit
    int getMaxClusterSize() const { return max_size_; }

    // pcl::PCLBase::setInputCloud: the search index over the cloud is built on the device (the cloud may go afterwards)
    void setInputCloud(const Cloud& cloud)
    {
        ltm_cloud h = 0;
        check(ltm_cloud_upload(ctx_, cloud.data(), cloud.size(), sizeof(PointType), &h));
        const int rc = build(h);
        ltm_cloud_free(ctx_, h);
        check(rc);
    }
    void setInputCloud(ltm_cloud cloud) { check(build(cloud)); }

    // pcl::EuclideanClusterExtraction::extract
    void extract(std::vector<PointIndices>& clusters)
    {
        if (!index_) throw std::logic_error("DeviceEuclideanClusterExtraction: setInputCloud has not been called");
        std::vector<std::vector<PointIndices>> all;
        std::vector<std::vector<int>> lab;
        run(&index_, 1, all, lab);
        clusters.swap(all[0]);
        labels_.swap(lab[0]);
    }
    // the cluster of every input point of the last extract, -1 = none
    const std::vector<int>& labels() const { return labels_; }

    // several clouds, ONE ltm_search_cluster: clusters[i] are the clusters of clouds[i] (labels, if given, likewise)
    void extract(const std::vector<const Cloud*>& clouds, std::vector<std::vector<PointIndices>>& clusters, std::vector<std::vector<int>>* labels = nullptr)
    {
        std::vector<ltm_search*> idx(clouds.size(), nullptr);
        try {
            for (size_t i = 0; i < clouds.size(); ++i) {
                ltm_cloud h = 0;
                check(ltm_cloud_upload(ctx_, clouds[i]->data(), clouds[i]->size(), sizeof(PointType), &h));
                const int rc = ltm_search_build(ctx_, h, &idx[i]);
                ltm_cloud_free(ctx_, h);
                check(rc);
            }
            std::vector<std::vector<int>> lab;
            run(idx.data(), idx.size(), clusters, lab);
            if (labels) labels->swap(lab);
        } catch (...) {
            for (ltm_search* s : idx) if (s) ltm_search_free(ctx_, s);
            throw;
        }
        for (ltm_search* s : idx) if (s) ltm_search_free(ctx_, s);
    }

private:
    void run(ltm_search* const* idx, size_t n, std::vector<std::vector<PointIndices>>& clusters, std::vector<std::vector<int>>& labels)
    {
        clusters.assign(n, std::vector<PointIndices>());
        labels.assign(n, std::vector<int>());
        if (!n) return;
        if (min_size_ < 1 || max_size_ < min_size_) throw std::runtime_error("DeviceEuclideanClusterExtraction: need 1 <= min size <= max size");
        ltm_cluster_params p;
        ltm_cluster_default_params(&p);
        p.tolerance = tolerance_;
        p.min_size = (uint32_t)min_size_;
        p.max_size = max_size_ == INT_MAX ? 0u : (uint32_t)max_size_;
        std::vector<ltm_clusters*> sets(n, nullptr);
        check(ltm_search_cluster(ctx_, n, idx, &p, sets.data()));
        try {
            for (size_t i = 0; i < n; ++i) {
                size_t nt = 0, nc = 0, np = 0;
                check(ltm_clusters_info(ctx_, sets[i], &nt, &nc, &np));
                const int32_t* d_labels = nullptr; const uint64_t* d_off = nullptr; const int32_t* d_idx = nullptr;
                check(ltm_clusters_device(ctx_, sets[i], &d_labels, &d_off, &d_idx));
                static_assert(sizeof(int) == sizeof(int32_t), "indices are int32");
                labels[i].resize(nt);
                std::vector<uint64_t> off(nc + 1, 0);
                std::vector<int> flat(np);
                if (nt) check(ltm_buffer_copy(ctx_, labels[i].data(), d_labels, nt * sizeof(int32_t), 1));
                check(ltm_buffer_copy(ctx_, off.data(), d_off, off.size() * sizeof(uint64_t), 1));
                if (np) check(ltm_buffer_copy(ctx_, flat.data(), d_idx, np * sizeof(int32_t), 1));
                clusters[i].resize(nc);
                for (size_t c = 0; c < nc; ++c) clusters[i][c].indices.assign(flat.begin() + (ptrdiff_t)off[c], flat.begin() + (ptrdiff_t)off[c + 1]);
            }
        } catch (...) {
            for (ltm_clusters* s : sets) if (s) ltm_clusters_free(ctx_, s);
            throw;
        }
        for (ltm_clusters* s : sets) if (s) ltm_clusters_free(ctx_, s);
    }
    int build(ltm_cloud h)
    {
        reset();
        return ltm_search_build(ctx_, h, &index_);
    }
    void reset()
    {
        if (index_) ltm_search_free(ctx_, index_);
        index_ = nullptr;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceEuclideanClusterExtraction: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_search* index_ = nullptr;
    double tolerance_ = 0.0;      // PCL's default: must be set
    int min_size_ = 1;
    int max_size_ = INT_MAX;
    std::vector<int> labels_;
};

} // namespace ltremovert
