// DeviceKdTree.h -- stands in for a pcl::KdTreeFLANN<PointType> member of the reference's Session (ltremovert/src/Session.cpp:18-23; setInputCloud at
// :404, :457, :489; nearestKSearch at :471, :592, :627) over the search index of the C ABI (include/ltm.h, "search index").  Header-only: the host
// sources the build lists stay as they are.  Semantics are those of include/ltm.h: L2_Simple squared distances in float, ascending, ties by the
// smaller target index; non-finite target points are never returned.  A swap for a KdTreeFLANN member is shown in INTEGRATION.md.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

class DeviceKdTree
{
public:
    explicit DeviceKdTree(ltm_ctx* ctx) : ctx_(ctx) {}
    ~DeviceKdTree() { reset(); }
    DeviceKdTree(const DeviceKdTree&) = delete;
    DeviceKdTree& operator=(const DeviceKdTree&) = delete;

    // pcl::KdTreeFLANN::setInputCloud: the index keeps its own copy, `cloud` may go afterwards
    void setInputCloud(const Cloud& cloud)
    {
        ltm_cloud h = 0;
        check(ltm_cloud_upload(ctx_, cloud.data(), cloud.size(), sizeof(PointType), &h));
        const int rc = build(h);
        ltm_cloud_free(ctx_, h);
        check(rc);
    }
    // the same for a cloud that is on the device already (a map handle of the Session mirror)
    void setInputCloud(ltm_cloud cloud) { check(build(cloud)); }

    // pcl::KdTreeFLANN::nearestKSearch: returns the number of neighbours found (k clamped to the target size; 0 for a non-finite query)
    int nearestKSearch(const PointType& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const
    {
        std::vector<std::vector<int>> ii;
        std::vector<std::vector<float>> dd;
        nearestKSearch(Cloud{point}, k, ii, dd);
        k_indices.swap(ii[0]);
        k_sqr_distances.swap(dd[0]);
        return (int)k_indices.size();
    }
    // batched: one row per query point (one device call for the whole cloud)
    void nearestKSearch(const Cloud& queries, int k, std::vector<std::vector<int>>& k_indices, std::vector<std::vector<float>>& k_sqr_distances) const
    {
        require_index();
        const size_t n = queries.size(), cells = n * (size_t)(k > 0 ? k : 0);
        k_indices.assign(n, {});
        k_sqr_distances.assign(n, {});
        if (!n) return;
        if (k < 1 || k > 64) throw std::invalid_argument("DeviceKdTree::nearestKSearch: k must be in [1, 64]");
        ltm_cloud q = upload(queries);
        void *di = nullptr, *dd = nullptr;
        int rc = ltm_buffer_alloc(ctx_, cells * 4, &di);
        if (rc == LTM_OK) rc = ltm_buffer_alloc(ctx_, cells * 4, &dd);
        if (rc == LTM_OK) rc = ltm_knn_search(ctx_, index_, q, k, static_cast<int32_t*>(di), static_cast<float*>(dd));
        std::vector<int32_t> hi(cells);
        std::vector<float> hd(cells);
        if (rc == LTM_OK) rc = ltm_buffer_copy(ctx_, hi.data(), di, cells * 4, 1);
        if (rc == LTM_OK) rc = ltm_buffer_copy(ctx_, hd.data(), dd, cells * 4, 1);
        if (dd) ltm_buffer_free(ctx_, dd);
        if (di) ltm_buffer_free(ctx_, di);
        ltm_cloud_free(ctx_, q);
        check(rc);
        for (size_t i = 0; i < n; ++i)
            for (int j = 0; j < k && hi[i * k + j] >= 0; ++j) { k_indices[i].push_back(hi[i * k + j]); k_sqr_distances[i].push_back(hd[i * k + j]); }
    }

    // pcl::KdTreeFLANN::radiusSearch (sorted results; max_nn = 0: no limit): returns the number of neighbours found
    int radiusSearch(const PointType& point, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, unsigned int max_nn = 0) const
    {
        std::vector<std::vector<int>> ii;
        std::vector<std::vector<float>> dd;
        radiusSearch(Cloud{point}, radius, ii, dd, max_nn);
        k_indices.swap(ii[0]);
        k_sqr_distances.swap(dd[0]);
        return (int)k_indices.size();
    }
    void radiusSearch(const Cloud& queries, double radius, std::vector<std::vector<int>>& k_indices, std::vector<std::vector<float>>& k_sqr_distances,
                      unsigned int max_nn = 0) const
    {
        require_index();
        const size_t n = queries.size();
        k_indices.assign(n, {});
        k_sqr_distances.assign(n, {});
        if (!n) return;
        ltm_cloud q = upload(queries);
        ltm_search_result* r = nullptr;
        int rc = ltm_radius_search(ctx_, index_, q, (float)radius, (int)max_nn, &r);
        size_t nq = 0, total = 0;
        const uint64_t* off = nullptr;
        const int32_t* idx = nullptr;
        const float* d2 = nullptr;
        if (rc == LTM_OK) rc = ltm_search_result_info(ctx_, r, &nq, &total, &off, &idx, &d2);
        std::vector<uint64_t> ho(n + 1);
        std::vector<int32_t> hi(total);
        std::vector<float> hd(total);
        if (rc == LTM_OK) rc = ltm_buffer_copy(ctx_, ho.data(), off, (n + 1) * 8, 1);
        if (rc == LTM_OK && total) rc = ltm_buffer_copy(ctx_, hi.data(), idx, total * 4, 1);
        if (rc == LTM_OK && total) rc = ltm_buffer_copy(ctx_, hd.data(), d2, total * 4, 1);
        if (r) ltm_search_result_free(ctx_, r);
        ltm_cloud_free(ctx_, q);
        check(rc);
        for (size_t i = 0; i < n; ++i) {
            k_indices[i].assign(hi.begin() + (long)ho[i], hi.begin() + (long)ho[i + 1]);
            k_sqr_distances[i].assign(hd.begin() + (long)ho[i], hd.begin() + (long)ho[i + 1]);
        }
    }

    ltm_search* handle() const { return index_; }

private:
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
    void require_index() const
    {
        if (!index_) throw std::logic_error("DeviceKdTree: setInputCloud has not been called");
    }
    ltm_cloud upload(const Cloud& pts) const
    {
        ltm_cloud h = 0;
        check(ltm_cloud_upload(ctx_, pts.data(), pts.size(), sizeof(PointType), &h));
        return h;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceKdTree: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_search* index_ = nullptr;
};

} // namespace ltremovert
