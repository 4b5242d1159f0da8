// DeviceNormalEstimation.h -- stands in for a pcl::NormalEstimation<PointType, pcl::Normal> over the normals section of the C ABI (include/ltm.h,
// "normals").  The reference estimates no normals; this is for users of the search index and of point-to-plane ICP (DeviceICP.h).  Header-only: the
// host sources the build lists stay as they are.  It keeps NormalEstimation's user-side names (setInputCloud, setKSearch, setViewPoint, compute).
// Semantics are those of include/ltm.h: the k nearest points the point itself included, covariance in double about the point, canonical sign, then the
// flip towards the viewpoint; NaN for non-finite points and for clouds of fewer than three finite points.
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

struct Normal { float normal_x, normal_y, normal_z, curvature; };      // pcl::Normal's named fields
using NormalCloud = std::vector<Normal>;

class DeviceNormalEstimation
{
public:
    explicit DeviceNormalEstimation(ltm_ctx* ctx) : ctx_(ctx) {}
    ~DeviceNormalEstimation() { reset(); }
    DeviceNormalEstimation(const DeviceNormalEstimation&) = delete;
    DeviceNormalEstimation& operator=(const DeviceNormalEstimation&) = delete;

    // pcl::Feature::setInputCloud: the search index over the cloud is built on the device (the cloud may go afterwards)
    void setInputCloud(const Cloud& cloud)
    {
        ltm_cloud h = 0;
        check(ltm_cloud_upload(ctx_, cloud.data(), cloud.size(), sizeof(PointType), &h));
        const int rc = build(h);
        ltm_cloud_free(ctx_, h);
        check(rc);
    }
    void setInputCloud(ltm_cloud cloud) { check(build(cloud)); }
    // an index somebody else owns (a DeviceICP's target, an index of ltm_search_build_scanset): the normals are left with it
    void setSearchIndex(ltm_search* index) { reset(); index_ = index; owned_ = false; }

    void setKSearch(int k) { k_ = k; }
    int getKSearch() const { return k_; }
    void setViewPoint(float vx, float vy, float vz) { vp_[0] = vx; vp_[1] = vy; vp_[2] = vz; }
    void getViewPoint(float& vx, float& vy, float& vz) const { vx = vp_[0]; vy = vp_[1]; vz = vp_[2]; }

    // pcl::Feature::compute: one normal per input point, in the input's order
    void compute(NormalCloud& output)
    {
        if (!index_) throw std::logic_error("DeviceNormalEstimation: setInputCloud has not been called");
        check(ltm_search_estimate_normals(ctx_, 1, &index_, k_, vp_));
        size_t n = 0;
        check(ltm_search_info(ctx_, index_, &n, nullptr));
        output.resize(n);
        static_assert(sizeof(Normal) == 4 * sizeof(float), "Normal must be four packed floats");
        check(ltm_search_normals_download(ctx_, index_, n ? &output[0].normal_x : nullptr));
    }
    ltm_search* index() const { return index_; }

private:
    int build(ltm_cloud h)
    {
        reset();
        owned_ = true;
        return ltm_search_build(ctx_, h, &index_);
    }
    void reset()
    {
        if (index_ && owned_) ltm_search_free(ctx_, index_);
        index_ = nullptr;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceNormalEstimation: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_search* index_ = nullptr;
    bool owned_ = false;
    int k_ = 10;
    float vp_[3] = {0.0f, 0.0f, 0.0f};
};

} // namespace ltremovert
