// DeviceFPFHEstimation.h -- stands in for pcl::FPFHEstimation<PointType, pcl::Normal, pcl::FPFHSignature33> over the descriptors of the C ABI
// (include/ltm.h, "fpfh"): the local shape descriptor that feature correspondences and a coarse alignment of a loop pair start from.  The reference
// computes no descriptors.
// Header-only: the host sources the build lists stay as they are.  The class keeps PCL's user-side names (setInputCloud, setInputNormals, setKSearch,
// compute).  The normals live with the search index on the device, so setInputNormals takes no cloud of normals: it means "estimate them on the index", with
// the k and the viewpoint of pcl::NormalEstimation.  setSearchIndex takes an index the caller built (and keeps): its normals are used as they are unless
// setInputNormals was called.  Semantics are those of include/ltm.h: rows in input order, NaN rows for points with a non-finite coordinate.
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

class DeviceFPFHEstimation
{
public:
    static constexpr int kDescriptorSize = 33;      // pcl::FPFHSignature33

    explicit DeviceFPFHEstimation(ltm_ctx* ctx) : ctx_(ctx) {}

    void setInputCloud(const Cloud& cloud) { input_ = &cloud; index_ = nullptr; }      // borrowed until compute, as PCL's shared pointer would be
    void setSearchIndex(ltm_search* index) { index_ = index; input_ = nullptr; }       // borrowed: the caller frees it
    // estimate the normals on the index before the descriptors: setKSearch and setViewPoint of pcl::NormalEstimation
    void setInputNormals(int k_normals = 10, float vx = 0.0f, float vy = 0.0f, float vz = 0.0f)
    {
        normals_k_ = k_normals;
        viewpoint_[0] = vx; viewpoint_[1] = vy; viewpoint_[2] = vz;
    }
    void setKSearch(int k) { k_ = k; }
    int getKSearch() const { return k_; }
    int getNormalsK() const { return normals_k_; }

    // pcl::Feature::compute: descriptors[33 i .. 33 i + 32] is the histogram of input point i
    void compute(std::vector<float>& descriptors)
    {
        if (!input_ && !index_) throw std::logic_error("DeviceFPFHEstimation: neither setInputCloud nor setSearchIndex has been called");
        if (k_ <= 0) throw std::logic_error("DeviceFPFHEstimation: setKSearch has not been called");
        if (input_ && normals_k_ <= 0) throw std::logic_error("DeviceFPFHEstimation: setInputNormals has not been called");
        ltm_search* own = nullptr;
        ltm_fpfh* set = nullptr;
        try {
            ltm_search* index = index_;
            if (!index) {
                ltm_cloud h = 0;
                check(ltm_cloud_upload(ctx_, input_->data(), input_->size(), sizeof(PointType), &h));
                const int rc = ltm_search_build(ctx_, h, &own);
                ltm_cloud_free(ctx_, h);
                check(rc);
                index = own;
            }
            if (normals_k_ > 0) check(ltm_search_estimate_normals(ctx_, 1, &index, normals_k_, viewpoint_));
            check(ltm_search_fpfh(ctx_, 1, &index, k_, &set));
            size_t n = 0;
            check(ltm_fpfh_info(ctx_, set, nullptr, &n, nullptr));
            descriptors.assign(n * kDescriptorSize + 1, 0.0f);
            check(ltm_fpfh_download(ctx_, set, nullptr, nullptr, descriptors.data(), nullptr));
            descriptors.resize(n * kDescriptorSize);
        } catch (...) {
            release(own, set);
            throw;
        }
        release(own, set);
    }

private:
    void release(ltm_search* own, ltm_fpfh* set)
    {
        if (set) ltm_fpfh_free(ctx_, set);
        if (own) ltm_search_free(ctx_, own);
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceFPFHEstimation: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    const Cloud* input_ = nullptr;
    ltm_search* index_ = nullptr;
    int k_ = 0;
    int normals_k_ = 0;
    float viewpoint_[3] = {0.0f, 0.0f, 0.0f};
};

} // namespace ltremovert
