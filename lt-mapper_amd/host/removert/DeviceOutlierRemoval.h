// DeviceOutlierRemoval.h -- stands in for pcl::StatisticalOutlierRemoval<PointType> and pcl::RadiusOutlierRemoval<PointType> over the outlier filters of the
// C ABI (include/ltm.h, "outlier filters"): the filters that take isolated speckle out of a change map before DeviceEuclideanClusterExtraction and stray
// returns out of a scan before normals, ICP or DeviceSACSegmentation.  The reference filters no outliers.
// Header-only: the host sources the build lists stay as they are.  The classes keep PCL's user-side names (setMeanK, setStddevMulThresh, setRadiusSearch,
// setMinNeighborsInRadius, setInputCloud, filter).  Semantics are those of include/ltm.h: points with a non-finite coordinate are removed, the kept points
// stay in input order; getRemovedIndices() lists the others (PCL's extract_removed_indices_).
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

// what the two filters share: the clouds go up, one search index each, ONE filter call, the labels come down
class DeviceOutlierRemovalBase
{
public:
    void setInputCloud(const Cloud& cloud) { input_ = &cloud; }      // borrowed until filter, as PCL's shared pointer would be

    // pcl::Filter::filter: the kept points of the input cloud, in input order
    void filter(Cloud& output)
    {
        if (!input_) throw std::logic_error(name_ + ": setInputCloud has not been called");
        std::vector<Cloud> out;
        std::vector<std::vector<int>> removed;
        filter({input_}, out, &removed);
        output.swap(out[0]);
        removed_.swap(removed[0]);
    }
    // the input positions the last filter(Cloud&) removed, ascending
    const std::vector<int>& getRemovedIndices() const { return removed_; }

    // several clouds, ONE filter call: outputs[i] are the kept points of clouds[i] (removed, if given, the positions taken out of it)
    void filter(const std::vector<const Cloud*>& clouds, std::vector<Cloud>& outputs, std::vector<std::vector<int>>* removed = nullptr)
    {
        const size_t n = clouds.size();
        outputs.assign(n, Cloud());
        if (removed) removed->assign(n, std::vector<int>());
        if (!n) return;
        std::vector<ltm_search*> idx(n, nullptr);
        ltm_outliers* set = nullptr;
        try {
            size_t total = 0;
            for (size_t i = 0; i < n; ++i) {
                ltm_cloud h = 0;
                check(ltm_cloud_upload(ctx_, clouds[i]->data(), clouds[i]->size(), sizeof(PointType), &h));
                const int rc = ltm_search_build(ctx_, h, &idx[i]);
                ltm_cloud_free(ctx_, h);
                check(rc);
                total += clouds[i]->size();
            }
            check(run(n, idx.data(), &set));
            std::vector<uint8_t> labels(total + 1);
            check(ltm_outliers_download(ctx_, set, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, labels.data(), nullptr, nullptr));
            size_t at = 0;
            for (size_t i = 0; i < n; ++i) {
                const Cloud& in = *clouds[i];
                for (size_t j = 0; j < in.size(); ++j, ++at) {
                    if (labels[at]) outputs[i].push_back(in[j]);
                    else if (removed) (*removed)[i].push_back((int)j);
                }
            }
        } catch (...) {
            release(idx, set);
            throw;
        }
        release(idx, set);
    }

protected:
    DeviceOutlierRemovalBase(ltm_ctx* ctx, const char* name) : ctx_(ctx), name_(name) {}
    ~DeviceOutlierRemovalBase() = default;
    virtual int run(size_t n, ltm_search* const* idx, ltm_outliers** out) = 0;

    ltm_ctx* ctx_;

private:
    void release(std::vector<ltm_search*>& idx, ltm_outliers* set)
    {
        if (set) ltm_outliers_free(ctx_, set);
        for (ltm_search* s : idx) if (s) ltm_search_free(ctx_, s);
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(name_ + ": " + ltm_last_error(ctx_));
    }

    std::string name_;
    const Cloud* input_ = nullptr;
    std::vector<int> removed_;
};

class DeviceStatisticalOutlierRemoval : public DeviceOutlierRemovalBase
{
public:
    explicit DeviceStatisticalOutlierRemoval(ltm_ctx* ctx) : DeviceOutlierRemovalBase(ctx, "DeviceStatisticalOutlierRemoval") { ltm_sor_default_params(&p_); }
    void setMeanK(int k) { p_.mean_k = k < 0 ? 0u : (uint32_t)k; }
    int getMeanK() const { return (int)p_.mean_k; }
    void setStddevMulThresh(double mul) { p_.stddev_mul = mul; }
    double getStddevMulThresh() const { return p_.stddev_mul; }

private:
    int run(size_t n, ltm_search* const* idx, ltm_outliers** out) override { return ltm_search_filter_statistical(ctx_, n, idx, &p_, out); }
    ltm_sor_params p_;
};

class DeviceRadiusOutlierRemoval : public DeviceOutlierRemovalBase
{
public:
    explicit DeviceRadiusOutlierRemoval(ltm_ctx* ctx) : DeviceOutlierRemovalBase(ctx, "DeviceRadiusOutlierRemoval") { ltm_ror_default_params(&p_); }
    void setRadiusSearch(double radius) { p_.radius = radius; }
    double getRadiusSearch() const { return p_.radius; }
    void setMinNeighborsInRadius(int n) { p_.min_neighbors = n < 0 ? 0u : (uint32_t)n; }
    int getMinNeighborsInRadius() const { return (int)p_.min_neighbors; }

private:
    int run(size_t n, ltm_search* const* idx, ltm_outliers** out) override { return ltm_search_filter_radius(ctx_, n, idx, &p_, out); }
    ltm_ror_params p_;
};

} // namespace ltremovert
