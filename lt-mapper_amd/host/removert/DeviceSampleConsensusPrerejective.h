// DeviceSampleConsensusPrerejective.h -- stands in for pcl::SampleConsensusPrerejective<PointType, PointType, pcl::FPFHSignature33> over the matches and the
// initial alignment of the C ABI (include/ltm.h, "fpfh matches" and "initial alignment"): the coarse alignment of a loop pair from its descriptors, whose
// transform ICP then refines (DeviceICP.h takes it as its guess).  The reference aligns no pair from descriptors.
// Header-only: the host sources the build lists stay as they are.  The class keeps PCL's user-side names (setInputSource, setInputTarget, setSourceFeatures,
// setTargetFeatures, setMaximumIterations, setNumberOfSamples, setCorrespondenceRandomness, setSimilarityThreshold, setMaxCorrespondenceDistance,
// setInlierFraction, align, hasConverged, getFinalTransformation).  The features are rows of 33 floats, one per input point in input order -- what
// DeviceFPFHEstimation::compute returns, or any other 33-float descriptor.  Semantics are those of include/ltm.h: three samples, all hypotheses
// evaluated, no redraw; align() does not transform a cloud, it finds the transform.
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

class DeviceSampleConsensusPrerejective
{
public:
    static constexpr int kDescriptorSize = 33;      // pcl::FPFHSignature33

    explicit DeviceSampleConsensusPrerejective(ltm_ctx* ctx) : ctx_(ctx) { ltm_sac_default_params(&params_); }

    void setInputSource(const Cloud& cloud) { source_ = &cloud; }      // borrowed until align, as PCL's shared pointers would be
    void setInputTarget(const Cloud& cloud) { target_ = &cloud; }
    void setSourceFeatures(const std::vector<float>& rows) { source_rows_ = &rows; }
    void setTargetFeatures(const std::vector<float>& rows) { target_rows_ = &rows; }
    void setMaximumIterations(int n) { params_.max_iterations = n < 0 ? 0u : (uint32_t)n; }
    void setNumberOfSamples(int n)
    {
        if (n != 3) throw std::logic_error("DeviceSampleConsensusPrerejective: the number of samples is 3");
    }
    void setCorrespondenceRandomness(int k) { kc_ = k; }
    void setSimilarityThreshold(float thr) { params_.similarity_threshold = thr; }
    void setMaxCorrespondenceDistance(double d) { params_.inlier_distance = d; }
    void setInlierFraction(float f) { params_.inlier_fraction = f; }
    void setSeed(uint32_t seed) { params_.seed = seed; }               // additions of this library
    void setEvaluationStride(uint32_t stride) { params_.eval_stride = stride; }
    int getCorrespondenceRandomness() const { return kc_; }
    int getMaximumIterations() const { return (int)params_.max_iterations; }

    // pcl::Registration::align without the output cloud: afterwards hasConverged() and getFinalTransformation()
    void align()
    {
        if (!source_ || !target_) throw std::logic_error("DeviceSampleConsensusPrerejective: setInputSource and setInputTarget have not both been called");
        if (!source_rows_ || !target_rows_) throw std::logic_error("DeviceSampleConsensusPrerejective: setSourceFeatures and setTargetFeatures have not both been called");
        if (source_rows_->size() != source_->size() * kDescriptorSize || target_rows_->size() != target_->size() * kDescriptorSize)
            throw std::logic_error("DeviceSampleConsensusPrerejective: the features are not 33 floats per input point");
        converged_ = false;
        consensus_ = 0;
        Handles h;
        try {
            h.index[0] = build(*target_, &h.cloud[0]);
            h.index[1] = build(*source_, &h.cloud[1]);
            const uint64_t toff[2] = {0, target_->size()}, soff[2] = {0, source_->size()};
            check(ltm_fpfh_upload(ctx_, 1, toff, target_rows_->data(), &h.rows[0]));
            check(ltm_fpfh_upload(ctx_, 1, soff, source_rows_->data(), &h.rows[1]));
            const uint32_t rec = 0;
            check(ltm_fpfh_match(ctx_, 1, h.rows[0], &rec, h.rows[1], &rec, kc_, &h.matches));
            check(ltm_sac_align(ctx_, 1, &h.index[0], &h.index[1], h.matches, &params_, &h.sac));
            uint8_t found = 0;
            check(ltm_sac_download(ctx_, h.sac, &found, nullptr, &consensus_, nullptr, nullptr, nullptr, T_, nullptr, nullptr));
            converged_ = found != 0;
        } catch (...) {
            release(h);
            throw;
        }
        release(h);
    }
    bool hasConverged() const { return converged_; }
    uint32_t getConsensus() const { return consensus_; }
    const double* getFinalTransformation() const { return T_; }      // 16 doubles, row-major, source -> target; NaN where no hypothesis was valid

private:
    struct Handles {
        ltm_cloud cloud[2] = {0, 0};
        ltm_search* index[2] = {nullptr, nullptr};
        ltm_fpfh* rows[2] = {nullptr, nullptr};
        ltm_matches* matches = nullptr;
        ltm_sac* sac = nullptr;
    };
    ltm_search* build(const Cloud& cloud, ltm_cloud* h)
    {
        ltm_search* index = nullptr;
        check(ltm_cloud_upload(ctx_, cloud.data(), cloud.size(), sizeof(PointType), h));
        check(ltm_search_build(ctx_, *h, &index));
        return index;
    }
    void release(Handles& h)
    {
        if (h.sac) ltm_sac_free(ctx_, h.sac);
        if (h.matches) ltm_matches_free(ctx_, h.matches);
        for (int i = 0; i < 2; ++i) {
            if (h.rows[i]) ltm_fpfh_free(ctx_, h.rows[i]);
            if (h.index[i]) ltm_search_free(ctx_, h.index[i]);
            if (h.cloud[i]) ltm_cloud_free(ctx_, h.cloud[i]);
        }
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceSampleConsensusPrerejective: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    const Cloud* source_ = nullptr;
    const Cloud* target_ = nullptr;
    const std::vector<float>* source_rows_ = nullptr;
    const std::vector<float>* target_rows_ = nullptr;
    ltm_sac_params params_;
    int kc_ = 2;                     // PCL's default correspondence randomness
    bool converged_ = false;
    uint32_t consensus_ = 0;
    double T_[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

} // namespace ltremovert
