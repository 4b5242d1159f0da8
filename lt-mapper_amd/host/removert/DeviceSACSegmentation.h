// DeviceSACSegmentation.h -- stands in for a pcl::SACSegmentation<PointType> over the planes section of the C ABI (include/ltm.h, "planes"): RANSAC plane
// segmentation, the step that takes the ground out of a scan before DeviceEuclideanClusterExtraction.  The reference segments no planes.
// Header-only: the host sources the build lists stay as they are.  It keeps SACSegmentation's user-side names (setModelType, setMethodType,
// setDistanceThreshold, setMaxIterations, setAxis, setEpsAngle, setOptimizeCoefficients, setInputCloud, segment).  Semantics are those of include/ltm.h:
// all iterations are evaluated, the draws are seeded (setSeed), the coefficients carry a canonical sign; inlier indices ascend.
// Every member reports a failure by throwing (std::invalid_argument for a model or method this class does not have, std::runtime_error with the context's
// message, std::logic_error for a call out of order).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/DeviceEuclideanClusterExtraction.h"      // PointIndices
#include "removert/utility.h"

namespace ltremovert
{

struct ModelCoefficients { std::vector<float> values; };      // pcl::ModelCoefficients without its header: a, b, c, d; empty = no plane

// PCL's enumerators, with PCL's values (model_types.h, method_types.h)
enum SacModel { SACMODEL_PLANE = 0, SACMODEL_PERPENDICULAR_PLANE = 11 };
enum SacMethod { SAC_RANSAC = 0 };

class DeviceSACSegmentation
{
public:
    explicit DeviceSACSegmentation(ltm_ctx* ctx) : ctx_(ctx) { ltm_plane_default_params(&p_); }

    void setModelType(int model)
    {
        if (model != SACMODEL_PLANE && model != SACMODEL_PERPENDICULAR_PLANE)
            throw std::invalid_argument("DeviceSACSegmentation: only SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE");
        model_ = model;
    }
    int getModelType() const { return model_; }
    void setMethodType(int method)
    {
        if (method != SAC_RANSAC) throw std::invalid_argument("DeviceSACSegmentation: only SAC_RANSAC");
    }
    int getMethodType() const { return SAC_RANSAC; }
    void setDistanceThreshold(double thr) { p_.distance_threshold = thr; }
    double getDistanceThreshold() const { return p_.distance_threshold; }
    void setMaxIterations(int n) { p_.max_iterations = n < 0 ? 0u : (uint32_t)n; }
    int getMaxIterations() const { return (int)p_.max_iterations; }
    void setAxis(double x, double y, double z) { axis_[0] = x; axis_[1] = y; axis_[2] = z; }      // used by SACMODEL_PERPENDICULAR_PLANE only, as in PCL
    void setEpsAngle(double rad) { p_.eps_angle = rad; }
    double getEpsAngle() const { return p_.eps_angle; }
    void setOptimizeCoefficients(bool on) { p_.refine = on ? 1 : 0; }
    bool getOptimizeCoefficients() const { return p_.refine != 0; }
    void setSeed(uint32_t seed) { p_.seed = seed; }

    void setInputCloud(const Cloud& cloud) { input_ = &cloud; }      // borrowed until segment, as PCL's shared pointer would be

    // pcl::SACSegmentation::segment: the inliers of the plane (empty: none found) and its four coefficients
    void segment(PointIndices& inliers, ModelCoefficients& coefficients)
    {
        if (!input_) throw std::logic_error("DeviceSACSegmentation: setInputCloud has not been called");
        std::vector<PointIndices> in;
        std::vector<ModelCoefficients> co;
        segment({input_}, in, co);
        inliers.indices.swap(in[0].indices);
        coefficients.values.swap(co[0].values);
    }

    // several clouds, ONE ltm_scanset_segment_planes: inliers[i] and coefficients[i] belong to clouds[i]
    void segment(const std::vector<const Cloud*>& clouds, std::vector<PointIndices>& inliers, std::vector<ModelCoefficients>& coefficients)
    {
        const size_t n = clouds.size();
        inliers.assign(n, PointIndices());
        coefficients.assign(n, ModelCoefficients());
        if (!n) return;
        ltm_plane_params p = p_;
        const bool perpendicular = model_ == SACMODEL_PERPENDICULAR_PLANE;
        for (int d = 0; d < 3; ++d) p.axis[d] = perpendicular ? axis_[d] : 0.0;
        if (!perpendicular) p.eps_angle = 0.0;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + clouds[i]->size();
        std::vector<PointType> all;
        all.reserve((size_t)off[n] + 1);
        for (size_t i = 0; i < n; ++i) all.insert(all.end(), clouds[i]->begin(), clouds[i]->end());
        ltm_scanset scans = 0;
        ltm_planes* planes = nullptr;
        try {
            check(ltm_scanset_upload(ctx_, all.data(), sizeof(PointType), off.data(), n, &scans));
            check(ltm_scanset_segment_planes(ctx_, scans, 0, n, &p, &planes));
            std::vector<uint8_t> found(n), labels((size_t)off[n] + 1);
            std::vector<double> coeff(4 * n);
            check(ltm_planes_download(ctx_, planes, found.data(), nullptr, nullptr, nullptr, nullptr, nullptr, coeff.data(), nullptr, labels.data(), nullptr,
                                      nullptr));
            for (size_t i = 0; i < n; ++i) {
                if (!found[i]) continue;
                for (int d = 0; d < 4; ++d) coefficients[i].values.push_back((float)coeff[4 * i + (size_t)d]);
                for (uint64_t j = off[i]; j < off[i + 1]; ++j)
                    if (labels[(size_t)j]) inliers[i].indices.push_back((int)(j - off[i]));
            }
        } catch (...) {
            if (planes) ltm_planes_free(ctx_, planes);
            if (scans) ltm_scanset_free(ctx_, scans);
            throw;
        }
        ltm_planes_free(ctx_, planes);
        ltm_scanset_free(ctx_, scans);
    }

private:
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceSACSegmentation: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_plane_params p_;
    int model_ = SACMODEL_PLANE;
    double axis_[3] = {0.0, 0.0, 0.0};
    const Cloud* input_ = nullptr;
};

} // namespace ltremovert
