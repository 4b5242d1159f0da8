// DeviceICP.h -- stands in for the pcl::IterativeClosestPoint<PointType, PointType> of the reference's LTslam::doICPVirtualRelative / doICPGlobalRelative
// (ltslam/src/LTslam.cpp:187-301) over the ICP section of the C ABI (include/ltm.h, "icp").  Header-only: the host sources the build lists stay as they
// are.  It keeps IterativeClosestPoint's user-side names; a transform is a Matrix4d (16 doubles, row-major) where the reference has an Eigen::Matrix4f.
// Semantics are those of include/ltm.h -- PCL 1.10's arithmetic with the departures named there (the transform is kept in double and always applied to the
// original source).  setInputTarget builds a search index on the device, which align and alignAll reuse until the next setInputTarget: addSCloops'
// loop over many sources against one submap becomes ONE alignAll.  The swap for the member of LTslam is shown in INTEGRATION.md.
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::logic_error for a call out of order).
// setMethod(PointToPlane) switches to pcl::IterativeClosestPointWithNormals' error (include/ltm.h, "icp, point-to-plane"): the target's normals are then
// estimated on the device (setKSearch / setViewPoint as on pcl::NormalEstimation) before the first alignment against a target.
// setMethod(Generalized) switches to pcl::GeneralizedIterativeClosestPoint's plane-to-plane error (include/ltm.h, "icp, generalized"): every source gets a
// search index of its own, and the normals of both sides -- which stand for GICP's covariances -- are estimated on the device with
// setCorrespondenceRandomness(k) neighbours (20, PCL's k_correspondences_).  setRotationEpsilon is accepted and unused: the stop tests are those of "icp".
// Not here: the Euler / gtsam::Pose3 conversions of the result stay on the host as they are (the submaps: DeviceLoopSubmaps.h).
#pragma once
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

class DeviceICP
{
public:
    explicit DeviceICP(ltm_ctx* ctx) : ctx_(ctx) { ltm_icp_default_params(&params_); reset_result(); }
    ~DeviceICP() { reset_target(); }
    DeviceICP(const DeviceICP&) = delete;
    DeviceICP& operator=(const DeviceICP&) = delete;

    void setMaxCorrespondenceDistance(double d) { params_.max_corr_dist = d; }
    void setMaximumIterations(int n) { params_.max_iterations = n; }
    void setTransformationEpsilon(double e) { params_.transformation_epsilon = e; }
    void setEuclideanFitnessEpsilon(double e) { params_.euclidean_fitness_epsilon = e; }
    const ltm_icp_params& params() const { return params_; }

    enum Method { PointToPoint, PointToPlane, Generalized };
    void setMethod(Method m) { method_ = m; have_normals_ = false; }
    Method method() const { return method_; }
    // the normals of the point-to-plane method: neighbours and viewpoint of pcl::NormalEstimation
    void setKSearch(int k) { normal_k_ = k; have_normals_ = false; }
    void setViewPoint(float vx, float vy, float vz) { viewpoint_[0] = vx; viewpoint_[1] = vy; viewpoint_[2] = vz; have_normals_ = false; }

    // the generalized method, under pcl::GeneralizedIterativeClosestPoint's names: the neighbours of the covariances (here: of the normals of both sides),
    // gicp_epsilon_ (no setter in PCL 1.10; the constant of the regularised covariance), and the rotation epsilon, which this library does not use
    void setCorrespondenceRandomness(int k) { gicp_k_ = k; have_normals_ = false; }
    int getCorrespondenceRandomness() const { return gicp_k_; }
    void setGicpEpsilon(double e) { gicp_epsilon_ = e; }
    void setRotationEpsilon(double e) { rotation_epsilon_ = e; }      // kept for the caller, unused (include/ltm.h, "icp, generalized", DEPARTURES)
    double getRotationEpsilon() const { return rotation_epsilon_; }

    // pcl::Registration::setInputSource: the cloud is copied (the reference keeps a shared pointer)
    void setInputSource(const Cloud& source) { source_ = source; }
    // pcl::Registration::setInputTarget: the search index over the target, built on the device
    void setInputTarget(const Cloud& target)
    {
        ltm_cloud h = 0;
        check(ltm_cloud_upload(ctx_, target.data(), target.size(), sizeof(PointType), &h));
        const int rc = build(h);
        ltm_cloud_free(ctx_, h);
        check(rc);
    }
    // the same for a cloud that is on the device already (a map handle of the Session mirror)
    void setInputTarget(ltm_cloud target) { check(build(target)); }

    // pcl::Registration::align: `output` receives the source under the final transform (in float, as transformPointCloud gives it)
    void align(Cloud& output) { align(output, identity()); }
    void align(Cloud& output, const Matrix4d& guess)
    {
        result_ = run({&source_}, &guess)[0];
        output = source_;
        const double* T = result_.T;
        for (PointType& p : output) {
            const double x = p.x, y = p.y, z = p.z;
            p.x = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
            p.y = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
            p.z = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
        }
    }
    bool hasConverged() const { return result_.converged != 0; }
    double getFitnessScore() const { return result_.fitness; }
    Matrix4d getFinalTransformation() const { return Matrix4d(result_.T, result_.T + 16); }
    const ltm_icp_result& result() const { return result_; }

    // every source against the target in one batch (the loops of LTslam::addSCloops / addRSloops over one submap); guesses: none, or one per source
    std::vector<ltm_icp_result> alignAll(const std::vector<const Cloud*>& sources, const std::vector<Matrix4d>& guesses = {})
    {
        if (!guesses.empty() && guesses.size() != sources.size()) throw std::invalid_argument("DeviceICP::alignAll: one guess per source, or none");
        std::vector<double> flat;
        for (const Matrix4d& g : guesses) {
            if (g.size() != 16) throw std::invalid_argument("DeviceICP::alignAll: a guess is not 16 doubles");
            flat.insert(flat.end(), g.begin(), g.end());
        }
        return run(sources, nullptr, guesses.empty() ? nullptr : flat.data());
    }
    std::vector<ltm_icp_result> alignAll(std::initializer_list<const Cloud*> sources) { return alignAll(std::vector<const Cloud*>(sources)); }

    ltm_search* target() const { return index_; }

private:
    static Matrix4d identity()
    {
        Matrix4d m(16, 0.0);
        m[0] = m[5] = m[10] = m[15] = 1.0;
        return m;
    }
    std::vector<ltm_icp_result> run(const std::vector<const Cloud*>& sources, const Matrix4d* one_guess, const double* guesses = nullptr)
    {
        if (!index_) throw std::logic_error("DeviceICP: setInputTarget has not been called");
        if (one_guess && one_guess->size() != 16) throw std::invalid_argument("DeviceICP::align: the guess is not 16 doubles");
        const size_t n = sources.size();
        std::vector<ltm_icp_result> out(n);
        if (!n) return out;
        std::vector<ltm_cloud> h(n, 0);
        std::vector<ltm_search*> t(n, index_);
        int rc = LTM_OK;
        for (size_t i = 0; i < n && rc == LTM_OK; ++i) rc = ltm_cloud_upload(ctx_, sources[i]->data(), sources[i]->size(), sizeof(PointType), &h[i]);
        if (rc == LTM_OK && method_ != PointToPoint && !have_normals_) {
            rc = ltm_search_estimate_normals(ctx_, 1, &index_, method_ == Generalized ? gicp_k_ : normal_k_, viewpoint_);
            have_normals_ = rc == LTM_OK;
        }
        std::vector<ltm_search*> s(method_ == Generalized ? n : 0, nullptr);
        if (method_ == Generalized) {
            // the sources' own indices and normals (one launch for all of them), then the batch over (target index, source index) pairs
            for (size_t i = 0; i < n && rc == LTM_OK; ++i) rc = ltm_search_build(ctx_, h[i], &s[i]);
            std::vector<float> vp;
            for (size_t i = 0; i < n; ++i) vp.insert(vp.end(), viewpoint_, viewpoint_ + 3);
            if (rc == LTM_OK) rc = ltm_search_estimate_normals(ctx_, n, s.data(), gicp_k_, vp.data());
            if (rc == LTM_OK)
                rc = ltm_icp_align_gicp(ctx_, n, t.data(), s.data(), one_guess ? one_guess->data() : guesses, &params_, gicp_epsilon_, out.data(), nullptr);
        } else if (rc == LTM_OK) {
            rc = (method_ == PointToPlane ? ltm_icp_align_plane : ltm_icp_align)(ctx_, n, t.data(), h.data(), one_guess ? one_guess->data() : guesses, &params_,
                                                                                 out.data(), nullptr);
        }
        std::string msg = rc != LTM_OK ? ltm_last_error(ctx_) : "";
        for (ltm_search* x : s) if (x) ltm_search_free(ctx_, x);
        for (ltm_cloud c : h) if (c) ltm_cloud_free(ctx_, c);
        if (rc != LTM_OK) throw std::runtime_error("DeviceICP: " + msg);
        return out;
    }
    int build(ltm_cloud h)
    {
        reset_target();
        return ltm_search_build(ctx_, h, &index_);
    }
    void reset_target()
    {
        if (index_) ltm_search_free(ctx_, index_);
        index_ = nullptr;
        have_normals_ = false;
    }
    void reset_result()
    {
        result_ = ltm_icp_result{};
        result_.T[0] = result_.T[5] = result_.T[10] = result_.T[15] = 1.0;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceICP: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_icp_params params_;
    Cloud source_;
    ltm_search* index_ = nullptr;
    ltm_icp_result result_;
    Method method_ = PointToPoint;
    int normal_k_ = 10;
    int gicp_k_ = 20;                // k_correspondences_
    double gicp_epsilon_ = 0.001;    // gicp_epsilon_
    double rotation_epsilon_ = 2e-3; // rotation_epsilon_: PCL's default, not used here
    float viewpoint_[3] = {0.0f, 0.0f, 0.0f};
    bool have_normals_ = false;      // of index_, with the current k and viewpoint
};

} // namespace ltremovert
