// DeviceLoopSubmaps.h -- stands in for the submap members of the reference's Session (ltslam/src/Session.cpp:91-142: loopFindNearKeyframesLocalCoord /
// loopFindNearKeyframesCentralCoord) and its transformPointCloud (ltslam/src/utility.cpp:80-103) over the "loop submaps" section of the C ABI
// (include/ltm.h).  Header-only: the host sources the build lists stay as they are.  It keeps the reference's names; a pose is a Pose6D (the x y z roll
// pitch yaw of the reference's PointTypePose), an affine 12 floats (rows 0..2 of the Eigen::Affine3f, row-major).  Semantics are those of include/ltm.h.
// The keyframe scans live on the device (a scan set); the batched forms return device handles -- a scan set with one submap per key and one search index
// per submap -- which DeviceICP / ltm_icp_align_scanset take as they are, so addSCloops' loop becomes: loopFindNearKeyframes* for all keys, buildTargets,
// one ICP batch.  Every member reports a failure by throwing (std::runtime_error with the context's message).
// Not here: the Euler / gtsam::Pose3 conversions of the ICP result stay on the host as they are.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

struct Pose6D { float x, y, z, roll, pitch, yaw; };
using Affine3f = std::array<float, 12>;

// pcl::getTransformation(x, y, z, roll, pitch, yaw) in float (needs no device)
inline Affine3f getTransformation(const Pose6D& p)
{
    const float in[6] = {p.x, p.y, p.z, p.roll, p.pitch, p.yaw};
    Affine3f t{};
    if (ltm_pose6d_to_affine3f(in, 1, t.data()) != LTM_OK) throw std::runtime_error("getTransformation: ltm_pose6d_to_affine3f failed");
    return t;
}

// transformPointCloud(cloudIn, transformIn) (utility.cpp:80-103) for a cloud on the host: the same float arithmetic, left to right (bit-identical to the
// device's when the including unit is compiled without fused multiply-adds: the x86-64 baseline, or -ffp-contract=off)
inline Cloud transformPointCloud(const Cloud& cloudIn, const Pose6D& transformIn)
{
    const Affine3f t = getTransformation(transformIn);
    Cloud out(cloudIn.size());
    for (size_t i = 0; i < cloudIn.size(); ++i) {
        const PointType& p = cloudIn[i];
        const float x = ((t[0] * p.x + t[1] * p.y) + t[2] * p.z) + t[3];
        const float y = ((t[4] * p.x + t[5] * p.y) + t[6] * p.z) + t[7];
        const float z = ((t[8] * p.x + t[9] * p.y) + t[10] * p.z) + t[11];
        out[i] = PointType{x, y, z, p.intensity};
    }
    return out;
}

class DeviceLoopSubmaps
{
public:
    // scans: the session's cloudKeyFrames as a scan set of `ctx` (stays the caller's); poses: cloudKeyPoses6D, one per keyframe
    DeviceLoopSubmaps(ltm_ctx* ctx, ltm_scanset scans, const std::vector<Pose6D>& poses, float leaf = 0.3f, int pcl_order = 1)
        : ctx_(ctx), scans_(scans), leaf_(leaf), order_(pcl_order)
    {
        affines_.resize(poses.size() * 12);
        for (size_t i = 0; i < poses.size(); ++i) {
            const Affine3f t = getTransformation(poses[i]);
            for (int k = 0; k < 12; ++k) affines_[12 * i + (size_t)k] = t[(size_t)k];
        }
    }

    // Session::loopFindNearKeyframesLocalCoord for every key at once: submap w of the result = keyframes keys[w] +- searchNum in the keyframes' own
    // frame (the reference multiplies by the origin pose, the identity), gridded at the leaf size.  The caller frees the scan set.
    ltm_scanset loopFindNearKeyframesLocalCoord(const std::vector<int32_t>& keys, int searchNum) const { return assemble(nullptr, keys, searchNum); }
    // Session::loopFindNearKeyframesCentralCoord: the same with every keyframe moved by its pose
    ltm_scanset loopFindNearKeyframesCentralCoord(const std::vector<int32_t>& keys, int searchNum) const
    {
        return assemble(affines_.data(), keys, searchNum);
    }
    // kdtree->setInputCloud for every submap at once; the caller frees each index with ltm_search_free
    std::vector<ltm_search*> buildTargets(ltm_scanset submaps) const
    {
        size_t n = 0;
        check(ltm_scanset_info(ctx_, submaps, &n, nullptr));
        std::vector<ltm_search*> out(n, nullptr);
        if (n) check(ltm_search_build_scanset(ctx_, submaps, 0, n, out.data()));
        return out;
    }
    // one submap on the host (what the reference's nearKeyframes holds afterwards)
    Cloud download(ltm_scanset submaps, size_t which) const
    {
        ltm_cloud h = 0;
        check(ltm_scanset_keyframe(ctx_, submaps, which, &h));
        size_t n = 0;
        int rc = ltm_cloud_size(ctx_, h, &n);
        Cloud out(n);
        if (rc == LTM_OK && n) rc = ltm_cloud_download(ctx_, h, out.data(), n, sizeof(PointType));
        const std::string msg = rc != LTM_OK ? ltm_last_error(ctx_) : "";
        ltm_cloud_free(ctx_, h);
        if (rc != LTM_OK) throw std::runtime_error("DeviceLoopSubmaps: " + msg);
        return out;
    }
    const std::vector<float>& affines() const { return affines_; }

private:
    ltm_scanset assemble(const float* affines, const std::vector<int32_t>& keys, int searchNum) const
    {
        ltm_scanset out = 0;
        check(ltm_submaps_assemble(ctx_, scans_, affines, keys.data(), keys.size(), searchNum, leaf_, order_, &out));
        return out;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceLoopSubmaps: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_scanset scans_;
    float leaf_;
    int order_;
    std::vector<float> affines_;
};

} // namespace ltremovert
