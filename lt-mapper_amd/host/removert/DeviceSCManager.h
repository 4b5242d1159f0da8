// DeviceSCManager.h -- stands in for the reference's SCManager (ltslam/include/ltslam/Scancontext.h:58-121, ltslam/src/Scancontext.cpp:69-324) over the
// scan-context section of the C ABI (include/ltm.h, "scan context").  Header-only: the host sources the build lists stay as they are.  It keeps
// SCManager's user-side names; a descriptor is a std::vector<double> of num_ring x num_sector entries, row-major [ring][sector], where the reference has an
// Eigen::MatrixXd.  Descriptors are saved on the host side first and reach the device in one batch the first time a query needs them (the reference
// builds its ring-key tree at the same moment, Scancontext.cpp:270-280).  Semantics are those of include/ltm.h.  The swap for the member of LTslam is
// shown in INTEGRATION.md.
// Every member reports a failure by throwing (std::runtime_error with the context's message, std::invalid_argument for a descriptor of the wrong size).
// Cost model: the host-side list is the database of record, as in the reference.  Every save drops the device copy, and the next query uploads the whole
// list again (9.6 KB per descriptor); the scan-set path builds descriptors on the device, downloads them into the list and uploads them again with the
// rest.  That suits the inter-session use (save a whole session, then query a whole session: one upload).  A loop that alternates single saves and
// queries transfers O(N^2) bytes over N keyframes; batch the saves, or use ltm_sc_* directly and keep the handles.
#pragma once
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ltm.h"
#include "removert/utility.h"

namespace ltremovert
{

class DeviceSCManager
{
public:
    using Descriptor = std::vector<double>;
    struct Loop { int loop_id; int nn_idx; double min_dist; int nn_align; float yaw_diff_rad; };

    explicit DeviceSCManager(ltm_ctx* ctx) : ctx_(ctx) { ltm_sc_default_params(&params_); }
    DeviceSCManager(ltm_ctx* ctx, const ltm_sc_params& params) : ctx_(ctx), params_(params) {}
    ~DeviceSCManager() { reset(); }
    DeviceSCManager(const DeviceSCManager&) = delete;
    DeviceSCManager& operator=(const DeviceSCManager&) = delete;

    const ltm_sc_params& params() const { return params_; }
    size_t size() const { return polarcontexts_.size(); }
    const Descriptor& getConstRefRecentSCD() const { return polarcontexts_.back(); }
    const std::vector<Descriptor>& polarcontexts() const { return polarcontexts_; }

    // SCManager::makeAndSaveScancontextAndKeys: descriptor of one scan, made on the device, appended to the database
    void makeAndSaveScancontextAndKeys(const Cloud& scan_down)
    {
        const uint64_t offsets[2] = {0, (uint64_t)scan_down.size()};
        ltm_scanset scans = 0;
        check(ltm_scanset_upload(ctx_, scan_down.data(), sizeof(PointType), offsets, 1, &scans));
        const int rc = append_from_scanset(scans);
        ltm_scanset_free(ctx_, scans);
        check(rc);
    }
    // the same for every keyframe of a scan set that is on the device already (a Session's scans): one launch sequence for all of them
    void makeAndSaveScancontextAndKeys(ltm_scanset scans) { check(append_from_scanset(scans)); }

    // SCManager::saveScancontextAndKeys: a descriptor made elsewhere (the SCD files LTslam reads)
    void saveScancontextAndKeys(const Descriptor& scd)
    {
        if (scd.size() != cells()) throw std::invalid_argument("DeviceSCManager::saveScancontextAndKeys: descriptor size is not num_ring x num_sector");
        polarcontexts_.push_back(scd);
        reset();
    }

    // SCManager::detectLoopClosureIDBetweenSession: {loop id or -1, yaw difference [rad]} of one query descriptor against the saved ones
    std::pair<int, float> detectLoopClosureIDBetweenSession(const Descriptor& curr_desc)
    {
        const std::vector<Loop> r = detectAll(std::vector<Descriptor>{curr_desc});
        return {r[0].loop_id, r[0].yaw_diff_rad};
    }
    // the whole query session in one call (the loop of LTslam::detectInterSessionSCloops, LTslam.cpp:304-333)
    std::vector<Loop> detectAll(const std::vector<Descriptor>& queries)
    {
        std::vector<Loop> out(queries.size());
        if (queries.empty()) return out;
        sync_database();
        ltm_sc* q = upload(queries);
        const size_t n = queries.size();
        std::vector<int32_t> loop(n), idx(n), align(n);
        std::vector<double> dist(n);
        std::vector<float> yaw(n);
        const int rc = ltm_sc_detect(ctx_, database_, q, &params_, loop.data(), idx.data(), dist.data(), align.data(), yaw.data());
        ltm_sc_free(ctx_, q);
        check(rc);
        for (size_t i = 0; i < n; ++i) out[i] = Loop{loop[i], idx[i], dist[i], align[i], yaw[i]};
        return out;
    }

    // SCManager::distanceBtnScanContext: {distance, column shift of sc2 that gives it}
    std::pair<double, int> distanceBtnScanContext(const Descriptor& sc1, const Descriptor& sc2)
    {
        ltm_sc* both = upload(std::vector<Descriptor>{sc1, sc2});
        const int32_t pair[2] = {0, 1};
        double dist = 0.0;
        int32_t shift = 0;
        const int rc = ltm_sc_distance(ctx_, both, both, pair, 1, &params_, &dist, &shift);
        ltm_sc_free(ctx_, both);
        check(rc);
        return {dist, (int)shift};
    }

    ltm_sc* handle()      // the database on the device (valid until the next save)
    {
        sync_database();
        return database_;
    }

private:
    // descriptors of every keyframe of `scans`, appended to the host-side list; an ltm error code (the message stays in the context)
    int append_from_scanset(ltm_scanset scans)
    {
        size_t n_kf = 0;
        ltm_sc* sc = nullptr;
        int rc = ltm_scanset_info(ctx_, scans, &n_kf, nullptr);
        if (rc == LTM_OK) rc = ltm_sc_from_scanset(ctx_, scans, 0, n_kf, &params_, &sc);
        if (rc != LTM_OK) return rc;
        std::vector<double> all(n_kf * cells());
        rc = ltm_sc_download(ctx_, sc, all.data(), nullptr, nullptr);
        ltm_sc_free(ctx_, sc);
        if (rc != LTM_OK) return rc;
        for (size_t k = 0; k < n_kf; ++k) polarcontexts_.emplace_back(all.begin() + (long)(k * cells()), all.begin() + (long)((k + 1) * cells()));
        reset();
        return LTM_OK;
    }
    size_t cells() const { return (size_t)params_.num_ring * (size_t)params_.num_sector; }
    ltm_sc* upload(const std::vector<Descriptor>& descs)
    {
        std::vector<double> flat;
        flat.reserve(descs.size() * cells());
        for (const Descriptor& d : descs) {
            if (d.size() != cells()) throw std::invalid_argument("DeviceSCManager: descriptor size is not num_ring x num_sector");
            flat.insert(flat.end(), d.begin(), d.end());
        }
        ltm_sc* h = nullptr;
        check(ltm_sc_from_descriptors(ctx_, flat.data(), descs.size(), &params_, &h));
        return h;
    }
    void sync_database()
    {
        if (!database_) database_ = upload(polarcontexts_);
    }
    void reset()
    {
        if (database_) ltm_sc_free(ctx_, database_);
        database_ = nullptr;
    }
    void check(int rc) const
    {
        if (rc != LTM_OK) throw std::runtime_error(std::string("DeviceSCManager: ") + ltm_last_error(ctx_));
    }

    ltm_ctx* ctx_;
    ltm_sc_params params_;
    std::vector<Descriptor> polarcontexts_;
    ltm_sc* database_ = nullptr;
};

} // namespace ltremovert
