// ltm_api_submap.cpp -- C ABI: the loop submaps, the counterpart of Session::loopFindNearKeyframesLocalCoord / CentralCoord (ltslam/src/Session.cpp:91-142)
// with transformPointCloud and pcl::getTransformation (ltslam/src/utility.cpp:80-103) for all the windows of a batch at once.  Kernel in ltm_k_submap.hip;
// the grid is ltm_voxel_grid_scanset's (ltm_api_voxel.cpp) with the order as an argument; the arithmetic is stated in include/ltm.h, "loop submaps".
#include "ltm_internal.h"

extern "C" {

int ltm_pose6d_to_affine3f(const float* xyzrpy, size_t n, float* affine12)
{
    if (!xyzrpy || !affine12) return LTM_E_INVALID;
    for (size_t i = 0; i < n; ++i) {
        const float* p = xyzrpy + 6 * i;
        float* t = affine12 + 12 * i;
        // pcl::getTransformation (PCL 1.10 common/impl/eigen.hpp), every product and sum rounded to float on its own (the unit is compiled with
        // -ffp-contract=off)
        const float A = cosf(p[5]), B = sinf(p[5]), C = cosf(p[4]), D = sinf(p[4]), E = cosf(p[3]), F = sinf(p[3]);
        const float DE = D * E, DF = D * F;
        const float ADF = A * DF, BE = B * E, BF = B * F, ADE = A * DE, AE = A * E, BDF = B * DF, BDE = B * DE, AF = A * F;
        t[0] = A * C; t[1] = ADF - BE; t[2] = BF + ADE; t[3] = p[0];
        t[4] = B * C; t[5] = AE + BDF; t[6] = BDE - AF; t[7] = p[1];
        t[8] = -D;    t[9] = C * F;    t[10] = C * E;   t[11] = p[2];
    }
    return LTM_OK;
}

int ltm_submaps_assemble(ltm_ctx* c, ltm_scanset hscans, const float* affine12, const int32_t* keys, size_t n_windows, int search_num, float leaf, int order,
                         ltm_scanset* out)
{
    return guarded(c, [&] {
        LTM_REQUIRE(out && (keys || !n_windows), "null argument");
        LTM_REQUIRE(search_num >= 0, "search_num must be >= 0");
        LTM_REQUIRE(std::isfinite(leaf) && leaf >= 0.0f, "leaf must be finite and >= 0 (0: no grid)");
        LTM_REQUIRE(order == 0 || order == 1, "order must be 0 (input) or 1 (PCL)");
        const ScanSet& s = get_ss(c, hscans);
        const int64_t nkf = (int64_t)s.nkf();
        // window w = keyframes keys[w] - search_num ... keys[w] + search_num inside [0, n_kf), ascending (Session.cpp:98-104).  Sizes first (the scan set's
        // host offsets give them), so that a batch beyond the grid's 32-bit point indices is refused before anything is built
        auto window = [&](size_t w, int64_t* lo, int64_t* hi) {
            *lo = std::max<int64_t>((int64_t)keys[w] - search_num, 0);
            *hi = std::min<int64_t>((int64_t)keys[w] + search_num, nkf - 1);
        };
        std::vector<uint64_t> off(n_windows + 1, 0);
        size_t n_pieces = 0;
        for (size_t w = 0; w < n_windows; ++w) {
            int64_t lo, hi;
            window(w, &lo, &hi);
            off[w + 1] = off[w] + (hi >= lo ? s.off[(size_t)hi + 1] - s.off[(size_t)lo] : 0);
            n_pieces += hi >= lo ? (size_t)(hi - lo + 1) : 0;
            if (off[w + 1] >= 0xffffffffull) throw Err{LTM_E_UNSUPPORTED, "the windows of one batch must hold fewer than 2^32 - 1 points before the grid: split the batch"};
        }
        // the pieces (window, source keyframe, affine) and the table that names the piece of every workgroup
        std::vector<SubmapPiece> pieces;
        BlockTable table;
        pieces.reserve(n_pieces);
        for (size_t w = 0; w < n_windows; ++w) {
            int64_t lo, hi;
            window(w, &lo, &hi);
            uint64_t at = off[w];
            for (int64_t k = lo; k <= hi; ++k) {
                const uint64_t n = s.off[(size_t)k + 1] - s.off[(size_t)k];
                if (!n) continue;
                SubmapPiece P;
                P.src = s.off[(size_t)k]; P.dst = at; P.n = (uint32_t)n;
                P.affine = affine12 ? (uint32_t)k : 0u;
                // (unreachable in practice at the table's default limit: with fewer than 2^32 - 1 points in all, checked above, it would take 2^31 - 2^24 pieces)
                if (!table.add((uint32_t)pieces.size(), n, 256, &P.span)) throw Err{LTM_E_UNSUPPORTED, "too many points in one batch of submaps"};
                pieces.push_back(P);
                at += n;
            }
        }
        const uint64_t total = off[n_windows];
        // the transformed concatenation, as a scan set of its own: the result (leaf == 0) or the input of the grid
        PoolBlocks own(c);
        float4* d = own.alloc<float4>(std::max<uint64_t>(total, 1));
        if (total) {
            static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            const size_t na = affine12 ? (size_t)nkf : 1;
            DevBuf d_aff(c, na * 12 * sizeof(float));
            h2d(c, d_aff.p, affine12 ? affine12 : kIdentity, na * 12 * sizeof(float));
            DevBuf d_pieces = to_device(c, pieces), d_bp = to_device(c, table.owner());
            ProfScope ps(c, "submap_assemble", (double)total, 32.0 * (double)total);
            LTM_HIP(submap_gather(s.d, d_pieces.as<SubmapPiece>(), d_bp.as<uint32_t>(), table.size(), d_aff.as<float>(), d, c->stream));
        }
        const ltm_scanset cat = new_scanset(c, d, std::move(off));
        own.release(d);      // the scan set owns the block now
        if (leaf == 0.0f) { *out = cat; return; }
        const int rc = voxel_grid_scanset_ordered(c, cat, leaf, order, out);
        const std::string msg = c->err;
        (void)ltm_scanset_free(c, cat);
        if (rc != LTM_OK) throw Err{rc, msg};
    });
}

} // extern "C"
