// ltm_api_scancontext.cpp -- C ABI: Scan Context descriptors, keys, pair distance and inter-session loop detection, the counterpart of the reference's
// SCManager (ltslam/src/Scancontext.cpp:69-324, driven by LTslam::detectInterSessionSCloops, LTslam.cpp:304-333).  Kernels in ltm_k_scancontext.hip.
#include "ltm_internal.h"

struct ltm_sc {
    PoolBlocks blocks;                // the four arrays: back in the pool with the handle
    size_t n = 0;
    int R = 0, S = 0;
    double* desc = nullptr;           // n x R x S, row-major [ring][sector]
    float* ring_keys = nullptr;       // n x R
    double* sector_keys = nullptr;    // n x S
    double* norms = nullptr;          // n x S column norms (the same at every shift)
    explicit ltm_sc(ltm_ctx* c) : blocks(c) {}
};

namespace {

constexpr int kMaxRing = 64, kMaxSector = 256, kMaxCandidates = 64;

ltm_sc_params params_or_default(const ltm_sc_params* p)
{
    ltm_sc_params d;
    ltm_sc_default_params(&d);
    return p ? *p : d;
}
void check_params(const ltm_sc_params& p)
{
    LTM_REQUIRE(p.num_ring >= 1 && p.num_sector >= 1, "num_ring and num_sector must be >= 1");
    if (p.num_ring > kMaxRing || p.num_sector > kMaxSector) throw Err{LTM_E_UNSUPPORTED, "num_ring > 64 or num_sector > 256"};
    LTM_REQUIRE(std::isfinite(p.lidar_height), "lidar_height is not finite");
    LTM_REQUIRE(std::isfinite(p.max_radius) && p.max_radius > 0.0, "max_radius must be finite and > 0");
    LTM_REQUIRE(p.num_candidates >= 0, "num_candidates must be >= 0 (0: every database entry)");
    LTM_REQUIRE(p.search_ratio >= 0.0, "search_ratio must be >= 0");
    LTM_REQUIRE(!std::isnan(p.dist_thres), "dist_thres is NaN");
}
void check_shape(const ltm_sc* s, const ltm_sc_params& p)
{
    LTM_REQUIRE(s->R == p.num_ring && s->S == p.num_sector, "num_ring / num_sector of the parameters differ from the descriptor set's");
}
// SEARCH_RADIUS of :123, cut at the sector count.  The kernel compares the circular distance to the aligned shift with it, so every value >= S / 2
// means the same: every shift
int shift_radius(const ltm_sc_params& p)
{
    if (p.search_ratio >= 1.0) return p.num_sector;
    return (int)std::min<double>(std::round(0.5 * p.search_ratio * p.num_sector), (double)p.num_sector);
}

// an error leaves nothing behind: the handle dies with `s`, its blocks with it
template <class F>
void sc_build(ltm_ctx* c, size_t n, const ltm_sc_params& p, ltm_sc** out, F&& fill)
{
    std::unique_ptr<ltm_sc> s(new ltm_sc(c));
    const size_t R = p.num_ring, S = p.num_sector;
    s->n = n; s->R = p.num_ring; s->S = p.num_sector;
    s->desc = s->blocks.alloc<double>(n * R * S);
    s->ring_keys = s->blocks.alloc<float>(n * R);
    s->sector_keys = s->blocks.alloc<double>(n * S);
    s->norms = s->blocks.alloc<double>(n * S);
    fill(s.get());
    *out = c->open.sc.adopt(s);
}

} // namespace

extern "C" {

void ltm_sc_default_params(ltm_sc_params* p)
{
    if (!p) return;
    p->lidar_height = 2.0;
    p->num_ring = 20;
    p->num_sector = 60;
    p->max_radius = 80.0;
    p->num_candidates = 3;
    p->search_ratio = 0.1;
    p->dist_thres = 0.3;
}

int ltm_sc_from_scanset(ltm_ctx* c, ltm_scanset hscans, size_t kf_begin, size_t kf_end, const ltm_sc_params* params, ltm_sc** out)
{
    return guarded(c, [&] {
        LTM_REQUIRE(out, "null argument");
        const ltm_sc_params p = params_or_default(params);
        check_params(p);
        const ScanSet& ss = get_ss(c, hscans);
        LTM_REQUIRE(kf_begin <= kf_end && kf_end <= ss.nkf(), "keyframe range outside the scan set");
        const size_t n = kf_end - kf_begin, nbins = (size_t)p.num_ring * p.num_sector;
        uint64_t n_pts = 0, max_kf = 0;
        for (size_t k = kf_begin; k < kf_end; ++k) max_kf = std::max(max_kf, ss.off[k + 1] - ss.off[k]);
        if (n) n_pts = ss.off[kf_end] - ss.off[kf_begin];
        sc_build(c, n, p, out, [&](ltm_sc* s) {
            if (!n) return;
            ProfScope ps(c, "sc_build", (double)n_pts, 16.0 * (double)n_pts + 12.0 * (double)(n * nbins));
            DevBuf bins(c, n * nbins * sizeof(uint32_t));
            LTM_HIP(hipMemsetAsync(bins.p, 0, n * nbins * sizeof(uint32_t), c->stream));
            LTM_HIP(sc_scatter(ss.d, ss.off_dev, kf_begin, n, max_kf, ScGeom{p.lidar_height, p.max_radius, p.num_ring, p.num_sector}, bins.as<uint32_t>(), c->stream));
            LTM_HIP(sc_finish(bins.as<uint32_t>(), n, s->R, s->S, s->desc, s->ring_keys, s->sector_keys, s->norms, c->stream));
        });
    });
}

int ltm_sc_from_descriptors(ltm_ctx* c, const double* desc_host, size_t n, const ltm_sc_params* params, ltm_sc** out)
{
    return guarded(c, [&] {
        LTM_REQUIRE(out && (desc_host || !n), "null argument");
        const ltm_sc_params p = params_or_default(params);
        check_params(p);
        sc_build(c, n, p, out, [&](ltm_sc* s) {
            if (!n) return;
            h2d(c, s->desc, desc_host, n * s->R * s->S * sizeof(double));
            LTM_HIP(sc_finish(nullptr, n, s->R, s->S, s->desc, s->ring_keys, s->sector_keys, s->norms, c->stream));
        });
    });
}

int ltm_sc_info(ltm_ctx* c, ltm_sc* hs, size_t* n, int* num_ring, int* num_sector)
{
    return guarded(c, [&] {
        const ltm_sc* s = c->open.sc.get(hs);
        if (n) *n = s->n;
        if (num_ring) *num_ring = s->R;
        if (num_sector) *num_sector = s->S;
    });
}

int ltm_sc_download(ltm_ctx* c, ltm_sc* hs, double* desc, float* ring_keys, double* sector_keys)
{
    return guarded(c, [&] {
        const ltm_sc* s = c->open.sc.get(hs);
        if (desc) d2h(c, desc, s->desc, s->n * s->R * s->S * sizeof(double));
        if (ring_keys) d2h(c, ring_keys, s->ring_keys, s->n * s->R * sizeof(float));
        if (sector_keys) d2h(c, sector_keys, s->sector_keys, s->n * s->S * sizeof(double));
    });
}

int ltm_sc_distance(ltm_ctx* c, ltm_sc* ha, ltm_sc* hb, const int32_t* pairs_host, size_t n_pairs, const ltm_sc_params* params, double* dist_host,
                    int32_t* shift_host)
{
    return guarded(c, [&] {
        const ltm_sc* a = c->open.sc.get(ha);
        const ltm_sc* b = c->open.sc.get(hb);
        LTM_REQUIRE(a->R == b->R && a->S == b->S, "the two descriptor sets differ in num_ring / num_sector");
        const ltm_sc_params p = params_or_default(params);
        check_params(p);
        check_shape(a, p);
        if (!n_pairs) return;
        LTM_REQUIRE(pairs_host, "null argument");
        LTM_REQUIRE(n_pairs < 0x80000000ull, "too many pairs");
        for (size_t k = 0; k < n_pairs; ++k)
            LTM_REQUIRE(pairs_host[2 * k] >= 0 && (size_t)pairs_host[2 * k] < a->n && pairs_host[2 * k + 1] >= 0 && (size_t)pairs_host[2 * k + 1] < b->n,
                        "pair index outside its descriptor set");
        ProfScope ps(c, "sc_distance", (double)n_pairs, (double)n_pairs * 16.0 * a->R * a->S);
        DevBuf pairs(c, n_pairs * 8), dist(c, n_pairs * 8), shift(c, n_pairs * 4);
        h2d(c, pairs.p, pairs_host, n_pairs * 8);
        LTM_HIP(sc_pair_distance(a->desc, a->sector_keys, a->norms, b->desc, b->sector_keys, b->norms, a->R, a->S, pairs.as<int32_t>(), b->n, n_pairs,
                                 shift_radius(p), dist.as<double>(), shift.as<int32_t>(), c->stream));
        if (dist_host) d2h(c, dist_host, dist.p, n_pairs * 8);
        if (shift_host) d2h(c, shift_host, shift.p, n_pairs * 4);
    });
}

int ltm_sc_detect(ltm_ctx* c, ltm_sc* hdb, ltm_sc* hq, const ltm_sc_params* params, int32_t* loop_id, int32_t* nn_idx, double* min_dist, int32_t* nn_align,
                  float* yaw_diff_rad)
{
    return guarded(c, [&] {
        const ltm_sc* db = c->open.sc.get(hdb);
        const ltm_sc* q = c->open.sc.get(hq);
        LTM_REQUIRE(db->R == q->R && db->S == q->S, "the two descriptor sets differ in num_ring / num_sector");
        const ltm_sc_params p = params_or_default(params);
        check_params(p);
        check_shape(db, p);
        const size_t nq = q->n, nd = db->n;
        if (!nq) return;
        std::vector<int32_t> idx(nq, 0), align(nq, 0);
        std::vector<double> dist(nq, 10000000.0);      // an empty database: no candidate, the initial values of :282-284 stay
        if (nd) {
            const bool exhaustive = p.num_candidates == 0 || (size_t)p.num_candidates >= nd;
            if (!exhaustive && p.num_candidates > kMaxCandidates) throw Err{LTM_E_UNSUPPORTED, "num_candidates > 64 (and below the database size)"};
            const size_t K = exhaustive ? nd : (size_t)p.num_candidates;
            // the ring-key distance matrix is nq x nd in either mode (K <= nd): one bound for it and for the pair list
            if (nd >= 0x80000000ull || nq >= 0x80000000ull || nq * nd >= 0x80000000ull)
                throw Err{LTM_E_UNSUPPORTED, "n_query x n_database >= 2^31 in one call: split the queries"};
            ProfScope ps(c, "sc_detect", (double)(nq * K), (double)(nq * K) * 16.0 * q->R * q->S);
            DevBuf rd(c, nq * nd * 4), pairs(c, exhaustive ? 8 : nq * K * 8), pd(c, nq * K * 8), psh(c, nq * K * 4);
            DevBuf o_idx(c, nq * 4), o_dist(c, nq * 8), o_align(c, nq * 4);
            const int32_t* pairs_dev = exhaustive ? nullptr : pairs.as<int32_t>();
            LTM_HIP(sc_ring_distances(q->ring_keys, nq, db->ring_keys, nd, q->R, rd.as<float>(), c->stream));
            if (!exhaustive) LTM_HIP(sc_candidates(rd.as<float>(), nq, nd, (int)K, pairs.as<int32_t>(), c->stream));
            LTM_HIP(sc_pair_distance(q->desc, q->sector_keys, q->norms, db->desc, db->sector_keys, db->norms, q->R, q->S, pairs_dev, nd, nq * K, shift_radius(p),
                                     pd.as<double>(), psh.as<int32_t>(), c->stream));
            LTM_HIP(sc_detect_reduce(pd.as<double>(), psh.as<int32_t>(), pairs_dev, rd.as<float>(), nq, nd, K, o_idx.as<int32_t>(), o_dist.as<double>(),
                                     o_align.as<int32_t>(), c->stream));
            d2h(c, idx.data(), o_idx.p, nq * 4);
            d2h(c, dist.data(), o_dist.p, nq * 8);
            d2h(c, align.data(), o_align.p, nq * 4);
        }
        const double unit = 360.0 / (double)q->S;      // PC_UNIT_SECTORANGLE
        for (size_t i = 0; i < nq; ++i) {
            if (loop_id) loop_id[i] = dist[i] < p.dist_thres ? idx[i] : -1;
            if (nn_idx) nn_idx[i] = idx[i];
            if (min_dist) min_dist[i] = dist[i];
            if (nn_align) nn_align[i] = align[i];
            if (yaw_diff_rad) {
                const float degrees = (float)((double)align[i] * unit);      // deg2rad takes a float (:17-20, :319)
                yaw_diff_rad[i] = (float)((double)degrees * M_PI / 180.0);
            }
        }
    });
}

int ltm_debug_sc_paths(int num_ring, int num_sector, int* scatter_in_lds, int* pair_in_lds)
{
    if (num_ring < 1 || num_ring > kMaxRing || num_sector < 1 || num_sector > kMaxSector) return LTM_E_INVALID;
    bool scatter = false, pair = false;
    sc_paths(num_ring, num_sector, &scatter, &pair);
    if (scatter_in_lds) *scatter_in_lds = scatter ? 1 : 0;
    if (pair_in_lds) *pair_in_lds = pair ? 1 : 0;
    return LTM_OK;
}

int ltm_sc_free(ltm_ctx* c, ltm_sc* s)
{
    return guarded(c, [&] { c->open.sc.free(s); });
}

} // extern "C"
